"""The CPU oracle's Categorical sites over the whole logits range (cat_range_ref.py: flat, wide, peaked, holed and shifted
rows at 1 .. 4096 classes) against an integer replay of the inverse-CDF rule and against float64, per draw.  Bit parity of the
HIP library with this oracle (test_gpu_cat_range.py) cannot see a mistake the two share: before the exact threshold product,
cat_invcdf's bits * Q wrapped at 64 bits once a row held 512 classes' worth of weight, and the flat rows of 513, 1000 and 4096
classes failed here, in layer 1 and in layer 2, while every parity test passed."""

import numpy as np
import pytest
import torch

import cat_range_ref as R

_np = R._np


def test_delta_g_is_the_measured_one(oracle_ops):
    d, k = R.measure_delta_g(R.make_log32(oracle_ops))
    print(f"delta_g = {d!r} at k = {k}")
    assert d == R.DELTA_G


def test_seed_exceptions_are_frequency_cases():
    """A case may sit on another seed only where its check is the frequency bound (Gumbel-max above 64 classes)."""
    for (route, K, impl, name), seed in R.FREQ_SEEDS.items():
        assert K > 64 and seed > 0 and impl in (0, 1)
        assert name == "" or name in R.FAMILIES or "+" in name or (route == "scan" and name in ("left_to_right", "peaked"))
        assert R.seed_of(route, K, 1, impl, name) == 0


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", R.KS)
def test_generic_sampler_shared_rows(oracle_ops, K, mode, impl):
    """sample_logpdf_categorical with one shared row, every family: layers 1 and 2 (mode 1), the float64 argmax per draw or the
    class frequencies (mode 0), scores against float64, logpdf_categorical == score."""
    stats = {}
    R.shared_rows_case(oracle_ops, oracle_ops, K, mode, impl, stats)
    print(f"K={K} mode {mode} impl {impl}: {stats}")


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", R.KS)
def test_generic_sampler_row_table(oracle_ops, K, mode, impl):
    stats = {}
    R.row_table_case(oracle_ops, oracle_ops, K, mode, impl, stats)
    print(f"K={K} mode {mode} impl {impl}: {stats}")


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [k for k in R.KS if k <= 64])
def test_generic_sampler_per_particle_rows(oracle_ops, K, mode, impl):
    stats = {}
    R.per_particle_case(oracle_ops, oracle_ops, K, mode, impl, stats)
    print(f"K={K} mode {mode} impl {impl}: {stats}")


@pytest.mark.parametrize("impl", [0, 1])
def test_threshold_zero_skips_classes_of_weight_zero(oracle_ops, impl):
    """Words below 512 on rows whose only mass is behind classes at -inf: thr = 0 = C_c for every leading hole, and the draw
    must be the first class WITH mass (strictly above the threshold).  The words are searched among 2^26 particles; on them
    the replay with `C_c >= thr` (the mutation) names a class at -inf and fails."""
    ops = oracle_ops
    ek, fold, words = R.edge_word_keys(ops, impl)
    n = words.size
    for row in R.EDGE_ROWS:
        row = R.f32(row)
        v, s = R.generic_case(ops, ops, ek.with_fold(fold), n, row[None, :], 1, what=f"edge words {row.tolist()}")
        assert (_np(v) == int(np.argmax(row))).all()
        with pytest.raises(AssertionError):
            R.check_draws(ops, row, _np(v), None, ops, ek.with_fold(fold), 1, mutation="ge")
        R.edge_plan_case(ops, ops, ek, fold, impl, row)
    print(f"impl {impl}: {n} edge words {words.tolist()}")


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["one", "flip"])
@pytest.mark.parametrize("K", [2, 17, 511, 512, 513, 1000])
def test_plan_route(oracle_ops, K, kind, mode, impl):
    """plan_create / importance_run with one latent Categorical site, or with a flip that selects one of two rows."""
    stats = {}
    R.plan_case(oracle_ops, oracle_ops, K, mode, impl, kind, 16384, stats)
    print(f"plan {kind} K={K} mode {mode} impl {impl}: {stats}")


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", R.PLAN_KS)
def test_plan_route_rows_from_an_input_column(oracle_ops, K, mode, impl):
    """The plans of the GPU suite's generated-kernel test, at its sizes and seeds: the oracle stays inside every bound here
    before the HIP kernels are held to it."""
    stats = {}
    for n in R.PLAN_NS:
        R.plan_case(oracle_ops, oracle_ops, K, mode, impl, "input", n, stats)
    print(f"plan input K={K} mode {mode} impl {impl}: {stats}")


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("kind", ["left_to_right", "peaked"])
@pytest.mark.parametrize("K", R.SCAN_KS)
def test_scan_plan_in_the_hmm_shape(oracle_ops, K, kind, impl):
    """The scans of the GPU suite on the oracle (whose plain walk the guide tables of the device must reproduce)."""
    print(f"K={K} {kind} impl {impl}: {R.scan_case(oracle_ops, oracle_ops, impl, K, kind)}")


@pytest.mark.parametrize("K", [1, 2, 3, 17, 255, 256])
def test_hmm_prepare_alias_tables(oracle_ops, K):
    """(K = 256, peak 17: p^ - p = 1.06e-5, the 255 classes at -17 all round to weight 0 — inside the derived bound.)"""
    st = R.alias_case(oracle_ops, oracle_ops, K, {})
    print(f"K={K}: {st}")


def test_alias_mutation_is_caught(oracle_ops):
    """One threshold moved by 2^-16 fails the first bound."""
    K = 17
    t = R.alias_tables(K)["families"]
    L = torch.from_numpy(t)
    tab = _np(oracle_ops.hmm_prepare(K, 0, L, L)[0]).reshape(K, K)
    r, j = next((r, j) for r in range(K) for j in range(K) if (tab[r, j] & 255) != j)
    R.alias_check(tab, t, R.make_exp32(oracle_ops))
    with pytest.raises(AssertionError):
        R.alias_check(tab, t, R.make_exp32(oracle_ops), shift=(r, j))


@pytest.mark.parametrize("K", [513, 1000, 4096])
def test_wrapping_product_is_caught(oracle_ops, K):
    """The replay with a product that wraps at 64 bits (the oracle's former line) fails on the flat rows from 513 classes."""
    ops, n = oracle_ops, R.n_for(K)
    row = np.zeros(K, dtype=np.float32)
    kb = R.key_batch(1, 3).with_fold(2)
    v, _ = ops.sample_logpdf_categorical(kb, n, torch.from_numpy(row[None, :].copy()), None, 1)
    R.check_draws(ops, row, _np(v), None, ops, kb, 1)
    with pytest.raises(AssertionError):
        R.check_draws(ops, row, _np(v), None, ops, kb, 1, mutation="wrap64")


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("N", [1, 2, 65, 1000])
def test_categorical_index_frequencies(oracle_ops, N, impl):
    """gjx_categorical_index (Gumbel-max over one row under a scalar key), 20 000 keys, by the frequency bound."""
    ops = oracle_ops
    row = R.index_row(N)
    L = torch.from_numpy(row)
    seed = R.seed_of("index", N, 0, impl)
    v = np.array([int(ops.categorical_index(R.key_batch(impl, b, seed), L, 0)) for b in range(R.INDEX_B)])
    R.never_draws_impossible(row, v)
    print(f"N={N} impl {impl}: worst {R.frequency_check(R.softmax64(row), v):.3f} of the allowance")


def test_hmm_filter_rms_is_the_measured_one(oracle_ops):
    """The bootstrap HMM filter on the left-to-right table (the GPU suite's case): the RMS error of log Z over 32 oracle
    filters is the recorded one, and the oracle's history holds no forbidden transition."""
    import genjax
    from genjax._amd.runtime import use_ops

    rms, errs = R.hmm_filter_rms(oracle_ops)
    print(f"RMS {rms!r}, largest {max(abs(e) for e in errs):.4f}")
    assert rms == pytest.approx(R.HMM_LOGZ_RMS, rel=1e-9)
    with use_ops(oracle_ops):
        r = R.hmm_filter_run(oracle_ops, genjax.random.key(R.HMM_FILTER["seed"], 1))
    R.hmm_filter_history_check(_np(r.history), _np(r.ancestors))
    assert abs(r.log_marginal_likelihood - R.hmm_filter_exact()) <= 5.0 * R.HMM_LOGZ_RMS


def host_api_uniform_prior(impl, n=65536, K=1000):
    """A one-site `@gen` model with a uniform prior over K labels drawn by inverse CDF: the fused route and the per-site
    route, -> (fused draws, per-site draws) as numpy."""
    import genjax
    from genjax import ChoiceMap, gen
    from genjax._amd.lang import Categorical, GenerateHandler, StaticTrace
    from genjax._amd.plan import try_fused_generate

    cat = Categorical()
    cat.sampling = "inverse_cdf"
    logits = [0.0] * K

    @gen
    def model():
        return cat(logits=logits) @ "label"

    keys = genjax.random.split(genjax.random.key(5, impl), n)
    fused = try_fused_generate(model, keys, ChoiceMap.empty(), ())
    assert fused is not None, "the model must lower to a fused plan"
    ftr, _ = fused
    h = GenerateHandler(keys, ChoiceMap.empty())
    retval = h.run(model.source, ())
    eager = StaticTrace(model, (), retval, h.traces)
    (_, fcol), = dict(ftr.get_choices().leaves()).items()
    (_, ecol), = dict(eager.get_choices().leaves()).items()
    return torch.as_tensor(fcol).cpu().numpy(), torch.as_tensor(ecol).cpu().numpy()


@pytest.mark.parametrize("impl", [0, 1])
def test_host_api_uniform_prior_over_1000_labels(oracle_ops, impl):
    """Before the exact product about half of these draws fell outside their class."""
    from genjax._amd.runtime import use_ops

    with use_ops(oracle_ops):
        f, e = host_api_uniform_prior(impl)
    assert np.array_equal(f, e), "the fused route and the per-site route differ"
    print(f"impl {impl}: worst {R.frequency_check(np.full(1000, 1e-3), f):.3f} of the allowance")
