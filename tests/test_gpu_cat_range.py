"""The HIP library's Categorical sites over the whole logits range of cat_range_ref.py: every check test_cat_range_cpu.py
holds the oracle to (the integer replay of the inverse-CDF rule, float64 per draw, scores, alias tables), HIP == oracle bit for
bit on every case, and the routes only the device has — the guide tables of the generated kernels (k_cat_prepare builds them,
jcat_invcdf_gb reads them; up to 511 classes), the on-the-fly jcat_invcdf above, in every kernel form; the scan plan in the
shape of the HMM workload; the bootstrap HMM filter on a left-to-right table; the batched single-index draw."""

import numpy as np
import pytest
import torch

import cat_range_ref as R

pytestmark = pytest.mark.gpu

IMPLS = [0, 1]
_np = R._np


@pytest.fixture(params=["specialized", "pair", "interpreter"])
def plan_mode(request, monkeypatch):
    """The importance kernel forms (test_gpu_parity_abi.plan_mode): the default generated kernel, two particles per lane
    (GJX_JIT_FORM=pair) and the site-table interpreter (GJX_PLAN_JIT=0)."""
    monkeypatch.setenv("GJX_PLAN_JIT", "0" if request.param == "interpreter" else "1")
    if request.param == "pair":
        monkeypatch.setenv("GJX_JIT_FORM", "pair")
    else:
        monkeypatch.delenv("GJX_JIT_FORM", raising=False)
    return request.param


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", R.KS)
def test_generic_sampler_shared_rows(hip_ops, oracle_ops, K, mode, impl):
    stats = {}
    R.shared_rows_case(hip_ops, oracle_ops, K, mode, impl, stats)
    print(f"K={K} mode {mode} impl {impl}: {stats}")


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", R.KS)
def test_generic_sampler_row_table(hip_ops, oracle_ops, K, mode, impl):
    stats = {}
    R.row_table_case(hip_ops, oracle_ops, K, mode, impl, stats)
    print(f"K={K} mode {mode} impl {impl}: {stats}")


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [k for k in R.KS if k <= 64])
def test_generic_sampler_per_particle_rows(hip_ops, oracle_ops, K, mode, impl):
    stats = {}
    R.per_particle_case(hip_ops, oracle_ops, K, mode, impl, stats)
    print(f"K={K} mode {mode} impl {impl}: {stats}")


@pytest.mark.parametrize("impl", IMPLS)
def test_threshold_zero_skips_classes_of_weight_zero(hip_ops, oracle_ops, impl):
    """Words below 512 on rows whose only mass is behind classes at -inf (thr = 0 = C_c for every leading hole): the generic
    kernel and, through a one-site plan, the generated kernel's guide bucket 0 (its `bits <= bound` on a class of weight 0)."""
    ek, fold, words = R.edge_word_keys(hip_ops, impl)
    n = words.size
    for row in R.EDGE_ROWS:
        row = R.f32(row)
        v, _ = R.generic_case(hip_ops, oracle_ops, ek.with_fold(fold), n, row[None, :], 1, what=f"edge words {row.tolist()}")
        assert (_np(v) == int(np.argmax(row))).all()
        if row.size == 5:  # (one plan, one compilation: the row with three leading holes)
            R.edge_plan_case(hip_ops, oracle_ops, ek, fold, impl, row)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", R.PLAN_KS)
def test_generated_importance_kernel(hip_ops, oracle_ops, K, mode, impl, plan_mode):
    """One latent Categorical site whose row — every family of the grid — is picked by an input column: ONE plan, one
    compilation per case.  K <= 511 takes the guide path in mode 1 (peaked rows, zero-mass heads and tails make the buckets
    where `multi` is set and where the class is not the bucket's first), K >= 512 the on-the-fly jcat_invcdf.  Layers 1 and 2 on
    every draw, and the score — in the guide path the log-probability bits the table stores — against float64."""
    stats = {}
    for n in R.PLAN_NS:
        R.plan_case(hip_ops, oracle_ops, K, mode, impl, "input", n, stats)
    print(f"{plan_mode} K={K} mode {mode} impl {impl}: {stats}")


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("K", [17, 511, 513])
def test_generated_kernel_constant_and_flipped_rows(hip_ops, oracle_ops, K, impl, plan_mode):
    """The row as a literal (peak17: the row of the design note's 1.06e-5) and as an earlier Bernoulli draw."""
    stats = {}
    R.plan_case(hip_ops, oracle_ops, K, 1, impl, "one", 16384, stats, names=["peak17"])
    R.plan_case(hip_ops, oracle_ops, K, 1, impl, "flip", 16384, stats, names=["head5+tail5"])
    print(f"{plan_mode} K={K} impl {impl}: {stats}")


# ---- the scan plan in the HmmScan shape ------------------------------------------------------------------------------------

@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("kind", ["left_to_right", "peaked"])
@pytest.mark.parametrize("K", R.SCAN_KS)
def test_scan_plan_in_the_hmm_shape(hip_ops, oracle_ops, K, kind, impl):
    """`z' ~ categorical(trans[z]); y ~ categorical(obs[z'])` as one scan launch.  300 rows cut the guide from 2^11 buckets
    per row to 2^8 (cat_tables_prepare keeps the table within 2 MB: 300 x 512 x 16 B is still above), fewer buckets than
    classes, so the walk behind a bucket's second class runs.  Transition counts per source row against the float64 row, no
    forbidden transition, and logw against float64 from the recorded states."""
    print(f"K={K} {kind} impl {impl}: {R.scan_case(hip_ops, oracle_ops, impl, K, kind)}")


# ---- alias tables ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 3, 17, 255, 256])
def test_hmm_prepare_alias_tables(hip_ops, oracle_ops, K):
    st = R.alias_case(hip_ops, oracle_ops, K, {})
    print(f"K={K}: {st}")


# ---- the bootstrap HMM filter on a left-to-right table ---------------------------------------------------------------------

def test_bootstrap_hmm_filter_left_to_right(hip_ops, oracle_ops):
    """K = 8, T = 6, n = 4096, history recorded: no forbidden transition in the history, log Z within 5 RMS errors (measured
    on the CPU oracle over 32 seeds: cat_range_ref.HMM_LOGZ_RMS) of the float64 forward algorithm, and the oracle's bits."""
    import genjax
    from genjax._amd.runtime import use_ops

    res = {}
    for name, ops in (("hip", hip_ops), ("oracle", oracle_ops)):
        with use_ops(ops):
            res[name] = R.hmm_filter_run(ops, genjax.random.key(R.HMM_FILTER["seed"], 1))
    h, o = res["hip"], res["oracle"]
    R._same_bits(h.history, o.history, "filter history")
    R._same_bits(h.ancestors, o.ancestors, "filter ancestors")
    assert h.log_marginal_likelihood == o.log_marginal_likelihood
    R.hmm_filter_history_check(_np(h.history), _np(h.ancestors))
    exact = R.hmm_filter_exact()
    print(f"log Z {h.log_marginal_likelihood!r}, float64 {exact!r}, RMS of the oracle {R.HMM_LOGZ_RMS}")
    assert abs(h.log_marginal_likelihood - exact) <= 5.0 * R.HMM_LOGZ_RMS


# ---- the host API ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("impl", IMPLS)
def test_host_api_uniform_prior_over_1000_labels(hip_ops, oracle_ops, impl):
    """`Categorical` with sampling = "inverse_cdf" over 1000 equal logits in a one-site `@gen` model: the fused route (the
    generated kernel's on-the-fly walk) and the per-site route, equal bit for bit, on the device and on the oracle."""
    from genjax._amd.runtime import use_ops
    from test_cat_range_cpu import host_api_uniform_prior

    with use_ops(hip_ops):
        f, e = host_api_uniform_prior(impl)
    with use_ops(oracle_ops):
        of, _ = host_api_uniform_prior(impl)
    assert np.array_equal(f, e), "the fused route and the per-site route differ"
    assert np.array_equal(f, of), "the device and the oracle differ"
    print(f"impl {impl}: worst {R.frequency_check(np.full(1000, 1e-3), f):.3f} of the allowance")


# ---- the batched single-index draw -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("N", [1, 2, 65, 1000])
def test_categorical_index_batch(hip_ops, oracle_ops, N, impl):
    """gjx_categorical_index_batch, B = 20 000 draws in launches of 64 (the call's limit; the last one holds 32), rows a
    padded stride apart, by frequencies; entry b == categorical_index for 8 of them and == the oracle's for all."""
    B, per, stride = R.INDEX_B, 64, N + 3
    row = R.index_row(N)
    seed = R.seed_of("index", N, 0, impl)
    kbs = [R.key_batch(impl, b, seed) for b in range(B)]
    padded = np.full((per, stride), 50.0, dtype=np.float32)  # (beyond n: would win every draw if it were read)
    padded[:, :N] = row
    logits = R.to_dev(hip_ops, padded)
    v = torch.cat([hip_ops.categorical_index_batch(kbs[b:b + per], logits, N) for b in range(0, B, per)])
    vn = _np(v).astype(np.int64)
    R.never_draws_impossible(row, vn)
    print(f"N={N} impl {impl}: worst {R.frequency_check(R.softmax64(row), vn):.3f} of the allowance")
    L1 = R.to_dev(hip_ops, row)
    for b in (0, 1, 63, 64, 255, 4099, 12345, B - 1):
        assert int(hip_ops.categorical_index(kbs[b], L1, 0)) == int(vn[b]), b
    Lo = torch.from_numpy(row)
    ov = torch.cat([oracle_ops.categorical_index(k, Lo, 0) for k in kbs])  # (what the oracle's batch call is by definition)
    R._same_bits(v, ov, "categorical_index_batch")
