"""PSIS-LOO of a plated tempered plan without a GPU: include/gjx_psis.h as a header of its own in the slot the binding tables
leave free, the C-side validation before any launch, the tail-length and workspace rules, the generated kernel compiled for
gfx950 offline (one source per plan, no data in it, no scratch), the numpy reference against itself (split form / direct
form) and against the closed-form leave-one-out of the conjugate regression, the cases the GPU suite takes its k-hat range
from, the host logic of PSISLOO — and the launch geometry restated from the headers' text (psis_ref.chunks): every case of
tests/test_gpu_psis.py walks its chunks in one round and sorts at most 256 keys, every case of tests/test_gpu_psis_shapes.py
has the geometry, the key-space property and the recorded noise it is named for."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import plate_ref as P
import pointwise_ref as W
import psis_ref as S
import temper_ref as R
from genjax import ChoiceMap, Target, gen, normal
from genjax._amd import abi, temper
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax.inference.smc import PSISLOO, PointwiseLikelihood, TemperedSMC
from offline import header_symbols, kernel_notes, ops  # noqa: F401  (ops: a fixture)
import test_gpu_psis_shapes as T
from test_gpu_psis import CASES, MODELS, case_data, lower_all, population

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
SYMBOLS = {"gjx_psis_version", "gjx_psis_tail_len", "gjx_psis_workspace_bytes", "gjx_temper_psis", "gjx_psis_source",
           "gjx_psis_compile_check"}


@pytest.fixture(scope="module")
def lowered(ops):  # noqa: F811
    return lower_all(ops)


def test_header_is_registered(ops, oracle_ops):  # noqa: F811
    h = abi.PLAN_HEADERS["psis"]
    keys = list(abi.PLAN_HEADERS)
    # the slot the earlier suites leave: inside PLAN_HEADERS, before "plate" (plate, predictive, pointwise stay last, in a row)
    assert keys[-3:] == ["plate", "predictive", "pointwise"] and keys.index("psis") == keys.index("plate") - 1
    assert list(abi.MOVE_HEADERS) == ["temper_cov"] and h in abi.all_optional_headers()
    assert all("psis" not in t for t in (abi.OPTIONAL_HEADERS, abi.EXTENSION_HEADERS, abi.MOVE_HEADERS))
    syms = header_symbols("gjx_psis.h")
    assert h.header == "gjx_psis.h" and syms == set(h.prototypes) == SYMBOLS and h.version_fn in syms
    assert h.prototypes is abi.PSIS_PROTOTYPES and h.version == abi.PSIS_ABI_VERSION and h.unavailable is abi.PsisUnavailable
    assert issubclass(abi.PsisUnavailable, abi.HeaderUnavailable) and abi.PsisUnavailable.header == "gjx_psis.h"
    for other in abi.all_optional_headers():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes))
    assert not (syms & header_symbols("gjx.h"))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_psis and ops.lib.has["psis"] and not oracle_ops.lib.has_psis
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_psis_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == abi.PSIS_ABI_VERSION
    txt = open(__file__.replace("tests/test_psis_cpu.py", "include/gjx_psis.h")).read()
    assert f"GJX_PSIS_VERSION_MAJOR {major.value}" in txt and f"GJX_PSIS_VERSION_MINOR {minor.value}" in txt
    assert f"GJX_PSIS_MAX_TAIL {abi.PSIS_MAX_TAIL}" in txt and abi.PSIS_MAX_TAIL == S.MAX_TAIL == 4095
    assert [f for f, _ in abi.PsisIO._fields_] == ["n", "x", "tail_len", "out", "tail", "ws", "ws_bytes"]
    assert C.sizeof(abi.PsisIO) == 8 + 8 * abi.TEMPER_MAX_LATENTS + 8 + 4 * 8


def test_oracle_bound_ops_refuse(oracle_ops):
    target, _ = P.target("normal", 20)
    cols = [torch.zeros(64), torch.zeros(64)]
    with use_ops(oracle_ops):
        with pytest.raises(abi.HeaderUnavailable, match="gjx_temper|gjx_plate|gjx_psis"):
            TemperedSMC(target, 64).loo(cols)
    with pytest.raises(abi.PsisUnavailable, match="gjx_temper_psis"):
        oracle_ops.lib.call("gjx_temper_psis", None, None, None)
    with pytest.raises(abi.PsisUnavailable, match="gjx_psis_tail_len"):
        oracle_ops.lib.call("gjx_psis_tail_len", 100, 1.0)


def test_tail_len(ops):  # noqa: F811
    tl = lambda n, r=1.0: int(ops.lib.call("gjx_psis_tail_len", n, r))
    for n in (24, 25, 4096, 4099, 10 ** 6, 4 * 10 ** 6, 2 ** 31 - 1):
        for r in (1.0, 0.5):
            assert tl(n, r) == S.tail_len(n, r), (n, r)
    assert tl(24) == 0 and tl(25) == 5 and tl(4096) == 192 and tl(4099) == 193 and tl(10 ** 6) == 3000
    assert tl(4 * 10 ** 6) == 4095 and tl(4096, 0.5) == 272  # the cap (the package's rule gives 6000); a lower efficiency, a longer tail
    assert tl(0) == 0 and tl(1 << 31) == 0 and tl(4096, 0.0) == 0 and tl(4096, -1.0) == 0 and tl(4096, math.inf) == 0 and tl(4096, math.nan) == 0


def test_workspace(ops):  # noqa: F811
    ws = lambda n, D, M: int(ops.lib.call("gjx_psis_workspace_bytes", n, D, M))
    pad = lambda b: (b + 255) & ~255
    chunks = lambda n, D: min(-(-n // 256), max(1, -(-2048 // -(-D // 4))))
    for n, D, M in ((25, 5, 5), (4096, 64, 192), (4099, 300, 193), (10 ** 6, 1000, 3000), (10 ** 6, 10000, 3000), (4 * 10 ** 6, 64, 4095)):
        assert ws(n, D, M) == pad(D * 2048 * 4) + pad(D * 16) + pad(D * (M + 1) * 4) + pad(chunks(n, D) * D * 8), (n, D, M)
    assert ws(10 ** 6, 1000, 3000) < 25 * 2 ** 20  # 8 KB of histogram and 12 KB of keys per row
    for n, D, M in ((0, 5, 5), (5, 0, 5), (1 << 31, 5, 5), (100, 1 << 31, 5), (100, 5, 4), (10 ** 6, 5, 4096)):
        assert ws(n, D, M) == 0


def test_psis_validation(ops, monkeypatch):  # noqa: F811
    """Every refusal is decided on the host, before anything is compiled or launched (the pointers are never followed)."""
    lib = ops.lib
    with use_ops(ops):
        target, _ = P.target("normal", 20, 9)
        tr = temper.lower(target, 64)
        plan = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))  # (a plan of its own: no parameters, no data yet)
    D, n, M = 20, 1000, 95
    need = int(lib.call("gjx_psis_workspace_bytes", n, D, M))

    def io(**kw):
        o = abi.PsisIO()
        o.n, o.tail_len, o.out, o.tail, o.ws, o.ws_bytes = n, M, 0x4000, 0x6000, 0x8000, need
        for l in range(2):
            o.x[l] = 0x1000 * (l + 1)
        for k, v in kw.items():
            if k in ("x0", "x1"):
                o.x[int(k[1])] = v
            else:
                setattr(o, k, v)
        return o

    call = lambda p, o: lib._gjx_temper_psis(p, C.byref(o) if o is not None else None, None)
    monkeypatch.setenv("GJX_PLAN_JIT", "0")  # whatever passes validation stops at GJX_ERR_UNSUPPORTED: nothing is launched
    assert call(plan.handle, io()) == INVALID  # fewer parameters than the table reads (none set)
    plan.set_params(tr.params)
    assert call(plan.handle, io()) == INVALID  # a plated plan without data
    cols = (C.c_void_p * 2)(0x5000, 0x6000)
    assert lib._gjx_temper_plan_set_data(plan.handle, cols, 2, D) == 0
    assert call(plan.handle, io()) == UNSUPPORTED and call(plan.handle, io(tail=None)) == UNSUPPORTED  # valid: only the compiler stops it
    assert call(None, io()) == INVALID and call(plan.handle, None) == INVALID
    assert call(plan.handle, io(x0=None)) == INVALID and call(plan.handle, io(x1=None)) == INVALID and call(plan.handle, io(out=None)) == INVALID
    assert call(plan.handle, io(n=0)) == INVALID and call(plan.handle, io(n=1 << 31)) == INVALID
    assert call(plan.handle, io(ws=0x8004)) == INVALID  # not 8-byte aligned
    assert call(plan.handle, io(tail_len=4)) == INVALID and call(plan.handle, io(tail_len=0)) == INVALID
    assert call(plan.handle, io(tail_len=4096)) == INVALID and call(plan.handle, io(n=10 ** 6, tail_len=4096)) == INVALID
    assert call(plan.handle, io(tail_len=n)) == INVALID and call(plan.handle, io(tail_len=n + 1)) == INVALID  # tail_len >= n
    assert call(plan.handle, io(n=M, tail_len=M)) == INVALID and call(plan.handle, io(n=M + 1)) == UNSUPPORTED
    assert call(plan.handle, io(tail_len=5)) == UNSUPPORTED  # (a shorter tail needs no more workspace)
    assert call(plan.handle, io(ws=None)) == WORKSPACE and call(plan.handle, io(ws_bytes=need - 1)) == WORKSPACE
    assert call(plan.handle, io(tail_len=M + 64)) == WORKSPACE and call(plan.handle, io(n=(1 << 31) - 1)) == WORKSPACE
    # a plan without a PLATED site has no PSIS kernel
    with use_ops(ops):
        t2 = temper.lower(R.models()["regression"], 64)
        flat = ops.temper_plan_create(t2.sites, keep=(t2.keep, t2))
        flat.set_params(t2.params)
    assert call(flat.handle, io()) == INVALID and flat.psis_compile_check() == INVALID
    assert lib._gjx_psis_source(flat.handle, None, 0, C.byref(C.c_size_t())) == INVALID
    assert lib._gjx_psis_source(None, None, 0, C.byref(C.c_size_t())) == INVALID and lib._gjx_psis_compile_check(None) == INVALID
    with pytest.raises(ValueError, match="no plated site"):
        ops.temper_psis(flat, [torch.zeros(64), torch.zeros(64)], 12)
    with pytest.raises(ValueError, match="tail_len"):
        ops.temper_psis(plan, [torch.zeros(64), torch.zeros(64)], 64)


@pytest.mark.parametrize("name", MODELS)
def test_psis_source(ops, lowered, tmp_path, name):  # noqa: F811
    """One source per plan: it compiles for gfx950 without scratch, is the same text for other data and other lengths, holds no
    data value and neither n, D nor the tail length, shares the pointwise kernel's row term, and reads the rows' data through
    the constant address space (scalar loads)."""
    plan = lowered[name][1]
    src = plan.psis_source()
    assert plan.psis_compile_check() == 0
    assert "gjx_psis_kernel(PsisArgs a, PlanParams prm, PlanTables tabs, PlateData pd)" in src and "(PlateCol)pd.col[0]" in src
    assert "pd.n_rows" in src and "psis_take(" in src and "psis_flush(" in src and "asm" not in src and "gjx_pointwise_kernel" not in src
    term = lambda s, f: s[s.index(f"float {f}("):s.index("extern \"C\"")].replace(f, "TERM")
    assert term(src, "ps_term") == term(plan.pointwise_source(), "pw_term")  # t[d, i] is the pointwise kernel's, text for text
    for D in (64, 300):
        data = case_data(lowered, name, D)
        for t in data:  # no data value as a literal (literals are hex words: gjx_plan_jit.hpp flit)
            for v in np.ascontiguousarray(t, dtype=np.float32).view(np.uint32):
                assert f"0x{int(v):08x}u" not in src or v in (0, 0x3f800000)
    assert "a.n" in src and "a.per" in src  # (n, D and the tail length reach the kernel as arguments: the plan never knows them)
    k = kernel_notes(src, tmp_path, f"psis_{name}")["gjx_psis_kernel"]
    print("psis kernel,", name, k)  # (profiles/psis_summary.md records these)
    assert k["private_segment_fixed_size"] == 0 and k["agpr_count"] == 0 and k["vgpr_count"] <= 64  # eight waves per SIMD


def test_source_is_one_per_plan(ops, lowered):  # noqa: F811
    with use_ops(ops):
        for D, seed in ((1000, 3), (20, 5)):
            target, _ = P.target("normal", D, seed)
            tr = temper.lower(target, 64)
            assert ops.temper_plan_create(tr.sites, keep=(tr.keep, tr)).psis_source() == lowered["normal"][1].psis_source()


def test_reference_split_form_is_the_direct_form():
    """elpd_loo by the header's split form (body terms exact, body weights through B) against log sum w p - log sum w over all
    n entries, on a posterior population and on a resampled one.  B sums exponentials at arguments rounded to f32: each
    body weight carries a relative error of at most 2^-24 |arg|, so the two forms agree within 2^-23 (1 + spread)."""
    model = P.conjugate(40)
    t = W.terms_f64(model, W.posterior_columns(model, 8192, 6000)).astype(np.float32)
    idx = np.random.default_rng(1).integers(0, 1500, 4096)
    for tab in (t, t[:, :1500][:, idx]):
        M = S.tail_len(tab.shape[1])
        out = S.psis(tab, M)
        err = np.asarray([abs(S.direct(tab[d], M) - out["elpd"][d]) for d in range(40)])
        bound = 2.0 ** -23 * (1.0 + W.spread(tab))
        print("split form against the direct form", err.max(), "bound", bound.min())
        assert np.all(err <= bound) and np.all(out["bad"] == 0)


def test_reference_recovers_the_closed_form():
    """The numpy PSIS on populations from the exact posterior of the conjugate regression with 40 rows, n = 8192: two seeds
    outside the 24 the spread was measured over land within four times that spread of the closed-form leave-one-out sum;
    and the end-to-end case's condition (no khat above the threshold) holds on the reference's own populations."""
    model = P.conjugate(40)
    err = S.closed_form_errors(model, 8192, (6000, 6001))
    print("sum elpd_loo minus the closed form", err, "bound", S.CLOSED_FORM_FACTOR * S.SPREAD_ELPD_SUM, "closed form", S.closed_form_loo(model).sum())
    assert np.all(np.abs(err) <= S.CLOSED_FORM_FACTOR * S.SPREAD_ELPD_SUM)
    e, kmax, _ = S.e2e_errors(model, 4096, S.E2E_SEEDS[:2] + (9000,))
    assert np.all(np.abs(e) <= S.E2E_FACTOR * S.E2E_SPREAD_ELPD) and kmax.max() < min(1.0 - 1.0 / math.log10(4096), 0.7)
    assert S.E2E_MAX_KHAT < 0.7


def test_khat_cases_reach_both_sides(ops, oracle_ops, lowered):  # noqa: F811
    """The reference's khat on the two cases the GPU suite takes from psis_ref: above 0.7 on the moved row, negative on the
    narrow population."""
    tracer = lowered["normal"][0]
    for which in ("high", "low"):
        cols, data = S.khat_case(which, case_data(lowered, "normal", 64), population)
        out = S.psis(W.terms(P.Assess(oracle_ops, tracer, data), cols), S.tail_len(4096))
        print(which, "khat", out["khat"].min(), "..", out["khat"].max(), "row", out["khat"][S.HIGH_K["row"]])
        assert out["khat"][S.HIGH_K["row"]] > 0.7 if which == "high" else out["khat"].min() < 0.0


def test_psisloo_host_logic():
    """The scalars from a hand-made table: four rows, one above the threshold, one not smoothed."""
    D, n = 4, 1000
    elpd = np.array([-1.0, -2.5, 0.25, -0.75])
    khat = np.array([0.1, 0.69, 0.71, math.inf])
    table = torch.from_numpy(np.stack([elpd, khat, np.array([1.0, 2.0, 3.0, math.nan]), elpd - 5, elpd - 1, np.full(D, 900.0), np.zeros(D)]))
    lppd = np.array([-0.9, -2.0, 0.5, -0.7])
    pw = PointwiseLikelihood(torch.from_numpy(np.stack([lppd + math.log(n), np.zeros(D), np.zeros(D), np.full(D, float(n))])), n)
    loo = PSISLOO(table, pw, n, 95)
    assert loo.elpd_loo.dtype == torch.float64 and loo.elpd_loo.shape == loo.khat.shape == loo.sigma.shape == loo.bad.shape == (D,)
    assert loo.pointwise is pw and loo.n == n and loo.tail_len == 95
    assert math.isclose(loo.elpd, elpd.sum(), abs_tol=1e-12) and loo.looic == -2.0 * loo.elpd
    assert math.isclose(loo.se, math.sqrt(D * np.var(elpd, ddof=1)), abs_tol=1e-12)
    assert math.isclose(loo.p_loo, (lppd - elpd).sum(), abs_tol=1e-12)
    assert loo.khat_threshold == min(1.0 - 1.0 / 3.0, 0.7) and loo.n_high == 3  # 0.69, 0.71 and +inf are above 2/3
    big = PSISLOO(table, pw, 10 ** 6, 3000)
    assert big.khat_threshold == 0.7 and big.n_high == 2
    with pytest.raises(ValueError):
        PSISLOO(table.float(), pw, n, 95)
    with pytest.raises(ValueError):
        PSISLOO(table[:4], pw, n, 95)


def test_loo_refusals(ops):  # noqa: F811
    target, _ = P.target("normal", 20)

    @gen
    def unplated(s):
        w = normal(0.0, 2.0) @ "w"
        b = normal(0.0, 2.0) @ "b"
        normal(w + b, s) @ "y"

    with use_ops(ops):
        alg = TemperedSMC(target, 64)
        with pytest.raises(PlanUnsupported, match="no plated site"):
            TemperedSMC(Target(unplated, (0.1,), ChoiceMap.d({"y": 0.5})), 64).loo([torch.zeros(64), torch.zeros(64)])
        with pytest.raises(ValueError, match="2 latent columns"):
            alg.loo([torch.zeros(64)])
        with pytest.raises(TypeError):
            alg.loo([torch.zeros(64), torch.zeros(64)], target=target)  # LOO scores the fitted rows: there is no target=


# ---- the geometry of the GPU suites (tests/test_gpu_psis.py, tests/test_gpu_psis_shapes.py) ------------------------------------
# (n, D) of every case of tests/test_gpu_psis.py: the pins, then identical particles, the non-finite entries and the k-hat
# range (4096 x 64), the end-to-end case (40 rows)
OLD_SHAPES = sorted({(n, D) for _, n, D, _ in CASES} | {(4096, 5), (4096, 64), (4096, 40)})
NEW_SHAPES = ([(n, D) for _, n, D, _ in T.TRIP_CASES] + [(n, T.TAIL_D) for n, _ in T.TAIL_CASES] + [(T.OUTSIDE_N, T.TAIL_D)]
              + [(n, T.KEY_D) for n, _ in T.KEY_SIZES] + [(T.PUBLIC_N, T.PUBLIC_ROWS)])


def _terms(oracle_ops, lowered, name, data, cols):
    return W.terms(P.Assess(oracle_ops, lowered[name][0], data), cols)


def test_chunk_rule_is_the_librarys(ops):  # noqa: F811
    """psis_ref.chunks against the library through the last term of gjx_psis_workspace_bytes (8 W D bytes, padded), on every
    shape of both GPU suites and on the shapes tools/time_psis.py times."""
    pad = lambda b: (b + 255) & ~255
    for n, D in OLD_SHAPES + NEW_SHAPES + [(10 ** 6, 64), (10 ** 6, 1000), (10 ** 6, 10000)]:
        M = S.tail_len(n)
        Wc, per = S.chunks(n, D)
        fixed = pad(D * 2048 * 4) + pad(D * 16) + pad(D * (M + 1) * 4)
        assert int(ops.lib.call("gjx_psis_workspace_bytes", n, D, M)) - fixed == pad(Wc * D * 8), (n, D)
        sizes = S.chunk_sizes(n, D)
        assert len(sizes) == Wc and sum(sizes) == n and max(sizes) == per and S.first_trip(n, D).sum() == sum(min(c, 256) for c in sizes)


def test_existing_gpu_cases_run_every_loop_once():
    """The gap tests/test_gpu_psis_shapes.py closes: no case of tests/test_gpu_psis.py has a chunk of more than 256 particles,
    an empty chunk, or more than 256 keys to sort."""
    assert OLD_SHAPES == [(25, 5), (25, 64), (25, 300), (4096, 5), (4096, 40), (4096, 64), (4096, 300), (4099, 5), (4099, 64)]
    for n, D in OLD_SHAPES:
        assert S.trips(n, D) == 1 and S.empty_chunks(n, D) == 0 and S.first_trip(n, D).all() and S.sort_size(S.tail_len(n)) <= 256, (n, D)
    assert {S.chunks(n, D) for n, D in OLD_SHAPES} == {(1, 25), (16, 256), (17, 242)}
    assert {S.tail_len(n) for n, _ in OLD_SHAPES} == {5, 192, 193}


def test_new_gpu_cases_have_the_geometry_they_are_named_for():
    for name, n, D, kind in T.TRIP_CASES:
        g = T.TRIP_GEOMETRY[n, D]
        sizes = S.chunk_sizes(n, D)
        assert S.chunks(n, D) == (g["W"], g["per"]) and S.trips(n, D) == g["trips"] > 1 and S.empty_chunks(n, D) == g["empty"], (n, D)
        assert g["per"] - 256 * (g["trips"] - 1) == g["last"] and [c for c in sizes if c][-1] == g["short"], (n, D)
        assert S.tail_len(n) == g["M"] and S.sort_size(g["M"]) == g["P"] and not S.first_trip(n, D).all(), (n, D)
    assert S.chunk_sizes(526000, 3)[-1] == 0 and 2047 * 257 >= 526000 and 3 % 4 != 0  # an empty chunk; a row of the block switched off
    assert {g["last"] for g in T.TRIP_GEOMETRY.values()} >= {1} and max(g["P"] for g in T.TRIP_GEOMETRY.values()) == 4096
    for (n, M), (Pk, padding, Gn) in T.TAIL_CASES.items():
        assert M < n and S.sort_size(M) == Pk and Pk - (M + 1) == padding and S.candidates(M) == Gn, (n, M)
    assert sorted(M for n, M in T.TAIL_CASES if n == T.TAIL_N) == [255, 256, 257, 1000, 2047, 2048, 4095] and (4096, 4095) in T.TAIL_CASES
    assert [S.sort_size(M) for M in (255, 256, 257, 1000, 2047, 2048, 4095)] == [256, 512, 512, 1024, 2048, 4096, 4096]
    assert S.sort_size(T.OUTSIDE_M) == 1024 and T.OUTSIDE_M < T.OUTSIDE_N
    assert T.KEY_SIZES[0][1] == S.tail_len(T.KEY_SIZES[0][0]) == 192 and T.KEY_SIZES[1] == (6000, 1000)
    assert S.tail_len(T.PUBLIC_N) == 425 and S.sort_size(425) == 512 and S.tail_len(7226) == 256  # (the rule passes 255 above n = 7225)
    assert S.sort_size(5) == 8 and S.sort_size(7) == 8 and S.sort_size(8) == 16 and S.sort_size(S.MAX_TAIL) == 4096


def _new_case_terms(oracle_ops, lowered):
    """(label, t, M) of every case of tests/test_gpu_psis_shapes.py, from the oracle's replay."""
    for case in T.TRIP_CASES:
        name, n, D, _ = case
        yield case, _terms(oracle_ops, lowered, name, case_data(lowered, name, D), T.trip_columns(case)), S.tail_len(n)
    tails = {n: _terms(oracle_ops, lowered, "normal", case_data(lowered, "normal", T.TAIL_D), T.tail_columns(n)) for n in {n for n, _ in T.TAIL_CASES}}
    for n, M in sorted(T.TAIL_CASES):
        yield ("normal", n, M), tails[n], M
    yield "outside", _terms(oracle_ops, lowered, "hetero", case_data(lowered, "hetero", T.TAIL_D), T.outside_columns()), T.OUTSIDE_M
    for n, M in T.KEY_SIZES:
        for kind in T.KEY_KINDS:
            cols, data = T.key_case(lowered, kind, n, M)
            yield (kind, n, M), _terms(oracle_ops, lowered, "normal", data, cols), M
    model = P.conjugate(T.PUBLIC_ROWS)
    given = [model.xs.astype(np.float32), model.ys.astype(np.float32)]
    cols = W.posterior_columns(model, T.PUBLIC_N, T.PUBLIC_SEED)
    yield "public", _terms(oracle_ops, lowered, "normal", [given[k] for k in lowered["normal"][2]], cols), S.tail_len(T.PUBLIC_N)


@pytest.fixture(scope="module")
def new_cases(ops, oracle_ops, lowered):  # noqa: F811
    return list(_new_case_terms(oracle_ops, lowered))


def test_new_cases_have_their_properties_on_the_reference(new_cases):
    """On the reference's terms: the key-space classes (one bin twice, the sign boundary inside the tail, -inf entries on
    fewer / more particles than the tail, a heavy tie across the cutoff), a smoothed row in every tail-length case, NaN keys
    inside the tail of the `outside` case, no k-hat above 0.7 in the public call's population."""
    seen = set()
    for label, t, M in new_cases:
        ref = S.psis(t, M)
        if label in T.TRIP_CASES:
            assert np.isfinite(t).all() and np.isfinite(ref["khat"]).any(), label
        elif label == "outside":
            assert np.all(np.isnan(ref["tail"][:, M])) and np.all(np.isnan(ref["tail"]).sum(axis=1) > 1) and np.all(ref["bad"] > 0)
        elif label == "public":
            assert ref["khat"].max() <= 0.7 and np.all(ref["bad"] == 0)
        elif label[0] == "normal":
            assert np.isfinite(ref["khat"]).any(), label  # (otherwise the fit at this tail length would not be compared)
        else:
            T.key_property(label[0], t, M)
            seen.add(label[0])
            assert np.all(np.isposinf(ref["khat"])) and np.isnan(ref["elpd"]).all() if label[0].startswith("ninf") else np.isfinite(ref["elpd"]).all()
    assert seen == set(T.KEY_KINDS)


def test_first_round_only_is_caught_by_the_new_cases_alone(oracle_ops, lowered, new_cases):  # noqa: F811
    """What the trip-count cases are for, shown on the reference: a selection that saw only the particles of each chunk's
    FIRST round of 256 is the true one on every shape of tests/test_gpu_psis.py (it sees everything) and has another tail
    on every row of every trip-count case."""
    for n, D in OLD_SHAPES:
        assert S.first_trip(n, D).all()
    for label, t, M in new_cases:
        if label in T.TRIP_CASES:
            seen = S.first_trip(label[1], label[2])
            assert all(not np.array_equal(S.select(t[d][seen], M)[0], S.select(t[d], M)[0]) for d in range(len(t))), label


def test_recorded_noise_covers_a_fresh_measurement(new_cases):
    """psis_ref.MEASURED_REORDER_LARGE is no smaller than reorder_noise on every case of tests/test_gpu_psis_shapes.py, and
    the case recorded as the largest is the largest; the new table does not touch the old one."""
    worst = {q: (0.0, None) for q in S.MEASURED_REORDER_LARGE}
    for label, t, M in new_cases:
        r = S.reorder_noise(t, M)
        worst = {q: max(worst[q], (r[q], label), key=lambda v: v[0]) for q in worst}
    print("reorder noise over the new cases", worst)
    for q, (v, label) in worst.items():
        assert v <= S.MEASURED_REORDER_LARGE[q] and label == S.MEASURED_REORDER_LARGE_CASE[q], (q, v, label)
        assert S.TOL_LARGE[q] == max(S.REORDER_FACTOR * S.MEASURED_REORDER_LARGE[q], S.REORDER_FLOOR)
    assert S.MEASURED_REORDER == dict(khat=2.9e-14, sigma=3.1e-14, elpd=5.5e-14) and S.REORDER_FACTOR == 2.0 ** 10 and S.REORDER_FLOOR == 1e-11


def test_reference_recovers_the_closed_form_at_20000():
    """As test_reference_recovers_the_closed_form, at the public call's n = 20000: two seeds outside the 24 measured ones —
    one of them the GPU case's own — within four times the recorded spread, no k-hat above the threshold."""
    model = P.conjugate(T.PUBLIC_ROWS)
    err = S.closed_form_errors(model, T.PUBLIC_N, (T.PUBLIC_SEED, T.PUBLIC_SEED + 1))
    print("sum elpd_loo minus the closed form at n = 20000", err, "bound", S.CLOSED_FORM_FACTOR * S.SPREAD_ELPD_SUM_20000)
    assert np.all(np.abs(err) <= S.CLOSED_FORM_FACTOR * S.SPREAD_ELPD_SUM_20000) and S.SPREAD_ELPD_SUM_20000 < S.SPREAD_ELPD_SUM
    assert T.PUBLIC_SEED not in W.CLOSED_FORM_SEEDS and min(1.0 - 1.0 / math.log10(T.PUBLIC_N), 0.7) == 0.7
