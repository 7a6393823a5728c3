"""Posterior predictive draws of a plated tempered plan without a GPU: include/gjx_predictive.h as a header of its own in the
slot the binding tables leave free, the generated predictive kernel compiled for gfx950 offline (one source per plan and
generator, no data in it, no scratch), the existing tempered sources left as they were, the C-side validation before any
launch, the chunk and workspace rule, the host logic of PosteriorPredictive, the refusals of `predictive()`, and the replay
of tests/predictive_ref.py against the oracle's own sampler and the closed form of the conjugate regression."""

import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import genjax
import plate_ref as P
import pointwise_ref as W
import predictive_ref as Q
import temper_ref as R
from genjax import ChoiceMap, Target, gen, normal
from genjax._amd import abi, prng, temper
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax.inference.smc import PosteriorPredictive, TemperedSMC
from offline import header_symbols, kernel_notes, ops  # noqa: F401  (ops: a fixture)

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
SYMBOLS = {"gjx_predictive_version", "gjx_predictive_chunks", "gjx_predictive_workspace_bytes", "gjx_temper_predictive",
           "gjx_predictive_source", "gjx_predictive_compile_check"}

# sha256 of the generated sources of plate_ref.MODELS lowered from 20 rows — the move kernel and the covariance move kernel
# per generator (TemperPlan.source(impl), cov_source(impl)) and the pointwise kernel — generated with the build of the commit
# before the predictive kernels existed: they add nothing to and change nothing in those sources.
PARENT_SOURCE_SHA256 = {
    ("normal", "move", 0): "65fd151cc0bde5c1c4194225bc2b7ac0b749d2b164b5ffaca0d39e217b2440ce",
    ("normal", "cov", 0): "8017c46dafd3318989a2754af137ff6a6ebffa6bf93567a6a621b67dc12072d7",
    ("normal", "move", 1): "54ea155818ee8bcade0388aa1aa8b6b31024d70f5686151071513603706976bf",
    ("normal", "cov", 1): "562fc62b30c1a30acc90408d1cee89596b5d5b0c8517a4c2705e5ab7478e6abb",
    ("normal", "pointwise", 0): "f61fbfddcae6b6bf5cc423f7a9e20104484d2b2bf6f2b22b78e7298ae1682a0f",
    ("hetero", "move", 0): "f981378f3e4d8a5c812441eeb9f896009f8dfd630116b61cb23a59e2370adca0",
    ("hetero", "cov", 0): "41ebb3ab6fcb2df66f84a1643a0ae86ffac9e2784098d0e37135fed88c60e70c",
    ("hetero", "move", 1): "62b4e0b20716fd6a1618dcefc3bc4dde5daf8e61637033b8aba9a49035358093",
    ("hetero", "cov", 1): "520b04b2cf3ac33b5ada6e9a52b3ff7ba1e14f5323d907610597cd4255cea6d7",
    ("hetero", "pointwise", 0): "40376fd96565de79a0fa3fb5a1326dac2aa0ab3fed3c0a4fc61a5246350ce713",
    ("logistic", "move", 0): "fe5a70112457fb2d43d873d86e33ab902c8e4c70c4501a1d40c908a71ea9e363",
    ("logistic", "cov", 0): "6203f45a2ac4cd94e7cd686c1ec1ff64ed40dae0be4db829c7e3e064a1b742bd",
    ("logistic", "move", 1): "6781db23c368582005ae57b71d2d929bd258dda3a079562222e3b1b9768f0eda",
    ("logistic", "cov", 1): "cffeff7bb7dc19b76c86d5803177508fe99ab5420dfead7f20f926b72a335b3f",
    ("logistic", "pointwise", 0): "8ba41da1865705f00d0627b1aa415b7826e7e126b408a519973d506728ece1fb",
    ("gamma_rate", "move", 0): "6a579cd3ae075bd87a69b48e4cd9e716f143b6fb642ee7acb73601229a5af92b",
    ("gamma_rate", "cov", 0): "cbabd1f971b99ecff53abfd030cfcdd49e1a9790516db4b98abc55558fc5f598",
    ("gamma_rate", "move", 1): "e5fcb506f98ece7943c96b43c3b375585a7755be558070c401c40940da1361be",
    ("gamma_rate", "cov", 1): "34d008a3af73f1ca5cb1f4fe6dd7973abc083e083a7cfc3d6026efa7834947fc",
    ("gamma_rate", "pointwise", 0): "1f98428135165709c54b0eb9f3c5bb5f6c41b52aea16d644a460f94af205240c",
}
# ... and of the predictive kernel per generator (TemperPlan.predictive_source(impl)), the two-plate body included, generated with
# the build of the commit before the tempered generators shared one shadow table and one particle loop.
PARENT_PREDICTIVE_SHA256 = {
    ("normal", 0): "30b0bfe243f5861fc1a392fb4f0331f4c654440604f817f29c4ef633d7ca8839",
    ("normal", 1): "90bdc0149df6eb7491e7faaf2a1466d267cebbc49c0af51c2530c970c311e58e",
    ("hetero", 0): "bc0cc773b657815ba52591cd1a394c9156dbb35ae94ddbf35005b6319029f849",
    ("hetero", 1): "7480b1e1d2daba8b0c222dfd0662cb4cc8c7a6c908a62b8a451f40eab7cdc1c4",
    ("logistic", 0): "2579704f6634e51b410bdedd0acae46187f4bce949b40c6eb1c974abf06bae3b",
    ("logistic", 1): "8213d9a9b8ce27f054dd936af25d8eb93a7e5498aeebf708d69fa0086b354d6b",
    ("gamma_rate", 0): "188dbb3fa9d2c3e23f9c7d6e97428e19146f96fa95d029c245cc21b49fd122dd",
    ("gamma_rate", 1): "e7fe2dc718e12f5c46babe59bdce1cca123bfd0913aca64ed29c418d7280ff8d",
    ("two_plate", 0): "3c512c8b5fc8ec21101637a10ac22341ed16bed757336ebb91085f1b29afe203",
    ("two_plate", 1): "9451d98b9bbd6b8b9a631fe9bb4f2f82eab07c5666d00de5d9e5d63380562e5a",
}

# Vector registers: at most 128 (four waves per SIMD out of 512).  ONE kernel does not meet it: `gamma_rate` under THREEFRY —
# two interleaved Marsaglia-Tsang rejection loops, each with a cipher block of its own in flight — takes 139; it is held to
# three waves per SIMD instead (512 / 3 = 170, in allocation granules of 8: 168).  profiles/predictive_summary.md has the counts.
VGPR_LIMIT = 128
VGPR_EXCEPTIONS = {("gamma_rate", 0): 168}


def _lower(ops, name, D, seed=0):  # noqa: F811
    with use_ops(ops):
        target, data = P.target(name, D, seed)
        tracer = temper.lower(target, 64)
        return target, tracer, ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer)), data


def _two_plate(ops, D=20, seed=0):  # noqa: F811
    import temper_fuzz as F

    xs, zs, y1, y2 = P.two_plate_data(D, seed)
    with use_ops(ops):
        target = F.target_of(P.TWO_PLATE, (xs, zs), {"y1": y1, "y2": y2})
        tracer = temper.lower(target, 64)
        return target, tracer, ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer)), [torch.from_numpy(c) for c in (xs, zs, y1, y2)]


@pytest.fixture(scope="module")
def lowered(ops):  # noqa: F811
    out = {name: _lower(ops, name, 20) for name in P.MODELS}
    out["two_plate"] = _two_plate(ops)
    return out


def test_header_is_registered(ops, oracle_ops):  # noqa: F811
    h = abi.PLAN_HEADERS["predictive"]
    keys = list(abi.PLAN_HEADERS)
    assert keys.index("predictive") == keys.index("plate") + 1 == keys.index("pointwise") - 1 and keys[-1] == "pointwise"
    assert h in abi.all_optional_headers() and list(abi.MOVE_HEADERS) == ["temper_cov"] and abi.all_optional_headers()[-1].key == "temper_cov"
    assert "predictive" not in abi.OPTIONAL_HEADERS and "predictive" not in abi.EXTENSION_HEADERS and "predictive" not in abi.MOVE_HEADERS
    syms = header_symbols("gjx_predictive.h")
    assert h.header == "gjx_predictive.h" and syms == set(h.prototypes) == SYMBOLS and h.version_fn in syms
    assert h.prototypes is abi.PREDICTIVE_PROTOTYPES and h.version == abi.PREDICTIVE_ABI_VERSION and h.unavailable is abi.PredictiveUnavailable
    assert issubclass(abi.PredictiveUnavailable, abi.HeaderUnavailable) and abi.PredictiveUnavailable.header == "gjx_predictive.h"
    for other in abi.all_optional_headers():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes))
    assert not (syms & header_symbols("gjx.h"))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_predictive and ops.lib.has["predictive"] and not oracle_ops.lib.has_predictive
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_predictive_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == abi.PREDICTIVE_ABI_VERSION == (0, 1)
    txt = open(__file__.replace("tests/test_predictive_cpu.py", "include/gjx_predictive.h")).read()
    assert f"GJX_PREDICTIVE_VERSION_MAJOR {major.value}" in txt and f"GJX_PREDICTIVE_VERSION_MINOR {minor.value}" in txt
    assert '#include "gjx_plate.h"' in txt and "gjx_pointwise.h\"" not in txt
    assert [f for f, _ in abi.PredictiveIO._fields_] == ["n", "x", "out", "draws", "draw_stride", "ws", "ws_bytes"]
    assert C.sizeof(abi.PredictiveIO) == 8 + 8 * abi.TEMPER_MAX_LATENTS + 5 * 8
    assert abi.PredictiveIO.draws.offset == 8 + 8 * abi.TEMPER_MAX_LATENTS + 8 and abi.PredictiveIO.ws_bytes.offset == C.sizeof(abi.PredictiveIO) - 8


def test_oracle_bound_ops_refuse(oracle_ops):
    target, _ = P.target("normal", 20)
    cols = [torch.zeros(8), torch.zeros(8)]
    key = genjax.random.key(0, "philox")
    with use_ops(oracle_ops):
        with pytest.raises(abi.HeaderUnavailable, match="gjx_temper|gjx_plate|gjx_predictive"):
            TemperedSMC(target, 64).predictive(cols, key)
    with pytest.raises(abi.PredictiveUnavailable, match="gjx_temper_predictive"):
        oracle_ops.lib.call("gjx_temper_predictive", None, None, None, None)
    with pytest.raises(abi.PredictiveUnavailable, match="gjx_predictive_chunks"):
        oracle_ops.lib.call("gjx_predictive_chunks", 1, 1)
    with pytest.raises(abi.PredictiveUnavailable, match="gjx_temper_predictive"):
        oracle_ops.temper_predictive(None, key, cols)


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("name", P.MODELS + ("two_plate",))
def test_predictive_source(ops, lowered, name, impl):  # noqa: F811
    """One source per plan and generator: it compiles for gfx950, is the same text for D = 20 and D = 1000 and for other data
    values, holds no data value, no LDS, no barrier and no inline assembly, reads the latent columns through the constant
    address space (scalar loads), and draws through the importance kernel's emitters."""
    plan, data = lowered[name][2], lowered[name][3]
    src = plan.predictive_source(impl)
    assert plan.predictive_compile_check(impl) == 0
    others = (_two_plate(ops, 1000, seed=3), _two_plate(ops, 20, seed=5)) if name == "two_plate" else (_lower(ops, name, 1000, seed=3), _lower(ops, name, 20, seed=5))
    assert src == others[0][2].predictive_source(impl) == others[1][2].predictive_source(impl)
    assert src != plan.predictive_source(1 - impl)
    assert "gjx_predictive_kernel(PredictiveArgs a, PlanParams prm, PlanTables tabs, PlateData pd)" in src
    assert "(PlateCol)a.x[0]" in src and "pd.n_rows" in src and f"predictive_pass_key<{impl}>(a.key, i)" in src
    assert "predictive_take(qA[s], yA[s], obA[s])" in src and "predictive_keep_rows<" in src and "predictive_store(" in src
    # PHILOX: the pair block of rows (2r, 2r + 1) once per lane (single-word draws), a Gamma site's two rows drawn together
    assert ("philox4x32(pk0, pk1, (uint32_t)pair0" in src) == (impl == 1 and name != "gamma_rate")
    assert ("std_gamma_multi<1, 2>" in src) == (impl == 1 and name == "gamma_rate")
    assert "__shared__" not in src and "__syncthreads" not in src and "asm" not in src
    assert "gjx_temper_move_kernel" not in src and "gjx_pointwise_kernel" not in src
    S = 2 if name == "two_plate" else 1
    assert f"PredictiveAcc qA[{S}], qB[{S}];" in src
    for t in data:  # no data value as a literal (literals are hex words: gjx_plan_jit.hpp flit)
        for v in t.to(torch.float32).numpy().view(np.uint32):
            assert f"0x{int(v):08x}u" not in src or v in (0, 0x3f800000)


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("name", P.MODELS + ("two_plate",))
def test_predictive_kernel_has_no_scratch(lowered, tmp_path, name, impl):
    k = kernel_notes(lowered[name][2].predictive_source(impl), tmp_path, f"predictive_{name}_{impl}")["gjx_predictive_kernel"]
    print("predictive kernel,", name, impl, k)  # (profiles/predictive_summary.md records these)
    assert k["private_segment_fixed_size"] == 0 and k["agpr_count"] == 0
    assert k["vgpr_count"] <= VGPR_EXCEPTIONS.get((name, impl), VGPR_LIMIT)


def test_existing_sources_are_the_parents(lowered):
    for (name, kind, impl), want in PARENT_SOURCE_SHA256.items():
        plan = lowered[name][2]
        src = plan.source(impl) if kind == "move" else plan.cov_source(impl) if kind == "cov" else plan.pointwise_source()
        assert hashlib.sha256(src.encode()).hexdigest() == want, (name, kind, impl)


def test_predictive_sources_are_the_parents(lowered):
    for (name, impl), want in PARENT_PREDICTIVE_SHA256.items():
        assert hashlib.sha256(lowered[name][2].predictive_source(impl).encode()).hexdigest() == want, (name, impl)


def test_chunks_and_workspace(ops):  # noqa: F811
    lib = ops.lib
    ch = lambda n, D: int(lib.call("gjx_predictive_chunks", n, D))
    ws = lambda n, D, S: int(lib.call("gjx_predictive_workspace_bytes", n, D, S))
    rule = lambda n, D: min(-(-n // 256), max(1, -(-2048 // -(-D // 512))))
    cases = [(1, 1), (256, 1), (257, 1), (1000, 513), (10 ** 6, 64), (10 ** 6, 1000), (10 ** 6, 10000), (2 ** 31 - 1, 2 ** 31 - 1),
             (10 ** 6, 512 * 2048), (10 ** 6, 512 * 2048 + 1), (5000, 513), (1000, 129)]
    for n, D in cases:
        assert ch(n, D) == rule(n, D), (n, D)
        for S in (1, 2, 5):
            assert ws(n, D, S) == 40 * ch(n, D) * D * S, (n, D, S)
    assert ch(257, 20) == 2 and ch(1000, 129) == 4 and ch(10 ** 6, 1000) == 1024 and ch(10 ** 6, 64) == 2048 and ch(10 ** 6, 10000) == 103
    assert ws(10 ** 6, 1000, 1) == 1024 * 1000 * 40  # 41 MB
    for n, D in ((0, 5), (5, 0), (1 << 31, 5), (5, 1 << 31)):
        assert ch(n, D) == 0 and ws(n, D, 1) == 0
    assert ws(1000, 20, 0) == 0 and ws(1000, 20, -1) == 0 and ws(1000, 20, abi.MAX_SITES + 1) == 0


def test_predictive_validation(ops, lowered, monkeypatch):  # noqa: F811
    """Every refusal is decided on the host, before anything is compiled or launched (the pointers are never followed)."""
    lib = ops.lib
    _, tr, plan, _ = _lower(ops, "normal", 20, seed=9)  # (a plan of its own: no parameters, no data yet)
    D, n = 20, 1000
    need = int(lib.call("gjx_predictive_workspace_bytes", n, D, 1))

    def io(**kw):
        o = abi.PredictiveIO()
        o.n, o.out, o.ws, o.ws_bytes = n, 0x4000, 0x8000, need
        for l in range(2):
            o.x[l] = 0x1000 * (l + 1)
        for k, v in kw.items():
            if k == "x0":
                o.x[0] = v
            elif k == "x1":
                o.x[1] = v
            else:
                setattr(o, k, v)
        return o

    def keys(kb):
        return ops._keys(kb, 1)

    lit = {impl: keys(genjax.random.key(3, impl).literal()) for impl in ("threefry", "philox")}
    call = lambda p, k, o: lib._gjx_temper_predictive(p, C.byref(k) if k is not None else None, C.byref(o) if o is not None else None, None)
    monkeypatch.setenv("GJX_PLAN_JIT", "0")  # whatever passes validation stops at GJX_ERR_UNSUPPORTED: nothing is launched
    k1 = lit["philox"]
    assert call(plan.handle, k1, io()) == INVALID  # fewer parameters than the table reads (none set)
    plan.set_params(tr.params)
    assert call(plan.handle, k1, io()) == INVALID  # a plated plan without data
    cols = (C.c_void_p * 2)(0x5000, 0x6000)
    assert lib._gjx_temper_plan_set_data(plan.handle, cols, 2, D) == 0
    for k in lit.values():
        assert call(plan.handle, k, io()) == UNSUPPORTED  # valid: only the switched-off compiler stops it
        assert call(plan.handle, k, io(draws=0x9000, draw_stride=7)) == UNSUPPORTED
        assert call(plan.handle, k, io(draws=0x9000, draw_stride=0)) == UNSUPPORTED
    laned = keys(prng.PRNGKey(1, 2, 1, 5).literal())  # (a PHILOX key with a lane is one literal key too)
    assert call(plan.handle, laned, io()) == UNSUPPORTED
    assert call(None, k1, io()) == INVALID and call(plan.handle, None, io()) == INVALID and call(plan.handle, k1, None) == INVALID
    # a key that is not ONE literal key: a lazy batch, an explicit batch, a stream fold, a generator that is none, a THREEFRY lane
    base = genjax.random.key(3, "philox")
    assert call(plan.handle, keys(prng.split_lazy(base, 4)), io()) == INVALID
    explicit = keys(base.literal())
    explicit.mode, explicit.keys = 0, 0x7000
    assert call(plan.handle, explicit, io()) == INVALID
    assert call(plan.handle, keys(base.literal().with_fold(0)), io()) == INVALID
    bad_impl = keys(base.literal())
    bad_impl.impl = 2
    assert call(plan.handle, bad_impl, io()) == INVALID
    tf_lane = keys(genjax.random.key(3, "threefry").literal())
    tf_lane.parent_lane = 1
    assert call(plan.handle, tf_lane, io()) == INVALID
    assert call(plan.handle, k1, io(x0=None)) == INVALID and call(plan.handle, k1, io(x1=None)) == INVALID and call(plan.handle, k1, io(out=None)) == INVALID
    assert call(plan.handle, k1, io(n=0)) == INVALID and call(plan.handle, k1, io(n=1 << 31)) == INVALID
    assert call(plan.handle, k1, io(draw_stride=1)) == INVALID and call(plan.handle, k1, io(draw_stride=1 << 40)) == INVALID  # draws NULL
    assert call(plan.handle, k1, io(ws=0x8004)) == INVALID  # not 8-byte aligned
    assert call(plan.handle, k1, io(ws=None)) == WORKSPACE and call(plan.handle, k1, io(ws_bytes=need - 1)) == WORKSPACE
    assert call(plan.handle, k1, io(n=(1 << 31) - 1)) == WORKSPACE  # (a larger population needs a larger workspace)
    # a plan without a PLATED site has no predictive kernel; neither has a generator that is none
    with use_ops(ops):
        t2 = temper.lower(R.models()["regression"], 64)
        flat = ops.temper_plan_create(t2.sites, keep=(t2.keep, t2))
        flat.set_params(t2.params)
    assert call(flat.handle, k1, io()) == INVALID and flat.predictive_compile_check(1) == INVALID
    assert lib._gjx_predictive_source(flat.handle, 1, None, 0, C.byref(C.c_size_t())) == INVALID
    assert lib._gjx_predictive_source(None, 1, None, 0, C.byref(C.c_size_t())) == INVALID and lib._gjx_predictive_compile_check(None, 1) == INVALID
    assert lib._gjx_predictive_source(plan.handle, 2, None, 0, C.byref(C.c_size_t())) == INVALID and plan.predictive_compile_check(-1) == INVALID
    with pytest.raises(ValueError, match="no plated site"):
        ops.temper_predictive(flat, genjax.random.key(0, "philox"), [torch.zeros(4), torch.zeros(4)])


def test_input_column_tables_are_refused(ops):  # noqa: F811
    """A table that reads a per-particle input column has no predictive kernel (the io has no such columns)."""
    _, tr, _, _ = _lower(ops, "normal", 20)
    sites = [abi.Site.from_buffer_copy(s) for s in tr.sites]
    sites[1].arg[0] = abi.Arg(abi.ARG_INPUT, 0, 1.0, 0.0, None)  # the prior of `b` reads input column 0
    plan = ops.temper_plan_create(sites, keep=(tr.keep, tr))
    plan.set_params(tr.params)
    cols = (C.c_void_p * 2)(0x5000, 0x6000)
    assert ops.lib._gjx_temper_plan_set_data(plan.handle, cols, 2, 20) == 0
    o = abi.PredictiveIO()
    o.n, o.out, o.ws, o.ws_bytes = 8, 0x4000, 0x8000, 1 << 20
    o.x[0], o.x[1] = 0x1000, 0x2000
    k = ops._keys(genjax.random.key(3, "philox").literal(), 1)
    assert ops.lib._gjx_temper_predictive(plan.handle, C.byref(k), C.byref(o), None) == INVALID
    assert plan.predictive_compile_check(1) == INVALID


def test_posterior_predictive_host_logic():
    n, D, S, k = 10, 4, 2, 3
    rng = np.random.default_rng(0)
    y = rng.standard_normal((S, D, n)).astype(np.float32)
    obs = y[:, :, 3].copy()  # (one draw equals the observed value exactly)
    table = torch.from_numpy(Q.summarize(y, obs))
    draws = torch.from_numpy(np.ascontiguousarray(np.transpose(y, (0, 2, 1))[:, ::k]))
    pp = PosteriorPredictive(["y1", ("y", 2)], table, n, draws, k)
    y64 = y.astype(np.float64)
    for s, a in enumerate(pp.addresses):
        assert np.allclose(pp.mean[a].numpy(), y64[s].mean(axis=1), rtol=0, atol=1e-15)
        assert np.allclose(pp.var[a].numpy(), y64[s].var(axis=1, ddof=1), rtol=0, atol=1e-14)
        below = (y[s] < obs[s][:, None]).sum(axis=1)
        assert np.array_equal(pp.below[a].numpy(), below) and np.array_equal(pp.equal[a].numpy(), np.ones(D))
        assert np.array_equal(pp.pit[a].numpy(), (below + 0.5) / n) and np.array_equal(pp.nan_count[a].numpy(), np.zeros(D))
        assert pp.draws[a].shape == (4, D) and torch.equal(pp.draws[a], draws[s])
        for f in (pp.mean, pp.var, pp.pit, pp.below, pp.equal, pp.nan_count):
            assert f[a].dtype == torch.float64 and f[a].shape == (D,)
    assert torch.equal(pp.index, torch.tensor([0, 3, 6, 9])) and pp.index.dtype == torch.int64
    # nothing observed: no pit, no counts against an observed value
    free = PosteriorPredictive(["y1", ("y", 2)], table, n, observed=False)
    assert free.pit is None and free.below is None and free.equal is None and free.draws is None and free.index is None
    assert torch.equal(free.mean["y1"], pp.mean["y1"]) and torch.equal(free.nan_count[("y", 2)], pp.nan_count[("y", 2)])
    # n = 1: no variance to speak of — zeros
    one = PosteriorPredictive(["y1", ("y", 2)], torch.from_numpy(Q.summarize(y[:, :, :1], obs)), 1)
    assert torch.equal(one.var["y1"], torch.zeros(D, dtype=torch.float64)) and np.array_equal(one.mean["y1"].numpy(), y64[0, :, 0])
    # a NaN draw: counted, visible in the moments, neither below nor equal
    y2 = y.copy()
    y2[0, 1, 5] = np.nan
    nan = PosteriorPredictive(["y1", ("y", 2)], torch.from_numpy(Q.summarize(y2, obs)), n)
    assert nan.nan_count["y1"][1] == 1 and torch.isnan(nan.mean["y1"][1]) and torch.isnan(nan.var["y1"][1])
    assert nan.below["y1"][1] + nan.equal["y1"][1] <= n - 1 and torch.isfinite(nan.mean["y1"][[0, 2, 3]]).all()
    for bad in (lambda: PosteriorPredictive(["y1", "y2"], table.float(), n), lambda: PosteriorPredictive(["y1"], table, n),
                lambda: PosteriorPredictive(["y1", "y2"], table, 0), lambda: PosteriorPredictive(["y1", "y2"], table, n, draws),
                lambda: PosteriorPredictive(["y1", "y2"], table, n, None, 3), lambda: PosteriorPredictive(["y1", "y2"], table, n, draws, 2),
                lambda: PosteriorPredictive(["y1", "y2"], table, n, draws.double(), k)):
        with pytest.raises(ValueError):
            bad()


def test_predictive_refusals(ops):  # noqa: F811
    target, _ = P.target("normal", 20)
    cols = [torch.zeros(8), torch.zeros(8)]
    key = genjax.random.key(0, "philox")

    @gen
    def other_names(xs, s):
        w = normal(0.0, 2.0) @ "slope"
        b = normal(0.0, 2.0) @ "b"
        normal(w * xs + b, s) @ "y"

    @gen
    def swapped(xs, s):
        b = normal(0.0, 2.0) @ "b"
        w = normal(0.0, 2.0) @ "w"
        normal(w * xs + b, s) @ "y"

    @gen
    def unplated(s):
        w = normal(0.0, 2.0) @ "w"
        b = normal(0.0, 2.0) @ "b"
        normal(w + b, s) @ "y"

    xs, ys = torch.linspace(0.0, 1.0, 7), torch.ones(7)
    held = Target(P.bodies()["normal"], (xs, 0.1), ChoiceMap.d({"y": ys}))
    with use_ops(ops):
        alg = TemperedSMC(target, 64)
        with pytest.raises(ValueError, match=r"\['slope', 'b'\].*\['w', 'b'\]"):
            alg.predictive(cols, key, target=Target(other_names, (xs, 0.1), ChoiceMap.d({"y": ys})))
        with pytest.raises(ValueError, match=r"\['b', 'w'\].*\['w', 'b'\]"):
            alg.predictive(cols, key, target=Target(swapped, (xs, 0.1), ChoiceMap.d({"y": ys})))
        with pytest.raises(PlanUnsupported, match="no plated site.*'y'"):
            alg.predictive(cols, key, target=Target(unplated, (0.1,), ChoiceMap.d({"y": 0.5})))
        with pytest.raises(PlanUnsupported, match="no plated site"):
            TemperedSMC(Target(unplated, (0.1,), ChoiceMap.d({"y": 0.5})), 64).predictive(cols, key)
        with pytest.raises(PlanUnsupported, match="data columns"):
            alg.predictive(cols, key, args=(0.5, 0.1))
        with pytest.raises(ValueError, match="not both"):
            alg.predictive(cols, key, target=held, args=(xs, 0.1))
        with pytest.raises(ValueError, match="not both"):
            alg.predictive(cols, key, n_draws=4, draw_stride=2)
        with pytest.raises(ValueError, match="n_draws >= 1"):
            alg.predictive(cols, key, n_draws=0)
        with pytest.raises(ValueError, match="draw_stride >= 1"):
            alg.predictive(cols, key, draw_stride=0)
        with pytest.raises(ValueError, match="2 latent columns"):
            alg.predictive(cols[:1], key)
        with pytest.raises(TypeError):
            alg.predictive(cols, key, target="held out")
        with pytest.raises(TypeError):
            alg.predictive(cols, key, args=[xs, 0.1])
        # args=: the fitted model at new inputs, every plated address constrained to zeros of the data length
        t = alg._unobserved_target(alg._state(), (xs, 0.1))
        assert isinstance(t, Target) and t.p is target.p and t.args == (xs, 0.1)
        assert torch.equal(t.constraint["y"], torch.zeros(7)) and temper.lower(t, 64).data_rows == 7


# ---- the replay's own checks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["threefry", "philox"])
def test_replay_normal_rows_are_the_oracles_sampler(ops, oracle_ops, impl):  # noqa: F811
    """The replay's rows of the Normal regression equal gjx_sample_logpdf_normal of the oracle under the same key batch
    and the site's fold (THREEFRY: the 1-based site counter of the shadow table; PHILOX: the 0-based draw index), at the
    location the table computes in f32."""
    D, n = 37, 6
    _, tr, _, data = _lower(ops, "normal", D, seed=4)
    data = [t.to(torch.float32).numpy().copy() for t in data]
    key = genjax.random.key(5, impl)
    replay = Q.Replay(oracle_ops, tr, data, key.impl)
    assert replay.S == 1 and replay.addrs == ["y"] and replay.sites[0].observed == 0 and replay.sites[0].out_col == 0
    assert replay.sites[0].arg[0].kind == abi.ARG_EXPR and replay.sites[0].arg[1].kind == abi.ARG_PARAM
    cols = W.centred_columns("normal", n, np.random.default_rng(6))
    y = replay.draws(key, cols)
    assert y.shape == (1, D, n)
    fold = 1 if key.impl == 0 else 0
    for i in range(n):
        loc = (cols[0][i] * data[0] + cols[1][i]).astype(np.float32)  # (w * xs) + b, one f32 rounding each
        val, _ = oracle_ops.sample_logpdf("normal", replay.key_batch(key, i).with_fold(fold), D, torch.from_numpy(loc), float(np.float32(0.1)),
                                          want_score=False)
        assert Q.same_bits(y[0, :, i], val.numpy()), (impl, i)
    assert np.array_equal(replay.observed()[0], data[1])
    # another key, another particle index: other draws
    assert not Q.same_bits(y[0, :, 0], replay.particle(key, 1, [c[0] for c in cols])[0])
    assert not Q.same_bits(y[0, :, 0], replay.particle(genjax.random.key(6, impl), 0, [c[0] for c in cols])[0])


def test_replay_recovers_the_closed_form(ops, oracle_ops):  # noqa: F811
    """The replay on a population of 8192 from the exact posterior of the conjugate regression with 500 rows sits within four
    times the spreads the float64 numpy reference measured; so does that reference at two seeds outside the 24."""
    model = P.conjugate(500)
    n = 8192
    ref = Q.closed_form_errors(model, n, (9000, 9001))
    bound = Q.CLOSED_FORM_FACTOR * np.array([Q.SPREAD_MEAN, Q.SPREAD_VAR, Q.SPREAD_PIT])
    print("numpy reference errors (mean, var, pit)", ref, "bound", bound)
    assert np.all(ref <= bound)
    xs, ys = torch.tensor(model.xs, dtype=torch.float32), torch.tensor(model.ys, dtype=torch.float32)
    with use_ops(ops):
        tracer = temper.lower(Target(P.bodies()["normal"], (xs, model.noise), ChoiceMap.d({"y": ys})), 64)
    replay = Q.Replay(oracle_ops, tracer, [xs.numpy(), ys.numpy()], 1)
    cols = W.posterior_columns(model, n, 9002)
    y = replay.draws(genjax.random.key(7, "philox"), cols)
    t = Q.summarize(y, replay.observed())[0]
    mean, var = t[0] / n, (t[1] - t[0] * t[0] / n) / (n - 1)
    e = np.array(Q.errors_of(model, n, mean, var, (t[2] + 0.5 * t[3]) / n))
    print("replay errors (mean, var, pit)", e, "bound", bound)
    assert np.all(e <= bound) and np.all(t[4] == 0)
