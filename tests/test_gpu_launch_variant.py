"""Which generated kernel a launch takes, on the device: the form (one, two or four adjacent particles per lane) follows from the
keys, from n and from the alignment of the buffers, and the source variant (write-through stores, full outputs, fused tail) from
the passes and outputs of the launch.

Every case creates a plan whose source no other test compiles (one literal differs: the module cache cannot hold it), makes one
small launch with GJX_PLAN_JIT_DUMP_FILE set, and compares what the library compiled with what gjx_plan_specialized_source
returns for the expected form and flags.  Scan plans have no source getter: the dumped kernel's launch bounds (64: four
particles per lane, 256: one) and the presence of the in-launch fold are checked instead.  Each launch's log-weights equal the
oracle's bit for bit."""

import ctypes as C

import pytest
import torch

from genjax._amd import abi, prng, workloads as W
from genjax._amd.ops import KeyBatch

pytestmark = pytest.mark.gpu

FUSED_TAIL, WT_STORES, FULL_OUTPUTS = 0x100, 0x200, 0x400  # include/gjx.h GJX_SOURCE_*
SEED = 211


def same(a, b, what):
    assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)), what


def _c(v):
    return abi.Arg(abi.ARG_CONST, 0, 0.0, v, None)


def sites_of(case):
    """z ~ Normal(lit, 1); x ~ Normal(z + 0.1, 0.5); y ~ Normal(x, 0.3) observed at 0.7.  `lit` is the case's own."""
    def site(a0, a1, out_col=-1, obs=None):
        s = abi.Site()
        s.dist, s.observed, s.out_col = abi.DIST_NORMAL, 0 if obs is None else 1, out_col
        s.arg[0], s.arg[1] = a0, a1
        if obs is not None:
            s.obs = obs
        return s

    return [site(_c(0.4173 + 0.0009 * case), _c(1.0), 0), site(abi.Arg(abi.ARG_SITE, 0, 1.0, 0.1, None), _c(0.5), 1),
            site(abi.Arg(abi.ARG_SITE, 1, 1.0, 0.0, None), _c(0.3), obs=_c(0.7))]


def source_of(ops, plan, impl):
    need = C.c_size_t()
    ops.lib.call("gjx_plan_specialized_source", plan.handle, impl, None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value)
    ops.lib.call("gjx_plan_specialized_source", plan.handle, impl, buf, need.value, None)
    return buf.value.decode()


def keys_of(ops, kind, impl, p, n):
    kb = W.importance_particle_keys(prng.key(SEED + p, impl), n, 1 if kind == "first1" else 0)
    return KeyBatch(impl, 0, tensor=ops.rng_keys(kb, n)) if kind == "materialised" else kb


def launch(ops, plan, kind, impl, n, passes, score, lse):
    """One launch -> logw [passes, n]: gjx_importance_run (one pass; `lse`: with a gjx_lse_out) or gjx_importance_run_batch."""
    if passes == 1:
        out = ops.importance_run(plan, keys_of(ops, kind, impl, 0, n), n, [], [torch.float32] * 2, want_score=score, want_rows=True, fuse_lse=lse)
        return out[2].reshape(1, n)
    stride, R = -(-n // 256) * 256, ops.num_max_partials(n)
    vals = [ops.empty((passes, stride), torch.float32) for _ in range(2)]
    sc, lw, mp = ops.empty((passes, stride), torch.float32), ops.empty((passes, stride), torch.float32), ops.empty((passes, R), torch.float32)
    row_e, row_s = ops.empty((passes, R), torch.int32), ops.empty((passes, R), torch.int64)
    keys = (abi.Keys * passes)(*[ops._keys(keys_of(ops, kind, impl, p, n), n) for p in range(passes)])
    outs = (C.c_void_p * 2)(*[t.data_ptr() for t in vals])
    ops.lib.call("gjx_importance_run_batch", plan.handle, keys, passes, stride, R, (C.c_void_p * 1)(), 0, outs, 2, ops._p(sc) if score else None,
                 ops._p(lw), n, ops._p(mp), ops._p(row_e), ops._p(row_s), ops.stream())
    return lw[:, :n]


# name: (keys, generator, n, passes, score passed, gjx_lse_out passed, GJX_JIT_FORM of the launch) -> (form, flags) of the source
CASES = {
    "every_output_one_pass": (("lazy", 1, 1024, 1, True, False, None), ("quad", FULL_OUTPUTS | WT_STORES)),
    "every_output_three_passes": (("lazy", 1, 1024, 3, True, False, None), ("quad", FULL_OUTPUTS)),
    "no_score_one_pass": (("lazy", 1, 1024, 1, False, False, None), ("quad", WT_STORES)),
    "no_score_three_passes": (("lazy", 1, 1024, 3, False, False, None), ("quad", 0)),
    "lse_one_pass": (("lazy", 1, 1024, 1, True, True, None), ("quad", FUSED_TAIL | WT_STORES)),
    "n_1026": (("lazy", 1, 1026, 1, True, False, None), ("pair", 0)),
    "n_1025": (("lazy", 1, 1025, 1, True, False, None), ("one", 0)),
    "first_index_1": (("first1", 1, 1024, 1, True, False, None), ("one", 0)),
    "materialised_keys": (("materialised", 1, 1024, 1, True, False, None), ("one", 0)),
    "threefry": (("lazy", 0, 1024, 1, True, False, None), ("one", 0)),
    "form_pair_preferred": (("lazy", 1, 1024, 1, True, False, "pair"), ("pair", 0)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_importance_launch_takes_the_expected_source(hip_ops, oracle_ops, case, tmp_path, monkeypatch):
    (kind, impl, n, passes, score, lse, pref), (form, flags) = CASES[case]
    sites = sites_of(list(CASES).index(case))
    plan, oplan = hip_ops.plan_create(sites), oracle_ops.plan_create(sites)
    dump = tmp_path / "kernel.hip"
    monkeypatch.setenv("GJX_PLAN_JIT_DUMP_FILE", str(dump))
    monkeypatch.delenv("GJX_JIT_FORM", raising=False)
    if pref:
        monkeypatch.setenv("GJX_JIT_FORM", pref)
    logw = launch(hip_ops, plan, kind, impl, n, passes, score, lse)
    torch.cuda.synchronize()
    assert dump.exists(), "the launch compiled nothing: the module cache held its source"
    monkeypatch.setenv("GJX_JIT_FORM", form)
    assert dump.read_text() == source_of(hip_ops, plan, impl | flags), f"{case}: not the {form} source with flags {flags:#x}"
    for p in range(passes):
        ref = oracle_ops.importance_run(oplan, keys_of(oracle_ops, kind, impl, p, n), n, [], [torch.float32] * 2)[2]
        same(logw[p], ref, f"{case}: logw of pass {p}")


def scan_sites(case):
    sites, nxt = W.lgssm_scan_sites()
    sites[0].arg[1] = _c(0.8131 + 0.0007 * case)  # the transition's scale: this case's own literal
    return sites, nxt


@pytest.mark.parametrize("lse", [False, True])
@pytest.mark.parametrize("n,bounds", [(512, "__launch_bounds__(64)"), (513, "__launch_bounds__(256)")])
def test_scan_launch_takes_the_expected_kernel(hip_ops, oracle_ops, n, bounds, lse, tmp_path, monkeypatch):
    T = 2
    sites, nxt = scan_sites(2 * (n - 512) + int(lse))
    plan, oplan = hip_ops.scan_plan_create(sites, nxt, 1), oracle_ops.scan_plan_create(sites, nxt, 1)
    kb = W.importance_particle_keys(prng.key(SEED, 1), n)
    obs = W.lgssm_data(T).reshape(T, 1)
    dump = tmp_path / "kernel.hip"
    monkeypatch.setenv("GJX_PLAN_JIT_DUMP_FILE", str(dump))
    if lse:  # (Ops.scan_run passes no gjx_lse_out: it is put into the call's gjx_scan_io on the way)
        fold = [hip_ops.empty(1, torch.int32), hip_ops.empty(1, torch.int64), hip_ops.empty(1, torch.float32)]
        lo = abi.LseOut(fold[0].data_ptr(), fold[1].data_ptr(), fold[2].data_ptr(), None, hip_ops.tickets().data_ptr())
        call = hip_ops.lib.call

        def with_lse(name, *a):
            if name == "gjx_scan_run":
                a[1]._obj.lse = C.cast(C.pointer(lo), C.c_void_p)
            return call(name, *a)

        monkeypatch.setattr(hip_ops.lib, "call", with_lse)
    got = hip_ops.scan_run(plan, kb, n, T, obs, [0.25], [torch.float32])
    torch.cuda.synchronize()
    src = dump.read_text()
    assert bounds in src and src.count("__launch_bounds__") == 1
    assert ("lse_tail(" in src) == lse
    ref = oracle_ops.scan_run(oplan, kb, n, T, obs, [0.25], [torch.float32])
    same(got["logw"], ref["logw"], f"scan n={n} lse={lse}: logw")
    if lse:
        want = oracle_ops.lse_rows(ref["rows"])
        assert int(fold[0].cpu()) == int(want[1]) and int(fold[1].cpu()) == int(want[2]), "the in-launch fold of the row sums"
