"""The four kinds of store of the quad importance kernel on the device (plain, write-through, non-temporal, both hints), each forced
through its escape (GJX_JIT_DEFINE=GJX_STORES_*), against the unchanged oracle bit for bit and against one another.

Flagship sites and the sigma = 0.3 model with nonzero locations; one lane / one full wave / a row with one live lane / four rows
and a lane; 1, 2, 3 and 32 passes per launch.  Values, score, logw, max_partials, row_e and row_s equal the oracle's; the padding
between n and the pass stride keeps the sentinel it was filled with; columns that are views 16 bytes and 1 KiB into a larger
allocation; three launches in a row into the same buffers; one compilation per kind used.  (The oracle's passes are computed once
and shared with tests/test_gpu_row_cuts.py, whose keys these launches take.)"""

import ctypes as C

import pytest
import torch

from genjax._amd import abi, workloads as W
from test_gpu_row_cuts import MODELS, _c, keys_of, plans_of, reference, same, sigma03_sites

pytestmark = pytest.mark.gpu

ESCAPES = {"plain": "GJX_STORES_PLAIN", "wt": "GJX_STORES_WT", "nt": "GJX_STORES_NT", "nt_wt": "GJX_STORES_NT_WT"}
POPULATIONS = [4, 256, 260, 1028]
PASSES = [1, 2, 3, 32]
SENTINEL = 4321.25
TAIL = 512  # floats behind the last pass of a view (so that a view may start 1 KiB into its allocation)


def launch(ops, plan, ncol, n, L, score=True, offsets=(0, 0), key_shift=0, into=None):
    """One launch of L passes into sentinel-filled buffers -> dict of [L, stride] views (`offsets`: where, in floats, the even
    and the odd columns start inside their allocations; `into`: the buffers of an earlier launch, reused as they are)."""
    stride, R = -(-n // 256) * 256, ops.num_max_partials(n)
    if into is None:
        def col(k):
            base = torch.full((L * stride + TAIL,), SENTINEL, dtype=torch.float32, device=ops.device())
            return base, base[offsets[k % 2]:offsets[k % 2] + L * stride].view(L, stride)

        cols = [col(k) for k in range(ncol + 2)]
        into = dict(bases=[b for b, _ in cols], values=[v for _, v in cols[:ncol]], logw=cols[ncol][1], score=cols[ncol + 1][1],
                    mp=torch.full((L, R), SENTINEL, dtype=torch.float32, device=ops.device()), row_e=ops.empty((L, R), torch.int32),
                    row_s=ops.empty((L, R), torch.int64))
    o = into
    keys = (abi.Keys * L)(*[ops._keys(keys_of(p + key_shift, n), n) for p in range(L)])
    ins = (C.c_void_p * 1)()
    outs = (C.c_void_p * ncol)(*[t.data_ptr() for t in o["values"]])
    ops.lib.call("gjx_importance_run_batch", plan.handle, keys, L, stride, R, ins, 0, outs, ncol, C.c_void_p(o["score"].data_ptr()) if score else None,
                 C.c_void_p(o["logw"].data_ptr()), n, ops._p(o["mp"]), ops._p(o["row_e"]), ops._p(o["row_s"]), ops.stream())
    return o


def check(o, oracle_ops, oplan, model, ncol, n, L, tag, score=True, offsets=(0, 0)):
    for p in range(L):
        ref = reference(oracle_ops, oplan, model, p, n)
        what = f"{tag}, pass {p} of {L}"
        for c in range(ncol):
            same(o["values"][c][p, :n], ref["values"][c], f"column {c}, {what}")
        same(o["logw"][p, :n], ref["logw"], f"logw, {what}")
        if score:
            same(o["score"][p, :n], ref["score"], f"score, {what}")
        same(o["mp"][p], ref["mp"], f"row maxima, {what}")
        same(o["row_e"][p], ref["row_e"], f"row anchors e, {what}")
        same(o["row_s"][p], ref["row_s"], f"row sums S, {what}")
    # nothing but the n particles of each pass was written: the padding up to the stride, and the allocation round a view
    cols = o["values"] + [o["logw"]] + ([o["score"]] if score else [])
    for k, t in enumerate(cols):
        assert bool((t[:, n:] == SENTINEL).all()), f"padding of column {k} written, {tag}"
    if not score:
        assert bool((o["score"] == SENTINEL).all()), f"an absent score was written, {tag}"
    stride = o["logw"].shape[1]
    for k, base in enumerate(o["bases"]):
        off = offsets[k % 2]
        assert bool((base[:off] == SENTINEL).all()) and bool((base[off + L * stride:] == SENTINEL).all()), f"bytes outside view {k} written, {tag}"


@pytest.mark.parametrize("kind", list(ESCAPES))
@pytest.mark.parametrize("model", ["flagship", "sigma03"])
def test_every_kind_equals_the_oracle(hip_ops, oracle_ops, model, kind, monkeypatch):
    monkeypatch.setenv("GJX_JIT_DEFINE", ESCAPES[kind])
    hplan, oplan = plans_of(hip_ops, oracle_ops, model)
    ncol = MODELS[model][1]
    for n in POPULATIONS:
        for L in PASSES:
            check(launch(hip_ops, hplan, ncol, n, L), oracle_ops, oplan, model, ncol, n, L, f"{model}, {kind}, n={n}")


@pytest.mark.parametrize("kind", list(ESCAPES))
def test_kinds_agree_without_a_score_in_views_and_after_earlier_launches(hip_ops, oracle_ops, kind, monkeypatch):
    """The guarded source (no score passed); columns that start 16 bytes (even ones) and 1 KiB (odd ones) into their allocations;
    three launches into the same buffers, the first two under other keys, the last one checked."""
    monkeypatch.setenv("GJX_JIT_DEFINE", ESCAPES[kind])
    model, n = "sigma03", 1028
    hplan, oplan = plans_of(hip_ops, oracle_ops, model)
    ncol = MODELS[model][1]
    for L in (1, 3):
        check(launch(hip_ops, hplan, ncol, n, L, score=False), oracle_ops, oplan, model, ncol, n, L, f"no score, {kind}", score=False)
        offsets = (4, 256)
        check(launch(hip_ops, hplan, ncol, n, L, offsets=offsets), oracle_ops, oplan, model, ncol, n, L, f"views, {kind}", offsets=offsets)
        o = launch(hip_ops, hplan, ncol, n, L, key_shift=100)
        launch(hip_ops, hplan, ncol, n, L, key_shift=200, into=o)
        check(launch(hip_ops, hplan, ncol, n, L, into=o), oracle_ops, oplan, model, ncol, n, L, f"third launch, {kind}")


def test_one_compilation_per_kind_used(hip_ops, monkeypatch):
    sites = sigma03_sites()
    sites[1].arg[1] = _c(0.3173)  # a structure no other test compiles
    plan = hip_ops.plan_create(sites)
    compiles = lambda: hip_ops.jit_stats()["compiles"]  # noqa: E731
    c0 = compiles()
    logw = {}
    for i, (kind, escape) in enumerate(ESCAPES.items()):
        monkeypatch.setenv("GJX_JIT_DEFINE", escape)
        logw[kind] = launch(hip_ops, plan, 2, 260, 3)["logw"].clone()
        assert compiles() == c0 + i + 1, f"{kind}: a kernel of its own"
    for kind, escape in ESCAPES.items():
        monkeypatch.setenv("GJX_JIT_DEFINE", escape)
        same(launch(hip_ops, plan, 2, 260, 3)["logw"], logw["plain"], f"{kind} == plain")
    assert compiles() == c0 + 4, "nothing is compiled twice"


def test_a_batch_of_the_benchmark_s_size_takes_both_hints_by_the_rule(hip_ops, oracle_ops, tmp_path, monkeypatch):
    """No escape: 32 passes that write 1.5 GB (ImportanceVariant::stores_of's threshold) compile the source with both hints, and its
    outputs equal those of the same launch under forced plain stores, every pass, and the oracle's in the last pass."""
    n, L, ncol = 2_930_000, 32, 2  # 16 bytes per particle and pass: 1.50016e9 bytes per launch
    sites = sigma03_sites()
    sites[1].arg[1] = _c(0.3391)  # a structure no other test compiles
    hplan, oplan = hip_ops.plan_create(sites), oracle_ops.plan_create(sites)
    dump = tmp_path / "kernel.hip"
    monkeypatch.delenv("GJX_JIT_DEFINE", raising=False)
    monkeypatch.setenv("GJX_PLAN_JIT_DUMP_FILE", str(dump))
    got = launch(hip_ops, hplan, ncol, n, L)
    torch.cuda.synchronize()
    src = dump.read_text()
    assert "const bool wt_one_pass = true;" in src and "const bool nt_stores = true;" in src, "not the source with both hints"
    small = tmp_path / "small.hip"  # one pass fewer stays under the threshold: plain stores, as before
    monkeypatch.setenv("GJX_PLAN_JIT_DUMP_FILE", str(small))
    launch(hip_ops, hplan, ncol, n, L - 1)
    torch.cuda.synchronize()
    assert "const bool wt_one_pass = false;" in small.read_text() and "nt_stores" not in small.read_text()
    monkeypatch.delenv("GJX_PLAN_JIT_DUMP_FILE")
    monkeypatch.setenv("GJX_JIT_DEFINE", ESCAPES["plain"])
    ref = launch(hip_ops, hplan, ncol, n, L)
    for k in ("logw", "score", "mp", "row_e", "row_s"):
        assert torch.equal(got[k], ref[k]), f"{k}: both hints != plain"
    for c in range(ncol):
        assert torch.equal(got["values"][c], ref["values"][c]), f"column {c}: both hints != plain"
    assert bool((got["logw"][:, n:] == SENTINEL).all()) and bool((got["score"][:, n:] == SENTINEL).all())
    p = L - 1
    vals, score, logw, mp, rows = oracle_ops.importance_run(oplan, keys_of(p, n), n, [], [torch.float32] * ncol, want_rows=True)
    same(got["logw"][p, :n], logw, "logw of the last pass")
    same(got["score"][p, :n], score, "score of the last pass")
    same(got["values"][1][p, :n], vals[1], "column 1 of the last pass")
    same(got["row_e"][p], rows.e, "row anchors of the last pass")
    same(got["row_s"][p], rows.s, "row sums of the last pass")
