"""Plan specialisation without a GPU: the straight-line HIP source generated for a site table
compiles for gfx950 (hiprtc cross-compiles offline), for both RNG schemes and for plans touching
every distribution / argument kind."""

import os

import pytest

from genjax._amd import abi, workloads as W
from offline import HIP_LIB, ROOT, importance_source as source_of, ops as hip_lib_nogpu  # noqa: F401


@pytest.mark.parametrize("impl", [0, 1])
def test_gaussian10_plan_compiles(hip_lib_nogpu, impl, monkeypatch):
    ops = hip_lib_nogpu
    plan = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))
    monkeypatch.setenv("GJX_JIT_FORM", "pair")
    src1 = source_of(ops, plan, impl)
    if impl == 0:  # jax key tree: one particle per lane, erfinv normals, 20 log-densities
        assert src1.count("std_normal(") == 10 and src1.count("logpdf_normal_pre(") == 20
        assert "__launch_bounds__(256" in src1 and "GJX_BM_LDS" not in src1 and "bm_stage" not in src1
    else:
        # the paired form: two adjacent particles per lane (A, B), ONE Box-Muller transform per Normal site for
        # the pair, and the pair's single-word draws two sites to a Philox block whatever is observed in between
        # (10 draws x 2 particles -> 5 blocks per pair), the cipher key is the (launch-uniform) parent key
        assert src1.count("bm_pair(") == 10 and src1.count("std_normal(") == 0
        assert src1.count("logpdf_normal_pre(") == 40
        assert src1.count("kTagPair") == 5 and src1.count("philox4x32(") == 5
        # the Box-Muller tables are staged in LDS once per workgroup, before the grid-stride loop over rows
        assert src1.startswith("#define GJX_BM_LDS 1") and src1.count("bm_stage();") == 1
        assert src1.index("bm_stage();") < src1.index("for (uint64_t g0")
        assert "ks.parent.k0" in src1 and "__launch_bounds__(128" in src1
        # the default form: FOUR adjacent particles per lane = two pairs, one wave per 256-particle row (no LDS,
        # no barrier in the row statistics), 16-byte column stores
        monkeypatch.delenv("GJX_JIT_FORM")
        src4 = source_of(ops, plan, impl)
        assert src4.count("bm_pair(") == 20 and src4.count("logpdf_normal_pre(") == 80
        assert src4.count("kTagPair") == 10 and "__launch_bounds__(64" in src4
        assert "make_uint4(" in src4 and "__syncthreads" not in src4.split("lse_tail")[0].split("void gjx_plan_kernel_philox")[1]
        # GJX_PLAN_FAST_MATH switches the device header's continuous functions to the hardware transcendentals
        fast = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()), fast_math=True)
        fsrc = source_of(ops, fast, impl)
        assert fsrc.startswith("#define GJX_FAST_MATH 1") and "GJX_BM_LDS" not in fsrc and "bm_stage" not in fsrc
        assert src4.startswith("#define GJX_BM_LDS 1") and src4.count("bm_stage();") == 1
        ops.lib.call("gjx_plan_compile_check", fast.handle, impl)
    ops.lib.call("gjx_plan_compile_check", plan.handle, impl)


@pytest.mark.parametrize("impl", [0, 1])
def test_mixed_plan_compiles(hip_lib_nogpu, impl):
    ops = hip_lib_nogpu
    A = abi.Arg
    fake_table = 0x7F0000001000  # pointers are only embedded, never dereferenced here
    s = []
    p = abi.Site(); p.dist, p.out_col = abi.DIST_BETA, 0
    p.arg[0], p.arg[1] = A(abi.ARG_CONST, 0, 0, 2.0, None), A(abi.ARG_CONST, 0, 0, 2.0, None); s.append(p)
    v = abi.Site(); v.dist, v.observed, v.out_col = abi.DIST_BERNOULLI, 1, -1
    v.arg[0] = A(abi.ARG_SITE, 0, 1.0, 0.0, None); v.obs = A(abi.ARG_CONST, 0, 0, 1.0, None); s.append(v)
    g = abi.Site(); g.dist, g.out_col = abi.DIST_GAMMA, 1
    g.arg[0], g.arg[1] = A(abi.ARG_CONST, 0, 0, 0.7, None), A(abi.ARG_SITE, 0, 2.0, 0.5, None); s.append(g)
    for mode in (0, 1):
        c = abi.Site(); c.dist, c.out_col = abi.DIST_CATEGORICAL, 2 + mode
        c.n_cat, c.n_rows, c.cat_mode = 3, 2, mode
        c.arg[0] = A(abi.ARG_SITE, 1, 1.0, 0.0, None); c.logits = fake_table; s.append(c)
    x = abi.Site(); x.dist, x.out_col = abi.DIST_NORMAL, 4
    x.arg[0], x.arg[1] = A(abi.ARG_TABLE, 3, 0, 0, fake_table), A(abi.ARG_INPUT, 0, 1.0, 0.1, None); s.append(x)
    y = abi.Site(); y.dist, y.observed, y.out_col = abi.DIST_NORMAL, 1, -1
    y.arg[0], y.arg[1] = A(abi.ARG_SITE, 5, 0.5, 1.0, None), A(abi.ARG_CONST, 0, 0, 2.0, None)
    y.obs = A(abi.ARG_INPUT, 1, 0, 0, None); s.append(y)
    plan = ops.plan_create(s)
    ops.lib.call("gjx_plan_compile_check", plan.handle, impl)


def test_invalid_plans_are_rejected(hip_lib_nogpu):
    ops = hip_lib_nogpu
    bad = abi.Site(); bad.dist = abi.DIST_NORMAL
    bad.arg[0] = abi.Arg(abi.ARG_SITE, 3, 1.0, 0.0, None)  # refers to a later site
    bad.arg[1] = abi.Arg(abi.ARG_CONST, 0, 0, 1.0, None)
    with pytest.raises(abi.GjxError):
        ops.plan_create([bad])
    with pytest.raises(abi.GjxError):
        ops.plan_create([])


@pytest.mark.parametrize("impl", [0, 1])
def test_smc_plan_compiles(hip_lib_nogpu, impl):
    """The generated step policy + init kernel of a plan-driven bootstrap filter compile offline."""
    ops = hip_lib_nogpu
    A = abi.Arg
    c = lambda v: A(abi.ARG_CONST, 0, 0.0, v, None)

    def site(dist, a0, a1=None, obs=None):
        s_ = abi.Site()
        s_.dist, s_.observed, s_.out_col = dist, 0 if obs is None else 1, -1
        s_.arg[0] = a0
        if a1 is not None:
            s_.arg[1] = a1
        if obs is not None:
            s_.obs = obs
        return s_

    plan = ops.smc_plan_create(
        [site(abi.DIST_NORMAL, c(0.0), c(1.0)), site(abi.DIST_GAMMA, c(2.0), c(2.0)),
         site(abi.DIST_NORMAL, A(abi.ARG_SITE, 0, 1.0, 0.0, None), c(0.7), A(abi.ARG_OBS, 0, 1.0, 0.0, None))],
        [site(abi.DIST_NORMAL, A(abi.ARG_STATE, 0, 0.8, 0.0, None), c(0.5)),
         site(abi.DIST_GAMMA, c(0.6), A(abi.ARG_STATE, 1, 1.0, 1.0, None)),
         site(abi.DIST_BERNOULLI, c(0.3)),
         site(abi.DIST_NORMAL, A(abi.ARG_SITE, 0, 1.0, 0.0, None), c(0.7), A(abi.ARG_OBS, 0, 1.0, 0.0, None))],
        [A(abi.ARG_SITE, 0, 1.0, 0.0, None), A(abi.ARG_SITE, 1, 1.0, 0.0, None)],
        [A(abi.ARG_SITE, 0, 1.0, 0.0, None), A(abi.ARG_SITE, 1, 0.5, 0.1, None)], 1)
    ops.lib.call("gjx_smc_plan_compile_check", plan.handle, impl)
    with pytest.raises(abi.GjxError):  # a STATE reference is not allowed in the init table
        ops.smc_plan_create([site(abi.DIST_NORMAL, A(abi.ARG_STATE, 0, 1.0, 0.0, None), c(1.0))],
                            [site(abi.DIST_NORMAL, c(0.0), c(1.0))], [c(0.0)], [c(0.0)], 0)


@pytest.mark.parametrize("impl", [0, 1])
def test_scan_plans_compile(hip_lib_nogpu, impl):
    """The one-launch scan kernels (gjx_scan_run) generate and compile for gfx950 offline."""
    from test_gpu_parity_abi import _scan_plans

    for plan in _scan_plans(hip_lib_nogpu):
        assert plan.compile_check(impl) == 0
    sites, nxt = W.lgssm_scan_sites()
    fast = hip_lib_nogpu.scan_plan_create(sites, nxt, 1, fast_math=True)
    assert fast.compile_check(impl) == 0


def test_hmm_scan_plan_compiles(hip_lib_nogpu):
    """categorical sites whose logits row is chosen by the carried state / an earlier site (the HMM as a scan kernel)"""
    for mode in (0, 1):
        A = abi.Arg
        z = abi.Site(); z.dist, z.observed, z.out_col = abi.DIST_CATEGORICAL, 0, 0
        z.n_cat, z.n_rows, z.cat_mode = 16, 16, mode
        z.arg[0] = A(abi.ARG_STATE, 0, 1.0, 0.0, None); z.logits = 0x7F0000001000
        y = abi.Site(); y.dist, y.observed, y.out_col = abi.DIST_CATEGORICAL, 1, -1
        y.n_cat, y.n_rows, y.cat_mode = 16, 16, mode
        y.arg[0] = A(abi.ARG_SITE, 0, 1.0, 0.0, None); y.obs = A(abi.ARG_OBS, 0, 1.0, 0.0, None); y.logits = 0x7F0000002000
        plan = hip_lib_nogpu.scan_plan_create([z, y], [A(abi.ARG_SITE, 0, 1.0, 0.0, None)], 1)
        for impl in (0, 1):
            assert plan.compile_check(impl) == 0


@pytest.mark.parametrize("impl", [0, 1])
def test_plans_with_invalid_constants_compile(hip_lib_nogpu, impl):
    """Compile-time constants that make a log-density NaN / infinite (a negative rate, a gamma observation below zero, NaN
    and infinite literals, a scale of zero) once put a CONSTANT NaN / +inf log-weight into the generated kernel, and this
    toolchain's backend died on it ("SmallVector unable to grow") — in-process, taking the caller with it.  Such constants
    are kept out of constant propagation now (gjx_device.hpp `opq`): the kernels compile, and DESIGN 3.11's GPU tests
    check what they compute."""
    ops = hip_lib_nogpu
    A = abi.Arg
    c = lambda v: A(abi.ARG_CONST, 0, 0.0, v, None)  # noqa: E731

    def site(dist, a0, a1=None, obs=None, out_col=-1):
        s_ = abi.Site()
        s_.dist, s_.observed, s_.out_col = dist, 0 if obs is None else 1, out_col
        s_.arg[0] = a0
        if a1 is not None:
            s_.arg[1] = a1
        if obs is not None:
            s_.obs = obs
        return s_

    nan, inf = float("nan"), float("inf")
    # the filter the fuzzer found: an observed gamma with rate -1 (its hoisted log-normaliser is NaN) feeding later sites
    init = [site(abi.DIST_GAMMA, c(1.746), c(-1.0), obs=c(1.827)),
            site(abi.DIST_BETA, A(abi.ARG_SITE, 0, 1.076, 0.759, None), A(abi.ARG_SITE, 0, 1.468, 0.706, None)),
            site(abi.DIST_GAMMA, A(abi.ARG_SITE, 1, 0.56, 0.82, None), c(3.0e38))]
    step = [site(abi.DIST_NORMAL, A(abi.ARG_STATE, 0, 0.8, 0.0, None), c(0.5)),
            site(abi.DIST_NORMAL, A(abi.ARG_SITE, 0, 1.0, 0.0, None), c(0.0), obs=A(abi.ARG_OBS, 0, 1.0, 0.0, None))]
    plan = ops.smc_plan_create(init, step, [A(abi.ARG_SITE, 0, 1.0, 0.0, None)], [A(abi.ARG_SITE, 0, 1.0, 0.0, None)], 1)
    ops.lib.call("gjx_smc_plan_compile_check", plan.handle, impl)
    tables = [
        [site(abi.DIST_NORMAL, c(0.0), c(1.0), out_col=0), site(abi.DIST_NORMAL, c(0.0), c(1.0), obs=c(inf))],      # +inf observation, all constant
        [site(abi.DIST_NORMAL, c(0.0), c(1.0), out_col=0), site(abi.DIST_GAMMA, c(2.0), c(1.5), obs=c(-0.5))],       # below the support
        [site(abi.DIST_NORMAL, c(0.0), c(1.0), out_col=0), site(abi.DIST_NORMAL, A(abi.ARG_SITE, 0, 1.0, 0.0, None), c(0.0), obs=c(0.3))],  # scale 0
        [site(abi.DIST_NORMAL, c(nan), c(-1.0), out_col=0), site(abi.DIST_BETA, c(-2.0), c(inf), out_col=1),
         site(abi.DIST_BERNOULLI, c(1.5), out_col=2), site(abi.DIST_NORMAL, A(abi.ARG_SITE, 1, 1.0, 0.0, None), c(1.0), obs=c(nan))],
        [site(abi.DIST_GAMMA, c(0.0), c(0.0), out_col=0), site(abi.DIST_NORMAL, c(1.0e38), c(1.0e-38), obs=c(-3.0e38))],
    ]
    keep = []
    neg = abi.expr_arg([(abi.EXPR_CONST, 0, 1.0), (abi.EXPR_CONST, 0, 3.0), (abi.EXPR_SUB, 0, 0.0)], keep)       # 1 - 3: a negative scale
    zero_by_zero = abi.expr_arg([(abi.EXPR_CONST, 0, 0.0), (abi.EXPR_CONST, 0, 0.0), (abi.EXPR_DIV, 0, 0.0)], keep)
    tables.append([site(abi.DIST_NORMAL, c(0.0), c(1.0), out_col=0),                                             # programs over literals only
                   site(abi.DIST_NORMAL, A(abi.ARG_SITE, 0, 1.0, 0.0, None), neg, obs=A(abi.ARG_INPUT, 0, 1.0, 0.0, None)),
                   site(abi.DIST_NORMAL, zero_by_zero, c(1.0), obs=c(0.2)), site(abi.DIST_GAMMA, neg, neg, out_col=1)])
    for sites in tables:
        plan = ops.plan_create(sites)
        ops.lib.call("gjx_plan_compile_check", plan.handle, impl)


def test_a_compiler_crash_is_an_error_code_not_an_abort():
    """hiprtc runs the AMDGPU backend in the caller's process, so a backend crash on generated source
    used to be an abort of the caller.  The library now compiles in a child process (csrc/gjx_jitc.cpp, next to the
    library): a source that makes the compiler DIE (`#pragma clang __debug crash`), or fail, comes back as GJX_ERR_JIT —
    and this process is still here to assert it; a valid kernel compiles."""
    import ctypes as C

    from genjax._amd import abi

    lib = abi.GjxLib(HIP_LIB, "cuda")
    good = b'#include "gjx_device.hpp"\nextern "C" __global__ void k(float* x) { x[threadIdx.x] = gjx::u2f(0x3f800000u); }\n'
    assert lib._gjx_jit_compile_source(good) == 0
    crash = b'#include "gjx_device.hpp"\n#pragma clang __debug crash\nextern "C" __global__ void k(float* x) { x[0] = 1.0f; }\n'
    assert lib._gjx_jit_compile_source(crash) == -6  # GJX_ERR_JIT
    bad = b'extern "C" __global__ void k(float* x) { this is not C++ }\n'
    assert lib._gjx_jit_compile_source(bad) == -6
    assert lib._gjx_jit_compile_source(good) == 0  # and the compiler is still usable
    _ = C


def test_compiler_routes_are_counted_and_a_missing_helper_is_an_error():
    """VERDICT r03 item 3 / `gjx_jit_routes`: every code object says which route produced it.  By default that is the helper
    process (child_compiles grows, inproc_compiles stays 0); a helper that cannot be started is GJX_ERR_JIT — never a
    silent move of the compiler into the caller — unless the caller opts in (GJX_JIT_INPROC_FALLBACK=1).  Each case in a
    process of its own: the helper's path is resolved once per process."""
    import subprocess
    import sys

    child = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
from genjax._amd import abi
from genjax._amd.ops import Ops
ops = Ops(abi.GjxLib(sys.argv[2], "cuda"))
good = b'#include "gjx_device.hpp"\nextern "C" __global__ void k(float* x) { x[threadIdx.x] = gjx::u2f(0x3f800000u); }\n'
bad = b'extern "C" __global__ void k(float* x) { this is not C++ }\n'
r0 = ops.jit_routes()
rc = [ops.lib._gjx_jit_compile_source(good), ops.lib._gjx_jit_compile_source(bad)]
r1 = ops.jit_routes()
print("RESULT", rc, {k: r1[k] - r0[k] for k in r1})
"""
    pkg = os.path.join(ROOT, "genjax-chi_amd")

    def run(**env):
        e = {k: v for k, v in os.environ.items() if not k.startswith("GJX_JIT")}
        e.update(env)
        r = subprocess.run([sys.executable, "-c", child, pkg, HIP_LIB], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT")][0]
        return eval(line[len("RESULT"):].strip().replace("] {", "], {")), r.stderr

    (rc, d), _ = run()
    assert rc == [0, -6] and d == dict(child_compiles=1, inproc_compiles=0, child_failures=1, spawn_failures=0)
    (rc, d), err = run(GJX_JITC="/nonexistent/gjx_jitc")
    assert rc == [-6, -6] and d == dict(child_compiles=0, inproc_compiles=0, child_failures=0, spawn_failures=2)
    assert "could not be started" in err
    (rc, d), err = run(GJX_JITC="/nonexistent/gjx_jitc", GJX_JIT_INPROC_FALLBACK="1")
    assert rc == [0, -6] and d == dict(child_compiles=0, inproc_compiles=1, child_failures=0, spawn_failures=2)
    (rc, d), _ = run(GJX_JIT_INPROC="1")
    assert rc == [0, -6] and d == dict(child_compiles=0, inproc_compiles=1, child_failures=0, spawn_failures=0)


def test_the_helper_leaves_no_files_behind(tmp_path):
    """the compiler's scratch directory is private to the PROCESS (re-created after a fork), its files are named
    per compilation and everything is removed at exit; the helper's environment carries no LD_PRELOAD / profiler variables."""
    import subprocess
    import sys

    child = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
from genjax._amd import abi
lib = abi.GjxLib(sys.argv[2], "cuda")
good = b'#include "gjx_device.hpp"\nextern "C" __global__ void k(float* x) { x[threadIdx.x] = 1.0f; }\n'
assert lib._gjx_jit_compile_source(good) == 0
mine = sorted(os.listdir(os.environ["TMPDIR"]))
pid = os.fork()
if pid == 0:
    ok = lib._gjx_jit_compile_source(good) == 0 and len(os.listdir(os.environ["TMPDIR"])) == len(mine) + 1
    os._exit(0 if ok else 1)
assert os.waitpid(pid, 0)[1] == 0
assert lib._gjx_jit_compile_source(good) == 0
print("DIRS", len(mine))
"""
    e = dict(os.environ, TMPDIR=str(tmp_path), LD_PRELOAD="/nonexistent/libprofiler.so")
    r = subprocess.run([sys.executable, "-c", child, os.path.join(ROOT, "genjax-chi_amd"), HIP_LIB], env=e, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "DIRS 1" in r.stdout, r.stdout + r.stderr
    # the parent's directory is gone at exit; the forked child left through _exit (no destructors): at most its directory stays
    left = [d for d in os.listdir(tmp_path) if d.startswith("gjx_jit_")]
    assert len(left) <= 1, left
    # a preloaded library in the CALLER's environment is not handed to the helper (ld.so would complain on its stderr)
    assert "libprofiler.so" not in r.stderr.split("DIRS")[0] or "gjx_jitc" not in r.stderr
