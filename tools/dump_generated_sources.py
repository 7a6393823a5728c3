#!/usr/bin/env python3
"""One line per generated kernel source of a fixed corpus of plans: kind, model, generator, form, flag bits, length, SHA-256.

A refactor of the generators (gjx_plan_jit.hpp) or of the layer that picks a variant (gjx_hip.hip) runs this at the parent and at
the change and diffs the two outputs: every line must be equal.  No GPU is needed: the library is loaded as tests/offline.py
loads it, plans are host objects, and the models are the builders the CPU tests use, with fixed seeds.

  importance  every model under both generators, GJX_JIT_FORM one / pair / quad and the sixteen combinations of GJX_SOURCE_*
  scan        five plans, both generators, one lane and quad, with and without the fused tail.  Scan plans have no source
              getter: the sources are what gjx_scan_plan_compile_check hands the compiler, recorded by a stand-in for gjx_jitc
              (GJX_JITC) that keeps its input and compiles nothing
  smc ...     plain, guided, parameterised and conditional filters, backward simulation and its MCMC moves, tempered move
              kernels (diagonal, covariance, plated), pointwise kernels, predictive kernels under both generators and PSIS kernels (a plan
              without one: "refused").  (The peer-transport step kernels have no source
              getter and no launch on one device: their text differs from the plain one in the constant kPeers alone.)

--text       also compiles every distinct source with gjx_jitc under the shipped options of its plan kind (compile_options in
             gjx_plan_jit.hpp) and prints the SHA-256 of the code object's .text section (llvm-objcopy -O binary
             --only-section=.text): where a text differs from the parent's, the machine code must not.
--device     on a machine with a GPU: plans with categorical sites are prepared first (gjx_plan_prepare, or a first scan
             launch), so that their sites have the prepared tables and the jcat_invcdf_gb form is emitted; their tables are real
             device tensors.  Only those plans are dumped (the others do not depend on the device).
--match RE   only the lines whose "kind model" matches."""

import argparse
import atexit
import ctypes as C
import hashlib
import os
import re
import shutil
import stat
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "genjax-chi_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from genjax._amd import abi, prng, workloads as W  # noqa: E402
from genjax._amd.abi import GjxLib  # noqa: E402
from genjax._amd.ops import Ops  # noqa: E402
from genjax._amd.runtime import use_ops  # noqa: E402
from offline import DEVICE_HDR, HIP_LIB, JITC, OPTIONS, importance_source, llvm_tool  # noqa: E402

FLAGS = tuple(range(0, 0x1000, 0x100))  # include/gjx.h GJX_SOURCE_FUSED_TAIL | _WT_STORES | _FULL_OUTPUTS | _NT_STORES
KIND_OPTIONS = {"importance": ["-fno-slp-vectorize"]}  # compile_options(PlanKind): the kind's own, after the four fixed ones
A = abi.Arg
LINES = []  # (kind, model, generator, form, flags, source)


def scratch_dir(prefix):
    """A temporary directory of this run, removed at exit."""
    d = tempfile.mkdtemp(prefix=prefix)
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def c(v):
    return A(abi.ARG_CONST, 0, 0.0, v, None)


def ref(site, scale=1.0, offset=0.0):
    return A(abi.ARG_SITE, site, scale, offset, None)


def site(dist, a0, a1=None, out_col=-1, obs=None):
    s = abi.Site()
    s.dist, s.observed, s.out_col = dist, 0 if obs is None else 1, out_col
    s.arg[0] = a0
    if a1 is not None:
        s.arg[1] = a1
    if obs is not None:
        s.obs = obs
    return s


class Tables:
    """Logits / lookup tables of categorical sites: an address that is never read (no GPU), or a device tensor (--device)."""

    def __init__(self, device):
        self.device, self.keep, self.rng = device, [], np.random.default_rng(7)

    def __call__(self, n_floats):
        if not self.device:
            self.keep.append(None)
            return 0x7F0000001000 + 0x1000 * len(self.keep)
        self.keep.append(torch.from_numpy(self.rng.standard_normal(n_floats).astype(np.float32)).cuda())
        return self.keep[-1].data_ptr()


# ---- importance ------------------------------------------------------------------------------------------------------------
def importance_models(ops, table):
    """-> [(name, plan, has categorical sites)]"""
    N, G, Bt, Be = abi.DIST_NORMAL, abi.DIST_GAMMA, abi.DIST_BETA, abi.DIST_BERNOULLI
    nan, inf = float("nan"), float("inf")
    keep = []
    out = [("gaussian10", W.gaussian10_sites(W.gaussian10_data()), {}), ("gaussian10_fast", W.gaussian10_sites(W.gaussian10_data()), dict(fast_math=True)),
           ("beta_bernoulli_obs", W.beta_bernoulli_sites(True), {}), ("beta_bernoulli", W.beta_bernoulli_sites(False), {}),
           ("gamma_normal", W.gamma_normal_sites(), {})]
    # tests/test_plan_specialization.py: test_mixed_plan_compiles, test_plans_with_invalid_constants_compile
    mixed = [site(Bt, c(2.0), c(2.0), 0), site(Be, ref(0), None, -1, c(1.0)), site(G, c(0.7), ref(0, 2.0, 0.5), 1)]
    for mode in (0, 1):
        k = site(abi.DIST_CATEGORICAL, ref(1), None, 2 + mode)
        k.n_cat, k.n_rows, k.cat_mode, k.logits = 3, 2, mode, table(6)
        mixed.append(k)
    mixed += [site(N, A(abi.ARG_TABLE, 3, 0, 0, table(3)), A(abi.ARG_INPUT, 0, 1.0, 0.1, None), 4),
              site(N, ref(5, 0.5, 1.0), c(2.0), -1, A(abi.ARG_INPUT, 1, 0, 0, None))]
    out.append(("mixed", mixed, {}))
    neg = abi.expr_arg([(abi.EXPR_CONST, 0, 1.0), (abi.EXPR_CONST, 0, 3.0), (abi.EXPR_SUB, 0, 0.0)], keep)
    zero_by_zero = abi.expr_arg([(abi.EXPR_CONST, 0, 0.0), (abi.EXPR_CONST, 0, 0.0), (abi.EXPR_DIV, 0, 0.0)], keep)
    invalid = [
        [site(N, c(0.0), c(1.0), 0), site(N, c(0.0), c(1.0), obs=c(inf))],
        [site(N, c(0.0), c(1.0), 0), site(G, c(2.0), c(1.5), obs=c(-0.5))],
        [site(N, c(0.0), c(1.0), 0), site(N, ref(0), c(0.0), obs=c(0.3))],
        [site(N, c(nan), c(-1.0), 0), site(Bt, c(-2.0), c(inf), 1), site(Be, c(1.5), None, 2), site(N, ref(1), c(1.0), obs=c(nan))],
        [site(G, c(0.0), c(0.0), 0), site(N, c(1.0e38), c(1.0e-38), obs=c(-3.0e38))],
        [site(N, c(0.0), c(1.0), 0), site(N, ref(0), neg, obs=A(abi.ARG_INPUT, 0, 1.0, 0.0, None)), site(N, zero_by_zero, c(1.0), obs=c(0.2)),
         site(G, neg, neg, 1)]]
    out += [(f"invalid{i}", s, {}) for i, s in enumerate(invalid)]
    # tests/test_row_cuts_cpu.py: the models of the three rule tests
    obs_at = lambda loc: site(N, loc, c(0.5), obs=c(0.7))  # noqa: E731
    cuts = [[site(N, c(0.0), c(1.0), 0), obs_at(ref(0))], [site(N, c(-0.0), c(1.0), 0), obs_at(ref(0))], [site(N, c(0.0), c(2.0), 0), obs_at(ref(0))],
            [site(N, c(0.0), c(1.0), 0), site(N, ref(0), c(1.0), 1), obs_at(ref(1))]]
    cuts += [[site(N, c(0.0), c(1.0), 0), obs_at(a)] for a in (ref(0, 2.0, 0.0), ref(0, 1.0, -0.0), ref(0, 1.0, 0.25))]
    cuts += [[site(G, c(2.0), c(2.0), 0), site(N, c(0.0), c(1.0), 1), obs_at(ref(1))],
             [site(G, c(2.0), c(2.0), 0), site(N, c(0.5), ref(0, 1.0, 0.1), obs=c(0.7)), site(N, c(0.25), c(0.5), obs=c(0.1))],
             [site(N, c(0.25), c(0.3), 0), site(N, c(0.0), c(1.0), 1), obs_at(ref(1))]]
    out += [(f"row_cuts{i}", s, {}) for i, s in enumerate(cuts)]
    # nested `@gen` calls: a callee with a Normal and a Gamma site between two sites of the caller; a call inside a call
    nested = [site(N, c(0.0), c(1.0), 0), site(N, ref(0), c(0.5), 1), site(G, c(2.0), c(1.5), 2), site(Be, c(0.3), None, 3),
              site(N, ref(1), c(0.5), obs=c(0.7))]
    out.append(("nested", nested, dict(scopes=[(0, 1, 4), (1, 2, 3)])))
    # postfix programs (GJX_ARG_EXPR) over a site, an input column and literals; launch parameters (GJX_ARG_PARAM)
    prog = abi.expr_arg([(abi.EXPR_SITE, 0, 0.0), (abi.EXPR_CONST, 0, 2.0), (abi.EXPR_MUL, 0, 0.0), (abi.EXPR_INPUT, 0, 0.0), (abi.EXPR_ADD, 0, 0.0)], keep)
    scale = abi.expr_arg([(abi.EXPR_SITE, 0, 0.0), (abi.EXPR_ABS, 0, 0.0), (abi.EXPR_CONST, 0, 0.5), (abi.EXPR_MAX, 0, 0.0)], keep)
    out.append(("expr", [site(N, c(0.0), c(1.0), 0), site(N, prog, scale, 1), site(N, ref(1), neg, obs=c(0.2))], {}))
    out.append(("param", [site(N, A(abi.ARG_PARAM, 0, 1.0, 0.0, None), c(1.0), 0), site(G, c(2.0), A(abi.ARG_PARAM, 1, 0.5, 0.1, None), 1),
                          site(N, ref(0), A(abi.ARG_PARAM, 2, 1.0, 0.0, None), obs=A(abi.ARG_PARAM, 3, 1.0, 0.0, None))], {}))
    has_cat = lambda sites: any(s.dist == abi.DIST_CATEGORICAL for s in sites)  # noqa: E731
    return [(name, ops.plan_create(sites, **kw), has_cat(sites)) for name, sites, kw in out], keep


def lazy_keys(ops, impl, n):
    return ops._keys(W.importance_particle_keys(prng.key(3, impl), n), n)


def dump_importance(ops, args, table):
    models, _keep = importance_models(ops, table)
    for name, plan, has_cat in models:
        if args.device:
            if not has_cat:
                continue
            ops.lib.call("gjx_plan_prepare", plan.handle, C.byref(lazy_keys(ops, 1, 1024)))
        for impl in (0, 1):
            for form in ("one", "pair", "quad"):
                os.environ["GJX_JIT_FORM"] = form
                for flags in FLAGS:
                    LINES.append(("importance", name, impl, form, flags, importance_source(ops, plan, impl | flags)))
    os.environ.pop("GJX_JIT_FORM", None)


# ---- scan ------------------------------------------------------------------------------------------------------------------
class Recorder:
    """A stand-in for gjx_jitc (GJX_JITC, resolved once per process: set before the first compilation): keeps every source it
    is handed, in order, and — while GJX_DUMP_STUB is set — answers with a one-line file instead of a code object, which is
    all a compile check asks for.  Without GJX_DUMP_STUB it runs the real helper (--device: launches need real kernels)."""

    def __init__(self):
        self.dir = scratch_dir("gjx_dump_")
        path = os.path.join(self.dir, "jitc.sh")
        with open(path, "w") as f:
            f.write('#!/bin/sh\nn=$(ls "$GJX_DUMP_DIR" | wc -l)\ncp "$1" "$GJX_DUMP_DIR/$(printf %06d "$n").hip"\n'
                    f'if [ -n "$GJX_DUMP_STUB" ]; then echo stub > "$3"; exit 0; fi\nexec "{JITC}" "$@"\n')
        os.chmod(path, os.stat(path).st_mode | stat.S_IXUSR)
        os.environ["GJX_JITC"] = path
        os.environ["GJX_DUMP_DIR"] = os.path.join(self.dir, "src")
        os.mkdir(os.environ["GJX_DUMP_DIR"])

    def take(self):
        """-> the sources recorded since the last call, in order."""
        d = os.environ["GJX_DUMP_DIR"]
        out = []
        for name in sorted(os.listdir(d)):
            with open(os.path.join(d, name)) as f:
                out.append(f.read())
            os.unlink(os.path.join(d, name))
        return out


def scan_plans(ops, table):
    """tests/test_plan_specialization.py: test_scan_plans_compile (tests/test_gpu_parity_abi.py _scan_plans) and
    test_hmm_scan_plan_compiles -> [(name, plan, n_obs, value dtypes, has categorical sites)]"""
    N, G, Bt, Be = abi.DIST_NORMAL, abi.DIST_GAMMA, abi.DIST_BETA, abi.DIST_BERNOULLI
    st = lambda k, s, o: A(abi.ARG_STATE, k, s, o, None)  # noqa: E731
    ob = lambda k: A(abi.ARG_OBS, k, 1.0, 0.0, None)  # noqa: E731
    sites, nxt = W.lgssm_scan_sites()
    rich = [site(N, st(0, 0.8, 0.0), ob(2), 0), site(G, c(0.6), st(1, 1.0, 1.0), 1), site(Be, c(0.3), None, 2), site(Bt, c(2.0), ref(2, 1.5, 0.5), 3),
            site(N, ref(0), ref(3, 1.0, 0.2), -1, ob(0)), site(Be, ref(3), None, -1, ob(1))]
    out = [("lgssm", ops.scan_plan_create(sites, nxt, 1), 1, [torch.float32], False),
           ("rich", ops.scan_plan_create(rich, [ref(0), ref(1, 0.5, 0.1)], 3), 3, [torch.float32, torch.float32, torch.int32, torch.float32], False),
           ("lgssm_fast", ops.scan_plan_create(sites, nxt, 1, fast_math=True), 1, [torch.float32], False)]
    for mode in (0, 1):
        z = site(abi.DIST_CATEGORICAL, st(0, 1.0, 0.0), None, 0)
        z.n_cat, z.n_rows, z.cat_mode, z.logits = 16, 16, mode, table(256)
        y = site(abi.DIST_CATEGORICAL, ref(0), None, -1, ob(0))
        y.n_cat, y.n_rows, y.cat_mode, y.logits = 16, 16, mode, table(256)
        out.append((f"hmm{mode}", ops.scan_plan_create([z, y], [ref(0)], 1), 1, [torch.int32], True))
    return out


def dump_scan(ops, args, table, rec):
    for name, plan, n_obs, dtypes, has_cat in scan_plans(ops, table):
        if args.device:
            if not has_cat:
                continue
            os.environ.pop("GJX_DUMP_STUB", None)  # a first launch: the sites get their prepared tables
            n, T = 512, 2
            ops.scan_run(plan, W.importance_particle_keys(prng.key(3, 1), n), n, T, np.ones((T, n_obs), dtype=np.float32), [0.0] * plan.n_state, dtypes)
            torch.cuda.synchronize()
            rec.take()
        os.environ["GJX_DUMP_STUB"] = "1"
        for impl in (0, 1):
            for flags in (0, 0x100):
                assert plan.compile_check(impl | flags) == 0
                srcs = rec.take()  # PHILOX: the quad form first, then one particle per lane
                assert len(srcs) == 1 + impl, (name, impl, len(srcs))
                for form, src in zip(("quad", "one") if impl else ("one",), srcs):
                    LINES.append(("scan", name, impl, form, flags, src))
    os.environ.pop("GJX_DUMP_STUB", None)


# ---- the plan kinds a change of the importance and scan kernels must not move ------------------------------------------------
def dump_filters(ops):
    import backsim_ref as B
    import guided_ref as G
    import smc_params_ref as SP
    import ssm_fuzz as S
    from genjax._amd.plan import PlanUnsupported
    from genjax._amd.smc_plan import build_guided_plan, build_smc_plan, build_transition_table
    from genjax.inference.smc import StateSpaceModel

    Y = [("y",)]

    def both(kind, name, get):
        for impl in (0, 1):
            try:
                LINES.append((kind, name, impl, "-", 0, get(impl)))
            except (abi.GjxError, PlanUnsupported) as e:
                LINES.append((kind, name, impl, "-", 0, f"refused: {type(e).__name__}"))

    def filter_sources(name, plan):
        both("smc", name, plan.source)
        both("csmc", name, plan.csmc_source)

    # (the HMM's categorical tables are tensors of the lowering backend's device: its transition table is lowered on the oracle
    # — compile-only, the tables are never read — and its filter plan, which would need them on a GPU, is left out)
    oracle = Ops(GjxLib(os.path.join(ROOT, "oracle", "libgjx_oracle.so"), "cpu"))
    with use_ops(oracle):
        hmm = build_transition_table(StateSpaceModel(*B.hmm_model(*B.hmm_tables(8))), [("x",)])
    with use_ops(ops):
        for name in ("lgssm", "two_component", "gamma", "hmm", "increment", "track"):
            addrs = [("u",), ("d",)] if name == "increment" else Y
            model = None if name == "hmm" else StateSpaceModel(*getattr(B, name + "_model")())
            if model is not None:
                filter_sources("B." + name, build_smc_plan(model, addrs)[0])
            try:
                t = ops.backsim_plan_create(hmm if model is None else build_transition_table(model, addrs))
            except PlanUnsupported as e:
                LINES.append(("backsim", "B." + name, "-", "-", 0, f"refused: {type(e).__name__}"))
                continue
            both("backsim", "B." + name, t.source)
            both("backmove", "B." + name, t.move_source)
        r = 0.05
        tq, sq, _ = G.lgssm_optimal(r)
        guided = {"lgssm": (*G.lgssm_model(r), tq, sq), "lgssm_noinit": (*G.lgssm_model(r), tq, None), "two_latent": G.two_latent_model(),
                  "gamma_scale": G.gamma_scale_model(), "mixed": (*G.mixed_model(), None)}
        for name, (init, step, track_q, start_q) in guided.items():
            filter_sources("guided.G." + name, build_guided_plan(StateSpaceModel(init, step), Y, track_q, start_q)[0])
        for name, (model, _literal, rows) in SP.MODELS.items():
            filter_sources("params." + name, build_smc_plan(model(), Y, rows(1)[0])[0])
        for params in (False, True):
            rng = np.random.default_rng(41 if params else 31)
            for i in range(20):
                src = S.random_ssm(rng, flat=i % 2 == 1, params=params)
                name = f"fuzz{'_params' if params else ''}{i}"
                try:
                    plan = build_smc_plan(S.build_model(*src[:2], params=params), [(n_,) for n_, _ in src[2]["obs"]], S.random_theta(rng) if params else None)[0]
                except PlanUnsupported as e:
                    LINES.append(("smc", name, "-", "-", 0, f"refused: {type(e).__name__}"))
                    continue
                filter_sources(name, plan)


def dump_tempered(ops):
    import plate_ref as P
    import temper_cov_ref as V
    import temper_fuzz as F
    import temper_ref as R
    from genjax._amd import temper
    from genjax._amd.plan import PlanUnsupported

    def sources(name, target):
        try:
            tracer = temper.lower(target, 64)
        except PlanUnsupported as e:
            LINES.append(("temper", name, "-", "-", 0, f"refused: {type(e).__name__}"))
            return
        plan = ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
        for impl in (0, 1):
            LINES.append(("temper", name, impl, "-", 0, plan.source(impl)))
            LINES.append(("temper_cov", name, impl, "-", 0, plan.cov_source(impl)))
        for kind, impl, get in (("pointwise", "-", plan.pointwise_source), ("predictive", 0, lambda: plan.predictive_source(0)),
                                ("predictive", 1, lambda: plan.predictive_source(1)), ("psis", "-", plan.psis_source)):
            try:
                LINES.append((kind, name, impl, "-", 0, get()))
            except abi.GjxError as e:
                LINES.append((kind, name, impl, "-", 0, f"refused: {type(e).__name__}"))

    with use_ops(ops):
        targets = dict(R.models())
        targets.update(correlated=V.correlated_target(), correlated_plated=V.correlated_target(plated=True), gaussian16=V.gaussian_chain_target(16))
        targets.update({"plate." + name: P.target(name, 20, 0)[0] for name in P.MODELS})
        xs, zs, y1, y2 = P.two_plate_data(20, 0)
        targets["two_plate"] = F.target_of(P.TWO_PLATE, (xs, zs), {"y1": y1, "y2": y2})
        targets["interleaved"] = F.target_of(F.INTERLEAVED, *F.head_rows(*F.interleaved_inputs(), 9))
        rng = np.random.default_rng(11)
        for i in range(20):
            src, sites = F.random_tempered_model(rng)
            a, obs = F.random_inputs(rng, sites, (2, 5, 9)[i % 3])
            targets[f"fuzz{i}"] = F.target_of(src, a, obs)
        for name, t in targets.items():
            sources(name, t)


# ---- output ----------------------------------------------------------------------------------------------------------------
def text_sha(kind, src, tmp, serial):
    """The SHA-256 of the .text section of `src` compiled by gjx_jitc under the shipped options of its plan kind."""
    stem = os.path.join(tmp, f"t{serial}")
    with open(stem + ".hip", "w") as f:
        f.write(src)
    r = subprocess.run([JITC, stem + ".hip", DEVICE_HDR, stem + ".co", stem + ".log", *OPTIONS, *KIND_OPTIONS.get(kind, [])], capture_output=True, text=True)
    if r.returncode != 0:
        return "compile-failed"
    subprocess.run([llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.text", stem + ".co", stem + ".bin"], check=True)
    with open(stem + ".bin", "rb") as f:
        h = hashlib.sha256(f.read()).hexdigest()
    for ext in (".hip", ".co", ".log", ".bin"):
        if os.path.exists(stem + ext):
            os.unlink(stem + ext)
    return h


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--text", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--match", default="")
    ap.add_argument("--sources", default="", help="a directory that receives every distinct source as <sha256>.hip")
    args = ap.parse_args()
    missing = [f for f in (HIP_LIB, JITC, os.path.join(ROOT, "oracle", "libgjx_oracle.so")) if not os.path.exists(f)]
    if missing:
        sys.exit("dump_generated_sources.py: not built yet (python __graft_entry__.py builds them): " + ", ".join(missing))
    rec = Recorder()
    ops = Ops(GjxLib(HIP_LIB, "cuda"))  # (without --device no compute call is made: plans are host objects)
    table = Tables(args.device)
    dump_importance(ops, args, table)
    dump_scan(ops, args, table, rec)
    if not args.device:
        dump_filters(ops)
        dump_tempered(ops)
    lines = [ln for ln in LINES if re.search(args.match, f"{ln[0]} {ln[1]}")]
    text = {}
    if args.text:
        todo = sorted({(ln[0], ln[5]) for ln in lines if not ln[5].startswith("refused")})
        tmp = scratch_dir("gjx_text_")
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            text = dict(zip(todo, pool.map(lambda a: text_sha(a[1][0], a[1][1], tmp, a[0]), enumerate(todo))))
    if args.sources:
        os.makedirs(args.sources, exist_ok=True)
    for kind, model, impl, form, flags, src in lines:
        if src.startswith("refused"):
            print(kind, model, impl, form, f"{flags:#x}", src)
            continue
        sha = hashlib.sha256(src.encode()).hexdigest()
        if args.sources:
            with open(os.path.join(args.sources, sha + ".hip"), "w") as f:
                f.write(src)
        print(kind, model, impl, form, f"{flags:#x}", len(src), sha, *(["text=" + text[(kind, src)]] if args.text else []))


if __name__ == "__main__":
    main()
