"""The reference the MCMC backward sampler (include/gjx_backmove.h) is held to, built from UNCHANGED oracle entry points
(the oracle knows no gjx_backmove.h).  Everything is O(m K T): no candidate loop over n.

  * keys: prng.fold_in on the host — k_t = fold_in(key, t), p_t = fold_in(k_t, 0), a_t = fold_in(k_t, 1);
  * leaves and proposals: the oracle's gjx_resample_multinomial under the LITERAL key p_t, n_out = m (leaves) or m K;
  * uniforms: the oracle's gjx_rng_bits over the lazy children of a_t, uniform01 restated in numpy, and the spec's
    logarithm as the oracle's gjx_logpdf_bernoulli(value 1, probs u);
  * the transition sum s for all m (candidate, next state) pairs of one move is the LOG-WEIGHT COLUMN of ONE run of an
    oracle importance plan: backsim_ref.transition_importance_plan's construction, with GJX_ARG_NEXT mapped to input
    columns D .. 2 D - 1 instead of launch parameters (the observation row stays a parameter);
  * the accept test and the select are numpy f32."""

import numpy as np
import torch

import backsim_ref as B
from genjax._amd import abi, prng
from genjax._amd.ops import KeyBatch


def _pair_arg(table, a, keep):
    """An argument of a transition table for the PAIR plan: the state is input column k, next-state component c input column
    D + c, observation k parameter k."""
    D = table.n_state
    if a.kind == abi.ARG_STATE:
        return abi.Arg(abi.ARG_INPUT, a.ref, a.scale, a.offset, None)
    if a.kind == abi.ARG_NEXT:
        return abi.Arg(abi.ARG_INPUT, D + a.ref, a.scale, a.offset, None)
    if a.kind == abi.ARG_OBS:
        return abi.Arg(abi.ARG_PARAM, a.ref, a.scale, a.offset, None)
    if a.kind == abi.ARG_EXPR:
        ops = (abi.ExprOp * a.ref).from_address(a.table)
        swap = {abi.EXPR_STATE: abi.EXPR_INPUT, abi.EXPR_OBS: abi.EXPR_PARAM}
        prog = [(swap.get(o.op, o.op), o.ref, o.value) for o in ops]
        return abi.expr_arg(prog, keep)
    return abi.Arg(a.kind, a.ref, a.scale, a.offset, a.table)


def pair_plan(oracle_ops, table):
    """-> the oracle importance plan whose log-weight column, run over m rows, is s for m (state, next state) pairs."""
    keep, sites = [], []
    for s in table.sites:
        c = abi.Site.from_buffer_copy(s)
        c.arg[0], c.arg[1], c.obs = (_pair_arg(table, a, keep) for a in (s.arg[0], s.arg[1], s.obs))
        c.observed, c.out_col = 1, -1
        sites.append(c)
    plan = oracle_ops.plan_create(sites)
    plan._keep = (keep, table)
    return plan


def uniform01(bits):
    """gjx.h uniform01 of int32 / uint32 words, in numpy."""
    w = np.asarray(bits).view(np.uint32)
    return ((w >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)


class Scorer:
    def __init__(self, oracle_ops, table, impl):
        self.ops, self.plan, self.impl = oracle_ops, pair_plan(oracle_ops, table), impl

    def __call__(self, state_cols, next_cols, obs_row):
        """s over rows: `state_cols`, `next_cols` lists of D float32 [m] tensors."""
        m = state_cols[0].numel()
        if obs_row is not None:
            self.plan.set_params(np.asarray(obs_row, dtype=np.float32))
        kb = prng.split_lazy(prng.key(0, self.impl), m)  # (the plan has no latent site: no draw is made)
        ins = [c.contiguous() for c in state_cols + next_cols]
        return self.ops.importance_run(self.plan, kb, m, ins, [], want_score=False, want_max_partials=False)[2].numpy().copy()


def backmove_ref(oracle_ops, table, key, cols, lw, anc, obs, m, n_moves, stats=None):
    """The specification of include/gjx_backmove.h from oracle pieces.  `cols`: CPU [T, n] tensors (float32, or int32 for the
    fixed HMM's states), `lw` f32[T, n], `anc` int32[T, n], `obs` [T, n_obs] or None.
    -> (lineage int32[T, m], [path columns [T, m]]).  `stats` (a dict): accepted moves are counted into stats["accepted"]."""
    T, n = lw.shape
    K = int(n_moves)
    cols = [c.detach().cpu() for c in cols]
    fcols = [c.to(torch.float32) for c in cols]  # (the kernel reads an int32 column as (float) value)
    lw = lw.detach().cpu().to(torch.float32)
    anc = anc.detach().cpu()
    obs = None if obs is None else np.asarray(obs, dtype=np.float32).reshape(T, -1)
    score = Scorer(oracle_ops, table, key.impl) if (T > 1 and K > 0) else None
    lineage = torch.empty((T, m), dtype=torch.int32)
    accepted = 0
    for t in range(T - 1, -1, -1):
        kt = prng.fold_in(key, t)
        pt, at = prng.fold_in(kt, 0), prng.fold_in(kt, 1)
        if t == T - 1:
            lineage[t] = oracle_ops.resample("multinomial", pt.literal(), lw[t].contiguous(), m)[0]
            continue
        nxt = lineage[t + 1].long()
        cur = torch.clamp(anc[t + 1][nxt].long() & 0xFFFFFFFF, max=n - 1)  # min((uint32) word, n - 1)
        if K > 0:
            nx = [c[t + 1][nxt] for c in fcols]
            row = None if obs is None else obs[t + 1]
            props = oracle_ops.resample("multinomial", pt.literal(), lw[t].contiguous(), m * K)[0].long().view(K, m)
            bits = oracle_ops.rng_bits(KeyBatch(key.impl, 1, parent=(at.k0, at.k1), first=0, parent_lane=at.lane), m * K, 0)
            u = torch.from_numpy(uniform01(bits.numpy()).copy())
            logu = oracle_ops.logpdf("bernoulli", m * K, 1, u).numpy().reshape(K, m)
            s_cur = score([c[t][cur] for c in fcols], nx, row)
            for r in range(K):
                s_new = score([c[t][props[r]] for c in fcols], nx, row)
                with np.errstate(invalid="ignore"):
                    d = (s_new - s_cur).astype(np.float32)  # f32 - f32: one rounding
                    acc = (d >= np.float32(0.0)) | (logu[r] < d)  # both False on NaN
                accepted += int(acc.sum())
                acc_t = torch.from_numpy(acc)
                cur = torch.where(acc_t, props[r], cur)
                s_cur = np.where(acc, s_new, s_cur)
        lineage[t] = cur.to(torch.int32)
    if stats is not None:
        stats["accepted"] = accepted
    idx = lineage.long()
    return lineage, [torch.gather(c, 1, idx) for c in cols]


def trace_back(anc, leaves):
    """numpy trace-back of `leaves` through `anc` int32[T, n] -> lineage int32[T, m]."""
    T = anc.shape[0]
    lin = torch.empty((T, leaves.numel()), dtype=torch.int32)
    lin[T - 1] = leaves
    for t in range(T - 2, -1, -1):
        lin[t] = anc[t + 1][lin[t + 1].long()]
    return lin
