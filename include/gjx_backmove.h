/*
 * gjx_backmove.h — MCMC backward simulation: smoothed paths at the filter's own size.
 *
 * A FIFTH header next to gjx.h (after gjx_paths.h, gjx_guided.h and gjx_backsim.h), with a version of its own and for the
 * same reason: gjx.h is the boundary the CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points,
 * the oracle library does not, and a binding loads them if present.  Conventions (status codes, gjx_stream, borrowed
 * "dev" pointers, no allocation, no host synchronisation) are those of gjx.h.  It works on an existing gjx_backsim_plan
 * (gjx_backsim.h): the same transition table, the same lowering, no plan kind of its own.
 *
 * Exact backward simulation (gjx_backsim.h) redraws every path from all n particles of every step: n m (T - 1) transition
 * densities.  This is the backward sampler of Bunch & Godsill (2013): path j starts step t at the genealogical ancestor
 * of its particle of step t + 1 and makes K Metropolis-Hastings moves whose proposals are drawn from step t's filter
 * weights.  The target of a move is W_t^i f(x_{t+1} | x_t^i) and the proposal is W_t itself, so the acceptance ratio is
 * f(x_{t+1} | proposal) / f(x_{t+1} | current): m K (T - 1) transition densities, whatever n is.  K = 0 is trace-back from
 * multinomial leaves.
 *
 * Specification (exact: the result is a function of the inputs and the key alone, bit for bit).  Inputs: those of
 * gjx_backsim_io — state columns col_c[T, n] (4-byte elements; int32 columns are read as (float) value), log-weights
 * lw[T, n], observation rows obs[T, n_obs], the plan's transition table, a key — plus the filter's ancestor table
 * anc int32[T, n] (anc[t][i] = the parent in step t - 1 of particle i of step t; row 0 is not read) and n_moves = K.
 *
 *   keys      k_t = fold_in(key, t) as in gjx_backsim.h; p_t = fold_in(k_t, 0) the PROPOSAL key, a_t = fold_in(k_t, 1) the
 *             ACCEPTANCE key.  All three are launch-uniform and evaluated on the host.
 *   last step idx[T-1][j] = element j of what gjx_resample_multinomial returns for the literal key p_{T-1} (mode 2, no
 *             fold), logw = lw[T-1], n, n_out = m: the max-anchored fixed-point weights of gjx.h, inclusive CDF C,
 *             Q = C_{n-1}, thr = mulhi64(bits64(j), Q), the first i with C_i > thr (n - 1 if there is none).
 *   step t < T-1, path j
 *     next    x+_c = col_c[t+1][idx[t+1][j]].
 *     s(i)    the transition sum of gjx_backsim.h: the f32 sum, from +0 and in table order, of the log-densities of the
 *             table's sites (one rounding per add, never contracted), with GJX_ARG_STATE k = col_k[t][i], GJX_ARG_NEXT c =
 *             x+_c, GJX_ARG_OBS k = obs[t+1][k].
 *     start   cur = min((uint32) anc[t+1][idx[t+1][j]], n - 1) — no address is formed from an unchecked word;
 *             s_cur = s(cur).
 *     props   prop_r, r = 0 .. K-1 = element r m + j of gjx_resample_multinomial(literal p_t, lw[t], n, n_out = m K).
 *     unifs   w_r = element r m + j of gjx_rng_bits(keys {mode 1, parent a_t, first 0, no fold}, sub 0);
 *             u_r = uniform01(w_r) = f32((w_r >> 9) | 0x3F800000) - 1;  l_r = the spec's logarithm of u_r (what
 *             gjx_logpdf_bernoulli(value 1, probs u_r) returns).
 *     moves   in order of r: d = s(prop_r) - s_cur (one f32 subtraction); ACCEPT iff d >= 0 || l_r < d (both comparisons
 *             are false on NaN); on accept cur = prop_r, s_cur = s(prop_r).
 *     result  idx[t][j] = cur.
 *   output    lineage[t][j] = idx[t][j];  path_c[t][j] = col_c[t][idx[t][j]], copied as 32 bits.
 *
 * lw[t] enters through the proposals only.  Nothing depends on tiling, grid size or max_workgroups.  Corner cases (no mass
 * at all, NaN or -inf weights, u = 0) are whatever the named entry points return.  Under PHILOX both keys have lane 0, so
 * the cipher key of every draw is wave-uniform.
 */
#ifndef GJX_BACKMOVE_H
#define GJX_BACKMOVE_H

#include "gjx_backsim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_BACKMOVE_VERSION_MAJOR 0
#define GJX_BACKMOVE_VERSION_MINOR 1

#define GJX_BACKMOVE_MAX_MOVES 256

typedef struct {
  /* The fields of gjx_backsim_io, in its order and with its meaning (gjx_backsim.h). */
  int32_t n_steps; /* T >= 1 */
  int32_t impl;    /* GJX_RNG_THREEFRY / GJX_RNG_PHILOX */
  uint64_t n;      /* particles per step, 1 .. 2^31 - 1 */
  uint64_t m;      /* paths,              1 .. 2^31 - 1, and m * max(n_moves, 1) < 2^31 */
  uint32_t key[2];
  uint64_t key_lane;
  const void* cols[GJX_SMC_MAX_STATE];
  uint64_t col_stride[GJX_SMC_MAX_STATE];
  int32_t col_is_i32[GJX_SMC_MAX_STATE];
  const float* logw;
  uint64_t logw_stride;
  const float* obs; /* HOST f32[T, n_obs] */
  int32_t* lineage_out; /* dev int32[T, lineage_stride], nullable: the rows then live in the workspace */
  uint64_t lineage_stride;
  void* paths_out[GJX_SMC_MAX_STATE];
  uint64_t paths_stride[GJX_SMC_MAX_STATE];
  uint32_t max_workgroups;
  /* ... plus: */
  const int32_t* ancestors; /* dev int32[T, anc_stride]: the filter's ancestor table (row 0 is not read) */
  uint64_t anc_stride;      /* >= n and < 2^32 */
  int32_t n_moves;          /* K, 0 .. GJX_BACKMOVE_MAX_MOVES */
} gjx_backmove_io;

int gjx_backmove_version(int* major, int* minor);
/* The HIP source of the plan's generated MOVE kernels for impl 0 / 1 (a module of their own: gjx_backsim_plan_source and
 * the kernels behind it are untouched). */
int gjx_backmove_plan_source(const gjx_backsim_plan* p, int impl, char* buf, size_t buf_len, size_t* needed);
/* Compiles that source for gfx950 without touching a GPU: GJX_OK, or GJX_ERR_UNSUPPORTED when it does not compile. */
int gjx_backmove_plan_compile_check(const gjx_backsim_plan* p, int impl);
/* Scratch of a run: one fixed-point CDF of n entries with its tile maxima and masses (reused by every step), and the
 * lineage rows, T m int32, for a call without lineage_out.  0 for arguments outside the ranges above. */
size_t gjx_backmove_workspace_bytes(int32_t n_steps, uint64_t n, uint64_t m);
/* ONE call enqueues the whole backward pass on `s`: per step T-1 .. 0 the CDF of lw[t] (three small launches; skipped
 * where a step draws nothing: t < T-1 with K = 0) and ONE move launch, one lane per path, which writes lineage row t and
 * the path values of step t itself — there is no finish launch, and no array of m K elements exists anywhere.  No host
 * synchronisation, no allocation.  The kernels are generated from the table and compiled on first use: with the compiler
 * switched off (GJX_PLAN_JIT=0) GJX_ERR_UNSUPPORTED, as gjx_backsim_run; GJX_ERR_JIT if it fails.
 * GJX_ERR_INVALID (nothing launched): a NULL plan / io / required pointer (ancestors included), T < 1, n or m
 * 0 or >= 2^31, n_moves outside 0 .. 256, m * max(n_moves, 1) >= 2^31, impl not 0 / 1, a lane with THREEFRY, a stride below
 * n (inputs, anc_stride) / m (outputs) or >= 2^32, no output at all, ws not 8-byte aligned.
 * GJX_ERR_WORKSPACE: ws NULL or ws_bytes < gjx_backmove_workspace_bytes(T, n, m). */
int gjx_backmove_run(gjx_backsim_plan* p, const gjx_backmove_io* io, void* ws, size_t ws_bytes, gjx_stream s);

#ifdef __cplusplus
}
#endif
#endif /* GJX_BACKMOVE_H */
