/*
 * gjx_backsim.h — backward-simulation smoothing over a recorded particle-filter history.
 *
 * A FOURTH header next to gjx.h (after gjx_paths.h and gjx_guided.h), with a version of its own and for the same
 * reason: gjx.h is the boundary the CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points,
 * the oracle library does not, and a binding loads them if present.  Conventions (status codes, gjx_stream, borrowed
 * "dev" pointers, no allocation, no host synchronisation) are those of gjx.h.
 *
 * Trace-back (gjx_paths.h) follows the filter's genealogy, and the genealogy collapses: early steps rest on a few
 * thousand distinct particles however many the filter ran.  Backward simulation draws every trajectory afresh from the
 * recorded populations: for m trajectories, from the last step to the first,
 *
 *   idx[T-1][j] ~ Categorical(lw[T-1][.])
 *   idx[t][j]   ~ Categorical(lw[t][i] + log f(x_{t+1} = col[t+1][idx[t+1][j]] | x_t = col[t][i]))      t = T-2 .. 0
 *
 * over ALL n particles of step t: n m (T - 1) transition densities and Gumbels, none of them materialised.  Ancestors
 * are not read.
 *
 * Specification (exact: the result is a function of the inputs and the key alone, bit for bit).  Inputs: state columns
 * col_c[T, n] (4-byte elements), log-weights lw[T, n] (the row each filter step wrote), observation rows obs[T, n_obs],
 * the model's TRANSITION TABLE (below), a key.
 *
 *   keys    k_t = fold_in(key, t).  Trajectory j at step t draws under split(k_t, m)[j] — the lazy gjx_keys {mode 1,
 *           parent k_t, first j, no fold} — and candidate i reads what gjx_categorical_index (mode 0) reads for logit i
 *           under that key: word 0 of sub-stream i (gjx.h "streams").  Under PHILOX all trajectories of a step share one
 *           cipher key (the lane carries j + 1), so the round keys are wave-uniform.
 *   logits  logit_t^j[i] = lw[t][i] + s, s = the f32 sum, from +0 and in table order, of the log-densities of the
 *           table's sites (one rounding per add, never contracted: what an importance plan's weight accumulates), with
 *           GJX_ARG_STATE k = col_k[t][i], GJX_ARG_NEXT c = col_c[t+1][idx[t+1][j]], GJX_ARG_OBS k = obs[t+1][k].
 *           For t = T-1 there are no terms: the logit is lw[T-1][i] itself.
 *   draw    idx[t][j] = gjx_categorical_index(mode 0) of those n logits: v = logit + gumbel, `v > best || i == 0`
 *           scanning i upwards — the first maximiser; a NaN at i > 0 never wins, a NaN at i = 0 always wins, all -inf
 *           gives 0.  Always in [0, n).
 *   result  lineage[t][j] = idx[t][j];  path_c[t][j] = col_c[t][idx[t][j]], copied as 32 bits.
 *
 * A maximum is exact and order-free: the result does not depend on how candidates are tiled over lanes, waves and
 * workgroups, nor on max_workgroups.
 *
 * The transition table is a gjx_site table in which EVERY site has observed == 1:
 *   - a latent site of the model's step becomes a site whose `obs` is {GJX_ARG_NEXT, ref = carry component c, 1, 0}: its
 *     value is component c of the trajectory's state at t + 1 (integer-valued sites round it, as observed sites do);
 *   - an observed site of the step keeps `obs` = {GJX_ARG_OBS, k} (or a constant);
 *   - arguments are those of an SMC step table (GJX_ARG_CONST / SITE / TABLE / STATE / OBS / EXPR).
 * GJX_ARG_NEXT is valid in `obs` of the tables given to gjx_backsim_plan_create only: every creator of gjx.h and
 * gjx_guided.h returns GJX_ERR_INVALID for it.
 */
#ifndef GJX_BACKSIM_H
#define GJX_BACKSIM_H

#include "gjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_BACKSIM_VERSION_MAJOR 0
#define GJX_BACKSIM_VERSION_MINOR 1

#define GJX_ARG_NEXT 8 /* gjx_arg.kind, in gjx_site.obs of a transition table: next-state component `ref` */

typedef struct gjx_backsim_plan gjx_backsim_plan;

typedef struct {
  int32_t n_steps; /* T >= 1 */
  int32_t impl;    /* GJX_RNG_THREEFRY / GJX_RNG_PHILOX */
  uint64_t n;      /* particles per step, 1 .. 2^31 - 1 */
  uint64_t m;      /* trajectories,       1 .. 2^31 - 1 */
  uint32_t key[2]; /* the user key ... */
  uint64_t key_lane; /* ... and its PHILOX lane (0 for THREEFRY) */
  /* Inputs.  Row t of an array starts t * stride ELEMENTS behind its base; strides >= n and < 2^32 (history rows are
   * padded to whole tiles). */
  const void* cols[GJX_SMC_MAX_STATE]; /* dev [T, col_stride[c]], required for c < the plan's n_state */
  uint64_t col_stride[GJX_SMC_MAX_STATE];
  int32_t col_is_i32[GJX_SMC_MAX_STATE]; /* != 0: the column holds int32 (the fixed HMM's states), read as (float) value */
  const float* logw;                     /* dev f32[T, logw_stride] */
  uint64_t logw_stride;
  const float* obs; /* HOST f32[T, n_obs] (as gjx_smc_run_plan takes them); required when the plan's n_obs > 0 */
  /* Outputs, either nullable but not both.  Row strides >= m and < 2^32. */
  int32_t* lineage_out; /* dev int32[T, lineage_stride] */
  uint64_t lineage_stride;
  void* paths_out[GJX_SMC_MAX_STATE]; /* dev [T, paths_stride[c]], each nullable */
  uint64_t paths_stride[GJX_SMC_MAX_STATE];
  uint32_t max_workgroups; /* 0 = the library chooses; otherwise a cap on every grid.  Results do not depend on it. */
} gjx_backsim_io;

int gjx_backsim_version(int* major, int* minor);
/* GJX_ERR_INVALID: n_sites outside 1 .. GJX_MAX_SITES, n_state outside 1 .. GJX_SMC_MAX_STATE, n_obs outside
 * 0 .. GJX_SMC_MAX_OBS, flags != 0 (none is defined yet), a site with observed != 1 (observed > 1 included), an operand
 * out of range (as gjx_smc_plan_create checks a step table), a GJX_ARG_NEXT with ref outside [0, n_state) or with
 * scale / offset other than 1 / 0.  The table is copied. */
int gjx_backsim_plan_create(const gjx_site* sites, int n_sites, int n_state, int n_obs, uint32_t flags,
                            gjx_backsim_plan** out);
int gjx_backsim_plan_destroy(gjx_backsim_plan* p);
/* The HIP source of the plan's generated kernels for impl 0 / 1, as gjx_smc_plan_source returns a filter's. */
int gjx_backsim_plan_source(const gjx_backsim_plan* p, int impl, char* buf, size_t buf_len, size_t* needed);
/* Compiles that source for gfx950 without touching a GPU: GJX_OK, or GJX_ERR_UNSUPPORTED when it does not compile. */
int gjx_backsim_plan_compile_check(const gjx_backsim_plan* p, int impl);
/* Scratch of a run: one 64-bit word per step and trajectory (the packed running maxima). */
size_t gjx_backsim_workspace_bytes(int32_t n_steps, uint64_t m);
/* ONE call enqueues the whole backward pass on `s`: the workspace is cleared, then one launch per step (T-1 .. 0; a
 * step's launch reads the winners of the step behind it in its prologue) and a last small launch that writes lineage and
 * paths.  No host synchronisation, no allocation.  The kernels are generated from the table and compiled on first use:
 * with the compiler switched off (GJX_PLAN_JIT=0) GJX_ERR_UNSUPPORTED, as guided plans; GJX_ERR_JIT if it fails.
 * GJX_ERR_INVALID (nothing launched): a NULL plan / io / required pointer, T < 1, n or m 0 or >= 2^31, impl not 0 / 1, a
 * lane with THREEFRY, a stride below n (inputs) / m (outputs) or >= 2^32, no output at all, ws not 8-byte aligned.
 * GJX_ERR_WORKSPACE: ws NULL or ws_bytes < gjx_backsim_workspace_bytes(T, m). */
int gjx_backsim_run(gjx_backsim_plan* p, const gjx_backsim_io* io, void* ws, size_t ws_bytes, gjx_stream s);

#ifdef __cplusplus
}
#endif
#endif /* GJX_BACKSIM_H */
