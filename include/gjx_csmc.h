/*
 * gjx_csmc.h — the conditional particle filter: one retained path kept alive inside the one-launch SMC step.
 *
 * One more header next to gjx.h, in the pattern of gjx_guided.h: a version of its own, exported by libgjx_hip.so and not
 * by the oracle library (gjx.h is the boundary the CPU oracle restates symbol for symbol); a binding loads it if
 * present.  Conventions are those of gjx.h.
 *
 * gjx_smc_plan_step_conditional is gjx_smc_plan_step with slot n_total - 1 RETAINED.  With x*[t][k] =
 * retained->path[k][t]:
 *
 *   t == 0   Every slot is initialised as gjx_smc_plan_step initialises it: same slot keys, same draw numbers, same
 *            bits.  In slot n - 1 every sampled site (latent or PROPOSED) takes x*[0][k], k the carry component the site
 *            is, as its VALUE.  The draw is still consumed — nothing is renumbered — and every log-density that reads
 *            the value is evaluated at the retained one: observed sites, lq of a PROPOSED site, lp of its GUIDED partner.
 *   t >= 1   Slots 0 .. n - 2 are served by the systematic comb of gjx.h with n_out = n - 1 teeth over all n source
 *            particles: the same u0 from resample_keys[t], the same tile records, the same float64 arithmetic.  Slot
 *            n - 1 has ancestor n - 1 and, as at t == 0, state x*[t].  With no mass at all slot j < n - 1 takes particle
 *            floor(j n / (n - 1)); the retained slot stays forced.
 *   Slot j's keys are those of the unconditional step for every j, n - 1 included.  The emitted tile records,
 *   sub-prefixes and (e, q) are those of all n log-weights; the log Z estimator is the unconditional one over n particles.
 *
 * The model condition: the retained values must determine the step.  In both bodies every sampled site is, by itself,
 * exactly one carry component (next_state[k] = {GJX_ARG_SITE, s, 1, 0}) and every carry component is such a site.  An
 * integer-valued site takes the retained f32 value rounded to nearest, as a state column is read everywhere else (clamped
 * to +-2^30 first, a NaN to -2^30: a value that is no category of the site is outside its support, log-density -inf).
 *
 * The conditional kernels are generated (a source of their own, next to the plan's unconditional kernels, which do not
 * change); with specialisation switched off (GJX_PLAN_JIT=0) the step returns GJX_ERR_UNSUPPORTED.
 * Out of scope: ESS-adaptive, batched, sharded and peer-distributed conditional filters, bodies with nested calls.
 */
#ifndef GJX_CSMC_H
#define GJX_CSMC_H

#include "gjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_CSMC_VERSION_MAJOR 0
#define GJX_CSMC_VERSION_MINOR 1

typedef struct {
  const float* path[GJX_SMC_MAX_STATE]; /* dev f32[T] per state component */
} gjx_csmc_path;

int gjx_csmc_version(int* major, int* minor);
/* gjx_smc_plan_step with slot n_total-1 retained: reads path[k][t].
 * GJX_ERR_INVALID: whatever gjx_smc_plan_step refuses; n_total < 2; `retained` or one of its first n_state components
 * NULL; a plan that breaks the model condition.
 * GJX_ERR_UNSUPPORTED: n_filters > 1; ess_threshold in (0, 1); peers; a sharded config (first_slot != 0 or
 * n_local != n_total); a plan with nested calls; GJX_PLAN_JIT=0. */
int gjx_smc_plan_step_conditional(const gjx_smc_config* cfg, gjx_smc_plan* plan, int t, const float* obs_t,
                                  const gjx_smc_pop* prev, const gjx_smc_pop* out, int32_t* prev_e_out, uint64_t* prev_q_out,
                                  int32_t* ancestors_out, const gjx_csmc_path* retained, gjx_stream s);
/* The HIP source of the plan's CONDITIONAL kernels (gjx_smc_step_kernel_conditional, gjx_smc_init_kernel_conditional),
 * as gjx_smc_plan_source returns that of the unconditional ones.  GJX_ERR_INVALID / GJX_ERR_UNSUPPORTED for a plan the
 * step refuses. */
int gjx_csmc_plan_source(const gjx_smc_plan* p, int impl, char* buf, size_t buf_len, size_t* needed);
int gjx_csmc_plan_compile_check(const gjx_smc_plan* p, int impl); /* offline, needs no GPU */

#ifdef __cplusplus
}
#endif
#endif /* GJX_CSMC_H */
