/*
 * gjx_guided.h — guided particle filters: user proposals inside the one-launch SMC step.
 *
 * A THIRD header next to gjx.h (after gjx_paths.h), with a version of its own and for the same reason: gjx.h is the
 * boundary the CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points, the oracle library
 * does not, and a binding loads them if present.  Conventions are those of gjx.h.
 *
 * A bootstrap filter (gjx_smc_plan_create) draws every latent site of a step from the model's own transition and
 * weights a particle by its observed sites.  A guided filter draws some latent sites from a PROPOSAL q(x_t | x_{t-1},
 * y_t) instead and corrects for it in the weight:
 *
 *   w_t = p(x_t | x_{t-1}) p(y_t | x_t) / q(x_t | x_{t-1}, y_t)
 *
 * gjx_site does not change shape.  gjx_site.observed takes two more values in the tables of a guided plan:
 *
 *   GJX_SITE_PROPOSED (2)  The site is sampled exactly as a latent site (observed == 0): it takes the same draw number
 *                          (THREEFRY: fold_in(slot key, 1-based table position); PHILOX: the 0-based index among the
 *                          sampled sites — latent and proposed ones alike — and so the same quad blocks).  Its
 *                          log-density lq at the drawn value is KEPT and enters nothing at the site's own position.
 *   GJX_SITE_GUIDED   (3)  `obs` is {GJX_ARG_SITE, ref = an EARLIER PROPOSED site of the same table, scale 1, offset 0}.
 *                          The site draws nothing; its value is that site's value (later sites that refer to either see
 *                          the same number).  With lp the site's own log-density at that value, the weight takes
 *                              d = lp - lq;  w = w + d        (f32, one rounding each, never contracted)
 *                          at THIS site's table position.  The difference is formed first, so a proposal that equals the
 *                          model's site cancels exactly (d == +0) for any number of latents.  A value outside the site's
 *                          support gives whatever the spec's log-density gives there, as for an observed value.
 *
 * Every PROPOSED site must be referenced by exactly one GUIDED site, and the two are both integer-valued (Bernoulli,
 * Categorical) or both float-valued.  Latent sites (observed == 0) keep being drawn from the model and contribute
 * nothing to the weight; observed sites contribute as in a bootstrap plan.
 *
 * The result is a plain gjx_smc_plan: gjx_smc_run_plan, gjx_smc_plan_step, filter batches, ESS-adaptive resampling
 * and graph capture apply unchanged.  Guided plans run as generated kernels only: with specialisation switched off
 * (GJX_PLAN_JIT=0) they return GJX_ERR_UNSUPPORTED, as plans with nested calls do.
 *
 * The creators of gjx.h (gjx_plan_create*, gjx_smc_plan_create*, gjx_scan_plan_create*) return GJX_ERR_INVALID for a
 * site with observed > 1.
 */
#ifndef GJX_GUIDED_H
#define GJX_GUIDED_H

#include "gjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_GUIDED_VERSION_MAJOR 0
#define GJX_GUIDED_VERSION_MINOR 1

#define GJX_SITE_PROPOSED 2
#define GJX_SITE_GUIDED 3

int gjx_guided_version(int* major, int* minor);
/* As gjx_smc_plan_create, with the two modes above accepted in both site tables.  GJX_ERR_INVALID: whatever
 * gjx_smc_plan_create refuses; observed outside 0..3; a GUIDED site whose `obs` is not {GJX_ARG_SITE, an earlier
 * PROPOSED site, 1, 0}; a PROPOSED site referenced by no GUIDED site or by more than one; an integer-valued site paired
 * with a float-valued one.  Destroy with gjx_smc_plan_destroy. */
int gjx_smc_plan_create_guided(const gjx_smc_model* m, gjx_smc_plan** out);
/* The HIP source of the plan's generated kernels (step policy, adaptive step, init) for impl 0 (THREEFRY) / 1 (PHILOX),
 * for ANY gjx_smc_plan, as gjx_plan_specialized_source returns an importance plan's: `needed` (nullable) receives the
 * size including the terminating 0; up to buf_len - 1 characters are copied into `buf` (nullable). */
int gjx_smc_plan_source(const gjx_smc_plan* p, int impl, char* buf, size_t buf_len, size_t* needed);

#ifdef __cplusplus
}
#endif
#endif /* GJX_GUIDED_H */
