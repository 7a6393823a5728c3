/*
 * gjx_smc_params.h — parameterised state-space models: a bank of particle filters, one parameter row each, per launch.
 *
 * A further header next to gjx.h (after gjx_paths.h, gjx_guided.h, gjx_backsim.h, gjx_backmove.h), with a version of its
 * own and for the same reason: gjx.h is the boundary the CPU oracle restates symbol for symbol.  libgjx_hip.so exports
 * these entry points, the oracle library does not, and a binding loads them if present.  Conventions are those of gjx.h.
 *
 * The plans of gjx_smc_plan_create* hold every model number as a constant of the generated source: another value is
 * another kernel.  A PARAMETERISED plan reads such numbers from a ROW of launch parameters instead — GJX_ARG_PARAM
 * arguments ({GJX_ARG_PARAM, slot, scale, offset}: scale * row[slot] + offset, as in importance plans) and GJX_EXPR_PARAM
 * leaves of postfix programs — so its source holds no parameter value and one compiled kernel serves every row.  The step
 * kernel runs up to 16 independent filters per launch (gjx_smc_config.n_filters); each of them may take a row of its own:
 * one launch then evaluates the likelihood at 16 parameter points.
 *
 * Per-site constants that gjx_smc_plan_create derives from constant arguments (a Normal's 1 / scale and log
 * normaliser, a Gamma's and a Beta's log normaliser) are derived on the host per row, with the same functions, for sites
 * whose arguments are constants or parameters: a parameter is bit-equal to the same number written as a constant.
 *
 * The result is a plain gjx_smc_plan: gjx_smc_run_plan, gjx_smc_plan_step (one filter: row 0), gjx_smc_plan_source,
 * gjx_smc_plan_compile_check, ESS-adaptive resampling and ancestor output apply unchanged.  A run copies the rows it
 * uses to a device table the plan owns, on the caller's stream, in front of its first launch (gjx_smc_plan_step: in front
 * of the first step after a gjx_smc_plan_set_params, and of every step 0): runs of ONE plan that may overlap on the device
 * must therefore share a stream.  Steps stay one launch each; there is no copy per step.
 *
 *   GJX_ERR_INVALID      a run or step before any gjx_smc_plan_set_params; n_rows > 1 and != the run's filter count
 *   GJX_ERR_UNSUPPORTED  the table-walking route (GJX_PLAN_JIT=0): parameterised plans run as generated kernels only, as
 *                        guided plans do; the sharded drivers (gjx_smc_sharded_run_plan) and cfg->peers
 */
#ifndef GJX_SMC_PARAMS_H
#define GJX_SMC_PARAMS_H

#include "gjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_SMC_PARAMS_VERSION_MAJOR 0
#define GJX_SMC_PARAMS_VERSION_MINOR 1

#define GJX_SMC_PARAMS_MAX_ROWS 16 /* = the filters of one launch */

int gjx_smc_params_version(int* major, int* minor);
/* As gjx_smc_plan_create_scoped (scopes nullable), with GJX_ARG_PARAM arguments and GJX_EXPR_PARAM leaves accepted
 * in both site tables, in init_state / next_state and in observed values; gjx_site.observed 0..3 (guided plans
 * included).  n_params: 1 .. GJX_MAX_PARAMS, greater than every referenced slot. */
int gjx_smc_plan_create_params(const gjx_smc_model* m, const gjx_scope* init_scopes, int n_init_scopes,
                               const gjx_scope* step_scopes, int n_step_scopes, int n_params, gjx_smc_plan** out);
/* rows: host f32[n_rows, n_params], copied.  n_rows == 1: the row serves every filter of the launches that follow;
 * n_rows == F: filter f of a run with cfg->n_filters == F takes row f (any other F: GJX_ERR_INVALID at the run). */
int gjx_smc_plan_set_params(gjx_smc_plan* p, const float* rows, int n_rows);

#ifdef __cplusplus
}
#endif
#endif /* GJX_SMC_PARAMS_H */
