/*
 * gjx_plate.h — plated likelihoods in a tempered plan: ONE observed site looped over the rows of a device data table.
 *
 * A NINTH header next to gjx.h (after gjx_paths.h, gjx_guided.h, gjx_backsim.h, gjx_backmove.h, gjx_smc_params.h, gjx_csmc.h
 * and gjx_temper.h), with a version of its own and for the same reason: gjx.h is the boundary the CPU oracle restates symbol
 * for symbol.  libgjx_hip.so exports these entry points, the oracle library does not, and a binding loads them if present.
 * Conventions (status codes, gjx_stream, borrowed "dev" pointers, no allocation, no host synchronisation) are those of gjx.h.
 *
 * A tempered plan (gjx_temper.h) holds every observation as a row of its site table and every number of the data set as a
 * launch parameter: GJX_MAX_SITES and GJX_MAX_PARAMS end it at about 30 (x, y) pairs.  A PLATED site is one row of the
 * table whose arguments and observed value are read from device DATA COLUMNS of length n_rows and which is evaluated for
 * the rows d = 0 .. n_rows - 1 inside assess.  Neither n_rows nor any data value is in the generated source: another data
 * set, of any length, costs no compilation.
 *
 *   GJX_SITE_PLATED (gjx_site.observed == 4)  an observed site evaluated once per data row.
 *   GJX_ARG_DATA    (gjx_arg.kind == 9)       value = scale * data[ref][d] + offset.
 *   GJX_EXPR_DATA   (gjx_expr_op.op == 21)    push data[ref][d].
 * DATA operands are valid in a0, a1 and obs of a PLATED site only, directly or inside a GJX_ARG_EXPR program (obs of a
 * PLATED site may be a program).  Every other creator (gjx_plan_create*, gjx_smc_plan_create*, gjx_scan_plan_create*,
 * gjx_backsim_plan_create, gjx_temper_plan_create) refuses mode 4 and both DATA kinds.
 *
 * Specification, added to `assess` of gjx_temper.h (exact: a function of the inputs alone).  At a PLATED site's table
 * position:
 *   for d = 0 .. n_rows - 1, in order: t_d = the f32 value gjx_logpdf_<dist> returns for the site's arguments and observed
 *   value evaluated in f32 at row d — every operator of an affine form or program rounds once, nothing is contracted; an
 *   integer-valued (Bernoulli) value is rint(data) != 0;
 *   acc = acc + (double) t_d, a FLOAT64 sum from +0.0;
 *   then ll = ll + (float) acc: one f32 rounding of the site's total, one rounding of the add.
 * Float64 because a sequential f32 sum over 10^4 terms of magnitude 1 drifts by about 10^-3 of a total of about 10^4 — an
 * error in the very difference the accept test takes — while the convert and the add cost two instructions per datum.
 * In numpy:  t = logpdf(args[d], obs[d]).astype(float32);  acc = 0.0;  for v in t: acc += float64(v);  ll = float32(ll + float32(acc)).
 *
 * Every lane of the move kernel reads the SAME row at the same moment: the row reads are wave-uniform loads through the
 * scalar data cache, issued for a block of rows before the block's arithmetic; no LDS, no barrier.
 */
#ifndef GJX_PLATE_H
#define GJX_PLATE_H

#include "gjx_temper.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_PLATE_VERSION_MAJOR 0
#define GJX_PLATE_VERSION_MINOR 1

#define GJX_SITE_PLATED 4 /* gjx_site.observed */
#define GJX_ARG_DATA 9    /* gjx_arg.kind (GJX_ARG_NEXT is 8) */
#define GJX_EXPR_DATA 21  /* gjx_expr_op.op (GJX_EXPR_SELECT is 20) */
#define GJX_PLATE_MAX_COLS 16

int gjx_plate_version(int* major, int* minor);
/* As gjx_temper_plan_create, with PLATED sites accepted; a table without one gives the plan gjx_temper_plan_create gives.
 * GJX_ERR_INVALID: whatever gjx_temper_plan_create refuses (a PLATED site counts as an observed one); `observed` outside
 * 0, 1, 4; a DATA operand outside a PLATED site; a column index >= GJX_PLATE_MAX_COLS; a PLATED Categorical site (table
 * rows per datum belong to a later change); a PLATED site whose `obs` holds no DATA operand. */
int gjx_temper_plan_create_plated(const gjx_site* sites /*host*/, int n_sites, uint32_t flags, gjx_temper_plan** out);
/* The data columns of the launches that follow: cols is a HOST array of n_cols dev f32[n_rows] pointers, BORROWED (they
 * must stay valid, and may change contents, until the next call or the plan's destruction).
 * GJX_ERR_INVALID: a NULL plan / array / referenced column, a plan without PLATED sites, n_rows 0 or >= 2^31, n_cols
 * outside 1 .. GJX_PLATE_MAX_COLS or not greater than the largest column the table reads.
 * gjx_temper_move on a plated plan without data returns GJX_ERR_INVALID and launches nothing. */
int gjx_temper_plan_set_data(gjx_temper_plan* p, const float* const* cols /*host array of dev f32[n_rows]*/, int n_cols,
                             uint64_t n_rows);

#ifdef __cplusplus
}
#endif
#endif /* GJX_PLATE_H */
