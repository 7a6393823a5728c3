/*
 * gjx_predictive.h — posterior predictive draws of a plated tempered plan: replicated data y_rep ~ p(y | x_i, data_d) for
 * every particle i and data row d, summarised per row over the PARTICLES, a strided subset of the draws stored.
 *
 * A TWELFTH header next to gjx.h (after gjx_paths.h, gjx_guided.h, gjx_backsim.h, gjx_backmove.h, gjx_smc_params.h,
 * gjx_csmc.h, gjx_temper.h, gjx_plate.h, gjx_pointwise.h and gjx_temper_cov.h), with a version of its own and for the same
 * reason: gjx.h is the boundary the CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points, the
 * oracle library does not, and a binding loads them if present.  Conventions (status codes, gjx_stream, borrowed "dev"
 * pointers, no allocation, no host synchronisation) are those of gjx.h.  It builds on gjx_plate.h alone.
 *
 * Specification (exact: the result is a function of the inputs and the key, bit for bit; D = n_rows of the plan's last
 * gjx_temper_plan_set_data, parameters those of its last gjx_temper_plan_set_params; the plan's PLATED sites are
 * s = 0 .. S-1 in table order).
 *
 *   shadow    the SHADOW TABLE of the plan holds its plated sites alone, in table order, as LATENT sites (observed = 0,
 *             value column s).  A GJX_ARG_DATA operand (GJX_EXPR_DATA leaf) of column c reads per-particle input column c;
 *             a reference to latent l of the plan reads input column C + l (C = the plan's data columns), a column that
 *             holds one value; parameters are unchanged.  No plated site reads another's draw: a plated site's value that
 *             feeds a later site is data (gjx_plate.h).
 *   draws     y[s][d, i] is the value gjx_importance_run of the shadow table writes for site s and "particle" d in a run
 *             over D particles under the lazy key batch {impl, mode 1, parent = fold_in(key, i), first = 0}, with input
 *             columns 0 .. C-1 the plan's data columns and column C + l holding x_l[i] in every row.  Site numbering, the
 *             PHILOX pair blocks of rows (2r, 2r + 1), the Box-Muller transform over such a pair and the sub-streams of the
 *             multi-word samplers are those of an importance pass: nothing new is specified.  Stored as f32 (Bernoulli: 0 / 1).
 *             Unplated observed sites and the prior do not enter.
 *   obs       obs[s][d]: the site's observed value at row d, evaluated in f32 as gjx_plate.h evaluates it (Bernoulli:
 *             rint(value) != 0, as 0 / 1).
 *   summaries per site s and row d over ALL n particles:
 *                 s1 = sum (double) y;  s2 = sum (double) y * (double) y   (the product rounded once);
 *                 below = #{y < obs};  equal = #{y == obs};  nan = #{y != y}.
 *             Comparisons are false on NaN; NaN and +-inf reach s1 and s2 by IEEE rules — visible, not hidden.
 *   order     the particle axis is cut into W = gjx_predictive_chunks(n, D) contiguous chunks of per = ceil(n / W) particles
 *             (the last one shorter), with tiles = ceil(D / 512):
 *                 W = min(ceil(n / 256), max(1, ceil(2048 / tiles)))
 *             A chunk is walked in index order from +0; the chunks' sums are folded in index order in float64 from +0.
 *             Counts are integers, stored as doubles.
 *   out       f64[S][5][D]: out[(s * 5 + k) * D + d], k = 0 .. 4: s1, s2, below, equal, nan.
 *   draws     with draw_stride = k >= 1, particle i with i % k == 0 stores its draws: draws[(s * m + i / k) * D + d] = y[s][d, i],
 *             m = ceil(n / k); f32[S][m][D].  k = 0 stores none (draws may be NULL).  A stride, not a prefix: after systematic
 *             resampling neighbouring particles are copies of one ancestor.
 * There is no grid knob: two calls on equal inputs give equal bits.
 *
 * TWO launches: the generated kernel (a lane owns the data rows 2r and 2r + 1 — under PHILOX one cipher block and one
 * Box-Muller transform serve both — and holds their data in registers; the particles of a chunk are wave-uniform scalar
 * loads; no LDS, no barrier) writes one (s1, s2, below, equal, nan) per chunk, site and row to the workspace; a fixed kernel
 * with one lane per row and site folds the chunks.  Rows occupy lanes: below 128 rows lanes idle.
 */
#ifndef GJX_PREDICTIVE_H
#define GJX_PREDICTIVE_H

#include "gjx_plate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_PREDICTIVE_VERSION_MAJOR 0
#define GJX_PREDICTIVE_VERSION_MINOR 1

typedef struct {
  uint64_t n;                                /* particles, 1 .. 2^31 - 1 */
  const float* x[GJX_TEMPER_MAX_LATENTS];    /* dev f32[n] per latent, in the plan's latent order */
  double* out;                               /* dev f64[S * 5 * n_rows] */
  float* draws;                              /* dev f32[S * ceil(n / draw_stride) * n_rows]; NULL with draw_stride 0 */
  uint64_t draw_stride;                      /* 0: no draws stored */
  void* ws;                                  /* dev, 8-byte aligned, gjx_predictive_workspace_bytes(n, n_rows, S) bytes */
  size_t ws_bytes;
} gjx_predictive_io;

int gjx_predictive_version(int* major, int* minor);
/* W of the specification above; 0 for n or n_rows outside 1 .. 2^31 - 1. */
uint32_t gjx_predictive_chunks(uint64_t n, uint64_t n_rows);
/* gjx_predictive_chunks(n, n_rows) * n_rows * n_plated * 40; 0 for arguments out of range (n_plated outside
 * 1 .. GJX_MAX_SITES included).  The workspace need not be initialised. */
size_t gjx_predictive_workspace_bytes(uint64_t n, uint64_t n_rows, int32_t n_plated);
/* TWO launches on stream s.  The kernel is generated from the table and compiled on first use, one per generator
 * (key->impl): with the compiler switched off (GJX_PLAN_JIT=0) GJX_ERR_UNSUPPORTED; GJX_ERR_JIT if it fails.
 * GJX_ERR_INVALID (nothing compiled, nothing launched): a NULL plan / key / io / latent column / out, a key that is not ONE
 * literal key (mode 2, no fold; a lane under PHILOX only), a plan without a PLATED site, a plated plan without data, n 0 or
 * >= 2^31, fewer parameters than the table reads, a table that reads a per-particle input column (GJX_ARG_INPUT: the io has
 * none), draw_stride > 0 with draws NULL, ws not 8-byte aligned.
 * GJX_ERR_WORKSPACE: ws NULL or smaller than gjx_predictive_workspace_bytes. */
int gjx_temper_predictive(gjx_temper_plan* p, const gjx_keys* key, const gjx_predictive_io* io, gjx_stream s);
/* The HIP source of the plan's generated predictive kernel under generator impl: it holds no data value, no parameter
 * value, neither n nor n_rows.  GJX_ERR_INVALID for a NULL plan, an impl that is neither generator, a plan without a PLATED
 * site or one that reads an input column. */
int gjx_predictive_source(const gjx_temper_plan* p, int impl, char* buf, size_t buf_len, size_t* needed);
/* Compiles that source for gfx950 without touching a GPU: GJX_OK, or GJX_ERR_UNSUPPORTED when it does not compile. */
int gjx_predictive_compile_check(const gjx_temper_plan* p, int impl);

#ifdef __cplusplus
}
#endif
#endif /* GJX_PREDICTIVE_H */
