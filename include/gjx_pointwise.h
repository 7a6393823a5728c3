/*
 * gjx_pointwise.h — pointwise predictive densities of a plated tempered plan: the per-row log-likelihood table of a
 * population, reduced over the PARTICLES.
 *
 * A TENTH header next to gjx.h (after gjx_paths.h, gjx_guided.h, gjx_backsim.h, gjx_backmove.h, gjx_smc_params.h,
 * gjx_csmc.h, gjx_temper.h and gjx_plate.h), with a version of its own and for the same reason: gjx.h is the boundary the
 * CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points, the oracle library does not, and a
 * binding loads them if present.  Conventions (status codes, gjx_stream, borrowed "dev" pointers, no allocation, no host
 * synchronisation) are those of gjx.h.
 *
 * The move kernel of a plated plan (gjx_plate.h) evaluates t[d, i] = log p(y_d | x_i, data_d) for every particle i and data
 * row d and keeps the sum over d per particle.  gjx_temper_pointwise keeps the OTHER reduction: per row, over the particles,
 * the log-sum-exp, the first two moments and the count of the entries above -inf — what the log pointwise predictive
 * density, WAIC and held-out scores are made of.  It draws nothing: no key, no generator choice, one source per plan.
 *
 * Specification (exact: the result is a function of the inputs alone, bit for bit; D = n_rows of the plan's last
 * gjx_temper_plan_set_data, parameters those of its last gjx_temper_plan_set_params).
 *
 *   t[d, i]   the f32 sum, from +0 and in table order, of the row-d terms of the plan's PLATED sites: each term is the t_d of
 *             gjx_plate.h — arguments and value evaluated in f32 at row d with the latents x_l[i] of particle i, every
 *             operator rounding once, nothing contracted.  (A plan with one plated site: that site's term.)  Unplated
 *             observed sites and the prior do not enter.
 *   chunks    the particle axis is cut into W = gjx_pointwise_chunks(n, D) contiguous chunks of per = ceil(n / W) particles
 *             (the last one shorter), with tiles = ceil(D / 256):
 *                 W = min(ceil(n / 256), max(1, ceil(2048 / tiles)))
 *             — about 2048 workgroups whatever D is, and a workspace of W * D * 40 bytes: at most 21 MB while D <= 2048
 *             tiles (524 288 rows), 40 bytes per row beyond.
 *   a chunk   walks its particles in index order in BLOCKS of four (then the remaining 0 .. 3 one by one), with the state
 *             m = -inf (f32), s = s1 = s2 = +0 (f64), c = 0.  For a block t_0 .. t_{B-1}:
 *                 s1 = s1 + (double) t_j,  s2 = s2 + (double) t_j * (double) t_j      j in order, the product rounded once;
 *                 bm = m;  bm = t_j > bm ? t_j : bm                                  j in order (false on NaN);
 *                 if bm > m:  s = s * (double) exp_f32(f32(m - bm)),  m = bm;
 *                 for j in order, if t_j > -inf:  s = s + (double) exp_f32(f32(t_j - m)),  c = c + 1.
 *             exp_f32 is the spec's f32 exponential (0 below -86, so a first finite entry rescales s = 0 by 0).
 *   the fold  per row, over the chunks k = 0 .. W-1 IN INDEX ORDER, in float64:  M = max_k m_k;
 *                 S = sum over the chunks with m_k > -inf of s_k * exp((double) m_k - (double) M)    (the double exp);
 *                 out[0 * D + d] = lse_d = (double) M + log(S), -inf when no entry is above -inf;
 *                 out[1 * D + d] = s1_d = sum_k s1_k;   out[2 * D + d] = s2_d = sum_k s2_k;
 *                 out[3 * D + d] = c_d = sum_k c_k, as a double.
 * An entry that is -inf or NaN contributes nothing to lse_d or c_d; s1 and s2 carry it by IEEE rules, so a NaN term reaches
 * the moments and is not hidden.  There is no grid knob: two calls on equal inputs give equal bits.
 *
 * TWO launches: the generated kernel (lanes are ROWS — a lane holds its row of the data columns in registers — and the
 * particles of a chunk are wave-uniform scalar loads; no LDS, no barrier) writes one (m, s, s1, s2, c) per chunk and row to
 * the workspace; a fixed kernel with one lane per row folds the chunks.  Rows occupy lanes: below 64 rows lanes idle — the
 * plated path exists for hundreds of rows and more.
 */
#ifndef GJX_POINTWISE_H
#define GJX_POINTWISE_H

#include "gjx_plate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_POINTWISE_VERSION_MAJOR 0
#define GJX_POINTWISE_VERSION_MINOR 1

typedef struct {
  uint64_t n;                                /* particles, 1 .. 2^31 - 1 */
  const float* x[GJX_TEMPER_MAX_LATENTS];    /* dev f32[n] per latent, in the plan's latent order */
  double* out;                               /* dev f64[4 * n_rows]: lse, s1, s2, c */
  void* ws;                                  /* dev, 8-byte aligned, gjx_pointwise_workspace_bytes(n, n_rows) bytes */
  size_t ws_bytes;
} gjx_pointwise_io;

int gjx_pointwise_version(int* major, int* minor);
/* W of the specification above; 0 for n or n_rows outside 1 .. 2^31 - 1. */
uint32_t gjx_pointwise_chunks(uint64_t n, uint64_t n_rows);
/* gjx_pointwise_chunks(n, n_rows) * n_rows * 40; 0 for arguments out of range.  The workspace need not be initialised. */
size_t gjx_pointwise_workspace_bytes(uint64_t n, uint64_t n_rows);
/* TWO launches on stream s.  The kernel is generated from the table and compiled on first use: with the compiler switched
 * off (GJX_PLAN_JIT=0) GJX_ERR_UNSUPPORTED; GJX_ERR_JIT if it fails.
 * GJX_ERR_INVALID (nothing launched): a NULL plan / io / latent column / out, a plan without a PLATED site, a plated plan
 * without data, n 0 or >= 2^31, fewer parameters than the table reads, a table that reads a per-particle input column
 * (GJX_ARG_INPUT: the io has none), ws not 8-byte aligned.
 * GJX_ERR_WORKSPACE: ws NULL or smaller than gjx_pointwise_workspace_bytes(n, n_rows). */
int gjx_temper_pointwise(gjx_temper_plan* p, const gjx_pointwise_io* io, gjx_stream s);
/* The HIP source of the plan's generated pointwise kernel: it holds no data value, no parameter value, neither n nor
 * n_rows.  GJX_ERR_INVALID for a NULL plan, a plan without a PLATED site or one that reads an input column. */
int gjx_pointwise_source(const gjx_temper_plan* p, char* buf, size_t buf_len, size_t* needed);
/* Compiles that source for gfx950 without touching a GPU: GJX_OK, or GJX_ERR_UNSUPPORTED when it does not compile. */
int gjx_pointwise_compile_check(const gjx_temper_plan* p);

#ifdef __cplusplus
}
#endif
#endif /* GJX_POINTWISE_H */
