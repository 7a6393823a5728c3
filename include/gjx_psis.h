/*
 * gjx_psis.h — Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO; Vehtari, Gelman & Gabry 2017; Vehtari et al.
 * 2024) over the plated site(s) of a tempered plan: per data row, the M + 1 smallest entries of the row's log-likelihood
 * over the particles selected EXACTLY, the generalised-Pareto fit of that tail, its shape k-hat and the row's elpd_loo.
 *
 * A THIRTEENTH header next to gjx.h (after gjx_paths.h, gjx_guided.h, gjx_backsim.h, gjx_backmove.h, gjx_smc_params.h,
 * gjx_csmc.h, gjx_temper.h, gjx_plate.h, gjx_pointwise.h, gjx_temper_cov.h and gjx_predictive.h), with a version of its own
 * and for the same reason: gjx.h is the boundary the CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry
 * points, the oracle library does not, and a binding loads them if present.  Conventions (status codes, gjx_stream, borrowed
 * "dev" pointers, no allocation, no host synchronisation) are those of gjx.h.
 *
 * Specification (D = n_rows of the plan's last gjx_temper_plan_set_data, parameters those of its last
 * gjx_temper_plan_set_params; n particles, equally weighted; M = tail_len).
 *
 *   t_i       = t[d, i] of gjx_pointwise.h: the f32 sum, in table order, of the row-d terms of the plan's PLATED sites at the
 *             latents of particle i.  The leave-one-out importance ratio of particle i is exp(-t_i): the SMALLEST entries
 *             of a row are its largest weights.
 *   order     entries are ordered by the integer key k(t) = bits(t) ^ (bits(t) >> 31 ? 0xFFFFFFFF : 0x80000000); every NaN
 *             maps to 0xFFFFFFFF.  The order is total: -inf first, -0 before +0, +inf, then the NaNs — so "the M + 1 smallest
 *             entries" is a well-defined multiset whatever ties there are.
 *   tail      tail[d, 0 .. M]: the M + 1 smallest entries in ascending order, f32, bit for bit (a NaN comes back as
 *             0x7FFFFFFF).  s = tail[0]; tT = tail[M], the cutoff, which is not itself smoothed; c_less = #{i: k(t_i) < k(tT)}.
 *   body      G = the sum, over the entries with k(t_i) >= k(tT) that are finite, of (double) exp_f32(f32(tT - t_i)) —
 *             exp_f32 the spec's f32 exponential at an argument never above 0, as gjx_pointwise.h uses it;
 *             B = G - (double)(M - c_less): the tail members tied with the cutoff contributed exactly 1 each.
 *             The particle axis is cut into W chunks (gjx_pointwise.h's rule with tiles = ceil(D / 4) row blocks and a
 *             target of 2048 workgroups); inside a chunk lane l of the 256 takes the particles lo + l, lo + l + 256, ... in
 *             that order, the lanes' sums are folded by a fixed binary tree, and the chunks' sums are added in index order:
 *             the order is a function of (n, D, M) alone.  No floating-point atomics: two calls on equal inputs give equal bits.
 *   bad       the number of entries that are NaN or +-inf.  A row with bad > 0: khat = +inf, sigma = NaN, elpd_loo = NaN.
 *   fit       float64 throughout, with the device library's log, log1p, exp, expm1 (not bit-pinned).  Exceedances in
 *             ascending order, x_j = exp(s - tail[M - j]) - exp(s - tT), j = 1 .. M (t_j = tail[M - j]).  Zhang & Stephens
 *             2009 with the constants of the `loo` package:
 *                 Gn = 30 + floor(sqrt(M));  xstar = x_[floor(M / 4 + 0.5)];
 *                 theta_j = 1 / x_M + (1 - sqrt(Gn / (j - 0.5))) / (3 xstar),  j = 1 .. Gn;
 *                 k_j = mean_i log1p(-theta_j x_i);  l_j = M (log(-theta_j / k_j) - k_j - 1);  w_j = 1 / sum_l exp(l_l - l_j);
 *                 theta = sum_j theta_j w_j;  k = mean_i log1p(-theta x_i);  sigma = -k / theta;  khat = (k M + 5) / (M + 10).
 *             A row with x_M <= 0 or xstar <= 0 (the tail is tied with its cutoff) is NOT smoothed: khat = +inf, sigma = NaN,
 *             raw weights kept.
 *   weights   in the scale where the largest raw weight is 0:  p_j = (j - 0.5) / M;
 *                 q_j = sigma expm1(-khat log1p(-p_j)) / khat   (-sigma log1p(-p_j) at khat == 0);
 *                 lw_j = min(log(q_j + exp(s - tT)), 0);        unsmoothed rows: lw_j = s - t_j.
 *   estimate  elpd_loo = log((n - M) e^s + sum_j exp(lw_j + t_j)) - log(e^(s - tT) B + sum_j exp(lw_j)),
 *             both logarithms with their largest exponent factored out.  (Every body term of the first sum is e^s exactly;
 *             the body of the second is B re-anchored: nothing cancels.)
 *
 *   out       f64 [7, D]: elpd_loo, khat, sigma, (double) s, (double) tT, B, bad.
 *
 * The tail length is the `loo` package's min(0.2 n, 3 sqrt(n / r_eff)) CAPPED at GJX_PSIS_MAX_TAIL = 4095, so that a row's
 * tail sorts and fits inside one workgroup's LDS: above n ~ 1.86e6 (at r_eff = 1) the tail is shorter than the package's.
 *
 * NINE launches and (with more than one chunk) one memset on the caller's stream, no host read: the generated kernel four
 * times (particles on lanes, a block of four rows wave-uniform: three passes of a radix select on the key with digits of
 * 11 / 11 / 10 bits, then the collect pass), a fixed kernel after each select pass (it extends the row's prefix), and a fixed
 * kernel of one workgroup per row that sorts the tail and runs the fit.
 */
#ifndef GJX_PSIS_H
#define GJX_PSIS_H

#include "gjx_pointwise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_PSIS_VERSION_MAJOR 0
#define GJX_PSIS_VERSION_MINOR 1

#define GJX_PSIS_MAX_TAIL 4095

typedef struct {
  uint64_t n;                                /* particles, tail_len + 1 .. 2^31 - 1 */
  const float* x[GJX_TEMPER_MAX_LATENTS];    /* dev f32[n] per latent, in the plan's latent order */
  uint32_t tail_len;                         /* M: 5 .. GJX_PSIS_MAX_TAIL, below n */
  double* out;                               /* dev f64[7 * n_rows]: elpd_loo, khat, sigma, s, tT, B, bad */
  float* tail;                               /* nullable: dev f32[n_rows * (tail_len + 1)], each row ascending */
  void* ws;                                  /* dev, 8-byte aligned, gjx_psis_workspace_bytes(n, n_rows, tail_len) bytes */
  size_t ws_bytes;
} gjx_psis_io;

int gjx_psis_version(int* major, int* minor);
/* min(floor(0.2 n), ceil(3 sqrt(n / r_eff)), GJX_PSIS_MAX_TAIL), or 0 when that is below 5 (n < 25) or an argument is out of
 * range (n 0 or >= 2^31, r_eff not a positive finite number). */
uint32_t gjx_psis_tail_len(uint64_t n, double r_eff);
/* 0 for arguments out of range (n, n_rows outside 1 .. 2^31 - 1, tail_len outside 5 .. GJX_PSIS_MAX_TAIL).  The workspace
 * need not be initialised. */
size_t gjx_psis_workspace_bytes(uint64_t n, uint64_t n_rows, uint32_t tail_len);
/* The kernel is generated from the table and compiled on first use: with the compiler switched off (GJX_PLAN_JIT=0)
 * GJX_ERR_UNSUPPORTED; GJX_ERR_JIT if it fails.
 * GJX_ERR_INVALID (nothing compiled, nothing launched): everything gjx_temper_pointwise refuses (a NULL plan / io / latent
 * column / out, a plan without a PLATED site, a plated plan without data, n 0 or >= 2^31, fewer parameters than the table
 * reads, a table that reads a per-particle input column, ws not 8-byte aligned), tail_len outside 5 .. GJX_PSIS_MAX_TAIL,
 * tail_len >= n.
 * GJX_ERR_WORKSPACE: ws NULL or smaller than gjx_psis_workspace_bytes(n, n_rows, tail_len). */
int gjx_temper_psis(gjx_temper_plan* p, const gjx_psis_io* io, gjx_stream s);
/* The HIP source of the plan's generated PSIS kernel: it holds no data value, no parameter value, neither n nor n_rows nor
 * tail_len.  GJX_ERR_INVALID for a NULL plan, a plan without a PLATED site or one that reads an input column. */
int gjx_psis_source(const gjx_temper_plan* p, char* buf, size_t buf_len, size_t* needed);
/* Compiles that source for gfx950 without touching a GPU: GJX_OK, or GJX_ERR_UNSUPPORTED when it does not compile. */
int gjx_psis_compile_check(const gjx_temper_plan* p);

#ifdef __cplusplus
}
#endif
#endif /* GJX_PSIS_H */
