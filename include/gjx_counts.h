/*
 * gjx_counts.h — count-data sites: Poisson(rate) and NegativeBinomial(total_count, probs), with TFP's parameterisation
 * (the negative binomial counts successes of probability `probs` before `total_count` failures; total_count real, > 0).
 *
 * A FOURTEENTH header next to gjx.h (after gjx_paths.h, gjx_guided.h, gjx_backsim.h, gjx_backmove.h, gjx_smc_params.h,
 * gjx_csmc.h, gjx_temper.h, gjx_plate.h, gjx_pointwise.h, gjx_temper_cov.h, gjx_predictive.h and gjx_psis.h), with a version
 * of its own and for the same reason: gjx.h is the boundary the CPU oracle restates symbol for symbol.  libgjx_hip.so exports
 * these entry points, the oracle library does not, and a binding loads them if present.  Conventions (status codes,
 * gjx_stream, gjx_keys, gjx_f32, borrowed "dev" pointers, no allocation, no host synchronisation) are those of gjx.h.
 *
 * Two distribution ids, both integer-valued (a value travels as int32, as a Categorical's does):
 *   GJX_DIST_POISSON = 5            a0 = rate
 *   GJX_DIST_NEGATIVE_BINOMIAL = 6  a0 = total_count (r), a1 = probs (p)
 * The creators of gjx.h and of every other header refuse both ids.
 *
 * Specification (exact, in the style of gjx.h: every operator below is an f32 operation that rounds once, nothing is
 * contracted, m_log / m_exp / m_lgamma / xlogy / uniform01 / std_gamma are the functions of DESIGN.md §3, and a result is a
 * function of the inputs and the key alone).
 *
 * Densities.  k = (float) value (a count is exact in f32 up to 2^24; hosts refuse larger observed counts), lf = m_lgamma(k + 1):
 *   Poisson            (xlogy(k, rate) - rate) - lf
 *   NegativeBinomial   (((m_lgamma(k + r) - lf) - m_lgamma(r)) + xlogy(k, p)) + xlogy(r, 1 - p)
 *   arguments outside the domain — not (rate >= 0); not (r > 0); not (0 <= p <= 1); NaN included — give NaN, as TFP does;
 *   otherwise a value that is not >= 0 (the comparison is taken on k, in float) gives -inf;
 *   p == 1 is inside the domain and follows the formula (xlogy(r, 0) = -inf), rate == 0 likewise (0 at k = 0 up to lf).
 * Accuracy floor: the terms are of size k log k and cancel, so one f32 ulp of a term is the error of the result — about 1e-2
 * nats at counts near 1e5, 1e-6 at counts below 10.  A better-conditioned form for large counts is not part of this version.
 *
 * Draws.  st = the site's draw stream (gjx.h: key plus fold), words(s) = (w0, w1) of its sub-stream s.
 * poisson(st, B, rate):
 *   not (rate >= 0), NaN included     -> -1 (outside the support; its score is NaN), no word read
 *   rate == 0                         -> 0, no word read
 *   rate > 2^30, +inf included        -> 2^30 (saturation: the value stays an int32 and exact in f32), no word read
 *   rate < 10: inversion by sequential search.  u = uniform01(w0 of words(B)); p = m_exp(-rate); s = p; k = 0;
 *              while (u >= s && k < 128) { k += 1; p = (p * rate) / (float) k; s = s + p; }       -> k
 *   rate >= 10: Hörmann's PTRS (1993), at most 64 attempts.  Once:
 *                slam = sqrt(rate); b = 0.931 + 2.53 slam; a = -0.059 + 0.02483 b;
 *                inv_alpha = 1.1239 + 1.1328 / (b - 3.4); vr = 0.9277 - 3.6224 / (b - 2)
 *              attempt att = 0 .. 63 over words(B + 1 + att):
 *                U = uniform01(w0) - 0.5; V = uniform01(w1); us = 0.5 - |U|;
 *                kf = floor((((2 a) / us + b) U + rate) + 0.43)
 *                reject unless 0 <= kf < 2^31 (a NaN or infinite kf is rejected here);
 *                accept at us >= 0.07 && V <= vr;
 *                reject at us < 0.013 && V > us;
 *                accept iff (m_log(V) + m_log(inv_alpha)) - m_log(a / (us us) + b) <= (-rate + kf m_log(rate)) - m_lgamma(kf + 1)
 *              an accepted attempt -> (int) kf; after 64 rejections -> (int) rate.
 * A Poisson site uses B = 0.  NegativeBinomial(r, p): arguments outside the domain, and p == 1 (the law has no finite count:
 * the density is -inf at every k) -> -1, whose score is NaN outside the domain and -inf at p == 1; else
 *   g = std_gamma(st, 0, r) * (p / (1 - p)), then poisson(st, 256, g): the gamma owns sub-streams 0 .. 128.
 * Every loop is bounded (128 steps, 64 attempts): no input makes a draw wait.
 * The score written next to a draw is the density above at that draw, bit for bit.
 */
#ifndef GJX_COUNTS_H
#define GJX_COUNTS_H

#include "gjx_plate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_COUNTS_VERSION_MAJOR 0
#define GJX_COUNTS_VERSION_MINOR 1

#define GJX_DIST_POISSON 5           /* gjx_site.dist (GJX_DIST_CATEGORICAL is 4) */
#define GJX_DIST_NEGATIVE_BINOMIAL 6 /* gjx_site.dist */
#define GJX_COUNTS_MAX_OBSERVED 16777216 /* 2^24: the largest observed count a host accepts */

int gjx_counts_version(int* major, int* minor);

/* score_out[i] = the density at value[i] (dev int32[n]), or at value_scalar where value is NULL.
 * GJX_ERR_INVALID: a NULL score_out. */
int gjx_logpdf_poisson(const int32_t* value /*nullable*/, int value_scalar, gjx_f32 rate, float* score_out /*dev f32[n]*/,
                       uint64_t n, gjx_stream s);
int gjx_logpdf_negative_binomial(const int32_t* value /*nullable*/, int value_scalar, gjx_f32 total_count, gjx_f32 probs,
                                 float* score_out /*dev f32[n]*/, uint64_t n, gjx_stream s);

/* One draw per key of the batch, as gjx_sample_logpdf_gamma takes it, under both ciphers; score_out may be NULL.
 * GJX_ERR_INVALID: a malformed key batch, a NULL value_out. */
int gjx_sample_logpdf_poisson(const gjx_keys* k, gjx_f32 rate, int32_t* value_out /*dev i32[n]*/, float* score_out /*nullable*/,
                              uint64_t n, gjx_stream s);
int gjx_sample_logpdf_negative_binomial(const gjx_keys* k, gjx_f32 total_count, gjx_f32 probs, int32_t* value_out /*dev i32[n]*/,
                                        float* score_out /*nullable*/, uint64_t n, gjx_stream s);

/* As gjx_temper_plan_create_plated (gjx_plate.h), with the two ids also accepted at OBSERVED (gjx_site.observed == 1) and
 * PLATED (4) sites; a table without a count site gives the plan gjx_temper_plan_create_plated gives, with the same generated
 * sources byte for byte.  Added to `assess` of gjx_temper.h / gjx_plate.h:
 *   an OBSERVED count site: k = (float) rint(obs), lf = m_lgamma(k + 1) in the kernel, the density above;
 *   a PLATED count site: obs is a plain DATA operand {GJX_ARG_DATA, c, 1, 0}; at row d, k = (float) rint(data[c][d]) and
 *   lf = data[c + 1][d] — log k! is DATA, not arithmetic: the caller fills column c + 1 with (float) lgamma(k + 1) taken in
 *   float64, it counts against GJX_PLATE_MAX_COLS, and gjx_temper_plan_set_data must be given it (n_cols > c + 1).
 * gjx_temper_pointwise, gjx_temper_psis and gjx_temper_predictive take such a plan as they take any plated plan; a
 * replicated count is drawn by the rule above from the stream of its (particle, row) key and compared with rint(data).
 * GJX_ERR_INVALID: whatever gjx_temper_plan_create_plated refuses; a count id at a latent site (a count-valued latent has no
 * random-walk move); a PLATED count site whose obs is a program, is scaled or shifted, or has c + 1 >= GJX_PLATE_MAX_COLS. */
int gjx_temper_plan_create_counts(const gjx_site* sites /*host*/, int n_sites, uint32_t flags, gjx_temper_plan** out);

#ifdef __cplusplus
}
#endif
#endif /* GJX_COUNTS_H */
