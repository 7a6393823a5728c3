/*
 * gjx_quantiles.h — exact quantiles and moments of f32 columns that sit in device memory: per column the order statistics
 * that bracket up to 8 probabilities, the interpolated quantiles, and NaN count, mean, sample variance, minimum and maximum.
 * What TemperedSMC.summary asks of the library: a scalar latent is one column, a grouped latent [G, n] is G columns.
 *
 * A NINETEENTH header next to gjx.h, with a version of its own and for the same reason as the others: gjx.h is the boundary
 * the CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points, the oracle library does not, and a
 * binding loads them if present.  Conventions (status codes, gjx_stream, borrowed "dev" pointers, no allocation, no host
 * synchronisation) are those of gjx.h.
 *
 * COLUMNS.  n_cols columns of f32[n], numbered through the segments in order: segment s holds seg[s].n_cols columns, its
 * column j starting at seg[s].base + j * seg[s].stride (in elements).  A column base need not be 16-byte aligned.
 *
 * Specification (exact: a function of the inputs alone; everything is per column c; Q = n_probs).
 *
 *   key       the order is the key of gjx_psis.h: k(x) = bits(x) ^ (bits(x) >> 31 ? 0xFFFFFFFF : 0x80000000); every NaN maps
 *             to 0xFFFFFFFF.  nan = the number of NaNs, m = n - nan the number of VALID entries; everything below is over the
 *             valid entries, +-inf among them; -0 orders before +0.
 *   rank      for probability p_j the real rank is h = (double)(m - 1) * p_j (one float64 product), lo = floor(h),
 *             hi = min(lo + 1, m - 1): the linear rule, numpy's default.
 *   bracket   bracket[c][j][0 .. 1] = the lo-th and the hi-th order statistic (0-based, ascending in the key) as f32, bit
 *             for bit.  m = 0: both NaN (0x7FC00000).
 *   quant     quant[c][j] = (double) x_lo where the two brackets have equal bits, else x_lo + (h - lo) * (x_hi - x_lo) in
 *             float64: the difference, the product and the sum round once each, no FMA.  m = 0: NaN.
 *   stats     stats[c][0 .. 4], f64: nan, mean, sample variance (divisor m - 1; NaN for m < 2), min, max (NaN for m = 0).
 *             mean = S1 / m, S1 the float64 sum of the valid entries; variance = S2 / (m - 1), S2 the float64 sum of
 *             ((double) x - mean)^2 over the valid entries taken in a LATER sweep, when the mean is known — not
 *             E[x^2] - E[x]^2.  Both sums in the same fixed order:
 *               blocks   the particle axis is cut into contiguous blocks of per = ceil(n / B) entries: ceil(n / per) of them, the
 *                        last shorter.
 *                        max_workgroups = 0: B = min(ceil(n / 16384), max(1, 2048 / C'), 1024), C' the columns of one
 *                        batch, min(n_cols, 256).  max_workgroups = w > 0: C' = min(n_cols, 256, w) and
 *                        B = min(ceil(n / 1024), max(1, w / C'), 1024): no launch of a sweep has more than w workgroups.
 *               a block  over [b0, b1): with a = the column base's offset from a 16-byte boundary in elements, the entries
 *                        before the first i >= b0 with (a + i) % 4 == 0 are the HEAD (at most 3), then QUADS of four, then the
 *                        TAIL (at most 3).  Lane t of 256 sums, from +0 and in this order: the quads t, t + 256, ... (each
 *                        quad's four entries in index order); then the head entry b0 + t if t < |head|, else the tail entry
 *                        number t - |head| if t < |head| + |tail|.  A NaN adds nothing.
 *               lanes    the BALANCED TREE over the 256 lane sums in lane order: level k = 0 .. 7 adds the sums of the two
 *                        adjacent aligned runs of 2^k lanes.
 *               fold     the blocks' sums in index order from +0.
 *   No floating-point atomics anywhere: two calls on equal inputs give equal bits — in bracket, quant, nan, min and max
 *   whatever max_workgroups is, in mean and variance at equal max_workgroups (it sets B).
 *
 * LAUNCHES, per batch of C' columns, fixed device code on the caller's stream, no host read: one small kernel that clears the
 * batch's histograms; THREE sweeps over the data — a radix select on the key with digits of 11 / 11 / 10 bits, a workgroup
 * owning one column and one particle block — and a one-workgroup-per-column pick kernel after each, which scans the
 * column's histograms, finds every target rank's bin and its rank inside that bin, merges equal bins into SLOTS (at most
 * 2 Q) and, after the last sweep, writes the outputs.  Sweeps 1 and 2 histogram only the entries whose prefix is one of the
 * column's slots, GJX_QUANTILES_SLOTS_PER_LAUNCH slots per launch (one LDS histogram each), and run again per four slots:
 * ceil(2 Q / 4) launches each, of which a column with fewer slots leaves all but the first at once.
 *
 * WEIGHTED COLUMNS (GJX_QUANTILES_WEIGHTED; the version stays 0.1: the addition changes no declaration and no struct layout
 * above, a C client detects it by the macro).  gjx_weighted_column_quantiles weighs entry i of data column c by the
 * log-weight logw[(c % V) * logw_stride + i], V = n_weight_cols: V = 1 is one weight vector for all columns (the weighted
 * paths of a trace-back), V = T with K segments of T columns a K-component carry's history against its T rows of
 * log-weights.  What SMCResult.summary and Trajectories.summary ask of the library.  The radix select above counts entries;
 * this one accumulates MASS, the max-anchored fixed-point weight of gjx.h — an integer, so a histogram of masses is
 * order-independent.  Specification (exact; per data column c with its weight column v = c % V):
 *
 *   mass      m_v = the maximum over the non-NaN log-weights of column v (as gjx_max_f32 skips NaNs; -inf if there is none),
 *             q_i = fixw(lw_i, m_v, F), F = min(gjx_frac_bits(n), 31): rint(exp(lw_i - m_v) 2^F) in the f32 arithmetic of
 *             gjx.h, exactly 2^F where lw_i == m_v.  q_i <= 2^31 fits a u32 and a column's total stays below 2^62.  A NaN,
 *             a -inf (also where it is the maximum) and anything more than 80 below the maximum weigh 0.  mass_out, where
 *             given, receives q as u32 [V][n].
 *   valid     an entry counts if its x is not NaN; nan = the number of NaN entries; W = the sum of q_i over the valid entries,
 *             an exact u64.
 *   target    T_j = min(max(ceil(p_j * (double) W), 1), W): one conversion, one float64 product, one ceil.
 *   quant     quant[c][j] = the f32 value, bit for bit, of the first entry, ascending in the key above, whose inclusive
 *             cumulative mass reaches T_j (entries of equal key are interchangeable): the inverted-CDF rule.  An entry of
 *             mass 0 is never returned.  W = 0: NaN (0x7FC00000).
 *   stats     stats[c][0 .. 5], f64: nan, mean, variance, min, max, ess; all but nan are NaN for W = 0.  min / max are over the
 *             valid entries of positive mass, so p = 0 returns min and p = 1 max.  With the sums over the valid entries of
 *             positive mass (a zero mass adds nothing, also before an infinite x):
 *               S1 = sum (double) q_i * (double) x_i,                     mean = S1 / (double) W
 *               S2 = sum (double) q_i * (((double) x_i - mean)^2),        variance = S2 / (double) W  (the population form: a
 *                    weighted sample has no m - 1), taken in a later sweep
 *               S0 = sum (double) q_i * (double) q_i,                     ess = (double) W * (double) W / S0
 *             every product and sum rounding once, no FMA, in the fixed order above: blocks (the same B), head / quads /
 *             tail by the DATA column's base, lanes, balanced tree, fold in index order.
 *   No floating-point atomics: quant, nan, min, max and mass_out are bit-equal whatever max_workgroups is; mean, variance and
 *   ess at equal max_workgroups.
 *
 * LAUNCHES, per batch: the clear, a PROLOGUE of two kernels — each weight column's maximum, then the u32 mass table (in the
 * workspace, or in mass_out) so that a mass is evaluated once and a sweep streams 8 bytes per entry — and three sweeps on
 * 12 / 10 / 10 key bits with u64 bins (4096 bins, then four slots of 1024: 32 KiB of LDS each), a pick kernel after each.
 * There is one target per probability: at most Q slots, ceil(Q / 4) launches of sweeps 1 and 2.
 */
#ifndef GJX_QUANTILES_H
#define GJX_QUANTILES_H

#include "gjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_QUANTILES_VERSION_MAJOR 0
#define GJX_QUANTILES_VERSION_MINOR 1

#define GJX_QUANTILES_MAX_PROBS 8
#define GJX_QUANTILES_MAX_SEGMENTS 32
#define GJX_QUANTILES_SLOTS_PER_LAUNCH 4
#define GJX_QUANTILES_BATCH_COLS 256 /* columns of one batch: the workspace does not grow beyond them */
#define GJX_QUANTILES_WEIGHTED 1     /* gjx_weighted_column_quantiles and its size function are declared below */

typedef struct {
  const float* base; /* dev f32: column j of the segment starts at base + j * stride */
  uint32_t n_cols;   /* 1 .. */
  uint64_t stride;   /* elements; >= n where n_cols > 1 */
} gjx_column_segment;

typedef struct {
  uint64_t n;                                          /* entries per column, 1 .. 2^31 - 1 */
  int32_t n_segments;                                  /* 1 .. GJX_QUANTILES_MAX_SEGMENTS */
  gjx_column_segment seg[GJX_QUANTILES_MAX_SEGMENTS];  /* n_cols = the sum of their n_cols, at most 2^31 - 1 */
  int32_t n_probs;                                     /* Q: 1 .. GJX_QUANTILES_MAX_PROBS */
  const double* probs;                                 /* HOST f64[Q], each in [0, 1] */
  float* bracket;                                      /* dev f32[n_cols][Q][2] */
  double* quant;                                       /* dev f64[n_cols][Q] */
  double* stats;                                       /* dev f64[n_cols][5]: nan, mean, variance, min, max */
  void* ws;                                            /* dev, 8-byte aligned; no word of it has to be zero */
  size_t ws_bytes;
  uint32_t max_workgroups;                             /* 0: the library's split (above); a test knob */
} gjx_column_quantiles_io;

int gjx_quantiles_version(int* major, int* minor);
/* 0 for whatever gjx_column_quantiles refuses by its shape: n outside 1 .. 2^31 - 1, n_cols outside 1 .. 2^31 - 1, n_probs
 * outside 1 .. GJX_QUANTILES_MAX_PROBS.  Grows with n_cols up to GJX_QUANTILES_BATCH_COLS columns and no further. */
size_t gjx_quantiles_workspace_bytes(uint64_t n, uint32_t n_cols, int32_t n_probs);
/* Per batch 5 + 2 ceil(2 Q / 4) launches on stream s.
 * GJX_ERR_INVALID (nothing launched): a NULL io / probs / output / segment base, n, n_segments, a segment's n_cols, the
 * columns' total or n_probs out of range, a stride below n in a segment of several columns, a probability outside [0, 1]
 * or NaN, ws not 8-byte aligned.
 * GJX_ERR_WORKSPACE: ws NULL or smaller than gjx_quantiles_workspace_bytes(n, n_cols, n_probs). */
int gjx_column_quantiles(const gjx_column_quantiles_io* io, gjx_stream s);

typedef struct {
  uint64_t n;                                          /* as gjx_column_quantiles_io */
  int32_t n_segments;
  gjx_column_segment seg[GJX_QUANTILES_MAX_SEGMENTS];
  const float* logw;                                   /* dev f32: weight column v starts at logw + v * logw_stride */
  uint32_t n_weight_cols;                              /* V: 1 .. n_cols; data column c is weighed by weight column c % V */
  uint64_t logw_stride;                                /* elements; >= n where V > 1 */
  int32_t n_probs;                                     /* Q: 1 .. GJX_QUANTILES_MAX_PROBS */
  const double* probs;                                 /* HOST f64[Q], each in [0, 1] */
  float* quant;                                        /* dev f32[n_cols][Q]: an ENTRY of the column, bit for bit */
  double* stats;                                       /* dev f64[n_cols][6]: nan, mean, variance, min, max, ess */
  uint32_t* mass_out;                                  /* dev u32[V][n], nullable: the masses q_i every sum is over */
  void* ws;                                            /* dev, 8-byte aligned; no word of it has to be zero */
  size_t ws_bytes;
  uint32_t max_workgroups;                             /* as gjx_column_quantiles_io */
} gjx_weighted_quantiles_io;

/* 0 for whatever gjx_weighted_column_quantiles refuses by its shape: as gjx_quantiles_workspace_bytes, and n_weight_cols
 * outside 1 .. n_cols.  No growth beyond GJX_QUANTILES_BATCH_COLS columns. */
size_t gjx_weighted_quantiles_workspace_bytes(uint64_t n, uint32_t n_cols, uint32_t n_weight_cols, int32_t n_probs);
/* Per batch 7 + 2 ceil(Q / 4) launches on stream s.
 * GJX_ERR_INVALID (nothing launched): what gjx_column_quantiles refuses, a NULL logw, n_weight_cols outside 1 .. n_cols,
 * logw_stride < n where n_weight_cols > 1.  GJX_ERR_WORKSPACE: ws NULL or smaller than the size function's answer. */
int gjx_weighted_column_quantiles(const gjx_weighted_quantiles_io* io, gjx_stream s);

#ifdef __cplusplus
}
#endif
#endif /* GJX_QUANTILES_H */
