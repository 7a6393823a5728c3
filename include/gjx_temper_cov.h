/*
 * gjx_temper_cov.h — full-covariance proposals for the tempered move: the one-launch weighted moments of a population with
 * the proposal factor built on the device, and the move kernel that proposes through that factor.
 *
 * An ELEVENTH header next to gjx.h (after gjx_paths.h, gjx_guided.h, gjx_backsim.h, gjx_backmove.h, gjx_smc_params.h,
 * gjx_csmc.h, gjx_temper.h, gjx_plate.h and gjx_pointwise.h), with a version of its own and for the same reason: gjx.h is
 * the boundary the CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points, the oracle library does
 * not, and a binding loads them if present.  Conventions (status codes, gjx_stream, borrowed "dev" pointers, no allocation,
 * no host synchronisation) are those of gjx.h.
 *
 * gjx_temper_move proposes x'_l = x_l + scales[l] * eps_l: a diagonal random walk.  On a posterior whose latents are
 * correlated (a regression over a design that is not centred) such a walk is accepted only at steps far below the
 * posterior's width and the population stops moving.  gjx_temper_move_cov proposes x' = x + F eps with a lower-triangular
 * F; gjx_temper_moments builds F = 2.38 / sqrt(L) times the Cholesky factor of the weighted covariance of the population
 * (Roberts, Gelman & Gilks 1997; Chopin 2002) in ONE launch whose outputs stay on the device, so that a stage makes no
 * host read for its proposal.
 *
 * PACKING.  A lower triangle is packed by rows: entry (l, j), j <= l, at l (l + 1) / 2 + j; L (L + 1) / 2 entries.
 *
 * THE MOMENTS (exact: the result is a function of the inputs alone, bit for bit, whatever the grid).
 *
 *   weights   the ladder's (gjx_temper.h).  The population is cut into W = gjx_temper_ladder_blocks(n) contiguous blocks of
 *             per = ceil(n / W) entries.  Block b has m_b = the maximum of its lw entries above -inf (a NaN is skipped; -inf
 *             when there is none) and e_i = (double) exp_f32(f32(lw_i - m_b)) (the spec's f32 exp) for an entry above -inf,
 *             e_i = 0 otherwise.  lw == NULL is equal weights: m_b = 0 and e_i = 1.
 *   terms     with d_l(i) = (double) x_l[i] - (double) x_l[0] (the shift by particle 0 keeps float64 cancellation harmless
 *             when a mean is large against its deviation), P = 1 + L + L (L + 1) / 2 sums are kept, numbered
 *                 p = 0:                         e_i
 *                 p = 1 + l:                     e_i d_l(i)
 *                 p = 1 + L + l (l + 1) / 2 + j: (e_i d_l(i)) d_j(i)            j <= l, every product rounded once.
 *             An entry with e_i = 0 (a weight of -inf or NaN, or an exponential that underflowed) adds nothing, whatever
 *             its x.
 *   a block   is walked in TILES of 256 consecutive entries.  A tile is cut into Q segments of 256 / Q consecutive entries,
 *             Q = the largest power of two <= 256 / P (a function of L alone: 32 at L = 2, 8 at L = 5, 1 from L = 11 on).
 *             Sum (p, q) of block b = the float64 sum, from +0, of term p over the entries of segment q of tile 0 in index
 *             order, then of segment q of tile 1, and so on (one accumulator through the block).  The block's sum p is
 *             ((s(p, 0) + s(p, 1)) + ...) + s(p, Q - 1).
 *   the fold  the workgroup that finishes last (a ticket, as in gjx_temper_ess_ladder) folds the blocks IN INDEX ORDER in
 *             float64: M = max_b m_b, f_b = exp((double) m_b - (double) M) (the double exp; 0 for m_b = -inf),
 *             T_p = sum_b f_b * s_b(p) from +0, every product and sum rounded once.  Then, each operation rounded once:
 *                 moments[0]     = T_0                                       the weight sum relative to the maximum
 *                 a_l            = T_{1 + l} / T_0
 *                 moments[1 + l] = (double) x_l[0] + a_l                     the weighted mean
 *                 S_lj           = T_{1 + L + l (l + 1) / 2 + j} / T_0 - a_l * a_j      moments[1 + L + ...], packed
 *                 scales[l]      = f32(c * sqrt(S_ll)) where S_ll > 0, else 0;   c = 2.38 / sqrt((double) L).
 *             If no entry is above -inf (M = -inf): every output is 0 and n_degenerate = L.
 *   factor    by one lane, in float64, every operation rounded once and never contracted, in this order:
 *                 for l = 0 .. L-1:
 *                   for j = 0 .. l-1:  t = +0;  t = t + G_lk * G_jk for k = 0 .. j-1 in order;
 *                                      G_lj = G_jj == 0 ? 0 : (S_lj - t) / G_jj
 *                   t = +0;  t = t + G_lk * G_lk for k = 0 .. l-1 in order;  p = S_ll - t
 *                   if !(p > 2^-40 * S_ll):  row l = (0, ..., 0, S_ll > 0 and finite ? sqrt(S_ll) : 0) — the latent moves
 *                                      on its own at its own deviation, or stays put — and n_degenerate goes up by one;
 *                   otherwise G_ll = sqrt(p).
 *                 factor = f32(c * G), packed.
 *             (A row whose divisor G_jj is 0 takes G_lj = 0: column j belongs to a latent that stays put.)
 *
 * ONE launch of fixed device code.  A workgroup stages a tile (256 particles x L deviations and their weights, float64) in
 * LDS, lane t sums pair t mod P over segment t / P: every column is read from memory once per launch, 4 (L + 1) bytes per
 * particle, after the pass over lw that finds m_b.
 *
 * THE MOVE.  gjx_temper_move_cov is gjx_temper_move (gjx_temper.h: start, keys, assess, energy, uniform, accept, output, the
 * clamp of ancestor words, the Gamma / Beta support rule, plated sites — word for word) with ONE change:
 *     propose   eps_l = element i of the value gjx_sample_logpdf_normal returns for the key batch {mode 1 (lazy split),
 *               parent p_r, first 0, has_fold 1, fold = l + 1 (THREEFRY) / l (PHILOX)}, loc = 0, scale = 1, n — the key
 *               batches and folds of gjx_temper_move's proposal;
 *               t_l = f32(F[l][0] * eps_0);  t_l = f32(t_l + f32(F[l][j] * eps_j)) for j = 1 .. l in order: products and sums
 *               round once each, no FMA;  x'_l = f32(x_l + t_l).
 * io->scales is not read.  The kernel forms eps_l = f32(+0 + z_l) from the draw z_l of the generator it shares with
 * gjx_sample_logpdf_normal: that entry point returns f32(0 + f32(1 * z)), and 1 * z is z, so the two agree bit for bit — the
 * addition of +0 is kept because it turns a draw of -0 into +0, the only value it changes.
 * F is read through the scalar cache (wave-uniform); it must not be written while the launch runs.  A diagonal F with
 * F[l][l] = scales[l] gives gjx_temper_move's outputs bit for bit wherever no draw and no latent is a zero.
 */
#ifndef GJX_TEMPER_COV_H
#define GJX_TEMPER_COV_H

#include "gjx_temper.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_TEMPER_COV_VERSION_MAJOR 0
#define GJX_TEMPER_COV_VERSION_MINOR 1

typedef struct {
  uint64_t n;                              /* particles, 1 .. 2^31 - 1 */
  int32_t n_latents;                       /* L, 1 .. GJX_TEMPER_MAX_LATENTS */
  const float* x[GJX_TEMPER_MAX_LATENTS];  /* dev f32[n] per latent */
  const float* lw;                         /* dev f32[n] log-weights, nullable: equal weights */
  double* moments;                         /* dev f64[1 + L + L (L + 1) / 2] */
  float* factor;                           /* dev f32[L (L + 1) / 2] */
  float* scales;                           /* dev f32[L] */
  uint32_t* n_degenerate;                  /* dev u32[1] */
  void* ws;                                /* dev, 8-byte aligned; its first 8 bytes hold the ticket: ZERO before the first
                                              call, left zero by every call (calls that share it must be stream-ordered) */
  size_t ws_bytes;
  uint32_t max_workgroups;                 /* 0: the library's choice (a test knob: nothing depends on it) */
} gjx_temper_moments_io;

int gjx_temper_cov_version(int* major, int* minor);
/* 0 for n outside 1 .. 2^31 - 1 or n_latents outside 1 .. GJX_TEMPER_MAX_LATENTS. */
size_t gjx_temper_moments_workspace_bytes(uint64_t n, int32_t n_latents);
/* ONE launch on stream s.
 * GJX_ERR_INVALID (nothing launched): a NULL io / latent column / output, n 0 or >= 2^31, n_latents out of range, ws not
 * 8-byte aligned.  GJX_ERR_WORKSPACE: ws NULL or smaller than gjx_temper_moments_workspace_bytes(n, n_latents). */
int gjx_temper_moments(const gjx_temper_moments_io* io, gjx_stream s);
/* ONE launch: gjx_temper_move with the proposal above.  factor: dev f32[L (L + 1) / 2], L the plan's latents.
 * GJX_ERR_INVALID (nothing launched): a NULL factor, and whatever gjx_temper_move refuses (io->scales may be NULL).
 * GJX_ERR_UNSUPPORTED / GJX_ERR_JIT as gjx_temper_move. */
int gjx_temper_move_cov(gjx_temper_plan* p, const gjx_temper_io* io, const float* factor, gjx_stream s);
/* The HIP source of the plan's generated covariance move kernel for impl 0 / 1 (it holds no parameter, observation or
 * factor value). */
int gjx_temper_cov_source(const gjx_temper_plan* p, int impl, char* buf, size_t buf_len, size_t* needed);
/* Compiles that source for gfx950 without touching a GPU: GJX_OK, or GJX_ERR_UNSUPPORTED when it does not compile. */
int gjx_temper_cov_compile_check(const gjx_temper_plan* p, int impl);

#ifdef __cplusplus
}
#endif
#endif /* GJX_TEMPER_COV_H */
