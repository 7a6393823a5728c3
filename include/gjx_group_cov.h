/*
 * gjx_group_cov.h — per-group covariance proposals for the grouped latents of a tempered plan: the weighted moments of every
 * group's S components with one S x S proposal factor per group built on the device, and the grouped move that proposes
 * through those factors (block-diagonal: one L x L factor for the scalars, one S x S factor per group).
 *
 * An EIGHTEENTH header next to gjx.h, with a version of its own and for the same reason as the others: gjx.h is the boundary
 * the CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points, the oracle library does not, and a
 * binding loads them if present.  Conventions (status codes, gjx_stream, borrowed "dev" pointers, no allocation, no host
 * synchronisation) are those of gjx.h.
 *
 * The group phase of gjx_temper_move_grouped (gjx_group.h) proposes z'_s = z_s + z_scales[s][g] * eps_s: a diagonal walk over
 * the S components of a group.  A random intercept and a random slope per group over a covariate that is not centred are
 * correlated near -1 inside every group, and that walk stalls as the diagonal walk over the scalars does (gjx_temper_cov.h).
 *
 * PACKING.  The lower triangle of gjx_temper_cov.h, per group: entry (s, j), j <= s, of group g at
 * g * S (S + 1) / 2 + s (s + 1) / 2 + j.
 *
 * THE MOMENTS (exact: a function of the inputs alone, bit for bit, whatever the grid).  The rules of gjx_temper_cov.h with L
 * replaced by S and x_l by z[s][g][.], once per group g:
 *
 *   weights   word for word those of gjx_temper_cov.h: W = gjx_temper_ladder_blocks(n) contiguous blocks of per = ceil(n / W)
 *             entries, m_b, e_i = (double) exp_f32(f32(lw_i - m_b)), 0 for -inf and NaN; lw == NULL: m_b = 0, e_i = 1.  The
 *             weights do not depend on the group.
 *   terms     d_s(i) = (double) z[s][g][i] - (double) z[s][g][0];  P = 1 + S + S (S + 1) / 2 sums (at most 15), numbered as
 *             there: e_i;  e_i d_s(i);  (e_i d_s(i)) d_j(i), j <= s, every product rounded once.  An entry with e_i = 0 adds
 *             nothing, whatever its z.
 *   a block   LANE t of 256 owns the block's entries lo + t, lo + t + 256, ... and sums term p over them from +0 in index
 *             order (one float64 accumulator through the block).  The block's sum p is the BALANCED TREE over the 256 lane
 *             sums in lane order: level k = 0 .. 7 adds the sums of the two adjacent aligned runs of 2^k lanes
 *             (((l_0 + l_1) + (l_2 + l_3)) + ...).  This differs from the segment rule of gjx_temper_cov.h on purpose: a lane
 *             reads its entries from memory in coalesced rows and keeps its P sums in registers, nothing is staged but the
 *             weights.
 *   the fold  per group, the blocks IN INDEX ORDER in float64 as there: M = max_b m_b, f_b = exp((double) m_b - (double) M)
 *             (0 for m_b = -inf), T_p = sum_b f_b * s_b(p) from +0, every product and sum rounded once.  Then
 *                 a_s = T_{1 + s} / T_0;   S_sj = T_{1 + S + s (s + 1) / 2 + j} / T_0 - a_s * a_j
 *                 scales[s][g] = f32(c * sqrt(S_ss)) where S_ss > 0, else 0;   c = 2.38 / sqrt((double) S).
 *   factor    the recursion of gjx_temper_cov.h word for word (the 2^-40 fallback-row rule included), factor = f32(c * G).
 *             A group whose weight sum is 0 (no entry above -inf) gets a zero factor, zero scales and S degenerate rows.
 *   n_degenerate[0] = the fallback rows summed over the groups.
 *
 * TWO launches of fixed device code, no floating-point atomic, no host read.  (1) A workgroup owns one particle block b and a
 * range of groups: one pass over lw[block] for m_b, the block's e_i staged ONCE in LDS as f32 (exact: they come from the f32
 * exp), then per group of its range the lanes walk the block with coalesced loads of z[s][g][i], P float64 accumulators per
 * lane in registers, ONE cross-lane reduction per (group, block), the block's sums to the workspace [G][W][P].  Every z
 * value is read from memory once.  (2) One lane per group folds the blocks in index order and builds the factor.  A second
 * launch was chosen over the last-workgroup ticket of gjx_temper_moments: the fold is G independent serial chains of W
 * steps, which one workgroup would run 256 at a time while the device idles, and the workspace needs no word that must be
 * zero between calls.
 * A block must fit in LDS: per <= GJX_GROUP_MOMENTS_MAX_BLOCK, that is n <= 256 * GJX_GROUP_MOMENTS_MAX_BLOCK = 4 096 000.
 * The workspace holds 8 P W bytes per group (30 KiB at S = 4, n >= 65536): gjx_group_moments_workspace_bytes grows linearly
 * in G, 1 GiB at G = 87 000 for S = 2.
 *
 * THE MOVE.  gjx_temper_move_grouped_cov is gjx_temper_move_grouped (gjx_group.h: start, gather, init, keys, assess, energy,
 * uniform, accept, the float64 sums, totals, outputs — word for word) with TWO changes:
 *     groups    eps_s = f32(+0 + the draw z'_s's proposal takes there) (same key batch and fold), Fg = the packed row of
 *               factor_z of group g;  t_s = f32(Fg[s][0] * eps_0);  t_s = f32(t_s + f32(Fg[s][j] * eps_j)) for j = 1 .. s in
 *               order: products and sums round once each, no FMA;  z'_s = f32(z_s + t_s).  io->z_scales is not read.
 *     scalars   factor_x != NULL: the proposal of gjx_temper_move_cov (x' = x + F eps, its rounding rule), io->t.scales is not
 *               read.  factor_x == NULL: unchanged, with io->t.scales.
 * Both factors are wave-uniform and read through the scalar cache; they must not be written while the launch runs.  A
 * diagonal factor_z with Fg[s][s] = z_scales[s][g] (and a diagonal factor_x with F[l][l] = scales[l], or NULL) gives
 * gjx_temper_move_grouped's outputs bit for bit wherever no draw and no latent is a zero.
 */
#ifndef GJX_GROUP_COV_H
#define GJX_GROUP_COV_H

#include "gjx_group.h"
#include "gjx_temper_cov.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_GROUP_COV_VERSION_MAJOR 0
#define GJX_GROUP_COV_VERSION_MINOR 1

#define GJX_GROUP_MOMENTS_MAX_BLOCK 16000 /* entries of one particle block: its f32 weights fit in 64 000 bytes of LDS */

typedef struct {
  uint64_t n;                            /* particles, 1 .. 256 * GJX_GROUP_MOMENTS_MAX_BLOCK */
  uint32_t G;                            /* groups, 1 .. 2^24 - 1 */
  int32_t S;                             /* grouped sites, 1 .. GJX_GROUP_MAX_SITES */
  const float* z[GJX_GROUP_MAX_SITES];   /* dev f32[G][n] per grouped site */
  const float* lw;                       /* dev f32[n] log-weights, nullable: equal weights */
  float* factor;                         /* dev f32[G][S (S + 1) / 2] */
  float* scales;                         /* dev f32[S][G] */
  uint32_t* n_degenerate;                /* dev u32[1] */
  void* ws;                              /* dev, 8-byte aligned; no word of it has to be zero */
  size_t ws_bytes;
  uint32_t max_workgroups;               /* 0: the library's choice (a test knob: nothing depends on it) */
} gjx_group_moments_io;

int gjx_group_cov_version(int* major, int* minor);
/* 0 for whatever gjx_group_moments refuses by its shape: n outside 1 .. 256 * GJX_GROUP_MOMENTS_MAX_BLOCK, G outside
 * 1 .. 2^24 - 1, S outside 1 .. GJX_GROUP_MAX_SITES. */
size_t gjx_group_moments_workspace_bytes(uint64_t n, uint32_t G, int32_t S);
/* TWO launches on stream s.
 * GJX_ERR_INVALID (nothing launched): a NULL io / column / output, n, G or S out of range, ws not 8-byte aligned.
 * GJX_ERR_WORKSPACE: ws NULL or smaller than gjx_group_moments_workspace_bytes(n, G, S). */
int gjx_group_moments(const gjx_group_moments_io* io, gjx_stream s);
/* ONE launch: gjx_temper_move_grouped with the proposals above.  factor_x: dev f32[L (L + 1) / 2], nullable; factor_z: dev
 * f32[G][S (S + 1) / 2], G the plan's groups.
 * GJX_ERR_INVALID (nothing launched): whatever gjx_temper_move_grouped refuses (io->z_scales may be NULL, and io->t.scales
 * with a factor_x), a plan without grouped sites, a NULL factor_z with n_moves > 0.
 * GJX_ERR_UNSUPPORTED / GJX_ERR_JIT as gjx_temper_move. */
int gjx_temper_move_grouped_cov(gjx_temper_plan* p, const gjx_group_io* io, const float* factor_x, const float* factor_z, gjx_stream s);
/* The HIP source of the grouped plan's generated block move kernel for impl 0 / 1 (it holds no parameter, observation, group
 * count or factor value).  GJX_ERR_INVALID for a plan without grouped sites. */
int gjx_group_cov_source(const gjx_temper_plan* p, int impl, char* buf, size_t buf_len, size_t* needed);
/* Compiles that source for gfx950 without touching a GPU: GJX_OK, or GJX_ERR_UNSUPPORTED when it does not compile. */
int gjx_group_cov_compile_check(const gjx_temper_plan* p, int impl);

#ifdef __cplusplus
}
#endif
#endif /* GJX_GROUP_COV_H */
