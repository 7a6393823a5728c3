/*
 * gjx_group.h — grouped latents in a tempered plan: per-group effects over a sorted group column.
 *
 * A FIFTEENTH header next to gjx.h, with a version of its own and for the same reason as the others: gjx.h is the boundary the
 * CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points, the oracle library does not, and a binding
 * loads them if present.  Conventions (status codes, gjx_stream, borrowed "dev" pointers, no allocation, no host
 * synchronisation) are those of gjx.h.
 *
 * A tempered plan (gjx_temper.h) keeps at most GJX_TEMPER_MAX_LATENTS scalar latents in registers.  A GROUPED site is a latent
 * with G components z[g], g = 0 .. G-1, i.i.d. given the scalar latents, kept in a device column [G][n] per site.  Row d of
 * the data table (gjx_plate.h) belongs to group g(d); the rows of a group are CONTIGUOUS: group g owns the rows
 * offsets[g] .. offsets[g + 1] - 1.  A plated site may read z[ref][g(d)] at row d.  In the move kernel a lane is a particle and
 * rows are wave-uniform, so every lane works on the same group at the same moment: a Metropolis-within-Gibbs move of z[g]
 * needs the rows of group g only, and a sweep over all G groups costs O(n_rows), not O(G n_rows).
 *
 *   GJX_SITE_GROUPED (gjx_site.observed == 5)  a latent site with G components (Normal, Gamma or Beta).  Its arguments are
 *                                              constants, parameters, scalar latent sites or programs over those.
 *   GJX_ARG_GROUP    (gjx_arg.kind == 10)      value = scale * z[ref][g(d)] + offset.
 *   GJX_EXPR_GROUP   (gjx_expr_op.op == 22)    push z[ref][g(d)].
 * `ref` is the grouped site's index among the grouped sites in table order (S of them, S <= GJX_GROUP_MAX_SITES).  GROUP
 * operands are valid in a0 and a1 of a PLATED site only, after the grouped site they name.  Every other creator (gjx_plan_create*,
 * gjx_smc_plan_create*, gjx_scan_plan_create*, gjx_backsim_plan_create, gjx_temper_plan_create, gjx_temper_plan_create_plated,
 * gjx_temper_plan_create_counts) refuses mode 5 and both GROUP kinds.
 *
 * Specification (exact, bit for bit: a function of the inputs and the keys alone).  x: the L scalar latents; z: the S grouped
 * columns.  A "group-reading" site is a PLATED site with a GROUP operand; a "flat" site is every other site but the grouped.
 *
 *   assess(x, z)  lp_flat, ll_flat = the f32 sums of gjx_temper.h / gjx_plate.h over the flat sites in table order (a flat
 *                 plated site keeps its float64 row rule).
 *                 lpz_g = the f32 sum from +0, in table order over the grouped sites s, of the site's log-density at z[s][g]
 *                 (the entry points gjx_logpdf_normal / _gamma / _beta at the site's arguments; -inf outside the OPEN
 *                 support and for NaN, as for a scalar latent).  LZ = the float64 sum over g = 0 .. G-1, in order, of
 *                 (double) lpz_g.
 *                 acc_g = the float64 sum from +0.0 over the rows d of group g, in order; within a row over the group-reading
 *                 sites in table order: acc = acc + (double) t, t the f32 log-density of gjx_plate.h at row d with
 *                 z[ref][g] for every GROUP operand.  A = the float64 sum over g, in order, of acc_g.
 *                 lp = f32(lp_flat + (float) LZ),  ll = f32(ll_flat + (float) A).
 *   start         a = the ancestor of gjx_temper.h; x_l = x_in[l][a]; z_out[s][g][i] = z_in[s][g][a] for all s, g: the gather,
 *                 done once — everything after works in place on lane i's own entries of z_out.
 *                 init != 0: z_in is not read; z[s][g] = element i of the value gjx_sample_logpdf_<dist> returns for the
 *                 site's arguments at the particle's scalars and the key batch {mode 1 (lazy split), parent
 *                 fold_in(init_key, g), first 0, has_fold 1, fold = s + 1 (THREEFRY) / s (PHILOX)}: the numbering of a plan
 *                 whose sites are the S grouped sites.
 *                 recompute != 0: (lp, ll) = assess(x, z); otherwise lp = lp_in[a], ll = ll_in[a].  lp_flat and ll_flat are
 *                 evaluated from x whenever n_moves > 0.
 *   sweep r       k_r, p_r, a_r as in gjx_temper.h.
 *     scalars     the rule of gjx_temper.h: propose all L scalars, (lp', ll') = assess(x', z) in full, h, h', d, the uniform
 *                 and the accept test as there.  On accept (x, lp, ll) = (x', lp', ll') and lp_flat, ll_flat are the
 *                 proposal's.
 *     groups      for g = 0 .. G-1, in order: kg = fold_in(fold_in(k_r, 2), g), proposal key fold_in(kg, 0), acceptance key
 *                 fold_in(kg, 1) (both lane 0).
 *                 z'_s = f32(z_s + f32(z_scales[s][g] * eps_s)), eps_s = element i of the standard Normal batch of the
 *                 proposal key with fold = s + 1 (THREEFRY) / s (PHILOX), as a scalar proposal takes its draw.
 *                 lpz_g, acc_g at z and lpz'_g, acc'_g at z' are evaluated FRESH over the group's rows, in one pass.
 *                 d = f32(f32(lpz'_g - lpz_g) + f32(beta * (float)(acc'_g - acc_g))): every operation rounds once, no FMA
 *                 (the difference of the two float64 sums is taken in float64).
 *                 The uniform of the acceptance key as in gjx_temper.h; accept iff d >= 0 || l < d (false on NaN).
 *                 On accept z[.][g] = z', the particle's group accept count goes up by one, and lpz'_g / acc'_g enter the
 *                 running float64 sums LZ and A; otherwise lpz_g / acc_g do.
 *     totals      lp = f32(lp_flat + (float) LZ), ll = f32(ll_flat + (float) A): by the sum order above this is assess(x, z)
 *                 of the new state exactly.
 *   output        x_out, z_out (in place), lp_out, ll_out, n_accept (scalar phase), n_accept_z (group phase, summed over g).
 *
 * A row bound read from `offsets` is clamped to n_rows before it is used: no address is formed from an unchecked word.
 * Nothing depends on the grid size.  z_out must not overlap z_in (another lane reads it).
 */
#ifndef GJX_GROUP_H
#define GJX_GROUP_H

#include "gjx_plate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_GROUP_VERSION_MAJOR 0
#define GJX_GROUP_VERSION_MINOR 1

#define GJX_SITE_GROUPED 5 /* gjx_site.observed (GJX_SITE_PLATED is 4) */
#define GJX_ARG_GROUP 10   /* gjx_arg.kind (GJX_ARG_DATA is 9) */
#define GJX_EXPR_GROUP 22  /* gjx_expr_op.op (GJX_EXPR_DATA is 21) */
#define GJX_GROUP_MAX_SITES 4
#define GJX_GROUP_MAX_GROUPS 16777216 /* G < 2^24 */

typedef struct {
  gjx_temper_io t;                            /* as gjx_temper_move reads it (scales: the L scalar latents') */
  const float* z_in[GJX_GROUP_MAX_SITES];     /* dev f32[G][n] per grouped site; not read (nullable) when init != 0 */
  float* z_out[GJX_GROUP_MAX_SITES];          /* dev f32[G][n] per grouped site */
  const float* z_scales[GJX_GROUP_MAX_SITES]; /* dev f32[G] per grouped site; nullable when n_moves == 0 */
  int32_t* n_accept_z;                        /* dev int32[n], nullable */
  int32_t init;                               /* != 0: draw z from the grouped sites' priors */
  uint32_t init_key[2];
  uint64_t init_key_lane;                     /* PHILOX: the key's lane (0 for THREEFRY) */
} gjx_group_io;

int gjx_group_version(int* major, int* minor);
/* As gjx_temper_plan_create_plated, with GROUPED sites and GROUP operands accepted; a table without a grouped site gives the
 * plan (and the generated source, byte for byte) gjx_temper_plan_create_plated gives.  A table WITH one may also hold the
 * count sites of gjx_counts.h, as gjx_temper_plan_create_counts accepts them.
 * GJX_ERR_INVALID: whatever that creator refuses; more than GJX_GROUP_MAX_SITES grouped sites; a grouped site that is not
 * Normal / Gamma / Beta or whose arguments read data, a grouped value, or a site that is not a scalar latent; a GROUP operand
 * outside a0 / a1 of a PLATED site or with ref not below the number of grouped sites before it; in a table with a grouped
 * site, ANY site (a flat one included) that refers to a site that is not a scalar latent, or that reads a per-particle
 * input column (the device functions of the grouped kernel define the scalar latents' values alone); a grouped site
 * without any group-reading site. */
int gjx_temper_plan_create_grouped(const gjx_site* sites /*host*/, int n_sites, uint32_t flags, gjx_temper_plan** out);
/* The groups of the launches that follow: offsets dev int32[G + 1], BORROWED.  The caller guarantees offsets[0] == 0, that
 * the offsets are non-decreasing and that offsets[G] == n_rows (the kernel clamps what it reads).
 * GJX_ERR_INVALID: a NULL plan / pointer, a plan without grouped sites, G outside 1 .. 2^24 - 1. */
int gjx_temper_plan_set_groups(gjx_temper_plan* p, const int32_t* offsets /*dev*/, uint32_t G);
int gjx_temper_plan_n_grouped(const gjx_temper_plan* p);
/* ONE launch: one lane per particle, no LDS, no barrier; the kernel is generated from the table (gjx_temper_plan_source and
 * gjx_temper_plan_compile_check give and check it for a grouped plan).
 * GJX_ERR_INVALID (nothing launched): whatever gjx_temper_move refuses; a plan without grouped sites; a grouped plan without
 * groups or data; a NULL z_out[s]; a NULL z_in[s] with init == 0; a NULL z_scales[s] with n_moves > 0; init != 0 with a key
 * lane under THREEFRY.  gjx_temper_move and gjx_temper_move_cov refuse a grouped plan (GJX_ERR_INVALID), and so do the entry
 * points of gjx_pointwise.h, gjx_predictive.h and gjx_psis.h. */
int gjx_temper_move_grouped(gjx_temper_plan* p, const gjx_group_io* io, gjx_stream s);

#ifdef __cplusplus
}
#endif
#endif /* GJX_GROUP_H */
