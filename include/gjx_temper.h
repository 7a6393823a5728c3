/*
 * gjx_temper.h — tempered SMC for static models: the fused resample-move launch and the one-launch ESS ladder.
 *
 * An EIGHTH header next to gjx.h (after gjx_paths.h, gjx_guided.h, gjx_backsim.h, gjx_backmove.h, gjx_smc_params.h and
 * gjx_csmc.h), with a version of its own and for the same reason: gjx.h is the boundary the CPU oracle restates symbol for
 * symbol.  libgjx_hip.so exports these entry points, the oracle library does not, and a binding loads them if present.
 * Conventions (status codes, gjx_stream, borrowed "dev" pointers, no allocation, no host synchronisation) are those of
 * gjx.h.
 *
 * A tempered sampler (Neal 2001; Del Moral, Doucet & Jasra 2006) walks a population from the prior to the posterior of a
 * static model through the targets  prior(x) * likelihood(x)^beta,  beta from 0 to 1.  A stage reweights by
 * likelihood^(beta' - beta), resamples, and MOVES every particle with K Metropolis-Hastings sweeps that leave the target
 * at beta' invariant.  The move is the hot part: gjx_temper_move reads a particle's latents THROUGH its ancestor index (no
 * separate gather), makes the K sweeps and writes the population back, in one launch.  gjx_temper_ess_ladder evaluates the
 * effective sample size of the increment for up to 64 candidate temperatures in one launch, so that choosing beta' is not a
 * host bisection of synchronising probes.
 *
 * THE PLAN.  A flat importance-style site table (gjx_site, as gjx_plan_create takes it: same argument kinds, same postfix
 * programs, GJX_ARG_PARAM values set by gjx_temper_plan_set_params, GJX_ARG_INPUT columns indexed by the particle's OWN
 * index i).  Latent sites (observed == 0) are the chain's state: float-valued (Normal, Gamma, Beta), numbered l = 0 .. L-1
 * in table order, 1 <= L <= GJX_TEMPER_MAX_LATENTS.  At least one site is observed.  out_col is ignored.
 *
 * Specification (exact: the result is a function of the inputs and the key alone, bit for bit).
 *
 *   assess(x)   walks the table in order.  A latent site's value is x_l: nothing is drawn.  lp = the f32 sum, from +0 and in
 *               table order, of the latent sites' terms: what gjx_logpdf_normal / _gamma / _beta returns at that value and
 *               the site's arguments if x_l lies in the site's OPEN support (Gamma: x > 0; Beta: 0 < x < 1; Normal: always),
 *               -inf otherwise (a NaN value included).  The support test is this header's: the density formulas of gjx.h
 *               are TFP's, NaN below 0 and finite there for a Gamma(1, b).  ll = the sum, taken the same way, of the
 *               observed sites' log-densities as those entry points return them.  One rounding per add, never
 *               contracted; arguments (affine forms, postfix programs) evaluate as in an importance plan.
 *               (A plan made by gjx_temper_plan_create_plated may hold sites evaluated once per row of a data table; what
 *               such a site adds to ll is specified in include/gjx_plate.h.  No table this header's creator accepts has one.)
 *   start       a = ancestors ? min((uint32) ancestors[i], n - 1) : i — no address is formed from an unchecked word;
 *               x_l = x_in[l][a].  recompute != 0: (lp, ll) = assess(x); otherwise lp = lp_in[a], ll = ll_in[a].
 *   keys        k_r = fold_in(key, r); p_r = fold_in(k_r, 0) the PROPOSAL key, a_r = fold_in(k_r, 1) the ACCEPTANCE key
 *               (both have lane 0; as in gjx_backmove.h the two batches are children of different keys, so no proposal
 *               word is an acceptance word).
 *   sweep r     r = 0 .. K-1, in order:
 *     propose   x'_l = element i of the value gjx_sample_logpdf_normal returns for the key batch {mode 1 (lazy split),
 *               parent p_r, first 0, has_fold 1, fold = l + 1 (THREEFRY) / l (PHILOX)}, loc = x_l, scale = scales[l], n:
 *               f32(x_l + f32(scales[l] * eps)).  The folds are those of a plan whose sites are the L latents, so under
 *               PHILOX the draws of latents 2 k and 2 k + 1 share cipher block k of the particle pair, as a plan's sites do.
 *     assess    (lp', ll') = assess(x').
 *     energy    h = f32(lp + f32(beta * ll)), h' likewise from (lp', ll'): the product and the sum round once each, no FMA;
 *               d = f32(h' - h).
 *     uniform   w = element i of gjx_rng_bits(keys {mode 1, parent a_r, first 0, no fold}, sub 0);
 *               u = uniform01(w) = f32((w >> 9) | 0x3F800000) - 1;  l_r = the spec's logarithm of u (what
 *               gjx_logpdf_bernoulli(value 1, probs u) returns).
 *     accept    iff d >= 0 || l_r < d (both comparisons are false on NaN).  A proposal outside a latent's support has
 *               lp' = -inf, h' = -inf (or NaN where ll' is NaN or +inf there) and is rejected by this rule.  On accept
 *               (x, lp, ll) = (x', lp', ll') and the particle's accept count goes up by one.
 *   output      x_out[l][i] = x_l, lp_out[i] = lp, ll_out[i] = ll, n_accept[i] = the count (when asked for).
 *
 * Nothing depends on the grid size.  The output columns must not overlap the input columns (another lane reads them).
 *
 * THE ESS LADDER.  For log-likelihoods ll[n] and steps delta_g >= 0, g < G <= GJX_TEMPER_MAX_LADDER, with M = max_i ll_i:
 *   S1_g = sum_i exp(delta_g (ll_i - M)),   S2_g = sum_i exp(2 delta_g (ll_i - M)),   ESS_g = S1_g^2 / S2_g.
 * An entry that is -inf or NaN contributes 0 to both sums (for delta = 0 too); if no entry is above -inf every sum is 0 and
 * M = -inf (the caller reads ESS = 0).  Exact form: the population is cut into W = gjx_temper_ladder_blocks(n) contiguous
 * blocks of ceil(n / W) entries, W a function of n alone.  Block b has m_b = its maximum and, per g, the float64 sums over
 * its entries of e and e * e, e = (double) exp_f32(f32(delta_g * f32(ll_i - m_b))) (the spec's f32 exp), taken per lane in
 * index order (lane t of 256 owns entries t, t + 256, ... of the block) and over the lanes in a fixed tree.  The workgroup
 * that finishes last (a ticket, as in gjx_importance_estimate) folds the blocks IN INDEX ORDER in float64:
 * S1_g = sum_b f p1, S2_g = sum_b f f p2 with f = exp((double) delta_g ((double) m_b - (double) M)).  The result is a
 * function of the inputs alone, whatever the grid scheduling.  delta = 0 gives S1 = S2 = the number of entries above -inf.
 */
#ifndef GJX_TEMPER_H
#define GJX_TEMPER_H

#include "gjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_TEMPER_VERSION_MAJOR 0
#define GJX_TEMPER_VERSION_MINOR 1

/* Latents per plan.  The chain keeps x, x' and the two (lp, ll) pairs in registers through a sweep: 2 L + 4 live values,
 * next to them the L proposal draws the compiler keeps in flight together.  Allocated on the generated gfx950 code
 * (profiles/temper_summary.md; THREEFRY / PHILOX): the regression (L = 2) 60 / 69 VGPRs, a Gaussian with L = 10 71 / 120, with
 * L = 16 99 / 166 — three waves per SIMD at the worst, no scratch anywhere.  L = 16 is where the PHILOX kernel still keeps
 * three waves (<= 168 registers); the two 16-entry pointer arrays are also what TemperArgs holds by value. */
#define GJX_TEMPER_MAX_LATENTS 16
#define GJX_TEMPER_MAX_MOVES 256
#define GJX_TEMPER_MAX_LADDER 64

typedef struct gjx_temper_plan gjx_temper_plan;

typedef struct {
  int32_t impl;      /* GJX_RNG_THREEFRY / GJX_RNG_PHILOX */
  int32_t n_moves;   /* K, 0 .. GJX_TEMPER_MAX_MOVES */
  int32_t recompute; /* != 0: (lp, ll) = assess(x) at the start; lp_in / ll_in are not read (may be NULL) */
  float beta;
  uint64_t n;        /* particles, 1 .. 2^31 - 1 */
  uint32_t key[2];
  uint64_t key_lane; /* PHILOX: the key's lane (0 for THREEFRY) */
  const float* x_in[GJX_TEMPER_MAX_LATENTS];  /* dev f32[n] per latent, in latent order */
  const float* lp_in;                          /* dev f32[n] */
  const float* ll_in;                          /* dev f32[n] */
  const int32_t* ancestors;                    /* dev int32[n], nullable: identity */
  const float* scales;                         /* HOST f32[L]: the random-walk proposal scales */
  const float* const* input_cols;              /* HOST array of dev f32[n] columns (GJX_ARG_INPUT), nullable when none is read */
  int32_t n_input_cols;
  float* x_out[GJX_TEMPER_MAX_LATENTS];        /* dev f32[n] per latent */
  float* lp_out;                               /* dev f32[n] */
  float* ll_out;                               /* dev f32[n] */
  int32_t* n_accept;                           /* dev int32[n], nullable */
  uint32_t max_workgroups;                     /* 0: the library's choice (a test knob: nothing depends on it) */
} gjx_temper_io;

int gjx_temper_version(int* major, int* minor);
/* GJX_ERR_INVALID: a NULL argument, n_sites outside 1 .. GJX_MAX_SITES, flags != 0, a site gjx_plan_create refuses,
 * observed > 1, an integer-valued (Bernoulli / Categorical) latent, no latent, more than GJX_TEMPER_MAX_LATENTS latents,
 * no observed site.  (Scopes / nested calls have no creator here.) */
int gjx_temper_plan_create(const gjx_site* sites /*host*/, int n_sites, uint32_t flags, gjx_temper_plan** out);
int gjx_temper_plan_destroy(gjx_temper_plan* p);
/* As gjx_plan_set_params: the values of the table's GJX_ARG_PARAM references for the launches that follow. */
int gjx_temper_plan_set_params(gjx_temper_plan* p, const float* params /*host*/, int n_params);
int gjx_temper_plan_n_latents(const gjx_temper_plan* p);
/* The HIP source of the plan's generated move kernel for impl 0 / 1 (it holds no parameter or observation value). */
int gjx_temper_plan_source(const gjx_temper_plan* p, int impl, char* buf, size_t buf_len, size_t* needed);
/* Compiles that source for gfx950 without touching a GPU: GJX_OK, or GJX_ERR_UNSUPPORTED when it does not compile. */
int gjx_temper_plan_compile_check(const gjx_temper_plan* p, int impl);
/* ONE launch: one lane per particle, no LDS, no barrier.  The kernel is generated from the table and compiled on first use:
 * with the compiler switched off (GJX_PLAN_JIT=0) GJX_ERR_UNSUPPORTED; GJX_ERR_JIT if it fails.
 * GJX_ERR_INVALID (nothing launched): a NULL plan / io / required pointer, n 0 or >= 2^31, n_moves outside 0 .. 256, impl not
 * 0 / 1, a lane with THREEFRY, recompute == 0 without lp_in / ll_in, scales NULL with n_moves > 0, fewer input columns or
 * parameters than the table reads. */
int gjx_temper_move(gjx_temper_plan* p, const gjx_temper_io* io, gjx_stream s);

/* W of the specification above: min(ceil(n / 256), 256), 0 for n = 0. */
uint32_t gjx_temper_ladder_blocks(uint64_t n);
/* 0 for arguments outside the ranges below. */
size_t gjx_temper_ladder_workspace_bytes(uint64_t n, int32_t n_deltas);
/* ONE launch.  ll dev f32[n]; deltas HOST f32[G], 1 <= G <= GJX_TEMPER_MAX_LADDER; out dev f64[2 G + 1]: out[2 g] = S1_g,
 * out[2 g + 1] = S2_g, out[2 G] = M.  ws: dev, 8-byte aligned, gjx_temper_ladder_workspace_bytes(n, G) bytes; its first
 * 8 bytes hold the ticket and must be ZERO before the first call — every call leaves them zero, so calls that share a
 * workspace must be stream-ordered.
 * GJX_ERR_INVALID: a NULL pointer, n 0 or >= 2^31, G out of range, a delta that is negative or not finite, ws misaligned.
 * GJX_ERR_WORKSPACE: ws NULL or too small. */
int gjx_temper_ess_ladder(const float* ll, uint64_t n, const float* deltas /*host*/, int32_t n_deltas, double* out, void* ws,
                          size_t ws_bytes, gjx_stream s);

#ifdef __cplusplus
}
#endif
#endif /* GJX_TEMPER_H */
