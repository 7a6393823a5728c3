/*
 * gjx_plate_loglik.h — the log-likelihood of a plated tempered plan over a population, the work split over data ROWS as
 * well as particles: what an importance sampler with a prior proposal weights its particles with.
 *
 * A TWENTIETH header next to gjx.h, with a version of its own and for the same reason as the others: gjx.h is the boundary
 * the CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points, the oracle library does not, and a
 * binding loads them if present.  Conventions (status codes, gjx_stream, borrowed "dev" pointers, no allocation, no host
 * synchronisation) are those of gjx.h.
 *
 * The only other evaluator of a plated site, the move kernel (gjx_plate.h), puts one particle on a lane and walks all
 * n_rows rows: it fills the device at n = 10^6 and leaves most of it idle at n = 4096, whatever n_rows is.  Here a workgroup
 * owns a tile of 256 particles AND one chunk of rows; the chunks' float64 partial sums meet in a second launch, in chunk
 * order.  No floating-point atomic anywhere: the result is a function of the inputs alone, bit for bit.
 *
 * THE PLAN.  A gjx_temper_plan made by gjx_temper_plan_create_plated or gjx_temper_plan_create_counts with at least one
 * PLATED site, after gjx_temper_plan_set_data (and gjx_temper_plan_set_params where the table reads parameters).  A plan
 * with GROUPED sites (gjx_group.h) is refused: grouped plans are out of scope here.
 *
 * Specification (exact).  For particle i with latents x_l = x_in[l][i]:
 *   lp   is `assess`'s lp of gjx_temper.h: the f32 sum, from +0 and in table order, of the latent sites' terms, -inf
 *        outside a site's open support.
 *   ll   is `assess`'s ll: from +0 and in table order; an observed site that is not plated adds its f32 log-density
 *        (ll = ll + t, one rounding).  At a PLATED site's table position, with t_d the f32 row terms of gjx_plate.h
 *        (gjx_counts.h for a count site), d = 0 .. n_rows - 1:
 *          the rows are cut into C contiguous chunks of R rows, the last one shorter: chunk c owns rows c R .. min((c + 1) R,
 *          n_rows) - 1;
 *          partial_c = the FLOAT64 sum of (double) t_d over the chunk's rows, in row order, from +0.0;
 *          acc       = the float64 sum of partial_0 .. partial_{C-1}, in chunk order, from +0.0;
 *          ll        = ll + (float) acc: one f32 rounding of the site's total, one of the add, as in gjx_plate.h.
 *        Every PLATED site of the table has its own partials and its own acc; all of them use the same R and C.
 *   With C = 1 this is the sum of gjx_plate.h: ll_out and lp_out equal those of gjx_temper_move(n_moves = 0, recompute = 1)
 *   on the same plan, data and columns, bit for bit.  Nothing depends on max_workgroups.
 *   In numpy:  t = terms.astype(float32)  # [n_rows]
 *              part = [sum64_in_order(t[c * R:(c + 1) * R]) for c in range(C)];  acc = 0.0;  for v in part: acc += v
 *              ll = float32(ll + float32(acc))
 *
 * THE RULE FOR R AND C, a function of (n, n_rows, rows_per_chunk) alone, with tiles = ceil(n / 256):
 *   rows_per_chunk == 0 (the library's choice):  want = ceil(GJX_PLATE_LOGLIK_TARGET_WORKGROUPS / tiles);
 *       R = max(GJX_PLATE_LOGLIK_MIN_ROWS, 4 ceil(ceil(n_rows / want) / 4)).
 *   rows_per_chunk != 0 (a test knob, a multiple of 4):  R = rows_per_chunk.
 *   then, if ceil(n_rows / R) > GJX_PLATE_LOGLIK_MAX_CHUNKS:  R = 4 ceil(ceil(n_rows / GJX_PLATE_LOGLIK_MAX_CHUNKS) / 4)
 *       (the library's own R never needs it: it gives C <= want <= GJX_PLATE_LOGLIK_TARGET_WORKGROUPS);
 *   C = ceil(n_rows / R).
 * The first launch has tiles x C workgroups of 256 lanes (four waves).  1024 workgroups are 4096 waves: four per SIMD of a
 * device with 256 compute units — and never fewer than two wherever n_rows >= 64 want, since rounding R up to the next
 * multiple of 4 removes less than half of the chunks there.  C = 1 from n = 261 889 on (1024 tiles): the particles alone fill
 * the device and the rows stay in one chunk, as in the move kernel.  The workspace is 8 n C bytes per PLATED site: under the
 * library's rule C <= want < 1024 / tiles + 1, so at most 8 (n + 262 144) bytes.
 */
#ifndef GJX_PLATE_LOGLIK_H
#define GJX_PLATE_LOGLIK_H

#include "gjx_plate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_PLATE_LOGLIK_VERSION_MAJOR 0
#define GJX_PLATE_LOGLIK_VERSION_MINOR 1

#define GJX_PLATE_LOGLIK_TARGET_WORKGROUPS 1024
#define GJX_PLATE_LOGLIK_MAX_CHUNKS 1024
#define GJX_PLATE_LOGLIK_MIN_ROWS 64

typedef struct {
  int32_t impl;                               /* GJX_RNG_THREEFRY / GJX_RNG_PHILOX: the generator whose kernels are used (nothing is drawn) */
  uint32_t rows_per_chunk;                    /* 0: the library's rule; otherwise R, a multiple of 4 (a test knob) */
  uint64_t n;                                 /* particles, 1 .. 2^31 - 1 */
  const float* x_in[GJX_TEMPER_MAX_LATENTS];  /* dev f32[n] per latent, in latent order */
  const float* const* input_cols;             /* HOST array of dev f32[n] columns (GJX_ARG_INPUT), nullable when none is read */
  int32_t n_input_cols;
  uint32_t max_workgroups;                    /* 0: the library's choice; caps the particle tiles in flight (a test knob) */
  float* ll_out;                              /* dev f32[n] */
  float* lp_out;                              /* dev f32[n], nullable */
} gjx_plate_loglik_io;

int gjx_plate_loglik_version(int* major, int* minor);
/* C of the rule above; 0 for n or n_rows outside 1 .. 2^31 - 1 or a rows_per_chunk that is not a multiple of 4. */
uint32_t gjx_plate_loglik_chunks(uint64_t n, uint64_t n_rows, uint32_t rows_per_chunk);
/* 8 n C n_plated bytes (n_plated: the PLATED sites of the plan, 1 .. GJX_MAX_SITES); 0 where C is 0 or n_plated is out of range. */
size_t gjx_plate_loglik_workspace_bytes(uint64_t n, uint64_t n_rows, uint32_t rows_per_chunk, int32_t n_plated);
/* The PLATED sites of a plan (GJX_ERR_INVALID for NULL). */
int gjx_temper_plan_n_plated(const gjx_temper_plan* p);
/* TWO launches: tiles x C workgroups write partial[site][c][i] (f64, coalesced) to the workspace; ceil(n / 256) workgroups
 * fold them per particle, add the other sites' terms and write ll_out / lp_out.  Both kernels are generated from the plan's
 * table and compiled on first use: GJX_ERR_UNSUPPORTED with the compiler switched off, GJX_ERR_JIT if it fails.  ws: dev,
 * 8-byte aligned, gjx_plate_loglik_workspace_bytes(...) bytes; it need not be initialised and holds nothing between calls.
 * GJX_ERR_INVALID (nothing launched): a NULL plan / io / ll_out / latent column; n 0 or >= 2^31; impl not 0 / 1; a plan
 * without PLATED sites, without data or with GROUPED sites; fewer input columns or parameters than the table reads; a
 * rows_per_chunk that is not a multiple of 4; ws not 8-byte aligned.
 * GJX_ERR_WORKSPACE: ws NULL or too small. */
int gjx_plate_loglik(gjx_temper_plan* p, const gjx_plate_loglik_io* io, void* ws, size_t ws_bytes, gjx_stream s);
/* The HIP source of generated kernel `kernel` (0: the row-chunk kernel, 1: the fold) under generator impl, and its
 * compilation for gfx950 without touching a GPU (as gjx_temper_plan_source / gjx_temper_plan_compile_check). */
int gjx_plate_loglik_source(const gjx_temper_plan* p, int kernel, int impl, char* buf, size_t buf_len, size_t* needed);
int gjx_plate_loglik_compile_check(const gjx_temper_plan* p, int kernel, int impl);

#ifdef __cplusplus
}
#endif
#endif /* GJX_PLATE_LOGLIK_H */
