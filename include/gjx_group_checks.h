/*
 * gjx_group_checks.h — pointwise densities, PSIS-LOO and posterior predictive draws of a tempered plan with GROUPED latents.
 *
 * A SIXTEENTH header next to gjx.h, with a version of its own and for the same reason as the others: gjx.h is the boundary the
 * CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points, the oracle library does not, and a binding
 * loads them if present.  Conventions (status codes, gjx_stream, borrowed "dev" pointers, no allocation, no host
 * synchronisation) are those of gjx.h.
 *
 * gjx_group.h gives a tempered plan per-group latents z[s][g] and a move over them.  The three reductions over a population
 * that gjx_pointwise.h, gjx_psis.h and gjx_predictive.h define for a plated plan refuse such a plan: their row term depends
 * on the particle's scalars and on row d's data alone.  Here the term also depends on z[s][g(d)][i], the particle's value of
 * the group that owns row d.  The entry points below are those three calls with the S grouped columns as one more argument;
 * the io structs, the workspace size functions (gjx_pointwise_workspace_bytes, gjx_psis_workspace_bytes,
 * gjx_predictive_workspace_bytes), gjx_psis_tail_len, the chunk counts, the output layouts and the launch counts (two, nine
 * and two) are those of the flat headers.  Nothing new is allocated.
 *
 * Specification (exact, bit for bit: a function of the inputs — and, for the draws, of the key — alone).  G and offsets: the
 * plan's last gjx_temper_plan_set_groups; D = n_rows of its last gjx_temper_plan_set_data; n = io->n; z[s]: f32 [G][n], entry
 * (g, i) at z[s][g * n + i] (a 64-bit index).
 *
 *   g(d)      the number of g' in 1 .. G-1 with offsets[g'] <= d (compared as signed 32-bit words).  For the non-decreasing
 *             offsets the caller guarantees (gjx_group.h) this is the group that owns row d: empty groups are skipped.  It
 *             lies in 0 .. G-1 whatever the words are, and only offsets[1 .. G-1] are read: no address is formed from an
 *             unchecked word.
 *   t[d, i]   the f32 sum, from +0 and in table order, of the row-d terms of the plan's PLATED sites, flat and group-reading
 *             alike: each term is the t_d of gjx_plate.h — arguments and value evaluated in f32 at row d with the scalar
 *             latents x_l[i], every GROUP operand (gjx_group.h) reading z[ref][g(d)][i]; every operator rounds once, nothing
 *             is contracted.  Grouped sites themselves, unplated observed sites and the prior do not enter.
 *   pointwise chunks, blocks of four and the fold of gjx_pointwise.h over this t; out = (lse, s1, s2, c) per row.
 *   psis      selection, collection, body sum, sort, Pareto fit, weights and estimate of gjx_psis.h over this t; out and
 *             tail as there.  The term is the pointwise term: the same function text in both kernels.
 *   predictive the draws of gjx_predictive.h: particle i's pass key is fold_in(key, i), row d draws under its lazy child d,
 *             the draws are numbered among the PLATED sites alone (the `drawn` table), and every argument is evaluated at
 *             x_l[i] and z[ref][g(d)][i].  Sums, counts, the stored subset and the fold as there.
 *
 * Device side: the kernels are generated from the table (the generators of the flat kernels in a grouped mode: the source of
 * a table without grouped sites does not change).  Pointwise and predictive put rows on lanes: a lane finds g(d) once, by a
 * bounded binary search, and reads its four (or twice four) z values per block of particles with dword loads at 4-byte
 * alignment; PSIS puts particles on lanes: the four rows' groups are wave-uniform and lane i reads z[s][g * n + i], coalesced.
 */
#ifndef GJX_GROUP_CHECKS_H
#define GJX_GROUP_CHECKS_H

#include "gjx_group.h"
#include "gjx_pointwise.h"
#include "gjx_predictive.h"
#include "gjx_psis.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_GROUP_CHECKS_VERSION_MAJOR 0
#define GJX_GROUP_CHECKS_VERSION_MINOR 1

typedef struct {
  const float* z[GJX_GROUP_MAX_SITES]; /* dev f32[G][n] per grouped site, n = io->n */
} gjx_group_cols;

int gjx_group_checks_version(int* major, int* minor);
/* gjx_temper_pointwise / gjx_temper_psis / gjx_temper_predictive over a plan with grouped sites: the same launches on
 * stream s, the same io, the same status codes in the same order.
 * GJX_ERR_INVALID (nothing launched): whatever the flat entry point refuses; a plan without grouped sites; a grouped plan
 * without groups (gjx_temper_plan_set_groups) or without data; a NULL gjx_group_cols, or a NULL z[s] for s < the plan's
 * number of grouped sites. */
int gjx_temper_pointwise_grouped(gjx_temper_plan* p, const gjx_pointwise_io* io, const gjx_group_cols* z, gjx_stream s);
int gjx_temper_psis_grouped(gjx_temper_plan* p, const gjx_psis_io* io, const gjx_group_cols* z, gjx_stream s);
int gjx_temper_predictive_grouped(gjx_temper_plan* p, const gjx_keys* key, const gjx_predictive_io* io, const gjx_group_cols* z,
                                  gjx_stream s);
/* The HIP source of a generated check kernel of a grouped plan — kernel: 0 pointwise, 1 psis, 2 predictive; impl (the
 * generator) is read for kernel 2 only.  It holds no data value, no parameter value and neither G, n nor n_rows.
 * GJX_ERR_INVALID for a NULL plan, a plan without grouped sites, a kernel outside 0 .. 2, impl outside 0 .. 1 for kernel 2. */
int gjx_group_checks_source(const gjx_temper_plan* p, int kernel, int impl, char* buf, size_t buf_len, size_t* needed);
/* Compiles that source for gfx950 without touching a GPU: GJX_OK, or GJX_ERR_UNSUPPORTED when it does not compile. */
int gjx_group_checks_compile_check(const gjx_temper_plan* p, int kernel, int impl);

#ifdef __cplusplus
}
#endif
#endif /* GJX_GROUP_CHECKS_H */
