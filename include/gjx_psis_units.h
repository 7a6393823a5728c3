/*
 * gjx_psis_units.h — PSIS leave-one-GROUP-out over a tempered plan: Pareto-smoothed importance sampling (gjx_psis.h) where
 * what is left out is a UNIT, a contiguous block of data rows — a group of a grouped plan, several of them, a part of one,
 * or a block of rows of a flat plated plan (leave-one-subject-out without a subject effect).
 *
 * A SEVENTEENTH header next to gjx.h, with a version of its own and for the same reason as the others: gjx.h is the boundary
 * the CPU oracle restates symbol for symbol.  libgjx_hip.so exports these entry points, the oracle library does not, and a
 * binding loads them if present.  Conventions (status codes, gjx_stream, borrowed "dev" pointers, no allocation, no host
 * synchronisation) are those of gjx.h.
 *
 * Specification (D = n_rows of the plan's last gjx_temper_plan_set_data; n = io->psis.n particles, equally weighted;
 * M = io->psis.tail_len; U units).
 *
 *   units     unit_offsets: dev int32[U + 1], borrowed.  Unit u owns the rows lo_u .. hi_u - 1 with lo_u = clamp(unit_offsets[u]),
 *             hi_u = max(lo_u, clamp(unit_offsets[u + 1])), clamp(w) = min(max(w, 0), D).  The caller guarantees unit_offsets[0] == 0,
 *             non-decreasing words and unit_offsets[U] == D; every word is clamped before use, so no address is formed from an
 *             unchecked word.  Empty units are legal.  Units are independent of the plan's groups.
 *   T[u, i]   (float) acc, acc the float64 sum from +0.0, over d = lo_u .. hi_u - 1 in ascending order, of (double) t[d, i].
 *             t[d, i] is the term of gjx_pointwise.h on a flat plan and of gjx_group_checks.h on a grouped one (every GROUP
 *             operand reads z[ref][g(d)][i]): the same generated function text as the pointwise and PSIS term.  T is exact,
 *             bit for bit.  A non-finite t makes T non-finite; it is then counted in `bad` by the rule of gjx_psis.h.
 *   psis      key order, tail, c_less, body sum, bad, fit, weights and estimate are gjx_psis.h verbatim with "row d" read as
 *             "unit u" and t_i as T[u, i].  An empty unit follows the general rule: every entry is +0, the tail is tied with
 *             its cutoff, nothing is smoothed — khat = +inf, elpd = 0.
 *   order     the particle axis is cut into W = ceil(n / 32768) chunks of 32768 particles.  Inside a chunk lane l of the 256
 *             takes the entries lo + 4 l .. lo + 4 l + 3, then those 1024 further on, and so on, in that order; the lanes'
 *             float64 sums are folded by the fixed binary tree of gjx_psis.h and the chunks' sums added in index order.  The
 *             order is a function of (n, M) alone: not of U, of the batch size or of a grid.  No floating-point atomics: two
 *             calls on equal inputs give equal bits, whatever their table_bytes.
 *   lse       m_u = the largest entry of unit u in the key order (a NaN if there is one);
 *             E_u = the sum, in the order above, of (double) exp_f32(f32(T[u, i] - m_u)) — exp_f32 as in gjx_pointwise.h;
 *             lse_u = (double) m_u + log(E_u).  It is log sum_i exp(T[u, i]) where bad_u == 0 and carries no meaning elsewhere.
 *
 *   out       f64 [8, U]: elpd, khat, sigma, (double) s, (double) tT, B, bad of gjx_psis.h, then lse.
 *   tail      nullable f32 [U, M + 1], each unit's M + 1 smallest entries in ascending order.
 *
 * Device side.  The row kernel of gjx_psis.h evaluates the term inside each of its four passes; a unit's
 * value costs a whole block of rows and is 4 bytes, so it is computed once and kept: per batch of Ub units ONE generated
 * launch writes T into a table [Ub][pitch] of the workspace (pitch = n rounded up to a multiple of 4), then the four fixed
 * passes of a radix select read that table with 16-byte loads, with gjx_psis.h's own select and finish launches between and
 * after them: nine launches per batch, ceil(U / Ub) batches on the caller's stream, and (with more than one chunk) one memset
 * before the first.  Ub is the largest multiple of 4 with Ub * pitch * 4 <= table_bytes, at most U rounded up to one.
 * The TABLE is what table_bytes bounds.  The rest of the workspace is per batch (8 KB of histogram, a state and M + 1 keys per
 * unit of the batch, 8 W Ub bytes of lse partials) except the body partials: gjx_psis.h's finish kernel reads them at the pitch
 * of its out rows, so they are one [W][U] float64 plane, 8 W U bytes — 2.5 MB at n = 1e6 (W = 31) and U = 10 000.
 */
#ifndef GJX_PSIS_UNITS_H
#define GJX_PSIS_UNITS_H

#include "gjx_group_checks.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_PSIS_UNITS_VERSION_MAJOR 0
#define GJX_PSIS_UNITS_VERSION_MINOR 1

#define GJX_PSIS_UNITS_TABLE_BYTES ((size_t)256 << 20) /* what table_bytes == 0 stands for */

typedef struct {
  gjx_psis_io psis;   /* n, x, tail_len, ws as in gjx_psis.h; out: dev f64[8 * U]; tail: nullable dev f32[U * (tail_len + 1)];
                         ws: gjx_psis_units_workspace_bytes(n, U, tail_len, table_bytes) bytes */
  size_t table_bytes; /* the bound of the cached table; 0: GJX_PSIS_UNITS_TABLE_BYTES */
} gjx_psis_units_io;

int gjx_psis_units_version(int* major, int* minor);
/* 0 for arguments out of range: n, U outside 1 .. 2^31 - 1, tail_len outside 5 .. GJX_PSIS_MAX_TAIL, a table_bytes (other
 * than 0) below four units' rows.  The workspace need not be initialised. */
size_t gjx_psis_units_workspace_bytes(uint64_t n, uint64_t U, uint32_t tail_len, size_t table_bytes);
/* z: the grouped columns of a grouped plan (gjx_group_checks.h), NULL on a flat plan.
 * GJX_ERR_INVALID (nothing compiled, nothing launched): whatever gjx_temper_psis (z == NULL) or gjx_temper_psis_grouped
 * refuses for the plan's kind — a grouped plan without z or without groups among it; z on a flat plan; NULL unit_offsets;
 * U outside 1 .. 2^31 - 1; a table_bytes (other than 0) below four units' rows.
 * GJX_ERR_WORKSPACE: ws NULL or smaller than gjx_psis_units_workspace_bytes(n, U, tail_len, table_bytes).
 * GJX_ERR_UNSUPPORTED / GJX_ERR_JIT as in gjx_psis.h. */
int gjx_temper_psis_units(gjx_temper_plan* p, const gjx_psis_units_io* io, const int32_t* unit_offsets, uint64_t U,
                          const gjx_group_cols* z, gjx_stream s);
/* The HIP source of the plan's generated unit-sum kernel (flat or grouped, as the plan is): it holds no data value, no
 * parameter value and neither n, n_rows, U nor G.  GJX_ERR_INVALID for a NULL plan, a plan without a PLATED site or one that
 * reads an input column. */
int gjx_psis_units_source(const gjx_temper_plan* p, char* buf, size_t buf_len, size_t* needed);
/* Compiles that source for gfx950 without touching a GPU: GJX_OK, or GJX_ERR_UNSUPPORTED when it does not compile. */
int gjx_psis_units_compile_check(const gjx_temper_plan* p);

#ifdef __cplusplus
}
#endif
#endif /* GJX_PSIS_UNITS_H */
