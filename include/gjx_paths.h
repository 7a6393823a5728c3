/*
 * gjx_paths.h — trajectory trace-back over a recorded particle-filter history, in one launch.
 *
 * A SECOND header next to gjx.h, with a version of its own: gjx.h is the boundary the CPU oracle restates symbol for
 * symbol, and the bindings refuse a library whose gjx_version differs, so anything added THERE has to be added to the
 * oracle in the same change.  The trace-back is specified in exact integers (below) and its reference is four lines of
 * numpy; it needs no oracle.  libgjx_hip.so exports these entry points, the oracle library does not, and a binding
 * loads them if present.  Conventions (status codes, gjx_stream, borrowed "dev" pointers, no allocation, no host
 * synchronisation) are those of gjx.h.
 *
 * Semantics.  A filter of n particles and T steps recorded ancestors anc int32[T, n] (gjx.h: ancestors_out; row 0 is
 * never read) and per-step 4-byte columns col_c [T, n] (the state columns, the log-weights).  For m leaves:
 *
 *   lin[T-1][j]  = clamp(leaf[j])                      j < m   (leaf = identity when `leaves` is NULL; then m == n)
 *   lin[t-1][j]  = clamp(anc[t][ lin[t][j] ])          t = T-1 .. 1
 *   path_c[t][j] = col_c[t][ lin[t][j] ]               every column c, copied as 32 bits (f32 or int32)
 *   clamp(i)     = min((uint32_t) i, n - 1)            applied to EVERY leaf and EVERY ancestor read: no address is
 *                                                      formed from an unchecked index, whatever the tables hold
 */
#ifndef GJX_PATHS_H
#define GJX_PATHS_H

#include "gjx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GJX_PATHS_VERSION_MAJOR 0
#define GJX_PATHS_VERSION_MINOR 1

#define GJX_PATHS_MAX_COLS (GJX_SMC_MAX_STATE + 1) /* the state columns and, if wanted, the log-weights */
#define GJX_PATHS_LEAVES_ORDERED 1u                /* flags: the caller declares leaf[j] non-decreasing in j */

typedef struct {
  int32_t n_steps; /* T >= 1 */
  int32_t n_cols;  /* 0 .. GJX_PATHS_MAX_COLS */
  uint64_t n;      /* particles per step, 1 .. 2^31 - 1 */
  uint64_t m;      /* leaves,             1 .. 2^31 - 1 */
  /* Inputs.  Row t of an array starts t * stride ELEMENTS behind its base; strides >= n (a filter-batch layout
   * [T, F, stride] is base + f * stride with stride F * stride). */
  const int32_t* ancestors; /* dev int32[T, anc_stride]; required when T > 1 */
  uint64_t anc_stride;
  const int32_t* leaves; /* dev int32[m], or NULL = identity (m == n required) */
  const void* cols[GJX_PATHS_MAX_COLS]; /* dev [T, col_stride[c]], 4-byte elements; required for c < n_cols */
  uint64_t col_stride[GJX_PATHS_MAX_COLS];
  int32_t col_is_f32[GJX_PATHS_MAX_COLS]; /* != 0: the column takes part in sum_out / sumsq_out */
  /* Outputs, each nullable (at least one must be given).  Row strides >= m. */
  int32_t* lineage_out; /* dev int32[T, lineage_stride]: lin */
  uint64_t lineage_stride;
  void* paths_out[GJX_PATHS_MAX_COLS]; /* dev [T, paths_stride[c]]: path_c */
  uint64_t paths_stride[GJX_PATHS_MAX_COLS];
  /* dev f64[n_cols, T]: sum_j path_c[t][j] and sum_j path_c[t][j]^2 in float64 (the square of an f32 is exact there);
   * rows of columns with col_is_f32 == 0 are set to 0.  DETERMINISTIC: the leaves are cut into chunks of 1024
   * whatever the grid, a chunk's sum is a fixed tree, and the chunks' partials are added in chunk order by the
   * last workgroup to finish — the same inputs give the same 8 bytes on every run and for every max_workgroups. */
  double* sum_out;
  double* sumsq_out;
  /* dev int64[T]: the number of distinct values in lin[t][0 .. m).  Only for non-decreasing leaves
   * (GJX_PATHS_LEAVES_ORDERED; GJX_ERR_INVALID without it — the library neither checks nor sorts): the filters'
   * ancestor rows are non-decreasing ("monotone ancestors", gjx.h), hence every lin[t] is, and the count is
   * 1 + #{j >= 1 : lin[t][j] != lin[t][j-1]}. */
  int64_t* unique_out;
  /* dev u32[1], required with sum_out / sumsq_out / unique_out: ZERO before the launch, left zero by it (the arrival
   * counter of the workgroups); launches that share it must be stream-ordered. */
  uint32_t* ticket;
  uint32_t flags;
  uint32_t max_workgroups; /* 0 = the library chooses; otherwise a cap on the grid.  Results do not depend on it. */
} gjx_paths_io;

int gjx_paths_version(int* major, int* minor);
/* Scratch of a call with sum_out / sumsq_out / unique_out (the per-chunk partials); 0 bytes are needed without them. */
size_t gjx_paths_workspace_bytes(int32_t n_steps, uint64_t m, int32_t n_cols);
/* ONE kernel launch.  GJX_ERR_INVALID (nothing launched): io NULL, T < 1, n or m 0 or >= 2^31, n_cols out of range, a
 * required pointer NULL, no output at all, a stride below n (inputs) / m (outputs), leaves NULL with m != n,
 * unique_out without GJX_PATHS_LEAVES_ORDERED, statistics without ticket, ws not 8-byte aligned.
 * GJX_ERR_WORKSPACE: statistics requested and ws NULL or ws_bytes < gjx_paths_workspace_bytes(T, m, n_cols). */
int gjx_paths_trace(const gjx_paths_io* io, void* ws, size_t ws_bytes, gjx_stream s);

#ifdef __cplusplus
}
#endif
#endif /* GJX_PATHS_H */
