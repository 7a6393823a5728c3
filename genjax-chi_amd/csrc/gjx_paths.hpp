// Trajectory trace-back over a recorded filter history (include/gjx_paths.h): lineage, paths, their float64 sums and the
// number of distinct ancestors per step, in ONE launch.  Included by gjx_hip.hip behind gjx_device.hpp.
//
// The walk is a chain of T-1 dependent 4-byte loads per leaf: latency-bound per lane, so every lane walks kPathsPer
// CONSECUTIVE leaves (independent chains; lineages are monotone in the leaf for the filters' tables, so the four loads of
// a lane and those of its neighbours fall into the same or adjacent lines, and a lane's four outputs are one 16-byte
// store).  The chain load of the next row is issued first; the column gathers and the stores of the current row hang
// off lin[t] and nothing waits for them but the statistics.  The kernel uses few registers and 1 KiB of LDS: 8 workgroups
// per CU.
//
// Statistics are deterministic: a CHUNK is the kPathsChunk leaves of one workgroup iteration — a partition of the leaves
// that does not depend on the grid.  Per step a chunk reduces (lane: 4 leaves in order; wave: the fixed DPP scan; workgroup:
// 4 waves in order) and stores one partial per statistic into the workspace, [chunk][step][statistic]; the last workgroup to
// take the ticket adds the partials of every (step, statistic) in chunk order, a thread per result.  Integer counts go the same
// way, so there is no atomic on a result at all.
#pragma once

#include "../../include/gjx_paths.h"

namespace gjx {

constexpr int kPathsPer = 4;                      // leaves per lane
constexpr int kPathsChunk = kBlock * kPathsPer;   // leaves per workgroup iteration: the unit of the partials
constexpr int kPathsMaxCols = GJX_PATHS_MAX_COLS;
constexpr int kPathsMaxSlots = 2 * kPathsMaxCols + 1;  // per column (sum, sum of squares), then the distinct count
constexpr unsigned kPathsMaxGrid = 2048;          // 256 CUs x 8 resident workgroups

struct PathsArgs {
  int32_t T, n_cols;
  uint32_t n, m;
  uint32_t f32_mask;  // bit c: column c is f32
  uint32_t n_chunks;
  const int32_t* anc;
  uint64_t anc_stride;
  const int32_t* leaves;
  const uint32_t* cols[kPathsMaxCols];
  uint64_t col_stride[kPathsMaxCols];
  int32_t* lin_out;
  uint64_t lin_stride;
  uint32_t* paths_out[kPathsMaxCols];
  uint64_t paths_stride[kPathsMaxCols];
  double* sum_out;
  double* sumsq_out;
  int64_t* unique_out;
  uint64_t* partials;  // [n_chunks][T][2 n_cols + 1]: doubles as bit patterns / counts
  uint32_t* ticket;
};

GJX_DEV uint64_t d2u(double x) { return __builtin_bit_cast(uint64_t, x); }
// Sum over the wave in a FIXED tree (the DPP scan of gjx_device.hpp with a float64 add: the same lanes meet in the same order
// whatever runs next to the wave); valid in every lane.
GJX_DEV double wave_sum_f64(double v) {
  return u2d(wave_last_u64(wave_scan_u64(d2u(v), d2u(0.0), [](uint64_t a, uint64_t b) { return d2u(u2d(a) + u2d(b)); })));
}
// 4 consecutive 4-byte elements of an output row: one 16-byte store where the address allows it
GJX_DEV void paths_store4(uint32_t* row, uint64_t j0, uint32_t m, const uint32_t (&v)[kPathsPer]) {
  uint32_t* p = row + j0;
  if (j0 + kPathsPer <= (uint64_t)m && ((uintptr_t)p & 15) == 0) {
    *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int r = 0; r < kPathsPer; ++r)
      if (j0 + r < (uint64_t)m) p[r] = v[r];
  }
}

template <bool STATS>
__global__ __launch_bounds__(kBlock) void k_paths_trace(PathsArgs A) {
  __shared__ uint64_t sh[2][kBlock / kWave][kPathsMaxSlots];
  __shared__ uint32_t sh_last;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t nm1 = A.n - 1;
  const int n_slots = 2 * A.n_cols + 1;
  const bool want_unique = STATS && A.unique_out != nullptr;
  for (uint32_t chunk = blockIdx.x; chunk < A.n_chunks; chunk += gridDim.x) {
    const uint64_t j0 = (uint64_t)chunk * kPathsChunk + (uint64_t)tid * kPathsPer;
    uint32_t idx[kPathsPer];
    bool ok[kPathsPer];
#pragma unroll
    for (int r = 0; r < kPathsPer; ++r) {
      const uint64_t j = j0 + r;
      ok[r] = j < (uint64_t)A.m;
      const uint32_t leaf = !ok[r] ? 0u : (A.leaves ? (uint32_t)A.leaves[j] : (uint32_t)j);
      idx[r] = leaf < nm1 ? leaf : nm1;  // (an idle slot walks particle 0: every load stays in bounds, nothing is stored)
    }
    // the distinct count compares a leaf with its left neighbour: the first lane of a wave walks the lineage of the leaf in
    // front of the wave's block as a fifth chain (the neighbour belongs to another wave or workgroup)
    const bool has_prev = want_unique && lane == 0 && j0 > 0 && ok[0];
    uint32_t pidx = 0;
    if (has_prev) {
      const uint32_t leaf = A.leaves ? (uint32_t)A.leaves[j0 - 1] : (uint32_t)(j0 - 1);
      pidx = leaf < nm1 ? leaf : nm1;
    }
    if (STATS) __syncthreads();  // (the previous chunk's last partials have left the LDS slots)
    for (int t = A.T - 1; t >= 0; --t) {
      // the chain first: the next row's indices
      uint32_t nxt[kPathsPer] = {0, 0, 0, 0}, pnxt = 0;
      if (t > 0) {
        const int32_t* anc_t = A.anc + (uint64_t)t * A.anc_stride;
#pragma unroll
        for (int r = 0; r < kPathsPer; ++r) nxt[r] = (uint32_t)anc_t[idx[r]];
        if (has_prev) pnxt = (uint32_t)anc_t[pidx];
      }
      // off the chain: gathers and stores of row t
      uint32_t v[kPathsMaxCols][kPathsPer];
#pragma unroll
      for (int c = 0; c < kPathsMaxCols; ++c) {
        if (c < A.n_cols) {
          const uint32_t* col_t = A.cols[c] + (uint64_t)t * A.col_stride[c];
#pragma unroll
          for (int r = 0; r < kPathsPer; ++r) v[c][r] = col_t[idx[r]];
        }
      }
      if (A.lin_out && ok[0]) paths_store4(reinterpret_cast<uint32_t*>(A.lin_out) + (uint64_t)t * A.lin_stride, j0, A.m, idx);
#pragma unroll
      for (int c = 0; c < kPathsMaxCols; ++c)
        if (c < A.n_cols && A.paths_out[c] && ok[0]) paths_store4(A.paths_out[c] + (uint64_t)t * A.paths_stride[c], j0, A.m, v[c]);
      if (STATS) {
        uint64_t* slot = sh[t & 1][w];
#pragma unroll
        for (int c = 0; c < kPathsMaxCols; ++c) {
          if (c < A.n_cols && ((A.f32_mask >> c) & 1u) && (A.sum_out || A.sumsq_out)) {
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int r = 0; r < kPathsPer; ++r) {
              const double d = ok[r] ? (double)u2f(v[c][r]) : 0.0;
              a += d;
              b += d * d;
            }
            a = wave_sum_f64(a);
            b = wave_sum_f64(b);
            if (lane == 0) { slot[2 * c] = d2u(a); slot[2 * c + 1] = d2u(b); }
          }
        }
        if (want_unique) {
          // lane i's left neighbour is lane i-1's last leaf; lane 0 has walked it itself (or starts the row: leaf 0 counts)
          uint32_t left = dpp_u32<kDppWaveShr1, 0xf, 0xf>(0u, idx[kPathsPer - 1]);
          bool first = lane == 0 ? (has_prev ? idx[0] != pidx : true) : idx[0] != left;
          uint32_t cnt = (ok[0] && first) ? 1u : 0u;
#pragma unroll
          for (int r = 1; r < kPathsPer; ++r) cnt += (ok[r] && idx[r] != idx[r - 1]) ? 1u : 0u;
          const uint32_t tot = (uint32_t)wave_sum_int((int)cnt);
          if (lane == 0) slot[2 * A.n_cols] = tot;
        }
        __syncthreads();  // (one barrier per step: the slots are double-buffered by the step's parity)
        if ((int)tid < n_slots) {
          const int c = (int)tid >> 1;
          const bool live = (int)tid == 2 * A.n_cols ? want_unique
                                                     : (((A.f32_mask >> c) & 1u) && ((tid & 1) ? A.sumsq_out != nullptr : A.sum_out != nullptr));
          if (live) {
            uint64_t r;
            if ((int)tid == 2 * A.n_cols) {
              r = 0;
              for (int i = 0; i < kBlock / kWave; ++i) r += sh[t & 1][i][tid];
            } else {
              double acc = u2d(sh[t & 1][0][tid]);
              for (int i = 1; i < kBlock / kWave; ++i) acc += u2d(sh[t & 1][i][tid]);
              r = d2u(acc);
            }
            // read by the last workgroup of THIS launch: written through (agent scope), as lse_store_row does
            __hip_atomic_store(A.partials + ((uint64_t)chunk * (uint32_t)A.T + (uint32_t)t) * n_slots + tid, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
      if (t > 0) {
#pragma unroll
        for (int r = 0; r < kPathsPer; ++r) idx[r] = nxt[r] < nm1 ? nxt[r] : nm1;
        pidx = pnxt < nm1 ? pnxt : nm1;
      }
    }
  }
  if (!STATS) return;
  // the ticket: every storing thread releases its partials, the workgroup meets, one lane arrives
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  if (tid == 0)
    sh_last = __hip_atomic_fetch_add(A.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (!sh_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  // a thread per (step, statistic): the chunks' partials in chunk order, one dependent add each with the loads running ahead
  // (neighbouring threads read neighbouring words of a chunk's row)
  const uint32_t n_out = (uint32_t)A.T * (uint32_t)n_slots;
  for (uint32_t o = tid; o < n_out; o += kBlock) {
    const uint32_t t = o / (uint32_t)n_slots, k = o - t * (uint32_t)n_slots;
    const uint64_t* p = A.partials + o;
    if (k == 2u * (uint32_t)A.n_cols) {
      if (!want_unique) continue;
      uint64_t acc = 0;
#pragma unroll 16
      for (uint32_t i = 0; i < A.n_chunks; ++i) acc += p[(uint64_t)i * n_out];
      A.unique_out[t] = (int64_t)acc;
      continue;
    }
    const uint32_t c = k >> 1;
    double* dst = (k & 1) ? A.sumsq_out : A.sum_out;
    if (!dst) continue;
    double acc = 0.0;
    if ((A.f32_mask >> c) & 1u) {
#pragma unroll 16
      for (uint32_t i = 0; i < A.n_chunks; ++i) acc += u2d(p[(uint64_t)i * n_out]);
    }
    dst[(uint64_t)c * (uint32_t)A.T + t] = acc;
  }
  if (tid == 0) __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace gjx
