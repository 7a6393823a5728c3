// Exact quantiles and moments of f32 columns in device memory (include/gjx_quantiles.h): a three-sweep radix select on the
// order key of gjx_psis.h for several interior ranks at once, with the float64 moments riding on sweeps 0 and 1.  Included by
// gjx_hip.hip behind gjx_device.hpp.
//
// SWEEPS.  A workgroup owns one column (blockIdx.y) and one particle block (blockIdx.x); particles sit on lanes.  A lane
// loads kQUnroll 16-byte quads per iteration (all issued before the first is used: 4 x 16 bytes in flight per lane), the
// at most 3 + 3 entries before and behind the block's aligned quads go through scalar loads of lanes 0 .. 5.  Sweep 0
// histograms the top 11 key bits into 2048 LDS bins and takes the valid sum and the min / max key; sweeps 1 and 2 histogram
// the next 11 / 10 bits of the entries whose prefix is one of the column's selected prefixes (its SLOTS), kQSlots slots per
// launch, one 2048-bin LDS histogram each: 32 KiB of LDS exactly (the lane sums are reduced in the same LDS after the flush),
// five workgroups (20 waves) per CU of 160 KiB.  Eight slots would be 64 KiB and two workgroups per CU, sixteen 128 KiB and
// one: for a streaming kernel whose only latency cover is waves in flight the four-slot launch is the one that keeps the
// memory pipe full, and posterior draws rarely need more than three slots (the lo and hi rank of a probability almost
// always share a prefix).  The slot map of a launch is its four prefixes, read
// once into scalar registers; an entry finds its slot by four compares, no gather.  Sweep 1 (first slot batch) also takes the
// centred square sum.  LDS histograms are flushed, non-zero bins only, into the column's global histogram by integer atomics.
//
// CONCENTRATED VALUES.  Posterior draws of one latent share sign, exponent and leading mantissa bits: in sweep 0 nearly every
// lane of a wave hits the same one to four bins, and a ds_add per lane would serialise 64 deep on one address.  q_hist_add
// aggregates inside the wave first: it PEELS the distinct bins of the wave's vector one at a time — the first live lane's
// bin is broadcast (v_readlane), the lanes that share it are balloted, the leader adds their population count with ONE LDS
// atomic, and they leave.  After kQPeel rounds whatever is still live (a spread wave) falls back to one atomic per lane.
// Per 64 entries, concentrated (d <= 4 distinct bins): d rounds of about 7 instructions (s_ff1, v_readlane, v_cmp, s_bcnt1,
// ds_add_u32 on one lane, s_andn2, branch) and d LDS atomics — 0.11 d instructions and d / 64 atomics per entry.  Spread:
// the 4 rounds (28 instructions, 4 single-lane atomics) and then one 64-lane ds_add_u32 — about 0.45 instructions and up to
// 1 atomic per entry, on distinct addresses.
//
// PICKS.  One workgroup per column: a thread owns 8 consecutive bins, a workgroup scan of the 256 sums, and every target rank
// is located by the one thread whose bins cover it.  Thread 0 merges equal bins into slots and folds the block sums in index
// order.  No floating-point atomic anywhere.
#pragma once

#include "../../include/gjx_quantiles.h"

namespace gjx {

constexpr int kQBins = 2048;                                  // bins of one histogram (sweep 2 fills the lower 1024)
constexpr int kQSlots = GJX_QUANTILES_SLOTS_PER_LAUNCH;       // LDS histograms of one sweep launch
constexpr int kQMaxProbs = GJX_QUANTILES_MAX_PROBS;
constexpr int kQMaxSlots = 2 * kQMaxProbs;                    // a slot per target rank at most
constexpr int kQMaxSegs = GJX_QUANTILES_MAX_SEGMENTS;
constexpr uint32_t kQMaxBlocks = 1024;                        // particle blocks of a column
constexpr int kQPeel = 4;                                     // peel rounds before the per-lane fallback
constexpr int kQUnroll = 4;                                   // quads in flight per lane

struct QColState {  // per column of a batch, in the workspace
  double mean, var;
  double frac[kQMaxProbs];      // h - lo per probability
  uint32_t m, kmin, kmax, R;    // valid entries; min / max key over them; slots in use
  uint32_t prefix[kQMaxSlots];  // slot -> key prefix (11 bits after pick 0, 22 after pick 1)
  uint32_t tslot[kQMaxSlots];   // target 2 j + side -> slot
  uint32_t trank[kQMaxSlots];   // its rank among the slot's entries
};

struct QArgs {
  const float* base[kQMaxSegs];
  uint64_t stride[kQMaxSegs];
  uint32_t first[kQMaxSegs];  // the segment's first column
  int32_t n_seg, Q;
  uint32_t n, per, B;         // entries per column; entries per particle block; blocks
  uint32_t col0, cols;        // the batch
  double probs[kQMaxProbs];
  uint32_t* hist0;            // [cols][kQBins]
  uint32_t* hist;             // [cols][kQMaxSlots][kQBins]
  double* part;               // [cols][2][kQMaxBlocks]: the blocks' S1, S2
  QColState* st;              // [cols]
  float* bracket;
  double* quant;
  double* stats;
};

// Column c's base.  The segment table is a kernel argument: constant indices only, so that it stays in scalar loads.
GJX_DEV const float* q_column(const QArgs& A, uint32_t c) {
  const float* b = A.base[0];
  uint64_t st = A.stride[0];
  uint32_t f = 0;
#pragma unroll
  for (int s = 1; s < kQMaxSegs; ++s)
    if (s < A.n_seg && c >= A.first[s]) {
      b = A.base[s];
      st = A.stride[s];
      f = A.first[s];
    }
  return b + (uint64_t)(c - f) * st;
}

// +1 into sh[bin] for every lane with `on`, aggregated inside the wave (the header comment).  Called in wave-uniform flow.
GJX_DEV void q_hist_add(uint32_t* sh, uint32_t bin, bool on) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  uint64_t live = __ballot(on);
#pragma unroll
  for (int r = 0; r < kQPeel; ++r) {
    if (!live) break;
    const int leader = __builtin_ctzll(live);
    const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
    const uint64_t same = __ballot(on && bin == d);
    if ((int)lane == leader) atomicAdd(&sh[d], (uint32_t)__popcll(same));
    live &= ~same;
  }
  if ((live >> lane) & 1ull) atomicAdd(&sh[bin], 1u);
}

__global__ __launch_bounds__(kBlock) void k_quant_clear(QArgs A) {
  const size_t i0 = (size_t)blockIdx.x * kBlock + threadIdx.x, step = (size_t)gridDim.x * kBlock;
  const size_t n0 = (size_t)A.cols * kQBins / 2, n1 = n0 * kQMaxSlots;  // (8-byte stores: the workspace's alignment)
  uint2* h0 = reinterpret_cast<uint2*>(A.hist0);
  uint2* h1 = reinterpret_cast<uint2*>(A.hist);
  for (size_t i = i0; i < n0; i += step) h0[i] = make_uint2(0u, 0u);
  for (size_t i = i0; i < n1; i += step) h1[i] = make_uint2(0u, 0u);
  for (size_t i = i0; i < A.cols; i += step) {
    A.st[i].kmin = 0xffffffffu;
    A.st[i].kmax = 0u;
    A.st[i].R = 0u;
  }
}

template <int SWEEP>
__global__ __launch_bounds__(kBlock) void k_quant_sweep(QArgs A, uint32_t slot0) {
#if defined(__HIP_DEVICE_COMPILE__)  // (psis_key: the device-only section of gjx_device.hpp)
  // sweep 0: 2048 bins and the min / max key; sweeps 1, 2: kQSlots x 2048 bins — 32 KiB exactly, five workgroups per CU
  __shared__ __align__(8) uint32_t sh[SWEEP == 0 ? kQBins + 2 : kQSlots * kQBins];
  const uint32_t t = threadIdx.x, cb = blockIdx.y, b = blockIdx.x;
  QColState* st = A.st + cb;
  uint32_t nslots = 0, p0 = 0, p1 = 0, p2 = 0, p3 = 0;
  double mean = 0.0;
  if (SWEEP > 0) {
    const uint32_t R = st->R;
    if (R <= slot0) return;  // (workgroup-uniform: a column with fewer slots, or without a valid entry)
    nslots = R - slot0 < (uint32_t)kQSlots ? R - slot0 : (uint32_t)kQSlots;
    // the launch's slot map: four prefixes in scalar registers (no prefix has more than 22 bits: all ones matches nothing)
    p0 = st->prefix[slot0];
    p1 = nslots > 1u ? st->prefix[slot0 + 1u] : 0xffffffffu;
    p2 = nslots > 2u ? st->prefix[slot0 + 2u] : 0xffffffffu;
    p3 = nslots > 3u ? st->prefix[slot0 + 3u] : 0xffffffffu;
    mean = st->mean;
  }
  const uint32_t nbins = SWEEP == 0 ? (uint32_t)kQBins : nslots * (uint32_t)kQBins;
  for (uint32_t i = t; i < nbins; i += kBlock) sh[i] = 0u;
  if (SWEEP == 0 && t == 0) {
    sh[kQBins] = 0xffffffffu;
    sh[kQBins + 1] = 0u;
  }
  __syncthreads();
  const bool squares = SWEEP == 1 && slot0 == 0;

  // the block [b0, b1) of column x: head, aligned quads, tail (b * per < n: B = ceil(n / per))
  const float* x = q_column(A, A.col0 + cb);
  const uint32_t b0 = b * A.per, b1 = A.n - b0 < A.per ? A.n : b0 + A.per;
  const uint32_t a = (uint32_t)((uintptr_t)x >> 2) & 3u;
  uint32_t head = (4u - ((a + b0) & 3u)) & 3u;
  if (head > b1 - b0) head = b1 - b0;
  const uint32_t q0 = b0 + head, nq = (b1 - q0) >> 2, tail0 = q0 + 4u * nq, ntail = b1 - tail0;
  const float4* xq = reinterpret_cast<const float4*>(x + q0);

  double acc = 0.0;
  uint32_t kmin = 0xffffffffu, kmax = 0u;
  auto entry = [&](float v, bool on) {
    const uint32_t k = psis_key(v);
    const bool valid = on && k != 0xffffffffu;
    if (SWEEP == 0) {
      q_hist_add(sh, k >> 21, on);  // (the NaNs are bin 2047, and nothing else is)
      if (valid) {
        acc = acc + (double)v;
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
      }
    } else {
      if (squares && valid) {
        const double d = (double)v - mean;
        acc = acc + d * d;
      }
      const uint32_t p = SWEEP == 1 ? k >> 21 : k >> 10;
      const uint32_t digit = SWEEP == 1 ? (k >> 10) & 2047u : k & 1023u;
      const uint32_t slot = p == p0 ? 0u : p == p1 ? 1u : p == p2 ? 2u : p == p3 ? 3u : 4u;
      q_hist_add(sh, (slot & 3u) * (uint32_t)kQBins + digit, valid && slot < 4u);
    }
  };
  for (uint32_t v0 = 0; v0 < nq; v0 += kBlock * kQUnroll) {  // (wave-uniform trip count: the ballots see whole waves)
    float4 q[kQUnroll];
    bool on[kQUnroll];
#pragma unroll
    for (int u = 0; u < kQUnroll; ++u) {
      const uint32_t v = v0 + (uint32_t)u * kBlock + t;
      on[u] = v < nq;
      q[u] = on[u] ? xq[v] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int u = 0; u < kQUnroll; ++u) {
      entry(q[u].x, on[u]);
      entry(q[u].y, on[u]);
      entry(q[u].z, on[u]);
      entry(q[u].w, on[u]);
    }
  }
  {
    const bool on = t < head + ntail;
    const float v = on ? x[t < head ? b0 + t : tail0 + (t - head)] : 0.0f;
    entry(v, on);
  }

  if (SWEEP == 0 && kmin != 0xffffffffu) {
    atomicMin(&sh[kQBins], kmin);
    atomicMax(&sh[kQBins + 1], kmax);
  }
  __syncthreads();
  if (SWEEP == 0 && t == 0 && sh[kQBins] != 0xffffffffu) {
    atomicMin(&st->kmin, sh[kQBins]);
    atomicMax(&st->kmax, sh[kQBins + 1]);
  }
  uint32_t* g = SWEEP == 0 ? A.hist0 + (size_t)cb * kQBins : A.hist + ((size_t)cb * kQMaxSlots + slot0) * kQBins;
  for (uint32_t i = t; i < nbins; i += kBlock) {
    const uint32_t c = sh[i];
    if (c) atomicAdd(&g[i], c);
  }
  if (SWEEP == 0 || squares) {  // the lanes' sums: the balanced tree in lane order, in the LDS the flushed bins leave free
    __syncthreads();
    double* red = reinterpret_cast<double*>(sh);
    red[t] = acc;
    __syncthreads();
    for (uint32_t w = 1; w < (uint32_t)kBlock; w <<= 1) {
      if ((t & (2u * w - 1u)) == 0u) red[t] = red[t] + red[t + w];
      __syncthreads();
    }
    if (t == 0) A.part[((size_t)cb * 2 + (SWEEP == 0 ? 0 : 1)) * kQMaxBlocks + b] = red[0];
  }
#endif
}

// The exclusive prefix of v over the workgroup's 256 threads (Hillis-Steele in LDS, sh[2][256]).
GJX_DEV uint32_t q_block_scan(uint32_t v, uint32_t* sh) {
  const uint32_t t = threadIdx.x;
  uint32_t cur = 0;
  sh[t] = v;
  __syncthreads();
  for (uint32_t off = 1; off < (uint32_t)kBlock; off <<= 1) {
    uint32_t y = sh[cur * kBlock + t];
    if (t >= off) y += sh[cur * kBlock + t - off];
    cur ^= 1u;
    sh[cur * kBlock + t] = y;
    __syncthreads();
  }
  const uint32_t incl = sh[cur * kBlock + t];
  __syncthreads();
  return incl - v;
}

// If rank r falls into this thread's 8 bins c8 (which start at exclusive count ex and bin index 8 t): its bin and its rank
// inside that bin, for target tt.
GJX_DEV void q_locate(uint32_t r, uint32_t ex, const uint32_t (&c8)[8], uint32_t sum, uint32_t shift_prefix, uint32_t* bin_out,
                      uint32_t* rank_out, uint32_t tt) {
  if (r < ex || r - ex >= sum) return;
  uint32_t cum = ex;
  bool found = false;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (!found && r - cum < c8[i]) {
      bin_out[tt] = shift_prefix | (8u * threadIdx.x + (uint32_t)i);
      rank_out[tt] = r - cum;
      found = true;
    }
    cum += c8[i];
  }
}

// Thread 0: the targets' new prefixes nbin[0 .. T) -> distinct slots, into the column's state.
GJX_DEV void q_merge(QColState* st, uint32_t T, const uint32_t* nbin, const uint32_t* nrank, uint32_t* spfx) {
  uint32_t R = 0;
  for (uint32_t tt = 0; tt < T; ++tt) {
    uint32_t s = 0;
    while (s < R && spfx[s] != nbin[tt]) ++s;
    if (s == R) {
      spfx[R] = nbin[tt];
      st->prefix[R] = nbin[tt];
      ++R;
    }
    st->tslot[tt] = s;
    st->trank[tt] = nrank[tt];
  }
  st->R = R;
}

template <int STAGE>
__global__ __launch_bounds__(kBlock) void k_quant_pick(QArgs A) {
#if defined(__HIP_DEVICE_COMPILE__)  // (psis_unkey: the device-only section of gjx_device.hpp)
  __shared__ uint32_t scan[2 * kBlock];
  __shared__ uint32_t nbin[kQMaxSlots], nrank[kQMaxSlots], spfx[kQMaxSlots], ts[kQMaxSlots], tr[kQMaxSlots], oldp[kQMaxSlots];
  const uint32_t t = threadIdx.x, cb = blockIdx.x;
  QColState* st = A.st + cb;
  const uint32_t T = 2u * (uint32_t)A.Q;
  if (t < (uint32_t)kQMaxSlots) nbin[t] = nrank[t] = 0u;
  uint32_t m;
  if (STAGE == 0) {
    uint32_t* h = A.hist0 + (size_t)cb * kQBins;
    m = A.n - h[kQBins - 1];  // (bin 2047: the NaNs)
    uint32_t c8[8], sum = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      c8[i] = 8u * t + (uint32_t)i == (uint32_t)kQBins - 1u ? 0u : h[8u * t + i];
      sum += c8[i];
    }
    const uint32_t ex = q_block_scan(sum, scan);
#pragma unroll
    for (int j = 0; j < kQMaxProbs; ++j)
      if (j < A.Q && m > 0u) {
        const double hr = (double)(m - 1u) * A.probs[j], fl = __builtin_floor(hr);
        const uint32_t lo = (uint32_t)fl, hi = lo + 1u < m - 1u ? lo + 1u : m - 1u;
        if (t == 0) st->frac[j] = hr - fl;
        q_locate(lo, ex, c8, sum, 0u, nbin, nrank, 2u * j);
        q_locate(hi, ex, c8, sum, 0u, nbin, nrank, 2u * j + 1u);
      }
    __syncthreads();
    if (t == 0) {
      st->m = m;
      q_merge(st, m > 0u ? T : 0u, nbin, nrank, spfx);
      double s1 = 0.0;
      for (uint32_t b = 0; b < A.B; ++b) s1 = s1 + A.part[((size_t)cb * 2 + 0) * kQMaxBlocks + b];
      st->mean = s1 / (double)m;
    }
    return;
  }
  m = st->m;
  const uint32_t R = st->R;
  if (t < (uint32_t)kQMaxSlots) {
    ts[t] = st->tslot[t];
    tr[t] = st->trank[t];
    oldp[t] = st->prefix[t];
  }
  __syncthreads();
  for (uint32_t s = 0; s < R; ++s) {
    uint32_t* h = A.hist + ((size_t)cb * kQMaxSlots + s) * kQBins + 8u * t;
    uint32_t c8[8], sum = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      c8[i] = h[i];
      sum += c8[i];
      if (STAGE == 1) h[i] = 0u;  // (sweep 2 fills the same histograms)
    }
    const uint32_t ex = q_block_scan(sum, scan);
    const uint32_t shifted = oldp[s] << (STAGE == 1 ? 11 : 10);
    for (uint32_t tt = 0; tt < T; ++tt)
      if (ts[tt] == s) q_locate(tr[tt], ex, c8, sum, shifted, nbin, nrank, tt);
  }
  __syncthreads();
  if (STAGE == 1) {
    if (t == 0) {
      q_merge(st, m > 0u ? T : 0u, nbin, nrank, spfx);
      double s2 = 0.0;
      for (uint32_t b = 0; b < A.B; ++b) s2 = s2 + A.part[((size_t)cb * 2 + 1) * kQMaxBlocks + b];
      st->var = m >= 2u ? s2 / (double)(m - 1u) : __builtin_nan("");
    }
    return;
  }
  // the keys are complete: the outputs
  const size_t c = (size_t)A.col0 + cb;
  const double qnan = __builtin_nan("");
  if (t < (uint32_t)A.Q) {
    const float xlo = m ? psis_unkey(nbin[2u * t]) : u2f(0x7fc00000u), xhi = m ? psis_unkey(nbin[2u * t + 1u]) : u2f(0x7fc00000u);
    A.bracket[(c * A.Q + t) * 2 + 0] = xlo;
    A.bracket[(c * A.Q + t) * 2 + 1] = xhi;
    const double dl = (double)xlo, diff = (double)xhi - dl, prod = st->frac[t] * diff;
    A.quant[c * A.Q + t] = !m ? qnan : f2u(xlo) == f2u(xhi) ? dl : dl + prod;
  }
  if (t == 0) {
    double* o = A.stats + c * 5;
    o[0] = (double)(A.n - m);
    o[1] = m ? st->mean : qnan;
    o[2] = m >= 2u ? st->var : qnan;
    o[3] = m ? (double)psis_unkey(st->kmin) : qnan;
    o[4] = m ? (double)psis_unkey(st->kmax) : qnan;
  }
#endif
}

}  // namespace gjx
