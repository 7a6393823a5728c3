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
//
// WEIGHTED COLUMNS (the second half of this file; kernels of their own, the ones above are untouched).  The select runs on
// histograms of MASS, the u32 fixed-point weight fixw(lw, max, 31).  A prologue of two kernels takes each weight row's
// maximum (as an order key, by integer atomics) and writes the mass table once, so a sweep streams 8 bytes per entry.  A
// table row in the workspace is shifted by the 16-byte phase of the first data column it weighs: the x quads (aligned by the
// column's own base, as above) and the mass quads are then aligned together for every column of that phase; the mass quad is
// loaded through a 4-byte-aligned type and is ONE global_load_dwordx4 whatever the phase (gfx950 ISA of every sweep: 8
// global_load_dwordx4 per iteration, 4 of x and 4 of masses).  Digits are 12 / 10 / 10 bits: u64 LDS bins (ds_add_u64), 4096
// in sweep 0 and four slots of 1024 in sweeps 1 and 2, 32 KiB and five workgroups per CU in every sweep.  NaN x are counted in
// a register, not histogrammed (bin 4095 stays empty), and min / max key, the NaN count and the lane sums S1, S0 (sweep 0)
// and S2 (sweep 1) are reduced after the flush, the keys and the count by a wave scan and one integer atomic per wave.  There
// is one target mass per probability, not two bracketing ranks: at most Q slots, ceil(Q / 4) launches of sweeps 1 and 2.
// wq_hist_add is q_hist_add's peel with the leader adding the SUM of the masses of the lanes that share its bin: the mass is
// cut into its low and high 16 bits and each half is summed over the wave by a u32 DPP scan (a u64 add cannot take a DPP
// operand).  Counted in the gfx950 ISA, per 64 entries: a peel round is about 70 instructions (s_ff1, v_readlane, v_cmp, two
// masked 8-step DPP sums with their s_nops, two v_readlane, the recombination and one single-lane ds_add_u64) against 7
// unweighted: concentrated (d <= 4 distinct bins) 1.1 d instructions and d / 64 atomics per entry; spread the 4 rounds and one
// 64-lane ds_add_u64, about 4.4 instructions and up to 1 atomic per entry, on distinct addresses.  Measured, the weighted call
// takes 1.7 to 2.2 times the unweighted one on the same columns (profiles/weighted_quantiles_summary.md): the doubled bytes.
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

// =====================================================================================================================
// WEIGHTED columns (gjx_weighted_column_quantiles): the same select on histograms of MASS.  Own kernels; nothing above changes.
// =====================================================================================================================
constexpr int kWQBins0 = 4096;                 // sweep 0: 12 key bits, u64 bins — 32 KiB
constexpr int kWQBins = 1024;                  // sweeps 1, 2: 10 bits each, kQSlots histograms of a launch — 32 KiB
constexpr int kWQMaxSlots = kQMaxProbs;        // one target per probability

struct WQColState {  // per column of a batch, in the workspace
  double mean, var, ess;
  uint64_t W;                    // mass of the valid entries
  uint64_t tres[kWQMaxSlots];    // target j: the mass still to reach inside its slot (1 .. the slot's mass)
  uint32_t nan, kmin, kmax, R;   // NaN entries; min / max key over the entries of positive mass; slots in use
  uint32_t prefix[kWQMaxSlots];  // slot -> key prefix (12 bits after pick 0, 22 after pick 1)
  uint32_t tslot[kWQMaxSlots];   // target j -> slot
};

struct WQArgs {
  const float* base[kQMaxSegs];
  uint64_t stride[kQMaxSegs];
  uint32_t first[kQMaxSegs];
  int32_t n_seg, Q;
  uint32_t n, per, B;
  uint32_t col0, cols;
  double probs[kQMaxProbs];
  const float* logw;
  uint64_t logw_stride;
  uint32_t V, by_v;     // weight columns; V <= the batch's size: the batch evaluates all V rows, else one row per column
  uint32_t rows;        // ... of the batch's prologue: V or cols
  int32_t frac;
  uint32_t* wmax;       // [rows of the batch]: the max key over the non-NaN log-weights (0: none)
  uint32_t* mass;       // the mass table: row r at mass + r * mstride (+ the row's phase when it sits in the workspace)
  uint64_t mstride;
  uint32_t phased, mass_by_v;  // rows carry the alignment phase of their first column; rows are indexed by weight column
  uint64_t* hist0;      // [cols][kWQBins0]
  uint64_t* hist;       // [cols][kWQMaxSlots][kWQBins]
  double* part;         // [cols][3][kQMaxBlocks]: the blocks' S1, S0, S2
  WQColState* st;       // [cols]
  float* quant;
  double* stats;
};

GJX_DEV const float* wq_column(const WQArgs& A, uint32_t c) {  // (q_column on this argument block)
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
// Row y of the batch's prologue: its weight column, its row of the mass table and the row's first entry.  A workspace row is
// shifted by the 16-byte phase of the first data column it weighs (column v where the batch holds all V rows, else the
// batch's column y), so that the x quads and the mass quads of that column — and of every column of the same phase: the
// padded history rows, [T, m] paths with m % 4 == 0 — are aligned together.
GJX_DEV uint32_t wq_weight_col(const WQArgs& A, uint32_t y) { return A.by_v ? y : (A.col0 + y) % A.V; }
GJX_DEV uint32_t* wq_mass_row(const WQArgs& A, uint32_t y) {
  const uint32_t v = wq_weight_col(A, y);
  uint32_t* row = A.mass + (size_t)(A.mass_by_v ? v : y) * A.mstride;
  if (A.phased) row += (uint32_t)((uintptr_t)wq_column(A, A.by_v ? v : A.col0 + y) >> 2) & 3u;
  return row;
}
GJX_DEV uint32_t wq_row_of_column(const WQArgs& A, uint32_t cb) { return A.by_v ? (A.col0 + cb) % A.V : cb; }

struct __attribute__((packed, aligned(4))) WQuad {  // four masses at 4-byte alignment: one 16-byte load all the same
  uint32_t x, y, z, w;
};

__global__ __launch_bounds__(kBlock) void k_wquant_clear(WQArgs A) {
  const size_t i0 = (size_t)blockIdx.x * kBlock + threadIdx.x, step = (size_t)gridDim.x * kBlock;
  const size_t n0 = (size_t)A.cols * kWQBins0, n1 = (size_t)A.cols * kWQMaxSlots * kWQBins;
  for (size_t i = i0; i < n0; i += step) A.hist0[i] = 0ull;
  for (size_t i = i0; i < n1; i += step) A.hist[i] = 0ull;
  for (size_t i = i0; i < A.cols; i += step) {
    A.st[i].kmin = 0xffffffffu;
    A.st[i].kmax = 0u;
    A.st[i].R = 0u;
    A.st[i].nan = 0u;
  }
  for (size_t i = i0; i < A.rows; i += step) A.wmax[i] = 0u;  // (below the key of -inf, 0x007fffff: no non-NaN log-weight yet)
}

// The prologue: pass 0 takes each weight row's maximum as an order key (integer atomics: any order), pass 1 writes the masses.
template <int PASS>
__global__ __launch_bounds__(kBlock) void k_wquant_mass(WQArgs A) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t y = blockIdx.y;
  const float* lw = A.logw + (size_t)wq_weight_col(A, y) * A.logw_stride;
  const uint32_t b0 = blockIdx.x * A.per, b1 = A.n - b0 < A.per ? A.n : b0 + A.per;
  if (PASS == 0) {
    uint32_t k = 0u;
    for (uint32_t i = b0 + threadIdx.x; i < b1; i += kBlock) {
      const uint32_t ki = psis_key(lw[i]);
      k = ki != 0xffffffffu && ki > k ? ki : k;
    }
    k = wave_last_u32(wave_scan_u32(k, 0u, [](uint32_t a, uint32_t b) { return a > b ? a : b; }));
    if ((threadIdx.x & (kWave - 1)) == 0 && k) atomicMax(&A.wmax[y], k);
  } else {
    const uint32_t km = A.wmax[y];
    const float m = km ? psis_unkey(km) : -__builtin_inff();
    uint32_t* row = wq_mass_row(A, y);
    for (uint32_t i = b0 + threadIdx.x; i < b1; i += kBlock) {
      const float l = lw[i];
      row[i] = l > -__builtin_inff() ? (uint32_t)fixw(l, m, A.frac) : 0u;  // (-inf weighs nothing, also as the maximum)
    }
  }
#endif
}

// +mass into sh[bin] for every lane with `on`, aggregated inside the wave: q_hist_add's peel, the leader adding the SUM of
// the masses of the lanes that share its bin.  A mass is at most 2^31: its low 16 and its high 16 bits are summed apart
// over the wave as u32 (a u32 add takes its DPP operand directly; 64 lanes stay below 2^22 in either half).
GJX_DEV void wq_hist_add(uint64_t* sh, uint32_t bin, uint32_t mass, bool on) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  uint64_t live = __ballot(on);
#pragma unroll
  for (int r = 0; r < kQPeel; ++r) {
    if (!live) break;
    const int leader = __builtin_ctzll(live);
    const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
    const bool mine = on && bin == d;
    const uint64_t same = __ballot(mine);
    const uint32_t lo = (uint32_t)wave_sum_int((int)(mine ? mass & 0xffffu : 0u));
    const uint32_t hi = (uint32_t)wave_sum_int((int)(mine ? mass >> 16 : 0u));
    if ((int)lane == leader) atomicAdd(reinterpret_cast<unsigned long long*>(&sh[d]), ((unsigned long long)hi << 16) + lo);
    live &= ~same;
  }
  if ((live >> lane) & 1ull) atomicAdd(reinterpret_cast<unsigned long long*>(&sh[bin]), (unsigned long long)mass);
}

template <int SWEEP>
__global__ __launch_bounds__(kBlock) void k_wquant_sweep(WQArgs A, uint32_t slot0) {
#if defined(__HIP_DEVICE_COMPILE__)
  // sweep 0: 4096 bins; sweeps 1, 2: kQSlots x 1024 bins — 32 KiB exactly either way, five workgroups per CU
  __shared__ uint64_t sh[kWQBins0];
  const uint32_t t = threadIdx.x, cb = blockIdx.y, b = blockIdx.x;
  WQColState* st = A.st + cb;
  uint32_t nslots = 0, p0 = 0, p1 = 0, p2 = 0, p3 = 0;
  double mean = 0.0;
  if (SWEEP > 0) {
    const uint32_t R = st->R;
    if (R <= slot0) return;  // (workgroup-uniform: a column with fewer slots, or without mass)
    nslots = R - slot0 < (uint32_t)kQSlots ? R - slot0 : (uint32_t)kQSlots;
    p0 = st->prefix[slot0];
    p1 = nslots > 1u ? st->prefix[slot0 + 1u] : 0xffffffffu;
    p2 = nslots > 2u ? st->prefix[slot0 + 2u] : 0xffffffffu;
    p3 = nslots > 3u ? st->prefix[slot0 + 3u] : 0xffffffffu;
    mean = st->mean;
  }
  const uint32_t nbins = SWEEP == 0 ? (uint32_t)kWQBins0 : nslots * (uint32_t)kWQBins;
  for (uint32_t i = t; i < nbins; i += kBlock) sh[i] = 0ull;
  __syncthreads();
  const bool squares = SWEEP == 1 && slot0 == 0;

  // the block [b0, b1) of column x and of its mass row: head, quads aligned by x, tail
  const float* x = wq_column(A, A.col0 + cb);
  const uint32_t* mq = wq_mass_row(A, wq_row_of_column(A, cb));
  const uint32_t b0 = b * A.per, b1 = A.n - b0 < A.per ? A.n : b0 + A.per;
  const uint32_t a = (uint32_t)((uintptr_t)x >> 2) & 3u;
  uint32_t head = (4u - ((a + b0) & 3u)) & 3u;
  if (head > b1 - b0) head = b1 - b0;
  const uint32_t q0 = b0 + head, nq = (b1 - q0) >> 2, tail0 = q0 + 4u * nq, ntail = b1 - tail0;
  const float4* xq = reinterpret_cast<const float4*>(x + q0);
  const WQuad* wq = reinterpret_cast<const WQuad*>(mq + q0);

  double acc = 0.0, acc0 = 0.0;
  uint32_t kmin = 0xffffffffu, kmax = 0u, nan = 0u;
  auto entry = [&](float v, uint32_t q, bool on) {
    const uint32_t k = psis_key(v);
    const bool pos = on && k != 0xffffffffu && q != 0u;  // (a zero mass adds nothing anywhere, also before an infinite x)
    if (SWEEP == 0) {
      wq_hist_add(sh, k >> 20, q, pos);  // (bin 4095 would be the NaNs alone: they are counted, not weighed)
      nan += on && k == 0xffffffffu ? 1u : 0u;
      if (pos) {
        const double dq = (double)q;
        acc = acc + dq * (double)v;
        acc0 = acc0 + dq * dq;
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
      }
    } else {
      if (squares && pos) {
        const double d = (double)v - mean;
        acc = acc + (double)q * (d * d);
      }
      const uint32_t p = SWEEP == 1 ? k >> 20 : k >> 10;
      const uint32_t digit = SWEEP == 1 ? (k >> 10) & 1023u : k & 1023u;
      const uint32_t slot = p == p0 ? 0u : p == p1 ? 1u : p == p2 ? 2u : p == p3 ? 3u : 4u;
      wq_hist_add(sh, (slot & 3u) * (uint32_t)kWQBins + digit, q, pos && slot < 4u);
    }
  };
  for (uint32_t v0 = 0; v0 < nq; v0 += kBlock * kQUnroll) {  // (wave-uniform trip count: the ballots see whole waves)
    float4 q[kQUnroll];
    WQuad w[kQUnroll];
    bool on[kQUnroll];
#pragma unroll
    for (int u = 0; u < kQUnroll; ++u) {
      const uint32_t v = v0 + (uint32_t)u * kBlock + t;
      on[u] = v < nq;
      q[u] = on[u] ? xq[v] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      w[u] = on[u] ? wq[v] : WQuad{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < kQUnroll; ++u) {
      entry(q[u].x, w[u].x, on[u]);
      entry(q[u].y, w[u].y, on[u]);
      entry(q[u].z, w[u].z, on[u]);
      entry(q[u].w, w[u].w, on[u]);
    }
  }
  {
    const bool on = t < head + ntail;
    const uint32_t i = t < head ? b0 + t : tail0 + (t - head);
    entry(on ? x[i] : 0.0f, on ? mq[i] : 0u, on);
  }

  __syncthreads();
  uint64_t* g = SWEEP == 0 ? A.hist0 + (size_t)cb * kWQBins0 : A.hist + ((size_t)cb * kWQMaxSlots + slot0) * kWQBins;
  for (uint32_t i = t; i < nbins; i += kBlock) {
    const uint64_t c = sh[i];
    if (c) atomicAdd(reinterpret_cast<unsigned long long*>(&g[i]), (unsigned long long)c);
  }
  if (SWEEP == 0) {  // the integer statistics: a wave reduction, then one atomic per wave (any order)
    const uint32_t lo = wave_last_u32(wave_scan_u32(kmin, 0xffffffffu, [](uint32_t p, uint32_t q) { return p < q ? p : q; }));
    const uint32_t hi = wave_last_u32(wave_scan_u32(kmax, 0u, [](uint32_t p, uint32_t q) { return p > q ? p : q; }));
    const uint32_t nn = (uint32_t)wave_sum_int((int)nan);
    if ((t & (kWave - 1)) == 0) {
      if (lo != 0xffffffffu) {
        atomicMin(&st->kmin, lo);
        atomicMax(&st->kmax, hi);
      }
      if (nn) atomicAdd(&st->nan, nn);
    }
  }
  if (SWEEP == 0 || squares) {  // the lanes' sums: the balanced tree in lane order, in the LDS the flushed bins leave free
    __syncthreads();
    double* red = reinterpret_cast<double*>(sh);
    red[t] = acc;
    red[kBlock + t] = acc0;
    __syncthreads();
    for (uint32_t w = 1; w < (uint32_t)kBlock; w <<= 1) {
      if ((t & (2u * w - 1u)) == 0u) {
        red[t] = red[t] + red[t + w];
        if (SWEEP == 0) red[kBlock + t] = red[kBlock + t] + red[kBlock + t + w];
      }
      __syncthreads();
    }
    if (t == 0) {
      double* part = A.part + (size_t)cb * 3 * kQMaxBlocks + b;
      part[SWEEP == 0 ? 0 : 2 * kQMaxBlocks] = red[0];
      if (SWEEP == 0) part[kQMaxBlocks] = red[kBlock];
    }
  }
#endif
}

// If the mass target r (1-based, inclusive) falls into this thread's NB bins c (which start at exclusive mass ex): the
// bin and the mass still to reach inside it, for target tt.  A bin without mass is never the answer.
template <int NB>
GJX_DEV void wq_locate(uint64_t r, uint64_t ex, const uint64_t (&c)[NB], uint64_t sum, uint32_t shift_prefix, uint32_t* bin_out,
                       uint64_t* res_out, uint32_t tt) {
  if (r <= ex || r - ex > sum) return;
  uint64_t cum = ex;
  bool found = false;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    if (!found && r - cum <= c[i]) {
      bin_out[tt] = shift_prefix | ((uint32_t)NB * threadIdx.x + (uint32_t)i);
      res_out[tt] = r - cum;
      found = true;
    }
    cum += c[i];
  }
}

// Thread 0: the targets' new prefixes nbin[0 .. T) -> distinct slots, into the column's state.
GJX_DEV void wq_merge(WQColState* st, uint32_t T, const uint32_t* nbin, const uint64_t* nres, uint32_t* spfx) {
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
    st->tres[tt] = nres[tt];
  }
  st->R = R;
}

GJX_DEV double wq_fold(const WQArgs& A, uint32_t cb, uint32_t which) {  // the blocks' sums in index order from +0
  double s = 0.0;
  for (uint32_t b = 0; b < A.B; ++b) s = s + A.part[((size_t)cb * 3 + which) * kQMaxBlocks + b];
  return s;
}

template <int STAGE>
__global__ __launch_bounds__(kBlock) void k_wquant_pick(WQArgs A) {
#if defined(__HIP_DEVICE_COMPILE__)
  __shared__ uint64_t scan[kBlock / kWave], nres[kWQMaxSlots], tr[kWQMaxSlots];
  __shared__ uint32_t nbin[kWQMaxSlots], spfx[kWQMaxSlots], ts[kWQMaxSlots], oldp[kWQMaxSlots];
  const uint32_t t = threadIdx.x, cb = blockIdx.x;
  WQColState* st = A.st + cb;
  const uint32_t T = (uint32_t)A.Q;
  if (t < (uint32_t)kWQMaxSlots) {
    nbin[t] = 0u;
    nres[t] = 0ull;
  }
  if (STAGE == 0) {
    constexpr int NB = kWQBins0 / kBlock;
    const uint64_t* h = A.hist0 + (size_t)cb * kWQBins0 + (size_t)NB * t;
    uint64_t c[NB], sum = 0, W;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      c[i] = h[i];
      sum += c[i];
    }
    const uint64_t ex = block_scan_excl(sum, scan, W);
#pragma unroll
    for (int j = 0; j < kQMaxProbs; ++j)
      if (j < A.Q && W > 0ull) {
        const double up = __builtin_ceil(A.probs[j] * (double)W);
        uint64_t tj = up < 1.0 ? 1ull : (uint64_t)up;  // (up <= 2^62: the conversion is exact)
        tj = tj > W ? W : tj;
        wq_locate<NB>(tj, ex, c, sum, 0u, nbin, nres, (uint32_t)j);
      }
    __syncthreads();
    if (t == 0) {
      st->W = W;
      wq_merge(st, W > 0ull ? T : 0u, nbin, nres, spfx);
      const double dw = (double)W;
      st->mean = wq_fold(A, cb, 0) / dw;
      st->ess = dw * dw / wq_fold(A, cb, 1);
    }
    return;
  }
  constexpr int NB = kWQBins / kBlock;
  const uint64_t W = st->W;
  const uint32_t R = st->R;
  if (t < (uint32_t)kWQMaxSlots) {
    ts[t] = st->tslot[t];
    tr[t] = st->tres[t];
    oldp[t] = st->prefix[t];
  }
  __syncthreads();
  for (uint32_t s = 0; s < R; ++s) {
    uint64_t* h = A.hist + ((size_t)cb * kWQMaxSlots + s) * kWQBins + (size_t)NB * t;
    uint64_t c[NB], sum = 0, total;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      c[i] = h[i];
      sum += c[i];
      if (STAGE == 1) h[i] = 0ull;  // (sweep 2 fills the same histograms)
    }
    const uint64_t ex = block_scan_excl(sum, scan, total);
    const uint32_t shifted = oldp[s] << 10;
    for (uint32_t tt = 0; tt < T; ++tt)
      if (ts[tt] == s) wq_locate<NB>(tr[tt], ex, c, sum, shifted, nbin, nres, tt);
  }
  __syncthreads();
  if (STAGE == 1) {
    if (t == 0) {
      wq_merge(st, W > 0ull ? T : 0u, nbin, nres, spfx);
      st->var = wq_fold(A, cb, 2) / (double)W;
    }
    return;
  }
  // the keys are complete: the outputs
  const size_t col = (size_t)A.col0 + cb;
  if (t < (uint32_t)A.Q) A.quant[col * A.Q + t] = W ? psis_unkey(nbin[t]) : u2f(0x7fc00000u);
  if (t == 0) {
    const double qnan = __builtin_nan("");
    double* o = A.stats + col * 6;
    o[0] = (double)st->nan;
    o[1] = W ? st->mean : qnan;
    o[2] = W ? st->var : qnan;
    o[3] = W ? (double)psis_unkey(st->kmin) : qnan;
    o[4] = W ? (double)psis_unkey(st->kmax) : qnan;
    o[5] = W ? st->ess : qnan;
  }
#endif
}

}  // namespace gjx
