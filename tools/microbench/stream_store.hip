// Streaming-store ceiling at the importance batch's shape: what the chip takes when 32 passes x 48.4 MB (1.55 GB) are written
// launch after launch into the same buffers, as `bench.py`'s 32-pass launches of the quad kernel write them.
//   grid (3907, 32), one 64-lane wave per workgroup; 12 columns; each lane one 16-byte store per column at
//   pass * 1 000 192 + row * 256 + 4 * lane floats (the last row of a pass is partial: n = 1e6).
// Between two stores a lane runs `chain` dependent fma steps (four chains, one per stored word), so the stores are spread
// over the wave's life as the kernel's are; chain 0 is the pure ceiling.  Kinds of store (template parameter):
//   plain | wt: write-through, the sc1 buffer store of gjx_device.hpp store16_at | nt: __builtin_nontemporal_store |
//   nt+wt: the same buffer store with the nt bit as well.
// Per kind and chain: us per pass and TB/s, median and minimum over the timed launches (HIP events round each launch, back to
// back, after an untimed ramp); the step time when a trivial one-workgroup kernel separates the launches (the dependent
// boundary, with and without dirty lines); the mean life of a wave (a run of its own, not timed).
//   hipcc --offload-arch=gfx950 -O3 -o stream_store stream_store.hip && ./stream_store [launches] [chain ...]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

constexpr uint32_t kRows = 3907, kPasses = 32, kCols = 12;
constexpr uint64_t kN = 1000000, kStride = 1000192;
enum { kPlain = 0, kWt = 1, kNt = 2, kNtWt = 3 };
static const char* const kNames[] = {"plain", "wt", "nt", "nt+wt"};
struct Cols { float* c[kCols]; };

typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
template <int K>
__device__ __forceinline__ void store16(float* ubase, uint32_t lane_bytes, v4u_t x) {
  if (K == kWt || K == kNtWt) {  // aux: bit 4 = sc1, bit 1 = nt (gfx94x / gfx950)
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(ubase, 0, 0x7fffffff, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(x, rs, (int)lane_bytes, 0, K == kWt ? 16 : 18);
  } else if (K == kNt) {
    __builtin_nontemporal_store(x, reinterpret_cast<v4u_t*>(reinterpret_cast<char*>(ubase) + lane_bytes));
  } else {
    *reinterpret_cast<v4u_t*>(reinterpret_cast<char*>(ubase) + lane_bytes) = x;
  }
}

template <int K, bool LIFE>
__global__ __launch_bounds__(64) void k_stream(Cols cols, int chain, float a, float b, unsigned* life) {
  const uint64_t t0 = LIFE ? wall_clock64() : 0;
  const uint32_t row = blockIdx.x, pass = blockIdx.y, lane = threadIdx.x;
  const uint64_t ub = (uint64_t)pass * kStride + (uint64_t)row * 256;
  const uint32_t lb = 16u * lane;
  if ((uint64_t)row * 256 + 4 * lane < kN) {  // (n a multiple of 4: a lane's four floats exist or none)
    float x = (float)lane, y = (float)row, z = (float)pass, w = 1.0f;
#pragma unroll
    for (uint32_t k = 0; k < kCols; ++k) {
      for (int j = 0; j < chain; ++j) {
        x = __builtin_fmaf(x, a, b); y = __builtin_fmaf(y, a, b); z = __builtin_fmaf(z, a, b); w = __builtin_fmaf(w, a, b);
      }
      v4u_t v;
      v[0] = __float_as_uint(x); v[1] = __float_as_uint(y); v[2] = __float_as_uint(z); v[3] = __float_as_uint(w) + k;
      store16<K>(cols.c[k] + ub, lb, v);
    }
  }
  if (LIFE) {  // (the wave's stores are issued, not drained: as the counters' wave cycles end); one word per wave
    const uint64_t dt = wall_clock64() - t0;
    if (lane == 0) life[pass * kRows + row] = (unsigned)dt;
  }
}
__global__ void k_trivial(unsigned* p) {
  if (threadIdx.x == 0) p[0] = p[0] + 1u;
}

struct Stat { double med, min; };
static Stat stat_of(std::vector<float>& ts) {
  std::sort(ts.begin(), ts.end());
  return {ts[ts.size() / 2], ts[0]};
}
#define CHECK(e)                                                                          \
  do {                                                                                    \
    const hipError_t err_ = (e);                                                          \
    if (err_ != hipSuccess) {                                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(err_));       \
      exit(1);                                                                            \
    }                                                                                     \
  } while (0)

template <int K>
static void run_kind(const Cols& cols, int chain, int launches, unsigned* tick, unsigned* life, double clock_mhz) {
  const dim3 grid(kRows, kPasses), block(64);
  const float a = 1.0001f, b = 0.5f;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (int r = 0; r < 10; ++r) k_stream<K, false><<<grid, block>>>(cols, chain, a, b, life);  // ramp, untimed
  CHECK(hipDeviceSynchronize());
  // back to back: events round each launch, nothing waits on the host between them
  std::vector<hipEvent_t> ev(2 * launches);
  for (auto& e : ev) CHECK(hipEventCreate(&e));
  for (int r = 0; r < launches; ++r) {
    CHECK(hipEventRecord(ev[2 * r]));
    k_stream<K, false><<<grid, block>>>(cols, chain, a, b, life);
    CHECK(hipEventRecord(ev[2 * r + 1]));
  }
  CHECK(hipDeviceSynchronize());
  std::vector<float> ts;
  for (int r = 0; r < launches; ++r) {
    float ms;
    CHECK(hipEventElapsedTime(&ms, ev[2 * r], ev[2 * r + 1]));
    ts.push_back(ms * 1e3f);
  }
  float whole_ms;
  CHECK(hipEventElapsedTime(&whole_ms, ev[0], ev[2 * launches - 1]));
  const Stat one = stat_of(ts);
  // launches separated by a trivial dependent kernel: the step is one streaming launch + one boundary pair
  CHECK(hipEventRecord(e0));
  for (int r = 0; r < launches; ++r) {
    k_stream<K, false><<<grid, block>>>(cols, chain, a, b, life);
    k_trivial<<<1, 64>>>(tick);
  }
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  float sep_ms;
  CHECK(hipEventElapsedTime(&sep_ms, e0, e1));
  // the mean life of a wave, in a run of its own
  std::vector<unsigned> ticks((size_t)kRows * kPasses);
  for (int r = 0; r < 3; ++r) k_stream<K, true><<<grid, block>>>(cols, chain, a, b, life);  // (the last one is read)
  CHECK(hipMemcpy(ticks.data(), life, ticks.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
  std::sort(ticks.begin(), ticks.end());
  const double bytes = 16.0 * kCols * (kN / 4) * kPasses;  // what a launch writes
  const double life_us = (double)ticks[ticks.size() / 2] / clock_mhz;  // (wall_clock64 ticks: hipDeviceAttributeWallClockRate)
  printf("%-6s chain %4d: per pass median %6.2f us (%5.2f TB/s)  min %6.2f us (%5.2f TB/s) | launch median %7.1f us, step back to back %7.1f us, "
         "step with a trivial kernel between %7.1f us | median wave life %6.2f us\n",
         kNames[K], chain, one.med / kPasses, bytes / (one.med * 1e-6) / 1e12, one.min / kPasses, bytes / (one.min * 1e-6) / 1e12, one.med,
         whole_ms * 1e3 / launches, sep_ms * 1e3 / launches, life_us);
  fflush(stdout);
  for (auto& e : ev) CHECK(hipEventDestroy(e));
  CHECK(hipEventDestroy(e0));
  CHECK(hipEventDestroy(e1));
}

int main(int argc, char** argv) {
  const int launches = argc > 1 ? std::max(50, atoi(argv[1])) : 50;
  std::vector<int> chains;
  for (int i = 2; i < argc; ++i) chains.push_back(std::max(0, atoi(argv[i])));
  if (chains.empty()) chains = {0, 32};
  Cols cols;
  for (uint32_t k = 0; k < kCols; ++k) CHECK(hipMalloc(&cols.c[k], kPasses * kStride * sizeof(float)));  // 12 x 128 MB
  unsigned* tick;
  unsigned* life;
  CHECK(hipMalloc(&tick, 64));
  CHECK(hipMalloc(&life, (size_t)kRows * kPasses * sizeof(unsigned)));
  int clock_khz = 0;
  CHECK(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, 0));
  const double clock_mhz = clock_khz > 0 ? clock_khz / 1e3 : 100.0;
  CHECK(hipMemset(tick, 0, 64));
  printf("grid (%u, %u) x 64 lanes, %u columns, %.1f MB per pass, %.2f GB per launch, %d timed launches per line, wall clock %.1f MHz\n", kRows,
         kPasses, kCols, 16.0 * kCols * (kN / 4) / 1e6, 16.0 * kCols * (kN / 4) * kPasses / 1e9, launches, clock_mhz);
  for (int chain : chains) {
    run_kind<kPlain>(cols, chain, launches, tick, life, clock_mhz);
    run_kind<kWt>(cols, chain, launches, tick, life, clock_mhz);
    run_kind<kNt>(cols, chain, launches, tick, life, clock_mhz);
    run_kind<kNtWt>(cols, chain, launches, tick, life, clock_mhz);
  }
  return 0;
}
