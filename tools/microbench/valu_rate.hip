// VALU issue rate on MI355X: wave-instructions per second for a few instruction kinds, at full occupancy with
// 8 independent chains per lane (no dependency stalls), plus the shader clock seen by clock64() vs wall time.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
template <int KIND>
__global__ __launch_bounds__(256) void k_rate(float* out, int iters, long long* clk) {
  float v[8];
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { v[k] = threadIdx.x * 0.001f + k; w[k] = threadIdx.x * 2654435761u + k; }
  uint32_t sk = (uint32_t)iters * 0x9E3779B9u;  // a wave-uniform round key: it lives in a scalar register
  float sel_lo = iters * 0.000125f, sel_hi = iters * 0.00075f;  // (run-time values either side of the threshold: nothing folds)
  asm volatile("" : "+v"(sel_lo), "+v"(sel_hi));
  const long long t0 = clock64();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (KIND == 0) v[k] = __builtin_fmaf(v[k], 1.0001f, 0.5f);                       // v_fma_f32
      if (KIND == 1) w[k] = w[k] ^ (w[k] >> 3);                                         // shift + xor (2 ops)
      if (KIND == 2) { const uint64_t p = (uint64_t)w[k] * 0xD2511F53u; w[k] = (uint32_t)(p >> 32) ^ (uint32_t)p; }  // v_mad_u64_u32 + xor
      if (KIND == 3) v[k] = __builtin_amdgcn_sqrtf(v[k]) + 1.5f;                        // v_sqrt_f32 + add
      if (KIND == 4) v[k] = v[k] > 2.0f ? v[k] - 1.0f : v[k] + 0.75f;                   // cmp + sub + add + cndmask
      if (KIND == 5) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(w[k]) : "v"(w[(k + 1) & 7]));  // v_xor_b32 alone (no v_xor3 folding)
      if (KIND == 6) v[k] = v[k] > 2.0f ? sel_lo : sel_hi;                              // v_cmp_lt_f32 + v_cndmask_b32 (mask through VCC / an SGPR pair)
      if (KIND == 8) { v[k] = (float)w[k]; w[k] = __float_as_uint(v[k]) + 3u; }         // v_cvt_f32_u32 + add
      // the Philox round's three-input XOR (hi ^ c1 ^ round key, the key scalar) as ONE v_bitop3_b32 and as the v_xor_b32 pair
      if (KIND == 9) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(w[k]) : "v"(w[(k + 1) & 7]), "s"(sk));
      if (KIND == 10) asm volatile("v_xor_b32 %0, %0, %1\n\tv_xor_b32 %0, %2, %0" : "+v"(w[k]) : "v"(w[(k + 1) & 7]), "s"(sk));
      // ... and in the round's own pattern (multiply, XOR3 of its two words with the key, multiply, ...)
      if (KIND == 11 || KIND == 12) {
        const uint64_t p = (uint64_t)0xD2511F53u * w[k];  // v_mad_u64_u32
        if (KIND == 11) asm volatile("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(w[k]) : "v"((uint32_t)(p >> 32)), "v"((uint32_t)p), "s"(sk));
        else asm volatile("v_xor_b32 %0, %1, %2\n\tv_xor_b32 %0, %3, %0" : "=&v"(w[k]) : "v"((uint32_t)(p >> 32)), "v"((uint32_t)p), "s"(sk));
      }
      if (KIND == 7) { uint64_t t = ((uint64_t)w[k] << 32) | w[(k + 1) & 7]; t += 0x123456789ull * (k + 1); w[k] = (uint32_t)(t >> 32) ^ (uint32_t)t; }  // 64-bit add + xor
    }
    if (KIND >= 9) sk += 0x9E3779B9u;  // (the key schedule: scalar, beside the vector issue)
  }
  const long long t1 = clock64();
  float s = 0; uint32_t x = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) { s += v[k]; x ^= w[k]; }
  if (s == -1.0f || x == 0x12345u) out[blockIdx.x] = s;
  if (blockIdx.x == 0 && threadIdx.x == 0) clk[0] = t1 - t0;
}
template <int KIND>
void run(const char* name, int ops_per_iter, float* out, long long* clk) {
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  const int iters = 4000, grid = 256 * 8 * 4;  // 8 workgroups of 4 waves per CU, 4 rounds
  hipLaunchKernelGGL(k_rate<KIND>, dim3(grid), dim3(256), 0, 0, out, iters, clk);
  hipEventRecord(a);
  hipLaunchKernelGGL(k_rate<KIND>, dim3(grid), dim3(256), 0, 0, out, iters, clk);
  hipEventRecord(b); hipEventSynchronize(b);
  float ms; hipEventElapsedTime(&ms, a, b);
  long long c; hipMemcpy(&c, clk, 8, hipMemcpyDeviceToHost);
  const double waves = (double)grid * 4, winstr = waves * iters * 8.0 * ops_per_iter;
  printf("%-28s %.3f ms  %.3e wave-instr/s  (= %.2f cycles per wave-instr per SIMD at 2.4 GHz)  clock64 span of one wave %lld\n", name, ms,
         winstr / (ms * 1e-3), 1024.0 * 2.4e9 / (winstr / (ms * 1e-3)), c);
}
typedef float float2v __attribute__((ext_vector_type(2)));
// CHAINS independent chains of packed multiplies per lane, 8 instructions per iteration either way: CHAINS = 8 never waits
// on its own result; CHAINS = 1 is ONE dependent chain (each v_pk_mul_f32 reads the pair the one before wrote) — the case
// that draws the hazard wait states, hidden only by the SIMD's other waves
template <int CHAINS>
__global__ __launch_bounds__(256) void k_pk(float* out, int iters) {
  float2v v[CHAINS];
#pragma unroll
  for (int k = 0; k < CHAINS; ++k) v[k] = float2v{threadIdx.x * 0.001f + k, threadIdx.x * 0.002f + k};
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k % CHAINS] = v[k % CHAINS] * float2v{1.0001f, 0.9999f};  // v_pk_mul_f32
  }
  float s = 0;
#pragma unroll
  for (int k = 0; k < CHAINS; ++k) s += v[k].x + v[k].y;
  if (s == -1.0f) out[blockIdx.x] = s;
}
// 8 fmas per iteration and, with LDS = 1, one 8-byte LDS read (ds_read_b64) whose index comes from the value read before:
// what a table lookup costs next to vector work (the Box-Muller tables of the importance kernels are two such reads per
// transform).  Reported per iteration; the difference to LDS = 0 is the read's share of the issue time.
template <int LDS>
__global__ __launch_bounds__(256) void k_lds(float* out, int iters) {
  __shared__ uint2 tab[256];
  tab[threadIdx.x] = make_uint2(threadIdx.x * 2654435761u, threadIdx.x + 1u);
  __syncthreads();
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = threadIdx.x * 0.001f + k;
  uint32_t idx = threadIdx.x, acc = 0;
  for (int i = 0; i < iters; ++i) {
    if (LDS) { const uint2 e = tab[idx & 255u]; idx = e.x >> 7; acc ^= e.y; }
#pragma unroll
    for (int k = 0; k < 8; ++k) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(v[k]) : "v"(1.0001f), "v"(0.5f));  // (kept unpacked)
  }
  float s = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += v[k];
  if (s == -1.0f || acc == 0x12345u) out[blockIdx.x] = s + (float)idx;
}
template <class K>
void run_plain(const char* name, K kernel, double instr_per_iter, float* out) {
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  const int iters = 4000, grid = 256 * 8 * 4;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, 0, out, iters);
  hipEventRecord(a);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, 0, out, iters);
  hipEventRecord(b); hipEventSynchronize(b);
  float ms; hipEventElapsedTime(&ms, a, b);
  const double winstr = (double)grid * 4 * iters * instr_per_iter;
  printf("%-28s %.3f ms  %.3e wave-instr/s  (= %.2f cycles per wave-instr per SIMD at 2.4 GHz)\n", name, ms, winstr / (ms * 1e-3),
         1024.0 * 2.4e9 / (winstr / (ms * 1e-3)));
}
int main() {
  float* out; long long* clk; hipMalloc(&out, 1 << 20); hipMalloc(&clk, 8);
  run<0>("fma_f32", 1, out, clk);
  run<1>("lshr+xor", 2, out, clk);
  run<2>("mad_u64_u32+xor", 2, out, clk);
  run<3>("sqrt_f32+add", 2, out, clk);
  run<4>("cmp+sub+add+cndmask", 4, out, clk);
  run<7>("add_u64+xor", 2, out, clk);
  run<5>("xor_b32", 1, out, clk);
  run<6>("cmp+cndmask (vcc)", 2, out, clk);
  run<8>("cvt_f32_u32+add", 2, out, clk);
  run<9>("bitop3_b32 (v, v, s)", 1, out, clk);
  run<10>("xor_b32 pair (v, v, s)", 2, out, clk);
  run<11>("mad_u64_u32+bitop3_b32", 2, out, clk);
  run<12>("mad_u64_u32+xor_b32 pair", 3, out, clk);
  run_plain("pk_mul_f32, 8 chains", k_pk<8>, 8.0, out);
  run_plain("pk_mul_f32, 1 dependent chain", k_pk<1>, 8.0, out);
  run_plain("8 fma (per iteration)", k_lds<0>, 1.0, out);
  run_plain("8 fma + ds_read_b64 (per iteration)", k_lds<1>, 1.0, out);
  return 0;
}
