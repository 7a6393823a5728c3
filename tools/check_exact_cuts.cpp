// check_exact_cuts.cpp — the sweeps behind the "same bits" claims of the algebraic cuts in gjx_device.hpp (bm_pair's radius
// word, sqrt_pos, logpdf_normal_pre's fused overload).  Host only; the forms are restated here operation for operation
// (every rounding explicit: build with -ffp-contract=off), the shipped form next to the cut one.
//
//   g++ -O2 -std=c++17 -fopenmp -ffp-contract=off [-mfma] -o check_exact_cuts tools/check_exact_cuts.cpp && ./check_exact_cuts
//
// Exit status 0: no mismatch inside the stated domains.  1: at least one (the first few are printed).  `--quick` runs every
// sweep on a 1/64 sample of its range (a smoke run of the tool itself, not of the claims).
//
//   A  the radius word of bm_pair: t over all 2^32 words.
//   B  sqrt_pos: every float of [1e-7, 45] and +-0, the reciprocal-square-root estimate set to the correctly rounded
//      1/sqrt(x) offset by -2 .. +2 ulp (the hardware's v_rsq_f32 is specified to 1 ulp), against sqrtf.
//   D  the residual x*rs - loc*rs against fma(-rs, loc, x*rs), rs = 2^0 .. 2^8, over seeded random bit patterns and edges.
//      Domain: loc*rs does not overflow (loc infinite or NaN is inside the domain).
//   F  (-0.5 d) d - L against fma(d*d, -0.5, -L), |L| >= 2^-100, over seeded random bit patterns and edges.
//      Domain: d*d does not overflow (d infinite or NaN is inside the domain).
//   D+F composed, as the generated kernels call them.
// Two NaNs compare equal whatever their payloads (a NaN log-density is a NaN weight either way).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

static inline uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline bool same(float a, float b) { return (a != a && b != b) || f2u(a) == f2u(b); }

// --- A
static inline uint32_t radius_t_shipped(uint32_t w) {
  const float u = ((float)w + 1.0f) * 2.3283064365386963e-10f;
  return f2u(u) - 0x3f3504f3u;
}
static inline uint32_t radius_t_cut(uint32_t w) { return f2u((float)w + 1.0f) - (0x3f3504f3u + (32u << 23)); }

// --- B (y: the estimate of 1/sqrt(max(x, 1e-30)))
static inline float sqrt_pos_cut(float x, float y) {
  float s = x * y, h = 0.5f * y;
  const float e = fmaf(-h, s, 0.5f);
  h = fmaf(h, e, h);
  s = fmaf(s, e, s);
  return fmaf(fmaf(-s, s, x), h, s);
}
static inline float rsq_rn(float x) { return (float)(1.0 / std::sqrt((double)x)); }

// --- D, F
static inline float resid_shipped(float x, float loc, float rs) { return x * rs - loc * rs; }
static inline float resid_cut(float x, float loc, float rs) { return fmaf(-rs, loc, x * rs); }
static inline float halfsq_shipped(float d, float L) { return (-0.5f * d) * d - L; }
static inline float halfsq_cut(float d, float L) { return fmaf(d * d, -0.5f, -L); }

static inline uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static inline bool finite_f(float v) { return v - v == 0.0f; }
static inline bool in_domain_D(float loc, float rs) { return !finite_f(loc) || finite_f(loc * rs); }
static inline bool in_domain_F(float d) { return !finite_f(d) || finite_f(d * d); }

static long long g_bad = 0;
static void report(const char* what, uint32_t a, uint32_t b, uint32_t c, float got, float want) {
#pragma omp critical
  {
    if (g_bad++ < 8) std::printf("  MISMATCH %s: inputs %08x %08x %08x -> %08x, shipped %08x\n", what, a, b, c, f2u(got), f2u(want));
  }
}

int main(int argc, char** argv) {
  const bool quick = argc > 1 && std::strcmp(argv[1], "--quick") == 0;
  const uint64_t step = quick ? 64 : 1;

  {  // A
    long long bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static)
    for (int64_t w = 0; w < (int64_t)1 << 32; w += (int64_t)step)
      if (radius_t_shipped((uint32_t)w) != radius_t_cut((uint32_t)w)) { ++bad; report("A", (uint32_t)w, 0, 0, 0.0f, 0.0f); }
    std::printf("A radius word: %llu words, %lld mismatches\n", (unsigned long long)(((uint64_t)1 << 32) / step), bad);
  }

  {  // B
    const uint32_t lo = f2u(1e-7f), hi = f2u(45.0f);
    for (int off = -2; off <= 2; ++off) {
      long long bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static)
      for (int64_t b = lo; b <= (int64_t)hi; b += (int64_t)step) {
        const float x = u2f((uint32_t)b), y = u2f(f2u(rsq_rn(x)) + (uint32_t)off);
        const float r = sqrt_pos_cut(x, y), want = std::sqrt(x);
        if (!same(r, want)) { ++bad; report("B", (uint32_t)b, f2u(y), 0, r, want); }
      }
      std::printf("B sqrt_pos, estimate %+d ulp: %llu floats, %lld mismatches\n", off, (unsigned long long)((hi - lo) / step + 1), bad);
    }
    const float y0 = rsq_rn(1e-30f);  // what max(x, 1e-30f) hands the estimate at a zero
    for (int off = -2; off <= 2; ++off) {
      const float y = u2f(f2u(y0) + (uint32_t)off);
      if (f2u(sqrt_pos_cut(0.0f, y)) != 0x00000000u) report("B +0", 0, f2u(y), 0, sqrt_pos_cut(0.0f, y), 0.0f);
      if (f2u(sqrt_pos_cut(-0.0f, y)) != 0x80000000u) report("B -0", 0x80000000u, f2u(y), 0, sqrt_pos_cut(-0.0f, y), -0.0f);
    }
    std::printf("B zeros: +0 -> +0, -0 -> -0 for the five estimates\n");
  }

  const uint32_t edge_bits[] = {
      0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x00800000u, 0x3f800000u, 0xbf800000u, 0x3f000000u, 0x40490fdbu,
      0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f000000u, 0x7e800000u, 0x5f7fffffu, 0xdf7fffffu,
      0x20800000u /* 2^-62 */, 0x207fffffu, 0x203504f3u /* 2^-62.5: d*d at 2^-125 */, 0x203504f2u, 0x203504f4u, 0xa03504f3u, 0x20000000u};
  const int n_edges = (int)(sizeof(edge_bits) / sizeof(edge_bits[0]));
  const int64_t n_rand = quick ? (int64_t)1 << 18 : (int64_t)1 << 24;

  {  // D
    long long bad = 0, outside = 0, checked = 0;
    for (int k = 0; k <= 8; ++k) {
      const float rs = std::ldexp(1.0f, k);
      for (int i = 0; i < n_edges; ++i)
        for (int j = 0; j < n_edges; ++j) {
          const float x = u2f(edge_bits[i]), loc = u2f(edge_bits[j]);
          if (!in_domain_D(loc, rs)) { ++outside; continue; }
          ++checked;
          if (!same(resid_cut(x, loc, rs), resid_shipped(x, loc, rs))) { ++bad; report("D edge", edge_bits[i], edge_bits[j], f2u(rs), resid_cut(x, loc, rs), resid_shipped(x, loc, rs)); }
        }
#pragma omp parallel for reduction(+ : bad, outside, checked) schedule(static)
      for (int64_t c = 0; c < n_rand; ++c) {
        uint64_t s = 0xD00Dull * 1000003ull + (uint64_t)k * 0x100000000ull + (uint64_t)c;
        const uint64_t r = splitmix(s), r2 = splitmix(s);
        float x = u2f((uint32_t)r), loc = u2f((uint32_t)(r >> 32));
        if (r2 & 1u) loc = u2f(f2u(x) + (uint32_t)((r2 >> 8) & 0xffu) - 128u);  // half the pairs: neighbours (the difference cancels)
        if (!in_domain_D(loc, rs)) { ++outside; continue; }
        ++checked;
        if (!same(resid_cut(x, loc, rs), resid_shipped(x, loc, rs))) { ++bad; report("D", f2u(x), f2u(loc), f2u(rs), resid_cut(x, loc, rs), resid_shipped(x, loc, rs)); }
      }
    }
    std::printf("D residual, rs = 2^0 .. 2^8: %lld pairs, %lld mismatches (%lld pairs outside the domain: loc*rs overflows)\n", checked, bad, outside);
  }

  const uint32_t lognorm_bits[] = {0x0d800000u /* 2^-100 */, 0x8d800000u, 0x0d800001u, 0x3f6b3f8eu /* 0.9189385 */, 0x3e672f3cu /* about 0.2258 */,
                                   0xbe91e0a6u /* about -0.2849 */, 0x42c80000u, 0xc2c80000u, 0x7f7fffffu, 0xff7fffffu, 0x0e000000u /* 2^-99 */};
  const int n_ln = (int)(sizeof(lognorm_bits) / sizeof(lognorm_bits[0]));
  {  // F
    long long bad = 0, outside = 0, checked = 0;
    for (int l = 0; l < n_ln; ++l) {
      const float L = u2f(lognorm_bits[l]);
      for (int i = 0; i < n_edges; ++i) {
        const float d = u2f(edge_bits[i]);
        if (!in_domain_F(d)) { ++outside; continue; }
        ++checked;
        if (!same(halfsq_cut(d, L), halfsq_shipped(d, L))) { ++bad; report("F edge", edge_bits[i], lognorm_bits[l], 0, halfsq_cut(d, L), halfsq_shipped(d, L)); }
      }
      // every d whose square lies within a factor 2^+-1 of 2^-125, both signs
#pragma omp parallel for reduction(+ : bad, checked) schedule(static)
      for (int64_t b = 0x1f800000; b < 0x21000000; b += (int64_t)step)
        for (uint32_t sign = 0; sign < 2; ++sign) {
          const float d = u2f((uint32_t)b | (sign << 31));
          ++checked;
          if (!same(halfsq_cut(d, L), halfsq_shipped(d, L))) { ++bad; report("F 2^-125", f2u(d), lognorm_bits[l], 0, halfsq_cut(d, L), halfsq_shipped(d, L)); }
        }
    }
#pragma omp parallel for reduction(+ : bad, outside, checked) schedule(static)
    for (int64_t c = 0; c < 4 * n_rand; ++c) {
      uint64_t s = 0xF00Dull * 1000003ull + (uint64_t)c;
      const uint64_t r = splitmix(s);
      const float d = u2f((uint32_t)r);
      float L = u2f((uint32_t)(r >> 32));
      if (!finite_f(L) || std::fabs(L) < 7.8886090522101181e-31f) L = u2f(lognorm_bits[c % n_ln]);  // a literal log-normaliser: finite, |L| >= 2^-100
      if (!in_domain_F(d)) { ++outside; continue; }
      ++checked;
      if (!same(halfsq_cut(d, L), halfsq_shipped(d, L))) { ++bad; report("F", f2u(d), f2u(L), 0, halfsq_cut(d, L), halfsq_shipped(d, L)); }
    }
    std::printf("F half-square, |lognorm| >= 2^-100: %lld cases, %lld mismatches (%lld outside the domain: d*d overflows)\n", checked, bad, outside);
  }

  {  // D + F as the generated kernels call them: logpdf_normal_pre(x, loc, rs, lognorm, NormalExactCuts())
    long long bad = 0, outside = 0, checked = 0;
#pragma omp parallel for reduction(+ : bad, outside, checked) schedule(static)
    for (int64_t c = 0; c < 4 * n_rand; ++c) {
      uint64_t s = 0xDFull * 1000003ull + (uint64_t)c;
      const uint64_t r = splitmix(s), r2 = splitmix(s);
      const float rs = std::ldexp(1.0f, (int)(r2 % 9u));
      const float x = u2f((uint32_t)r);
      float loc = u2f((uint32_t)(r >> 32));
      if (r2 & 0x100u) loc = u2f(f2u(x) + (uint32_t)((r2 >> 16) & 0xffffu) - 32768u);
      const float L = u2f(lognorm_bits[(r2 >> 40) % n_ln]);
      const float d0 = resid_shipped(x, loc, rs);
      if (!in_domain_D(loc, rs) || !in_domain_F(d0)) { ++outside; continue; }
      ++checked;
      const float got = halfsq_cut(resid_cut(x, loc, rs), L), want = halfsq_shipped(d0, L);
      if (!same(got, want)) { ++bad; report("D+F", f2u(x), f2u(loc), f2u(rs), got, want); }
    }
    std::printf("D+F composed: %lld cases, %lld mismatches (%lld outside the domains)\n", checked, bad, outside);
  }

  std::printf("%s: %lld mismatches in all\n", g_bad ? "FAILED" : "ok", g_bad);
  return g_bad ? 1 : 0;
}
