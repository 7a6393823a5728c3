// check_row_cuts.cpp — the sweeps behind the "same bits" claims of the row-loop cuts in gjx_device.hpp: the zero location fused
// into the transform's last product (bm_pair, PlusZero), rowfix's clamp and scaling, the wave maximum on ordered integer
// keys (wave_max_ordered) and the first accumulation (first_acc).  Host only; the forms are restated here operation for
// operation (every rounding explicit: build with -ffp-contract=off), the former form next to the cut one.  The transform's
// tables and steps are the oracle's (oracle/gjx_oracle_math.h o_bm_pair: the same constants, tools/gen_bm_tables.py).
//
//   g++ -O2 -std=c++17 -fopenmp -ffp-contract=off [-mfma] -o check_row_cuts tools/check_row_cuts.cpp && ./check_row_cuts
//
// Exit status 0: no mismatch inside the stated domains.  1: at least one (the first few are printed).
//
//   a  (r t) + (+0) against fma(r, t, +0), both outputs, over every angle word (the transform reads its top 24 bits: 2^24
//      distinct words) at the edge radius words — 0, 1, 0xFFFFFFFF (r = 0), 0xFFFFFF00 and its neighbours, 2^k +- 1 — and
//      over a seeded million radius words at a seeded angle word each.  Reports the smallest nonzero |t| and |r t| seen.
//   R  rowfix, former form against new: every float d of [-86, 1] (as lw with e = 0, where d = lw), and the dead cases (NaN,
//      +-inf, e == kRowEmpty, d > 1) over a spread of anchors.
//   M  the wave maximum: a 64-lane host model of the DPP scan under the integer maximum against the sequential select chain,
//      active-lane counts 1 .. 64 (the other lanes hold -inf, as the kernels pass it), over seeded bit patterns, ties, all
//      -inf, NaNs in any lane, +0 with negatives.  Sets that hold both +0 and -0 are outside the domain: counted apart.
//   c  0.0f + lp == lp over the NormalExactCuts density fma(d d, -0.5, -L) for seeded d and the literal log-normalisers of
//      sigma = 0.3, 0.5, 1, 2.
// Two NaNs compare equal whatever their payloads.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../oracle/gjx_oracle_math.h"

static inline uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline bool same(float a, float b) { return (a != a && b != b) || f2u(a) == f2u(b); }
static inline uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static long long g_bad = 0;
static void report(const char* what, uint32_t a, uint32_t b, uint32_t got, uint32_t want) {
#pragma omp critical
  {
    if (g_bad++ < 8) std::printf("  MISMATCH %s: inputs %08x %08x -> %08x, former %08x\n", what, a, b, got, want);
  }
}

// --- a: the transform in parts (o_bm_pair's steps; z_cos = r * t_cos, z_sin = r * t_sin)
static inline float bm_radius(uint32_t w_radius) {
  const float u = ((float)w_radius + 1.0f) * 2.3283064365386963e-10f;
  const uint32_t t = f2u(u) - 0x3f3504f3u;
  const o_bm_ent lg = o_bm_lg[(t >> 17) & 63u];
  const float m = u2f((t & 0x007fffffu) + 0x3f3504f3u);
  const float fe = (float)((int32_t)t >> 23);
  const float q = fmaf(m, u2f(lg.a), -1.0f);
  float p = fmaf(q, -0.25f, 0.333333343f);
  p = fmaf(p, q, -0.5f);
  const float l1 = fmaf(p, q * q, q);
  const float lu = fmaf(fe, 0.693147182f, u2f(lg.b)) + l1;
  return sqrtf(-2.0f * lu);
}
static inline void bm_angle(uint32_t w_angle, float& t_cos, float& t_sin) {
  const o_bm_ent cs = o_bm_cs[w_angle >> 24];
  const float d = fmaf((float)((w_angle >> 8) & 0xffffu), 3.74507035e-07f, -0.0122718466f);
  const float d2 = d * d;
  const float sd = fmaf(d2 * d, -0.166666672f, d);
  const float cd = fmaf(d2, fmaf(d2, 0.0416666679f, -0.5f), 1.0f);
  const float ca = u2f(cs.a), sa = u2f(cs.b);
  t_cos = fmaf(ca, cd, -(sa * sd));
  t_sin = fmaf(sa, cd, ca * sd);
}
struct MinSeen {
  float t = INFINITY, rt = INFINITY;
  void see(float r, float t_) {
    const float at = std::fabs(t_), art = std::fabs(r * t_);
    if (at != 0.0f && at < t) t = at;
    if (art != 0.0f && art < rt) rt = art;
  }
  void merge(const MinSeen& o) { t = o.t < t ? o.t : t; rt = o.rt < rt ? o.rt : rt; }
};
static inline long long check_a(float r, float t, uint32_t wr, uint32_t wa, MinSeen& ms) {
  ms.see(r, t);
  const float former = 0.0f + 1.0f * (r * t), cut = fmaf(r, t, 0.0f);
  if (same(former, cut) && f2u(cut) != 0x80000000u) return 0;  // (and never -0: what the identity reference relies on)
  report("a", wr, wa, f2u(cut), f2u(former));
  return 1;
}

// --- R: rowfix (gjx_device.hpp, the device path; m_exp_core restated)
static const int32_t kRowEmpty = -(1 << 30);
static inline float exp_core_y(float x, int32_t& n) {
  const float fx = rintf(x * 1.44269504088896341f);
  x = fmaf(fx, -0.693359375f, x);
  x = fmaf(fx, 2.12194440e-4f, x);
  const float z = x * x;
  float p = 1.9875691500E-4f;
  p = fmaf(p, x, 1.3981999507E-3f);
  p = fmaf(p, x, 8.3334519073E-3f);
  p = fmaf(p, x, 4.1665795894E-2f);
  p = fmaf(p, x, 1.6666665459E-1f);
  p = fmaf(p, x, 5.0000001201E-1f);
  n = (int32_t)fx;
  return fmaf(p, z, x) + 1.0f;
}
static inline float anchored(float lw, int32_t e) {
  const float fe = (float)e;
  const float d = fmaf(-fe, 0.693359375f, lw);
  return fmaf(-fe, -2.12194440e-4f, d);
}
static inline uint32_t rowfix_former(float lw, int32_t e) {
  float d = anchored(lw, e);
  d = d > 1.0f ? 1.0f : d;
  const bool live = e != kRowEmpty && lw > -INFINITY && d >= -86.0f;
  int32_t n;
  const float y = exp_core_y(live ? d : 0.0f, n);
  const uint32_t q = (uint32_t)rintf(u2f(f2u(y) + ((uint32_t)n << 23)) * 1073741824.0f);
  return live ? q : 0u;
}
static inline float min_f32(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }  // (v_min_f32 / fminf: the number)
static inline uint32_t rowfix_cut(float lw, int32_t e) {
  float d = anchored(lw, e);
  d = min_f32(d, 1.0f);
  const bool live = e != kRowEmpty && lw > -INFINITY && d >= -86.0f;
  int32_t n;
  const float y = exp_core_y(live ? d : 0.0f, n);
  const uint32_t q = (uint32_t)rintf(u2f(f2u(y) + ((uint32_t)(n + 30) << 23)));
  return live ? q : 0u;
}

// --- M: the wave maximum
static inline int32_t order_key(uint32_t b) { return (int32_t)(b ^ ((uint32_t)((int32_t)b >> 31) & 0x7fffffffu)); }
static inline float scrub(float v) { return v == v ? v : -INFINITY; }
// the select chain of the specification: a sequential x > m ? x : m over the lanes, NaNs skipped
static inline float max_chain(const float* v) {
  float m = -INFINITY;
  for (int l = 0; l < 64; ++l) { const float x = scrub(v[l]); m = x > m ? x : m; }
  return m;
}
// gjx_device.hpp GJX_WAVE_SCAN_BODY under op = integer maximum, identity INT32_MIN; the result is lane 63's
static inline int32_t imax(int32_t a, int32_t b) { return b > a ? b : a; }
static inline float max_ordered_model(const float* v) {
  const int32_t id = INT32_MIN;
  int32_t x[64], r[64], t[64];
  for (int l = 0; l < 64; ++l) x[l] = order_key(f2u(scrub(v[l])));
  auto shr = [&](const int32_t* src, int l, int k) { return (l & 15) >= k ? src[l - k] : id; };  // row_shr:k inside a row of 16
  for (int l = 0; l < 64; ++l) r[l] = imax(x[l], shr(x, l, 1));
  for (int l = 0; l < 64; ++l) r[l] = imax(r[l], shr(x, l, 2));
  for (int l = 0; l < 64; ++l) r[l] = imax(r[l], shr(x, l, 3));
  for (int l = 0; l < 64; ++l) t[l] = ((l & 15) >> 2) >= 1 ? imax(r[l], shr(r, l, 4)) : r[l];  // bank mask 0xe
  for (int l = 0; l < 64; ++l) r[l] = ((l & 15) >> 2) >= 2 ? imax(t[l], shr(t, l, 8)) : t[l];  // bank mask 0xc
  for (int l = 0; l < 64; ++l) t[l] = ((l >> 4) & 1) ? imax(r[l], r[(l & ~15) - 1]) : r[l];    // row_bcast:15, row mask 0xa
  for (int l = 0; l < 64; ++l) r[l] = (l >> 5) ? imax(t[l], t[31]) : t[l];                     // row_bcast:31, row mask 0xc
  return u2f((uint32_t)order_key((uint32_t)r[63]));
}

int main() {
  {  // a
    const uint32_t edges[] = {0u, 1u, 2u, 0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFF80u, 0xFFFFFF7Fu, 0xFFFFFF00u, 0xFFFFFF01u, 0xFFFFFEFFu, 0xFFFFFE80u, 0xFFFFFE7Fu};
    uint32_t radii[12 + 3 * 32];
    int n_radii = 0;
    for (uint32_t e : edges) radii[n_radii++] = e;
    for (int k = 2; k < 32; ++k) { radii[n_radii++] = (1u << k) - 1u; radii[n_radii++] = 1u << k; radii[n_radii++] = (1u << k) + 1u; }
    long long bad = 0, cases = 0;
    MinSeen ms;
    float r_min = INFINITY;
    float rs[12 + 3 * 32];
    for (int i = 0; i < n_radii; ++i) {
      rs[i] = bm_radius(radii[i]);
      if (rs[i] != 0.0f && rs[i] < r_min) r_min = rs[i];
    }
#pragma omp parallel
    {
      MinSeen mine;
      long long b = 0;
#pragma omp for schedule(static) nowait
      for (int64_t a = 0; a < (int64_t)1 << 24; ++a) {
        float tc, ts;
        bm_angle((uint32_t)a << 8, tc, ts);
        for (int i = 0; i < n_radii; ++i)
          b += check_a(rs[i], tc, radii[i], (uint32_t)a << 8, mine) + check_a(rs[i], ts, radii[i], (uint32_t)a << 8, mine);
      }
#pragma omp critical
      { ms.merge(mine); bad += b; }
    }
    cases = (long long)n_radii * ((long long)2 << 24);
    std::printf("a edge radii: %d radius words x 2^24 angle words x 2 outputs = %lld cases, %lld mismatches\n", n_radii, cases, bad);
    long long bad2 = 0;
#pragma omp parallel
    {
      MinSeen mine;
      long long b = 0;
      float rm = INFINITY;
#pragma omp for schedule(static) nowait
      for (int64_t c = 0; c < 1000000; ++c) {
        uint64_t s = 0xA0ull * 1000003ull + (uint64_t)c;
        const uint64_t w = splitmix(s);
        const float r = bm_radius((uint32_t)w);
        if (r != 0.0f && r < rm) rm = r;
        float tc, ts;
        bm_angle((uint32_t)(w >> 32), tc, ts);
        b += check_a(r, tc, (uint32_t)w, (uint32_t)(w >> 32), mine) + check_a(r, ts, (uint32_t)w, (uint32_t)(w >> 32), mine);
      }
#pragma omp critical
      { ms.merge(mine); bad2 += b; r_min = rm < r_min ? rm : r_min; }
    }
    std::printf("a seeded: 1000000 word pairs x 2 outputs, %lld mismatches\n", bad2);
    std::printf("a smallest nonzero: r %.9g, |t| %.9g, |r t| %.9g (2^-126 = %.9g)\n", r_min, ms.t, ms.rt, 1.17549435e-38);
  }

  {  // R
    long long bad = 0, cases = 0;
    const uint32_t neg_lo = f2u(-86.0f), pos_hi = f2u(1.0f);
    // d = lw at e = 0: the negative floats -0 .. -86 and the positive ones +0 .. 1
#pragma omp parallel for reduction(+ : bad, cases) schedule(static)
    for (int64_t b = 0x80000000ll; b <= (int64_t)neg_lo; ++b) {
      const float lw = u2f((uint32_t)b);
      ++cases;
      if (rowfix_former(lw, 0) != rowfix_cut(lw, 0)) { ++bad; report("R", (uint32_t)b, 0, rowfix_cut(lw, 0), rowfix_former(lw, 0)); }
    }
#pragma omp parallel for reduction(+ : bad, cases) schedule(static)
    for (int64_t b = 0; b <= (int64_t)pos_hi; ++b) {
      const float lw = u2f((uint32_t)b);
      ++cases;
      if (rowfix_former(lw, 0) != rowfix_cut(lw, 0)) { ++bad; report("R", (uint32_t)b, 0, rowfix_cut(lw, 0), rowfix_former(lw, 0)); }
    }
    std::printf("R rowfix, every d of [-86, 1]: %lld floats, %lld mismatches\n", cases, bad);
    // the dead cases and the clamp, over a spread of anchors; and seeded (lw, e) pairs around their anchors
    const uint32_t dead_bits[] = {0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x7f800000u, 0xff800000u, 0x3f800001u /* > 1 */, 0x40000000u, 0x42c80000u,
                                  0x7f7fffffu, 0xff7fffffu, 0xc2ac0001u /* just below -86 */, 0xc2ac0000u, 0xc2abffffu, 0x00000000u, 0x80000000u};
    const int32_t anchors[] = {kRowEmpty, 0, 1, -1, 5, -5, 127, -127, 1000, -1000, 16777216, -16777216};
    long long bad2 = 0, cases2 = 0;
    for (int32_t e : anchors)
      for (uint32_t b : dead_bits) {
        const float lw = u2f(b);
        ++cases2;
        if (rowfix_former(lw, e) != rowfix_cut(lw, e)) { ++bad2; report("R dead", b, (uint32_t)e, rowfix_cut(lw, e), rowfix_former(lw, e)); }
      }
#pragma omp parallel for reduction(+ : bad2, cases2) schedule(static)
    for (int64_t c = 0; c < (int64_t)1 << 24; ++c) {
      uint64_t s = 0x0Full * 1000003ull + (uint64_t)c;
      const uint64_t r = splitmix(s), r2 = splitmix(s);
      const int32_t e = (r2 & 15u) == 0 ? kRowEmpty : (int32_t)(r2 >> 40) % 2000 - 1000;
      // lw near the anchor's own range (e ln 2 - 90 .. e ln 2 + 3), or any bit pattern
      const float lw = (r2 & 16u) ? u2f((uint32_t)r) : (float)e * 0.693147182f + (-90.0f + 93.0f * (float)((r >> 8) & 0xffffffu) * 5.9604644775390625e-08f);
      ++cases2;
      if (rowfix_former(lw, e) != rowfix_cut(lw, e)) { ++bad2; report("R seeded", f2u(lw), (uint32_t)e, rowfix_cut(lw, e), rowfix_former(lw, e)); }
    }
    std::printf("R rowfix, dead cases and seeded (lw, e): %lld cases, %lld mismatches\n", cases2, bad2);
  }

  {  // M
    long long bad = 0, cases = 0, outside = 0;
#pragma omp parallel for reduction(+ : bad, cases, outside) schedule(dynamic, 64)
    for (int64_t c = 0; c < 64 * 4096; ++c) {
      const int active = (int)(c & 63) + 1, kind = (int)((c >> 6) & 7);
      uint64_t s = 0x3Aull * 1000003ull + (uint64_t)c;
      float v[64];
      for (int l = 0; l < 64; ++l) {
        const uint64_t r = splitmix(s);
        float x;
        switch (kind) {
          case 0: x = u2f((uint32_t)r); break;                                                  // any bit pattern (NaNs, infinities, both zeros)
          case 1: x = -(float)(r & 7u); x = x == 0.0f ? 0.0f : x; break;                         // ties; +0 with negatives
          case 2: x = -INFINITY; break;                                                         // all -inf
          case 3: x = (r & 3u) == 0 ? u2f(0x7fc00000u | (uint32_t)(r >> 40)) : -100.0f + (float)(r >> 40) * 1e-5f; break;  // NaNs in any lane
          case 4: x = (float)((int32_t)(r & 15u) - 8) * 0.25f; x = x == 0.0f ? 0.0f : x; break;  // small values of both signs around +0, tied
          case 5: x = -1e3f + (float)(r >> 40) * 1e-4f; break;                                  // log-weights
          case 6: x = (r & 1u) ? -0.0f : -(float)(r & 6u); break;                               // -0 with negatives (no +0 ... unless r & 6 == 0)
          default: x = u2f(((uint32_t)r & 0x807fffffu) | 0x3f800000u); break;                   // one binade, both signs
        }
        if (kind == 6 && x == 0.0f) x = -0.0f;
        v[l] = l < active ? x : -INFINITY;  // (the lanes past the population pass -inf)
      }
      if (kind == 6 && ((c >> 9) & 1)) v[0] = 0.0f;  // ... and a +0 next to them: outside the domain wherever a -0 is active
      bool pz = false, nz = false;
      for (int l = 0; l < 64; ++l) { pz = pz || f2u(v[l]) == 0u; nz = nz || f2u(v[l]) == 0x80000000u; }
      if (pz && nz) { ++outside; continue; }
      ++cases;
      const float got = max_ordered_model(v), want = max_chain(v);
      if (f2u(got) != f2u(want)) { ++bad; report("M", (uint32_t)active, (uint32_t)kind, f2u(got), f2u(want)); }
    }
    std::printf("M ordered maximum: %lld lane sets (1 .. 64 active lanes), %lld mismatches (%lld sets hold both zeros: outside the domain)\n", cases, bad, outside);
  }

  {  // c
    const float sigmas[] = {0.3f, 0.5f, 1.0f, 2.0f};
    long long bad = 0, cases = 0;
    for (float sg : sigmas) {
      const float L = 0.91893853320467f + o_log(sg);  // normal_lognorm
      if (L == 0.0f) { std::printf("  c: sigma %g has a zero log-normaliser\n", sg); ++g_bad; }
#pragma omp parallel for reduction(+ : bad, cases) schedule(static)
      for (int64_t c = 0; c < (int64_t)1 << 24; ++c) {
        uint64_t s = 0xC0ull * 1000003ull + (uint64_t)c;
        const uint64_t r = splitmix(s);
        const float d = (r & 1u) ? u2f((uint32_t)(r >> 32)) : ((float)(int32_t)(r >> 32)) * 4.65661287e-9f;  // any bit pattern, or [-10, 10]
        const float lp = fmaf(d * d, -0.5f, -L);
        ++cases;
        if (!same(0.0f + lp, lp) || f2u(lp) == 0x80000000u) { ++bad; report("c", f2u(d), f2u(L), f2u(lp), f2u(0.0f + lp)); }
      }
    }
    std::printf("c first accumulation: %lld densities, %lld mismatches\n", cases, bad);
  }

  std::printf("%s: %lld mismatches in all\n", g_bad ? "FAILED" : "ok", g_bad);
  return g_bad ? 1 : 0;
}
