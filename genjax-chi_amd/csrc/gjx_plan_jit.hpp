// gjx_plan_jit.hpp — plan specialisation: one straight-line gfx950 kernel per site table.
//
// The interpreter kernel (k_importance) pays ~200 scalar instructions and ~28 scalar loads per
// site to decode the table (rocprofv3 PMC, profiles/r01_b_*).  A static model's table is known when
// the plan is created, so we emit the walk of static.py:340-399 as straight-line HIP — the same
// device functions from gjx_device.hpp in the same order, with every constant folded into a literal
// — and compile it for gfx950 with hiprtc.  Both kernels implement the one arithmetic spec and are
// bit-identical (tests/test_gpu_parity_abi.py runs each plan both ways).
//
// This is included by gjx_hip.hip inside its anonymous namespace users; it needs CSite / gjx_plan.
#pragma once
#include <hip/hiprtc.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <mutex>
#include <sstream>
#include <string>
#include <unordered_map>
#include <cstring>
#include <utility>
#include <vector>

#include <dirent.h>
#include <dlfcn.h>
#include <spawn.h>
#include <sys/wait.h>
#include <unistd.h>
#include <cerrno>

extern "C" char** environ;

namespace gjx_jit {

// The device header, embedded at build time (see __graft_entry__.build()).
static const char kDeviceHeader[] =
#include "gjx_device_embed.inc"
    ;

inline std::string flit(float f) {
  char b[64];
  // (a NaN / infinite literal is kept out of constant propagation: gjx_device.hpp opq)
  std::snprintf(b, sizeof b, (f - f == 0.0f) ? "u2f(0x%08xu)" : "opq(u2f(0x%08xu))", gjx::f2u(f));
  return b;
}
// a finite literal that must still stay opaque (a parameter outside its domain, an observation outside the support)
inline std::string flit_opaque(float f) { return (f - f == 0.0f) ? "opq(" + flit(f) + ")" : flit(f); }
// Device pointers of a generated kernel: entry k of the `tabs` kernel argument (gjx_device.hpp PlanTables), numbered in
// order of first use while the source is generated — the SOURCE holds indices, never addresses, so it is the same for
// every plan of the same structure; the plan keeps the addresses and passes them at launch.  (Beyond kMaxPlanTables
// distinct tables — 48: never seen — the address is written into the source as before.)
struct TableReg {
  std::vector<const void*> ptrs;
  int index_of(const void* p) {
    for (size_t i = 0; i < ptrs.size(); ++i)
      if (ptrs[i] == p) return (int)i;
    if ((int)ptrs.size() >= gjx::kMaxPlanTables) return -1;
    ptrs.push_back(p);
    return (int)ptrs.size() - 1;
  }
  gjx::PlanTables tables() const {
    gjx::PlanTables t;
    std::memset(&t, 0, sizeof t);
    for (size_t i = 0; i < ptrs.size(); ++i) t.p[i] = ptrs[i];
    return t;
  }
};
inline TableReg*& active_tables() {
  static thread_local TableReg* reg = nullptr;
  return reg;
}
struct TableScope {  // the registry of one source generation
  TableReg reg;
  TableReg* prev;
  TableScope() : prev(active_tables()) { active_tables() = &reg; }
  ~TableScope() { active_tables() = prev; }
};
inline std::string plit_as(const char* type, const void* p) {
  char b[96];
  const int k = active_tables() ? active_tables()->index_of(p) : -1;
  if (k >= 0) std::snprintf(b, sizeof b, "((const %s*)tabs.p[%d])", type, k);
  else std::snprintf(b, sizeof b, "((const %s*)0x%llxull)", type, (unsigned long long)(uintptr_t)p);
  return b;
}
inline std::string plit(const void* p) { return plit_as("float", p); }

// Emits the walk of one site table as straight-line HIP, in exactly the interpreter's operation
// order.  mode 0 = importance (particle index `i`, particle key `pkey`, input columns, score and
// output columns); mode 1 = SMC step / init (slot `j`, `a.step_key`, ancestor state `st_k`,
// observation constants `a.obs[]`, weight only).  `sfx` is appended to every per-particle name, so two
// emitters ("A", "B") can interleave the walks of the two particles a lane owns.
// Nested `@gen` calls (gjx.h gjx_scope): which key every site draws under and with which fold.  Derived once per plan
// from the scopes' ranges: every `@` site and every call takes the next counter of the scope it sits in (THREEFRY: the
// 1-based counter over all of them; PHILOX: the 0-based index among those that consume randomness — unobserved sites and
// calls), a callee numbers its own sites afresh under fold_in(caller's key, the call's counter).
// gjx_site.observed (include/gjx.h: 0 latent, 1 observed; include/gjx_guided.h: 2 proposed, 3 guided): does the site
// consume randomness?  Latent and proposed sites do — same draw numbering, same quad blocks.
inline bool sampled_mode(int observed) { return observed == 0 || observed == GJX_SITE_PROPOSED; }
struct ScopeInfo {
  int n_scopes = 0;
  int site_scope[GJX_MAX_SITES];
  uint32_t fold_t[GJX_MAX_SITES], fold_p[GJX_MAX_SITES];
  int parent[GJX_MAX_SCOPES + 1], begin[GJX_MAX_SCOPES + 1], end[GJX_MAX_SCOPES + 1];
  uint32_t s_fold_t[GJX_MAX_SCOPES + 1], s_fold_p[GJX_MAX_SCOPES + 1];
};
inline bool derive_scopes(const gjx_site* sites, int n_sites, const gjx_scope* sc, int n_sc, ScopeInfo& out) {
  if (n_sc < 0 || n_sc > GJX_MAX_SCOPES || (n_sc && !sc)) return false;
  struct Frame { int id, end; uint32_t ct, dr; };
  Frame fr[8];
  int depth = 0, next = 0;
  fr[depth++] = Frame{0, n_sites, 1u, 0u};
  out.n_scopes = n_sc;
  out.parent[0] = -1;
  for (int q = 0; q <= n_sites; ++q) {
    while (next < n_sc && sc[next].begin == q) {  // the calls made at this position, in call order
      const gjx_scope& k = sc[next];
      if (k.parent < 0 || k.parent > next || k.end < k.begin || k.end > n_sites) return false;
      while (depth > 0 && fr[depth - 1].id != k.parent) {
        if (fr[depth - 1].end > q) return false;  // the caller is not the innermost open scope
        --depth;
      }
      if (depth == 0 || k.end > fr[depth - 1].end || depth >= 5) return false;
      out.parent[next + 1] = k.parent;
      out.begin[next + 1] = k.begin;
      out.end[next + 1] = k.end;
      out.s_fold_t[next + 1] = fr[depth - 1].ct++;
      out.s_fold_p[next + 1] = fr[depth - 1].dr++;
      fr[depth++] = Frame{next + 1, k.end, 1u, 0u};
      ++next;
    }
    if (next < n_sc && sc[next].begin < q) return false;  // not in call order
    while (depth > 1 && fr[depth - 1].end <= q) --depth;
    if (q == n_sites) break;
    out.site_scope[q] = fr[depth - 1].id;
    out.fold_t[q] = fr[depth - 1].ct++;
    out.fold_p[q] = fr[depth - 1].dr;
    if (sampled_mode(sites[q].observed)) fr[depth - 1].dr++;
  }
  return next == n_sc;
}

template <class CSiteT, class CArgT>
struct SiteEmitter {
  std::ostringstream& o;
  int impl, mode;
  const CSiteT* sites;
  int n_sites;
  const char* ind;
  std::string sfx = "";
  int cur_blk = -1;
  bool store_values = true;  // false: the caller stores (the paired kernel writes both particles at once)
  bool ext_bits = false;     // true: the caller defines bits<q><sfx> of one-word draws (SMC quads share a block)
  bool exact_cuts = true;    // false: Normal log-densities keep the three-operation form everywhere (normal_exact_cuts)
  bool row_cuts = false;     // true (the pair / quad importance and scan kernels): the exact zero-add cuts below, each only where
                             // its conditions hold.  Off everywhere else — the tempered plans' sources are pinned byte for byte
  const ScopeInfo* sc = nullptr;  // nested calls: per-site key scope and fold (null: a flat body, the implicit numbering)
  // (a) A latent Normal site of the lane's own scope whose location is the literal +0.0f (not -0.0f: the add of -0 is the
  // identity and folds by itself) and whose scale is the literal 1.0f: its value 0.0f + 1.0f * z is the transform's output
  // itself under the PlusZero overload of bm_pair (gjx_device.hpp), which fuses the add into its last product.
  bool zero_loc_unit(int q) const {
    const CSiteT& st = sites[q];
    return row_cuts && pairs_normals() && st.dist == GJX_DIST_NORMAL && st.observed == 0 && scope_of(q) == 0 && !retained(q) &&
           st.a0.kind == GJX_ARG_CONST && gjx::f2u(st.a0.offset) == 0u && st.a1.kind == GJX_ARG_CONST && st.a1.offset == 1.0f;
  }
  // (b) A reference to such a site with literal scale 1.0f and offset +0.0f is the value itself: 1.0f * v folds, and v + 0.0f
  // is v unless v is -0 — which a value produced by an fma (or an addition) with +0 never is.
  bool identity_ref(const CArgT& a) const {
    return a.kind == GJX_ARG_SITE && a.scale == 1.0f && gjx::f2u(a.offset) == 0u && a.ref_site >= 0 && a.ref_site < n_sites &&
           zero_loc_unit(a.ref_site);
  }
  // include/gjx_csmc.h (the conditional kernels only): ret_comp[q] >= 0 — sampled site q is carry component ret_comp[q]; its
  // draw is made as ever (named vd<q> / vj<q>) and its VALUE is `rsel<sfx> ? rv_<k> : the draw`: a select in front of every
  // log-density that reads it.  null: the source of the unconditional kernels, byte for byte.
  const int* ret_comp = nullptr;
  bool retained(int q) const { return ret_comp && ret_comp[q] >= 0 && sampled(sites[q]); }

  int scope_of(int q) const { return sc ? sc->site_scope[q] : 0; }
  std::string key_of_scope(int k) const { return k == 0 ? "pkey" + sfx : "skey" + std::to_string(k) + sfx; }
  std::string key_of(int q) const { return key_of_scope(scope_of(q)); }
  // the keys of the nested scopes, each fold_in(caller's key, the counter its call took); after pkey<sfx> is defined
  void emit_scope_keys() {
    if (!sc) return;
    for (int k = 1; k <= sc->n_scopes; ++k)
      o << ind << "const Key " << key_of_scope(k) << " = fold_in<" << impl << ">(" << key_of_scope(sc->parent[k]) << ", "
        << (impl == 0 ? sc->s_fold_t[k] : sc->s_fold_p[k]) << "u); (void)" << key_of_scope(k) << ";\n";
    for (int k = 1; k <= sc->n_scopes; ++k) o << ind << "float " << acc("w", k) << " = 0.0f, " << acc("sc", k) << " = 0.0f;\n";
  }

  static bool is_int(const CSiteT& s) { return s.dist >= GJX_DIST_BERNOULLI; }
  // include/gjx_counts.h: Poisson / NegativeBinomial (tempered plans made by gjx_temper_plan_create_counts only)
  static bool is_count(const CSiteT& s) { return s.dist == GJX_DIST_POISSON || s.dist == GJX_DIST_NEGATIVE_BINOMIAL; }
  static bool sampled(const CSiteT& s) { return sampled_mode(s.observed); }  // consumes randomness (latent or proposed)
  static bool proposed(const CSiteT& s) { return s.observed == GJX_SITE_PROPOSED; }
  static bool guided(const CSiteT& s) { return s.observed == GJX_SITE_GUIDED; }
  std::string nm(const char* base, int q) const { return std::string(base) + std::to_string(q) + sfx; }
  std::string val_f32(int site) const { return is_int(sites[site]) ? "(float)" + nm("vi", site) : nm("vf", site); }
  std::string val_i32(int site) const {
    return is_int(sites[site]) ? nm("vi", site) : "(int32_t)__builtin_rintf(" + nm("vf", site) + ")";
  }
  std::string arg(const CArgT& a) const {
    switch (a.kind) {
      case GJX_ARG_CONST: return flit(a.offset);
      case GJX_ARG_SITE:
        if (identity_ref(a)) return nm("vf", a.ref_site);
        return "((" + flit(a.scale) + " * " + val_f32(a.ref_site) + ") + " + flit(a.offset) + ")";
      case GJX_ARG_INPUT:
        return "((" + flit(a.scale) + " * cols.in[" + std::to_string(a.ref) + "][li" + sfx + "]) + " + flit(a.offset) + ")";
      case GJX_ARG_STATE: return "((" + flit(a.scale) + " * st_" + std::to_string(a.ref) + sfx + ") + " + flit(a.offset) + ")";
      case GJX_ARG_OBS: return "((" + flit(a.scale) + " * a.obs[" + std::to_string(a.ref) + "]) + " + flit(a.offset) + ")";
      // (include/gjx_plate.h: column `ref` at the row of the plated loop — dc<ref> is the row's value, defined by GenTemper)
      // (with the emitter's suffix: GenPredictive holds two rows per lane, dc<ref>A and dc<ref>B)
      case GJX_ARG_DATA: return "((" + flit(a.scale) + " * dc" + std::to_string(a.ref) + sfx + ") + " + flit(a.offset) + ")";
      // (include/gjx_group.h: grouped site `ref` at the group of the row — gz_<ref> is the current group's value, an argument
      // of the device functions GenTemperGrouped emits)
      case GJX_ARG_GROUP: return "((" + flit(a.scale) + " * gz_" + std::to_string(a.ref) + sfx + ") + " + flit(a.offset) + ")";
      case GJX_ARG_PARAM:
        // (an SMC plan's parameter as it stands is the row's value itself: no multiply by 1, no add of 0 — a uniform value
        // stays in its scalar register — and what gjx_smc_plan_set_params derives the site's constants from)
        if (mode == 1 && a.scale == 1.0f && a.offset == 0.0f) return "prm.p[" + std::to_string(a.ref) + "]";
        return "((" + flit(a.scale) + " * prm.p[" + std::to_string(a.ref) + "]) + " + flit(a.offset) + ")";
      case GJX_ARG_EXPR: {
        // the postfix program as ONE parenthesised f32 expression: every operator rounds once, in program order (the
        // translation unit is compiled with -ffp-contract=off: no fusion, no re-association)
        const gjx_expr_op* ops = reinterpret_cast<const gjx_expr_op*>(a.table);
        std::vector<std::string> st;
        for (int k = 0; k < a.ref; ++k) {
          const std::string r = std::to_string(ops[k].ref);
          switch (ops[k].op) {
            case GJX_EXPR_CONST: st.push_back(flit(ops[k].value)); break;
            case GJX_EXPR_SITE: st.push_back(val_f32(ops[k].ref)); break;
            case GJX_EXPR_INPUT: st.push_back("cols.in[" + r + "][li" + sfx + "]"); break;
            case GJX_EXPR_PARAM: st.push_back("prm.p[" + r + "]"); break;
            case GJX_EXPR_STATE: st.push_back("st_" + r + sfx); break;
            case GJX_EXPR_OBS: st.push_back("a.obs[" + r + "]"); break;
            case GJX_EXPR_DATA: st.push_back("dc" + r + sfx); break;
            case GJX_EXPR_GROUP: st.push_back("gz_" + r + sfx); break;
            case GJX_EXPR_NEG: st.back() = "(-" + st.back() + ")"; break;
            case GJX_EXPR_EXP: st.back() = "e_exp(" + st.back() + ")"; break;
            case GJX_EXPR_LOG: st.back() = "m_log(" + st.back() + ")"; break;
            case GJX_EXPR_SQRT: st.back() = "__builtin_sqrtf(" + st.back() + ")"; break;
            case GJX_EXPR_ABS: st.back() = "__builtin_fabsf(" + st.back() + ")"; break;
            case GJX_EXPR_LT: case GJX_EXPR_LE: case GJX_EXPR_EQ: {
              const std::string b = st.back();
              st.pop_back();
              const char* op = ops[k].op == GJX_EXPR_LT ? " < " : (ops[k].op == GJX_EXPR_LE ? " <= " : " == ");
              st.back() = "((" + st.back() + op + b + ") ? 1.0f : 0.0f)";
              break;
            }
            case GJX_EXPR_SELECT: {
              const std::string f = st.back();
              st.pop_back();
              const std::string t = st.back();
              st.pop_back();
              st.back() = "((" + st.back() + " != 0.0f) ? " + t + " : " + f + ")";
              break;
            }
            case GJX_EXPR_MAX: case GJX_EXPR_MIN: {
              const std::string b = st.back();
              st.pop_back();
              st.back() = std::string(ops[k].op == GJX_EXPR_MAX ? "e_max(" : "e_min(") + st.back() + ", " + b + ")";
              break;
            }
            default: {
              const std::string b = st.back();
              st.pop_back();
              const char* op = ops[k].op == GJX_EXPR_ADD ? " + " : (ops[k].op == GJX_EXPR_SUB ? " - " : (ops[k].op == GJX_EXPR_MUL ? " * " : " / "));
              st.back() = "(" + st.back() + op + b + ")";
            }
          }
        }
        return st.back();
      }
      default: return plit(a.table) + "[" + val_i32(a.ref_site) + "]";
    }
  }
  // does any site draw (and so need the per-particle key)?
  bool needs_pk() const {
    for (int q = 0; q < n_sites; ++q)
      if (sampled(sites[q])) return true;
    return false;
  }
  bool needs_stream_key() const {
    for (int q = 0; q < n_sites; ++q)
      if (sampled(sites[q]) && !one_word(sites[q])) return true;
    return false;
  }
  // fold of site q: THREEFRY the 1-based site counter; PHILOX the 0-based index among the sampled sites
  uint32_t fold_of(int q) const {
    if (sc) return impl == 0 ? sc->fold_t[q] : sc->fold_p[q];
    if (impl == 0) return (uint32_t)(q + 1);
    uint32_t d = 0;
    for (int p = 0; p < q; ++p) d += sampled(sites[p]) ? 1u : 0u;
    return d;
  }
  bool one_word(const CSiteT& st) const {
    return st.dist == GJX_DIST_NORMAL || st.dist == GJX_DIST_BERNOULLI ||
           (st.dist == GJX_DIST_CATEGORICAL && st.cat_mode == 1);
  }
  // Importance plans under PHILOX pair particles at Normal sites (gjx_device.hpp bm_pair / site_normal);
  // SMC steps keep the single-draw inverse-CDF form (one latent per slot-step: a pair would cost two blocks).
  // Scan steps (mode 2) are importance walks under the step's chained key: same draws as mode 0.
  bool pairs_normals() const { return impl == 1 && mode != 1; }
  // does the postfix program of `a` (a GJX_ARG_EXPR argument) read nothing but literals?
  static bool literal_program(const CArgT& a) {
    const gjx_expr_op* ops = reinterpret_cast<const gjx_expr_op*>(a.table);
    for (int k = 0; k < a.ref; ++k)
      if ((ops[k].op >= GJX_EXPR_SITE && ops[k].op <= GJX_EXPR_OBS) || ops[k].op == GJX_EXPR_DATA || ops[k].op == GJX_EXPR_GROUP) return false;
    return true;
  }

  // Part 1 of site q: arguments, the observed value, or the draw word(s).
  void head(int q) {
    const CSiteT& st = sites[q];
    const std::string Q = std::to_string(q) + sfx;
    const uint32_t fold = fold_of(q);
    o << ind << "// site " << q << sfx << " dist " << st.dist << (guided(st) ? " guided" : proposed(st) ? " proposed" : st.observed ? " observed" : " latent") << "\n";
    if (st.dist == GJX_DIST_CATEGORICAL) {
      std::string rr;
      if (st.a0.kind == GJX_ARG_SITE) rr = val_i32(st.a0.ref_site);
      else if (st.a0.kind == GJX_ARG_CONST) rr = "(int32_t)__builtin_rintf(" + flit(st.a0.offset) + ")";
      else rr = "(int32_t)__builtin_rintf(" + arg(st.a0) + ")";
      o << ind << "int32_t rr" << Q << " = " << rr << "; rr" << Q << " = rr" << Q << " < 0 ? 0 : (rr" << Q
        << " >= " << st.n_rows << " ? " << st.n_rows - 1 << " : rr" << Q << ");\n";
      o << ind << "const float* row" << Q << " = " << plit(st.logits) << " + (size_t)rr" << Q << " * " << st.n_cat << ";\n";
    } else {
      // a CONSTANT argument outside its domain (scale / rate / concentration <= 0, a probability outside [0, 1]) or an
      // observed constant outside the support would fold into a NaN / +inf constant log-density: kept opaque (opq)
      auto carg = [&](const CArgT& a, int which) {
        float v = a.offset;
        if (a.kind == GJX_ARG_EXPR) {  // a program over literals only is a constant too: its value, by the program's own steps
          if (!literal_program(a)) return arg(a);  // (not a constant)
          const gjx_expr_op* ops = reinterpret_cast<const gjx_expr_op*>(a.table);
          float stk[8];
          int d = 0;
          for (int k = 0; k < a.ref; ++k) {
            if (ops[k].op == GJX_EXPR_CONST) { stk[d++] = ops[k].value; continue; }
            if (ops[k].op == GJX_EXPR_NEG) { stk[d - 1] = -stk[d - 1]; continue; }
            if (ops[k].op == GJX_EXPR_EXP) { stk[d - 1] = gjx::e_exp(stk[d - 1]); continue; }
            if (ops[k].op == GJX_EXPR_LOG) { stk[d - 1] = gjx::m_log(stk[d - 1]); continue; }
            if (ops[k].op == GJX_EXPR_SQRT) { stk[d - 1] = __builtin_sqrtf(stk[d - 1]); continue; }
            if (ops[k].op == GJX_EXPR_ABS) { stk[d - 1] = __builtin_fabsf(stk[d - 1]); continue; }
            if (ops[k].op == GJX_EXPR_SELECT) { const float r = stk[d - 3] != 0.0f ? stk[d - 2] : stk[d - 1]; d -= 2; stk[d - 1] = r; continue; }
            if (ops[k].op == GJX_EXPR_LT || ops[k].op == GJX_EXPR_LE || ops[k].op == GJX_EXPR_EQ) {
              const float y = stk[--d], x = stk[d - 1];
              stk[d - 1] = (ops[k].op == GJX_EXPR_LT ? x < y : (ops[k].op == GJX_EXPR_LE ? x <= y : x == y)) ? 1.0f : 0.0f;
              continue;
            }
            const float y = stk[--d], x = stk[d - 1];
            stk[d - 1] = ops[k].op == GJX_EXPR_ADD ? x + y : ops[k].op == GJX_EXPR_SUB ? x - y : ops[k].op == GJX_EXPR_MUL ? x * y
                         : ops[k].op == GJX_EXPR_MAX ? gjx::e_max(x, y) : ops[k].op == GJX_EXPR_MIN ? gjx::e_min(x, y) : x / y;
          }
          v = stk[0];
        } else if (a.kind != GJX_ARG_CONST) {
          return arg(a);
        }
        bool ok = v - v == 0.0f;
        if (st.dist == GJX_DIST_NORMAL) ok = ok && (which == 0 || v > 0.0f);
        else if (st.dist == GJX_DIST_BERNOULLI) ok = ok && v >= 0.0f && v <= 1.0f;
        else if (st.dist == GJX_DIST_POISSON) ok = ok && v >= 0.0f;
        else if (st.dist == GJX_DIST_NEGATIVE_BINOMIAL && which == 1) ok = ok && v >= 0.0f && v < 1.0f;
        else ok = ok && v > 0.0f;
        if (a.kind == GJX_ARG_EXPR) return ok ? arg(a) : "opq(" + arg(a) + ")";
        return ok ? flit(v) : flit_opaque(v);
      };
      o << ind << "const float a0_" << Q << " = " << carg(st.a0, 0) << ";\n";
      if (st.dist != GJX_DIST_BERNOULLI && st.dist != GJX_DIST_POISSON) o << ind << "const float a1_" << Q << " = " << carg(st.a1, 1) << ";\n";
    }
    if (guided(st)) {  // the value its partner (an earlier proposed site) drew
      if (is_int(st)) o << ind << "const int32_t vi" << Q << " = " << val_i32(st.obs.ref_site) << ";\n";
      else o << ind << "const float vf" << Q << " = " << val_f32(st.obs.ref_site) << ";\n";
      return;
    }
    if (st.observed == 1) {
      std::string ov;
      if (st.obs.kind == GJX_ARG_CONST) {
        const float v = st.obs.offset;
        const bool in_support = st.dist == GJX_DIST_GAMMA ? v > 0.0f : (st.dist == GJX_DIST_BETA ? (v > 0.0f && v < 1.0f) : (is_count(st) ? v >= 0.0f : true));
        ov = in_support ? flit(v) : flit_opaque(v);
      }
      else if (st.obs.kind == GJX_ARG_OBS) ov = "a.obs[" + std::to_string(st.obs.ref) + "]";
      else if (st.obs.kind == GJX_ARG_NEXT) ov = "nx_" + std::to_string(st.obs.ref);  // (transition tables: gjx_backsim.h)
      else if (st.obs.kind == GJX_ARG_PARAM || st.obs.kind == GJX_ARG_DATA || st.obs.kind == GJX_ARG_EXPR) ov = arg(st.obs);  // (DATA, EXPR: a plated site's)
      else if (st.obs.kind == GJX_ARG_GROUP) ov = "gz_" + std::to_string(st.obs.ref) + sfx;  // (a grouped site's own value: TemperTable)
      else ov = "cols.in[" + std::to_string(st.obs.ref) + "][li" + sfx + "]";
      // (a count keeps its float too: the support test k >= 0 of gjx_counts.h is taken before any conversion to an integer)
      if (is_count(st)) o << ind << "const float vk" << Q << " = __builtin_rintf(" << ov << ");\n" << ind << "const int32_t vi" << Q << " = (int32_t)vk" << Q << ";\n";
      else if (is_int(st)) o << ind << "const int32_t vi" << Q << " = (int32_t)__builtin_rintf(" << ov << ");\n";
      else o << ind << "const float vf" << Q << " = " << ov << ";\n";
      return;
    }
    if (!one_word(st) || (ext_bits && scope_of(q) == 0)) return;  // (a callee's sites draw under their own lone keys)
    if (impl == 1) {  // (the generic form: kernels that own whole pairs / quads define bits themselves, ext_bits)
      o << ind << "const uint32_t bits" << Q << " = philox_single_draw(" << key_of(q) << ", " << fold << "u);\n";
    } else {
      o << ind << "const uint32_t bits" << Q << " = Stream<0>(" << key_of(q) << ", true, " << fold << "u).bits32(0);\n";
    }
  }

  // A Beta site with a literal shape that is not below 1: beta_from_gammas (gjx_device.hpp) is its first line, the bare ratio; the
  // source says so and the log-space branch is not compiled in.
  static bool beta_plain_ratio(const CSiteT& st) {
    return (st.a0.kind == GJX_ARG_CONST && !(st.a0.offset < 1.0f)) || (st.a1.kind == GJX_ARG_CONST && !(st.a1.offset < 1.0f));
  }

  // Part 2 of site q: the sampled value (Normal sites take their standard normal from `eps`: an expression
  // or, empty, this particle's own derivation), the log-density, the accumulators and the stored column.
  bool presampled = false;  // tail(): a Gamma / Beta site's value vf<q> has been defined by the caller
  bool defer_acc = false;   // tail(): only the sampled value; the caller accumulates lp_of(q)
  void tail(int q, const std::string& eps = "") {
    const CSiteT& st = sites[q];
    const std::string I = std::to_string(impl), Q = std::to_string(q) + sfx, K = key_of(q);
    const uint32_t fold = fold_of(q);
    const std::string row = "row" + Q;
    const bool isint = is_int(st);
    const std::string VF = (retained(q) ? "vd" : "vf") + Q, VI = (retained(q) ? "vj" : "vi") + Q;  // what the draw defines
    // (presampled: the pair / quad forms draw the gammas of a lane's particles together — std_gamma_multi — and define vf<q> themselves)
    if (sampled(st) && !(presampled && (st.dist == GJX_DIST_GAMMA || st.dist == GJX_DIST_BETA))) {
      switch (st.dist) {
        case GJX_DIST_NORMAL: {
          std::string e = eps;
          if (zero_loc_unit(q)) {  // (the caller drew eps through bm_pair's PlusZero overload: the value itself)
            o << ind << "const float " << VF << " = " << e << ";\n";
            break;
          }
          if (e.empty())
            e = pairs_normals() ? "site_normal<1>(Stream<1>(" + K + ", true, " + std::to_string(fold) + "u))"
                                : "std_normal(bits" + Q + ")";
          o << ind << "const float t" << Q << " = a1_" << Q << " * " << e << ";\n";
          o << ind << "const float " << VF << " = a0_" << Q << " + t" << Q << ";\n";
          break;
        }
        case GJX_DIST_BERNOULLI:
          o << ind << "const int32_t " << VI << " = uniform01(bits" << Q << ") < a0_" << Q << " ? 1 : 0;\n";
          break;
        case GJX_DIST_GAMMA:
          o << ind << "const Stream<" << I << "> strm" << Q << "(" << K << ", true, " << fold << "u);\n";
          o << ind << "const float " << VF << " = std_gamma<" << I << ">(strm" << Q << ", 0, a0_" << Q << ") / a1_" << Q << ";\n";
          break;
        case GJX_DIST_BETA:
          o << ind << "const Stream<" << I << "> strm" << Q << "(" << K << ", true, " << fold << "u);\n";
          o << ind << "const float g1_" << Q << " = std_gamma<" << I << ">(strm" << Q << ", 0, a0_" << Q << ");\n";
          o << ind << "const float g2_" << Q << " = std_gamma<" << I << ">(strm" << Q << ", 1, a1_" << Q << ");\n";
          if (beta_plain_ratio(st))
            o << ind << "const float " << VF << " = g1_" << Q << " / (g1_" << Q << " + g2_" << Q << ");\n";
          else
            o << ind << "const float " << VF << " = beta_from_gammas<" << I << ">(strm" << Q << ", a0_" << Q << ", a1_" << Q << ", g1_" << Q << ", g2_" << Q << ");\n";
          break;
        case GJX_DIST_POISSON:  // (gjx_device.hpp poisson_draw / negative_binomial_draw: the one-particle form under both ciphers)
          o << ind << "const Stream<" << I << "> strm" << Q << "(" << K << ", true, " << fold << "u);\n";
          o << ind << "const int32_t " << VI << " = poisson_draw<" << I << ">(strm" << Q << ", 0u, a0_" << Q << ");\n";
          break;
        case GJX_DIST_NEGATIVE_BINOMIAL:
          o << ind << "const Stream<" << I << "> strm" << Q << "(" << K << ", true, " << fold << "u);\n";
          o << ind << "const int32_t " << VI << " = negative_binomial_draw<" << I << ">(strm" << Q << ", a0_" << Q << ", a1_" << Q << ");\n";
          break;
        default:
          if (st.cat_mode == 0) {
            o << ind << "const Stream<" << I << "> strm" << Q << "(" << K << ", true, " << fold << "u);\n";
            o << ind << "const int32_t " << VI << " = jcat_gumbel<" << I << ">(" << row << ", " << st.n_cat << "u, strm" << Q << ");\n";
          } else if (st.cat_ent) {  // the row's prepared {CDF, log-probability} entries, entered at the guide of the draw's
                                    // top byte (same integers as the two-pass walk: the same category); the entry the walk
                                    // ends on carries the log-density
            o << ind << "uint32_t lpb" << Q << ";\n";
            o << ind << "const int32_t " << VI << " = jcat_invcdf_gb(" << plit_as("uint4", st.cat_guide4) << " + ((size_t)rr" << Q << " << " << st.cat_gbits << "), "
              << plit_as("uint2", st.cat_ent) << " + (size_t)rr" << Q << " * " << st.n_cat << ", " << st.n_cat << "u, bits" << Q << ", " << (32 - st.cat_gbits) << ", lpb" << Q << ");\n";
          } else {
            o << ind << "const int32_t " << VI << " = jcat_invcdf(" << row << ", " << st.n_cat << "u, bits" << Q << ");\n";
          }
      }
      if (retained(q)) {  // (the state column's f32 value, converted as val_i32 converts one)
        const std::string rv = "rv_" + std::to_string(ret_comp[q]);
        // (clamped to +-2^30 first, a NaN to -2^30: the conversion is defined for every f32, and whatever is not a
        // category of the site is outside its support — log-density -inf — as for an observed value)
        if (isint) o << ind << "const int32_t vi" << Q << " = rsel" << sfx << " ? (int32_t)__builtin_rintf(__builtin_fminf(__builtin_fmaxf(" << rv << ", -1073741824.0f), 1073741824.0f)) : " << VI << ";\n";
        else o << ind << "const float vf" << Q << " = rsel" << sfx << " ? " << rv << " : " << VF << ";\n";
      }
    }
    if (defer_acc) return;  // (the caller adds lp_of(q) to the accumulators itself: emit_pair_lane_sites)
    const std::string lp = lp_of(q);
    const std::string v = (isint ? "vi" : "vf") + Q;
    const std::string aw = acc("w", scope_of(q)), as = acc("sc", scope_of(q));
    if (proposed(st)) {  // q's log-density enters nothing here: its guided partner adds lp - lq at ITS position
      o << ind << "const float lq" << Q << " = " << lp << ";\n";
    } else if (guided(st)) {  // the difference first (a proposal equal to the model's site cancels exactly), then the sum
      o << ind << "{ const float lp = " << lp << "; " << as << " = " << as << " + lp; const float d = lp - " << nm("lq", st.obs.ref_site)
        << "; " << aw << " = " << aw << " + d; }\n";
    } else {
      o << ind << "{ const float lp = " << lp << "; " << as << " = " << as << " + lp;"
        << (st.observed ? " " + aw + " = " + aw + " + lp;" : "") << " }\n";
    }
    if ((mode == 0 || mode == 2) && st.out_col >= 0 && store_values)
      o << ind << "reinterpret_cast<uint32_t*>(cols.out[" << st.out_col << "])[" << (mode == 2 ? "oi" : "i") << sfx << "] = "
        << (isint ? "(uint32_t)" + v : "f2u(" + v + ")") << ";\n";
  }
  // A Normal site whose hoisted constants are literals of the source, the reciprocal scale a power of two 2^k with k >= 0 and
  // the log-normaliser of magnitude >= 2^-100: its log-density is the fused overload of logpdf_normal_pre (gjx_device.hpp
  // NormalExactCuts: two operations fewer, the same bits).  Both conditions or neither: a site is emitted in one of two forms.
  // Constants derived from launch parameters (pre == 2) and scales read at run time keep the three-operation form, and so do
  // the tempered plans (GenTemper, GenPointwise: tests/test_pointwise_cpu.py pins their generated move sources byte for byte).
  bool normal_exact_cuts(const CSiteT& st) const {
    if (!exact_cuts || st.dist != GJX_DIST_NORMAL || st.pre != 1) return false;
    const uint32_t rs = gjx::f2u(st.pre0);
    const bool pow2 = (rs & 0x807fffffu) == 0u && rs >= 0x3f800000u && rs < 0x7f800000u;  // positive, no mantissa bits, 2^0 .. 2^127
    return pow2 && st.pre1 - st.pre1 == 0.0f && __builtin_fabsf(st.pre1) >= 7.8886090522101181e-31f;  // finite, >= 2^-100
  }
  // the log-density of site q at its value, as an expression over the names head() and tail() have defined
  std::string lp_of(int q) const {
    const CSiteT& st = sites[q];
    const std::string Q = std::to_string(q) + sfx;
    const std::string row = "row" + Q;
    const bool isint = is_int(st);
    std::string lp;
    const std::string v = (isint ? "vi" : "vf") + Q;
    // hoisted per-site constants: literals (pre == 1) or derived from the launch's parameters (pre == 2)
    const std::string p0 = st.pre == 2 ? "prm.d[" + std::to_string(2 * q) + "]" : flit(st.pre0);
    const std::string p1 = st.pre == 2 ? "prm.d[" + std::to_string(2 * q + 1) + "]" : flit(st.pre1);
    switch (st.dist) {
      case GJX_DIST_NORMAL:
        lp = st.pre ? "logpdf_normal_pre(" + v + ", a0_" + Q + ", " + p0 + ", " + p1 + (normal_exact_cuts(st) ? ", NormalExactCuts())" : ")")
                    : "logpdf_normal(" + v + ", a0_" + Q + ", a1_" + Q + ")";
        break;
      case GJX_DIST_GAMMA:
        lp = st.pre ? "logpdf_gamma_pre(" + v + ", a0_" + Q + ", a1_" + Q + ", " + p1 + ")"
                    : "logpdf_gamma(" + v + ", a0_" + Q + ", a1_" + Q + ")";
        break;
      case GJX_DIST_BETA:
        lp = st.pre ? "logpdf_beta_pre(" + v + ", a0_" + Q + ", a1_" + Q + ", " + p1 + ")"
                    : "logpdf_beta(" + v + ", a0_" + Q + ", a1_" + Q + ")";
        break;
      case GJX_DIST_BERNOULLI: lp = "logpdf_bernoulli(" + v + " != 0, a0_" + Q + ")"; break;
      case GJX_DIST_POISSON:
      case GJX_DIST_NEGATIVE_BINOMIAL: {
        // an observed value: its float vk<q> (head()); a plated one reads log k! from the data column after its own (dc<c + 1>:
        // gjx_counts.h), a scalar one and a draw evaluate m_lgamma(k + 1)
        const std::string fn = st.dist == GJX_DIST_POISSON ? "logpdf_poisson" : "logpdf_negative_binomial";
        const std::string as = ", a0_" + Q + (st.dist == GJX_DIST_POISSON ? std::string() : ", a1_" + Q);
        if (st.observed && st.obs.kind == GJX_ARG_DATA) lp = fn + "_lf(vk" + Q + as + ", dc" + std::to_string(st.obs.ref + 1) + sfx + ")";
        else lp = fn + "(" + (st.observed ? "vk" + Q : "(float)" + v) + as + ")";
        break;
      }
      default:
        const bool lpb_drawn = st.cat_ent && sampled(st) && st.cat_mode != 0;
        if (lpb_drawn && !retained(q))
          lp = "u2f(lpb" + Q + ")";  // a drawn category is in range
        else
          lp = std::string(lpb_drawn ? "(!rsel" + sfx + " ? u2f(lpb" + Q + ") : " : "") + "((" + v + " < 0 || " + v + " >= " + std::to_string(st.n_cat) + ") ? -__builtin_inff() : " +
               (st.cat_logp_t ? plit(st.cat_logp_t) + "[(size_t)" + v + " * " + std::to_string(st.n_rows) + " + rr" + Q + "]"
                : st.cat_ent ? "u2f(" + plit_as("uint2", st.cat_ent) + "[(size_t)rr" + Q + " * " + std::to_string(st.n_cat) + " + " + v + "].y)"
                             : row + "[" + v + "] - jrow_lse(" + row + ", " + std::to_string(st.n_cat) + "u)") + ")" + (lpb_drawn ? ")" : "");
    }
    // an observed site whose arguments and value are ALL compile-time constants has a compile-time log-density: opaque, so
    // that no overflow of valid constants (-inf, +inf) becomes a constant log-weight either
    auto is_const = [](const CArgT& a) {  // a literal, or a program over literals only
      return a.kind == GJX_ARG_CONST || (a.kind == GJX_ARG_EXPR && literal_program(a));
    };
    const bool all_const = st.observed == 1 && st.obs.kind == GJX_ARG_CONST && is_const(st.a0) &&
                           (st.dist == GJX_DIST_BERNOULLI || st.dist == GJX_DIST_CATEGORICAL || is_const(st.a1));
    if (all_const) lp = "opq(" + lp + ")";
    return lp;
  }

  // a callee's weight and score are ITS totals, added to the caller's when the call returns (static.py:374-380: the
  // caller adds `w`; StaticTrace.get_score sums the sub-traces' scores): one accumulator pair per scope
  std::string acc(const char* base, int k) const { return k == 0 ? std::string(base) + sfx : std::string(base) + "_s" + std::to_string(k) + sfx; }
  void close_scopes(int pos) {  // the calls that have returned once the sites before `pos` are done (inner ones first)
    if (!sc) return;
    for (int k = sc->n_scopes; k >= 1; --k)
      if (sc->end[k] == pos && sc->begin[k] < pos)
        o << ind << acc("w", sc->parent[k]) << " = " << acc("w", sc->parent[k]) << " + " << acc("w", k) << "; "
          << acc("sc", sc->parent[k]) << " = " << acc("sc", sc->parent[k]) << " + " << acc("sc", k) << ";\n";
  }
  void run() {
    emit_scope_keys();
    for (int q = 0; q < n_sites; ++q) {
      head(q);
      tail(q);
      close_scopes(q + 1);
    }
  }
};

// bm_lds: the kernels of this source stage the Box-Muller tables in LDS (each calls bm_stage() at entry; gjx_device.hpp),
// `block` threads per workgroup (a constant of the source: bm_stage forms its table addresses from it).  What the sites call
// by name — jrow_lse, jcat_invcdf, jcat_invcdf_gb, jcat_gumbel ... — is in the device header, like every other fixed function.
inline void emit_prelude(std::ostringstream& o, bool fast_math = false, bool bm_lds = false, int block = 0) {
  if (bm_lds) o << "#define GJX_BM_LDS 1\n#define GJX_BM_BLOCK " << block << "\n";
  if (fast_math) o << "#define GJX_FAST_MATH 1\n";  // gjx.h GJX_PLAN_FAST_MATH: hardware transcendentals (gjx_device.hpp d_exp / bm_pair)
  o << "#include \"gjx_device.hpp\"\nusing namespace gjx;\n";
}
// PHILOX Normal sites draw through the Box-Muller tables: the importance and scan kernels of such a source stage them in LDS
// (gjx_device.hpp bm_stage)
template <class CSiteT>
inline bool bm_lds(int impl, bool fast_math, const CSiteT* sites, int n_sites) {
  if (impl != 1 || fast_math) return false;
  for (int q = 0; q < n_sites; ++q)
    if (!sites[q].observed && sites[q].dist == GJX_DIST_NORMAL) return true;
  return false;
}

// The 2 or 4 particles a lane owns (suffixes A, B [, C, D]): one SiteEmitter each, and the lists a generated source spells out
// particle by particle.  The lane owns whole pairs / quads, so the single-word draws of its own scope come from cipher blocks
// the group shares (ext_bits); whatever else differs from an emitter's defaults is set through each(), once for all particles.
template <class CSiteT, class CArgT>
struct LaneGroup {
  using Emitter = SiteEmitter<CSiteT, CArgT>;
  static constexpr const char* kSfx[4] = {"A", "B", "C", "D"};
  std::vector<Emitter> em;
  LaneGroup(std::ostringstream& o, int P, int impl, int mode, const CSiteT* sites, int n_sites, const char* ind) {
    for (int u = 0; u < P; ++u) { em.push_back(Emitter{o, impl, mode, sites, n_sites, ind, kSfx[u]}); em.back().ext_bits = true; }
  }
  int size() const { return (int)em.size(); }
  // f(u, the emitter of particle u), in particle order
  template <class F> void each(F f) { for (int u = 0; u < size(); ++u) f(u, em[u]); }
  // expr(the emitter of a particle) -> a string; those of all particles, comma-separated
  template <class F> std::string join(F expr) const {
    std::string t;
    for (int u = 0; u < size(); ++u) t += (u ? ", " : "") + std::string(expr(em[u]));
    return t;
  }
  std::string list(const std::string& pre, const std::string& post = "") const {  // pre<suffix>post of every particle
    return join([&](const Emitter& e) { return pre + e.sfx + post; });
  }
};

// The row sums of a kernel without the fused fold are read by a later launch: plain stores (lse_store_row's last argument).
inline const char* tail_scope(bool fused_tail) { return fused_tail ? "tail.tickets != nullptr" : "false"; }
// The closing braces of the row loop and of the kernel and, in the fused-tail variant, the in-launch fold of the row sums
// between them (gjx_device.hpp lse_tail).  `ticket`: the workgroup's ticket and the count of all tickets, as lse_tail takes them.
inline void emit_kernel_close(std::ostringstream& o, bool fused_tail, const char* ticket) {
  o << "  }\n";
  if (fused_tail) o << "  if (row_e) lse_tail(row_e, row_s, (n + 255) / 256, tail, " << ticket << ");\n";
  o << "}\n";
}
// The end of a row and of the kernel where a lane owns ONE particle (the importance and scan kernels of that form): the row's
// maximum and its row-anchored sum by four waves through LDS (block_max / block_sum over `tmax`, -inf in a lane that is not
// `live`), written by thread 0 at index `row`.  The forms in which a lane owns 2 or 4 particles reduce by waves and keep their
// own statistics (Gen::run_paired, GenScan::run_quad): nothing but the close is common to them — they differ in the
// reduction, the writer lane, the known outputs and, between the two quad forms, in how the lane's maximum is taken, which
// the compiler turns into different machine code.
inline void emit_row_epilogue_per_lane(std::ostringstream& o, const char* row, bool fused_tail, const char* ticket) {
  o << "    if (max_partials || row_e) {\n";
  o << "      const float bm = block_max(tmax, sh_red);\n";
  o << "      if (max_partials && threadIdx.x == 0) max_partials[" << row << "] = bm;\n";
  o << "      if (row_e) {\n";
  o << "        const int32_t eb = row_anchor(bm);\n";
  o << "        const uint64_t sb = block_sum(live ? rowfix(tmax, eb) : 0, sh_sum);\n";
  o << "        if (threadIdx.x == 0) lse_store_row(row_e, row_s, " << row << ", eb, sb, " << tail_scope(fused_tail) << ");\n";
  o << "      }\n    }\n";
  emit_kernel_close(o, fused_tail, ticket);
}

// The sites of a lane that owns NP whole PAIRS of adjacent particles (suffixes A, B [, C, D]) under PHILOX: one cipher
// block per pair and two draws (pk0 / pk1: the cipher key; pair0 [, pair1]: the pairs' counter words — defined by the
// caller), one Box-Muller transform per pair and Normal site, every stored column one vector store at `store_at`.
// The quad kernels store write-through (sc1) when a launch holds ONE pass (store16_out, gjx_device.hpp): the kernel's end
// no longer waits for the write-back of its 48 MB — 4.94e10 -> 5.47e10 particles/s at one pass per launch; a batch
// of the benchmark's size takes the write-through store with the non-temporal hint as well, and several passes
// that stay in the caches plain stores (ImportanceVariant::stores_of has the measurements), hence the source
// variants (ImportanceVariant::stores: `wt_one_pass` is a constant of the generated source; `store_kind` is what a store
// line passes for it — the non-temporal kinds add a second constant, `nt_stores`).
template <class CSiteT, class CArgT>
inline void emit_pair_lane_sites(std::ostringstream& o, LaneGroup<CSiteT, CArgT>& lanes, const std::string& ind, const std::string& store_at,
                                 const std::string& sc_guard = "", const std::string& ubase = "", const std::string& lane_bytes = "",
                                 bool sc_known = false, const bool* skip = nullptr, const std::string& store_kind = "wt_one_pass") {
  auto& em = lanes.em;
  const auto& sfx = lanes.kSfx;
  const CSiteT* sites = em[0].sites;
  const int n_sites = em[0].n_sites, P = lanes.size(), NP = P / 2;
  int cur_pair_blk = -1;
  // `sc_known` (ImportanceVariant::full_outputs): the launch stores the scores — no question is asked at the sites
  const std::string if_sc = sc_known ? "" : "if (" + sc_guard + ") ";
  // (c) The first contribution to the lane's weights (and to its scores) initialises them where it is a NormalExactCuts
  // density: that is fma(d d, -0.5, -L) with L a nonzero literal, never -0, so 0.0f + lp is lp (gjx_device.hpp first_acc).
  // Any other first contribution is added to the +0 the accumulators are declared with.  Flat bodies only: a callee's totals
  // reach the caller's accumulators through close_scopes.
  bool w_open = false, sc_open = false;
  for (int q = 0; q < n_sites; ++q) {
    if (skip && skip[q]) continue;  // (GenPredictive: a site the caller has emitted itself — nothing is drawn or summed at it)
    const CSiteT& st = sites[q];
    // `sc_guard` (the importance kernels: the name of the score pointer): the lane's weights and scores are brought up to
    // date AT the site, pair by pair (gjx_device.hpp pinned2), the scores only where the launch stores them — so w and sc
    // are the only values that live from one site to the next.  (A callee's sites keep the plain per-particle form.)
    const bool pinned = !sc_guard.empty() && em[0].scope_of(q) == 0;
    for (int u = 0; u < P; ++u) em[u].defer_acc = pinned;
    for (int u = 0; u < P; ++u) em[u].head(q);
    const std::string Q = std::to_string(q);
    if (!st.observed && em[0].one_word(st) && em[0].scope_of(q) == 0) {  // (a callee's sites: every particle's own lone key)
      // draw f of a pair: block f >> 1 holds words (even, odd particle) of draw 2 (f >> 1) and of draw 2 (f >> 1) + 1
      const uint32_t f = em[0].fold_of(q);
      const int blk = (int)(f >> 1);
      const std::string B = std::to_string(blk);
      if (blk != cur_pair_blk) {
        cur_pair_blk = blk;
        for (int pi = 0; pi < NP; ++pi) {
          const std::string V = "pp" + std::to_string(pi) + "_" + B;
          o << ind << "uint32_t " << V << "_0, " << V << "_1, " << V << "_2, " << V << "_3;\n";
          o << ind << "philox4x32(pk0, pk1, (uint32_t)pair" << pi << ", (uint32_t)(pair" << pi << " >> 32), " << blk << "u, kTagPair, " << V
            << "_0, " << V << "_1, " << V << "_2, " << V << "_3);\n";
        }
      }
      for (int pi = 0; pi < NP; ++pi) {
        const std::string V = "pp" + std::to_string(pi) + "_" + B;
        o << ind << "const uint32_t bits" << Q << sfx[2 * pi] << " = " << V << "_" << ((f & 1u) << 1) << ", bits" << Q << sfx[2 * pi + 1]
          << " = " << V << "_" << (((f & 1u) << 1) | 1u) << ";\n";
      }
    }
    if (!st.observed && st.dist == GJX_DIST_NORMAL && em[0].scope_of(q) == 0) {
      for (int pi = 0; pi < NP; ++pi) {
        const std::string Z = Q + "_" + std::to_string(pi);
        o << ind << "float zc" << Z << ", zs" << Z << ";\n      bm_pair(bits" << Q << sfx[2 * pi] << ", bits" << Q << sfx[2 * pi + 1] << ", zc" << Z
          << ", zs" << Z << (em[0].zero_loc_unit(q) ? ", PlusZero());\n" : ");\n");
      }
      for (int pi = 0; pi < NP; ++pi) {
        const std::string Z = Q + "_" + std::to_string(pi);
        em[2 * pi].tail(q, "zc" + Z);
        em[2 * pi + 1].tail(q, "zs" + Z);
      }
    } else if (!st.observed && (st.dist == GJX_DIST_GAMMA || st.dist == GJX_DIST_BETA)) {
      // the lane's P particles draw their gammas TOGETHER (gjx_device.hpp std_gamma_multi: the first attempts straight-line,
      // the retries in one shared loop): the same values as P std_gamma calls, fewer divergent wave-trips
      const std::string I = std::to_string(em[0].impl), PS = std::to_string(P);
      const uint32_t fold = em[0].fold_of(q);
      o << ind << "float vg0_" << Q << "[" << PS << "]" << (st.dist == GJX_DIST_BETA ? ", vg1_" + Q + "[" + PS + "]" : std::string()) << ";\n";
      o << ind << "{\n" << ind << "  const Stream<" << I << "> gs[" << PS << "] = {"
        << lanes.join([&](const auto& e) { return "Stream<" + I + ">(" + e.key_of(q) + ", true, " + std::to_string(fold) + "u)"; }) << "};\n";
      o << ind << "  const float gc0[" << PS << "] = {" << lanes.list("a0_" + Q) << "};\n"
        << ind << "  std_gamma_multi<" << I << ", " << PS << ">(gs, 0, gc0, vg0_" << Q << ");\n";
      if (st.dist == GJX_DIST_BETA)
        o << ind << "  const float gc1[" << PS << "] = {" << lanes.list("a1_" + Q) << "};\n"
          << ind << "  std_gamma_multi<" << I << ", " << PS << ">(gs, 1, gc1, vg1_" << Q << ");\n";
      o << ind << "}\n";
      for (int u = 0; u < P; ++u) {
        if (st.dist == GJX_DIST_GAMMA)
          o << ind << "const float vf" << Q << sfx[u] << " = vg0_" << Q << "[" << u << "] / a1_" << Q << sfx[u] << ";\n";
        else if (em[0].beta_plain_ratio(st))
          o << ind << "const float vf" << Q << sfx[u] << " = vg0_" << Q << "[" << u << "] / (vg0_" << Q << "[" << u << "] + vg1_" << Q << "[" << u << "]);\n";
        else
          o << ind << "const float vf" << Q << sfx[u] << " = beta_from_gammas<" << I << ">(Stream<" << I << ">(" << em[u].key_of(q) << ", true, " << fold
            << "u), a0_" << Q << sfx[u] << ", a1_" << Q << sfx[u] << ", vg0_" << Q << "[" << u << "], vg1_" << Q << "[" << u << "]);\n";
        em[u].presampled = true;
        em[u].tail(q);
        em[u].presampled = false;
      }
    } else {
      for (int u = 0; u < P; ++u) em[u].tail(q);
    }
    if (pinned) {
      auto pins = [&](const char* base) {
        std::string t;
        for (int pi = 0; pi < NP; ++pi) {
          const std::string a = std::string(base) + sfx[2 * pi], b = std::string(base) + sfx[2 * pi + 1];
          t += " { const pin2_t t = pinned2(" + a + ", " + b + "); " + a + " = t[0]; " + b + " = t[1]; }";
        }
        return t;
      };
      const bool never_neg_zero = em[0].row_cuts && !em[0].sc && st.observed <= 1 && em[0].normal_exact_cuts(st);
      auto acc_to = [&](const char* base, bool first, int u, const std::string& lp) {
        const std::string a = std::string(base) + sfx[u];
        return first ? a + " = first_acc(" + lp + "); " : a + " = " + a + " + " + lp + "; ";
      };
      if (st.observed) {  // the log-density enters the weight (always needed) and the score
        for (int u = 0; u < P; ++u) o << ind << "const float lp" << Q << sfx[u] << " = " << em[u].lp_of(q) << ";\n";
        o << ind;
        for (int u = 0; u < P; ++u) o << acc_to("w", !w_open && never_neg_zero, u, "lp" + Q + sfx[u]);
        o << pins("w") << "\n";
        o << ind << if_sc << "{ ";
        for (int u = 0; u < P; ++u) o << acc_to("sc", !sc_open && never_neg_zero, u, "lp" + Q + sfx[u]);
        o << pins("sc") << " }\n";
        w_open = true;
      } else {  // a latent site's log-density is part of the score alone
        o << ind << if_sc << "{\n";
        for (int u = 0; u < P; ++u)
          o << ind << "  { const float lp = " << em[u].lp_of(q) << "; " << acc_to("sc", !sc_open && never_neg_zero, u, "lp") << "}\n";
        o << ind << " " << pins("sc") << "\n" << ind << "}\n";
      }
      sc_open = true;
      for (int u = 0; u < P; ++u) em[u].defer_acc = false;
    }
    for (int u = 0; u < P; ++u) em[u].close_scopes(q + 1);
    if (st.out_col >= 0) {  // the lane's particles are adjacent in the column: one 8- / 16-byte store per lane
      const bool isint = SiteEmitter<CSiteT, CArgT>::is_int(st);
      const std::string vals = isint ? lanes.list("(uint32_t)vi" + Q) : lanes.list("f2u(vf" + Q, ")");
      if (P == 4 && !ubase.empty())  // (wave-uniform base + the lane's byte offset: gjx_device.hpp store16_at)
        o << ind << "store16_at(reinterpret_cast<uint32_t*>(cols.out[" << st.out_col << "]) + " << ubase << ", " << lane_bytes << ", make_uint4(" << vals << "), " << store_kind << ");\n";
      else if (P == 4)
        o << ind << "store16_out(reinterpret_cast<uint32_t*>(cols.out[" << st.out_col << "]) + " << store_at << ", make_uint4(" << vals << "), " << store_kind << ");\n";
      else
        o << ind << "*reinterpret_cast<uint" << P << "*>(reinterpret_cast<uint32_t*>(cols.out[" << st.out_col << "]) + " << store_at << ") = make_uint" << P
          << "(" << vals << ");\n";
    }
  }
}

// The importance kernel of a plan.  Two forms:
//  * generic: one 256-particle row per 256-thread workgroup, one particle per lane, any key batch;
//  * paired (PHILOX, lazy children of a lane-0 key, even first index): one row per 128-thread workgroup,
//    TWO ADJACENT PARTICLES per lane.  The lane derives both particles' words anyway, so every Normal site
//    costs one shared Box-Muller transform for the pair, and the cipher key (the parent's) is uniform over
//    the launch: the round keys live in scalar registers.
//
// Which of these kernels a source is — the value that travels from a launch (gjx_hip.hip importance_launch) to the generator,
// and the index of the plan's slot for the compiled kernel.
struct ImportanceVariant {
  int impl = 0;            // the generator: 0 THREEFRY, 1 PHILOX
  int lane_particles = 1;  // adjacent particles per lane: 1; 2 = the paired form (128-thread workgroup per 256-particle row);
                           // 4 = two pairs: one WAVE owns the whole row, so the row statistics are wave reductions (DPP only:
                           // no LDS, no barrier) and every column store is 16 bytes per lane.  Above 1 is PHILOX only
  bool fused_tail = false;  // the kernel folds the row sums itself (gjx_device.hpp lse_tail; launches that pass a gjx_lse_out).
                            // A variant of its own: inlined into every kernel, the fold cost 22 VGPRs — one wave per SIMD —
                            // on launches that never enter it (132 -> 110 in the 10-latent quad kernel)
  // The kinds of store: bit 0 write-through (sc1), bit 1 non-temporal (nt) — the two flags gjx_device.hpp store16_at takes.
  enum : int { kStorePlain = 0, kStoreWt = 1, kStoreNt = 2, kStoreNtWt = 3 };
  int stores = kStorePlain;  // the kind of the quad form's 16-byte stores.  A variant of its own: as a run-time flag every store was a
                   // uniform branch pair (88 scalar instructions per row of the 10-latent kernel) and a basic block of its own
  bool full_outputs = false;  // the one-row quad form of a launch that passes score, logw, max_partials, row_e and row_s (and no
                              // gjx_lse_out): all five are known non-null, so the source asks nothing about them — as run-time
                              // questions they were 25 uniform branches and a compare per site in every row of the 10-latent
                              // kernel, and cut the row into some 40 basic blocks.  Every other form ignores the flag

  // Which combinations a launch can take: pairs and quads under PHILOX only; the four kinds of store and the known outputs
  // exist at four particles per lane only, the known outputs not together with the fused tail.
  constexpr bool launched() const {
    return (impl == 0 || impl == 1) && (lane_particles == 1 || ((lane_particles == 2 || lane_particles == 4) && impl == 1)) &&
           stores >= kStorePlain && stores <= kStoreNtWt && (stores == kStorePlain || lane_particles == 4) && (!full_outputs || (lane_particles == 4 && !fused_tail));
  }
  // The variant of a launch.  `allowed`: how many adjacent particles a lane may own given the keys, n and the alignment of
  // the buffers (gjx_hip.hip lane_particles); `form_pref`: GJX_JIT_FORM, the most the caller wants (three become two).
  // `n_pass`, `bytes`: the passes of the launch and what its columns write in all; `stores_pref`: the kind of store an escape
  // forces (GJX_JIT_DEFINE=GJX_STORES_*, gjx_hip.hip jit_stores_pref), -1 for the measured rule.
  static constexpr ImportanceVariant of_launch(int impl, int allowed, int form_pref, bool lse, int n_pass, uint64_t bytes, bool every_output,
                                               int stores_pref = -1) {
    const int most = impl == 1 ? (allowed < form_pref ? allowed : form_pref) : 1, P = most >= 4 ? 4 : (most >= 2 ? 2 : 1);
    return ImportanceVariant{impl, P, lse, P == 4 ? (stores_pref >= 0 ? stores_pref : stores_of(n_pass, bytes)) : (int)kStorePlain, every_output && !lse && P == 4};
  }
  // The kind of store of a quad launch: the measured rule (profiles/stream_store_summary.md; one MI355X, the 10-latent model,
  // 1e6 particles, `python bench.py`, builds and kinds alternating in one job, five runs each).
  //  * ONE pass: write-through — the kernel's end does not wait for the write-back of its 48 MB (4.94e10 -> 5.47e10
  //    particles/s at one pass per launch).
  //  * a batch of the size this was measured at (32 passes of 1e6 particles: 1.54 GB per launch, six times the Infinity
  //    Cache) or larger: write-through AND non-temporal.  Against
  //    the plain stores such a batch took before (parent 1.0072e11 particles/s, range 0.9999 .. 1.0097): write-through
  //    +1.1 %, non-temporal +2.1 %, both +2.9 % (1.0343 .. 1.0504e11, every run above every run of the parent).  The launch
  //    itself is 3 % shorter (0.308 -> 0.299 ms) and nothing is left dirty in the L2s for the boundary behind it.
  //  * smaller batches: plain, as before.  Event-timed indications at 97 - 387 MB per launch favour write-through, not both
  //    hints, and at 960 MB whole runs overlapped the parent's: nothing there went through the five-run protocol, so the
  //    threshold is the measured size, not a crossover.
  static constexpr uint64_t kStreamBytes = 1500000000ull;
  static constexpr int stores_of(int n_pass, uint64_t bytes) { return n_pass <= 1 ? kStoreWt : (bytes >= kStreamBytes ? kStoreNtWt : kStorePlain); }
  // The variant the diagnostics name: `bits` = impl | GJX_SOURCE_*, `form` the particles per lane of a PHILOX source.  Any
  // combination of the flags stands, full outputs with the fused tail too (no launch takes it; the source exists); what a
  // form ignores is dropped: one particle per lane has one kind of store and asks about every output, and so does the pair
  // form, which still says the kind of store in its text (`wt_one_pass`), so that flag stays with it; the non-temporal bit
  // exists at four particles per lane only.
  static ImportanceVariant of_source(int bits, int form) {
    const int impl = bits & ~(GJX_SOURCE_FUSED_TAIL | GJX_SOURCE_WT_STORES | GJX_SOURCE_FULL_OUTPUTS | GJX_SOURCE_NT_STORES), P = impl == 1 ? form : 1;
    return ImportanceVariant{impl, P, (bits & GJX_SOURCE_FUSED_TAIL) != 0,
                             ((bits & GJX_SOURCE_WT_STORES) != 0 && P >= 2 ? kStoreWt : 0) | ((bits & GJX_SOURCE_NT_STORES) != 0 && P == 4 ? kStoreNt : 0),
                             (bits & GJX_SOURCE_FULL_OUTPUTS) != 0 && P == 4};
  }
  // The plan's slot of a variant a launch can take: the six (form, fused tail) pairs below four particles per lane, then the
  // twelve quad variants (guarded, fused tail, every output; four kinds of store each).  Dense: kSlots of them, no two alike
  // (the static_assert below walks them all).
  static constexpr int kSlots = 18;
  constexpr int slot() const {
    if (lane_particles < 4) return 2 * (lane_particles == 2 ? 2 : impl) + (fused_tail ? 1 : 0);
    return 6 + 4 * (full_outputs ? 2 : (fused_tail ? 1 : 0)) + stores;
  }
  const char* kname() const { return impl == 0 ? "gjx_plan_kernel_threefry" : "gjx_plan_kernel_philox"; }
};
constexpr bool importance_slots_distinct() {
  bool seen[ImportanceVariant::kSlots] = {};
  int n = 0;
  for (int k = 0; k < 2 * 3 * 16; ++k) {  // every generator, form, kind of store and flag combination
    const ImportanceVariant v{k & 1, 1 << ((k >> 1) % 3), ((k / 6) & 1) != 0, ((k / 6) >> 2) & 3, ((k / 6) & 2) != 0};
    if (!v.launched()) continue;
    if (v.slot() < 0 || v.slot() >= ImportanceVariant::kSlots || seen[v.slot()]) return false;
    seen[v.slot()] = true, ++n;
  }
  return n == ImportanceVariant::kSlots;
}
static_assert(importance_slots_distinct(), "two importance variants a launch can take share a slot of gjx_plan::jit");

template <class CSiteT, class CArgT>
struct Gen {
  std::ostringstream o;
  ImportanceVariant v;
  const CSiteT* sites;
  int n_sites;
  int min_waves = 0;  // __launch_bounds__ waves-per-SIMD hint (0 = none)
  int block = 256;    // threads per workgroup of the generated kernel
  int rows_per_block = 1;
  bool fast_math = false;  // GJX_PLAN_FAST_MATH
  const ScopeInfo* sc = nullptr;  // nested calls (null: a flat body)

  static const char* signature() {
    return "(KeySrc ks, RunCols cols, float* score, float* logw, uint64_t n, float* max_partials, int32_t* row_e, "
           "uint64_t* row_s, LseTail tail, PassBatch bt, PlanParams prm, PlanTables tabs) {\n";
  }
  // the waves-per-SIMD hint is a macro with the plan's choice as its default (0 = none), so that
  // GJX_JIT_DEFINE=GJX_WAVES_HINT=<k> builds the same kernel under another hint for an A/B (tools/ab_waves_hint.py)
  std::string bounds(int threads) const { return "__launch_bounds__(" + std::to_string(threads) + ", GJX_WAVES_HINT)"; }
  void emit_hint_default() { o << "#ifndef GJX_WAVES_HINT\n#define GJX_WAVES_HINT " << (min_waves > 0 ? min_waves : 0) << "\n#endif\n"; }
  // (one ticket per workgroup of the two-dimensional grid: its linear id, x fastest, and the count of all of them)
  static constexpr const char* kTicket = "blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y";
  // The grid is (rows of a pass / R, passes): a workgroup's pass is blockIdx.y and its first row blockIdx.x — known to the
  // dispatcher, so the kernel divides nothing, and the address of the pass's parent key (bt.parent[pass], in the kernel
  // argument block) is known at the first instruction: its load goes out with the other arguments'.  The loop over x is for
  // rows beyond the grid limit (2^31 - 1 workgroups of 256 particles: dead at any size that fits in memory).
  void emit_pass_key() {
    o << "  const uint32_t pass = blockIdx.y, grid_x = gridDim.x;  // (pass < bt.n_pass <= kMaxPasses: the host launches n_pass rows of workgroups)\n";
    o << "  const uint32_t bk0 = bt.parent[pass][0], bk1 = bt.parent[pass][1];\n";
  }

  std::string run_paired() {
    // NP pairs of adjacent particles per lane; a 256-particle row is 128 / NP lanes.  R rows per workgroup.
    const int NP = v.lane_particles / 2;
    const int lanes_per_row = 128 / NP;
    const bool lds = bm_lds(v.impl, fast_math, sites, n_sites);
    // rows per workgroup: 1 when the walk stores value columns (measured r02); a walk without any (an estimate of the
    // log-marginal alone: row sums out, nothing else) runs 4 one-wave rows per workgroup — 256 lanes fold the row sums in
    // the fused tail in one trip of loads instead of 8 by a single wave (host-API call 52.5 -> 47.6 us at 1e6 particles)
    bool any_col = false;
    for (int q = 0; q < n_sites; ++q) any_col = any_col || sites[q].out_col >= 0;
    const int R = (NP == 2 && !any_col) ? 4 : 1;
    block = lanes_per_row * R;
    rows_per_block = R;
    const int waves_per_row = lanes_per_row / 64;  // 2 (pairs) or 1 (quads)
    // the quad form's stores: one wave-uniform base per column and row (scalar registers) plus ONE per-lane byte offset
    // (gjx_device.hpp store16_at); the four-row workgroup of the estimate-only kernel has no block-uniform row
    const bool ubase = NP == 2 && R == 1;
    const bool full = v.full_outputs && ubase;  // (ImportanceVariant::full_outputs)
    emit_prelude(o, fast_math, lds, block);
    emit_hint_default();
    o << "extern \"C\" __global__ " << bounds(block) << " void " << v.kname() << signature();
    if (waves_per_row > 1) o << "  __shared__ float sh_red[" << waves_per_row * R << "];\n  __shared__ uint64_t sh_sum[" << waves_per_row * R << "];\n";
    if (R == 1) o << "  const int wv = threadIdx.x >> 6, pr = 0, tr = threadIdx.x;  // (block-uniform row: the cipher key stays scalar)\n";
    else o << "  const int wv = threadIdx.x >> 6, pr = threadIdx.x / " << lanes_per_row << ", tr = threadIdx.x % " << lanes_per_row << ";\n";
    o << "  (void)wv;\n";
    // the Box-Muller tables' loads first (they wait for no argument: gjx_device.hpp bm_issue), then the kernel's scalar
    // arguments in ONE round of loads (gjx_device.hpp: resample_args_anchor has the measurement), the pass's parent key among
    // them: one wait for both
    if (lds) o << "  const BmLoads bm_loads = bm_issue();\n";
    emit_pass_key();
    o << "  asm volatile(\"\" :: \"s\"(n), \"s\"(score), \"s\"(logw), \"s\"(max_partials), \"s\"(row_e), \"s\"(row_s), \"s\"(bt.n_pass), \"s\"(bt.rows_per_pass), \"s\"(bt.pass_stride), \"s\"(bt.row_stride), \"s\"(ks.first), \"s\"(ks.parent.k0), \"s\"(ks.parent.k1), \"s\"(bk0), \"s\"(bk1), \"s\"(grid_x)"
      << (v.fused_tail ? ", \"s\"(tail.tickets)" : "") << ");\n";
    {
      bool seen[64] = {};  // ... and the value columns this plan stores (RunCols::out has 64)
      for (int q = 0; q < n_sites; ++q)
        if (sites[q].out_col >= 0 && sites[q].out_col < 64 && !seen[sites[q].out_col]) {
          seen[sites[q].out_col] = true;
          o << "  asm volatile(\"\" :: \"s\"(cols.out[" << sites[q].out_col << "]));\n";
        }
    }
    if (lds) o << "  bm_loads.bm_stage();\n";
    // (the text of the generated comment names the flag as it was called when it was a member of Gen: sources stay as they were)
    o << "  const bool wt_one_pass = " << ((v.stores & ImportanceVariant::kStoreWt) ? "true" : "false") << "; (void)wt_one_pass;  // (Gen::wt_stores)\n";
    // the non-temporal kinds say so in a second constant, passed by every store line (the other sources keep their text)
    const bool nt = (v.stores & ImportanceVariant::kStoreNt) != 0 && NP == 2;
    if (nt) o << "  const bool nt_stores = true; (void)nt_stores;  // (ImportanceVariant::stores)\n";
    const std::string kind = nt ? "wt_one_pass, nt_stores" : "wt_one_pass";
    o << "  const uint32_t pk0 = bt.n_pass > 1 ? bk0 : ks.parent.k0, pk1 = bt.n_pass > 1 ? bk1 : ks.parent.k1;\n";
    o << "  const uint64_t po = (uint64_t)pass * bt.pass_stride, ro = (uint64_t)pass * bt.row_stride;  // this pass's outputs\n";
    o << "  for (uint64_t g0 = (uint64_t)blockIdx.x * " << R << "; g0 < bt.rows_per_pass; g0 += (uint64_t)grid_x * " << R << ") {\n";
    o << "    const uint64_t row = g0 + pr;\n";
    o << "    const bool live_row = row < bt.rows_per_pass;  // (the four-row workgroup: the dead rows at the end of a pass)\n";
    // the row's index in the per-row arrays.  (The one-row quad form makes it opaque per row: folded into the three arrays'
    // bases it is hoisted out of the row loop as an address pair and a stride pair each, and with the cipher's round keys in
    // scalar registers that was more than fit — a pair spilled to VGPR lanes and read back for every row.)
    o << "    uint64_t rrow = ro + row;\n";
    if (NP == 2 && R == 1) o << "    asm volatile(\"\" : \"+s\"(rrow));\n";
    const int P = 2 * NP;  // particles per lane
    LaneGroup<CSiteT, CArgT> lanes(o, P, v.impl, 0, sites, n_sites, "      ");
    lanes.each([&](int, auto& e) { e.store_values = false; e.row_cuts = true; e.sc = sc; });  // (the lane stores its particles at once)
    o << "    const uint64_t iA = row * 256 + " << P << " * (uint64_t)tr;\n";
    lanes.each([&](int u, auto& e) { if (u) o << "    const uint64_t i" << e.sfx << " = iA + " << u << ";\n"; });
    // n is a multiple of P in this form (checked by the host): all particles of a lane exist or none
    o << "    const bool ok = live_row && iA < n;\n";
    // (the lane's offset is made opaque per row: folded into the columns' bases it would be hoisted out of the row loop
    // as one 64-bit address pair per column)
    if (ubase) o << "    const uint64_t ub = po + row * 256;\n    uint32_t lb = 16u * (uint32_t)tr;\n    asm volatile(\"\" : \"+v\"(lb));\n";
    lanes.each([&](int, auto& e) { o << "    const uint64_t li" << e.sfx << " = i" << e.sfx << "; (void)li" << e.sfx << ";\n"; });
    lanes.each([&](int, auto& e) { o << "    float w" << e.sfx << " = 0.0f, sc" << e.sfx << " = 0.0f;\n"; });
    o << "    if (ok) {\n";
    o << "      const uint64_t lnA = ks.first + iA + 1u;\n";
    lanes.each([&](int u, auto& e) {
      if (u) o << "      const uint64_t ln" << e.sfx << " = lnA + " << u << "u;\n";
      o << "      const Key pkey" << e.sfx << "{pk0, pk1, (uint32_t)ln" << e.sfx << ", (uint32_t)(ln" << e.sfx << " >> 32)}; (void)pkey" << e.sfx << ";\n";
    });
    lanes.each([&](int, auto& e) { e.emit_scope_keys(); });
    o << "      const uint64_t pair0 = (lnA - 1u) >> 1;\n";
    if (NP == 2) o << "      const uint64_t pair1 = pair0 + 1u;\n";
    emit_pair_lane_sites(o, lanes, "      ", "po + iA", "score", ubase ? "ub" : "", "lb", full, nullptr, kind);
    if (P == 4) {
      const std::string wb = lanes.list("f2u(w", ")"), sb = lanes.list("f2u(sc", ")");
      if (ubase) {
        o << "      " << (full ? "" : "if (logw) ") << "store16_at(logw + ub, lb, make_uint4(" << wb << "), " << kind << ");\n";
        o << "      " << (full ? "" : "if (score) ") << "store16_at(score + ub, lb, make_uint4(" << sb << "), " << kind << ");\n";
      } else {
        o << "      if (logw) store16_out(logw + po + iA, make_uint4(" << wb << "), " << kind << ");\n";
        o << "      if (score) store16_out(score + po + iA, make_uint4(" << sb << "), " << kind << ");\n";
      }
    } else {
      o << "      if (logw) *reinterpret_cast<float" << P << "*>(logw + po + iA) = make_float" << P << "(" << lanes.list("w") << ");\n";
      o << "      if (score) *reinterpret_cast<float" << P << "*>(score + po + iA) = make_float" << P << "(" << lanes.list("sc") << ");\n";
    }
    o << "    }\n";
    o << "    " << (full ? "" : "if (max_partials || row_e) ") << "{\n";
    o << "      const float ninf = -__builtin_inff();\n";
    {
      std::string mx = "wA";
      for (int u = 1; u < P; ++u) mx = "(" + mx + " > w" + lanes.kSfx[u] + " ? " + mx + " : w" + lanes.kSfx[u] + ")";
      // (one wave per row: the maximum on integer keys — a generated kernel's log-weights are never -0, gjx_device.hpp)
      o << "      float bm = " << (waves_per_row == 1 ? "wave_max_ordered" : "wave_max") << "(ok ? " << mx << " : ninf);\n";
    }
    if (waves_per_row > 1) {
      o << "      __syncthreads();\n      if ((threadIdx.x & 63) == 0) sh_red[wv] = bm;\n      __syncthreads();\n";
      o << "      bm = sh_red[2 * pr] > sh_red[2 * pr + 1] ? sh_red[2 * pr] : sh_red[2 * pr + 1];\n";
    }
    // the row's writer lane.  The one-row quad form asks the row's own opaque lane offset: `tr == 0` is hoisted out of the row
    // loop as a lane mask that lives in a scalar-register pair, and with the cipher's round keys held in scalar registers
    // (v_bitop3_b32 reads them in place, gjx_device.hpp xor3) the allocator spilled that pair to a 65th VGPR — one more than
    // eight waves per SIMD allow.  One v_cmp per row instead.
    const char* lane0 = ubase ? "lb == 0u" : "tr == 0";
    o << "      if (" << (full ? "" : "max_partials && ") << lane0 << " && live_row) max_partials[rrow] = bm;\n";
    o << "      " << (full ? "" : "if (row_e) ") << "{\n";
    o << "        const int32_t eb = row_anchor(bm);\n";
    {
      std::string sm;
      for (int u = 0; u < P; ++u) sm += (u ? " + rowfix(w" : "rowfix(w") + std::string(lanes.kSfx[u]) + ", eb)";
      o << "        uint64_t sb = wave_sum_52(ok ? (" << sm << ") : 0);  // (at most four weights below 2^32)\n";
    }
    if (waves_per_row > 1) {
      o << "        __syncthreads();\n        if ((threadIdx.x & 63) == 0) sh_sum[wv] = sb;\n        __syncthreads();\n";
      o << "        sb = sh_sum[2 * pr] + sh_sum[2 * pr + 1];\n";
    }
    o << "        if (" << lane0 << " && live_row) lse_store_row(row_e, row_s, rrow, eb, sb, " << tail_scope(v.fused_tail) << ");\n";
    o << "      }\n    }\n";
    emit_kernel_close(o, v.fused_tail, kTicket);
    return o.str();
  }

  std::string run() {
    if (v.lane_particles >= 2 && v.impl == 1) return run_paired();
    const int impl = v.impl;
    const bool lds = bm_lds(impl, fast_math, sites, n_sites);
    emit_prelude(o, fast_math, lds, 256);
    emit_hint_default();
    // One workgroup per 256-particle row (grid-stride): short blocks keep every SIMD's wave slots
    // full even at 1e6 particles (15 rows per lane), where a 4-row block would serialise its rows.
    o << "extern \"C\" __global__ " << bounds(256) << " void " << v.kname() << signature();
    o << "  __shared__ float sh_red[4];\n  __shared__ uint64_t sh_sum[4];\n";
    emit_pass_key();
    o << "  asm volatile(\"\" :: \"s\"(bk0), \"s\"(bk1), \"s\"(grid_x));\n";
    if (lds) o << "  bm_stage();\n";
    o << "  const uint64_t po = (uint64_t)pass * bt.pass_stride, ro = (uint64_t)pass * bt.row_stride;\n";
    o << "  KeySrc kp = ks;\n";
    o << "  if (bt.n_pass > 1) { kp.parent.k0 = bk0; kp.parent.k1 = bk1; }\n";
    o << "  for (uint64_t row = blockIdx.x; row < bt.rows_per_pass; row += grid_x) {\n";
    o << "    float tmax = -__builtin_inff();\n    bool live = false;\n";
    o << "    {\n";
    o << "      const uint64_t li = row * 256 + threadIdx.x, i = po + li;\n";
    o << "      const bool ok = li < n;\n";
    o << "      if (ok) {\n";
    o << "        const Key pkey = key_at<" << impl << ">(kp, li);\n";
    o << "        float w = 0.0f, sc = 0.0f;\n";
    SiteEmitter<CSiteT, CArgT> em{o, impl, 0, sites, n_sites, "        "};
    em.sc = sc;
    em.run();
    o << "        if (logw) logw[i] = w;\n        if (score) score[i] = sc;\n        tmax = w;\n        live = true;\n";
    o << "      }\n    }\n";
    emit_row_epilogue_per_lane(o, "ro + row", v.fused_tail, kTicket);
    return o.str();
  }
};

// Importance over a Scan model (gjx_scan_run): one lane per particle walks all T steps — the key chain, the carry and
// the running weight / score stay in registers, every step stores its sampled values as one coalesced row of the
// time-major columns, and the epilogue is the importance kernel's (row maxima, row-anchored sums, in-launch fold).
//
// Which scan kernel a source is: the value that travels from gjx_scan_run to the generator, and the plan's slot.
struct ScanVariant {
  int impl = 0;       // the generator: 0 THREEFRY, 1 PHILOX
  bool quad = false;  // PHILOX, the lazy children of a lane-0 key, n and the columns multiples of four: FOUR adjacent particles
                      // per lane (one wave per 256-particle row).  A step's keys are lanes (scan_step_key_philox), so the
                      // lane's two pairs share their cipher blocks and Box-Muller transforms exactly as in the importance
                      // kernel's quad form; row statistics are wave reductions, every store is 16 bytes per lane.
  bool fused_tail = false;  // as ImportanceVariant::fused_tail: the in-launch fold of the row sums is a variant of its own (inlined,
                            // it took the one-particle-per-lane LGSSM kernel from 64 to 133 VGPRs, 7 -> 3 waves per SIMD)
  // `bits` = impl | GJX_SOURCE_FUSED_TAIL (the diagnostics), or a launch's generator with its tail bit; THREEFRY has no quad form
  static ScanVariant of(int bits, bool quad) {
    return ScanVariant{bits & ~GJX_SOURCE_FUSED_TAIL, quad && (bits & ~GJX_SOURCE_FUSED_TAIL) == 1, (bits & GJX_SOURCE_FUSED_TAIL) != 0};
  }
  static constexpr int kSlots = 6;  // THREEFRY, PHILOX one particle per lane, PHILOX four per lane; then the same with the fused fold
  constexpr int slot() const { return (quad ? 2 : impl) + (fused_tail ? 3 : 0); }
  const char* kname() const { return impl == 0 ? "gjx_scan_kernel_threefry" : "gjx_scan_kernel_philox"; }
};
static_assert(ScanVariant{0, false, false}.slot() == 0 && ScanVariant{1, false, false}.slot() == 1 && ScanVariant{1, true, false}.slot() == 2 &&
                  ScanVariant{0, false, true}.slot() == 3 && ScanVariant{1, false, true}.slot() == 4 && ScanVariant{1, true, true}.slot() == 5,
              "the six scan variants (THREEFRY has no quad form) have a slot of gjx_scan_plan::jit each");

template <class CSiteT, class CArgT>
struct GenScan {
  std::ostringstream o;
  ScanVariant v;
  const CSiteT* sites;
  int n_sites;
  const CArgT* next_state;
  int n_state, n_obs;
  bool fast_math = false;
  const ScopeInfo* sc = nullptr;  // nested calls inside the step kernel (null: a flat body)
  int block = 256;
  static constexpr const char* kSignature =
      "(KeySrc ks, RunCols cols, ScanArgs sa, float* score, float* logw, float* max_partials, int32_t* row_e, uint64_t* row_s, LseTail tail, PlanTables tabs) {\n";
  static constexpr const char* kTicket = "blockIdx.x, gridDim.x";  // (a one-dimensional grid)

  std::string run_quad() {
    block = 64;
    const bool lds = bm_lds(v.impl, fast_math, sites, n_sites);
    LaneGroup<CSiteT, CArgT> lanes(o, 4, v.impl, 2, sites, n_sites, "        ");
    lanes.each([&](int, auto& e) { e.store_values = false; e.row_cuts = true; e.sc = sc; });
    emit_prelude(o, fast_math, lds, block);
    o << "struct StepObs { const float* obs; };\n";
    o << "extern \"C\" __global__ __launch_bounds__(64) void " << v.kname() << kSignature;
    if (lds) o << "  bm_stage();\n";
    o << "  const uint64_t n = sa.n, rows_all = (n + 255) / 256;\n";
    o << "  const bool wt_one_pass = false; (void)wt_one_pass;  // (a scan's stores spread over its T steps)\n";
    o << "  const uint32_t pk0 = ks.parent.k0, pk1 = ks.parent.k1;\n";
    o << "  for (uint64_t row = blockIdx.x; row < rows_all; row += gridDim.x) {\n";
    o << "    const uint64_t iA = row * 256 + 4 * (uint64_t)threadIdx.x;\n";
    o << "    const bool ok = iA < n;  // (n is a multiple of four in this form: all particles of a lane exist or none)\n";
    lanes.each([&](int, auto& e) { o << "    float wt" << e.sfx << " = 0.0f, sct" << e.sfx << " = 0.0f;\n"; });
    o << "    if (ok) {\n";
    o << "      const uint64_t lnA = ks.first + iA + 1u;\n";
    lanes.each([&](int u, auto& e) {
      for (int k = 0; k < n_state; ++k) o << "      float st_" << k << e.sfx << " = sa.carry0_cols[" << k << "] ? sa.carry0_cols[" << k << "][iA + " << u << "] : sa.carry0[" << k << "];\n";
    });
    o << "      for (int32_t t = 0; t < sa.n_steps; ++t) {\n";
    o << "        const uint64_t lt = lnA + (((uint64_t)(uint32_t)t + 1u) << 40);  // the lanes of step t (scan_step_key_philox)\n";
    lanes.each([&](int u, auto& e) { o << "        const Key pkey" << e.sfx << "{pk0, pk1, (uint32_t)(lt + " << u << "u), (uint32_t)((lt + " << u << "u) >> 32)}; (void)pkey" << e.sfx << ";\n"; });
    o << "        const uint64_t pair0 = (lt - 1u) >> 1, pair1 = pair0 + 1u;\n";
    o << "        StepObs a; a.obs = sa.obs + (size_t)t * " << n_obs << "; (void)a;\n";
    o << "        const uint64_t oiA = (uint64_t)t * sa.col_stride + iA; (void)oiA;\n";
    lanes.each([&](int, auto& e) { o << "        float w" << e.sfx << " = 0.0f, sc" << e.sfx << " = 0.0f;\n"; });
    lanes.each([&](int, auto& e) { e.emit_scope_keys(); });
    emit_pair_lane_sites(o, lanes, "        ", "oiA");
    for (auto& e : lanes.em)
      for (int k = 0; k < n_state; ++k) o << "        const float nx_" << k << e.sfx << " = " << e.arg(next_state[k]) << ";\n";
    for (auto& e : lanes.em)
      for (int k = 0; k < n_state; ++k) o << "        st_" << k << e.sfx << " = nx_" << k << e.sfx << ";\n";
    lanes.each([&](int, auto& e) { o << "        wt" << e.sfx << " = wt" << e.sfx << " + w" << e.sfx << "; sct" << e.sfx << " = sct" << e.sfx << " + sc" << e.sfx << ";\n"; });
    o << "      }\n";
    for (int k = 0; k < n_state; ++k)
      o << "      if (sa.carry_out[" << k << "]) *reinterpret_cast<float4*>(sa.carry_out[" << k << "] + iA) = make_float4(" << lanes.list("st_" + std::to_string(k)) << ");\n";
    o << "      if (logw) *reinterpret_cast<float4*>(logw + iA) = make_float4(" << lanes.list("wt") << ");\n";
    o << "      if (score) *reinterpret_cast<float4*>(score + iA) = make_float4(" << lanes.list("sct") << ");\n";
    o << "    }\n";
    // (this form's own row statistics: see emit_row_epilogue_per_lane)
    o << "    if (max_partials || row_e) {\n";
    o << "      const float ninf = -__builtin_inff();\n";
    o << "      const float m4 = ((wtA > wtB ? wtA : wtB) > wtC ? (wtA > wtB ? wtA : wtB) : wtC);\n";
    o << "      const float bm = wave_max_ordered(ok ? (m4 > wtD ? m4 : wtD) : ninf);  // (wt starts at +0: never -0)\n";
    o << "      if (max_partials && threadIdx.x == 0) max_partials[row] = bm;\n";
    o << "      if (row_e) {\n";
    o << "        const int32_t eb = row_anchor(bm);\n";
    o << "        const uint64_t sb = wave_sum(ok ? (rowfix(wtA, eb) + rowfix(wtB, eb) + rowfix(wtC, eb) + rowfix(wtD, eb)) : 0);\n";
    o << "        if (threadIdx.x == 0) lse_store_row(row_e, row_s, row, eb, sb, " << tail_scope(v.fused_tail) << ");\n";
    o << "      }\n    }\n";
    emit_kernel_close(o, v.fused_tail, kTicket);
    return o.str();
  }
  std::string run() {
    if (v.quad && v.impl == 1) return run_quad();
    const int impl = v.impl;
    const bool lds = bm_lds(impl, fast_math, sites, n_sites);
    emit_prelude(o, fast_math, lds, 256);
    o << "struct StepObs { const float* obs; };\n";
    o << "extern \"C\" __global__ __launch_bounds__(256) void " << v.kname() << kSignature;
    o << "  __shared__ float sh_red[4];\n  __shared__ uint64_t sh_sum[4];\n";
    if (lds) o << "  bm_stage();\n";
    o << "  const uint64_t n = sa.n, rows_all = (n + 255) / 256;\n";
    o << "  for (uint64_t row = blockIdx.x; row < rows_all; row += gridDim.x) {\n";
    o << "    float tmax = -__builtin_inff();\n    bool live = false;\n";
    o << "    const uint64_t i = row * 256 + threadIdx.x;\n";
    o << "    if (i < n) {\n";
    o << "      Key " << (impl == 0 ? "pkey" : "pkey0") << " = key_at<" << impl << ">(ks, i);\n";
    for (int k = 0; k < n_state; ++k)
      o << "      float st_" << k << " = sa.carry0_cols[" << k << "] ? sa.carry0_cols[" << k << "][i] : sa.carry0[" << k << "];\n";
    o << "      float wt = 0.0f, sct = 0.0f;\n";
    o << "      for (int32_t t = 0; t < sa.n_steps; ++t) {\n";
    if (impl == 0) o << "        pkey = fold_in<0>(pkey, (uint32_t)t);  // chained: the folded key is carried (scan.py:267-268)\n";
    else o << "        const Key pkey = scan_step_key_philox(pkey0, (uint32_t)t);  // a lane per (particle, step): no cipher block\n";
    o << "        StepObs a; a.obs = sa.obs + (size_t)t * " << n_obs << "; (void)a;\n";
    o << "        const uint64_t oi = (uint64_t)t * sa.col_stride + i; (void)oi;\n";
    o << "        float w = 0.0f, sc = 0.0f;\n";
    SiteEmitter<CSiteT, CArgT> em{o, impl, 2, sites, n_sites, "        "};
    em.sc = sc;
    em.run();
    for (int k = 0; k < n_state; ++k) o << "        const float nx_" << k << " = " << em.arg(next_state[k]) << ";\n";
    for (int k = 0; k < n_state; ++k) o << "        st_" << k << " = nx_" << k << ";\n";
    o << "        wt = wt + w;\n        sct = sct + sc;\n      }\n";
    for (int k = 0; k < n_state; ++k) o << "      if (sa.carry_out[" << k << "]) sa.carry_out[" << k << "][i] = st_" << k << ";\n";
    o << "      if (logw) logw[i] = wt;\n      if (score) score[i] = sct;\n      tmax = wt;\n      live = true;\n    }\n";
    emit_row_epilogue_per_lane(o, "row", v.fused_tail, kTicket);
    return o.str();
  }
};

// Plan-driven bootstrap SMC: a generated policy inside the fused resample kernel (step) and a plain
// per-slot kernel (init).  State columns are gathered from global memory by ancestor index like the fixed models.
template <class CSiteT, class CArgT>
struct GenSmc {
  std::ostringstream o;
  int impl;
  const CSiteT* init_sites;
  int n_init;
  const CSiteT* step_sites;
  int n_step;
  const CArgT* init_state;
  const CArgT* next_state;
  int n_state;
  const ScopeInfo* sc_init = nullptr;  // nested calls inside init / step (null: flat bodies)
  const ScopeInfo* sc_step = nullptr;
  bool peers = false;  // r04: the step kernels of the peer transport (the source population lives in the peers' arenas)
  // include/gjx_smc_params.h: > 0 — the bodies read `prm.p[slot]` / `prm.d[2 site (+ 1)]` from the workgroup's filter's row
  // of the plan's device table, f32[filters][row_len()]: the caller's parameters, then the derived constants of the init
  // table's sites, then those of the step table's.  Both kernels take the table as one more argument
  // (`const float* __restrict__`: read-only for the launch) and copy the entries their body names into members at entry,
  // where the filter is known: a compile-time offset from a workgroup-uniform base each, so scalar loads into scalar
  // registers (entries no body names are never loaded).  0: the source is the plain plan's, byte for byte.
  int n_params = 0;
  int row_len() const { return n_params + 2 * (n_init + n_step); }
  // include/gjx_csmc.h: the CONDITIONAL kernels, a source of their own (gjx_smc_step_kernel_conditional,
  // gjx_smc_init_kernel_conditional: one more argument, CsmcRet).  The policy is GenPolicy plus one select per sampled site:
  // the slot CsmcRet names takes the retained value as the site's value — after the draw (consumed as ever: no draw is
  // renumbered) and in front of every log-density that reads it.  The lane that owns the slot loads the path's values; no
  // other lane, so no other workgroup, reads them.  false: today's source, byte for byte.
  bool cond = false;
  int ret_init[GJX_MAX_SITES], ret_step[GJX_MAX_SITES];  // csmc_components of the two bodies
  // The model condition: every sampled site of a body is, by itself, exactly one carry component ({GJX_ARG_SITE, s, 1, 0})
  // and every carry component is such a site.  comp[q] = the component of site q, or -1.
  static bool csmc_components(const CSiteT* sites, int n_sites, const CArgT* state, int n_state, int* comp) {
    for (int q = 0; q < n_sites; ++q) comp[q] = -1;
    for (int k = 0; k < n_state; ++k) {
      const CArgT& a = state[k];
      if (a.kind != GJX_ARG_SITE || a.scale != 1.0f || a.offset != 0.0f || a.ref_site < 0 || a.ref_site >= n_sites) return false;
      if (!sampled_mode(sites[a.ref_site].observed) || comp[a.ref_site] >= 0) return false;
      comp[a.ref_site] = k;
    }
    for (int q = 0; q < n_sites; ++q)
      if (sampled_mode(sites[q].observed) && comp[q] < 0) return false;
    return true;
  }
  // the retained values of a lane (`own`: does it hold the slot?) and, per slot of the lane, whether it is the slot
  void emit_ret_values(const char* ind, const std::string& own) {
    for (int k = 0; k < n_state; ++k) o << ind << "float rv_" << k << " = 0.0f;\n";
    o << ind << "if (" << own << ") {\n";
    for (int k = 0; k < n_state; ++k) o << ind << "  rv_" << k << " = ret.path[" << k << "][ret.t];\n";
    o << ind << "}\n";
  }
  void emit_prm_struct(const char* name, int n_sites, int d_off) {
    o << "struct " << name << " {\n  float p[" << n_params << "], d[" << 2 * n_sites << "];\n";
    o << "  __device__ __forceinline__ void load(const float* __restrict__ rows, uint32_t f) {\n";
    o << "    const float* __restrict__ row = rows + (size_t)f * " << row_len() << "u;\n";
    o << "#pragma unroll\n    for (int k = 0; k < " << n_params << "; ++k) p[k] = row[k];\n";
    o << "#pragma unroll\n    for (int k = 0; k < " << 2 * n_sites << "; ++k) d[k] = row[" << d_off << " + k];\n  }\n};\n";
  }

  // PHILOX: the four consecutive slots jq .. jq+3 of a lane (jq a multiple of 4) walked together.  One-word draw
  // number f of the quad is ONE block, PH(ctr = (g_lo, g_hi, f, 'Q'), key = step key), g = jq / 4, slot u taking
  // word u (for f = 0 and one Normal site this is the fixed LGSSM filter, bit for bit); Normal sites are two
  // Box-Muller transforms over the quad's words; multi-word samplers keep their per-slot streams.
  // The draws of the quad that do not depend on the ancestors — the cipher block of every one-word draw of the body's own
  // sites and the Box-Muller transforms of its Normal sites — can run under the latency of the step's first loads: the
  // policy's prefetch() (as the hand-written LgssmPolicy has it) keeps them in members (registers).
  int quad_draws(const CSiteT* sites, int n_sites, const ScopeInfo* sc) const {
    int n = 0;
    SiteEmitter<CSiteT, CArgT> e{const_cast<std::ostringstream&>(o), impl, 1, sites, n_sites, "", ""};
    e.sc = sc;
    for (int q = 0; q < n_sites; ++q)
      if (e.sampled(sites[q]) && e.one_word(sites[q]) && e.scope_of(q) == 0) ++n;
    return n;
  }
  void emit_prefetch(const CSiteT* sites, int n_sites, const ScopeInfo* sc) {
    SiteEmitter<CSiteT, CArgT> e{o, impl, 1, sites, n_sites, "    ", ""};
    e.sc = sc;
    o << "  __device__ __forceinline__ void prefetch(int64_t jq) {\n    const uint64_t g = (uint64_t)jq >> 2;\n";
    int i = 0;
    for (int q = 0; q < n_sites; ++q) {
      const CSiteT& st = sites[q];
      if (!e.sampled(st) || !e.one_word(st) || e.scope_of(q) != 0) continue;
      o << "    philox4x32(a.step_key.k0, a.step_key.k1, (uint32_t)g, (uint32_t)(g >> 32), " << e.fold_of(q) << "u, kTagQuad, pf_w[" << i
        << "][0], pf_w[" << i << "][1], pf_w[" << i << "][2], pf_w[" << i << "][3]);\n";
      if (st.dist == GJX_DIST_NORMAL) {
        o << "    bm_pair(pf_w[" << i << "][0], pf_w[" << i << "][1], pf_z[" << i << "][0], pf_z[" << i << "][1]);\n";
        o << "    bm_pair(pf_w[" << i << "][2], pf_w[" << i << "][3], pf_z[" << i << "][2], pf_z[" << i << "][3]);\n";
      }
      ++i;
    }
    o << "  }\n";
  }
  void emit_quad_body(const CSiteT* sites, int n_sites, const CArgT* state_args, bool step, bool prefetched = false) {
    int pf_i = 0;
    const ScopeInfo* sc = step ? sc_step : sc_init;
    LaneGroup<CSiteT, CArgT> lanes(o, 4, impl, 1, sites, n_sites, "    ");
    lanes.each([&](int, auto& e) { e.sc = sc; });
    auto& em = lanes.em;
    const auto& sf = lanes.kSfx;
    o << "    const uint64_t g = (uint64_t)jq >> 2;\n";
    if (cond) {  // (the retained slot may be any word of its quad)
      for (int u = 0; u < 4; ++u) {
        em[u].ret_comp = step ? ret_step : ret_init;
        o << "    const bool rsel" << sf[u] << " = jq + " << u << " == ret.slot;\n";
      }
      emit_ret_values("    ", "(uint64_t)(ret.slot - jq) < 4u");
    }
    for (int u = 0; u < 4; ++u) {
      if (step)
        for (int k = 0; k < n_state; ++k) o << "    const float st_" << k << sf[u] << " = src_load<kPeers>(a.prev_state[" << k << "], src[" << u << "], pd, tpr);\n";
      if (em[u].needs_stream_key() || sc) o << "    const Key pkey" << sf[u] << " = slot_key<1>(a.step_key, (uint64_t)jq + " << u << "u);\n";
      o << "    float w" << sf[u] << " = 0.0f, sc" << sf[u] << " = 0.0f;\n";
      em[u].emit_scope_keys();
    }
    for (int q = 0; q < n_sites; ++q) {
      const CSiteT& st = sites[q];
      const std::string Q = std::to_string(q);
      for (int u = 0; u < 4; ++u) em[u].head(q);
      const bool drawn = em[0].sampled(st) && em[0].one_word(st) && em[0].scope_of(q) == 0;  // (a callee's sites: their own lone keys)
      const bool normal = drawn && st.dist == GJX_DIST_NORMAL;
      if (drawn && prefetched) {  // (computed by prefetch(): the same block, the same transforms)
        for (int u = 0; u < 4; ++u) o << "    const uint32_t bits" << Q << sf[u] << " = pf_w[" << pf_i << "][" << u << "]; (void)bits" << Q << sf[u] << ";\n";
        if (normal)
          for (int u = 0; u < 4; ++u) o << "    const float z" << Q << sf[u] << " = pf_z[" << pf_i << "][" << u << "];\n";
        ++pf_i;
      } else if (drawn) {
        o << "    uint32_t qw" << Q << "_0, qw" << Q << "_1, qw" << Q << "_2, qw" << Q << "_3;\n";
        o << "    philox4x32(a.step_key.k0, a.step_key.k1, (uint32_t)g, (uint32_t)(g >> 32), " << em[0].fold_of(q)
          << "u, kTagQuad, qw" << Q << "_0, qw" << Q << "_1, qw" << Q << "_2, qw" << Q << "_3);\n";
        for (int u = 0; u < 4; ++u) o << "    const uint32_t bits" << Q << sf[u] << " = qw" << Q << "_" << u << ";\n";
        if (normal) {
          o << "    float z" << Q << "A, z" << Q << "B, z" << Q << "C, z" << Q << "D;\n";
          o << "    bm_pair(bits" << Q << "A, bits" << Q << "B, z" << Q << "A, z" << Q << "B);\n";
          o << "    bm_pair(bits" << Q << "C, bits" << Q << "D, z" << Q << "C, z" << Q << "D);\n";
        }
      }
      for (int u = 0; u < 4; ++u) em[u].tail(q, normal ? "z" + Q + sf[u] : std::string());
      for (int u = 0; u < 4; ++u) em[u].close_scopes(q + 1);
    }
    for (int u = 0; u < 4; ++u) {
      for (int k = 0; k < n_state; ++k) o << "    out[" << u << "].s[" << k << "] = " << em[u].arg(state_args[k]) << ";\n";
      o << "    (void)sc" << sf[u] << ";\n    wq[" << u << "] = w" << sf[u] << ";\n";
    }
  }
  void emit_quad(const CSiteT* sites, int n_sites, const CArgT* state_args, bool step) {
    const int nq = quad_draws(sites, n_sites, step ? sc_step : sc_init);
    if (nq > 0) {
      o << "  uint32_t pf_w[" << nq << "][4];\n  float pf_z[" << nq << "][4];\n";
      emit_prefetch(sites, n_sites, step ? sc_step : sc_init);
    }
    o << "  __device__ __forceinline__ void compute_quad(int64_t jq, const uint32_t (&src)[4], Out (&out)[4], float (&wq)[4]) const {\n";
    emit_quad_body(sites, n_sites, state_args, step, nq > 0);
    o << "  }\n";
  }

  std::string run() {
    const std::string I = std::to_string(impl), D = std::to_string(n_state);
    emit_prelude(o);
    SiteEmitter<CSiteT, CArgT> es{o, impl, 1, step_sites, n_step, "    "};
    SiteEmitter<CSiteT, CArgT> ei{o, impl, 1, init_sites, n_init, "        "};
    es.sc = sc_step;
    ei.sc = sc_init;
    if (cond) { es.ret_comp = ret_step; ei.ret_comp = ret_init; }
    const std::string RET_ARG = cond ? ", CsmcRet ret" : "";
    // ---- step policy
    if (n_params > 0) emit_prm_struct("GenStepPrm", n_step, n_params + 2 * n_init);
    o << "struct GenPolicy {\n  static constexpr bool kEmit = true;\n  static constexpr bool kPeers = " << (peers ? "true" : "false") << ";\n  PlanPolicyArgs a;\n  PlanTables tabs;\n";
    o << "  const int64_t* pd = nullptr;\n  uint32_t tpr = 1;\n";
    if (cond) o << "  CsmcRet ret;\n";
    o << "  __device__ __forceinline__ void set_peers(const int64_t* d, uint32_t t) { pd = d; tpr = t; }\n";
    o << "  struct Out { float s[" << D << "]; };\n";
    if (n_params > 0) {
      o << "  GenStepPrm prm;\n  const float* __restrict__ prm_rows = nullptr;\n";
      o << "  __device__ __forceinline__ void load_params(uint32_t f) { prm.load(prm_rows, f); }\n";
    }
    o << "  __device__ __forceinline__ void select_filter(uint64_t off, Key k) {\n";
    o << "    for (int c = 0; c < " << D << "; ++c) { a.prev_state[c] += off; a.state_out[c] += off; }\n";
    o << "    if (a.anc_out) a.anc_out += off; a.step_key = k;\n  }\n";
    o << "  __device__ __forceinline__ float compute(int64_t j, uint32_t src_global, Out& out) const {\n";
    for (int k = 0; k < n_state; ++k) o << "    const float st_" << k << " = src_load<kPeers>(a.prev_state[" << k << "], src_global, pd, tpr);\n";
    if (es.needs_pk() || sc_step) o << "    const Key pkey = slot_key<" << I << ">(a.step_key, (uint64_t)j);\n";
    o << "    float w = 0.0f, sc = 0.0f;\n";
    if (cond) {
      o << "    const bool rsel = j == ret.slot;\n";
      emit_ret_values("    ", "rsel");
    }
    es.run();
    for (int k = 0; k < n_state; ++k) o << "    out.s[" << k << "] = " << es.arg(next_state[k]) << ";\n";
    o << "    (void)sc;\n    return w;\n  }\n";
    if (impl == 1) emit_quad(step_sites, n_step, next_state, true);
    o << "  __device__ __forceinline__ void store(int64_t j, int64_t out_lo, uint32_t src, const Out& out) const {\n";
    o << "    for (int k = 0; k < " << D << "; ++k) a.state_out[k][j - out_lo] = out.s[k];\n";
    o << "    if (a.anc_out) a.anc_out[j - out_lo] = (int32_t)src;\n  }\n";
    // the lane's four consecutive slots at once: one 16-byte (write-through, for one-filter launches) store per column
    o << "  __device__ __forceinline__ void store_quad(int64_t jq, int64_t out_lo, const uint32_t (&anc)[4], const Out (&o)[4], const bool (&ok)[4]) const {\n";
    o << "    const int64_t k = jq - out_lo;\n";
    o << "    uintptr_t al = (uintptr_t)a.anc_out;\n";
    o << "    for (int c = 0; c < " << D << "; ++c) al |= (uintptr_t)a.state_out[c];\n";
    o << "    if ((al & 15) == 0 && ok[0] && ok[1] && ok[2] && ok[3]) {\n";
    o << "      for (int c = 0; c < " << D << "; ++c) store16_out(a.state_out[c] + k, make_uint4(f2u(o[0].s[c]), f2u(o[1].s[c]), f2u(o[2].s[c]), f2u(o[3].s[c])), a.wt != 0);\n";
    o << "      if (a.anc_out) store16_out(a.anc_out + k, make_uint4(anc[0], anc[1], anc[2], anc[3]), a.wt != 0);\n";
    o << "      return;\n    }\n";
    o << "    for (int u = 0; u < 4; ++u) if (ok[u]) store(jq + u, out_lo, anc[u], o[u]);\n  }\n};\n";
    // two instantiations, as for the hand-written filters: the every-step form carries no ESS decision / keep-your-particle path
    const std::string PRM_ARG = n_params > 0 ? ", const float* __restrict__ prm_rows" : "", PRM_SET = n_params > 0 ? "  P.prm_rows = prm_rows;\n" : "";
    if (cond) {  // (every-step, one device: no adaptive and no peer form)
      o << "extern \"C\" __global__ __launch_bounds__(256) void gjx_smc_step_kernel_conditional(ResampleArgs A, PlanPolicyArgs PA, PlanTables T" << PRM_ARG << RET_ARG << ") {\n";
      o << "  GenPolicy P;\n  P.a = PA;\n  P.tabs = T;\n  P.ret = ret;\n" << PRM_SET << "  resample_body<" << I << ", GenPolicy, false, false, true>(A, P);\n}\n";
    } else {
    o << "extern \"C\" __global__ __launch_bounds__(256) void gjx_smc_step_kernel(ResampleArgs A, PlanPolicyArgs PA, PlanTables T" << PRM_ARG << ") {\n";
    o << "  GenPolicy P;\n  P.a = PA;\n  P.tabs = T;\n" << PRM_SET << "  resample_body<" << I << ", GenPolicy, false, GenPolicy::kPeers>(A, P);\n}\n";
    o << "extern \"C\" __global__ __launch_bounds__(256) void gjx_smc_step_kernel_adaptive(ResampleArgs A, PlanPolicyArgs PA, PlanTables T" << PRM_ARG << ") {\n";
    o << "  GenPolicy P;\n  P.a = PA;\n  P.tabs = T;\n" << PRM_SET << "  resample_body<" << I << ", GenPolicy, true, GenPolicy::kPeers>(A, P);\n}\n";
    }
    // ---- init kernel: one workgroup per LOCAL tile, like k_lgssm_init
    if (n_params > 0) emit_prm_struct("GenInitPrm", n_init, n_params);
    if (impl == 1) {
      o << "struct GenInitOut { float s[" << D << "]; };\n";
      o << "__device__ __forceinline__ void init_quad(const PlanPolicyArgs& a, const PlanTables& tabs, " << (n_params > 0 ? "const GenInitPrm& prm, " : "")
        << "int64_t jq, GenInitOut (&out)[4], float (&wq)[4]" << (cond ? ", const CsmcRet& ret" : "") << ") {\n";
      emit_quad_body(init_sites, n_init, init_state, false);
      o << "}\n";
    }
    o << "extern \"C\" __global__ __launch_bounds__(256) void gjx_smc_init_kernel" << (cond ? "_conditional" : "") << "(PlanPolicyArgs a, uint64_t first_slot, uint64_t n_local, EmitOut em, FilterBatch fb, PlanTables tabs" << PRM_ARG << RET_ARG << ") {\n";
    o << "  uint64_t ltile = blockIdx.x;\n";
    if (n_params > 0) o << "  uint32_t filter = 0;\n";
    o << "  if (fb.n_filters > 1) {  // several filters per launch: tile of filter f, its key, its outputs\n";
    o << "    const uint32_t f = (uint32_t)(ltile / fb.tiles);\n    ltile -= (uint64_t)f * fb.tiles;\n    a.step_key = fb.step_key[f];\n";
    if (n_params > 0) o << "    filter = f;\n";
    o << "    for (int k = 0; k < " << D << "; ++k) a.state_out[k] += (uint64_t)f * fb.stride;\n";
    o << "    if (a.anc_out) a.anc_out += (uint64_t)f * fb.stride;\n    select_filter_emit(em, fb, f);\n  }\n";
    if (n_params > 0) o << "  GenInitPrm prm;\n  prm.load(prm_rows, filter);  // (this filter's row: scalar loads, in front of every store)\n";
    o << "  const uint64_t loc = ltile * kTile + 4 * (uint64_t)threadIdx.x;\n  const uint64_t gq = first_slot + loc;\n";
    o << "  float wq[4];\n  bool okq[4];\n  for (int u = 0; u < 4; ++u) okq[u] = loc + u < n_local;\n";
    if (impl == 1) {  // four consecutive slots per lane, one cipher block per one-word draw of the quad
      o << "  {\n    const int64_t jq = (int64_t)gq;\n    GenInitOut out[4];\n";
      o << "    init_quad(a, tabs, " << (n_params > 0 ? "prm, " : "") << "jq, out, wq" << (cond ? ", ret" : "") << ");\n";
      o << "    for (int u = 0; u < 4; ++u) {\n      if (okq[u]) {\n";
      for (int k = 0; k < n_state; ++k) o << "        a.state_out[" << k << "][loc + u] = out[u].s[" << k << "];\n";
      o << "        if (a.anc_out) a.anc_out[loc + u] = (int32_t)(gq + u);\n      }\n    }\n  }\n";
    } else {
      o << "  for (int u = 0; u < 4; ++u) {\n    const uint64_t j = gq + u;\n    wq[u] = 0.0f;\n    {\n";
      if (ei.needs_pk() || sc_init) o << "        const Key pkey = slot_key<" << I << ">(a.step_key, j);\n";
      o << "        float w = 0.0f, sc = 0.0f;\n";
      if (cond) {
        o << "        const bool rsel = (int64_t)j == ret.slot;\n";
        emit_ret_values("        ", "rsel");
      }
      ei.run();
      for (int k = 0; k < n_state; ++k) o << "        const float ns_" << k << " = " << ei.arg(init_state[k]) << ";\n";
      o << "        (void)sc;\n        wq[u] = w;\n        if (okq[u]) {\n";
      for (int k = 0; k < n_state; ++k) o << "          a.state_out[" << k << "][loc + u] = ns_" << k << ";\n";
      o << "          if (a.anc_out) a.anc_out[loc + u] = (int32_t)j;\n        }\n    }\n  }\n";
    }
    o << "  emit_init_tile(wq, okq, em, loc, first_slot / kTile + ltile);\n}\n";
    return o.str();
  }
};

// The transition table of a backward pass as ONE device function, the static member of a generated struct:
// GenTrans::trans_lp(a, tabs, state of candidate i, next state of trajectory j) -> the f32 sum of the table's log-densities,
// emitted by SiteEmitter exactly as an SMC step's weight is (mode 1: st_<k>, a.obs[]; nx_<c> for GJX_ARG_NEXT).  `a` is the
// kernel's argument block (BacksimArgs or BackmoveArgs: the walk reads a.obs[] alone).
template <class CSiteT, class CArgT>
inline void emit_trans_struct(std::ostringstream& o, int impl, const CSiteT* sites, int n_sites, int n_state) {
  o << "struct GenTrans {\n  template <class Args>\n  static __device__ __forceinline__ float trans_lp(const Args& a, const PlanTables& tabs, const float (&st)["
    << n_state << "], const float (&nx)[" << n_state << "]) {\n";
  for (int k = 0; k < n_state; ++k) o << "    const float st_" << k << " = st[" << k << "], nx_" << k << " = nx[" << k << "];\n";
  for (int k = 0; k < n_state; ++k) o << "    (void)st_" << k << "; (void)nx_" << k << ";\n";
  o << "    float w = 0.0f, sc = 0.0f;\n";
  SiteEmitter<CSiteT, CArgT> e{o, impl, 1, sites, n_sites, "    ", ""};
  e.run();
  o << "    (void)sc;\n    return w;\n  }\n};\n";
}

// The kernels of a backward-simulation plan (include/gjx_backsim.h): the transition struct and two instantiations of
// gjx_device.hpp backsim_body (the last step's has no next state).
template <class CSiteT, class CArgT>
struct GenBacksim {
  std::ostringstream o;
  int impl;
  const CSiteT* sites;
  int n_sites;
  int n_state;

  std::string run() {
    emit_prelude(o);
    emit_trans_struct<CSiteT, CArgT>(o, impl, sites, n_sites, n_state);
    const std::string ID = "<" + std::to_string(impl) + ", " + std::to_string(n_state);
    o << "extern \"C\" __global__ __launch_bounds__(256) void gjx_backsim_step_kernel(BacksimArgs a, PlanTables tabs) { backsim_body" << ID << ", GenTrans, false>(a, tabs); }\n";
    o << "extern \"C\" __global__ __launch_bounds__(256) void gjx_backsim_last_kernel(BacksimArgs a, PlanTables tabs) { backsim_body" << ID << ", GenTrans, true>(a, tabs); }\n";
    return o.str();
  }
};

// The kernels of the MCMC backward sampler (include/gjx_backmove.h) over the SAME transition table: the same struct, and
// around it the helpers of gjx_device.hpp (backmove_score, backmove_stage, backmove_draw, backmove_moves<B>, backmove_store).
// The two kernels' own loops over paths are still emitted here: inside a device function they lose what the compiler does
// for a kernel function alone (the uniform-workgroup form of blockDim.x, the no-clobber marks of its argument loads), and
// the machine code changes (profiles/fixed_bodies_summary.md).
template <class CSiteT, class CArgT>
struct GenBackmove {
  std::ostringstream o;
  int impl;
  const CSiteT* sites;
  int n_sites;
  int n_state;

  std::string run() {
    emit_prelude(o);
    emit_trans_struct<CSiteT, CArgT>(o, impl, sites, n_sites, n_state);
    const std::string I = std::to_string(impl), D = std::to_string(n_state), IDT = "<" + I + ", " + D + ", GenTrans, ";
    // step t < T - 1: path j starts at the ancestor of its row-(t + 1) particle and makes a.n_moves moves
    o << "extern \"C\" __global__ __launch_bounds__(256) void gjx_backmove_step_kernel(BackmoveArgs a, PlanTables tabs) {\n";
    o << "  __shared__ uint64_t sh_ends[kBackmoveLdsTiles];\n";
    o << "  const uint32_t n = a.n, m = a.m, K = a.n_moves;\n  uint64_t Q = 0;\n";
    o << "  if (K) {\n    Q = a.cdf[n - 1u];\n    if (a.coarse) backmove_stage(a, sh_ends);\n  }\n";
    o << "  for (uint64_t j64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j64 < m; j64 += (uint64_t)gridDim.x * blockDim.x) {\n";
    o << "    const uint32_t j = (uint32_t)j64;\n";
    o << "    uint32_t nxt = (uint32_t)a.lin_next[j];\n    nxt = nxt < n ? nxt : n - 1u;\n";
    o << "    float nx[" << D << "];\n    for (int c = 0; c < " << D << "; ++c) nx[c] = backsim_col(a.col_next[c][nxt], (a.i32_mask >> c) & 1u);\n";
    o << "    uint32_t cur = (uint32_t)a.anc_next[nxt];\n    cur = cur < n ? cur : n - 1u;\n";
    o << "    if (K) {\n      float s_cur = backmove_score<" << D << ", GenTrans>(a, tabs, cur, nx);\n      uint32_t r = 0;\n";
    o << "      for (; r + 4u <= K; r += 4u) backmove_moves" << IDT << "4>(a, tabs, sh_ends, Q, j, r, nx, cur, s_cur);\n";
    o << "      if (K - r >= 2u) { backmove_moves" << IDT << "2>(a, tabs, sh_ends, Q, j, r, nx, cur, s_cur); r += 2u; }\n";
    o << "      if (K - r >= 1u) backmove_moves" << IDT << "1>(a, tabs, sh_ends, Q, j, r, nx, cur, s_cur);\n    }\n";
    o << "    backmove_store<" << D << ">(a, j, cur);\n  }\n}\n";
    // step T - 1: path j is one multinomial draw from the final weights
    o << "extern \"C\" __global__ __launch_bounds__(256) void gjx_backmove_last_kernel(BackmoveArgs a, PlanTables tabs) {\n";
    o << "  __shared__ uint64_t sh_ends[kBackmoveLdsTiles];\n  (void)tabs;\n";
    o << "  const uint64_t Q = a.cdf[a.n - 1u];\n  if (a.coarse) backmove_stage(a, sh_ends);\n";
    o << "  for (uint64_t j64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j64 < a.m; j64 += (uint64_t)gridDim.x * blockDim.x) {\n";
    o << "    const uint32_t e[1] = {(uint32_t)j64};\n    uint32_t i[1];\n    backmove_draw<" << I << ", 1>(a, sh_ends, Q, e, i);\n";
    o << "    backmove_store<" << D << ">(a, e[0], i[0]);\n  }\n}\n";
    return o.str();
  }
};

// The shadow table of the tempered family (GenTemper, GenPointwise, GenPredictive), built once from a plan's site table: a COPY
// in which every latent site is an observed one whose value is the function argument nx_<l> — the register or the column
// entry the caller holds (the GJX_ARG_NEXT form of the transition tables, ref l in table order, scale 1) — and a PLATED site
// (include/gjx_plate.h) is re-moded for the emitters: an observed site inside its loop over the data rows, or, `drawn`, a
// LATENT one whose value is drawn and goes to no output column (the draws go where predictive_keep_rows puts them).
template <class CSiteT, class CArgT>
struct TemperTable {
  std::vector<CSiteT> tab;
  int L = 0;                // latents
  std::vector<int> plated;  // table positions of the plated sites: plated site s is plated[s]
  std::vector<int> cs;      // the data columns the plated sites read between them, in ascending order
  std::vector<int> grouped;  // table positions of the grouped sites (include/gjx_group.h): grouped site s is grouped[s]

  // Does site `st` read a grouped value (a GROUP operand in a0 / a1, directly or in a program)?
  static bool reads_group(const CSiteT& st) {
    for (const CArgT* a : {&st.a0, &st.a1}) {
      if (a->kind == GJX_ARG_GROUP) return true;
      if (a->kind != GJX_ARG_EXPR) continue;
      const gjx_expr_op* ops = reinterpret_cast<const gjx_expr_op*>(a->table);
      for (int k = 0; k < a->ref; ++k)
        if (ops[k].op == GJX_EXPR_GROUP) return true;
    }
    return false;
  }

  // The data columns plated site q reads (a0, a1, obs; affine operands and program leaves), in ascending order.
  static std::vector<int> plate_cols(const CSiteT& st) {
    bool used[GJX_PLATE_MAX_COLS] = {};
    // (a count site's log k! column, the one after its observed column: include/gjx_counts.h)
    if ((st.dist == GJX_DIST_POISSON || st.dist == GJX_DIST_NEGATIVE_BINOMIAL) && st.obs.kind == GJX_ARG_DATA) used[st.obs.ref + 1] = true;
    for (const CArgT* a : {&st.a0, &st.a1, &st.obs}) {
      if (a->kind == GJX_ARG_DATA) used[a->ref] = true;
      if (a->kind != GJX_ARG_EXPR) continue;
      const gjx_expr_op* ops = reinterpret_cast<const gjx_expr_op*>(a->table);
      for (int k = 0; k < a->ref; ++k)
        if (ops[k].op == GJX_EXPR_DATA) used[ops[k].ref] = true;
    }
    return set_of(used);
  }
  static std::vector<int> set_of(const bool (&used)[GJX_PLATE_MAX_COLS]) {
    std::vector<int> cs;
    for (int c = 0; c < GJX_PLATE_MAX_COLS; ++c)
      if (used[c]) cs.push_back(c);
    return cs;
  }
  TemperTable(const CSiteT* sites, int n_sites, bool drawn = false) : tab(sites, sites + n_sites) {
    bool used[GJX_PLATE_MAX_COLS] = {};
    for (int q = 0; q < n_sites; ++q) {
      if (sites[q].observed == GJX_SITE_PLATED) {
        for (int c : plate_cols(sites[q])) used[c] = true;
        tab[q].observed = drawn ? 0 : 1;
        if (drawn) tab[q].out_col = -1;
        plated.push_back(q);
      }
      if (sites[q].observed == GJX_SITE_GROUPED) {  // (include/gjx_group.h) an observed site whose value is the argument gz_<s>
        tab[q].observed = 1;
        tab[q].out_col = -1;
        tab[q].obs = CArgT{};
        tab[q].obs.kind = GJX_ARG_GROUP;
        tab[q].obs.ref = (int)grouped.size();
        tab[q].obs.scale = 1.0f;
        grouped.push_back(q);
        continue;
      }
      if (sites[q].observed) continue;
      tab[q].observed = 1;
      tab[q].obs = CArgT{};
      tab[q].obs.kind = GJX_ARG_NEXT;
      tab[q].obs.ref = L++;
      tab[q].obs.scale = 1.0f;
    }
    cs = set_of(used);
  }
  // pre0post pre1post ... pre<L-1>post: the latents as parameters or arguments
  std::string list(const std::string& pre, const std::string& post = "") const {
    std::string t;
    for (int l = 0; l < L; ++l) t += pre + std::to_string(l) + post;
    return t;
  }
  // pre<c>sfx for every data column c and every lane suffix: the rows' data values dc<c> (SiteEmitter's names of a DATA
  // operand under the suffixes) as parameters or arguments
  std::string data_list(const std::string& pre, std::initializer_list<const char*> sfx) const {
    std::string t;
    for (int c : cs)
      for (const char* s : sfx) t += pre + std::to_string(c) + s;
    return t;
  }
  // pre<s>sfx for every grouped site s and every lane suffix: the values gz_<s> of the row's group (SiteEmitter's names of a
  // GROUP operand under the suffixes) as parameters or arguments; empty for a table without grouped sites
  std::string group_list(const std::string& pre, std::initializer_list<const char*> sfx) const {
    std::string t;
    for (int s = 0; s < (int)grouped.size(); ++s)
      for (const char* x : sfx) t += pre + std::to_string(s) + x;
    return t;
  }
  // The numbering of the draws of a `drawn` table, as a ScopeInfo of one scope.  It numbers the PLATED sites alone, in table
  // order — include/gjx_predictive.h defines the draws as an importance pass over a table of just those sites — so site q
  // carries the count of plated sites before it: fold_t, THREEFRY's 1-based counter of that table's sites; fold_p, PHILOX's
  // 0-based index among its sampled sites (all of them).  (The entries of the other sites are never read: they draw nothing.)
  ScopeInfo draw_numbering() const {
    ScopeInfo si;
    si.n_scopes = 0;
    si.parent[0] = -1;
    uint32_t s = 0;
    for (int q = 0; q < (int)tab.size(); ++q) {
      si.site_scope[q] = 0;
      si.fold_t[q] = s + 1u;
      si.fold_p[q] = s;
      if (s < plated.size() && plated[s] == q) ++s;
    }
    return si;
  }
};

// The transposed particle loop of GenPointwise and GenPredictive: lanes are data ROWS, the particles of the workgroup's chunk
// (blockIdx.y) are wave-uniform and walked in index order.  The latent columns are read through constant-address-space pointers
// at the loop counter — scalar loads, issued for a block of NB particles (x<l>_<j>) before `block`, the block's statements; a
// remainder loop runs `rest` (the loop's body, reading xc<l>[i]: no read past x_l[n - 1]).  `prologue` and `epilogue` are the
// accumulators' lines around the two loops.
template <class Table>
inline void emit_particle_loop(std::ostream& o, const Table& t, int NB, const std::string& prologue, const std::string& block,
                               const std::string& rest, const std::string& epilogue) {
  for (int l = 0; l < t.L; ++l) o << "  const PlateCol xc" << l << " = (PlateCol)a.x[" << l << "];\n";
  o << "  const uint64_t lo64 = (uint64_t)blockIdx.y * a.per;\n";
  o << "  const uint32_t lo = lo64 < a.n ? (uint32_t)lo64 : a.n;\n";
  o << "  const uint32_t hi = a.n - lo > a.per ? lo + a.per : a.n;\n";
  o << prologue << "  uint32_t i = lo;\n";
  o << "  for (; hi - i >= " << NB << "u; i += " << NB << "u) {\n";
  for (int l = 0; l < t.L; ++l)
    for (int j = 0; j < NB; ++j) o << "    const float x" << l << "_" << j << " = xc" << l << "[(size_t)i + " << j << "u];\n";
  o << block << "  }\n";
  o << "  for (; i < hi; ++i)" << rest << epilogue;
}

// The move kernel of a tempered SMC sampler (include/gjx_temper.h) over a flat importance-style site table: one lane per
// particle, the chain's state (L latent values, lp, ll) in registers, K Metropolis-Hastings sweeps in a run-time loop.
//   assess   tm_assess is the table's walk by SiteEmitter (mode 0: parameters, input columns and postfix programs as in an
//            importance kernel) over the TemperTable: every latent site is an observed one whose value is the function
//            argument nx_<l> — the register the chain holds.
//            Nothing is drawn in it; the latent sites' log-densities go to lp (-inf outside a Gamma's / Beta's open support:
//            the density formulas are TFP's and do not say so themselves — a Gamma(1, b) is finite below 0), the observed
//            sites' to ll.
//   propose  x'_l = x_l + scales[l] * site_normal(Stream(split_at(p_r, i), fold of latent l)): what k_sample_normal computes
//            for the lazy children of p_r.  Under PHILOX latents 2 k and 2 k + 1 read the same pair block (one cipher
//            call after common-subexpression elimination).
//   cov      the SECOND kernel of a plan (include/gjx_temper_cov.h; `cov`): gjx_temper_move_cov_kernel proposes
//            x' = x + F eps through a packed lower triangle F, one more pointer argument (before PlateData).  It shares
//            tm_assess and everything else; the source of the diagonal kernel does not change with it.
//   keys     fold_in(key, r) and its two children are wave-uniform: three cipher blocks per sweep on the scalar side.
//   plated   a GJX_SITE_PLATED site (include/gjx_plate.h) is a loop over the data rows inside tm_assess (emit_plated): its
//            arguments and value read the row of the data columns, its f32 log-densities enter ll through a float64 sum.  The
//            columns and the row count are one more kernel argument (PlateData pd), of plated plans only: the source of a
//            table without plated sites is what it was before they existed, byte for byte.
// No LDS (the Box-Muller tables are read from the constant arrays: GJX_BM_LDS is not defined), no barrier.
template <class CSiteT, class CArgT>
struct GenTemper {
  std::ostringstream o;
  int impl;
  const CSiteT* sites;
  int n_sites;
  bool cov = false;  // the covariance move (include/gjx_temper_cov.h): gjx_temper_move_cov_kernel, x' = x + F eps

  // A PLATED site (include/gjx_plate.h) at its table position: the loop over the data rows.  The row index is a counter
  // against a kernel argument and the columns are constant-address-space pointers out of the argument block, so every read
  // is a wave-uniform SCALAR load; a block of kPlateBlock rows issues its loads (one s_load_dwordx4 per column) before its
  // arithmetic, a remainder loop takes the last n_rows % kPlateBlock rows.  Rows enter the float64 sum in index order.
  static constexpr int kPlateBlock = 4;
  void emit_plated(int q, const CSiteT* tab) {
    const std::vector<int> cs = TemperTable<CSiteT, CArgT>::plate_cols(tab[q]);
    const std::string Q = std::to_string(q);
    std::ostringstream body;  // one row: head (arguments and value from dc<c>), the log-density, the float64 accumulate
    SiteEmitter<CSiteT, CArgT> e{body, impl, 0, tab, n_sites, "      ", ""};
    e.exact_cuts = false;
    e.head(q);
    body << "      pacc" << Q << " = pacc" << Q << " + (double)(" << e.lp_of(q) << ");\n";
    o << "  // site " << q << ": plated over pd.n_rows data rows\n";
    for (int c : cs) o << "  const PlateCol pc" << Q << "_" << c << " = (PlateCol)pd.col[" << c << "];\n";
    o << "  double pacc" << Q << " = 0.0;\n  uint32_t d" << Q << " = 0u;\n";
    o << "  for (; d" << Q << " + " << kPlateBlock << "u <= pd.n_rows; d" << Q << " += " << kPlateBlock << "u) {\n";
    for (int c : cs)
      for (int j = 0; j < kPlateBlock; ++j)
        o << "    const float r" << c << "_" << j << " = pc" << Q << "_" << c << "[d" << Q << " + " << j << "u];\n";
    for (int j = 0; j < kPlateBlock; ++j) {
      o << "    {\n";
      for (int c : cs) o << "      const float dc" << c << " = r" << c << "_" << j << ";\n";
      o << body.str() << "    }\n";
    }
    o << "  }\n  for (; d" << Q << " < pd.n_rows; ++d" << Q << ") {\n    {\n";
    for (int c : cs) o << "      const float dc" << c << " = pc" << Q << "_" << c << "[d" << Q << "];\n";
    o << body.str() << "    }\n  }\n";
    o << "  ll = ll + (float)pacc" << Q << ";\n";
  }

  // `v` outside the OPEN support of a latent of family `dist` (a NaN included) has log-density -inf, whatever the density
  // formula gives there: the test that guards `lp`, or "" for a Normal.
  static std::string in_support(int dist, const std::string& v) {
    return dist == GJX_DIST_GAMMA ? "(" + v + " > 0.0f)" : dist == GJX_DIST_BETA ? "(" + v + " > 0.0f && " + v + " < 1.0f)" : "";
  }
  // Site q of tm_assess, by emitter `e` (over `o` and the shadow table `tab`): a plated site's loop, an observed site's term
  // into ll, a latent's into lp.
  void emit_site(SiteEmitter<CSiteT, CArgT>& e, int q, const CSiteT* tab) {
    if (sites[q].observed == GJX_SITE_PLATED) {
      emit_plated(q, tab);
      return;
    }
    e.head(q);
    if (sites[q].observed) {
      o << "  ll = ll + " << e.lp_of(q) << ";\n";
      return;
    }
    const std::string in = in_support(sites[q].dist, e.nm("vf", q));
    if (in.empty()) o << "  lp = lp + " << e.lp_of(q) << ";\n";
    else o << "  lp = lp + (" << in << " ? " << e.lp_of(q) << " : -__builtin_inff());\n";
  }

  std::string run() {
    const std::string I = std::to_string(impl);
    emit_prelude(o);
    const TemperTable<CSiteT, CArgT> t(sites, n_sites);
    const int L = t.L;
    const bool plated = !t.plated.empty();
    o << "__device__ __forceinline__ void tm_assess(const RunCols& cols, const PlanParams& prm, const PlanTables& tabs, uint32_t li"
      << t.list(", float nx_") << ", float& lp_out, float& ll_out" << (plated ? ", const PlateData& pd" : "") << ") {\n";
    o << "  (void)cols; (void)prm; (void)tabs; (void)li;\n  float lp = 0.0f, ll = 0.0f;\n";
    SiteEmitter<CSiteT, CArgT> e{o, impl, 0, t.tab.data(), n_sites, "  ", ""};
    e.exact_cuts = false;
    for (int q = 0; q < n_sites; ++q) emit_site(e, q, t.tab.data());
    o << "  lp_out = lp; ll_out = ll;\n}\n";
    if (cov) o << "typedef const __attribute__((address_space(4))) float* FactorPtr;\n";
    o << "extern \"C\" __global__ __launch_bounds__(256) void " << (cov ? "gjx_temper_move_cov_kernel" : "gjx_temper_move_kernel")
      << "(TemperArgs a, RunCols cols, PlanParams prm, PlanTables tabs" << (cov ? ", const float* factor" : "")
      << (plated ? ", PlateData pd" : "") << ") {\n";
    o << "  const uint32_t n = a.n;\n";
    if (cov) o << "  FactorPtr F = (FactorPtr)factor;\n";
    o << "  for (uint64_t i64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < n; i64 += (uint64_t)gridDim.x * blockDim.x) {\n";
    o << "    const uint32_t i = (uint32_t)i64;\n";
    o << "    uint32_t an = a.anc ? (uint32_t)a.anc[i] : i;\n    an = an < n ? an : n - 1u;\n";
    for (int l = 0; l < L; ++l) o << "    float x" << l << " = a.x_in[" << l << "][an];\n";
    o << "    float lp, ll;\n";
    o << "    if (a.recompute) tm_assess(cols, prm, tabs, i" << t.list(", x") << ", lp, ll" << (plated ? ", pd" : "") << ");\n";
    o << "    else { lp = a.lp_in[an]; ll = a.ll_in[an]; }\n";
    o << "    int32_t acc = 0;\n";
    o << "    for (uint32_t r = 0; r < a.n_moves; ++r) {\n";
    o << "      const Key kr = fold_in<" << I << ">(a.key, r);\n";
    o << "      const Key pk = split_at<" << I << ">(fold_in<" << I << ">(kr, 0u), (uint64_t)i);\n";
    o << "      const Key ak = split_at<" << I << ">(fold_in<" << I << ">(kr, 1u), (uint64_t)i);\n";
    // the covariance move: the L draws first (+0 + z: what gjx_sample_logpdf_normal returns at loc 0, scale 1), then row l of
    // the packed triangle against them, every product and sum rounded once.  F is wave-uniform and read through the scalar
    // cache; the empty asm makes the pointer a value of THIS sweep, so the L (L + 1) / 2 loads are not hoisted out of the
    // sweep loop into scalar registers they would not fit next to the key and the pointers.
    if (cov) o << "      asm volatile(\"\" : \"+s\"(F));\n";
    for (int l = 0; cov && l < L; ++l) {
      const uint32_t fold = impl == 0 ? (uint32_t)(l + 1) : (uint32_t)l;
      o << "      const float e" << l << " = 0.0f + site_normal<" << I << ">(Stream<" << I << ">(pk, true, " << fold << "u));\n";
    }
    for (int l = 0; cov && l < L; ++l) {
      o << "      float t" << l << " = F[" << l * (l + 1) / 2 << "] * e0;\n";
      for (int j = 1; j <= l; ++j) o << "      t" << l << " = t" << l << " + F[" << l * (l + 1) / 2 + j << "] * e" << j << ";\n";
      o << "      const float y" << l << " = x" << l << " + t" << l << ";\n";
    }
    for (int l = 0; !cov && l < L; ++l) {
      const uint32_t fold = impl == 0 ? (uint32_t)(l + 1) : (uint32_t)l;  // (SiteEmitter::fold_of for a table of L latents)
      o << "      const float t" << l << " = a.scales[" << l << "] * site_normal<" << I << ">(Stream<" << I << ">(pk, true, " << fold << "u));\n";
      o << "      const float y" << l << " = x" << l << " + t" << l << ";\n";
    }
    o << "      float lpn, lln;\n      tm_assess(cols, prm, tabs, i" << t.list(", y") << ", lpn, lln" << (plated ? ", pd" : "") << ");\n";
    o << "      const float bh = a.beta * ll;\n      const float h = lp + bh;\n";
    o << "      const float bn = a.beta * lln;\n      const float hn = lpn + bn;\n";
    o << "      const float d = hn - h;\n";
    o << "      const float lg = m_log(uniform01(Stream<" << I << ">(ak, false, 0u).bits32(0u)));\n";
    o << "      if (d >= 0.0f || lg < d) {";
    for (int l = 0; l < L; ++l) o << " x" << l << " = y" << l << ";";
    o << " lp = lpn; ll = lln; ++acc; }\n";
    o << "    }\n";
    for (int l = 0; l < L; ++l) o << "    a.x_out[" << l << "][i] = x" << l << ";\n";
    o << "    a.lp_out[i] = lp;\n    a.ll_out[i] = ll;\n    if (a.n_accept) a.n_accept[i] = acc;\n";
    o << "  }\n}\n";
    return o.str();
  }
};

// The move kernel of a tempered plan with GROUPED latents (include/gjx_group.h): GenTemper's kernel with a [G][n] column per
// grouped site next to the scalars in registers.  One lane per particle, no LDS, no barrier.
//   tm_flat    tm_assess over the FLAT sites (GenTemper::emit_site): the scalar latents' terms and every observed or plated
//              site that reads no grouped value.
//   gz_lp      the f32 sum over the grouped sites of the log-density at the group's values gz_<s> (arguments of the function;
//              SiteEmitter names a GROUP operand so), -inf outside the open support.
//   gm_term    one data row: the group-reading plated sites' f32 log-densities into a float64 accumulator, in table order.
//   gm_rows1 / gm_rows2   the rows lo .. hi - 1 of one group, at the group's values (and, gm_rows2, at the proposal's in the same
//              pass: the two evaluations share the row's data registers).  The loop of GenTemper::emit_plated: the bounds are
//              wave-uniform (read from the offsets through a constant-address-space pointer and clamped to n_rows), so the
//              row reads are scalar loads issued for a block of kPlateBlock rows, then a remainder loop.
//   gm_assess  LZ and A of the specification: the loop over the groups at the lane's own entries of z_out (coalesced loads).
//   gi_draw    init: the grouped sites as the LATENT sites of a table of their own (SiteEmitter's draws, numbered among
//              themselves) under the key split_at(fold_in(init_key, g), i).
// The key folds of a group (fold_in(fold_in(k_r, 2), g) and its two children) are wave-uniform: scalar-side cipher blocks.
// The grouped columns, offsets and scales are one more kernel argument (GroupArgs), of grouped plans only.
template <class CSiteT, class CArgT>
struct GenTemperGrouped {
  std::ostringstream o;
  int impl;
  const CSiteT* sites;
  int n_sites;

  std::string run() {
    using Table = TemperTable<CSiteT, CArgT>;
    using Emitter = SiteEmitter<CSiteT, CArgT>;
    constexpr int NB = GenTemper<CSiteT, CArgT>::kPlateBlock;
    const std::string I = std::to_string(impl);
    emit_prelude(o);
    const Table t(sites, n_sites);
    const int L = t.L, S = (int)t.grouped.size();
    bool gread[GJX_MAX_SITES] = {}, flat[GJX_MAX_SITES] = {}, used[GJX_PLATE_MAX_COLS] = {};
    for (int q = 0; q < n_sites; ++q) {
      gread[q] = sites[q].observed == GJX_SITE_PLATED && Table::reads_group(sites[q]);
      flat[q] = !gread[q] && sites[q].observed != GJX_SITE_GROUPED;
      if (gread[q])
        for (int c : Table::plate_cols(sites[q])) used[c] = true;
    }
    const std::vector<int> gcs = Table::set_of(used);  // the data columns the group-reading sites read
    auto zl = [&](const std::string& pre, const std::string& post = "") {  // pre0post ... pre<S-1>post
      std::string r;
      for (int s = 0; s < S; ++s) r += pre + std::to_string(s) + post;
      return r;
    };
    auto dl = [&](const std::string& pre, const std::string& post = "") {
      std::string r;
      for (int c : gcs) r += pre + std::to_string(c) + post;
      return r;
    };
    const std::string head = "(const PlanParams& prm, const PlanTables& tabs", nxs = t.list(", float nx_"), gzs = zl(", float gz_");
    auto latent_heads = [&](Emitter& e) {  // the scalar latents' values vf<q> = nx_<l>: what a later site's argument may name
      for (int q = 0; q < n_sites; ++q)
        if (sites[q].observed == 0) e.head(q);
    };

    // -- tm_flat ---------------------------------------------------------------------------------------------------------------
    {
      GenTemper<CSiteT, CArgT> g;
      g.impl = impl; g.sites = sites; g.n_sites = n_sites;
      Emitter e{g.o, impl, 0, t.tab.data(), n_sites, "  ", ""};
      e.exact_cuts = false;
      o << "__device__ __forceinline__ void tm_flat(const RunCols& cols, const PlanParams& prm, const PlanTables& tabs, uint32_t li" << nxs
        << ", float& lp_out, float& ll_out, const PlateData& pd) {\n";
      o << "  (void)cols; (void)prm; (void)tabs; (void)li; (void)pd;\n  float lp = 0.0f, ll = 0.0f;\n";
      for (int q = 0; q < n_sites; ++q)
        if (flat[q]) g.emit_site(e, q, t.tab.data());
      o << g.o.str() << "  lp_out = lp; ll_out = ll;\n}\n";
    }
    // -- gz_lp -----------------------------------------------------------------------------------------------------------------
    {
      Emitter e{o, impl, 0, t.tab.data(), n_sites, "  ", ""};
      e.exact_cuts = false;
      o << "__device__ __forceinline__ float gz_lp" << head << nxs << gzs << ") {\n  (void)prm; (void)tabs;\n";
      latent_heads(e);
      o << "  float lp = 0.0f;\n";
      for (int q : t.grouped) {
        e.head(q);
        const std::string in = GenTemper<CSiteT, CArgT>::in_support(sites[q].dist, e.nm("vf", q));
        if (in.empty()) o << "  lp = lp + " << e.lp_of(q) << ";\n";
        else o << "  lp = lp + (" << in << " ? " << e.lp_of(q) << " : -__builtin_inff());\n";
      }
      o << "  return lp;\n}\n";
    }
    // -- gm_term ---------------------------------------------------------------------------------------------------------------
    {
      Emitter e{o, impl, 0, t.tab.data(), n_sites, "  ", ""};
      e.exact_cuts = false;
      o << "__device__ __forceinline__ void gm_term" << head << nxs << gzs << dl(", float dc") << ", double& acc) {\n  (void)prm; (void)tabs;\n";
      latent_heads(e);
      for (int q = 0; q < n_sites; ++q) {
        if (!gread[q]) continue;
        e.head(q);
        o << "  acc = acc + (double)(" << e.lp_of(q) << ");\n";
      }
      o << "}\n";
    }
    // -- gm_rows1, gm_rows2 ------------------------------------------------------------------------------------------------------
    for (int two = 0; two < 2; ++two) {
      o << "__device__ __forceinline__ void gm_rows" << (two ? 2 : 1) << head << ", const PlateData& pd, uint32_t lo, uint32_t hi" << nxs << gzs
        << (two ? zl(", float gy_") : "") << ", double& acc" << (two ? ", double& accn" : "") << ") {\n";
      for (int c : gcs) o << "  const PlateCol pc" << c << " = (PlateCol)pd.col[" << c << "];\n";
      auto row = [&](const std::string& ind, const std::string& dcs) {
        o << ind << "gm_term(prm, tabs" << t.list(", nx_") << zl(", gz_") << dcs << ", acc);\n";
        if (two) o << ind << "gm_term(prm, tabs" << t.list(", nx_") << zl(", gy_") << dcs << ", accn);\n";
      };
      o << "  uint32_t d = lo;\n  for (; d + " << NB << "u <= hi; d += " << NB << "u) {\n";
      for (int c : gcs)
        for (int j = 0; j < NB; ++j) o << "    const float r" << c << "_" << j << " = pc" << c << "[d + " << j << "u];\n";
      for (int j = 0; j < NB; ++j) row("    ", dl(", r", "_" + std::to_string(j)));
      o << "  }\n  for (; d < hi; ++d) {\n";
      for (int c : gcs) o << "    const float r" << c << " = pc" << c << "[d];\n";
      row("    ", dl(", r"));
      o << "  }\n}\n";
    }
    // -- gm_assess ---------------------------------------------------------------------------------------------------------------
    auto bounds = [](const std::string& ind) {  // the rows of group g, each bound clamped to n_rows
      return ind + "uint32_t lo = (uint32_t)off[g], hi = (uint32_t)off[g + 1u];\n" + ind + "lo = lo < pd.n_rows ? lo : pd.n_rows;\n" + ind +
             "hi = hi < pd.n_rows ? hi : pd.n_rows;\n";
    };
    o << "__device__ __forceinline__ void gm_assess" << head << ", const PlateData& pd, const GroupArgs& ga, GroupOff off, uint32_t n, uint32_t i" << nxs
      << ", double& lz_out, double& a_out) {\n  double LZ = 0.0, A = 0.0;\n  for (uint32_t g = 0; g < ga.G; ++g) {\n" << bounds("    ");
    for (int s = 0; s < S; ++s) o << "    const float z" << s << " = ga.z_out[" << s << "][(size_t)g * n + i];\n";
    o << "    LZ = LZ + (double)gz_lp(prm, tabs" << t.list(", nx_") << zl(", z") << ");\n";
    o << "    double acc = 0.0;\n    gm_rows1(prm, tabs, pd, lo, hi" << t.list(", nx_") << zl(", z") << ", acc);\n    A = A + acc;\n  }\n";
    o << "  lz_out = LZ; a_out = A;\n}\n";
    // -- gi_draw -----------------------------------------------------------------------------------------------------------------
    {
      std::vector<CSiteT> drawn(t.tab);
      ScopeInfo si;
      si.n_scopes = 0;
      si.parent[0] = -1;
      for (int q = 0, s = 0; q < n_sites; ++q) {
        si.site_scope[q] = 0;
        si.fold_t[q] = (uint32_t)s + 1u;
        si.fold_p[q] = (uint32_t)s;
        if (s < S && t.grouped[s] == q) {
          drawn[q].observed = 0;
          ++s;
        }
      }
      Emitter e{o, impl, 0, drawn.data(), n_sites, "  ", ""};
      e.exact_cuts = false; e.store_values = false; e.defer_acc = true; e.sc = &si;
      o << "__device__ __forceinline__ void gi_draw" << head << ", Key pkey" << nxs << ", float (&zv)[" << S << "]) {\n  (void)prm; (void)tabs; (void)pkey;\n";
      latent_heads(e);
      for (int s = 0; s < S; ++s) {
        e.head(t.grouped[s]);
        e.tail(t.grouped[s]);
        o << "  zv[" << s << "] = " << e.nm("vf", t.grouped[s]) << ";\n";
      }
      o << "}\n";
    }
    // -- the kernel ----------------------------------------------------------------------------------------------------------------
    o << "extern \"C\" __global__ __launch_bounds__(256) void gjx_temper_move_grouped_kernel(TemperArgs a, RunCols cols, PlanParams prm, "
         "PlanTables tabs, PlateData pd, GroupArgs ga) {\n";
    o << "  const uint32_t n = a.n;\n  const GroupOff off = (GroupOff)ga.off;\n";
    for (int s = 0; s < S; ++s) o << "  const PlateCol zs" << s << " = (PlateCol)ga.z_scales[" << s << "];\n";
    o << "  for (uint64_t i64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < n; i64 += (uint64_t)gridDim.x * blockDim.x) {\n";
    o << "    const uint32_t i = (uint32_t)i64;\n";
    o << "    uint32_t an = a.anc ? (uint32_t)a.anc[i] : i;\n    an = an < n ? an : n - 1u;\n";
    for (int l = 0; l < L; ++l) o << "    float x" << l << " = a.x_in[" << l << "][an];\n";
    o << "    if (ga.init) {\n      for (uint32_t g = 0; g < ga.G; ++g) {\n";
    o << "        float zv[" << S << "];\n        gi_draw(prm, tabs, split_at<" << I << ">(fold_in<" << I << ">(ga.init_key, g), (uint64_t)i)" << t.list(", x") << ", zv);\n";
    for (int s = 0; s < S; ++s) o << "        ga.z_out[" << s << "][(size_t)g * n + i] = zv[" << s << "];\n";
    o << "      }\n    } else {\n      for (uint32_t g = 0; g < ga.G; ++g) {\n";
    for (int s = 0; s < S; ++s) o << "        ga.z_out[" << s << "][(size_t)g * n + i] = ga.z_in[" << s << "][(size_t)g * n + an];\n";
    o << "      }\n    }\n";
    o << "    float lp, ll, lpf = 0.0f, llf = 0.0f;\n";
    o << "    if (a.recompute || a.n_moves) tm_flat(cols, prm, tabs, i" << t.list(", x") << ", lpf, llf, pd);\n";
    o << "    if (a.recompute) {\n      double LZ, A;\n      gm_assess(prm, tabs, pd, ga, off, n, i" << t.list(", x") << ", LZ, A);\n";
    o << "      lp = lpf + (float)LZ; ll = llf + (float)A;\n    } else { lp = a.lp_in[an]; ll = a.ll_in[an]; }\n";
    o << "    int32_t acc = 0, accz = 0;\n";
    o << "    for (uint32_t r = 0; r < a.n_moves; ++r) {\n";
    o << "      const Key kr = fold_in<" << I << ">(a.key, r);\n";
    o << "      const Key pk = split_at<" << I << ">(fold_in<" << I << ">(kr, 0u), (uint64_t)i);\n";
    o << "      const Key ak = split_at<" << I << ">(fold_in<" << I << ">(kr, 1u), (uint64_t)i);\n";
    for (int l = 0; l < L; ++l) {
      const uint32_t fold = impl == 0 ? (uint32_t)(l + 1) : (uint32_t)l;
      o << "      const float t" << l << " = a.scales[" << l << "] * site_normal<" << I << ">(Stream<" << I << ">(pk, true, " << fold << "u));\n";
      o << "      const float y" << l << " = x" << l << " + t" << l << ";\n";
    }
    o << "      {\n        float lpfn, llfn;\n        tm_flat(cols, prm, tabs, i" << t.list(", y") << ", lpfn, llfn, pd);\n";
    o << "        double LZn, An;\n        gm_assess(prm, tabs, pd, ga, off, n, i" << t.list(", y") << ", LZn, An);\n";
    o << "        const float lpn = lpfn + (float)LZn;\n        const float lln = llfn + (float)An;\n";
    o << "        const float bh = a.beta * ll;\n        const float h = lp + bh;\n";
    o << "        const float bn = a.beta * lln;\n        const float hn = lpn + bn;\n";
    o << "        const float d = hn - h;\n";
    o << "        const float lg = m_log(uniform01(Stream<" << I << ">(ak, false, 0u).bits32(0u)));\n";
    o << "        if (d >= 0.0f || lg < d) {";
    for (int l = 0; l < L; ++l) o << " x" << l << " = y" << l << ";";
    o << " lp = lpn; ll = lln; lpf = lpfn; llf = llfn; ++acc; }\n      }\n";
    // the group phase: Metropolis within Gibbs, one group at a time, against the group's own rows
    o << "      const Key kz = fold_in<" << I << ">(kr, 2u);\n      double LZ = 0.0, A = 0.0;\n";
    o << "      for (uint32_t g = 0; g < ga.G; ++g) {\n";
    o << "        const Key kg = fold_in<" << I << ">(kz, g);\n";
    o << "        const Key gpk = split_at<" << I << ">(fold_in<" << I << ">(kg, 0u), (uint64_t)i);\n";
    o << "        const Key gak = split_at<" << I << ">(fold_in<" << I << ">(kg, 1u), (uint64_t)i);\n";
    o << bounds("        ");
    o << "        const size_t zi = (size_t)g * n + i;\n";
    for (int s = 0; s < S; ++s) {
      const uint32_t fold = impl == 0 ? (uint32_t)(s + 1) : (uint32_t)s;
      o << "        const float zc" << s << " = ga.z_out[" << s << "][zi];\n";
      o << "        const float zw" << s << " = zs" << s << "[g] * site_normal<" << I << ">(Stream<" << I << ">(gpk, true, " << fold << "u));\n";
      o << "        const float zy" << s << " = zc" << s << " + zw" << s << ";\n";
    }
    o << "        const float lz = gz_lp(prm, tabs" << t.list(", x") << zl(", zc") << ");\n";
    o << "        const float lzn = gz_lp(prm, tabs" << t.list(", x") << zl(", zy") << ");\n";
    o << "        double ac = 0.0, acn = 0.0;\n";
    o << "        gm_rows2(prm, tabs, pd, lo, hi" << t.list(", x") << zl(", zc") << zl(", zy") << ", ac, acn);\n";
    o << "        const float dz = lzn - lz;\n        const float da = (float)(acn - ac);\n        const float bd = a.beta * da;\n";
    o << "        const float d = dz + bd;\n";
    o << "        const float lg = m_log(uniform01(Stream<" << I << ">(gak, false, 0u).bits32(0u)));\n";
    o << "        const bool ok = d >= 0.0f || lg < d;\n        if (ok) {";
    for (int s = 0; s < S; ++s) o << " ga.z_out[" << s << "][zi] = zy" << s << ";";
    o << " ++accz; }\n";
    o << "        LZ = LZ + (double)(ok ? lzn : lz);\n        A = A + (ok ? acn : ac);\n      }\n";
    o << "      lp = lpf + (float)LZ;\n      ll = llf + (float)A;\n    }\n";
    for (int l = 0; l < L; ++l) o << "    a.x_out[" << l << "][i] = x" << l << ";\n";
    o << "    a.lp_out[i] = lp;\n    a.ll_out[i] = ll;\n    if (a.n_accept) a.n_accept[i] = acc;\n    if (ga.n_accept_z) ga.n_accept_z[i] = accz;\n";
    o << "  }\n}\n";
    return o.str();
  }
};

// The GROUPED mode of the three check generators (include/gjx_group_checks.h), taken exactly when the table holds a grouped
// site — the text of a table without one is what it was before the mode existed, byte for byte.  The row term also depends
// on z[s][g(d)][i]: the kernels are named gjx_*_grouped_kernel and take one more argument (GroupCols gc), the term functions
// take gz_<s> (SiteEmitter's name of a GROUP operand) between the latents and the data values, and g(d) is found once per
// row by group_of_row (gjx_device.hpp), before the particle loop.  What differs per kernel is the orientation of the z loads:
//   pointwise   a lane is a row: per block of kPointwiseBlock particles four dword loads of z[s][g(d) * n + i ..] per grouped
//               site (4-byte alignment is all n guarantees); the lanes of a group read one address — rows are sorted by group;
//   PSIS        a lane is a particle, the workgroup's four rows are wave-uniform: their groups are found on the scalar side
//               and lane i reads z[s][g(row) * n + i], coalesced, once per round;
//   predictive  a lane owns two rows: gA and gB once, pd_particle takes gz_<s>A and gz_<s>B; the samplers are untouched.
// No LDS beyond the PSIS histogram, no barrier added, no scratch; the source holds neither G nor n.

// The pointwise kernel of a plated tempered plan (include/gjx_pointwise.h): the TRANSPOSED loop of emit_plated.  The move
// kernel puts particles on lanes and reads data rows through the scalar cache; the reduction here runs over the particles,
// so lanes are ROWS and particles are wave-uniform:
//   * a workgroup owns a tile of 256 rows (blockIdx.x) and one chunk of particles (blockIdx.y); a lane loads its row of the
//     data columns the plated sites read ONCE, into registers (dc<c>, the names SiteEmitter gives a DATA operand);
//   * the chunk's particles are walked by emit_particle_loop in blocks of kPointwiseBlock;
//   * pw_term is tm_assess without the sums it does not need, over the same TemperTable: the unplated sites' heads define the
//     values a plated site may refer to (a latent's is the function argument nx_<l>), the plated sites' log-densities add up
//     in f32 in table order;
//   * the accumulators and the stores are fixed device code (gjx_device.hpp pointwise_take / pointwise_store).
// Lanes at or past n_rows leave at once and store nothing.  No LDS, no barrier, no draw: one source per plan, whatever impl.
// The source holds no data value, no parameter value and neither n nor n_rows.  (A table that reads a per-particle input
// column has no pointwise source: the entry points refuse it before this runs.)
// pw_term(prm, tabs, nx_<l>..., dc<c>...): the entry t[d, i] of include/gjx_pointwise.h as a device function of a particle's
// latents and a row's data values — what GenPointwise and GenPsis (under `name`) reduce in their two orientations.
template <class CSiteT, class CArgT>
inline void emit_row_term(std::ostringstream& o, const TemperTable<CSiteT, CArgT>& t, const CSiteT* sites, int n_sites, const char* name = "pw_term") {
  o << "__device__ __forceinline__ float " << name << "(const PlanParams& prm, const PlanTables& tabs" << t.list(", float nx_")
    << t.group_list(", float gz_", {""}) << t.data_list(", float dc", {""}) << ") {\n";
  o << "  (void)prm; (void)tabs;\n";
  SiteEmitter<CSiteT, CArgT> e{o, 0, 0, t.tab.data(), n_sites, "  ", ""};
  e.exact_cuts = false;
  bool first = true;
  for (int q = 0; q < n_sites; ++q) {
    e.head(q);
    if (sites[q].observed != GJX_SITE_PLATED) continue;
    // (the sum starts at the first term: +0 + t differs from t in the sign of a zero only, which no output can tell)
    o << (first ? "  float t = " : "  t = t + ") << e.lp_of(q) << ";\n";
    first = false;
  }
  o << "  return t;\n}\n";
}

template <class CSiteT, class CArgT>
struct GenPointwise {
  std::ostringstream o;
  const CSiteT* sites;
  int n_sites;

  std::string run() {
    constexpr int NB = gjx::kPointwiseBlock;
    emit_prelude(o);
    const TemperTable<CSiteT, CArgT> t(sites, n_sites);
    const int S = (int)t.grouped.size();  // the grouped mode (see above): nothing below emits a character without it
    const std::string dcs = t.data_list(", dc", {""});
    emit_row_term(o, t, sites, n_sites);
    o << "extern \"C\" __global__ __launch_bounds__(256) void " << (S ? "gjx_pointwise_grouped_kernel" : "gjx_pointwise_kernel")
      << "(PointwiseArgs a, PlanParams prm, PlanTables tabs, PlateData pd" << (S ? ", GroupCols gc" : "") << ") {\n";
    o << "  const uint32_t d = blockIdx.x * 256u + threadIdx.x;\n  if (d >= pd.n_rows) return;\n";
    for (int c : t.cs) o << "  const float dc" << c << " = pd.col[" << c << "][d];\n";
    if (S) o << "  const size_t zb = (size_t)group_of_row((GroupOff)gc.off, gc.G, d) * a.n;  // (row g(d) of the [G][n] columns)\n";
    for (int s = 0; s < S; ++s) o << "  const float* zp" << s << " = gc.z[" << s << "] + zb;\n";
    std::string block;
    for (int s = 0; s < S; ++s)  // (four dword loads: g(d) * n + i is 4-byte aligned and no more)
      for (int j = 0; j < NB; ++j)
        block += "    const float gz" + std::to_string(s) + "_" + std::to_string(j) + " = zp" + std::to_string(s) + "[(size_t)i + " + std::to_string(j) + "u];\n";
    block += "    const float t[" + std::to_string(NB) + "] = {";
    for (int j = 0; j < NB; ++j)
      block += std::string(j ? ", " : "") + "pw_term(prm, tabs" + t.list(", x", "_" + std::to_string(j)) + t.group_list(", gz", {("_" + std::to_string(j)).c_str()}) + dcs + ")";
    block += "};\n    pointwise_take<" + std::to_string(NB) + ">(q, t);\n";
    std::string zrest;
    for (int s = 0; s < S; ++s) zrest += ", zp" + std::to_string(s) + "[i]";
    emit_particle_loop(o, t, NB, "  PointwiseAcc q = pointwise_start();\n", block,
                       " {\n    const float t[1] = {pw_term(prm, tabs" + t.list(", xc", "[i]") + zrest + dcs + ")};\n    pointwise_take<1>(q, t);\n  }\n",
                       "  pointwise_store(a, pd.n_rows, blockIdx.y, d, q);\n}\n");
    return o.str();
  }
};

// The PSIS kernel of a plated tempered plan (include/gjx_psis.h): the orientation of emit_plated, not of emit_particle_loop —
// PARTICLES on lanes, rows wave-uniform:
//   * a workgroup owns a block of kPsisRows rows (blockIdx.x) and one contiguous chunk of particles (blockIdx.y); the rows'
//     data values are read through constant-address-space pointers at indices derived from blockIdx (scalar loads, once); a
//     row past the last one reads the last row's data again and is switched off (`on`);
//   * a lane loads a particle's latents once per round of 256 particles and evaluates the kPsisRows terms with ps_term — the
//     pointwise kernel's pw_term, emitted by the same function, so t[d, i] is the same f32 in both;
//   * what happens to a term depends on a.mode (the three select passes, the collect pass) and is fixed device code
//     (gjx_device.hpp psis_begin / psis_take / psis_flush), as are the launches between the passes.
// The loop's trip count is uniform over the workgroup (a lane past the chunk's end reads the chunk's last particle and is
// switched off), so the barriers of psis_begin and psis_flush are reached by every lane.  32 KB of LDS;
// no draw: one source per plan, whatever impl.  The source holds no data value, no parameter value and neither n, n_rows
// nor tail_len.
template <class CSiteT, class CArgT>
struct GenPsis {
  std::ostringstream o;
  const CSiteT* sites;
  int n_sites;

  std::string run() {
    constexpr int R = gjx::kPsisRows;
    emit_prelude(o);
    const TemperTable<CSiteT, CArgT> t(sites, n_sites);
    emit_row_term(o, t, sites, n_sites, "ps_term");
    const int S = (int)t.grouped.size();  // the grouped mode
    o << "extern \"C\" __global__ __launch_bounds__(256) void " << (S ? "gjx_psis_grouped_kernel" : "gjx_psis_kernel")
      << "(PsisArgs a, PlanParams prm, PlanTables tabs, PlateData pd" << (S ? ", GroupCols gc" : "") << ") {\n";
    o << "  __shared__ double shd[kPsisRows * kPsisBins / 2];\n  uint32_t* sh = reinterpret_cast<uint32_t*>(shd);\n";
    o << "  const uint32_t r0 = blockIdx.x * (uint32_t)kPsisRows;\n";
    for (int c : t.cs) o << "  const PlateCol pc" << c << " = (PlateCol)pd.col[" << c << "];\n";
    for (int j = 0; j < R; ++j) {
      const std::string J = std::to_string(j);
      o << "  const bool on" << J << " = r0 + " << J << "u < pd.n_rows;\n";
      o << "  const uint32_t d" << J << " = on" << J << " ? r0 + " << J << "u : pd.n_rows - 1u;\n";
      for (int c : t.cs) o << "  const float dc" << c << "_" << J << " = pc" << c << "[d" << J << "];\n";
      o << "  const uint32_t key" << J << " = psis_row_key(a, d" << J << ");\n  const float tT" << J << " = psis_unkey(key" << J << ");\n";
      // (d<J> is wave-uniform: the search runs on the scalar side)
      if (S) o << "  const size_t zb" << J << " = (size_t)group_of_row((GroupOff)gc.off, gc.G, d" << J << ") * a.n;\n";
    }
    o << "  double g[kPsisRows] = {};\n  uint32_t bad[kPsisRows] = {};\n";
    o << "  const uint64_t lo64 = (uint64_t)blockIdx.y * a.per;\n";
    o << "  const uint32_t lo = lo64 < a.n ? (uint32_t)lo64 : a.n;\n";
    o << "  const uint32_t hi = a.n - lo > a.per ? lo + a.per : a.n;\n";
    o << "  psis_begin(a, sh);\n";
    o << "  for (uint32_t i0 = lo; i0 < hi; i0 += 256u) {\n";
    o << "    const bool live = hi - i0 > threadIdx.x;\n    const uint32_t i = live ? i0 + threadIdx.x : hi - 1u;\n";
    for (int l = 0; l < t.L; ++l) o << "    const float x" << l << " = a.x[" << l << "][i];\n";
    for (int s = 0; s < S; ++s)
      for (int j = 0; j < R; ++j) o << "    const float gz" << s << "_" << j << " = gc.z[" << s << "][zb" << j << " + i];\n";
    for (int j = 0; j < R; ++j) {
      const std::string J = std::to_string(j);
      o << "    psis_take(a, sh + " << J << " * kPsisBins, d" << J << ", key" << J << ", tT" << J << ", live && on" << J << ", ps_term(prm, tabs"
        << t.list(", x") << t.group_list(", gz", {("_" + J).c_str()}) << t.data_list(", dc", {("_" + J).c_str()}) << "), g[" << J << "], bad[" << J << "]);\n";
    }
    o << "  }\n  psis_flush(a, sh, pd.n_rows, r0, g, bad);\n}\n";
    return o.str();
  }
};

// The predictive kernel of a plated tempered plan (include/gjx_predictive.h): the transposed loop of emit_particle_loop — rows
// on lanes, the particles of a chunk wave-uniform — with a DRAW where the pointwise kernel has a density.  The header defines the draws
// as an importance pass over the data rows, so the sites are emitted by the importance kernel's own emitters:
//   * a lane owns the rows dA = 2 r and dA + 1 — the "particles" A and B of a LaneGroup.  Under PHILOX the plated sites go
//     through emit_pair_lane_sites (pair r of the pass: one cipher block per two single-word draws of both rows, one
//     Box-Muller transform per Normal site, the gammas of both rows drawn together); under THREEFRY through the two
//     emitters' head() / tail(), the one-particle form twice.  No sampler is written here;
//   * the pass's parent key fold_in(a.key, i) is wave-uniform, the rows' keys are its lazy children d (split_at);
//   * the table walked is the `drawn` TemperTable: the plated sites as LATENT ones (their draws), every other site only
//     defines the value a plated site may refer to (a latent's is the argument nx_<l>), emitted here by head() and skipped by
//     the pair emitter.  The draws are numbered by TemperTable::draw_numbering, handed to the emitters as their ScopeInfo;
//   * a lane loads its two rows of the data columns once (dc<c>A, dc<c>B: SiteEmitter's names under the suffixes).  With an
//     odd row count the last lane has row A only: B reads row A's data again, is summed into accumulators nobody stores and
//     is never stored itself;
//   * accumulators, the stored subset and the stores are fixed device code (gjx_device.hpp predictive_*).
// Lanes past the last row leave at once.  No LDS (the Box-Muller tables are read from the constant arrays), no barrier, no
// inline assembly in the generated text.  The source holds no data value, no parameter value and neither n nor n_rows.
template <class CSiteT, class CArgT>
struct GenPredictive {
  std::ostringstream o;
  int impl;
  const CSiteT* sites;
  int n_sites;

  std::string run() {
    using Emitter = SiteEmitter<CSiteT, CArgT>;
    constexpr int NB = gjx::kPredictiveBlock;
    const std::string I = std::to_string(impl);
    emit_prelude(o);
    const TemperTable<CSiteT, CArgT> t(sites, n_sites, true);
    const std::vector<int>& plated = t.plated;
    const ScopeInfo si = t.draw_numbering();
    bool skip[GJX_MAX_SITES] = {};  // the sites that draw nothing: emitted here by head(), skipped by the pair emitter
    for (int q = 0; q < n_sites; ++q) skip[q] = t.tab[q].observed != 0;
    const int S = (int)plated.size();
    const int Z = (int)t.grouped.size();  // the grouped mode
    const std::string SS = std::to_string(S), dcs = t.data_list(", dc", {"A", "B"});
    // particle i at the lane's two rows: the draws of every plated site, into the accumulators and (every stride-th) the table
    o << "__device__ __forceinline__ void pd_particle(const PredictiveArgs& a, const PlanParams& prm, const PlanTables& tabs, PredictiveKeep& kp, "
         "uint32_t i, uint32_t n_rows, uint32_t dA, bool hasB" << t.list(", float nx_") << t.group_list(", float gz_", {"A", "B"}) << t.data_list(", float dc", {"A", "B"}) << ", PredictiveAcc (&qA)[" << SS
      << "], PredictiveAcc (&qB)[" << SS << "]) {\n";
    o << "  (void)prm; (void)tabs;\n";
    o << "  const Key pk = predictive_pass_key<" << I << ">(a.key, i);  // (fold_in(a.key, i), wave-uniform: the parent key of this particle's pass over the rows)\n";
    o << "  const Key pkeyA = split_at<" << I << ">(pk, (uint64_t)dA); (void)pkeyA;\n";
    o << "  const Key pkeyB = split_at<" << I << ">(pk, (uint64_t)dA + 1u); (void)pkeyB;\n";
    LaneGroup<CSiteT, CArgT> lanes(o, 2, impl, 0, t.tab.data(), n_sites, "  ");
    lanes.each([&](int, Emitter& e) { e.store_values = false; e.sc = &si; e.ext_bits = impl == 1; e.defer_acc = true; });
    for (int q = 0; q < n_sites; ++q)
      if (skip[q]) lanes.each([&](int, Emitter& e) { e.head(q); });
    if (impl == 1) {
      o << "  const uint32_t pk0 = pk.k0, pk1 = pk.k1; (void)pk0; (void)pk1;\n";
      o << "  const uint64_t pair0 = (uint64_t)(dA >> 1); (void)pair0;\n";
      // (the pair emitter adds a latent site's log-density to the lane's scores: nothing reads them here — dead code)
      o << "  float scA = 0.0f, scB = 0.0f;\n";
      emit_pair_lane_sites(o, lanes, "  ", "", "", "", "", false, skip);
      o << "  (void)scA; (void)scB;\n";
    } else {
      for (int q : plated) {
        lanes.each([&](int, Emitter& e) { e.head(q); });
        lanes.each([&](int, Emitter& e) { e.tail(q); });
      }
    }
    auto values = [&](const Emitter& e) {
      std::string t;
      for (int s = 0; s < S; ++s) t += (s ? ", " : "") + e.val_f32(plated[s]);
      return t;
    };
    // the observed values of gjx_plate.h at the two rows (a Bernoulli site's as 0 / 1), from the ORIGINAL sites' operands
    auto observed = [&](const Emitter& e) {
      std::string t;
      for (int s = 0; s < S; ++s) {
        const CSiteT& st = sites[plated[s]];
        const std::string ov = e.arg(st.obs);
        t += (s ? ", " : "") + (Emitter::is_count(st) ? "__builtin_rintf(" + ov + ")"  // (a count's observed value is rint(data) itself)
                                : Emitter::is_int(st) ? "((int32_t)__builtin_rintf(" + ov + ") != 0 ? 1.0f : 0.0f)" : ov);
      }
      return t;
    };
    lanes.each([&](int, Emitter& e) {
      o << "  const float y" << e.sfx << "[" << SS << "] = {" << values(e) << "};\n";
      o << "  const float ob" << e.sfx << "[" << SS << "] = {" << observed(e) << "};\n";
    });
    o << "#pragma unroll\n  for (int s = 0; s < " << SS << "; ++s) {\n    predictive_take(qA[s], yA[s], obA[s]);\n    predictive_take(qB[s], yB[s], obB[s]);\n  }\n";
    o << "  predictive_keep_rows<" << SS << ">(a, kp, i, n_rows, dA, hasB, yA, yB);\n}\n";

    o << "extern \"C\" __global__ __launch_bounds__(256) void " << (Z ? "gjx_predictive_grouped_kernel" : "gjx_predictive_kernel")
      << "(PredictiveArgs a, PlanParams prm, PlanTables tabs, PlateData pd" << (Z ? ", GroupCols gc" : "") << ") {\n";
    o << "  const uint32_t dA = (blockIdx.x * 256u + threadIdx.x) * 2u;\n  if (dA >= pd.n_rows) return;\n";
    o << "  const bool hasB = dA + 1u < pd.n_rows;\n  const uint32_t dB = hasB ? dA + 1u : dA;  // (an odd row count: row n_rows is never read)\n";
    for (int c : t.cs) o << "  const float dc" << c << "A = pd.col[" << c << "][dA], dc" << c << "B = pd.col[" << c << "][dB];\n";
    // (the groups of the lane's two rows, found once: rows g(dA), g(dB) of the [G][n] columns)
    if (Z) o << "  const size_t zbA = (size_t)group_of_row((GroupOff)gc.off, gc.G, dA) * a.n, zbB = (size_t)group_of_row((GroupOff)gc.off, gc.G, dB) * a.n;\n";
    for (int s = 0; s < Z; ++s) o << "  const float* zp" << s << "A = gc.z[" << s << "] + zbA;\n  const float* zp" << s << "B = gc.z[" << s << "] + zbB;\n";
    auto particle = [&](const std::string& i, const std::string& xs, const std::string& zs) {
      return "pd_particle(a, prm, tabs, kp, " + i + ", pd.n_rows, dA, hasB" + xs + zs + dcs + ", qA, qB);\n";
    };
    auto zat = [&](const std::string& at) {  // zp<s>A[at], zp<s>B[at] for every grouped site
      std::string r;
      for (int s = 0; s < Z; ++s) r += ", zp" + std::to_string(s) + "A[" + at + "], zp" + std::to_string(s) + "B[" + at + "]";
      return r;
    };
    std::string block;
    for (int s = 0; s < Z; ++s)  // (the block's loads before its arithmetic: four dwords per row and grouped site)
      for (int j = 0; j < NB; ++j)
        for (const char* r : {"A", "B"})
          block += "    const float gz" + std::to_string(s) + r + "_" + std::to_string(j) + " = zp" + std::to_string(s) + r + "[(size_t)i + " + std::to_string(j) + "u];\n";
    for (int j = 0; j < NB; ++j) {
      const std::string J = "_" + std::to_string(j);
      block += "    " + particle("i + " + std::to_string(j) + "u", t.list(", x", J), t.group_list(", gz", {("A" + J).c_str(), ("B" + J).c_str()}));
    }
    emit_particle_loop(o, t, NB,
                       "  PredictiveAcc qA[" + SS + "], qB[" + SS + "];\n#pragma unroll\n  for (int s = 0; s < " + SS +
                           "; ++s) qA[s] = qB[s] = predictive_start();\n  PredictiveKeep kp = predictive_keep_start(a, lo);\n",
                       block, " " + particle("i", t.list(", xc", "[i]"), zat("i")),
                       "#pragma unroll\n  for (int s = 0; s < " + SS + "; ++s) {\n    predictive_store(a, pd.n_rows, (uint32_t)s, blockIdx.y, dA, qA[s]);\n"
                       "    if (hasB) predictive_store(a, pd.n_rows, (uint32_t)s, blockIdx.y, dA + 1u, qB[s]);\n  }\n}\n");
    return o.str();
  }
};

// One source generation: the generator numbers the plan's device tables while it runs (TableScope); `tabs` (nullable) takes
// their addresses, in that order — the kernel argument of every launch of the source.
template <class G>
inline std::string generated_source(G& g, gjx::PlanTables* tabs) {
  TableScope ts;
  std::string src = g.run();
  if (tabs) *tabs = ts.reg.tables();
  return src;
}

inline bool enabled() {
  const char* e = std::getenv("GJX_PLAN_JIT");
  return !(e && e[0] == '0');
}

// ---- the compiler runs in a CHILD process (gjx_jitc.cpp) ---------------------------------------------------------------
// hiprtc is the whole AMDGPU backend in-process: a backend crash on generated source would be an abort() of the caller
// (it happened once: a constant-folded NaN log-weight; the generator now keeps such constants opaque, but ANY other
// backend bug would do the same).  So generated kernels are compiled by `gjx_jitc`, a helper next to this library: a fresh
// process that never touches the GPU, started with posix_spawn (a child process — the caller is not replaced), source /
// header / code object / log in files of a private temporary directory.  A child that dies => false + a log line
// (callers return GJX_ERR_JIT).  GJX_JIT_INPROC=1 compiles in-process (the round-1/2 behaviour).  A helper that cannot be
// started is GJX_ERR_JIT too (r04: the silent in-process fallback is opt-in, GJX_JIT_INPROC_FALLBACK=1); gjx_jit_routes
// says which route produced the code objects of this process.
inline std::string jitc_path() {
  static const std::string path = [] {
    if (const char* e = std::getenv("GJX_JITC")) return std::string(e);
    Dl_info info;
    if (dladdr((const void*)&kDeviceHeader, &info) && info.dli_fname) {
      std::string p(info.dli_fname);
      const size_t k = p.rfind('/');
      p = (k == std::string::npos ? std::string(".") : p.substr(0, k)) + "/gjx_jitc";
      if (access(p.c_str(), X_OK) == 0) return p;
    }
    return std::string();
  }();
  return path;
}
inline bool write_file(const std::string& path, const char* data, size_t n) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(data, 1, n, f) == n;
  return std::fclose(f) == 0 && ok;
}
inline bool read_file(const std::string& path, std::string* out) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  char buf[1 << 16];
  size_t n;
  out->clear();
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, n);
  std::fclose(f);
  return true;
}
// The plan kinds that generate kernels.  Each has its own compiler option list (compile_options).
enum class PlanKind { importance, scan, smc, backsim, temper, predictive, psis };
// The options of one plan kind: four fixed ones, then the kind's own, then the A/B knobs (a later option wins).
//  * importance: -fno-slp-vectorize.  The SLP vectoriser turns pairs of f32 operations into v_pk_* forms, which issue no
//    faster per flop than two scalar ones (tools/README.md) but cost v_mov shuffles to build register pairs and hazard wait
//    states between dependent packed instructions.  Without it the 10-latent quad kernel has 303 more vector instructions,
//    1.5 % fewer priced issue cycles (tools/price_kernel.py), a third of the wait states and 62 instead of 67 VGPRs: 8 waves
//    per SIMD; measured 11.9 -> 10.9 us per pass (profiles/issue_cost_summary.md).
//  * scan: nothing of its own.  The scan kernels share emit_pair_lane_sites, but the LGSSM quad kernel prices at 1337.0
//    cycles per row and step with SLP and 1345.6 without (56 / 50 VGPRs: eight waves per SIMD either way).
//  * smc, backsim: nothing of their own (not priced).
//  * temper: nothing of its own (not priced): one particle per lane, nothing for the SLP vectoriser to pair.
//  * predictive: nothing of its own (not priced; profiles/predictive_summary.md has its instruction counts).
//  * psis: nothing of its own (not priced; profiles/psis_summary.md has its register counts).
inline std::vector<std::string> compile_options(PlanKind kind) {
  std::vector<std::string> opts = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"};
  if (kind == PlanKind::importance) opts.push_back("-fno-slp-vectorize");
  // GJX_JIT_DEFINE=NAME[=VALUE]: one extra -D for the generated kernel (A/B knob for device-header variants)
  if (const char* d = std::getenv("GJX_JIT_DEFINE")) opts.push_back(std::string("-D") + d);
  // GJX_JIT_OPTS="opt opt ...": extra compiler options for the generated kernel (scheduling experiments; -fslp-vectorize
  // gives an importance kernel its former option list back)
  if (const char* e = std::getenv("GJX_JIT_OPTS")) {
    std::istringstream is(e);
    for (std::string t; is >> t;) opts.push_back(t);
  }
  return opts;
}
// Which route compiled what (gjx_jit_routes): child = code objects produced by gjx_jitc, inproc = by hiprtc inside this
// process (GJX_JIT_INPROC=1 / GJX_JIT_INPROC_FALLBACK=1 only), child_failures = children that died or rejected a source,
// spawn_failures = helpers that could not be started at all.
struct RouteCounters {
  std::atomic<uint64_t> child{0}, inproc{0}, child_failures{0}, spawn_failures{0};
};
inline RouteCounters& routes() {
  static RouteCounters r;
  return r;
}
// The private directory of THIS process (re-created after a fork: a child of the host program must not share its parent's
// files), removed at exit.  Files inside are named per compilation.
struct JitDir {
  std::string path;
  pid_t owner = 0;
  bool hdr_ok = false;
  void remove_all() {
    if (path.empty() || owner != getpid()) return;  // (a forked child never deletes its parent's directory)
    if (DIR* d = opendir(path.c_str())) {
      while (dirent* e = readdir(d)) {
        if (!std::strcmp(e->d_name, ".") || !std::strcmp(e->d_name, "..")) continue;
        unlink((path + "/" + e->d_name).c_str());
      }
      closedir(d);
    }
    rmdir(path.c_str());
    path.clear();
  }
  ~JitDir() {
    if (!std::getenv("GJX_JIT_KEEP_FILES")) remove_all();
  }
  // -> the directory of the calling process ("" on failure); called under the compile lock
  const std::string& get() {
    if (!path.empty() && owner == getpid()) return path;
    const char* t = std::getenv("TMPDIR");
    std::string d = std::string(t && *t ? t : "/tmp") + "/gjx_jit_XXXXXX";
    path = mkdtemp(&d[0]) ? d : std::string();
    owner = getpid();
    hdr_ok = !path.empty() && write_file(path + "/gjx_device.hpp", kDeviceHeader, sizeof(kDeviceHeader) - 1);
    return path;
  }
};
// The child's environment: the caller's without what would make the helper more than a compiler — a profiler's or
// sanitizer's preloaded library (under rocprofv3 LD_PRELOAD would initialise the GPU inside gjx_jitc and add its output),
// and the ROCm tool variables that go with it.
inline std::vector<char*> child_environ() {
  static const char* const drop[] = {"LD_PRELOAD=", "ROCP_", "ROCPROFILER_", "ROCPROF_", "HSA_TOOLS_", "ROCTX_", "ROCTRACER_"};
  std::vector<char*> env;
  for (char** e = environ; e && *e; ++e) {
    bool skip = false;
    for (const char* d : drop) skip = skip || std::strncmp(*e, d, std::strlen(d)) == 0;
    if (!skip) env.push_back(*e);
  }
  env.push_back(nullptr);
  return env;
}
// -> 1 compiled, 0 compilation failed or the child died (logged), -1 the child could not be started
inline int compile_in_child(const std::string& src, std::string* code, PlanKind kind) {
  const std::string helper = jitc_path();
  if (helper.empty()) return -1;
  static std::mutex mu;  // compilations are serialised by the module cache's lock anyway
  std::lock_guard<std::mutex> lock(mu);
  static JitDir jd;
  static uint64_t serial = 0;
  const std::string dir = jd.get();
  if (dir.empty() || !jd.hdr_ok) return -1;
  const std::string stem = dir + "/k" + std::to_string(++serial);
  const std::string fsrc = stem + ".hip", fhdr = dir + "/gjx_device.hpp", fout = stem + ".co", flog = stem + ".log";
  if (!write_file(fsrc, src.data(), src.size())) return -1;
  const std::vector<std::string> opts = compile_options(kind);
  std::vector<char*> argv = {const_cast<char*>(helper.c_str()), const_cast<char*>(fsrc.c_str()), const_cast<char*>(fhdr.c_str()),
                             const_cast<char*>(fout.c_str()), const_cast<char*>(flog.c_str())};
  for (const std::string& o : opts) argv.push_back(const_cast<char*>(o.c_str()));
  argv.push_back(nullptr);
  std::vector<char*> env = child_environ();
  pid_t pid = 0;
  // a CHILD process (fork + exec inside posix_spawn): the caller itself is never replaced
  if (posix_spawn(&pid, helper.c_str(), nullptr, nullptr, argv.data(), env.data()) != 0) {
    unlink(fsrc.c_str());
    return -1;
  }
  int status = 0;
  while (waitpid(pid, &status, 0) < 0) {
    if (errno != EINTR) return -1;
  }
  const bool ok = WIFEXITED(status) && WEXITSTATUS(status) == 0 && read_file(fout, code) && !code->empty();
  if (ok) {
    routes().child++;
  } else if (WIFEXITED(status) && WEXITSTATUS(status) == 127) {
    // posix_spawn reports an exec failure of the child as exit status 127: the helper did not start
    unlink(fsrc.c_str());
    return -1;
  } else if (WIFSIGNALED(status)) {
    routes().child_failures++;
    std::fprintf(stderr, "[gjx] the plan compiler (gjx_jitc, pid %d) died with signal %d on a generated kernel; source kept in %s\n",
                 (int)pid, WTERMSIG(status), fsrc.c_str());
  } else {
    routes().child_failures++;
    std::string log;
    (void)read_file(flog, &log);
    std::fprintf(stderr, "[gjx] hiprtc: plan specialisation failed to compile (child status %d)%s\n", WIFEXITED(status) ? WEXITSTATUS(status) : -1,
                 std::getenv("GJX_PLAN_JIT_VERBOSE") ? ":" : "; GJX_PLAN_JIT_VERBOSE=1 prints the compiler log");
    if (std::getenv("GJX_PLAN_JIT_VERBOSE")) std::fprintf(stderr, "%s\n", log.c_str());
  }
  unlink(fout.c_str());
  unlink(flog.c_str());
  if (ok || !WIFSIGNALED(status)) unlink(fsrc.c_str());  // (the source of a crashed compilation is kept for the report)
  return ok ? 1 : 0;
}

// Compile `src` for gfx950; on success `code` holds the code object.
inline bool compile_to_code(const std::string& src, std::string* code, PlanKind kind) {
  // GJX_PLAN_JIT_DUMP_FILE=path: the source about to be compiled (overwritten per compilation: after a compiler crash the
  // file holds the offending kernel)
  if (const char* f = std::getenv("GJX_PLAN_JIT_DUMP_FILE")) {
    if (FILE* fp = fopen(f, "w")) {
      fwrite(src.data(), 1, src.size(), fp);
      fclose(fp);
    }
  }
  const char* inproc = std::getenv("GJX_JIT_INPROC");
  if (!(inproc && inproc[0] == '1')) {
    const int r = compile_in_child(src, code, kind);
    if (r >= 0) return r == 1;
    routes().spawn_failures++;
    // no silent change of route: a caller that accepts the compiler inside its own address space says so
    const char* fb = std::getenv("GJX_JIT_INPROC_FALLBACK");
    if (!(fb && fb[0] == '1')) {
      std::fprintf(stderr, "[gjx] gjx_jitc (the plan compiler's child process) could not be started%s: GJX_ERR_JIT.  "
                           "GJX_JIT_INPROC_FALLBACK=1 (or GJX_JIT_INPROC=1) compiles inside the calling process instead\n",
                   jitc_path().empty() ? " (no executable gjx_jitc next to the library; GJX_JITC=path overrides)" : "");
      return false;
    }
    static bool warned = false;
    if (!warned) {
      warned = true;
      std::fprintf(stderr, "[gjx] gjx_jitc could not be started: compiling in-process (GJX_JIT_INPROC_FALLBACK=1)\n");
    }
  }
  hiprtcProgram prog;
  const char* hn[] = {"gjx_device.hpp"};
  const char* hs[] = {kDeviceHeader};
  if (hiprtcCreateProgram(&prog, src.c_str(), "gjx_plan.hip", 1, hs, hn) != HIPRTC_SUCCESS) return false;
  const std::vector<std::string> extra = compile_options(kind);
  std::vector<const char*> opts;
  for (const std::string& t : extra) opts.push_back(t.c_str());
  const hiprtcResult r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
  if (r != HIPRTC_SUCCESS) {
    size_t ls = 0;
    hiprtcGetProgramLogSize(prog, &ls);
    std::string log(ls, 0);
    if (ls) hiprtcGetProgramLog(prog, &log[0]);
    // always say THAT it failed; the full compiler log on request
    std::fprintf(stderr, "[gjx] hiprtc: plan specialisation failed to compile (%s)%s\n", hiprtcGetErrorString(r),
                 std::getenv("GJX_PLAN_JIT_VERBOSE") ? ":" : "; GJX_PLAN_JIT_VERBOSE=1 prints the compiler log");
    if (std::getenv("GJX_PLAN_JIT_VERBOSE")) std::fprintf(stderr, "%s\n", log.c_str());
    hiprtcDestroyProgram(&prog);
    return false;
  }
  size_t cs = 0;
  hiprtcGetCodeSize(prog, &cs);
  code->assign(cs, 0);
  hiprtcGetCode(prog, &(*code)[0]);
  hiprtcDestroyProgram(&prog);
  routes().inproc++;
  return true;
}
inline bool compile_only(const std::string& src, PlanKind kind) {
  std::string code;
  return compile_to_code(src, &code, kind) && !code.empty();
}

// The module cache.  Identical sources (same model structure) share one loaded module process-wide, so re-creating a
// plan — or running the same model on another dataset, whose values are launch parameters, not source — does not
// recompile.  Entries are reference-counted by the plans that use them; unreferenced modules stay cached for reuse up to
// GJX_JIT_CACHE_MAX entries (default 64) and are then unloaded least-recently-used first, so a long-lived process that
// keeps generating NEW model structures holds a bounded number of code objects.
struct ModuleCache {
  struct Entry {
    hipModule_t mod = nullptr;
    int refs = 0;
    uint64_t tick = 0;
  };
  std::mutex mu;
  std::unordered_map<std::string, Entry> map;
  uint64_t clock = 0, compiles = 0, evictions = 0;
  size_t cap = [] {
    const char* e = std::getenv("GJX_JIT_CACHE_MAX");
    const long v = e ? atol(e) : 64;
    return (size_t)(v < 1 ? 1 : v);
  }();
  static ModuleCache& get() {
    static ModuleCache c;
    return c;
  }
  // The key of a source: the source itself and the compiler options beyond the four fixed ones (the plan kind's own and
  // the A/B knobs GJX_JIT_DEFINE, GJX_JIT_OPTS) — the same text compiled under another option is another module.
  static std::string key_of(const std::string& src, PlanKind kind) {
    const std::vector<std::string> opts = compile_options(kind);
    std::string key = src;
    for (size_t k = 4; k < opts.size(); ++k) key += "\n// " + opts[k];  // (the four fixed options come first)
    return key;
  }
  // -> the loaded module of `src` with one more reference, or nullptr (compile / load failure, logged); `key_out`: what
  // release() takes
  hipModule_t acquire(const std::string& src, PlanKind kind, std::string* key_out) {
    const std::string key = key_of(src, kind);
    *key_out = key;
    std::lock_guard<std::mutex> lock(mu);
    auto it = map.find(key);
    if (it == map.end()) {
      std::string code;
      if (!compile_to_code(src, &code, kind)) return nullptr;
      hipModule_t mod = nullptr;
      const hipError_t le = hipModuleLoadData(&mod, code.data());
      if (le != hipSuccess) {
        (void)hipGetLastError();
        std::fprintf(stderr, "[gjx] hipModuleLoadData failed for a specialised plan kernel: %s\n", hipGetErrorString(le));
        return nullptr;
      }
      ++compiles;
      it = map.emplace(key, Entry{mod, 1, ++clock}).first;  // referenced before anything is evicted
      evict_locked();
      return mod;
    }
    it->second.refs++;
    it->second.tick = ++clock;
    return it->second.mod;
  }
  void release(const std::string& key) {
    if (key.empty()) return;
    std::lock_guard<std::mutex> lock(mu);
    auto it = map.find(key);
    if (it != map.end() && it->second.refs > 0) it->second.refs--;
    evict_locked();
  }
  void evict_locked() {
    while (map.size() > cap) {
      auto victim = map.end();
      for (auto it = map.begin(); it != map.end(); ++it)
        if (it->second.refs == 0 && (victim == map.end() || it->second.tick < victim->second.tick)) victim = it;
      if (victim == map.end()) return;  // everything is in use
      // no plan references the module, but launches of its kernels may still be in flight on some stream: an eviction
      // is rare (a process that keeps generating new model structures), so wait for the device before unloading
      (void)hipDeviceSynchronize();
      (void)hipModuleUnload(victim->second.mod);
      map.erase(victim);
      ++evictions;
    }
  }
};

// One slot of a plan: a reference on the cached module of one generated source, and the plan's device tables as that
// source numbers them.  The plan kinds derive from it and add the function handles of their kernels.
struct Module {
  int state = 0;  // 0 untried, 1 ready, -1 failed
  std::string key;  // the module-cache entry this slot holds a reference on (ModuleCache::key_of the source)
  gjx::PlanTables tabs;  // the device tables of THIS plan, in the order the source numbers them (kernel argument)

  void release() {
    ModuleCache::get().release(key);
    key.clear();
  }
  // The module of `src` (compiled, or shared with plans of the same structure) and its kernels `names` into `fns`.  A slot
  // that is being rebuilt (e.g. without the occupancy hint) lets go of its module first.
  bool load(const std::string& src, PlanKind kind, std::initializer_list<const char*> names, std::initializer_list<hipFunction_t*> fns) {
    release();
    std::string k;
    hipModule_t mod = ModuleCache::get().acquire(src, kind, &k);
    if (!mod) return false;
    key = k;
    auto fn = fns.begin();
    for (const char* name : names) {
      const hipError_t ge = hipModuleGetFunction(*fn++, mod, name);
      if (ge == hipSuccess) continue;
      (void)hipGetLastError();
      std::fprintf(stderr, "[gjx] hipModuleGetFunction failed for the generated kernel %s: %s\n", name, hipGetErrorString(ge));
      for (hipFunction_t* f : fns) *f = nullptr;
      release();
      return false;
    }
    return true;
  }
};
struct CompiledKernel : Module {  // one generated kernel: each of the four slots of a tempered plan (gjx_hip.hip TemperKernel)
  hipFunction_t fn = nullptr;
};
struct Compiled : CompiledKernel {  // an importance or scan kernel
  int block = 256;  // threads per workgroup of the compiled kernel
  int rows_per_block = 1;  // 256-particle rows per workgroup
};
struct CompiledSmc : Module {  // the kernels of a filter (bootstrap or guided)
  hipFunction_t step = nullptr, step_adaptive = nullptr, init = nullptr;
};
struct CompiledBacksim : Module {  // the two kernels of a backward pass
  hipFunction_t step = nullptr, last = nullptr;
};

}  // namespace gjx_jit
