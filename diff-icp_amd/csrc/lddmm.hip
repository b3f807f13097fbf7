// C-ABI entry points of the Gaussian-kernel reductions (GenKernel, kernel.py:58-337) and of
// the fused LDDMM geodesic-shooting ODE (LDDMMModel.ODE, LDDMM.py:176-227) for gfx950.
#include "launch.hpp"
#include "lddmm_ops.hpp"
#include "lddmm_sym.hpp"
#include "packed.hpp"
#include "lddmm_sym_pk.hpp"
#include "mfma_fwd.hpp"
#include "ext_pk.hpp"

#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <type_traits>

using namespace dicp;

namespace {

#ifndef DICP_KR
#define DICP_KR 2
#endif
constexpr int kR = DICP_KR;  // rows per thread for the light reductions (KRed etc.)

// Rows per thread of the fused ODE passes (tuning knobs, env DICP_R_FWD / DICP_R_BWD in
// {1, 2, 4}; read once).  Defaults chosen from measurements on MI355X.
int env_r(const char* name, int def) {
  const char* v = getenv(name);
  if (!v) return def;
  const int r = atoi(v);
  return (r == 1 || r == 2 || r == 4) ? r : def;
}
int g_r_fwd = -1, g_r_bwd = -1;
int r_fwd() { if (g_r_fwd < 0) g_r_fwd = env_r("DICP_R_FWD", 2); return g_r_fwd; }
int r_bwd() { if (g_r_bwd < 0) g_r_bwd = env_r("DICP_R_BWD", 1); return g_r_bwd; }
// eta = 0 VJP: 0 = OpOdeSelfBwd (55 VALU/pair), 1 = OpOdeSelfBwd2 (48), 2 = symmetric
// pair-once kernel (lddmm_sym.hpp, ~32 VALU per ordered pair), 3 = the same pair-once
// decomposition with the lane's two rows packed as float2 (lddmm_sym_pk.hpp, v_pk_*_f32; default: 5-7% faster on MI355X at 50k-100k)
int g_bwd_alg = 3;
// eta != 0 VJP: 0 = ordered OpOdeSelfBwdEta, 1 = symmetric pair-once SymBwdEta (lddmm_sym.hpp),
// 2 = the same with packed-FP32 rows (lddmm_sym_pk.hpp SymBwdEtaPk)
#ifndef DICP_BWD_ETA_ALG
#define DICP_BWD_ETA_ALG 2
#endif
int g_bwd_eta_alg = DICP_BWD_ETA_ALG;
// external-point passes and KRed below the centred path's sizes: 0 = generic scalar rows in
// original units (OpOdeExtFwd / OpOdeExtBwdX / OpOdeExtBwdQ / OpKRed), 1 = packed-FP32 rows in
// scaled coordinates (ext_pk.hpp; the external-point VJP only for eta = 0)
int g_ext_alg = 1;
// coordinates of the default packed shooting kernels (OpOdeSelfFwdPk, SymBwdPk): 0 = scaled,
// q' = alpha (q - q_0), one packed multiply per two pairs fewer; 1 = original units, exact
// differences whatever the cloud's extent.  Per HOST THREAD (the shooting
// sets it around its own launches; concurrent frames run on their own threads).
thread_local int tl_coord_raw = 0;
// eta = 0 forward: 0 = OpOdeSelfFwd (ordered rows, R = 2), 1 = symmetric pair-once kernel
// (lddmm_sym.hpp SymFwd: 17 VALU + 0.5 exp per ordered pair instead of 20 + 1, but 3-5%
// slower: issue-stalled on its rotating column sums), 2 = packed-FP32 rows (packed.hpp: the
// thread's two rows as float2, 11 VALU instructions per pair; measured 4-11% faster
// than 0 at 200k-20k on MI355X), 3 = the column contraction on the matrix cores
// (mfma_fwd.hpp: VALU evaluates K, one v_mfma_f32_16x16x4_f32 per 64 pairs sums 16 channels;
// eta = 0 only, eta != 0 keeps 2), 4 = the symmetric pair-once kernel with packed-FP32 rows
// (lddmm_sym_pk.hpp SymFwdPk; all rows only, row slices take 2)
#ifndef DICP_FWD_ALG
#define DICP_FWD_ALG 2
#endif
int g_fwd_alg = DICP_FWD_ALG;
#ifndef DICP_MFMA_RMAX_X100
#define DICP_MFMA_RMAX_X100 300
#endif
struct MfmaRmaxInit {
  MfmaRmaxInit() { if (mfma_rmax_x100() < 0) mfma_rmax_x100() = DICP_MFMA_RMAX_X100; }
} g_mfma_rmax_init;

// Run-time values to template arguments.  A functor receives the value as an integral constant
// (`decltype(d)::value`) or the operator as a tag (`op_of<decltype(t)>`).
template <int V> using Int = std::integral_constant<int, V>;
template <class Op> struct OpTag { using type = Op; };
template <class Tag> using op_of = typename Tag::type;
template <size_t N> size_t max_of(const size_t (&v)[N]) { return *std::max_element(v, v + N); }

bool supported_dim(int D) { return D == 2 || D == 3; }

// f(Int<D>) for a supported D ...
template <class F>
auto for_dim(int D, F&& f) {
  return D == 2 ? f(Int<2>{}) : f(Int<3>{});
}
// ... and for the D of an entry point, which may be any
template <class F>
int with_dim(int D, const char* entry, F&& f) {
  if (!supported_dim(D)) {
    set_error("%s: D=%d unsupported (compiled in: 2, 3)", entry, D);
    return DICP_ERR_UNSUPPORTED;
  }
  return for_dim(D, f);
}

// f(Int<R>) for the rows per thread of an ordered scalar pass (r_fwd() / r_bwd(): 1, 2 or 4)
template <class F>
auto for_rows(int R, F&& f) {
  return R == 1 ? f(Int<1>{}) : R == 4 ? f(Int<4>{}) : f(Int<2>{});
}

// f(std::bool_constant<b>)
template <class F>
auto for_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

template <class Op>
int launch_r(int R, const char* name, const Args& a, const Scal& sc, int64_t M, int64_t N,
             const Outs& o, void* ws, size_t wsb, hipStream_t st) {
  return for_rows(R, [&](auto r) { return launch_rowred<Op, decltype(r)::value>(name, a, sc, M, N, o, ws, wsb, st); });
}

template <class Op>
size_t ws_r(int R, int64_t M, int64_t N) {
  return for_rows(R, [&](auto r) { return rowred_ws_bytes<Op, decltype(r)::value>(M, N); });
}

template <template <int> class OpT>
int red_dispatch(const char* name, int D, const Args& a, const Scal& sc, int64_t M, int64_t N,
                 float* out, void* ws, size_t wsb, hipStream_t st) {
  return with_dim(D, name, [&](auto d) {
    return launch_rowred<OpT<decltype(d)::value>, kR>(name, a, sc, M, N, make_outs(out), ws, wsb, st);
  });
}

template <int D> using OpGradLapKPlain = OpGradLapK<D, false>;
template <int D> using OpGradLapKScal = OpGradLapK<D, true>;

template <template <int> class OpT>
size_t red_ws(int D, int64_t M, int64_t N) {
  return for_dim(D, [&](auto d) { return rowred_ws_bytes<OpT<decltype(d)::value>, kR>(M, N); });
}

// Scaled-coordinate ops (OpOdeSelfFwd / OpOdeSelfBwd): alpha = sqrt(log2 e / (2 sigma^2)),
// aux1 = s / alpha.
// The coordinate origin is the first column point (a.c0: the support q of the self ops, the
// support of the external-point x pass, y of KRed), the same for rows and columns.
void scale_coords(Args& a, Scal& sc, double sigma) {
  const double alpha = std::sqrt(1.4426950408889634 / (2.0 * sigma * sigma));
  a.scale = (float)alpha;
  a.shift = a.c0;
  sc.aux1 = (float)(1.0 / (sigma * sigma) / alpha);
}

// original-unit coordinates for the RAW packed kernels: alpha = 1, no shift, aux1 = s / 1
void raw_coords(Args& a, Scal& sc) {
  a.scale = 1.f;
  a.shift = nullptr;
  sc.aux1 = sc.s;
}

// ---- the packed ordered forward (packed.hpp OpOdeSelfFwdPk): THE variant table ----
// One pass: the divergence sums (g rows), the eta terms, the Gs' sums (mG), the divergence rows
// (zs) and original-unit coordinates.  Everything that launches or sizes these passes goes
// through visit_pk_fwd / for_each_pk_fwd, so a new variant is added here and nowhere else.
struct PkFwd {
  bool div, eta, g, zs, raw;
};
// the variants that exist (the static_assert of the operator: zs rows have the divergence sums
// and no eta; the eta sums contain the divergence's, so eta comes with div only)
constexpr bool pk_fwd_exists(PkFwd v) { return (!v.zs || (v.div && !v.eta)) && (!v.eta || v.div); }

template <int D, bool DIV, bool ETA, bool G, bool ZS, class F>
auto pk_fwd_coords(bool raw, F&& f) {
  return raw ? f(OpTag<OpOdeSelfFwdPk<D, DIV, ETA, G, ZS, true>>{})
             : f(OpTag<OpOdeSelfFwdPk<D, DIV, ETA, G, ZS, false>>{});
}
// f(OpTag<the pass>) for the flags; zs and eta imply div
template <int D, class F>
auto visit_pk_fwd(PkFwd v, F&& f) {
  if (v.zs)
    return v.g ? pk_fwd_coords<D, true, false, true, true>(v.raw, f)
               : pk_fwd_coords<D, true, false, false, true>(v.raw, f);
  if (v.eta)
    return v.g ? pk_fwd_coords<D, true, true, true, false>(v.raw, f)
               : pk_fwd_coords<D, true, true, false, false>(v.raw, f);
  if (v.div)
    return v.g ? pk_fwd_coords<D, true, false, true, false>(v.raw, f)
               : pk_fwd_coords<D, true, false, false, false>(v.raw, f);
  return v.g ? pk_fwd_coords<D, false, false, true, false>(v.raw, f)
             : pk_fwd_coords<D, false, false, false, false>(v.raw, f);
}
// f(OpTag<pass>) for every variant that exists
template <int D, class F>
void for_each_pk_fwd(F&& f) {
  for (int i = 0; i < 32; ++i) {
    const PkFwd v = {(i & 1) != 0, (i & 2) != 0, (i & 4) != 0, (i & 8) != 0, (i & 16) != 0};
    if (pk_fwd_exists(v)) visit_pk_fwd<D>(v, f);
  }
}

const char* pk_fwd_name(PkFwd v) {
  if (v.zs) return v.g ? "ode_self_fwd(pk, zs)" : "ode_self_fwd(pk, no mG, zs)";
  if (v.eta) return v.g ? "ode_self_fwd_eta(pk)" : "ode_self_fwd_eta(pk, no mG)";
  return v.g ? "ode_self_fwd(pk)" : "ode_self_fwd(pk, no mG)";
}

template <int D>
int launch_fwd_pk(PkFwd v, Args a, Scal sc, int64_t nrows, int64_t M, const Outs& o, void* ws, size_t wsb,
                  hipStream_t st) {
  if (v.raw) raw_coords(a, sc);
  return visit_pk_fwd<D>(v, [&](auto t) {
    return launch_rowred_pk<op_of<decltype(t)>>(pk_fwd_name(v), a, sc, nrows, M, o, ws, wsb, st);
  });
}
template <int D>
size_t fwd_pk_ws(int64_t nrows, int64_t M) {
  size_t m = 0;
  for_each_pk_fwd<D>([&](auto t) { m = std::max(m, rowred_pk_ws_bytes<op_of<decltype(t)>>(nrows, M)); });
  return m;
}

}  // namespace

extern "C" int dicp_supports_dim(int D) { return supported_dim(D) ? 1 : 0; }

// Tuning knobs (include/difficp_hip.h lists them in this order): one row per option, read by
// dicp_set_option and dicp_get_option alike.
namespace {
struct Option {
  const char* name;
  int (*get)();
  void (*set)(int);
  int lo, hi;        // allowed range ...
  const int* only;   // ... or, when not NULL, the allowed set (ends with -1)
  bool or_zero;      // 0 (automatic) is allowed besides the range
  bool per_thread;   // the value belongs to the calling host thread
};
#define DICP_OPTION(name, read, lvalue, ...) \
  {name, [] { return (int)(read); }, [](int v) { lvalue = v; }, __VA_ARGS__}
constexpr int kNoMax = INT32_MAX;
constexpr int kRows124[] = {1, 2, 4, -1}, kRows0468[] = {0, 4, 6, 8, -1}, kRows048[] = {0, 4, 8, -1};
const Option kOptions[] = {
    DICP_OPTION("fwd_alg", g_fwd_alg, g_fwd_alg, 0, 6),
    DICP_OPTION("bwd_alg", g_bwd_alg, g_bwd_alg, 0, 3),
    DICP_OPTION("bwd_eta_alg", g_bwd_eta_alg, g_bwd_eta_alg, 0, 2),
    DICP_OPTION("r_fwd", r_fwd(), g_r_fwd, 0, 0, kRows124),
    DICP_OPTION("r_bwd", r_bwd(), g_r_bwd, 0, 0, kRows124),
    DICP_OPTION("split_rounds", split_rounds(), split_rounds(), 0, 64),
    DICP_OPTION("force_splits", force_splits(), force_splits(), 0, 65536),
    DICP_OPTION("sym_L", sym_L(), sym_L(), 0, 64),
    DICP_OPTION("min_chunk", min_chunk(), min_chunk(), 16, 65536, nullptr, true),
    DICP_OPTION("pk_rp", pk_rp_force(), pk_rp_force(), 0, kPkRPMax),
    DICP_OPTION("sym_rp", sym_rp(), sym_rp(), 0, 2),
    DICP_OPTION("red_alg", red_alg(), red_alg(), 0, 2),
    DICP_OPTION("sym_red", sym_red(), sym_red(), 0, 2),
    DICP_OPTION("sym_red_rows", sym_red_rows(), sym_red_rows(), 0, 0, kRows048),
    DICP_OPTION("sym_fwd_rows", sym_fwd_rows(), sym_fwd_rows(), 0, 0, kRows0468),
    DICP_OPTION("pair_cutoff", pair_cutoff(), pair_cutoff(), 0, 2),
    DICP_OPTION("pair_cutoff_log2", pair_cutoff_log2(), pair_cutoff_log2(), 8, 150),
    DICP_OPTION("lse_pk", lse_pk(), lse_pk(), 0, 1),
    DICP_OPTION("lse_adapt", lse_adapt(), lse_adapt(), 0, kNoMax),
    DICP_OPTION("lse_bound", lse_bound(), lse_bound(), 0, 1),
    DICP_OPTION("cx_rho_x100", cx_rho_x100(), cx_rho_x100(), 0, 100000),
    DICP_OPTION("mfma_rmax_x100", mfma_rmax_x100(), mfma_rmax_x100(), 0, kNoMax),
    DICP_OPTION("ext_alg", g_ext_alg, g_ext_alg, 0, 1),
    DICP_OPTION("batch_share", batch_share(), tl_batch_share, 1, 4096, nullptr, false, true),
    DICP_OPTION("coord_raw", tl_coord_raw, tl_coord_raw, 0, 1, nullptr, false, true),
};
#undef DICP_OPTION

const Option* find_option(const char* name) {
  for (const Option& o : kOptions)
    if (!strcmp(name, o.name)) return &o;
  return nullptr;
}
bool option_allows(const Option& o, int v) {
  if (v == 0 && o.or_zero) return true;
  if (o.only == nullptr) return v >= o.lo && v <= o.hi;
  for (const int* s = o.only; *s >= 0; ++s)
    if (*s == v) return true;
  return false;
}
}  // namespace

extern "C" int dicp_set_option(const char* name, int value) {
  const Option* o = name ? find_option(name) : nullptr;
  if (o == nullptr) {
    set_error("dicp_set_option: unknown option %s", name ? name : "(NULL)");
    return DICP_ERR_INVALID;
  }
  if (!option_allows(*o, value)) return DICP_ERR_INVALID;
  o->set(value);
  return DICP_OK;
}

extern "C" int dicp_get_option(const char* name, int* value) {
  if (name == nullptr || value == nullptr) {
    set_error("dicp_get_option: NULL argument");
    return DICP_ERR_INVALID;
  }
  const Option* o = find_option(name);
  if (o == nullptr) {
    set_error("dicp_get_option: unknown option %s", name);
    return DICP_ERR_INVALID;
  }
  *value = o->get();
  return DICP_OK;
}

extern "C" int dicp_gauss_red_f32(int op, const float* x, int64_t M, const float* y, int64_t N,
                                  int D, const float* b, const float* c, double sigma, float* out,
                                  void* ws, size_t ws_bytes, dicp_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (M < 0 || N < 0 || (M > 0 && (!x || !out)) || (N > 0 && !y) || !(sigma > 0)) {
    set_error("dicp_gauss_red_f32: invalid arguments");
    return DICP_ERR_INVALID;
  }
  Args a = {x, c, nullptr, nullptr, y, b, nullptr, nullptr};
  const Scal sc = make_scal(sigma, 0.0);
  const bool needb = op == DICP_KREDSCAL || op == DICP_KRED || op == DICP_GRADK_REV ||
                     op == DICP_DDK || op == DICP_GENDK || op == DICP_HESSK ||
                     op == DICP_GRADKSCAL || op == DICP_GRADLAPKSCAL;
  const bool needc = op == DICP_GENDK || op == DICP_HESSK;
  if ((needb && N > 0 && !b) || (needc && M > 0 && !c)) {
    set_error("dicp_gauss_red_f32: op %d needs b%s", op, needc ? " and c" : "");
    return DICP_ERR_INVALID;
  }
  if (cx_has_op(op) && (D == 2 || D == 3) && (cx_eligible(M, N) || scx_eligible(op, x, M, y, N)))
    return cx_gauss_red(op, x, M, y, N, D, b, sigma, out, ws, ws_bytes, st);
  if (op == DICP_KRED && g_ext_alg == 1 && (D == 2 || D == 3) && N > 0) {
    // KRed = the external-point forward's velocity sum: the packed scaled-coordinate kernel
    const Args ak = {x, nullptr, nullptr, nullptr, y, b, nullptr, nullptr};
    const Scal sk = make_scal(sigma, 0.0);
    const Outs o = make_outs(out);
    return D == 2 ? launch_rowred_pk<OpExtFwdPk<2, false, false>>("KRed", ak, sk, M, N, o, ws, ws_bytes, st)
                  : launch_rowred_pk<OpExtFwdPk<3, false, false>>("KRed", ak, sk, M, N, o, ws, ws_bytes, st);
  }
  switch (op) {
    case DICP_KBASE: return red_dispatch<OpKBase>("KBase", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_KREDSCAL: return red_dispatch<OpKRedScal>("KRedScal", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_KRED: return red_dispatch<OpKRed>("KRed", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_GRADK: return red_dispatch<OpGradK>("GradKRed", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_GRADK_REV: return red_dispatch<OpZDotB>("GradKRed_rev", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_DDK: return red_dispatch<OpDDK>("DDKRed", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_GENDK: return red_dispatch<OpGenDK>("GenDKRed", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_HESSK: return red_dispatch<OpHessK>("HessKRed", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_LAPK: return red_dispatch<OpLapK>("LapKRed", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_GRADLAPK: return red_dispatch<OpGradLapKPlain>("GradLapKRed", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_GRADKSCAL: return red_dispatch<OpGradKScal>("GradKScal", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_GRADLAPKSCAL: return red_dispatch<OpGradLapKScal>("GradLapKScal", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_MIN_SQDIST: return red_dispatch<OpMinSqDist>("MinSqDist", D, a, sc, M, N, out, ws, ws_bytes, st);
    case DICP_MIN_SQDIST_OTHER:
      if (N != M || x != y || M > INT32_MAX) {
        set_error("dicp_gauss_red_f32: MIN_SQDIST_OTHER needs y == x (same buffer, M == N < 2^31)");
        return DICP_ERR_INVALID;
      }
      return red_dispatch<OpMinSqDistOther>("MinSqDistOther", D, a, sc, M, N, out, ws, ws_bytes, st);
    default: set_error("dicp_gauss_red_f32: unknown op %d", op); return DICP_ERR_UNSUPPORTED;
  }
}

extern "C" int dicp_radius_count_f32(const float* x, int64_t M, const float* y, int64_t N, int D,
                                     double R, float* counts, void* ws, size_t ws_bytes,
                                     dicp_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (M < 0 || N < 0 || (M > 0 && (!x || !counts)) || (N > 0 && !y) || !(R >= 0)) {
    set_error("dicp_radius_count_f32: invalid arguments");
    return DICP_ERR_INVALID;
  }
  const Args a = {x, nullptr, nullptr, nullptr, y, nullptr, nullptr, nullptr};
  Scal sc = make_scal(1.0, 0.0);
  sc.aux0 = (float)(R * R);  // torch compares the float32 distances with (float)(R**2)
  return red_dispatch<OpRadiusCount>("RadiusCount", D, a, sc, M, N, counts, ws, ws_bytes, st);
}

// ---------------------------------------------------------------------------------------
// Fused ODE
// ---------------------------------------------------------------------------------------
namespace {

// packed forward algorithms: 2 (default: ordered rows, the symmetric 4-row pass for whole
// passes from DICP_SYM_FWD4_MIN_M points), 5 (symmetric 4-row wherever it applies), 6 (ordered
// rows always)
bool packed_fwd_alg(int alg) { return alg == 2 || alg == 5 || alg == 6; }
#ifndef DICP_SYM_FWD4_MIN_M
#define DICP_SYM_FWD4_MIN_M 20000
#endif
// The symmetric 4-row forward (SymFwdPk4) for this pass?  Whole passes (all rows) in scaled
// coordinates only.  Automatic rule (fwd_alg 2), measured on MI355X: with the column groups
// of sym_geom's wg_min 4096 rule the Euler step with divergence rows is 1.03x the ordered
// pass at 20k, 1.10x at 40k, 1.01x at 50k, 1.07x at 60k, 1.10x at 80k-200k
// (tools/probes/sym_L_rows4.py KIND=fwd, profiles/r04_ab_fwd4_L_small.jsonl; with L = 4 it lost
// below 75k: r04_ab_fwd_sym4.jsonl) -- from 20k points, or, with the geometry hint
// batch_share > 1 (concurrent / batched frames), when the sharing calls have >= 1e9 pairs
// (as the 4-row VJP, lddmm_sym.hpp DICP_SYM_SHARE4_MIN_PAIRS).
bool use_sym_fwd4(int alg, int64_t M, bool all, bool raw) {
  if (!all || raw || !(alg == 2 || alg == 5)) return false;
  if (alg == 5) return true;
  if (batch_share() > 1) return M >= 8192 && (double)M * (double)M * batch_share() >= DICP_SYM_SHARE4_MIN_PAIRS;
  return M >= DICP_SYM_FWD4_MIN_M;
}

// rows per lane of the symmetric forward (SymFwdPkN) when the pass runs alone on the chip
// (batch_share 1; a lockstep batch takes each frame's own rule, so a batched call equals the
// call made alone bitwise): 6 (384-point groups, 3 waves / SIMD) from
// DICP_SYM_FWD6_MIN_M points, 8 (512-point groups, 2 waves / SIMD) from DICP_SYM_FWD8_MIN_M,
// else 4; sym_fwd_rows 4 / 6 / 8 forces.  Measured r06 (tools/probes/symfwd_L.py, the Euler
// step with divergence rows, profiles/r06_symfwd_rows.jsonl): 6 rows against 4 -2% at 40k,
// -4% at 60k, -5% at 80k-100k (3.235 vs 3.394 ms at the north_star's 100k), -4% / -7% at
// 120k / 150k; 8 rows lose at 100k (3.86: 2 workgroups per CU, a ragged last round) and win
// from ~200k (12.67 vs 13.02 ms)
#ifndef DICP_SYM_FWD6_MIN_M
#define DICP_SYM_FWD6_MIN_M 40000
#endif
#ifndef DICP_SYM_FWD8_MIN_M
#define DICP_SYM_FWD8_MIN_M 180000
#endif
int sym_fwd_rows_for(int64_t M) {
  const int f = sym_fwd_rows();
  if (f == 4 || f == 6 || f == 8) return f;
  if (batch_share() > 1) return 4;
  return M >= DICP_SYM_FWD8_MIN_M ? 8 : M >= DICP_SYM_FWD6_MIN_M ? 6 : 4;
}
template <int D, bool DIV>
int launch_sym_fwd_rows(const Args& a, const Scal& sc, int64_t M, const Outs& o, void* ws, size_t wsb,
                        hipStream_t st, bool zs) {
  switch (sym_fwd_rows_for(M)) {
    case 8: return launch_sym_fwd8<D, DIV>(a, sc, M, o, ws, wsb, st, zs);
    case 6: return launch_sym_fwd6<D, DIV>(a, sc, M, o, ws, wsb, st, zs);
    default: return launch_sym_fwd4<D, DIV>(a, sc, M, o, ws, wsb, st, zs);
  }
}

// Which kernel family runs a forward pass: the one rule, first match wins.
enum class FwdFamily { kPacked, kScalar, kSym, kMfma, kSymRows, kZsUnsupported };
struct FwdWant {   // the pass's terms and outputs
  bool eta, mg, div, h, zs;
};
FwdFamily fwd_family(int alg, bool all, bool raw, FwdWant w, int64_t M) {
  if (w.zs) {
    // divergence rows out through the (unused) h slot: the packed passes only
    if (w.eta || w.h || (w.mg && !packed_fwd_alg(alg))) return FwdFamily::kZsUnsupported;
    // (the mG-less last step keeps the ordered pass without the Gs' sums: 2.49 against 3.27 ms
    // for the symmetric pass, which forms them anyway, at 100k)
    return w.mg && use_sym_fwd4(alg, M, all, raw) ? FwdFamily::kSymRows : FwdFamily::kPacked;
  }
  if (w.eta) return alg >= 2 ? FwdFamily::kPacked : FwdFamily::kScalar;
  if (!w.mg) return FwdFamily::kPacked;   // mG not wanted: the packed forward without the Gs' sums
  if ((alg == 1 || alg == 4) && all) return FwdFamily::kSym;
  if (alg == 3) return FwdFamily::kMfma;
  if (use_sym_fwd4(alg, M, all, raw)) return FwdFamily::kSymRows;   // pair-once, 4 / 6 / 8 rows per lane
  return alg >= 2 ? FwdFamily::kPacked : FwdFamily::kScalar;
}

// rows [row0, row0 + nrows) of the pass against all M columns (row-split over ranks);
// nrows < 0: all rows.  Output pointers in `o` address the row slice.
// order: optional nrows int32 row indices (a permutation of the slice's rows) that groups
// spatially close rows into the same workgroup -- used by the matrix-core forward, whose
// fp32 error grows with the spread of a workgroup's rows (mfma_fwd.hpp); ignored otherwise.
template <int D>
int ode_self_fwd_d(const float* q, const float* p, int64_t M, double sigma, double eta,
                   Outs o, void* ws, size_t wsb, hipStream_t st, int64_t row0 = 0,
                   int64_t nrows = -1, const int* order = nullptr, float* zs = nullptr) {
  if (nrows < 0) nrows = M;
  const bool all = row0 == 0 && nrows == M;
  Args a = {q + row0 * D, p + row0 * D, nullptr, nullptr, q, p, nullptr, nullptr, 0.f};
  Scal sc = make_scal(sigma, eta);
  scale_coords(a, sc, sigma);
  const bool raw = tl_coord_raw != 0;   // the packed kernels; the others stay scaled
  const FwdWant w = {eta != 0.0, o.ptr[1] != nullptr, o.ptr[2] != nullptr || zs != nullptr,
                     o.ptr[3] != nullptr, zs != nullptr};
  const FwdFamily fam = fwd_family(g_fwd_alg, all, raw, w, M);
  if (fam == FwdFamily::kZsUnsupported) {
    set_error("ode_self_fwd: divergence rows (zs) need eta = 0, no h output and fwd_alg 2, 5 or 6");
    return DICP_ERR_INVALID;
  }
  if (w.zs) {
    o.ptr[3] = zs;
    o.base[3] = o.add[3] = nullptr;
    o.accumulate[3] = 0;
    o.alpha[3] = 1.f;
  }
  switch (fam) {
    case FwdFamily::kPacked:
      return launch_fwd_pk<D>({w.div, w.eta, w.mg, w.zs, raw}, a, sc, nrows, M, o, ws, wsb, st);
    case FwdFamily::kSym:
      return for_bool(w.div, [&](auto div) {
        return launch_sym_fwd<D, decltype(div)::value>(a, sc, M, o, ws, wsb, st, g_fwd_alg == 4);
      });
    case FwdFamily::kMfma:
      return for_bool(w.div, [&](auto div) {
        return launch_mfma_fwd<D, decltype(div)::value>("ode_self_fwd(mfma)", a, sc, nrows, M, o, ws, wsb, st, order);
      });
    case FwdFamily::kSymRows:
      return for_bool(w.div, [&](auto div) {
        return launch_sym_fwd_rows<D, decltype(div)::value>(a, sc, M, o, ws, wsb, st, w.zs);
      });
    default:   // kScalar (the eta sums contain the divergence's)
      if (w.eta) return launch_r<OpOdeSelfFwd<D, true, true>>(r_fwd(), "ode_self_fwd", a, sc, nrows, M, o, ws, wsb, st);
      return for_bool(w.div, [&](auto div) {
        return launch_r<OpOdeSelfFwd<D, false, decltype(div)::value>>(r_fwd(), "ode_self_fwd", a, sc, nrows, M, o, ws, wsb, st);
      });
  }
}

// the workspace of every variant that ode_self_fwd_d may launch for nrows rows of M (their
// occupancies, hence splits, differ); a whole pass may run a symmetric forward
template <int D>
size_t ode_self_fwd_rows_ws(int64_t nrows, int64_t M) {
  return max_of({ws_r<OpOdeSelfFwd<D, true, true>>(r_fwd(), nrows, M),
                 ws_r<OpOdeSelfFwd<D, false, true>>(r_fwd(), nrows, M),
                 ws_r<OpOdeSelfFwd<D, false, false>>(r_fwd(), nrows, M), fwd_pk_ws<D>(nrows, M),
                 mfma_fwd_ws_bytes<D, true>(nrows, M), mfma_fwd_ws_bytes<D, false>(nrows, M),
                 nrows == M ? sym_ws_bytes(M, 3 * D) : 0});
}

// ---- the ordered (row-reduction) VJP: eta != 0 its own operator, else bwd_alg 1 or 0 ----
template <int D, class F>
auto visit_bwd_ord(bool eta, int alg, F&& f) {
  if (eta) return f(OpTag<OpOdeSelfBwdEta<D>>{});
  return alg == 1 ? f(OpTag<OpOdeSelfBwd2<D>>{}) : f(OpTag<OpOdeSelfBwd<D>>{});
}
// workspace of any VJP kernel for part 1 / nparts of M points (nparts = 1: the whole VJP);
// SymBwd and SymBwdEta: W = 2D
template <int D>
size_t ode_self_bwd_ws(int64_t M, int nparts) {
  const int64_t per = (M + nparts - 1) / nparts;
  size_t m = sym_ws_bytes(M, 2 * D, nparts);
  for (int v = 0; v < 3; ++v)   // bwd_alg 0, bwd_alg 1, eta
    visit_bwd_ord<D>(v == 2, v, [&](auto t) { m = std::max(m, ws_r<op_of<decltype(t)>>(r_bwd(), per, M)); });
  return m;
}

// Pair subset `part` of `nparts` of the VJP (row-split over ranks; the sum over parts is the
// full VJP; nparts = 1: the whole VJP, exactly the single-device kernel): symmetric kernels
// (eta = 0, and eta != 0 packed) -> the quads Q = part (mod nparts), written to all rows;
// otherwise (ordered kernels) the row slice [part * ceil(M/nparts), ...) against all columns,
// other rows zero.  Outputs of a part are plain (no epilogue).
template <int D>
int ode_self_bwd_d(const float* q, const float* p, const float* gv, const float* gmG,
                   const float* gdiv, int64_t M, double sigma, double eta, Outs o, void* ws,
                   size_t wsb, hipStream_t st, const float* zs = nullptr, int64_t zr0 = 0,
                   int64_t zn = 0, int part = 0, int nparts = 1) {
  const char* who = nparts == 1 ? "ode_self_bwd" : "ode_self_bwd_part";
  const bool has_eta = eta != 0.0;
  // gmG == NULL: zero cotangent on mG (the B0 symmetric packed kernels never read it; the
  // record slot is pointed at gv so every address stays valid)
  const bool b0 = gmG == nullptr;
  const bool pk = b0 || g_bwd_alg == 3;   // eta = 0: the packed symmetric kernel
  if (zs != nullptr && (has_eta || !pk)) {
    set_error("%s: divergence rows (zs) need eta = 0 and the packed VJP (bwd_alg 3)", who);
    return DICP_ERR_INVALID;
  }
  if (b0 && has_eta && g_bwd_eta_alg != 2) {
    set_error("%s: a NULL mG cotangent (zero) needs the packed eta kernel (bwd_eta_alg 2)", who);
    return DICP_ERR_INVALID;
  }
  const float* gb = b0 ? gv : gmG;
  Args a = {q, p, gv, gb, q, p, gv, gb, 0.f};
  Scal sc = make_scal(sigma, has_eta ? eta : 0.0);
  sc.dev0 = gdiv;  // nullptr -> aux0 = 0
  bool raw = false;
  if (!has_eta) {
    scale_coords(a, sc, sigma);
    raw = tl_coord_raw != 0 && pk;   // packed kernels only
    if (raw) raw_coords(a, sc);
  }
  if (has_eta) {   // symmetric: parts only in the packed form
    if (nparts == 1 ? g_bwd_eta_alg >= 1 : g_bwd_eta_alg == 2)
      return launch_sym_bwd_eta<D>(a, sc, M, o, ws, wsb, st, g_bwd_eta_alg == 2, part, nparts, b0);
  } else if (pk || g_bwd_alg == 2) {
    return launch_sym_bwd<D>(a, sc, M, o, ws, wsb, st, part, nparts, pk, b0, zs, zr0, zn, raw);
  }
  int64_t rows = M;
  if (nparts > 1) {   // the part's row slice, the other rows zero
    if (int rc = no_batch("ode_self_bwd_part(ordered)")) return rc;
    const int64_t per = (M + nparts - 1) / nparts;
    const int64_t r0 = std::min(per * part, M), r1 = std::min(r0 + per, M);
    if ((o.ptr[0] && hipMemsetAsync(o.ptr[0], 0, (size_t)M * D * sizeof(float), st) != hipSuccess) ||
        hipMemsetAsync(o.ptr[1], 0, (size_t)M * D * sizeof(float), st) != hipSuccess) {
      set_error("ode_self_bwd_part: hipMemsetAsync failed");
      return DICP_ERR_HIP;
    }
    if (r1 <= r0) return DICP_OK;
    rows = r1 - r0;
    const int64_t o0 = r0 * D;
    a.r0 += o0, a.r1 += o0, a.r2 += o0, a.r3 += o0;
    if (o.ptr[0]) o.ptr[0] += o0;
    o.ptr[1] += o0;
  }
  return visit_bwd_ord<D>(has_eta, g_bwd_alg, [&](auto t) {
    return launch_r<op_of<decltype(t)>>(r_bwd(), has_eta ? "ode_self_bwd_eta" : "ode_self_bwd", a, sc, rows, M, o,
                                        ws, wsb, st);
  });
}

// the external-point forward with or without the eta terms and the divergence rows gx:
// f(OpTag<scalar rows>, OpTag<packed rows>), ext_alg chooses between the two
template <int D, class F>
auto visit_ext_fwd(bool eta, bool gx, F&& f) {
  return for_bool(eta, [&](auto e) {
    return for_bool(gx, [&](auto g) {
      constexpr bool kEta = decltype(e)::value, kG = decltype(g)::value;
      return f(OpTag<OpOdeExtFwd<D, kEta, kG>>{}, OpTag<OpExtFwdPk<D, kEta, kG>>{});
    });
  });
}

template <int D>
int ode_ext_fwd_d(const float* x, int64_t N, const float* q, const float* p, int64_t M,
                  double sigma, double eta, float* vx, float* gx, void* ws, size_t wsb,
                  hipStream_t st) {
  if (cx_eligible(N, M, true)) return cx_ext_fwd(x, N, q, p, M, D, sigma, eta, vx, gx, ws, wsb, st);
  const Outs o = make_outs(vx, gx);
  const Args a = {x, nullptr, nullptr, nullptr, q, p, nullptr, nullptr};
  const Scal sc = make_scal(sigma, eta);
  return visit_ext_fwd<D>(eta != 0.0, gx != nullptr, [&](auto scalar, auto packed) {
    return g_ext_alg == 1
               ? launch_rowred_pk<op_of<decltype(packed)>>("ode_ext_fwd", a, sc, N, M, o, ws, wsb, st)
               : launch_rowred<op_of<decltype(scalar)>, kR>("ode_ext_fwd", a, sc, N, M, o, ws, wsb, st);
  });
}

template <int D>
size_t ode_ext_fwd_ws(int64_t N, int64_t M) {
  size_t m = cx_eligible(N, M, true) ? cx_ext_ws(N, M, D) : 0;
  for (int v = 0; v < 4; ++v)
    visit_ext_fwd<D>((v & 1) != 0, (v & 2) != 0, [&](auto scalar, auto packed) {
      m = std::max({m, rowred_ws_bytes<op_of<decltype(scalar)>, kR>(N, M),
                    rowred_pk_ws_bytes<op_of<decltype(packed)>>(N, M)});
    });
  return m;
}

template <int D>
int ode_ext_bwd_d(const float* x, int64_t N, const float* q, const float* p, int64_t M,
                  double sigma, double eta, const float* gvx, const float* gdiv, float* gxo,
                  float* gq, float* gp, void* ws, size_t wsb, hipStream_t st) {
  if (g_ext_alg == 1 && eta == 0.0) {
    const Args a = {x, gvx, nullptr, nullptr, q, p, nullptr, nullptr};
    Scal sc = make_scal(sigma, 0.0);
    sc.dev0 = gdiv;
    int rc = launch_rowred_pk<OpExtBwdXPk<D>>("ode_ext_bwd_x", a, sc, N, M, make_outs(gxo), ws, wsb, st);
    if (rc) return rc;
    const Args b = {q, p, nullptr, nullptr, x, gvx, nullptr, nullptr};
    Outs o = make_outs(gq, gp);
    o.accumulate[0] = o.accumulate[1] = 1;
    return launch_rowred_pk<OpExtBwdQPk<D>>("ode_ext_bwd_q", b, sc, M, N, o, ws, wsb, st);
  }
  Scal sc = make_scal(sigma, eta);
  sc.dev0 = gdiv;
  // rows x: gradient w.r.t. the carried points
  {
    const Args a = {x, gvx, nullptr, nullptr, q, p, nullptr, nullptr};
    const Outs o = make_outs(gxo);
    int rc = eta != 0.0
        ? launch_rowred<OpOdeExtBwdXEta<D>, kR>("ode_ext_bwd_x", a, sc, N, M, o, ws, wsb, st)
        : launch_rowred<OpOdeExtBwdX<D>, kR>("ode_ext_bwd_x", a, sc, N, M, o, ws, wsb, st);
    if (rc) return rc;
  }
  // rows q: gradient w.r.t. support points and momenta (accumulated)
  {
    const Args a = {q, p, nullptr, nullptr, x, gvx, nullptr, nullptr};
    Outs o = make_outs(gq, gp);
    o.accumulate[0] = o.accumulate[1] = 1;
    return eta != 0.0
        ? launch_rowred<OpOdeExtBwdQEta<D>, kR>("ode_ext_bwd_q", a, sc, M, N, o, ws, wsb, st)
        : launch_rowred<OpOdeExtBwdQ<D>, kR>("ode_ext_bwd_q", a, sc, M, N, o, ws, wsb, st);
  }
}

template <int D>
size_t ode_ext_bwd_ws(int64_t N, int64_t M) {
  size_t m = 0;
  for (size_t v : {rowred_ws_bytes<OpOdeExtBwdX<D>, kR>(N, M), rowred_ws_bytes<OpOdeExtBwdQ<D>, kR>(M, N),
                   rowred_ws_bytes<OpOdeExtBwdXEta<D>, kR>(N, M),
                   rowred_ws_bytes<OpOdeExtBwdQEta<D>, kR>(M, N),
                   rowred_pk_ws_bytes<OpExtBwdXPk<D>>(N, M), rowred_pk_ws_bytes<OpExtBwdQPk<D>>(M, N)})
    m = v > m ? v : m;
  return m;
}

}  // namespace

// ---- what the entry points below share ----
namespace {
// The forward for entry point `entry`: rows [row0, row0 + nrows) (nrows < 0: all) in `order`.
int self_fwd(const char* entry, int D, const float* q, const float* p, int64_t M, double sigma, double eta,
             const Outs& o, void* ws, size_t wsb, dicp_stream_t stream, int64_t row0 = 0, int64_t nrows = -1,
             const int32_t* order = nullptr, float* zs = nullptr) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return with_dim(D, entry, [&](auto d) {
    return ode_self_fwd_d<decltype(d)::value>(q, p, M, sigma, eta, o, ws, wsb, st, row0, nrows, order, zs);
  });
}

// Outputs of an Euler step of the rows from row0: x_next = x + dt * (the pass's rows)
Outs euler_outs(const float* q, const float* p, int64_t row0, int D, double dt, float* q_next, float* p_next,
                float* g) {
  Outs o = make_outs(q_next, p_next, g, nullptr);
  o.base[0] = q + row0 * D;
  o.base[1] = p + row0 * D;
  o.alpha[0] = o.alpha[1] = (float)dt;
  return o;
}

// The arguments of a row-slice entry: 0 <= row0, row0 + nrows <= M, sigma > 0 and, for a slice
// with rows, every pointer of `need` and no output equal to one of its `others` (NULL: skipped).
struct NoAlias {
  const float* out;
  const float* others[4];
};
int check_rows(const char* entry, int64_t M, int64_t row0, int64_t nrows, double sigma,
               std::initializer_list<const void*> need, std::initializer_list<NoAlias> no_alias = {}) {
  bool bad = M < 0 || row0 < 0 || nrows < 0 || row0 + nrows > M || !(sigma > 0);
  if (nrows > 0) {
    for (const void* ptr : need) bad = bad || ptr == nullptr;
    for (const NoAlias& n : no_alias)
      for (const float* x : n.others) bad = bad || (n.out != nullptr && n.out == x);
  }
  if (!bad) return DICP_OK;
  set_error("%s: invalid arguments%s", entry, no_alias.size() ? " (outputs must not alias inputs)" : "");
  return DICP_ERR_INVALID;
}

// p_next may be NULL: the momenta update is not wanted (the packed pass skips its Gs' / Hs /
// GL' sums); zs may be NULL (no divergence rows)
int euler_step_rows(const char* entry, const float* q, const float* p, int64_t M, int64_t row0, int64_t nrows,
                    int D, double sigma, double eta, double dt, const int32_t* row_order, float* q_next,
                    float* p_next, float* g, float* zs, void* ws, size_t ws_bytes, dicp_stream_t stream) {
  if (int rc = check_rows(entry, M, row0, nrows, sigma, {q, p, q_next},
                          {{q_next, {q, p}}, {p_next, {q, p}}, {zs, {q, p, q_next, p_next}}}))
    return rc;
  if (nrows == 0) return DICP_OK;
  return self_fwd(entry, D, q, p, M, sigma, eta, euler_outs(q, p, row0, D, dt, q_next, p_next, g), ws, ws_bytes,
                  stream, row0, nrows, row_order, zs);
}

// lq_next may be NULL: only lp_next is produced (the gq half of the eta = 0 symmetric VJP is
// then never evaluated -- the last adjoint step when the start points need no gradient).
// lp may be NULL: a zero cotangent on the momenta (the first adjoint step when the loss does
// not depend on the final momenta; eta = 0), the b terms of the VJP are then skipped.
// zs may be NULL (no divergence rows).
int euler_adjoint_step(const char* entry, const float* q, const float* p, const float* lq, const float* lp,
                       const float* gdiv, int64_t M, int D, double sigma, double eta, double dt,
                       const float* addq, const float* addp, const float* zs, float* lq_next, float* lp_next,
                       void* ws, size_t ws_bytes, dicp_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  bool alias = false;
  for (const float* x : {q, p, lq, lp, zs}) alias = alias || (x && ((lq_next && x == lq_next) || x == lp_next));
  if (M < 0 || (M > 0 && (!q || !p || !lq || !lp_next || alias)) || !(sigma > 0)) {
    set_error("%s: invalid arguments (outputs must not alias inputs)", entry);
    return DICP_ERR_INVALID;
  }
  Outs o = make_outs(lq_next, lp_next);
  o.base[0] = lq;
  o.base[1] = lp;
  o.add[0] = addq;
  o.add[1] = addp;
  o.alpha[0] = o.alpha[1] = (float)dt;
  return with_dim(D, entry, [&](auto d) {
    return ode_self_bwd_d<decltype(d)::value>(q, p, lq, lp, gdiv, M, sigma, eta, o, ws, ws_bytes, st, zs, 0, M);
  });
}

// gq may be NULL (gp only), gmG NULL = zero cotangent; zs: divergence rows [zrow0, zrow0 + znrows)
int self_bwd_part(const char* entry, const float* q, const float* p, const float* gv, const float* gmG,
                  const float* gdiv, int64_t M, int D, double sigma, double eta, int part, int nparts,
                  const float* zs, int64_t zrow0, int64_t znrows, float* gq, float* gp, void* ws,
                  size_t ws_bytes, dicp_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (M < 0 || nparts < 1 || part < 0 || part >= nparts || (M > 0 && (!q || !p || !gv || !gp)) ||
      !(sigma > 0) || (zs && (zrow0 < 0 || znrows < 0 || zrow0 + znrows > M))) {
    set_error("%s: invalid arguments", entry);
    return DICP_ERR_INVALID;
  }
  if (M == 0) return DICP_OK;
  return with_dim(D, entry, [&](auto d) {
    return ode_self_bwd_d<decltype(d)::value>(q, p, gv, gmG, gdiv, M, sigma, eta, make_outs(gq, gp), ws, ws_bytes,
                                              st, zs, zrow0, znrows, part, nparts);
  });
}
}  // namespace

extern "C" int dicp_lddmm_ode_self_fwd_f32(const float* q, const float* p, int64_t M, int D,
                                           double sigma, double eta, float* v, float* mG,
                                           float* g, float* h, void* ws, size_t ws_bytes,
                                           dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  if (M < 0 || (M > 0 && (!q || !p || !v || !mG)) || !(sigma > 0)) {
    set_error("dicp_lddmm_ode_self_fwd_f32: invalid arguments");
    return DICP_ERR_INVALID;
  }
  return self_fwd("dicp_lddmm_ode_self_fwd_f32", D, q, p, M, sigma, eta, make_outs(v, mG, g, h), ws, ws_bytes,
                  stream);
}

extern "C" int dicp_lddmm_ode_self_bwd_f32(const float* q, const float* p, const float* gv,
                                           const float* gmG, const float* gdiv, int64_t M,
                                           int D, double sigma, double eta, float* gq,
                                           float* gp, void* ws, size_t ws_bytes,
                                           dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (M < 0 || (M > 0 && (!q || !p || !gv || !gp)) || !(sigma > 0)) {  // gmG NULL = zero (eta = 0)
    set_error("dicp_lddmm_ode_self_bwd_f32: invalid arguments");
    return DICP_ERR_INVALID;
  }
  return with_dim(D, "dicp_lddmm_ode_self_bwd_f32", [&](auto d) {
    return ode_self_bwd_d<decltype(d)::value>(q, p, gv, gmG, gdiv, M, sigma, eta, make_outs(gq, gp), ws, ws_bytes,
                                              st);
  });
}

// One explicit-Euler step of the shooting ODE with the state update fused into the
// reduction's epilogue: q_next = q + dt v(q,p), p_next = p + dt mG(q,p), g rows as in
// dicp_lddmm_ode_self_fwd_f32 (integrators.py:20-33 EulerIntegrator over LDDMM.py:176-227).
extern "C" int dicp_lddmm_euler_step_f32(const float* q, const float* p, int64_t M, int D,
                                         double sigma, double eta, double dt, float* q_next,
                                         float* p_next, float* g, void* ws, size_t ws_bytes,
                                         dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  if (M < 0 || (M > 0 && (!q || !p || !q_next || !p_next)) || !(sigma > 0) ||
      (M > 0 && (q_next == q || q_next == p || p_next == q || p_next == p))) {
    set_error("dicp_lddmm_euler_step_f32: invalid arguments (outputs must not alias inputs)");
    return DICP_ERR_INVALID;
  }
  return self_fwd("dicp_lddmm_euler_step_f32", D, q, p, M, sigma, eta,
                  euler_outs(q, p, 0, D, dt, q_next, p_next, g), ws, ws_bytes, stream);
}

// The matching adjoint step (exact discrete adjoint of the Euler step):
//   lq_next = lq + dt * d/dq[lq.v + lp.mG + gdiv sum g] + addq,
//   lp_next = lp + dt * d/dp[...]                        + addp
// (addq / addp: the loss's own cotangent on the state at this time, or NULL).
extern "C" int dicp_lddmm_euler_adjoint_step_zs_f32(const float* q, const float* p, const float* lq,
                                                    const float* lp, const float* gdiv, int64_t M,
                                                    int D, double sigma, double eta, double dt,
                                                    const float* addq, const float* addp,
                                                    const float* zs, float* lq_next, float* lp_next,
                                                    void* ws, size_t ws_bytes, dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  return euler_adjoint_step("dicp_lddmm_euler_adjoint_step_zs_f32", q, p, lq, lp, gdiv, M, D, sigma, eta, dt, addq,
                            addp, zs, lq_next, lp_next, ws, ws_bytes, stream);
}

extern "C" int dicp_lddmm_euler_adjoint_step_f32(const float* q, const float* p, const float* lq,
                                                 const float* lp, const float* gdiv, int64_t M,
                                                 int D, double sigma, double eta, double dt,
                                                 const float* addq, const float* addp,
                                                 float* lq_next, float* lp_next, void* ws,
                                                 size_t ws_bytes, dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  return euler_adjoint_step("dicp_lddmm_euler_adjoint_step_f32", q, p, lq, lp, gdiv, M, D, sigma, eta, dt, addq,
                            addp, nullptr, lq_next, lp_next, ws, ws_bytes, stream);
}

extern "C" int dicp_lddmm_ode_ext_fwd_f32(const float* x, int64_t N, const float* q,
                                          const float* p, int64_t M, int D, double sigma,
                                          double eta, float* vx, float* gx, void* ws,
                                          size_t ws_bytes, dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (N < 0 || M < 0 || (N > 0 && (!x || !vx)) || (M > 0 && (!q || !p)) || !(sigma > 0)) {
    set_error("dicp_lddmm_ode_ext_fwd_f32: invalid arguments");
    return DICP_ERR_INVALID;
  }
  return with_dim(D, "dicp_lddmm_ode_ext_fwd_f32", [&](auto d) {
    return ode_ext_fwd_d<decltype(d)::value>(x, N, q, p, M, sigma, eta, vx, gx, ws, ws_bytes, st);
  });
}

extern "C" int dicp_lddmm_ode_ext_bwd_f32(const float* x, int64_t N, const float* q,
                                          const float* p, int64_t M, int D, double sigma,
                                          double eta, const float* gvx, const float* gdiv,
                                          float* gxo, float* gq, float* gp, void* ws,
                                          size_t ws_bytes, dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (N < 0 || M < 0 || (N > 0 && (!x || !gvx || !gxo)) || (M > 0 && (!q || !p || !gq || !gp)) ||
      !(sigma > 0)) {
    set_error("dicp_lddmm_ode_ext_bwd_f32: invalid arguments");
    return DICP_ERR_INVALID;
  }
  return with_dim(D, "dicp_lddmm_ode_ext_bwd_f32", [&](auto d) {
    return ode_ext_bwd_d<decltype(d)::value>(x, N, q, p, M, sigma, eta, gvx, gdiv, gxo, gq, gp, ws, ws_bytes, st);
  });
}

// Row-split (multi-GPU single frame): rows [row0, row0 + nrows) of the fused
// forward against all M columns; outputs address the slice (nrows rows).
extern "C" int dicp_lddmm_ode_self_fwd_rows_f32(const float* q, const float* p, int64_t M,
                                                int64_t row0, int64_t nrows, int D,
                                                double sigma, double eta, float* v, float* mG,
                                                float* g, float* h, void* ws, size_t ws_bytes,
                                                dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  const char* entry = "dicp_lddmm_ode_self_fwd_rows_f32";
  if (int rc = check_rows(entry, M, row0, nrows, sigma, {q, p, v, mG})) return rc;
  if (nrows == 0) return DICP_OK;
  return self_fwd(entry, D, q, p, M, sigma, eta, make_outs(v, mG, g, h), ws, ws_bytes, stream, row0, nrows);
}

extern "C" int dicp_lddmm_euler_step_rows_f32(const float* q, const float* p, int64_t M,
                                              int64_t row0, int64_t nrows, int D, double sigma,
                                              double eta, double dt, float* q_next,
                                              float* p_next, float* g, void* ws,
                                              size_t ws_bytes, dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  const char* entry = "dicp_lddmm_euler_step_rows_f32";
  if (int rc = check_rows(entry, M, row0, nrows, sigma, {q, p, q_next, p_next})) return rc;
  if (nrows == 0) return DICP_OK;
  return self_fwd(entry, D, q, p, M, sigma, eta, euler_outs(q, p, row0, D, dt, q_next, p_next, g), ws, ws_bytes,
                  stream, row0, nrows);
}

// Ordered forms (rows [row0, row0 + nrows) visited in row_order, or NULL = natural order):
// the general entry points behind the four above.
extern "C" int dicp_lddmm_ode_self_fwd_zs_f32(const float* q, const float* p, int64_t M, int64_t row0,
                                              int64_t nrows, int D, double sigma, double eta,
                                              const int32_t* row_order, float* v, float* mG, float* g,
                                              float* zs, void* ws, size_t ws_bytes, dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  const char* entry = "dicp_lddmm_ode_self_fwd_zs_f32";
  if (int rc = check_rows(entry, M, row0, nrows, sigma, {q, p, v, mG, zs})) return rc;
  if (nrows == 0) return DICP_OK;
  return self_fwd(entry, D, q, p, M, sigma, eta, make_outs(v, mG, g, nullptr), ws, ws_bytes, stream, row0, nrows,
                  row_order, zs);
}

extern "C" int dicp_lddmm_ode_self_fwd_ord_f32(const float* q, const float* p, int64_t M,
                                               int64_t row0, int64_t nrows, int D, double sigma,
                                               double eta, const int32_t* row_order, float* v,
                                               float* mG, float* g, float* h, void* ws,
                                               size_t ws_bytes, dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  const char* entry = "dicp_lddmm_ode_self_fwd_ord_f32";
  if (int rc = check_rows(entry, M, row0, nrows, sigma, {q, p, v, mG})) return rc;
  if (nrows == 0) return DICP_OK;
  return self_fwd(entry, D, q, p, M, sigma, eta, make_outs(v, mG, g, h), ws, ws_bytes, stream, row0, nrows,
                  row_order);
}

extern "C" int dicp_lddmm_euler_step_zs_f32(const float* q, const float* p, int64_t M, int64_t row0,
                                            int64_t nrows, int D, double sigma, double eta, double dt,
                                            const int32_t* row_order, float* q_next, float* p_next,
                                            float* g, float* zs, void* ws, size_t ws_bytes,
                                            dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  return euler_step_rows("dicp_lddmm_euler_step_zs_f32", q, p, M, row0, nrows, D, sigma, eta, dt, row_order, q_next,
                         p_next, g, zs, ws, ws_bytes, stream);
}

extern "C" int dicp_lddmm_euler_step_ord_f32(const float* q, const float* p, int64_t M,
                                             int64_t row0, int64_t nrows, int D, double sigma,
                                             double eta, double dt, const int32_t* row_order,
                                             float* q_next, float* p_next, float* g, void* ws,
                                             size_t ws_bytes, dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  return euler_step_rows("dicp_lddmm_euler_step_ord_f32", q, p, M, row0, nrows, D, sigma, eta, dt, row_order, q_next,
                         p_next, g, nullptr, ws, ws_bytes, stream);
}

// ---- the fused steps with the Gaussian cutoff of far tile pairs (lddmm_sym.hpp kCutTile) ----
// boxes: dicp_pair_boxes_f32 of q (ceil(M / 64) x 2D floats), or NULL = the dense entry above,
// bit for bit.  With boxes the symmetric 4 / 6 / 8-row forward and the 4-row packed VJP skip far
// (row group, 64-column sub-tile) pairs; a pass that runs another kernel (the ordered rows below
// the symmetric forward's size, the mG-less last step, the 2-row VJP) ignores them.  Whole
// passes, eta = 0, scaled coordinates (not coord_raw), outside launch batches.
namespace {
int cut_check(const char* what, const float* boxes, double eta) {
  if (boxes == nullptr) return DICP_OK;
  if (eta != 0.0 || tl_coord_raw != 0 || batching()) {
    set_error("%s: boxes need eta = 0, scaled coordinates and no launch batch", what);
    return DICP_ERR_INVALID;
  }
  return DICP_OK;
}
template <int D>
int pair_boxes_d(const float* q, int64_t M, double sigma, float* boxes, hipStream_t st) {
  Args a = {nullptr, nullptr, nullptr, nullptr, q, nullptr, nullptr, nullptr, 0.f};
  Scal sc = make_scal(sigma, 0.0);
  scale_coords(a, sc, sigma);
  return launch_pair_boxes<D>(a, M, boxes, st);
}
}  // namespace

extern "C" int dicp_pair_boxes_f32(const float* q, int64_t M, int D, double sigma, float* boxes,
                                   dicp_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (M < 0 || (M > 0 && (!q || !boxes)) || !(sigma > 0)) {
    set_error("dicp_pair_boxes_f32: invalid arguments");
    return DICP_ERR_INVALID;
  }
  return with_dim(D, "dicp_pair_boxes_f32",
                  [&](auto d) { return pair_boxes_d<decltype(d)::value>(q, M, sigma, boxes, st); });
}

extern "C" int dicp_lddmm_ode_self_fwd_box_f32(const float* q, const float* p, int64_t M, int D, double sigma,
                                               double eta, float* v, float* mG, float* g, float* zs,
                                               const float* boxes, void* ws, size_t ws_bytes,
                                               dicp_stream_t stream) {
  if (int rc = cut_check("dicp_lddmm_ode_self_fwd_box_f32", boxes, eta)) return rc;
  dicp::CutScope cut_(boxes);
  if (zs != nullptr)
    return dicp_lddmm_ode_self_fwd_zs_f32(q, p, M, 0, M, D, sigma, eta, nullptr, v, mG, g, zs, ws, ws_bytes, stream);
  return dicp_lddmm_ode_self_fwd_ord_f32(q, p, M, 0, M, D, sigma, eta, nullptr, v, mG, g, nullptr, ws, ws_bytes,
                                         stream);
}

extern "C" int dicp_lddmm_euler_step_box_f32(const float* q, const float* p, int64_t M, int D, double sigma,
                                             double eta, double dt, float* q_next, float* p_next, float* g,
                                             float* zs, const float* boxes, float* boxes_next, void* ws,
                                             size_t ws_bytes, dicp_stream_t stream) {
  if (int rc = cut_check("dicp_lddmm_euler_step_box_f32", boxes, eta)) return rc;
  {
    dicp::CutScope cut_(boxes);
    if (int rc = dicp_lddmm_euler_step_zs_f32(q, p, M, 0, M, D, sigma, eta, dt, nullptr, q_next, p_next, g, zs, ws,
                                              ws_bytes, stream))
      return rc;
  }
  // the new state's boxes, on the same stream after the step's merge wrote q_next
  return boxes_next != nullptr ? dicp_pair_boxes_f32(q_next, M, D, sigma, boxes_next, stream) : DICP_OK;
}

extern "C" int dicp_lddmm_euler_adjoint_step_box_f32(const float* q, const float* p, const float* lq,
                                                     const float* lp, const float* gdiv, int64_t M, int D,
                                                     double sigma, double eta, double dt, const float* addq,
                                                     const float* addp, const float* zs, const float* boxes,
                                                     float* lq_next, float* lp_next, void* ws, size_t ws_bytes,
                                                     dicp_stream_t stream) {
  if (int rc = cut_check("dicp_lddmm_euler_adjoint_step_box_f32", boxes, eta)) return rc;
  dicp::CutScope cut_(boxes);
  return dicp_lddmm_euler_adjoint_step_zs_f32(q, p, lq, lp, gdiv, M, D, sigma, eta, dt, addq, addp, zs, lq_next,
                                              lp_next, ws, ws_bytes, stream);
}

// A row-split Euler step in two column phases (core/shooting.py, RowSplit.overlap): phase 0
// runs the rank's rows against its own slice -- the rows' values, which the rank holds before
// the all-gather of the step's input has landed -- into the first partial slots of `ws`;
// phase 1 runs them against the other M - nrows points (the wrapped column range from
// row0 + nrows) into the remaining slots and merges all slots once, with the Euler epilogue.
// The two calls must see the same sizes, output pointers (which select the pass) and `ws`.
// The pair operators' stores are linear in the column sums, so the result is the one-pass
// step's up to fp32 summation order (and the coordinate origin of each phase: its first
// column point).  Ordered packed passes (fwd_alg 2, 5, 6); zs needs eta = 0.
namespace {
template <int D>
int euler_step_phase_d(int phase, const float* q_loc, const float* p_loc, const float* q, const float* p, int64_t M,
                       int64_t row0, int64_t nrows, double sigma, double eta, const Outs& o, void* ws, size_t wsb,
                       hipStream_t st) {
  // phase 0: rows = columns = the local slice, read in place; phase 1: rows = the slice of
  // (q, p), columns = all of (q, p) read from row0 + nrows on (wrapping), M - nrows of them
  Args a = {q_loc, p_loc, nullptr, nullptr, q_loc, p_loc, nullptr, nullptr, 0.f};
  if (phase == 1) a = {q + row0 * D, p + row0 * D, nullptr, nullptr, q, p, nullptr, nullptr, 0.f};
  Scal sc = make_scal(sigma, eta);
  const PkFwd v = {o.ptr[2] != nullptr, eta != 0.0, o.ptr[1] != nullptr, o.ptr[3] != nullptr, tl_coord_raw != 0};
  scale_coords(a, sc, sigma);
  if (v.raw) raw_coords(a, sc);
  const int64_t coff = phase == 0 || row0 + nrows >= M ? 0 : row0 + nrows;
  return visit_pk_fwd<D>(v, [&](auto t) {
    return launch_pk_phase<op_of<decltype(t)>>("ode_self_fwd(pk, phase)", phase, a, sc, nrows, nrows, M - nrows, coff,
                                               phase == 0 ? nrows : M, o, ws, wsb, st);
  });
}

template <int D>
size_t euler_step_phase_ws(int64_t nrows, int64_t M) {
  size_t m = 0;
  for_each_pk_fwd<D>(
      [&](auto t) { m = std::max(m, pk_phase_ws_bytes<op_of<decltype(t)>>(nrows, nrows, M - nrows)); });
  return m;
}
}  // namespace

extern "C" int dicp_lddmm_euler_step_phase_f32(int phase, const float* q_loc, const float* p_loc, const float* q,
                                               const float* p, int64_t M, int64_t row0, int64_t nrows, int D,
                                               double sigma, double eta, double dt, float* q_next, float* p_next,
                                               float* g, float* zs, void* ws, size_t ws_bytes,
                                               dicp_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  auto overlaps = [](const float* out, int64_t n_out, const float* in, int64_t n_in) {
    return out && in && out < in + n_in && in < out + n_out;
  };
  bool bad = (phase != 0 && phase != 1) || M < 0 || row0 < 0 || nrows < 0 || row0 + nrows > M ||
             (nrows > 0 && nrows == M) || !(sigma > 0) || (nrows > 0 && !q_next) || (zs && eta != 0.0) ||
             (nrows > 0 && phase == 0 && (!q_loc || !p_loc)) || (nrows > 0 && phase == 1 && (!q || !p));
  // outputs (phase 1 writes them) must not overlap (q, p); they may be the local slice's
  // buffers, which only phase 0 reads
  const float* outs_[4] = {q_next, p_next, g, zs};
  const int64_t w_[4] = {D, D, 1, D};
  for (int k = 0; k < 4 && !bad && phase == 1; ++k) {
    const int64_t n = nrows * w_[k];
    bad = overlaps(outs_[k], n, q, M * D) || overlaps(outs_[k], n, p, M * D);
  }
  if (bad) {
    set_error("dicp_lddmm_euler_step_phase_f32: invalid arguments (phase 0/1, 0 <= nrows < M, outputs must "
              "not overlap the inputs, zs needs eta = 0)");
    return DICP_ERR_INVALID;
  }
  if (!packed_fwd_alg(g_fwd_alg)) {
    set_error("dicp_lddmm_euler_step_phase_f32: needs an ordered packed forward (fwd_alg 2, 5 or 6)");
    return DICP_ERR_UNSUPPORTED;
  }
  if (nrows == 0) return DICP_OK;
  Outs o = make_outs(q_next, p_next, g, zs);
  o.alpha[0] = o.alpha[1] = (float)dt;
  if (phase == 1) {
    o.base[0] = q + row0 * D;
    o.base[1] = p_next ? p + row0 * D : nullptr;
  }
  return with_dim(D, "dicp_lddmm_euler_step_phase_f32", [&](auto d) {
    return euler_step_phase_d<decltype(d)::value>(phase, q_loc, p_loc, q, p, M, row0, nrows, sigma, eta, o, ws,
                                                  ws_bytes, st);
  });
}

extern "C" int dicp_lddmm_ode_self_bwd_part_zs_f32(const float* q, const float* p, const float* gv,
                                                   const float* gmG, const float* gdiv, int64_t M,
                                                   int D, double sigma, double eta, int part,
                                                   int nparts, const float* zs, int64_t zrow0,
                                                   int64_t znrows, float* gq, float* gp, void* ws,
                                                   size_t ws_bytes, dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  return self_bwd_part("dicp_lddmm_ode_self_bwd_part_zs_f32", q, p, gv, gmG, gdiv, M, D, sigma, eta, part, nparts,
                       zs, zrow0, znrows, gq, gp, ws, ws_bytes, stream);
}

extern "C" int dicp_lddmm_ode_self_bwd_part_f32(const float* q, const float* p, const float* gv,
                                                const float* gmG, const float* gdiv, int64_t M,
                                                int D, double sigma, double eta, int part,
                                                int nparts, float* gq, float* gp, void* ws,
                                                size_t ws_bytes, dicp_stream_t stream) {
  dicp::BatchCall batch_call_;  // a call of a launch batch (batch.hpp)
  return self_bwd_part("dicp_lddmm_ode_self_bwd_part_f32", q, p, gv, gmG, gdiv, M, D, sigma, eta, part, nparts,
                       nullptr, 0, 0, gq, gp, ws, ws_bytes, stream);
}

// Workspace sizes for the LDDMM entries (the GMM ones live in gmm.hip).
size_t dicp_lddmm_ws(int kind, int64_t M, int64_t N, int D) {
  if (!supported_dim(D)) return 0;
  return for_dim(D, [&](auto d) -> size_t {
    constexpr int kD = decltype(d)::value;
    switch (kind) {
      case DICP_WS_RED: {
        size_t m = max_of({red_ws<OpKBase>(D, M, N), red_ws<OpKRed>(D, M, N), red_ws<OpGradK>(D, M, N),
                           red_ws<OpGenDK>(D, M, N), red_ws<OpHessK>(D, M, N), red_ws<OpLapK>(D, M, N),
                           red_ws<OpGradLapKPlain>(D, M, N), red_ws<OpGradKScal>(D, M, N),
                           red_ws<OpMinSqDist>(D, M, N), red_ws<OpZDotB>(D, M, N), red_ws<OpDDK>(D, M, N),
                           red_ws<OpKRedScal>(D, M, N), red_ws<OpGradLapKScal>(D, M, N),
                           red_ws<OpMinSqDistOther>(D, M, N), red_ws<OpRadiusCount>(D, M, N),
                           rowred_pk_ws_bytes<OpExtFwdPk<kD, false, false>>(M, N)});
        if (cx_eligible(M, N) || (M == N && sym_red() == 2))   // (sym_red 2: x = y forced)
          m = std::max(m, cx_red_ws(M, N, D));
        return m;
      }
      case DICP_WS_ODE_SELF_FWD: return ode_self_fwd_rows_ws<kD>(M, M);
      case DICP_WS_ODE_SELF_BWD: return ode_self_bwd_ws<kD>(M, 1);
      case DICP_WS_ODE_EXT_FWD: return ode_ext_fwd_ws<kD>(N, M);
      case DICP_WS_ODE_EXT_BWD: return ode_ext_bwd_ws<kD>(N, M);
      case DICP_WS_ODE_SELF_FWD_ROWS: return ode_self_fwd_rows_ws<kD>(M, N);
      case DICP_WS_ODE_SELF_FWD_PHASED: return M <= 0 || M >= N ? 0 : euler_step_phase_ws<kD>(M, N);
      case DICP_WS_ODE_SELF_BWD_PART: return ode_self_bwd_ws<kD>(M, N < 1 ? 1 : (int)N);
      default: return 0;
    }
  });
}

// Diagnostics: the column splits of the D = 3 ordered operators.
int dicp_lddmm_splits(int kind, int64_t M, int64_t N) {
  switch (kind) {
    case DICP_WS_ODE_SELF_BWD:
      return visit_bwd_ord<3>(false, g_bwd_alg, [&](auto t) {
        return for_rows(r_bwd(), [&](auto r) { return rowred_splits<op_of<decltype(t)>, decltype(r)::value>(M, M); });
      });
    case DICP_WS_ODE_SELF_FWD:
      return for_rows(r_fwd(), [&](auto r) {
        return rowred_splits<OpOdeSelfFwd<3, false, true>, decltype(r)::value>(M, M);
      });
    default: return rowred_splits<OpKRed<3>, kR>(M, N);
  }
}
