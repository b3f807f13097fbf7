// Second-order operator of the eta = 0 LDDMM ODE for gfx950: what the second-order adjoint of the
// shooting (core/LDDMM.py loss_hvp) needs beside the VJP and the tangent-linear model.  With the
// Hamiltonian H(q, p) = 1/2 sum_ij K_ij p_i.p_j, the VJP and the TLM are both D^2 H(S)[a, .]; this
// is its derivative T(S; a, b) = grad_S (D^2 H(S)[a, b]) along a shared direction a = (a_q, a_p)
// and L directions b_l = (b_q, b_p)_l, plus -- where the cost channel of the hybrid model is on --
// gdiv times the Hessian-vector product D^2 C(S) b_l of the divergence sum
// C(q, p) = s sum_ij K_ij (q_i - q_j).p_j.  One packed row reduction (packed.hpp rowred_pk_body,
// coordinates in original units as tlm.hip).  With s = 1/sigma^2, z = q_i - q_j,
// K = exp(-s |z|^2 / 2) (one exp2 per pair), alpha = a_q,i - a_q,j, beta = b_q,i - b_q,j and
//   P = p_i.p_j,  P_a = a_p,i.p_j + p_i.a_p,j,  P_b = b_p,i.p_j + p_i.b_p,j,
//   P_ab = a_p,i.b_p,j + b_p,i.a_p,j,  A = s^2 (z.alpha)(z.beta) - s (alpha.beta),
//   c = A P - s (z.alpha) P_b - s (z.beta) P_a + P_ab:
//
//   T_p,i = sum_j K { A p_j - s (z.alpha) b_p,j - s (z.beta) a_p,j }
//   T_q,i = sum_j K { -s c z + [s^2 (z.beta) P - s P_b] alpha + [s^2 (z.alpha) P - s P_a] beta }
//
// and, with u = p_i - p_j, du = b_p,i - b_p,j, e = s (z.beta)(z.u) - beta.u - z.du:
//
//   (D^2 C b)_p,i = s sum_j K [ s (z.beta) z - beta ]
//   (D^2 C b)_q,i = s sum_j K { -s e z + s (z.u) beta + s (z.beta) u - du }
//
// Outputs out_q, out_p (L, M, D) = T(S; a, b_l) + gdiv D^2 C(S) b_l.  The accumulators are
// out_q / s (D) | out_p (D) per row; gdiv is folded into the pair coefficients, so the cost terms
// add no accumulator.  The diagonal j = i contributes nothing (z = alpha = beta = u = du = 0).
// Rows and columns are the same six arrays (q, p, a_q, a_p, b_q, b_p): column records are 6 D
// floats in whole float4s -- D = 3: 18 floats in 5 float4s, so the double-buffered 256-column
// tiles take 40 KB of LDS (D = 2: 24 KB).  One row pair per thread: the row state alone is 6 D
// packed registers.  Directions, column chunks and merge: tlm_pass.hpp.
#include "tlm_pass.hpp"

using namespace dicp;

namespace {

template <int D>
struct OpHvpS {
  static constexpr int CW4 = cw4(6 * D);
  static constexpr int NACC = 2 * D;
  static constexpr int kNOut = 2;
  static constexpr int kOutW[4] = {D, D, 0, 0};
  static constexpr bool kMin = false;
  using Row = NoRow;   // the store needs nothing of the row
  // rows = columns: r0..r3 = (q, p, a_q, a_p), c0, c1 = (b_q, b_p) of the direction
  __device__ static void load_col(const Args& a, int64_t j, float* rec) {
    ld<D>(a.r0, j, rec);
    ld<D>(a.r1, j, rec + D);
    ld<D>(a.r2, j, rec + 2 * D);
    ld<D>(a.r3, j, rec + 3 * D);
    ld<D>(a.c0, j, rec + 4 * D);
    ld<D>(a.c1, j, rec + 5 * D);
#pragma unroll
    for (int k = 6 * D; k < 4 * CW4; ++k) rec[k] = 0.f;
  }
  __device__ static void store(const Scal& sc, const Row&, const float* t, float* v) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      v[d] = sc.s * t[d];
      v[D + d] = t[D + d];
    }
  }
};

// COST: the gdiv D^2 C b terms (Scal::dev0 = gdiv, read into aux0 at kernel start)
template <int D, bool COST>
struct OpHvpPk {
  using Base = OpHvpS<D>;
  static constexpr int kRP = 1;
  static constexpr int CW4 = Base::CW4;
  static constexpr int NACC = Base::NACC;
  static constexpr int kNOut = Base::kNOut;
  static constexpr bool kMin = false;
  struct Row2 { f2 q[D], p[D], aq[D], ap[D], bq[D], bp[D]; f2 nc, s, g, gs; };
  __device__ static void load_rows_s(const Args& a, const Scal& sc, int64_t i0, int64_t i1, Row2& r, NoRow&,
                                     NoRow&) {
    ld_rows2<D>(a.r0, i0, i1, r.q);
    ld_rows2<D>(a.r1, i0, i1, r.p);
    ld_rows2<D>(a.r2, i0, i1, r.aq);
    ld_rows2<D>(a.r3, i0, i1, r.ap);
    ld_rows2<D>(a.c0, i0, i1, r.bq);
    ld_rows2<D>(a.c1, i0, i1, r.bp);
    r.nc = splat(sc.nc);
    r.s = splat(sc.s);
    r.g = splat(sc.aux0);
    r.gs = splat(sc.aux0 * sc.s);
  }
  __device__ static void pair2(const Row2& r, const float* rec, f2* acc) {
    f2 z[D], al[D], be[D];
    f2 r2 = splat(0.f), za = splat(0.f), zb = splat(0.f), ab = splat(0.f);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      z[d] = r.q[d] - splat(rec[d]);
      al[d] = r.aq[d] - splat(rec[2 * D + d]);
      be[d] = r.bq[d] - splat(rec[4 * D + d]);
      r2 = pk_fma(z[d], z[d], r2);
      za = pk_fma(z[d], al[d], za);
      zb = pk_fma(z[d], be[d], zb);
      ab = pk_fma(al[d], be[d], ab);
    }
    const f2 e2 = r.nc * r2;
    const f2 K = f2{fast_exp2(e2.x), fast_exp2(e2.y)};
    const f2 sza = r.s * za, szb = r.s * zb;
    const f2 A = pk_fma(sza, szb, -(r.s * ab));
    f2 P = splat(0.f), Pa = splat(0.f), Pb = splat(0.f), Pab = splat(0.f);
    const f2 Kgs = K * r.gs;     // COST: out_p += gdiv s K [s (z.beta) z - beta]
    const f2 Kp = Kgs * szb;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const f2 pj = splat(rec[D + d]), apj = splat(rec[3 * D + d]), bpj = splat(rec[5 * D + d]);
      P = pk_fma(r.p[d], pj, P);
      Pa = pk_fma(r.ap[d], pj, pk_fma(r.p[d], apj, Pa));
      Pb = pk_fma(r.bp[d], pj, pk_fma(r.p[d], bpj, Pb));
      Pab = pk_fma(r.ap[d], bpj, pk_fma(r.bp[d], apj, Pab));
      const f2 t = pk_fma(A, pj, pk_fma(-sza, bpj, -(szb * apj)));
      acc[D + d] = pk_fma(K, t, acc[D + d]);
      if constexpr (COST) acc[D + d] = pk_fma(Kp, z[d], pk_fma(-Kgs, be[d], acc[D + d]));
    }
    const f2 c = pk_fma(A, P, pk_fma(-sza, Pb, pk_fma(-szb, Pa, Pab)));
    f2 Kc = K * c;                           // out_q / s: -Kc z + Kca alpha + Kcb beta
    const f2 Kca = K * pk_fma(szb, P, -Pb);
    f2 Kcb = K * pk_fma(sza, P, -Pa);
    if constexpr (COST) {
      f2 u[D], du[D];
      f2 zu = splat(0.f), bu = splat(0.f), zdu = splat(0.f);
#pragma unroll
      for (int d = 0; d < D; ++d) {
        u[d] = r.p[d] - splat(rec[D + d]);
        du[d] = r.bp[d] - splat(rec[5 * D + d]);
        zu = pk_fma(z[d], u[d], zu);
        bu = pk_fma(be[d], u[d], bu);
        zdu = pk_fma(z[d], du[d], zdu);
      }
      const f2 e = pk_fma(szb, zu, -bu) - zdu;
      const f2 Kg = K * r.g;
      Kc = pk_fma(Kg, r.s * e, Kc);
      Kcb = pk_fma(Kg, r.s * zu, Kcb);
      const f2 Kgb = Kg * szb;
#pragma unroll
      for (int d = 0; d < D; ++d) acc[d] = pk_fma(Kgb, u[d], pk_fma(-Kg, du[d], acc[d]));
    }
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = pk_fma(-Kc, z[d], pk_fma(Kca, al[d], pk_fma(Kcb, be[d], acc[d])));
  }
};

template <int D>
int hvp_d(const char* name, const float* q, const float* p, const float* aq, const float* ap, const float* bq,
          const float* bp, int64_t M, int L, double sigma, const float* gdiv, float* out_q, float* out_p, void* ws,
          hipStream_t st) {
  Scal sc = make_scal(sigma, 0.0);
  sc.dev0 = gdiv;
  const int64_t md = M * D;
  const Args a = {q, p, aq, ap, bq, bp, nullptr, nullptr, 0.f, nullptr};
  const TlmDir dir = {{0, 0, 0, 0}, {md, md, 0, 0}, {0, 0, 0, 0}};
  const Outs fin = make_outs(out_q, out_p);
  // always one row pair per thread (kRP): option "pk_rp" does not apply
  if (gdiv != nullptr) return tlm_launch_rp<OpHvpPk<D, true>, 1>(name, a, sc, M, M, L, dir, fin, ws, st);
  return tlm_launch_rp<OpHvpPk<D, false>, 1>(name, a, sc, M, M, L, dir, fin, ws, st);
}

}  // namespace

// dicp_num_splits(DICP_WS_ODE_HVP, M support points, .): the column chunks, those of the TLM
int dicp_hvp_splits(int64_t M, int64_t) { return tlm_splits(M); }

// dicp_workspace_bytes(DICP_WS_ODE_HVP, M, ., D): the partial slabs (out_q | out_p) of ONE
// direction; a call with L directions needs L times as much
size_t dicp_hvp_ws(int64_t M, int64_t, int D) {
  if ((D != 2 && D != 3) || M <= 0) return 0;
  return tlm_slab_bytes(M, 2 * M, D);
}

extern "C" int dicp_lddmm_ode_hvp_f32(const float* q, const float* p, const float* aq, const float* ap,
                                      const float* bq, const float* bp, int64_t M, int L, int D, double sigma,
                                      const float* gdiv, float* out_q, float* out_p, void* ws, size_t ws_bytes,
                                      dicp_stream_t stream) {
  const char* name = "dicp_lddmm_ode_hvp_f32";
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (M < 0 || L < 0 || L > kMaxDirs || !(sigma > 0)) {
    set_error("%s: invalid arguments (M = %lld: >= 0; L = %d: 0 ... %d; sigma = %g: > 0)", name, (long long)M, L,
              kMaxDirs, sigma);
    return DICP_ERR_INVALID;
  }
  if (D != 2 && D != 3) {
    set_error("%s: D=%d unsupported", name, D);
    return DICP_ERR_UNSUPPORTED;
  }
  if (M == 0 || L == 0 || (out_q == nullptr && out_p == nullptr)) return DICP_OK;
  if (!q || !p || !aq || !ap || !bq || !bp) {
    set_error("%s: invalid arguments (NULL pointer)", name);
    return DICP_ERR_INVALID;
  }
  for (const float* in : {q, p, aq, ap, bq, bp, gdiv})
    if (in != nullptr && (in == out_q || in == out_p)) {
      set_error("%s: invalid arguments (outputs must not alias inputs)", name);
      return DICP_ERR_INVALID;
    }
  const size_t need = (size_t)L * tlm_slab_bytes(M, 2 * M, D);
  if (need > 0 && (ws == nullptr || ws_bytes < need)) {
    set_error("%s: workspace too small (%zu < %zu bytes)", name, ws_bytes, need);
    return DICP_ERR_WORKSPACE;
  }
  if (int rc = no_batch("ode_hvp")) return rc;
  return D == 2 ? hvp_d<2>("ode_hvp", q, p, aq, ap, bq, bp, M, L, sigma, gdiv, out_q, out_p, ws, st)
                : hvp_d<3>("ode_hvp", q, p, aq, ap, bq, bp, M, L, sigma, gdiv, out_q, out_p, ws, st);
}
