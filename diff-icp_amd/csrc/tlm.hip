// Tangent-linear model (TLM) of the eta = 0 LDDMM ODE for gfx950: the exact derivative of the
// right-hand side at (q, p) -- and of the velocity at carried points x -- along L directions
// (dq_l, dp_l, dx_l), as packed row reductions (packed.hpp rowred_pk_body; coordinates in
// original units as ext_pk.hpp / ext_jac.hip).  With s = 1/sigma^2, K = exp(-s |z|^2 / 2) (one
// exp2 per pair):
//
//   self rows i (z = q_i - q_j, dz = dq_i - dq_j):
//     dv_i  =   sum_j K [ dp_j - s (z.dz) p_j ]
//     dmG_i = s sum_j K [ (dp_i.p_j + p_i.dp_j) z + (p_i.p_j) dz - s (p_i.p_j)(z.dz) z ]
//   carried rows i (z = x_i - q_j, dz = dx_i - dq_j):
//     dvx_i =   sum_j K [ dp_j - s (z.dz) p_j ]
//
// The accumulators are the outputs themselves: dv (D) | dmG / s (D) per self row, dvx (D) per
// carried row; the diagonal j = i of the self part adds dp_i to dv_i and nothing else (z = dz = 0).
// Column records are (q_j, p_j, dq_j, dp_j), 4 D floats: at D = 3 the double-buffered 256-column
// tiles take 24 KB of LDS.  The direction is the grid's z dimension: block (bx, by, l) reads the
// shared (q, p, x) and direction l's tangents and writes direction l's outputs, so a direction's
// result never depends on the others of the call.
//
// Column chunks: S = tlm_splits(M) chunks of ceil(M / S) columns, a function of the support size
// alone (not of the device, the options or L), so the bits depend on the sizes only; the chunks'
// partial outputs add up in slabs in chunk order (tlm_merge_kernel), no atomics.  The direction
// grid, the chunk count and the merge are tlm_pass.hpp, shared with hvp.hip.
#include "tlm_pass.hpp"

using namespace dicp;

namespace {

// the column record both parts stage: (q_j, p_j, dq_j, dp_j)
template <int D>
__device__ __forceinline__ void tlm_load_col(const Args& a, int64_t j, float* rec) {
  ld<D>(a.c0, j, rec);
  ld<D>(a.c1, j, rec + D);
  ld<D>(a.c2, j, rec + 2 * D);
  ld<D>(a.c3, j, rec + 3 * D);
}

// z, dz, K and w = s (z.dz) of a row pair against one column record
template <int D>
__device__ __forceinline__ void tlm_pair_head(const f2* x, const f2* dx, f2 nc, f2 s, const float* rec, f2* z,
                                              f2* dz, f2& K, f2& w) {
  f2 r2 = splat(0.f), zdz = splat(0.f);
#pragma unroll
  for (int d = 0; d < D; ++d) {
    z[d] = x[d] - splat(rec[d]);
    dz[d] = dx[d] - splat(rec[2 * D + d]);
    r2 = pk_fma(z[d], z[d], r2);
    zdz = pk_fma(z[d], dz[d], zdz);
  }
  const f2 e = nc * r2;
  K = f2{fast_exp2(e.x), fast_exp2(e.y)};
  w = s * zdz;
}

template <int D>
struct OpTlmSelfS {
  static constexpr int CW4 = cw4(4 * D);
  static constexpr int NACC = 2 * D;
  static constexpr int kNOut = 2;
  static constexpr int kOutW[4] = {D, D, 0, 0};
  static constexpr bool kMin = false;
  using Row = NoRow;   // the store needs nothing of the row
  __device__ static void load_col(const Args& a, int64_t j, float* rec) { tlm_load_col<D>(a, j, rec); }
  __device__ static void store(const Scal& sc, const Row&, const float* t, float* v) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      v[d] = t[d];
      v[D + d] = sc.s * t[D + d];
    }
  }
};

// rows r0..r3 = (q, p, dq_l, dp_l), columns c0..c3 the same arrays
template <int D>
struct OpTlmSelfPk {
  using Base = OpTlmSelfS<D>;
  // one row pair per thread: the row state alone is 4 D packed registers
  static constexpr int kRP = 1;
  static constexpr int CW4 = Base::CW4;
  static constexpr int NACC = Base::NACC;
  static constexpr int kNOut = Base::kNOut;
  static constexpr bool kMin = false;
  struct Row2 { f2 q[D], p[D], dq[D], dp[D]; f2 nc, s; };
  __device__ static void load_rows_s(const Args& a, const Scal& sc, int64_t i0, int64_t i1, Row2& r, NoRow&,
                                     NoRow&) {
    ld_rows2<D>(a.r0, i0, i1, r.q);
    ld_rows2<D>(a.r1, i0, i1, r.p);
    ld_rows2<D>(a.r2, i0, i1, r.dq);
    ld_rows2<D>(a.r3, i0, i1, r.dp);
    r.nc = splat(sc.nc);
    r.s = splat(sc.s);
  }
  __device__ static void pair2(const Row2& r, const float* rec, f2* acc) {
    f2 z[D], dz[D], K, w;
    tlm_pair_head<D>(r.q, r.dq, r.nc, r.s, rec, z, dz, K, w);
    const float* pj = rec + D;
    const float* dpj = rec + 3 * D;
    f2 pp = splat(0.f), dpp = splat(0.f);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const f2 pjd = splat(pj[d]), dpjd = splat(dpj[d]);
      acc[d] = pk_fma(K, pk_fma(-w, pjd, dpjd), acc[d]);
      pp = pk_fma(r.p[d], pjd, pp);
      dpp = pk_fma(r.p[d], dpjd, pk_fma(r.dp[d], pjd, dpp));
    }
    const f2 Kc = K * pk_fma(-w, pp, dpp);   // K [(dp_i.p_j + p_i.dp_j) - s (z.dz)(p_i.p_j)]
    const f2 Kpp = K * pp;
#pragma unroll
    for (int d = 0; d < D; ++d) acc[D + d] = pk_fma(Kc, z[d], pk_fma(Kpp, dz[d], acc[D + d]));
  }
};

template <int D>
struct OpTlmExtS {
  static constexpr int CW4 = cw4(4 * D);
  static constexpr int NACC = D;
  static constexpr int kNOut = 1;
  static constexpr int kOutW[4] = {D, 0, 0, 0};
  static constexpr bool kMin = false;
  using Row = NoRow;
  __device__ static void load_col(const Args& a, int64_t j, float* rec) { tlm_load_col<D>(a, j, rec); }
  __device__ static void store(const Scal&, const Row&, const float* t, float* v) {
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = t[d];
  }
};

// rows r0, r1 = (x, dx_l), columns as the self part
template <int D>
struct OpTlmExtPk {
  using Base = OpTlmExtS<D>;
  static constexpr int kRP = 2;   // 4 rows per thread on large passes, as OpExtJacPk at eta = 0
  static constexpr int CW4 = Base::CW4;
  static constexpr int NACC = Base::NACC;
  static constexpr int kNOut = Base::kNOut;
  static constexpr bool kMin = false;
  struct Row2 { f2 x[D], dx[D]; f2 nc, s; };
  __device__ static void load_rows_s(const Args& a, const Scal& sc, int64_t i0, int64_t i1, Row2& r, NoRow&,
                                     NoRow&) {
    ld_rows2<D>(a.r0, i0, i1, r.x);
    ld_rows2<D>(a.r1, i0, i1, r.dx);
    r.nc = splat(sc.nc);
    r.s = splat(sc.s);
  }
  __device__ static void pair2(const Row2& r, const float* rec, f2* acc) {
    f2 z[D], dz[D], K, w;
    tlm_pair_head<D>(r.x, r.dx, r.nc, r.s, rec, z, dz, K, w);
#pragma unroll
    for (int d = 0; d < D; ++d)
      acc[d] = pk_fma(K, pk_fma(-w, splat(rec[D + d]), splat(rec[3 * D + d])), acc[d]);
  }
};

template <int D>
int tlm_d(const char* name, const float* q, const float* p, const float* dq, const float* dp, int64_t M,
          const float* x, const float* dx, int64_t N, int L, double sigma, float* dv, float* dmG, float* dvx,
          void* ws, hipStream_t st) {
  const Scal sc = make_scal(sigma, 0.0);
  const int64_t md = M * D, nd = N * D;
  if (dv != nullptr || dmG != nullptr) {
    const Args a = {q, p, dq, dp, q, p, dq, dp, 0.f, nullptr};
    const TlmDir dir = {{0, 0, md, md}, {0, 0, md, md}, {0, 0, 0, 0}};
    if (int rc = tlm_launch<OpTlmSelfPk<D>>(name, a, sc, M, M, L, dir, make_outs(dv, dmG), ws, st)) return rc;
  }
  if (N > 0) {   // after the self part's merge on the same stream: the slabs are free again
    const Args a = {x, dx, nullptr, nullptr, q, p, dq, dp, 0.f, nullptr};
    const TlmDir dir = {{0, nd, 0, 0}, {0, 0, md, md}, {0, 0, 0, 0}};
    if (int rc = tlm_launch<OpTlmExtPk<D>>(name, a, sc, N, M, L, dir, make_outs(dvx), ws, st)) return rc;
  }
  return DICP_OK;
}

}  // namespace

// dicp_num_splits(DICP_WS_ODE_TLM, M support points, N carried points): the column chunks of
// both parts (their columns are the support)
int dicp_tlm_splits(int64_t M, int64_t) { return tlm_splits(M); }

// dicp_workspace_bytes(DICP_WS_ODE_TLM, M, N, D): the partial slabs of ONE direction -- (dv | dmG)
// of the M self rows or dvx of the N carried rows, whichever is larger (the parts run one after
// the other); a call with L directions needs L times as much
size_t dicp_tlm_ws(int64_t M, int64_t N, int D) {
  if ((D != 2 && D != 3) || M <= 0) return 0;
  return tlm_slab_bytes(M, 2 * M > N ? 2 * M : N, D);
}

extern "C" int dicp_lddmm_ode_tlm_f32(const float* q, const float* p, const float* dq, const float* dp, int64_t M,
                                      const float* x, const float* dx, int64_t N, int L, int D, double sigma,
                                      float* dv, float* dmG, float* dvx, void* ws, size_t ws_bytes,
                                      dicp_stream_t stream) {
  const char* name = "dicp_lddmm_ode_tlm_f32";
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (M < 0 || N < 0 || L < 0 || L > kMaxDirs || !(sigma > 0)) {
    set_error("%s: invalid arguments (M = %lld, N = %lld: >= 0; L = %d: 0 ... %d; sigma = %g: > 0)", name,
              (long long)M, (long long)N, L, kMaxDirs, sigma);
    return DICP_ERR_INVALID;
  }
  if (D != 2 && D != 3) {
    set_error("%s: D=%d unsupported", name, D);
    return DICP_ERR_UNSUPPORTED;
  }
  if (x == nullptr) N = 0;   // no carried part
  const bool self = M > 0 && (dv != nullptr || dmG != nullptr);
  if (L == 0 || (!self && N == 0)) return DICP_OK;
  if ((M > 0 && (!q || !p || !dq || !dp)) || (N > 0 && (!dx || !dvx))) {
    set_error("%s: invalid arguments (NULL pointer)", name);
    return DICP_ERR_INVALID;
  }
  for (const float* in : {q, p, dq, dp, x, dx})
    if (in != nullptr && (in == dv || in == dmG || in == dvx)) {
      set_error("%s: invalid arguments (outputs must not alias inputs)", name);
      return DICP_ERR_INVALID;
    }
  const int64_t slab_rows = self && 2 * M > N ? 2 * M : N;   // of the parts this call runs
  const size_t need = (size_t)L * tlm_slab_bytes(M, slab_rows, D);
  if (need > 0 && (ws == nullptr || ws_bytes < need)) {
    set_error("%s: workspace too small (%zu < %zu bytes)", name, ws_bytes, need);
    return DICP_ERR_WORKSPACE;
  }
  if (int rc = no_batch("ode_tlm")) return rc;
  if (M == 0) {   // no support: the field and its tangent vanish
    const hipError_t e = hipMemsetAsync(dvx, 0, (size_t)L * N * D * sizeof(float), st);
    if (e == hipSuccess) return DICP_OK;
    set_error("%s: %s", name, hipGetErrorString(e));
    return DICP_ERR_HIP;
  }
  return D == 2 ? tlm_d<2>("ode_tlm", q, p, dq, dp, M, x, dx, N, L, sigma, dv, dmG, dvx, ws, st)
                : tlm_d<3>("ode_tlm", q, p, dq, dp, M, x, dx, N, L, sigma, dv, dmG, dvx, ws, st);
}
