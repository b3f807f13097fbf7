// Velocity gradient at carried points for gfx950: the D x D matrix A_i = dv/dx (x_i) of the
// LDDMM vector field of the support (q, p), next to v(x_i) itself, in one packed row reduction
// (packed.hpp rowred_pk_kernel; rows x, columns (q, p) records, coordinates in original units as
// the external-point forward OpExtFwdPk of ext_pk.hpp).  With s = 1/sigma^2, z = x_i - q_j,
// K = exp(-s |z|^2 / 2) (one exp2 per pair):
//
//   v_d      = sum K p_d + eta s sum K z_d
//   A[d][a]  = -s sum K z_a p_d + eta s (delta_da sum K - s sum K z_d z_a)
//
// (trace A = -g, the divergence row of dicp_lddmm_ode_ext_fwd_f32).  Sums per row, in
// accumulator order:  V (D) | T[d][a] = sum K z_a p_d (D^2) | eta != 0: Z (D), the upper
// triangle of H[d][a] = sum K z_d z_a (D (D + 1) / 2), S = sum K.
// Every output is linear in the sums, so the column chunks' partial outputs add up in the
// skeleton's slabs (merge_slabs_kernel, chunk order, no atomics).
//
// The Euler step of the displacement gradient G = J - I of the discrete flow,
//   x+ = x + dt v,   G+ = G + dt A (I + G),
// is the same pass: the row's product A (I + G) is formed where the row is stored (linear in
// the sums as well, so it too passes through the slabs) and base + dt * value is the
// skeleton's output epilogue, in the kernel or in the merge.
//
// The Newton update towards F(x) = y of a step map F of that flow (the exact inverse of the
// discrete flow, LDDMMModel.flow_inverse) needs the same (v, A) but is not linear in them: the
// pass writes them to a scratch region and a row-wise kernel solves the D x D system (below).
#include "launch.hpp"
#include "lddmm_ops.hpp"
#include "packed.hpp"

using namespace dicp;

namespace {

template <int D, bool ETA>
struct OpExtJacS {
  static constexpr int kTri = D * (D + 1) / 2;
  static constexpr int CW4 = cw4(2 * D);
  static constexpr int NACC = D + D * D + (ETA ? D + kTri + 1 : 0);
  static constexpr int kNOut = 2;
  static constexpr int kOutW[4] = {D, D * D, 0, 0};
  static constexpr bool kMin = false;
  // index of H[d][a] (d <= a) in the upper triangle, row-major
  __host__ __device__ static constexpr int tri(int d, int a) { return d * D - d * (d - 1) / 2 + (a - d); }
  // what the row's store needs: its G (D x D, row-major) of a step, or NULL (G = 0, or A itself
  // wanted); the coordinates live in the packed Row2 only
  struct Row {
    const float* g;
  };
  __device__ static void load_row(const Args& a, int64_t i, Row& r) {
    r.g = a.r1 ? a.r1 + i * (D * D) : nullptr;
  }
  __device__ static void load_col(const Args& a, int64_t j, float* rec) {
    ld<D>(a.c0, j, rec);
    ld<D>(a.c1, j, rec + D);
  }
  __device__ static void store(const Scal& sc, const Row& r, const float* t, float* v) {
    const float s = sc.s;
    const float es = sc.eta * sc.s;
    const float* T = t + D;
    constexpr int o = D + D * D;
    float A[D][D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      v[d] = ETA ? fmaf(es, t[o + d], t[d]) : t[d];
#pragma unroll
      for (int a = 0; a < D; ++a) {
        float m = -s * T[d * D + a];
        if (ETA) {
          const float H = t[o + D + (d <= a ? tri(d, a) : tri(a, d))];
          const float S = d == a ? t[o + D + kTri] : 0.f;
          m = fmaf(es, fmaf(-s, H, S), m);
        }
        A[d][a] = m;
      }
    }
    float* out = v + D;
    if (r.g != nullptr) {   // A (I + G)
      float G[D * D];
      ld<D * D>(r.g, 0, G);
#pragma unroll
      for (int d = 0; d < D; ++d)
#pragma unroll
        for (int a = 0; a < D; ++a) {
          float m = A[d][a];
#pragma unroll
          for (int c = 0; c < D; ++c) m = fmaf(A[d][c], G[c * D + a], m);
          out[d * D + a] = m;
        }
    } else {
#pragma unroll
      for (int d = 0; d < D; ++d)
#pragma unroll
        for (int a = 0; a < D; ++a) out[d * D + a] = A[d][a];
    }
  }
};

template <int D, bool ETA>
struct OpExtJacPk {
  using Base = OpExtJacS<D, ETA>;
  // 4 rows per thread on large passes (packed.hpp pk_rp) share every column record; with the 22
  // sums of eta != 0 a second row pair would double 88 accumulator registers: one pair
  static constexpr int kRP = ETA ? 1 : 2;
  static constexpr int CW4 = Base::CW4;
  static constexpr int NACC = Base::NACC;
  static constexpr int kNOut = Base::kNOut;
  static constexpr bool kMin = false;
  struct Row2 { f2 x[D]; f2 nc; };
  __device__ static void load_rows_s(const Args& a, const Scal& sc, int64_t i0, int64_t i1, Row2& r,
                                     typename Base::Row& b0, typename Base::Row& b1) {
    Base::load_row(a, i0, b0);
    Base::load_row(a, i1, b1);
    float x0[D], x1[D];
    ld<D>(a.r0, i0, x0);
    ld<D>(a.r0, i1, x1);
#pragma unroll
    for (int d = 0; d < D; ++d) r.x[d] = f2{x0[d], x1[d]};
    r.nc = splat(sc.nc);
  }
  __device__ static void pair2(const Row2& r, const float* rec, f2* acc) {
    f2 z[D];
    f2 r2 = splat(0.f);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      z[d] = r.x[d] - splat(rec[d]);
      r2 = pk_fma(z[d], z[d], r2);
    }
    const f2 e = r.nc * r2;
    const f2 K = f2{fast_exp2(e.x), fast_exp2(e.y)};
    const float* pj = rec + D;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const f2 Kp = K * splat(pj[d]);
      acc[d] = acc[d] + Kp;
#pragma unroll
      for (int a = 0; a < D; ++a) acc[D + d * D + a] = pk_fma(Kp, z[a], acc[D + d * D + a]);
    }
    if constexpr (ETA) {
      constexpr int o = D + D * D;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const f2 Kz = K * z[d];
        acc[o + d] = acc[o + d] + Kz;
#pragma unroll
        for (int a = d; a < D; ++a)
          acc[o + D + Base::tri(d, a)] = pk_fma(Kz, z[a], acc[o + D + Base::tri(d, a)]);
      }
      acc[o + D + Base::kTri] = acc[o + D + Base::kTri] + K;
    }
  }
};

// step = false: (o0, o1) = (vx (N, D) or NULL, A (N, D, D)); step = true: the Euler step,
// (o0, o1) = (x_next, G_next) with G (N, D, D) or NULL (zero)
template <int D>
int ext_jac_d(const char* name, const float* x, const float* G, int64_t N, const float* q, const float* p,
              int64_t M, double sigma, double eta, bool step, double dt, float* o0, float* o1, void* ws,
              size_t wsb, hipStream_t st) {
  const Args a = {x, step ? G : nullptr, nullptr, nullptr, q, p, nullptr, nullptr, 0.f, nullptr};
  const Scal sc = make_scal(sigma, eta);
  Outs o = make_outs(o0, o1);
  if (step) {
    o.base[0] = x;
    o.alpha[0] = (float)dt;
    o.base[1] = G;
    o.alpha[1] = (float)dt;
  }
  if (eta != 0.0) return launch_rowred_pk<OpExtJacPk<D, true>>(name, a, sc, N, M, o, ws, wsb, st);
  return launch_rowred_pk<OpExtJacPk<D, false>>(name, a, sc, N, M, o, ws, wsb, st);
}

template <int D>
int jac_splits_d(int64_t N, int64_t M) {
  const int a = rowred_pk_splits<OpExtJacPk<D, false>>(N, M);
  const int b = rowred_pk_splits<OpExtJacPk<D, true>>(N, M);
  return a > b ? a : b;
}

// the same checks for both entries; *done: nothing left to launch
int jac_check(const char* name, const float* x, int64_t N, const float* q, const float* p, int64_t M, int D,
              double sigma, const float* out, bool* done) {
  *done = false;
  if (N < 0 || M < 0 || !(sigma > 0)) {
    set_error("%s: invalid arguments (N = %lld, M = %lld, sigma = %g)", name, (long long)N, (long long)M, sigma);
    return DICP_ERR_INVALID;
  }
  if (D != 2 && D != 3) {
    set_error("%s: D=%d unsupported", name, D);
    return DICP_ERR_UNSUPPORTED;
  }
  if (N == 0) {
    *done = true;
    return DICP_OK;
  }
  if (!x || !out || (M > 0 && (!q || !p))) {
    set_error("%s: invalid arguments (NULL pointer)", name);
    return DICP_ERR_INVALID;
  }
  return DICP_OK;
}

int hip_rc(const char* name, hipError_t e) {
  if (e == hipSuccess) return DICP_OK;
  set_error("%s: %s", name, hipGetErrorString(e));
  return DICP_ERR_HIP;
}


// ---- Newton update of one step map of the discrete flow (dicp_lddmm_ext_inv_step_f32) ----
// The update x+ = x - DF^-1 r is not linear in the pair sums, so it cannot pass through the
// partial slabs as an output: (v | A) of the pass go, through the slabs where the pass is split,
// into a scratch region at the head of the workspace, and a row-wise kernel applies the update.

// mid-point of the Ralston step: xm = x + h v1 (the rows of the second stage's pair pass)
__global__ __launch_bounds__(kBlock) void inv_mid_kernel(const float* __restrict__ x, const float* __restrict__ v1,
                                                         float h, int64_t n, float* __restrict__ xm) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e < n) xm[e] = fmaf(h, v1[e], x[e]);
}

// One thread per row.  va: (v (N, D) | A (N, D, D)) of the pass, or NULL (no support: zero).
// v1 == NULL: Euler, F = x + dt v, DF = I + dt A; otherwise Ralston with (v, A) = (v2, A2):
// F = x + dt/4 v1 + 3 dt/4 v2, DF = I + dt/4 A1 + 3 dt/4 A2 (I + h A1), h = 2 dt / 3.
// r = (x - y) + (F - x); the D x D solve by cofactors, every index a compile-time constant.
template <int D>
__global__ __launch_bounds__(kBlock) void inv_update_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ v1,
                                                            const float* __restrict__ A1,
                                                            const float* __restrict__ va, int64_t N, float dt,
                                                            float* __restrict__ xn, float* __restrict__ res) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  float xi[D], yi[D], v[D], A[D * D], r[D], m[D * D];
  ld<D>(x, i, xi);
  ld<D>(y, i, yi);
  if (va != nullptr) {
    ld<D>(va, i, v);
    ld<D * D>(va + N * D, i, A);
  } else {
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = 0.f;
#pragma unroll
    for (int e = 0; e < D * D; ++e) A[e] = 0.f;
  }
  if (v1 == nullptr) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      r[d] = fmaf(dt, v[d], xi[d] - yi[d]);
#pragma unroll
      for (int a = 0; a < D; ++a) m[d * D + a] = fmaf(dt, A[d * D + a], d == a ? 1.f : 0.f);
    }
  } else {
    float w[D], B[D * D];
    ld<D>(v1, i, w);
    ld<D * D>(A1, i, B);
    const float h = dt * (2.f / 3.f), c1 = 0.25f * dt, c2 = 0.75f * dt;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      r[d] = (xi[d] - yi[d]) + fmaf(c2, v[d], c1 * w[d]);
#pragma unroll
      for (int a = 0; a < D; ++a) {
        float t = A[d * D + a];   // A2 (I + h A1)
#pragma unroll
        for (int c = 0; c < D; ++c) t = fmaf(h * A[d * D + c], B[c * D + a], t);
        m[d * D + a] = fmaf(c2, t, fmaf(c1, B[d * D + a], d == a ? 1.f : 0.f));
      }
    }
  }
  float dx[D];
  if constexpr (D == 2) {
    const float det = m[0] * m[3] - m[1] * m[2];
    dx[0] = (m[3] * r[0] - m[1] * r[1]) / det;
    dx[1] = (m[0] * r[1] - m[2] * r[0]) / det;
  } else {
    const float c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const float c10 = m[2] * m[7] - m[1] * m[8], c11 = m[0] * m[8] - m[2] * m[6], c12 = m[1] * m[6] - m[0] * m[7];
    const float c20 = m[1] * m[5] - m[2] * m[4], c21 = m[2] * m[3] - m[0] * m[5], c22 = m[0] * m[4] - m[1] * m[3];
    const float det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    dx[0] = (c00 * r[0] + c10 * r[1] + c20 * r[2]) / det;   // adj = cofactors transposed
    dx[1] = (c01 * r[0] + c11 * r[1] + c21 * r[2]) / det;
    dx[2] = (c02 * r[0] + c12 * r[1] + c22 * r[2]) / det;
  }
  float o[D], rm = 0.f, chk = 0.f;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    // no support, Euler: F is the identity and the solution is y itself
    o[d] = (va == nullptr && v1 == nullptr) ? yi[d] : xi[d] - dx[d];
    rm = fmaxf(rm, fabsf(r[d]));
    chk += o[d] + r[d];
  }
  // singular DF (det = 0: x / 0) or a non-finite input: the whole row, and only it, is marked
  const bool bad = !(fabsf(chk) <= 3.0e38f);
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int d = 0; d < D; ++d) xn[i * D + d] = bad ? nan : o[d];
  res[i] = bad ? nan : rm;
}

template <int D>
int ext_inv_d(const char* name, const float* x, const float* y, const float* v1, const float* A1, int64_t N,
              const float* q, const float* p, int64_t M, double sigma, double eta, double dt, float* xn,
              float* res, void* ws, size_t wsb, hipStream_t st) {
  const size_t scratch = (size_t)N * (D + D * D) * sizeof(float);
  float* va = nullptr;
  if (M > 0) {
    if (ws == nullptr || wsb < scratch) {
      set_error("%s: workspace too small (%zu < %zu bytes)", name, wsb, scratch);
      return DICP_ERR_WORKSPACE;
    }
    va = reinterpret_cast<float*>(ws);
    const float* rows = x;
    if (v1 != nullptr) {   // x_next holds the mid-point until the update overwrites it
      const int64_t n = N * D;
      inv_mid_kernel<<<dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st>>>(
          x, v1, (float)(2.0 * dt / 3.0), n, xn);
      if (int rc = check_launch(name)) return rc;
      rows = xn;
    }
    if (int rc = ext_jac_d<D>("ext_inv_step", rows, nullptr, N, q, p, M, sigma, eta, false, 0.0, va, va + N * D,
                              reinterpret_cast<char*>(ws) + scratch, wsb - scratch, st))
      return rc;
  }
  inv_update_kernel<D><<<dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, st>>>(
      x, y, v1, A1, va, N, (float)dt, xn, res);
  return check_launch(name);
}

}  // namespace

extern "C" int dicp_lddmm_ode_ext_jac_f32(const float* x, int64_t N, const float* q, const float* p, int64_t M,
                                          int D, double sigma, double eta, float* vx, float* A, void* ws,
                                          size_t ws_bytes, dicp_stream_t stream) {
  const char* name = "dicp_lddmm_ode_ext_jac_f32";
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  bool done;
  if (int rc = jac_check(name, x, N, q, p, M, D, sigma, A, &done)) return rc;
  if (done) return DICP_OK;
  if (int rc = no_batch("ode_ext_jac")) return rc;
  if (M == 0) {   // no support: v = 0, A = 0
    if (vx)
      if (int rc = hip_rc(name, hipMemsetAsync(vx, 0, (size_t)N * D * sizeof(float), st))) return rc;
    return hip_rc(name, hipMemsetAsync(A, 0, (size_t)N * D * D * sizeof(float), st));
  }
  return D == 2 ? ext_jac_d<2>("ode_ext_jac", x, nullptr, N, q, p, M, sigma, eta, false, 0.0, vx, A, ws, ws_bytes, st)
                : ext_jac_d<3>("ode_ext_jac", x, nullptr, N, q, p, M, sigma, eta, false, 0.0, vx, A, ws, ws_bytes, st);
}

extern "C" int dicp_lddmm_ext_jac_step_f32(const float* x, const float* G, int64_t N, const float* q,
                                           const float* p, int64_t M, int D, double sigma, double eta, double dt,
                                           float* x_next, float* G_next, void* ws, size_t ws_bytes,
                                           dicp_stream_t stream) {
  const char* name = "dicp_lddmm_ext_jac_step_f32";
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  bool done;
  if (int rc = jac_check(name, x, N, q, p, M, D, sigma, G_next, &done)) return rc;
  if (done) return DICP_OK;
  if (!x_next) {
    set_error("%s: invalid arguments (NULL pointer)", name);
    return DICP_ERR_INVALID;
  }
  if (x_next == x || G_next == G) {
    set_error("%s: invalid arguments (outputs must not alias inputs)", name);
    return DICP_ERR_INVALID;
  }
  if (int rc = no_batch("ext_jac_step")) return rc;
  if (M == 0) {   // no support: the points and their gradient stay
    const size_t nx = (size_t)N * D * sizeof(float), ng = nx * D;
    if (int rc = hip_rc(name, hipMemcpyAsync(x_next, x, nx, hipMemcpyDeviceToDevice, st))) return rc;
    return hip_rc(name, G ? hipMemcpyAsync(G_next, G, ng, hipMemcpyDeviceToDevice, st)
                          : hipMemsetAsync(G_next, 0, ng, st));
  }
  return D == 2 ? ext_jac_d<2>("ext_jac_step", x, G, N, q, p, M, sigma, eta, true, dt, x_next, G_next, ws, ws_bytes, st)
                : ext_jac_d<3>("ext_jac_step", x, G, N, q, p, M, sigma, eta, true, dt, x_next, G_next, ws, ws_bytes, st);
}

// dicp_num_splits(DICP_WS_ODE_EXT_JAC, M support points, N carried points): the largest split
// count of the instantiations (the entry has neither D nor eta)
int dicp_ext_jac_splits(int64_t M, int64_t N) {
  const int a = jac_splits_d<2>(N, M), b = jac_splits_d<3>(N, M);
  return a > b ? a : b;
}

// dicp_workspace_bytes(DICP_WS_ODE_EXT_JAC, M, N, D): the partial slabs (vx | A) of N rows for
// that many chunks, whichever of them a call at this D then uses
size_t dicp_ext_jac_ws(int64_t M, int64_t N, int D) {
  if ((D != 2 && D != 3) || M <= 0 || N <= 0) return 0;
  const int S = dicp_ext_jac_splits(M, N);
  if (S <= 1) return 0;
  return (size_t)S * (size_t)N * (size_t)(D + D * D) * sizeof(float);
}

extern "C" int dicp_lddmm_ext_inv_step_f32(const float* x, const float* y, const float* v1, const float* A1,
                                           int64_t N, const float* q, const float* p, int64_t M, int D,
                                           double sigma, double eta, double dt, float* x_next, float* res,
                                           void* ws, size_t ws_bytes, dicp_stream_t stream) {
  const char* name = "dicp_lddmm_ext_inv_step_f32";
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  bool done;
  if (int rc = jac_check(name, x, N, q, p, M, D, sigma, x_next, &done)) return rc;
  if ((v1 == nullptr) != (A1 == nullptr)) {
    set_error("%s: invalid arguments (v1 and A1 go together)", name);
    return DICP_ERR_INVALID;
  }
  if (done) return DICP_OK;
  if (!y || !res) {
    set_error("%s: invalid arguments (NULL pointer)", name);
    return DICP_ERR_INVALID;
  }
  if (x_next == x || x_next == y || x_next == v1) {
    set_error("%s: invalid arguments (outputs must not alias inputs)", name);
    return DICP_ERR_INVALID;
  }
  if (int rc = no_batch("ext_inv_step")) return rc;
  return D == 2 ? ext_inv_d<2>(name, x, y, v1, A1, N, q, p, M, sigma, eta, dt, x_next, res, ws, ws_bytes, st)
                : ext_inv_d<3>(name, x, y, v1, A1, N, q, p, M, sigma, eta, dt, x_next, res, ws, ws_bytes, st);
}

// dicp_workspace_bytes(DICP_WS_ODE_EXT_INV, M, N, D): the (v | A) scratch of N rows at the head,
// then the partial slabs of DICP_WS_ODE_EXT_JAC (in its 256-byte granule)
size_t dicp_ext_inv_ws(int64_t M, int64_t N, int D) {
  if ((D != 2 && D != 3) || M <= 0 || N <= 0) return 0;
  const size_t slabs = (dicp_ext_jac_ws(M, N, D) + 255) / 256 * 256;
  return (size_t)N * (size_t)(D + D * D) * sizeof(float) + slabs;
}
