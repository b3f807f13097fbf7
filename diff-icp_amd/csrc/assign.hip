// Hard / top-K correspondences for gfx950: a biased top-K row reduction
//   val_ij = bias_j - k2 |r_i - y_j|^2,   k2 = log2(e) / (2 sigma^2)   (log2 domain)
//   out: the K largest val_ij of every row i with their column indices, in descending order.
// One kernel serves both directions of the GMM match: rows = points, columns = components with
// bias w2_c (GaussianMixtureUnif.assign), or rows = components, columns = points with bias
// -T2_n (nearest_points; the row constant w2_c is added by the caller).
// The column-tile sweep of coltile.hpp over records {y, bias}; a chunk's partial is the K
// (val, idx) pairs of each row.  The distance from coordinate differences keeps a
// nearest-neighbour decision's bits when the cloud sits far from the origin.
// Order (total, deterministic): larger val first; equal val: smaller column index first.  The
// running top-K is a sorted insertion in registers that only a strictly larger val moves up, the
// columns are visited in increasing order, and the merge pushes the chunks' lists in chunk
// order, so the rule holds whatever the number of chunks: the result is bitwise independent of it.
// A column is returned only if its val is > -inf (a dead component, bias = -inf, never is) and
// not NaN; slots that cannot be filled hold idx = -1, val = -inf; a row with a non-finite
// coordinate holds idx = -1, val = NaN in every slot.
#include "coltile.hpp"

using namespace dicp;

namespace {

#ifndef DICP_ASSIGN_H
#define DICP_ASSIGN_H 1
#endif
// packed row pairs per lane.  Two pairs (4 rows) measured 1.84 against 1.97 ms at K = 1 but 2.82
// against 2.35 ms at K = 4, 100k x 100k (profiles/assign_split_sweep.txt): one pair
constexpr int kAssignH = DICP_ASSIGN_H;
constexpr int kAssignR = 2 * kAssignH;    // rows per lane
constexpr int kAssignMaxK = 4;
// the merge reads a row's partials one after the other (one lane per row)
constexpr int kAssignMaxSplits = 256;

struct ValIdx {
  float v;
  int i;
};

// Sorted (descending) top-K of one row.  push(): a candidate enters only if strictly larger
// than the last slot (NaN never does), then bubbles up past strictly smaller entries -- among
// equal values the earlier pushed (the smaller column index) stays in front.
template <int K>
struct TopK {
  float v[K];
  int i[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      v[s] = -__builtin_huge_valf();
      i[s] = -1;
    }
  }
  __device__ __forceinline__ void push(float x, int j) {
    if (x > v[K - 1]) {
      v[K - 1] = x;
      i[K - 1] = j;
#pragma unroll
      for (int s = K - 1; s > 0; --s) {
        const bool up = v[s] > v[s - 1];
        const float a = v[s - 1], b = v[s];
        const int ia = i[s - 1], ib = i[s];
        v[s - 1] = up ? b : a;
        v[s] = up ? a : b;
        i[s - 1] = up ? ib : ia;
        i[s] = up ? ia : ib;
      }
    }
  }
};

template <int K>
__device__ __forceinline__ void store_final(bool finite, const TopK<K>& t, int64_t i,
                                            int32_t* __restrict__ idx, float* __restrict__ val) {
#pragma unroll
  for (int s = 0; s < K; ++s) {
    idx[i * K + s] = finite ? t.i[s] : -1;
    val[i * K + s] = finite ? t.v[s] : __builtin_nanf("");
  }
}

// rows (M, D); cols (N, D), bias (N,) or NULL; nc = -k2.  part != NULL: the chunk's partial of
// row i at part[(blockIdx.y * M + i) * K ...]; NULL (one chunk): the final outputs.
template <int D, int K>
__global__ __launch_bounds__(kBlock) void assign_rowred_kernel(const float* __restrict__ rows, int64_t M,
                                                               const float* __restrict__ cols,
                                                               const float* __restrict__ bias, int64_t N,
                                                               float nc, int64_t chunk,
                                                               ValIdx* __restrict__ part,
                                                               int32_t* __restrict__ idx,
                                                               float* __restrict__ val) {
  __shared__ float4 lds[2][kTile];
  const int64_t ibase = (int64_t)blockIdx.x * (kBlock * kAssignR) + threadIdx.x;
  float xr[kAssignR][D];
  f2 x[kAssignH][D];   // pair h: rows 2h (.x) and 2h + 1 (.y)
#pragma unroll
  for (int h = 0; h < kAssignH; ++h) {
    const int64_t i0 = ibase + (int64_t)(2 * h) * kBlock;
    load_row_pair<D>(rows, M, i0, i0 + kBlock, xr[2 * h], xr[2 * h + 1], x[h]);
  }
  const f2 nc2 = splat(nc);
  TopK<K> top[kAssignR];
#pragma unroll
  for (int r = 0; r < kAssignR; ++r) top[r].clear();

  const int64_t j0 = (int64_t)blockIdx.y * chunk;
  int64_t j1 = j0 + chunk;
  if (j1 > N) j1 = N;

  auto stage = [&](int buf, int64_t j, int cnt) {
    const int tid = threadIdx.x;   // read here: captured by reference it costs two VGPRs
    if (tid < cnt) {
      float y[D];
      ld<D>(cols, j + tid, y);
      const float b = bias ? bias[j + tid] : 0.f;
      lds[buf][tid] = BiasCol::pack<D>(y, b);
    }
  };
  for (ColTiles ts(j0, j1, stage); ts.begin_tile(); ts.end_tile()) {
    const float4* tile = lds[ts.buf];
    const int jb = (int)ts.jt;   // N < 2^31 (checked by the entry)
#pragma unroll 2
    for (int t = 0; t < ts.cnt; ++t) {
      float y[3], b;
      BiasCol::unpack<D>(tile[t], y, b);
#pragma unroll
      for (int h = 0; h < kAssignH; ++h) {
        // pk_sqdist written out: through the helper <3, 1> takes one VGPR more
        f2 z = x[h][0] - splat(y[0]);
        f2 d2 = z * z;
#pragma unroll
        for (int d = 1; d < D; ++d) {
          z = x[h][d] - splat(y[d]);
          d2 = pk_fma(z, z, d2);
        }
        const f2 v = pk_fma(nc2, d2, splat(b));
        top[2 * h].push(v.x, jb + t);
        top[2 * h + 1].push(v.y, jb + t);
      }
    }
  }

#pragma unroll
  for (int r = 0; r < kAssignR; ++r) {
    const int64_t i = ibase + (int64_t)r * kBlock;
    if (i >= M) continue;
    const TopK<K>& t = top[r];
    if (part != nullptr) {
      ValIdx* dst = part + ((int64_t)blockIdx.y * M + i) * K;
#pragma unroll
      for (int s = 0; s < K; ++s) dst[s] = ValIdx{t.v[s], t.i[s]};
    } else {
      store_final<K>(finite_row<D>(xr[r]), t, i, idx, val);
    }
  }
}

// Merge the S chunk partials of each row in chunk order (a lower chunk wins ties: its entries
// are pushed first and only a strictly larger val passes them) and write the outputs.  S = 0
// (no columns) writes the unfilled slots.
template <int D, int K>
__global__ __launch_bounds__(kBlock) void assign_merge_kernel(const ValIdx* __restrict__ part, int64_t M,
                                                              int S, const float* __restrict__ rows,
                                                              int32_t* __restrict__ idx,
                                                              float* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= M) return;
  TopK<K> t;
  t.clear();
  for (int s = 0; s < S; ++s) {
    const ValIdx* p = part + ((int64_t)s * M + i) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) t.push(p[k].v, p[k].i);
  }
  float x[D];
  ld<D>(rows, i, x);
  store_final<K>(finite_row<D>(x), t, i, idx, val);
}

// One split model for every (D, K) instantiation (dicp_num_splits has neither argument): the
// resident workgroups of the largest one.  Few rounds of workgroups (one per 32000 rows, at most
// 3; the E-step takes 6 at 100k rows): the shorter a chunk, the more often a column enters some
// lane's running top-K (~K ln(chunk) times per row, a divergent insertion for K > 1), while
// one round alone leaves the chip unbalanced.  Measured at 100k x 100k, D = 3
// (profiles/assign_split_sweep.txt, run 1), K = 1 / K = 4 in ms: 11 chunks 2.14 / 2.35, 21
// chunks 2.00 / 2.23, 31 chunks 1.88 / 2.26, 63 chunks 1.88 / 2.70, 121 chunks 1.87 / 3.36.
int assign_splits(int64_t M, int64_t N) {
  static int64_t cap = -1;
  if (cap < 0) cap = (int64_t)device_cus() * blocks_per_cu(assign_rowred_kernel<3, kAssignMaxK>);
  return splits_capped(M, N, kAssignR, cap, 32000, 3, kAssignMaxSplits);
}

size_t assign_ws_bytes(int64_t M, int64_t N, int K) {
  const int S = assign_splits(M, N);
  if (S <= 1 || M <= 0) return 0;
  return (size_t)S * (size_t)M * (size_t)K * sizeof(ValIdx);
}

template <int D, int K>
int launch_assign(const float* rows, int64_t M, const float* cols, const float* bias, int64_t N,
                  double sigma, int32_t* idx, float* val, void* ws, size_t ws_bytes, hipStream_t st) {
  if (int rc = check_ws("gmm_assign", ws, ws_bytes, assign_ws_bytes(M, N, K))) return rc;
  const int S = N > 0 ? assign_splits(M, N) : 0;
  const int64_t chunk = S > 0 ? chunk_of(N, S) : 0;
  const float nc = make_scal(sigma, 0.0).nc;
  ValIdx* part = S > 1 ? reinterpret_cast<ValIdx*>(ws) : nullptr;
  return launch_chunked(
      "gmm_assign", (M + kBlock - 1) / kBlock, (M + kBlock * kAssignR - 1) / (kBlock * kAssignR), S,
      [&](dim3 grid) {
        assign_rowred_kernel<D, K><<<grid, dim3(kBlock), 0, st>>>(rows, M, cols, bias, N, nc, chunk, part, idx, val);
      },
      [&](dim3 grid) { assign_merge_kernel<D, K><<<grid, dim3(kBlock), 0, st>>>(part, M, S, rows, idx, val); });
}

template <int D>
int assign_d(int K, const float* rows, int64_t M, const float* cols, const float* bias, int64_t N,
             double sigma, int32_t* idx, float* val, void* ws, size_t wsb, hipStream_t st) {
  switch (K) {
    case 1: return launch_assign<D, 1>(rows, M, cols, bias, N, sigma, idx, val, ws, wsb, st);
    case 2: return launch_assign<D, 2>(rows, M, cols, bias, N, sigma, idx, val, ws, wsb, st);
    case 3: return launch_assign<D, 3>(rows, M, cols, bias, N, sigma, idx, val, ws, wsb, st);
    default: return launch_assign<D, 4>(rows, M, cols, bias, N, sigma, idx, val, ws, wsb, st);
  }
}

}  // namespace

extern "C" int dicp_gmm_assign_f32(const float* rows, int64_t M, const float* cols, const float* bias,
                                   int64_t N, int D, double sigma, int K, int32_t* idx, float* val,
                                   void* ws, size_t ws_bytes, dicp_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if ((D != 2 && D != 3) || K < 1 || K > kAssignMaxK) {
    set_error("dicp_gmm_assign_f32: invalid arguments (D = %d: 2 or 3; K = %d: 1..%d)", D, K, kAssignMaxK);
    return DICP_ERR_INVALID;
  }
  if (M < 0 || N < 0 || N > 0x7fffffffLL || M > 0x7fffffffLL * kBlock) {
    set_error("dicp_gmm_assign_f32: invalid sizes (M = %lld, N = %lld)", (long long)M, (long long)N);
    return DICP_ERR_INVALID;
  }
  if (M == 0) return DICP_OK;
  if (!rows || !idx || !val || (N > 0 && !cols) || !(sigma > 0)) {
    set_error("dicp_gmm_assign_f32: invalid arguments");
    return DICP_ERR_INVALID;
  }
  if (int rc = no_batch("gmm_assign")) return rc;
  return D == 2 ? assign_d<2>(K, rows, M, cols, bias, N, sigma, idx, val, ws, ws_bytes, st)
                : assign_d<3>(K, rows, M, cols, bias, N, sigma, idx, val, ws, ws_bytes, st);
}

// dicp_workspace_bytes(DICP_WS_GMM_ASSIGN, M rows, N columns, D): sized for K = 4
size_t dicp_assign_ws(int64_t M, int64_t N, int D) {
  if (D != 2 && D != 3) return 0;
  return assign_ws_bytes(M, N, kAssignMaxK);
}

int dicp_assign_splits(int64_t M, int64_t N) { return assign_splits(M, N); }
