// RKHS Gram entries of a ragged list of momentum fields for gfx950: for each listed pair (a, b)
// of fields (q, p) over their own supports,
//   out[n] = sum_{i in a} sum_{j in b} (p_i . p_j) exp(-|q_i - q_j|^2 / (2 sigma^2)),
// the inner product <v_a, v_b>_V of the eta = 0 velocity fields -- the input of tangent-space
// statistics of an atlas (core/statistics.py).  One scalar per pair, in float64.
// The column-tile sweep of coltile.hpp over the records {q, p} of field b, the exponent in the
// log2 domain with one v_exp_f32 per pair term.
// The grid is (pair, row block of a, column chunk of b): every workgroup sums its kBlock *
// kGramR rows x kGramChunk columns and writes ONE double into its own workspace slot; a
// second launch adds each pair's slots in a fixed order.  No atomics.
// Where float32 ends: a pair term (p_i . p_j) 2^(nc |z|^2) is float32, and a lane sums the terms
// of one staged tile (<= kTile per row) in float32, one fused multiply-add per term in column
// order (tests/gram_ref.py restates this arithmetic on the host).  Everything above a tile is
// float64: the lane's running total, the workgroup's tree in LDS, the slots and their merge.
// Geometry: the row blocks and the column chunks have fixed sizes, and the slot grid is sized
// from max_rows alone -- so the tiles, chunks and slots of a pair depend on that pair's two
// sizes and on max_rows, never on the other pairs or fields of the call, and out[n] has the
// same bits wherever the pair stands in whichever call (with the same max_rows).  Workgroups
// beyond a pair's extent write 0.0 into their slot and leave.
// Non-finite input: a point with a non-finite coordinate has its momentum replaced by NaN (an
// infinite distance alone would give weight 0 and hide it), so every pair that contains the
// field and whose other field is not empty is non-finite; no other pair reads the point.
#include "coltile.hpp"

using namespace dicp;

namespace {

constexpr int kGramR = 2;                       // rows per lane: one packed pair
constexpr int64_t kGramRows = kBlock * kGramR;  // rows per workgroup
constexpr int64_t kGramChunk = 8 * kTile;       // columns per workgroup (a whole number of tiles)
constexpr int64_t kGramMaxRows = 65535 * kGramRows;   // gridDim.y (and .z, the longer extent)

// workgroup total of one double per lane, in a fixed tree; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  return red[0];
}

// grid (npairs, BY row blocks, BZ column chunks); part[(n * BY + by) * BZ + bz]
template <int D>
__global__ __launch_bounds__(kBlock) void gram_pair_kernel(const float* __restrict__ q,
                                                           const float* __restrict__ p,
                                                           const int64_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ pairs, float nc,
                                                           double* __restrict__ part) {
  __shared__ float4 lq[2][kTile];                   // D = 2: {q, p};  D = 3: {q, p_0}
  __shared__ float2 lp[2][D == 3 ? kTile : 1];      // D = 3: {p_1, p_2}
  __shared__ double red[kBlock];
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x;
  const int a = pairs[2 * n], b = pairs[2 * n + 1];
  const int64_t oa = offsets[a], Ma = offsets[a + 1] - oa;
  const int64_t ob = offsets[b], Mb = offsets[b + 1] - ob;
  const int64_t slot = (n * gridDim.y + blockIdx.y) * gridDim.z + blockIdx.z;
  const int64_t r0 = (int64_t)blockIdx.y * kGramRows;
  const int64_t j0 = (int64_t)blockIdx.z * kGramChunk;
  if (r0 >= Ma || j0 >= Mb) {   // beyond this pair's extent (uniform over the workgroup)
    if (tid == 0) part[slot] = 0.0;
    return;
  }
  int64_t j1 = j0 + kGramChunk;
  if (j1 > Mb) j1 = Mb;

  const float nan = __builtin_nanf("");
  float xr[kGramR][D], pr[kGramR][D];
#pragma unroll
  for (int r = 0; r < kGramR; ++r) {
    const int64_t i = r0 + tid + (int64_t)r * kBlock;
    if (i < Ma) {
      ld<D>(q, oa + i, xr[r]);
      ld<D>(p, oa + i, pr[r]);
      if (!finite_row<D>(xr[r])) {
#pragma unroll
        for (int d = 0; d < D; ++d) pr[r][d] = nan;
      }
    } else {   // a row past the field: zero momentum adds +-0 to finite sums
#pragma unroll
      for (int d = 0; d < D; ++d) xr[r][d] = 0.f, pr[r][d] = 0.f;
    }
  }
  f2 x[D], pi[D];   // rows r0 + tid (.x) and r0 + tid + kBlock (.y)
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = f2{xr[0][d], xr[1][d]};
    pi[d] = f2{pr[0][d], pr[1][d]};
  }
  const f2 nc2 = splat(nc);

  auto stage = [&](int buf, int64_t j, int cnt) {
    if (tid < cnt) {
      float y[D], pj[D];
      ld<D>(q, ob + j + tid, y);
      ld<D>(p, ob + j + tid, pj);
      if (!finite_row<D>(y)) {
#pragma unroll
        for (int d = 0; d < D; ++d) pj[d] = nan;
      }
      if constexpr (D == 2) {
        lq[buf][tid] = make_float4(y[0], y[1], pj[0], pj[1]);
      } else {
        lq[buf][tid] = make_float4(y[0], y[1], y[D - 1], pj[0]);
        lp[buf][tid] = make_float2(pj[1], pj[D - 1]);
      }
    }
  };

  double tot = 0.0;
  for (ColTiles ts(j0, j1, stage); ts.begin_tile(); ts.end_tile()) {
    const float4* tq = lq[ts.buf];
    const float2* tp = lp[ts.buf];
    f2 acc = splat(0.f);
#pragma unroll 2
    for (int t = 0; t < ts.cnt; ++t) {
      const float4 c = tq[t];
      float y[3], pj[3];
      y[0] = c.x, y[1] = c.y;
      if constexpr (D == 2) {
        y[2] = 0.f, pj[0] = c.z, pj[1] = c.w, pj[2] = 0.f;
      } else {
        const float2 e = tp[t];
        y[2] = c.z, pj[0] = c.w, pj[1] = e.x, pj[2] = e.y;
      }
      f2 dot = pi[0] * splat(pj[0]);
#pragma unroll
      for (int d = 1; d < D; ++d) dot = pk_fma(pi[d], splat(pj[d]), dot);
      const f2 e = nc2 * pk_sqdist<D>(x, y);
      const f2 k = f2{fast_exp2(e.x), fast_exp2(e.y)};
      acc = pk_fma(dot, k, acc);
    }
    tot += (double)acc.x;
    tot += (double)acc.y;
  }
  const double s = block_sum(tot, red);
  if (tid == 0) part[slot] = s;
}

// out[n] = the pair's `slots` partials: lane t adds slots t, t + kBlock, ... in that order, then
// the fixed tree.  slots = 0 (max_rows = 0: every field is empty) writes 0.0.
__global__ __launch_bounds__(kBlock) void gram_merge_kernel(const double* __restrict__ part, int64_t slots,
                                                            double* __restrict__ out) {
  __shared__ double red[kBlock];
  const int64_t n = blockIdx.x;
  double s = 0.0;
  for (int64_t k = threadIdx.x; k < slots; k += kBlock) s += part[n * slots + k];
  const double r = block_sum(s, red);
  if (threadIdx.x == 0) out[n] = r;
}

int64_t gram_row_blocks(int64_t max_rows) { return (max_rows + kGramRows - 1) / kGramRows; }
int64_t gram_chunks(int64_t max_rows) { return (max_rows + kGramChunk - 1) / kGramChunk; }

size_t gram_ws_bytes(int64_t max_rows, int64_t npairs) {
  if (max_rows <= 0 || npairs <= 0 || max_rows > kGramMaxRows) return 0;
  return (size_t)npairs * (size_t)gram_row_blocks(max_rows) * (size_t)gram_chunks(max_rows) * sizeof(double);
}

}  // namespace

extern "C" int dicp_rkhs_gram_f32(const float* q, const float* p, const int64_t* offsets, int F,
                                  int64_t max_rows, const int32_t* pairs, int npairs, int D, double sigma,
                                  double* out, void* ws, size_t ws_bytes, dicp_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if ((D != 2 && D != 3) || F < 0 || npairs < 0 || max_rows < 0 || max_rows > kGramMaxRows) {
    set_error("dicp_rkhs_gram_f32: invalid arguments (D = %d: 2 or 3; F = %d, npairs = %d: >= 0; "
              "max_rows = %lld: 0 ... %lld)", D, F, npairs, (long long)max_rows, (long long)kGramMaxRows);
    return DICP_ERR_INVALID;
  }
  if (npairs == 0) return DICP_OK;
  const size_t need = gram_ws_bytes(max_rows, npairs);
  if (!offsets || !pairs || !out || (max_rows > 0 && (!q || !p)) || (need > 0 && !ws) || !(sigma > 0)) {
    set_error("dicp_rkhs_gram_f32: invalid arguments (a null pointer, or sigma <= 0)");
    return DICP_ERR_INVALID;
  }
  if (int rc = check_ws("rkhs_gram", ws, ws_bytes, need)) return rc;
  if (int rc = no_batch("rkhs_gram")) return rc;
  double* part = reinterpret_cast<double*>(ws);
  const int64_t by = gram_row_blocks(max_rows), bz = gram_chunks(max_rows);
  if (max_rows > 0) {
    const float nc = make_scal(sigma, 0.0).nc;
    const dim3 grid((unsigned)npairs, (unsigned)by, (unsigned)bz);
    if (D == 2)
      gram_pair_kernel<2><<<grid, dim3(kBlock), 0, st>>>(q, p, offsets, pairs, nc, part);
    else
      gram_pair_kernel<3><<<grid, dim3(kBlock), 0, st>>>(q, p, offsets, pairs, nc, part);
    if (int rc = check_launch("rkhs_gram")) return rc;
  }
  gram_merge_kernel<<<dim3((unsigned)npairs), dim3(kBlock), 0, st>>>(part, by * bz, out);
  return check_launch("rkhs_gram");
}

// dicp_workspace_bytes(DICP_WS_RKHS_GRAM, M = max_rows, N = npairs, D): one double per
// (pair, row block, column chunk)
size_t dicp_gram_ws(int64_t M, int64_t N, int D) {
  if (D != 2 && D != 3) return 0;
  return gram_ws_bytes(M, N);
}

// dicp_num_splits(DICP_WS_RKHS_GRAM, M = max_rows, N = npairs): the column chunks of a pair
// of max_rows-point fields, whatever the number of pairs
int dicp_gram_splits(int64_t M, int64_t) {
  const int64_t s = gram_chunks(M);
  return s < 1 ? 1 : (int)s;
}
