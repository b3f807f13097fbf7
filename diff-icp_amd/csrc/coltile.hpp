// What assign.hip, carry.hip and gram.hip share, as pieces (no Op framework: each kernel keeps
// its own registers, LDS arrays and epilogue).  A lane holds two rows as one packed float2 pair;
// a workgroup sweeps the columns [j0, j1) of its chunk in double-buffered LDS tiles of kTile
// records (ColTiles).  Column chunks (gridDim.y) write per-row partials into the workspace, a
// second launch merges them in chunk order (launch_chunked).  No atomics.
#pragma once
#include "launch.hpp"
#include "lddmm_ops.hpp"
#include "packed.hpp"

namespace dicp {

template <int D>
__device__ __forceinline__ bool finite_row(const float* x) {
  bool ok = true;
#pragma unroll
  for (int d = 0; d < D; ++d) ok = ok && (fabsf(x[d]) <= 3.4028234663852886e38f);   // NaN: false
  return ok;
}

// Rows i0 (.x) and i1 (.y) of rows (M, D) as one packed pair; a row past the end reads row
// M - 1 (its lane stores nothing).  xr0 / xr1 keep the scalars for the epilogue.
template <int D>
__device__ __forceinline__ void load_row_pair(const float* __restrict__ rows, int64_t M, int64_t i0, int64_t i1,
                                              float* xr0, float* xr1, f2* x) {
  ld<D>(rows, i0 < M ? i0 : M - 1, xr0);
  ld<D>(rows, i1 < M ? i1 : M - 1, xr1);
#pragma unroll
  for (int d = 0; d < D; ++d) x[d] = f2{xr0[d], xr1[d]};
}

// |x - y|^2 from the coordinate differences (it keeps its bits far from the origin), in this
// order of operations, on which the results' bits depend: z z for d = 0, then one fma per d
template <int D>
__device__ __forceinline__ f2 pk_sqdist(const f2* x, const float* y) {
  f2 z = x[0] - splat(y[0]);
  f2 d2 = z * z;
#pragma unroll
  for (int d = 1; d < D; ++d) {
    z = x[d] - splat(y[d]);
    d2 = pk_fma(z, z, d2);
  }
  return d2;
}

// LDS column record {y, bias}: D = 2 {y0, y1, b, 0}, D = 3 {y, b}; one ds_read_b128 per column
struct BiasCol {
  template <int D>
  __device__ __forceinline__ static float4 pack(const float* y, float b) {
    return D == 2 ? make_float4(y[0], y[1], b, 0.f) : make_float4(y[0], y[1], y[D - 1], b);
  }
  template <int D>
  __device__ __forceinline__ static void unpack(const float4 q, float y[3], float& b) {
    y[0] = q.x, y[1] = q.y, y[2] = q.z;
    b = D == 2 ? q.z : q.w;
  }
};

// The sweep as the header of the kernel's tile loop (the body stays in the kernel: running sums
// that a body closure holds by reference cost registers):
//   for (ColTiles ts(j0, j1, stage); ts.begin_tile(); ts.end_tile()) { ... }
// The body consumes the ts.cnt columns from ts.jt on in buffer ts.buf.  stage(buf, j, cnt) fills
// buffer buf with the cnt columns from j on (cnt < kTile: the tail; 0 after the last tile).  The
// constructor stages tile 0 and sets the first barrier; begin_tile() stages tile k + 1 into the
// other buffer before the body of tile k; end_tile() sets the ONE barrier per tile, which
// publishes tile k + 1 and retires the reads of tile k, and steps.  Every lane of the workgroup
// must run the loop and fall through to end_tile() in every trip: no continue, break or return
// in the body (the barriers).
template <class Stage>
struct ColTiles {
  const Stage& stage;
  int64_t jt;
  const int64_t j1;
  int buf = 0, cnt, cntn = 0;
  __device__ __forceinline__ ColTiles(int64_t j0, int64_t j1_, const Stage& st)
      : stage(st), jt(j0), j1(j1_), cnt(count(j0)) {
    stage(0, j0, cnt);
    __syncthreads();
  }
  __device__ __forceinline__ int count(int64_t j) const {
    return j < j1 ? (int)((j1 - j) < kTile ? (j1 - j) : kTile) : 0;
  }
  __device__ __forceinline__ bool begin_tile() {
    if (jt >= j1) return false;
    cntn = count(jt + kTile);
    stage(buf ^ 1, jt + kTile, cntn);
    return true;
  }
  __device__ __forceinline__ void end_tile() {
    __syncthreads();
    buf ^= 1;
    cnt = cntn;
    jt += kTile;
  }
};

// num_splits_cap, then at most max_splits chunks (a merge that walks a row's chunks serially)
inline int splits_capped(int64_t M, int64_t N, int R, int64_t cap, int64_t round_rows, int64_t max_rounds,
                         int max_splits) {
  const int S = num_splits_cap(M, N, R, cap, round_rows, max_rounds);
  if (S <= max_splits) return S;
  const int64_t chunk = round_chunk(N, max_splits);
  return (int)((N + chunk - 1) / chunk);
}

inline int check_ws(const char* name, const void* ws, size_t ws_bytes, size_t need) {
  if (need == 0 || (ws != nullptr && ws_bytes >= need)) return DICP_OK;
  set_error("%s: workspace too small (%zu < %zu bytes)", name, ws_bytes, need);
  return DICP_ERR_WORKSPACE;
}

// One chunked pass over S column chunks: S = 0 (no columns) the merge alone, which writes the
// empty result; S = 1 launch_part alone, writing the final outputs; S > 1 the partials, then
// the merge.  launch_part(grid (bx, S)), launch_merge(grid (nb_rows)).
template <class Part, class Merge>
int launch_chunked(const char* name, int64_t nb_rows, int64_t bx, int S, Part&& launch_part,
                   Merge&& launch_merge) {
  if (S > 0) {
    launch_part(dim3((unsigned)bx, (unsigned)S));
    const int rc = check_launch(name);
    if (rc || S == 1) return rc;
  }
  launch_merge(dim3((unsigned)nb_rows));
  return check_launch(name);
}

}  // namespace dicp
