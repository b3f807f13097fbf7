// Packed row passes over L directions (the grid's z dimension), shared by the tangent-linear
// model (tlm.hip) and the second-order operator (hvp.hip): block (bx, by, l) runs
// rowred_pk_body on direction l's rows, columns and outputs, so a direction's result never
// depends on the others of the call.  Column chunks are a function of the support size alone
// (tlm_splits); the chunks' partial outputs add up in slabs in chunk order (tlm_merge_kernel),
// no atomics.
#pragma once
#include "launch.hpp"
#include "lddmm_ops.hpp"
#include "packed.hpp"

namespace dicp {

struct NoRow {};

// field `src` (rows x D) of the rows i0, i1 as packed pairs
template <int D>
__device__ __forceinline__ void ld_rows2(const float* __restrict__ src, int64_t i0, int64_t i1, f2* dst) {
  float u0[D], u1[D];
  ld<D>(src, i0, u0);
  ld<D>(src, i1, u1);
#pragma unroll
  for (int d = 0; d < D; ++d) dst[d] = f2{u0[d], u1[d]};
}

// element strides from one direction to the next: row / column tangents and outputs (0: shared)
struct TlmDir {
  int64_t r[4], c[4], o[4];
};

// block (bx, by, l): rows block bx, column chunk by of S = gridDim.y, direction l
template <class Op, int RP>
__global__ __launch_bounds__(kBlock) void tlm_pk_kernel(Args a, Scal sc, int64_t rows, int64_t cols, int64_t chunk,
                                                        Outs outs, TlmDir dir) {
  const int64_t l = blockIdx.z;
  a.r0 += l * dir.r[0];
  a.r1 += l * dir.r[1];
  a.r2 += l * dir.r[2];
  a.r3 += l * dir.r[3];
  a.c0 += l * dir.c[0];
  a.c1 += l * dir.c[1];
  a.c2 += l * dir.c[2];
  a.c3 += l * dir.c[3];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (outs.ptr[k] != nullptr) outs.ptr[k] += l * dir.o[k];
  rowred_pk_body<Op, RP>(a, sc, rows, cols, chunk, outs, blockIdx.x, blockIdx.y, gridDim.y);
}

// The skeleton's merge (common.hpp merge_slabs_body: chunk order, no epilogue to apply) with the
// direction as blockIdx.z and the output as blockIdx.y: the S slabs of n floats of direction l
// follow those of direction l - 1.  Plain pointer arguments: a MergeSet adjusted per block would
// be indexed at run time and live in scratch.  (A template: defined in a header included by
// several objects.)
template <int I = 0>
__global__ __launch_bounds__(kBlock) void tlm_merge_kernel(const float* __restrict__ slab0,
                                                           const float* __restrict__ slab1, float* __restrict__ out0,
                                                           float* __restrict__ out1, int64_t n, int S) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n) return;
  const int64_t l = blockIdx.z;
  const float* slab = (blockIdx.y == 0 ? slab0 : slab1) + l * S * n;
  float a = slab[e];
  for (int s = 1; s < S; ++s) a += slab[(int64_t)s * n + e];
  (blockIdx.y == 0 ? out0 : out1)[l * n + e] = a;
}

// Column chunks of a pass against M support points: 512 columns each up to 64 chunks, from 131072
// points on 2048 columns each.  Non-decreasing in M (the maximum of two non-decreasing counts).
inline int tlm_splits(int64_t M) {
  if (M <= 0) return 1;
  const int64_t a = (M + 511) / 512, b = (M + 2047) / 2048;
  const int64_t f = a < 64 ? a : 64;
  return (int)(f > b ? f : b);
}

constexpr int kMaxDirs = 65535;   // the grid's z extent

// the partial slabs of one direction: D floats per slab row and column chunk
inline size_t tlm_slab_bytes(int64_t M, int64_t slab_rows, int D) {
  const int S = tlm_splits(M);
  return S <= 1 ? 0 : (size_t)S * (size_t)slab_rows * (size_t)D * sizeof(float);
}

template <class Op, int RP>
int tlm_launch_rp(const char* name, const Args& a, const Scal& sc, int64_t rows, int64_t cols, int L,
                  const TlmDir& dir, const Outs& fin, void* ws, hipStream_t st) {
  using Base = typename Op::Base;
  const int S = tlm_splits(cols);
  const int64_t chunk = (cols + S - 1) / S;
  const int64_t bx = (rows + (int64_t)kBlock * 2 * RP - 1) / ((int64_t)kBlock * 2 * RP);
  if (bx > 0x7fffffff || S > 65535) {
    set_error("%s: too many rows or columns (%lld x %lld)", name, (long long)rows, (long long)cols);
    return DICP_ERR_INVALID;
  }
  const dim3 grid((unsigned)bx, (unsigned)S, (unsigned)L), block(kBlock, 1, 1);
  TlmDir d = dir;
  if (S == 1) {
    for (int k = 0; k < Base::kNOut; ++k) d.o[k] = rows * Base::kOutW[k];
    tlm_pk_kernel<Op, RP><<<grid, block, 0, st>>>(a, sc, rows, cols, chunk, fin, d);
    return check_launch(name);
  }
  // slabs: output k of direction l, chunk s at ws_k + ((l S + s) rows + i) w_k (the caller
  // checked the workspace: tlm_slab_bytes per direction)
  static_assert(Base::kNOut <= 2 && (Base::kNOut < 2 || Base::kOutW[1] == Base::kOutW[0]), "tlm_merge_kernel");
  const int64_t n = rows * Base::kOutW[0];   // floats per slab: every output is D wide
  Outs part = fin;
  const float* slab[2] = {nullptr, nullptr};
  float* out[2] = {nullptr, nullptr};
  int nk = 0;
  float* cur = reinterpret_cast<float*>(ws);
  for (int k = 0; k < Base::kNOut; ++k) {
    part.ptr[k] = fin.ptr[k] ? cur : nullptr;
    d.o[k] = (int64_t)S * n;
    cur += (int64_t)L * S * n;
    if (!fin.ptr[k]) continue;
    slab[nk] = part.ptr[k];
    out[nk] = fin.ptr[k];
    ++nk;
  }
  tlm_pk_kernel<Op, RP><<<grid, block, 0, st>>>(a, sc, rows, cols, chunk, part, d);
  if (int rc = check_launch(name)) return rc;
  if (nk == 0) return DICP_OK;
  const int64_t nb = (n + kBlock - 1) / kBlock;
  tlm_merge_kernel<><<<dim3((unsigned)nb, (unsigned)nk, (unsigned)L), block, 0, st>>>(slab[0], slab[1], out[0], out[1],
                                                                                      n, S);
  return check_launch(name);
}

template <class Op>
int tlm_launch(const char* name, const Args& a, const Scal& sc, int64_t rows, int64_t cols, int L,
               const TlmDir& dir, const Outs& fin, void* ws, hipStream_t st) {
  // pk_rp: option "pk_rp" may force either form (beyond 2 row pairs: 2)
  if (pk_rp<Op>(rows, cols) >= 2) return tlm_launch_rp<Op, 2>(name, a, sc, rows, cols, L, dir, fin, ws, st);
  return tlm_launch_rp<Op, 1>(name, a, sc, rows, cols, L, dir, fin, ws, st);
}

}  // namespace dicp
