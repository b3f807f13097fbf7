// Soft label / field transfer for gfx950: a fused responsibility-weighted mean, i.e. a softmax
// over the columns of Gaussian logits applied to a feature matrix (attention with logits
// bias_j - |r_i - y_j|^2 / 2 sigma^2), in the log2 domain as assign.hip:
//   e_ij    = bias_j - k2 |r_i - y_j|^2,   k2 = log2(e) / (2 sigma^2)
//   lse2_i  = log2 sum_j 2^e_ij
//   out_i,f = sum_j 2^(e_ij - lse2_i) feat_j,f
// One kernel serves both directions of the GMM match: rows = points, columns = components with
// bias w2_c and component attributes (GaussianMixtureUnif.carry_to_points), or rows =
// components, columns = points with bias -T2_n + log2 (1 - gamma0_n) and a per-point field
// (pool_from_points).
// The column-tile sweep of coltile.hpp over records {y, bias} + FB feature channels; a chunk's
// partial is (m, l, acc[FB]) of each row.
// Channels go in blocks of FB in {1, 4, 8, 16} (<= kCarryMaxF), one pass per block
// on the same stream; every block forms bitwise the same weights, so a channel's result does not
// depend on which block, or which F, it is computed in.
// Shift rule (no shift comes from the caller).  Each row carries a reference m_i, an integer
// (the floor of a logit), and sums l = sum_j 2^(e_ij - m_i), acc_f = sum_j 2^(e_ij - m_i) feat_jf,
// per tile and then into the chunk's totals.  A cheap maximum pass over the chunk's first tile
// sets m_i = floor(max_j e_ij).  Afterwards m_i moves only when a tile's sum reaches 2^60 (some
// logit of the tile is then above m_i + 52; none ever adds more than 2^60 unnoticed): a wave
// with such a row takes the tile's maximum, sets m_i = floor of it for the rows concerned,
// rescales their totals by 2^(m_old - m_new) -- an exact power of two -- and redoes the tile.
// The branch is wave-uniform and rare (logits that rise steadily along the columns take it once
// per ~60 log2 units).  So sums of up to 2^31 terms <= 2^60 cannot overflow, m_i never exceeds
// the running maximum (the largest term is >= 1) and never trails it by more than 61, and
// v_exp_f32 flushes nothing above 2^-126 of 2^m_i, i.e. 2^-65 of the running maximum.
// A column with bias = -inf is dead: its weight is exactly 0 and its features are zeroed at
// staging (0 * NaN would be NaN).  No live column (N = 0 or all dead): lse2 = -inf, out = NaN.
// A row with a non-finite coordinate: lse2 = NaN, out = NaN.  A non-finite feature in a live
// column makes its channel non-finite in every row (no skipping by weight).
#include "coltile.hpp"

using namespace dicp;

namespace {

constexpr int kCarryMaxF = 16;        // channels per pass
constexpr int kCarryR = 2;            // rows per lane: one packed pair
// the merge reads a row's partials one after the other (one lane per row)
constexpr int kCarryMaxSplits = 256;
constexpr float kCarryNoRef = -3.4028234663852886e38f;   // m of a row that met no live column
constexpr float kCarryMove = 1.152921504606846976e18f;   // 2^60: a tile sum that moves m

// part: slab (s, k) of M floats at part[((int64_t)s * (FB + 2) + k) * M], k = 0: m, 1: l, 2 + f: acc_f
template <int FB>
__device__ __forceinline__ void store_final(bool finite, float m, float l, const float* acc, int64_t i,
                                            int F, int f0, int fw, float* __restrict__ out,
                                            float* __restrict__ lse2) {
  const float nan = __builtin_nanf("");
  if (lse2 != nullptr) lse2[i] = finite ? m + log2f(l) : nan;   // l = 0: -inf
#pragma unroll
  for (int f = 0; f < FB; ++f)
    if (f < fw) out[i * F + f0 + f] = finite ? acc[f] / l : nan;   // l = 0: 0 / 0
}

// rows (M, D); cols (N, D), bias (N,) or NULL; feat (N, F), channels [f0, f0 + fw), fw <= FB;
// nc = -k2.  part != NULL: the chunk's partial; NULL (one chunk): the final outputs.
template <int D, int FB>
__global__ __launch_bounds__(kBlock) void carry_rowred_kernel(const float* __restrict__ rows, int64_t M,
                                                              const float* __restrict__ cols,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ feat, int64_t N,
                                                              int F, int f0, int fw, float nc, int64_t chunk,
                                                              float* __restrict__ part,
                                                              float* __restrict__ out,
                                                              float* __restrict__ lse2) {
  __shared__ float4 lds[2][kTile];
  __shared__ __attribute__((aligned(16))) float ldf[2][kTile * FB];
  const int tid = threadIdx.x;
  const int64_t ibase = (int64_t)blockIdx.x * (kBlock * kCarryR) + tid;
  float xr[kCarryR][D];
  f2 x[D];   // rows ibase (.x) and ibase + kBlock (.y)
  load_row_pair<D>(rows, M, ibase, ibase + kBlock, xr[0], xr[1], x);
  const f2 nc2 = splat(nc);

  const int64_t j0 = (int64_t)blockIdx.y * chunk;
  int64_t j1 = j0 + chunk;
  if (j1 > N) j1 = N;

  auto stage = [&](int buf, int64_t j, int cnt) {
    if (tid < cnt) {
      float y[D];
      ld<D>(cols, j + tid, y);
      const float b = bias ? bias[j + tid] : 0.f;
      lds[buf][tid] = BiasCol::pack<D>(y, b);
    }
    for (int e = tid; e < cnt * FB; e += kBlock) {
      const int t = e / FB, c = e % FB;
      const bool dead = bias != nullptr && bias[j + t] == -__builtin_huge_valf();
      ldf[buf][e] = (c < fw && !dead) ? feat[(j + t) * F + f0 + c] : 0.f;
    }
  };
  auto logit = [&](const float4 q) {
    float y[3], b;
    BiasCol::unpack<D>(q, y, b);
    return pk_fma(nc2, pk_sqdist<D>(x, y), splat(b));
  };
  // floor of the tile's largest logit per row (-inf without a live column; NaN logits pass by)
  auto tile_max = [&](const float4* tile, int cnt) {
    f2 mx = splat(-__builtin_huge_valf());
    for (int t = 0; t < cnt; ++t) {
      const f2 e = logit(tile[t]);
      mx = f2{fmaxf(mx.x, e.x), fmaxf(mx.y, e.y)};
    }
    return mx;
  };

  f2 m = splat(kCarryNoRef);
  f2 ltot = splat(0.f);
  f2 tot[FB];
#pragma unroll
  for (int f = 0; f < FB; ++f) tot[f] = splat(0.f);

  // The sweep of coltile.hpp written out, with the reference pass over the chunk's first tile
  // after the first barrier: under the ColTiles loop header the staging code around the loop
  // compiles differently (2 VGPRs more at D = 3, FB = 1; 1 % slower at 10 tiles per chunk)
  int cnt = j0 < j1 ? (int)((j1 - j0) < kTile ? (j1 - j0) : kTile) : 0;
  stage(0, j0, cnt);
  __syncthreads();
  {
    const f2 mx = tile_max(lds[0], cnt);
    m = f2{mx.x > m.x ? floorf(mx.x) : m.x, mx.y > m.y ? floorf(mx.y) : m.y};
  }
  int buf = 0;
  for (int64_t jt = j0; jt < j1; jt += kTile) {
    const int64_t jn = jt + kTile;
    const int cntn = jn < j1 ? (int)((j1 - jn) < kTile ? (j1 - jn) : kTile) : 0;
    stage(buf ^ 1, jn, cntn);
    const float4* tile = lds[buf];
    const float* tf = ldf[buf];
    f2 l, acc[FB];
    for (;;) {
      l = splat(0.f);
#pragma unroll
      for (int f = 0; f < FB; ++f) acc[f] = splat(0.f);
#pragma unroll 2
      for (int t = 0; t < cnt; ++t) {
        const f2 a = logit(tile[t]) - m;
        const f2 p = f2{fast_exp2(a.x), fast_exp2(a.y)};
        l += p;
        if constexpr (FB >= 4) {
          const float4* q4 = reinterpret_cast<const float4*>(tf + t * FB);
#pragma unroll
          for (int g = 0; g < FB / 4; ++g) {
            const float4 q = q4[g];
            acc[4 * g + 0] = pk_fma(p, splat(q.x), acc[4 * g + 0]);
            acc[4 * g + 1] = pk_fma(p, splat(q.y), acc[4 * g + 1]);
            acc[4 * g + 2] = pk_fma(p, splat(q.z), acc[4 * g + 2]);
            acc[4 * g + 3] = pk_fma(p, splat(q.w), acc[4 * g + 3]);
          }
        } else {
#pragma unroll
          for (int f = 0; f < FB; ++f) acc[f] = pk_fma(p, splat(tf[t * FB + f]), acc[f]);
        }
      }
      // a tile sum of 2^60 or more (inf included; NaN is not): some logit left m far behind
      const bool mvx = l.x >= kCarryMove, mvy = l.y >= kCarryMove;
      if (!__any(mvx || mvy)) break;
      const f2 mx = tile_max(tile, cnt);
      const f2 mn = f2{mvx ? floorf(mx.x) : m.x, mvy ? floorf(mx.y) : m.y};
      const f2 dm = m - mn;   // integers: exact, or beyond -2^24 where 2^dm = 0 anyway
      const f2 sc = f2{fast_exp2(dm.x), fast_exp2(dm.y)};
      ltot *= sc;
#pragma unroll
      for (int f = 0; f < FB; ++f) tot[f] *= sc;
      m = mn;
    }
    ltot += l;
#pragma unroll
    for (int f = 0; f < FB; ++f) tot[f] += acc[f];
    __syncthreads();
    buf ^= 1;
    cnt = cntn;
  }

#pragma unroll
  for (int r = 0; r < kCarryR; ++r) {
    const int64_t i = ibase + (int64_t)r * kBlock;
    if (i >= M) continue;
    float a[FB];
#pragma unroll
    for (int f = 0; f < FB; ++f) a[f] = r == 0 ? tot[f].x : tot[f].y;
    const float mr = r == 0 ? m.x : m.y, lr = r == 0 ? ltot.x : ltot.y;
    if (part != nullptr) {
      float* dst = part + (int64_t)blockIdx.y * (FB + 2) * M + i;
      dst[0] = mr;
      dst[M] = lr;
#pragma unroll
      for (int f = 0; f < FB; ++f) dst[(int64_t)(2 + f) * M] = a[f];
    } else {
      store_final<FB>(finite_row<D>(xr[r]), mr, lr, a, i, F, f0, fw, out, lse2);
    }
  }
}

// Merge the S chunk partials of each row: the reference is the largest of the chunks' (each
// rescale an exact power of two), the sums are taken in chunk order.  S = 0 (no columns)
// writes lse2 = -inf, out = NaN.
template <int D, int FB>
__global__ __launch_bounds__(kBlock) void carry_merge_kernel(const float* __restrict__ part, int64_t M, int S,
                                                             const float* __restrict__ rows, int F, int f0,
                                                             int fw, float* __restrict__ out,
                                                             float* __restrict__ lse2) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= M) return;
  float m = kCarryNoRef;
  for (int s = 0; s < S; ++s) m = fmaxf(m, part[(int64_t)s * (FB + 2) * M + i]);
  float l = 0.f, acc[FB];
#pragma unroll
  for (int f = 0; f < FB; ++f) acc[f] = 0.f;
  for (int s = 0; s < S; ++s) {
    const float* p = part + (int64_t)s * (FB + 2) * M + i;
    const float sc = fast_exp2(p[0] - m);
    l = fmaf(p[M], sc, l);
#pragma unroll
    for (int f = 0; f < FB; ++f) acc[f] = fmaf(p[(int64_t)(2 + f) * M], sc, acc[f]);
  }
  float x[D];
  ld<D>(rows, i, x);
  store_final<FB>(finite_row<D>(x), m, l, acc, i, F, f0, fw, out, lse2);
}

// One split model for every (D, FB) instantiation (dicp_num_splits has neither argument): the
// resident workgroups of the widest one, one round of them per 11000 rows, at most 9, at most
// 256 chunks.  Measured at 100k x 100k, D = 3 (profiles/carry_split_sweep.txt), F = 1 / F = 16 in
// ms: 8 chunks 2.69 / 6.85, 16 chunks 2.42 / 6.01, 32 chunks 2.32 / 5.59, 48 chunks 2.29 / 5.52,
// 63 chunks 2.36 / 5.62, 121 chunks 2.55 / 5.99 (every chunk pays the maximum sweep of its first
// tile); at 512 rows x 640k columns the time falls with the chunk count up to the cap (32 chunks
// 1.11 / 2.78, 128 chunks 0.35 / 0.79, 250 chunks 0.26 / 0.52).
int carry_splits(int64_t M, int64_t N) {
  static int64_t cap = -1;
  if (cap < 0) cap = (int64_t)device_cus() * blocks_per_cu(carry_rowred_kernel<3, kCarryMaxF>);
  return splits_capped(M, N, kCarryR, cap, 11000, 9, kCarryMaxSplits);
}

// sized for one channel block of kCarryMaxF: (m, l, acc[16]) per chunk and row
size_t carry_ws_bytes(int64_t M, int64_t N) {
  const int S = carry_splits(M, N);
  if (S <= 1 || M <= 0) return 0;
  return (size_t)S * (size_t)M * (size_t)(kCarryMaxF + 2) * sizeof(float);
}

template <int D, int FB>
int launch_carry(const float* rows, int64_t M, const float* cols, const float* bias, const float* feat,
                 int64_t N, int F, int f0, int fw, float nc, int S, float* out, float* lse2, float* part,
                 hipStream_t st) {
  const int64_t chunk = S > 0 ? chunk_of(N, S) : 0;
  if (S <= 1) part = nullptr;
  return launch_chunked(
      "gmm_carry", (M + kBlock - 1) / kBlock, (M + kBlock * kCarryR - 1) / (kBlock * kCarryR), S,
      [&](dim3 grid) {
        carry_rowred_kernel<D, FB><<<grid, dim3(kBlock), 0, st>>>(rows, M, cols, bias, feat, N, F, f0, fw, nc,
                                                                  chunk, part, out, lse2);
      },
      [&](dim3 grid) {
        carry_merge_kernel<D, FB><<<grid, dim3(kBlock), 0, st>>>(part, M, S, rows, F, f0, fw, out, lse2);
      });
}

template <int D>
int carry_d(const float* rows, int64_t M, const float* cols, const float* bias, const float* feat, int64_t N,
            int F, double sigma, float* out, float* lse2, void* ws, size_t ws_bytes, hipStream_t st) {
  const int S = N > 0 ? carry_splits(M, N) : 0;   // 0: no columns, the merge alone
  if (int rc = check_ws("gmm_carry", ws, ws_bytes, carry_ws_bytes(M, N))) return rc;
  const float nc = make_scal(sigma, 0.0).nc;
  float* part = reinterpret_cast<float*>(ws);
  // channel blocks one after the other on the stream: each reuses the workspace
  for (int f0 = 0; f0 < F; f0 += kCarryMaxF) {
    const int fw = F - f0 < kCarryMaxF ? F - f0 : kCarryMaxF;
    float* l2 = f0 == 0 ? lse2 : nullptr;
    int rc;
    if (fw == 1)
      rc = launch_carry<D, 1>(rows, M, cols, bias, feat, N, F, f0, fw, nc, S, out, l2, part, st);
    else if (fw <= 4)
      rc = launch_carry<D, 4>(rows, M, cols, bias, feat, N, F, f0, fw, nc, S, out, l2, part, st);
    else if (fw <= 8)
      rc = launch_carry<D, 8>(rows, M, cols, bias, feat, N, F, f0, fw, nc, S, out, l2, part, st);
    else
      rc = launch_carry<D, 16>(rows, M, cols, bias, feat, N, F, f0, fw, nc, S, out, l2, part, st);
    if (rc) return rc;
  }
  return DICP_OK;
}

}  // namespace

extern "C" int dicp_gmm_carry_f32(const float* rows, int64_t M, const float* cols, const float* bias,
                                  const float* feat, int64_t N, int F, int D, double sigma, float* out,
                                  float* lse2, void* ws, size_t ws_bytes, dicp_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if ((D != 2 && D != 3) || F < 1) {
    set_error("dicp_gmm_carry_f32: invalid arguments (D = %d: 2 or 3; F = %d: >= 1)", D, F);
    return DICP_ERR_INVALID;
  }
  if (M < 0 || N < 0 || N > 0x7fffffffLL || M > 0x7fffffffLL) {
    set_error("dicp_gmm_carry_f32: invalid sizes (M = %lld, N = %lld)", (long long)M, (long long)N);
    return DICP_ERR_INVALID;
  }
  if (M == 0) return DICP_OK;
  if (!rows || !out || (N > 0 && (!cols || !feat)) || !(sigma > 0)) {
    set_error("dicp_gmm_carry_f32: invalid arguments (a null pointer, or sigma <= 0)");
    return DICP_ERR_INVALID;
  }
  if (int rc = no_batch("gmm_carry")) return rc;
  return D == 2 ? carry_d<2>(rows, M, cols, bias, feat, N, F, sigma, out, lse2, ws, ws_bytes, st)
                : carry_d<3>(rows, M, cols, bias, feat, N, F, sigma, out, lse2, ws, ws_bytes, st);
}

// dicp_workspace_bytes(DICP_WS_GMM_CARRY, M rows, N columns, D): sized for one channel block
size_t dicp_carry_ws(int64_t M, int64_t N, int D) {
  if (D != 2 && D != 3) return 0;
  return carry_ws_bytes(M, N);
}

int dicp_carry_splits(int64_t M, int64_t N) { return carry_splits(M, N); }
