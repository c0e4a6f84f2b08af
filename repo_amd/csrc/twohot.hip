// The two-hot symlog critic (config.value_dist = "twohot"; Hafner et al. 2023): the value head writes K logits
// per row over bins b_k = low + k delta that are uniform in symlog space.  Three streaming kernels over (rows, K) logits:
//   decode      v = symexp(sum_k softmax(z)_k b_k)                        the value the returns and the baseline read
//   decode_bwd  dz_k = g (|v| + 1) p_k (b_k - m)                          the actor's gradient through the returns
//   nll         CE(two-hot(clamp(symlog R)), softmax(z)), dz = scale w (p - t), sums [sum w CE, sum w]
// ONE wave per row, the row in registers: lane l holds the quads k = 256 j + 4 l .. + 3, j < NC = ceil(K / 256) <= 4, so
// every logit is read once per kernel and the max, the denominator and sum p b are wave reductions (no LDS, no re-read).
// Four waves per 256-thread block, a grid-stride loop over the rows above kRedBlocks blocks.  A full quad moves as 16 bytes
// where the row base and pitch allow it (vec); the row's ragged last quad, and every quad of an unaligned operand, moves as
// dwords -- nothing outside [row * ld, row * ld + K) is read or written.
#include <cmath>

#include "common.h"

namespace repo {

constexpr int kThRowsPerBlock = 4;   // waves of a 256-thread block
constexpr int kThMaxK = 1024;        // 4 quads per lane

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// The bins, counted from the middle: b_k = mid + (2k - (K - 1)) (delta / 2), one double product, rounded to float once.
// For symmetric bounds mid is 0, so b_k = -b_{K-1-k} in bits and the middle bin of an odd K is exactly 0.
struct ThBins {
  double mid, hdelta;
  int K;
  __device__ __forceinline__ float at(int k) const { return (float)fma((double)(2 * k - (K - 1)), hdelta, mid); }
};

// lane's NC quads of the row at p; elements at k >= K read as -inf (their softmax weight is exactly 0)
template <int NC>
__device__ __forceinline__ void th_load(const float* __restrict__ p, int K, int lane, int vec, float (&z)[NC][4]) {
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int k = 256 * j + 4 * lane;
    if (vec && k + 3 < K) {
      const float4 q = *reinterpret_cast<const float4*>(p + k);
      z[j][0] = q.x; z[j][1] = q.y; z[j][2] = q.z; z[j][3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) z[j][e] = (k + e < K) ? p[k + e] : -INFINITY;
    }
  }
}
template <int NC>
__device__ __forceinline__ void th_store(float* __restrict__ p, int K, int lane, int vec, const float (&d)[NC][4]) {
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int k = 256 * j + 4 * lane;
    if (vec && k + 3 < K) {
      *reinterpret_cast<float4*>(p + k) = make_float4(d[j][0], d[j][1], d[j][2], d[j][3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k + e < K) p[k + e] = d[j][e];
    }
  }
}

// z -> e = exp(z - max) in place; returns (den = sum e, m = sum e b / den) on every lane.  sum e b is taken in double: a
// product of two floats is exact there, and so is the whole sum when the weights are equal -- the zero-initialised head
// decodes to exactly 0 over symmetric bins, whatever the order of the additions.
template <int NC>
__device__ __forceinline__ void th_softmax_mean(float (&z)[NC][4], int lane, const ThBins bins, float& den, float& m) {
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < NC; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) mx = fmaxf(mx, z[j][e]);
  mx = wave_max(mx);
  float s = 0.f;
  double sb = 0.0;
#pragma unroll
  for (int j = 0; j < NC; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ex = expf(z[j][e] - mx);
      z[j][e] = ex;
      s += ex;
      sb = fma((double)ex, (double)bins.at(256 * j + 4 * lane + e), sb);
    }
  den = wave_sum(s);
  m = (float)(wave_sum_d(sb) / (double)den);
}

__device__ __forceinline__ float symexp(float m) { return copysignf(expm1f(fabsf(m)), m); }

template <int NC>
__global__ __launch_bounds__(256) void twohot_decode_kernel(long rows, int K, const float* __restrict__ logits, long ld,
                                                            const ThBins bins, int vec, float* __restrict__ v_out,
                                                            float* __restrict__ m_out) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (long row = (long)blockIdx.x * kThRowsPerBlock + wid; row < rows; row += (long)gridDim.x * kThRowsPerBlock) {
    float z[NC][4], den, m;
    th_load<NC>(logits + (size_t)row * ld, K, lane, vec, z);
    th_softmax_mean<NC>(z, lane, bins, den, m);
    if (lane == 0) {
      v_out[row] = symexp(m);
      if (m_out) m_out[row] = m;
    }
  }
}

template <int NC>
__global__ __launch_bounds__(256) void twohot_decode_bwd_kernel(long rows, int K, const float* __restrict__ logits, long ld,
                                                                const ThBins bins, int vec,
                                                                const float* __restrict__ g, float* __restrict__ dlogits,
                                                                long ldd, int vec_d, const float* __restrict__ gmul) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float gm = gmul ? *gmul : 1.f;
  for (long row = (long)blockIdx.x * kThRowsPerBlock + wid; row < rows; row += (long)gridDim.x * kThRowsPerBlock) {
    float z[NC][4], den, m;
    th_load<NC>(logits + (size_t)row * ld, K, lane, vec, z);
    th_softmax_mean<NC>(z, lane, bins, den, m);
    // symexp'(m) = exp(|m|) = |v| + 1
    const float coef = g[row] * gm * expf(fabsf(m)) / den;
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) z[j][e] = coef * z[j][e] * (bins.at(256 * j + 4 * lane + e) - m);
    th_store<NC>(dlogits + (size_t)row * ldd, K, lane, vec_d, z);
  }
}

// parts[0][blk] = sum w CE ; parts[1][blk] = sum w
template <int NC>
__global__ __launch_bounds__(256) void twohot_nll_kernel(long rows, int K, const float* __restrict__ logits, long ld,
                                                         const float* __restrict__ returns,
                                                         const float* __restrict__ weights, float lowf, float highf,
                                                         double low, double delta, float scale, int vec,
                                                         float* __restrict__ dlogits, long ldd, int vec_d,
                                                         float* __restrict__ parts, float* __restrict__ red_out,
                                                         unsigned* __restrict__ ticket) {
  __shared__ float red[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float a = 0.f, wsum = 0.f;
  for (long row = (long)blockIdx.x * kThRowsPerBlock + wid; row < rows; row += (long)gridDim.x * kThRowsPerBlock) {
    float z[NC][4];
    th_load<NC>(logits + (size_t)row * ld, K, lane, vec, z);
    // the two-hot target of this row's return.  Comparisons, not fminf / fmaxf: a NaN return stays NaN through the clamp
    const float R = returns[row];
    float y = copysignf(log1pf(fabsf(R)), R);
    if (y < lowf) y = lowf;
    if (y > highf) y = highf;
    float pos = (float)(((double)y - low) / delta);
    if (pos > (float)(K - 1)) pos = (float)(K - 1);   // (the division's last bit)
    const bool bad = pos != pos;
    // the float -> int conversion sees a finite value in [0, K - 2] only; a NaN row takes k0 = 0 and a NaN target below
    const int k0 = bad ? 0 : (int)fminf(floorf(fmaxf(pos, 0.f)), (float)(K - 2));
    const float f = pos - (float)k0;
    const float w = weights ? weights[row] : 1.f;
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) mx = fmaxf(mx, z[j][e]);
    mx = wave_max(mx);
    float s = 0.f, tz = 0.f;
    float t[NC][4];
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 256 * j + 4 * lane + e;
        const float zc = z[j][e] - mx;
        const float tk = bad ? pos : k == k0 ? 1.f - f : k == k0 + 1 ? f : 0.f;
        t[j][e] = tk;
        if (bad || k == k0 || k == k0 + 1) tz = fmaf(tk, zc, tz);   // (never 0 * -inf of the lanes past K)
        const float ex = expf(zc);
        z[j][e] = ex;
        s += ex;
      }
    const float den = wave_sum(s);
    tz = wave_sum(tz);
    if (lane == 0) {
      a = fmaf(w, logf(den) - tz, a);   // CE = -sum t log_softmax(z) = log den - sum t (z - max), sum t = 1
      wsum += w;
    }
    if (dlogits) {
      const float sw = scale * w, inv = 1.f / den;
#pragma unroll
      for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) z[j][e] = sw * (z[j][e] * inv - t[j][e]);
      th_store<NC>(dlogits + (size_t)row * ldd, K, lane, vec_d, z);
    }
  }
  const float s0 = block_sum(a, red);
  const float s1 = block_sum(wsum, red);
  if (threadIdx.x == 0) {
    parts[blockIdx.x] = s0;
    parts[gridDim.x + blockIdx.x] = s1;
  }
  last_block_finishes(parts, 2, red_out, ticket, red);
}

static inline ThBins th_bins(float low, float high, int64_t K) {
  return ThBins{0.5 * ((double)low + (double)high), ((double)high - (double)low) / (2.0 * (double)(K - 1)), (int)K};
}
static inline int th_vec(const void* p, int64_t ld) { return ((uintptr_t)p & 15u) == 0 && (ld & 3) == 0; }
static inline bool th_bounds_ok(float low, float high) { return std::isfinite(low) && std::isfinite(high) && low < high; }

}  // namespace repo

using namespace repo;

#define TH_DISPATCH(K, LAUNCH)              \
  do {                                      \
    const int _nc = ((K) + 255) / 256;      \
    if (_nc == 1) { LAUNCH(1); }            \
    else if (_nc == 2) { LAUNCH(2); }       \
    else if (_nc == 3) { LAUNCH(3); }       \
    else { LAUNCH(4); }                     \
  } while (0)

extern "C" int repo_twohot_geometry(int* rows_per_block, int* last_block_max_grid, int* max_blocks) {
  REPO_REQUIRE(rows_per_block && last_block_max_grid && max_blocks, REPO_E_BADARG);
  *rows_per_block = kThRowsPerBlock;
  *last_block_max_grid = kLastBlockMaxGrid;
  *max_blocks = kRedBlocks;
  return REPO_OK;
}

extern "C" int repo_twohot_decode(int64_t rows, int64_t K, const float* logits, int64_t ld, float low, float high,
                                  float* v_out, float* m_out, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(rows > 0 && rows < kMaxIdx && K >= 2 && K <= kThMaxK && ld >= K, REPO_E_SHAPE);
  REPO_REQUIRE(logits && v_out && th_bounds_ok(low, high), REPO_E_BADARG);
  const ThBins bins = th_bins(low, high, K);
  const int blocks = red_blocks(rows, kThRowsPerBlock);
#define LAUNCH(NC)                                                                                                      \
  hipLaunchKernelGGL(twohot_decode_kernel<NC>, dim3(blocks), dim3(256), 0, stream, (long)rows, (int)K, logits, (long)ld, \
                     bins, th_vec(logits, ld), v_out, m_out)
  TH_DISPATCH((int)K, LAUNCH);
#undef LAUNCH
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_twohot_decode_bwd(int64_t rows, int64_t K, const float* logits, int64_t ld, float low, float high,
                                      const float* g, float* dlogits, int64_t ldd, const float* gmul,
                                      hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(rows > 0 && rows < kMaxIdx && K >= 2 && K <= kThMaxK && ld >= K && ldd >= K, REPO_E_SHAPE);
  REPO_REQUIRE(logits && g && dlogits && th_bounds_ok(low, high), REPO_E_BADARG);
  const ThBins bins = th_bins(low, high, K);
  const int blocks = red_blocks(rows, kThRowsPerBlock);
#define LAUNCH(NC)                                                                                                     \
  hipLaunchKernelGGL(twohot_decode_bwd_kernel<NC>, dim3(blocks), dim3(256), 0, stream, (long)rows, (int)K, logits,     \
                     (long)ld, bins, th_vec(logits, ld), g, dlogits, (long)ldd, th_vec(dlogits, ldd), gmul)
  TH_DISPATCH((int)K, LAUNCH);
#undef LAUNCH
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_twohot_nll(int64_t rows, int64_t K, const float* logits, int64_t ld, const float* returns,
                               const float* weights, float low, float high, float scale, float* dlogits, int64_t ldd,
                               float* sums2, void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(rows > 0 && rows < kMaxIdx && K >= 2 && K <= kThMaxK && ld >= K && (!dlogits || ldd >= K), REPO_E_SHAPE);
  REPO_REQUIRE(logits && returns && sums2 && th_bounds_ok(low, high), REPO_E_BADARG);
  REPO_REQUIRE(ws && ws_bytes >= repo_reduce_workspace_bytes(), REPO_E_WS_TOO_SMALL);
  const double delta = ((double)high - (double)low) / (double)(K - 1);
  const int blocks = red_blocks(rows, kThRowsPerBlock);
#define LAUNCH(NC)                                                                                                       \
  hipLaunchKernelGGL(twohot_nll_kernel<NC>, dim3(blocks), dim3(256), 0, stream, (long)rows, (int)K, logits, (long)ld,    \
                     returns, weights, low, high, (double)low, delta, scale, th_vec(logits, ld), dlogits, (long)ldd,     \
                     dlogits ? th_vec(dlogits, ldd) : 0, red_parts(ws), sums2, red_ticket(ws, blocks))
  TH_DISPATCH((int)K, LAUNCH);
#undef LAUNCH
  REPO_CHECK_LAUNCH();
  return red_finish(ws, blocks, 2, sums2, stream);
}
