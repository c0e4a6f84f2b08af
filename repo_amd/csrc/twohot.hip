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
// The _x siblings (config.value_bin_space / reward_bin_space / value_slow_reg) take the bin space and, for the
// cross-entropy, a second target.  Space 0 runs the kernels above -- the same instantiations, so the same bits.  Space 1 puts
// the bins at B_k = symexp(b_k):
//   decode      v = sum_k p_k B_k, summed in mirrored pairs                a true expectation, exactly 0 for equal logits
//   decode_bwd  dz_k = g p_k (B_k - v)
//   nll         two-hot(clamp(R, B_0, B_{K-1})) between the B_k, located through symlog(y) and moved by at most one bin
// and, in both spaces, nll with target_b: ONE logsumexp per row, dz = scale w ((p - t_a) + reg (p - t_b)), three sums.
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

// ---- space 1: the bins at B_k = symexp(b_k)
// This lane's bin values B[j][e] and, for the elements that are the LOWER member of a mirrored pair (2k < K - 1), the
// partner's Bm[j][e] = B_{K-1-k}: functions of (lane, K, bounds) only, so they are formed once, ahead of the row loop.
template <int NC>
__device__ __forceinline__ void th_symexp_bins(const ThBins bins, int lane, float (&B)[NC][4], float (&Bm)[NC][4]) {
#pragma unroll
  for (int j = 0; j < NC; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 256 * j + 4 * lane + e;
      B[j][e] = k < bins.K ? symexp(bins.at(k)) : 0.f;
      Bm[j][e] = 2 * k < bins.K - 1 ? symexp(bins.at(bins.K - 1 - k)) : 0.f;
    }
}

// z -> e = exp(z - max) in place; returns (den = sum e, v = sum e B / den) on every lane.  sum e B is taken pair by pair:
// the lane that holds bin k < (K - 1) / 2 reads the partner logit z_{K-1-k} of its own row again (a dword inside the row,
// just loaded: it comes from the cache), forms the partner's e by the same expression -- so the same bits as its owner
// holds -- and adds (e' B' + e B) in double, where both products are exact; the middle bin of an odd K enters alone.  With
// equal logits over symmetric bins every pair is exactly 0, and so is every sum of pairs.
template <int NC>
__device__ __forceinline__ void th_softmax_expect(float (&z)[NC][4], const float* __restrict__ p, int K, int lane,
                                                  const float (&B)[NC][4], const float (&Bm)[NC][4], float& den,
                                                  float& v) {
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
      const int k = 256 * j + 4 * lane + e;
      const float ex = expf(z[j][e] - mx);
      z[j][e] = ex;
      s += ex;
      if (2 * k < K - 1) {          // (k < K follows)
        const float exm = expf(p[K - 1 - k] - mx);
        sb += (double)exm * (double)Bm[j][e] + (double)ex * (double)B[j][e];
      } else if (2 * k == K - 1) {
        sb += (double)ex * (double)B[j][e];
      }
    }
  den = wave_sum(s);
  v = (float)(wave_sum_d(sb) / (double)den);
}

template <int NC>
__global__ __launch_bounds__(256) void twohot_decode_s1_kernel(long rows, int K, const float* __restrict__ logits, long ld,
                                                               const ThBins bins, int vec, float* __restrict__ v_out,
                                                               float* __restrict__ m_out) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float B[NC][4], Bm[NC][4];
  th_symexp_bins<NC>(bins, lane, B, Bm);
  for (long row = (long)blockIdx.x * kThRowsPerBlock + wid; row < rows; row += (long)gridDim.x * kThRowsPerBlock) {
    float z[NC][4], den, v;
    const float* p = logits + (size_t)row * ld;
    th_load<NC>(p, K, lane, vec, z);
    th_softmax_expect<NC>(z, p, K, lane, B, Bm, den, v);
    if (lane == 0) {
      v_out[row] = v;
      if (m_out) m_out[row] = v;
    }
  }
}

template <int NC>
__global__ __launch_bounds__(256) void twohot_decode_bwd_s1_kernel(long rows, int K, const float* __restrict__ logits,
                                                                   long ld, const ThBins bins, int vec,
                                                                   const float* __restrict__ g,
                                                                   float* __restrict__ dlogits, long ldd, int vec_d,
                                                                   const float* __restrict__ gmul) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float gm = gmul ? *gmul : 1.f;
  float B[NC][4], Bm[NC][4];
  th_symexp_bins<NC>(bins, lane, B, Bm);
  for (long row = (long)blockIdx.x * kThRowsPerBlock + wid; row < rows; row += (long)gridDim.x * kThRowsPerBlock) {
    float z[NC][4], den, v;
    const float* p = logits + (size_t)row * ld;
    th_load<NC>(p, K, lane, vec, z);
    th_softmax_expect<NC>(z, p, K, lane, B, Bm, den, v);
    const float coef = g[row] * gm / den;
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) z[j][e] = coef * z[j][e] * (B[j][e] - v);
    th_store<NC>(dlogits + (size_t)row * ldd, K, lane, vec_d, z);
  }
}

// The two-hot target of one row, on every lane: (k0, f) with t_{k0} = 1 - f, t_{k0+1} = f, or bad with `nanv` a NaN that
// every t of the row takes.  Comparisons, not fminf / fmaxf: a NaN target stays NaN through the clamps.
struct ThTarget {
  int k0;
  float f, f0, nanv;   // f0 = 1 - f
  bool bad;
};
template <int SPACE>
__device__ __forceinline__ ThTarget th_target(float R, int K, float lowf, float highf, double low, double delta,
                                              const ThBins bins, float b_lo, float b_hi) {
  ThTarget t;
  if constexpr (SPACE == 0) {
    float y = copysignf(log1pf(fabsf(R)), R);
    if (y < lowf) y = lowf;
    if (y > highf) y = highf;
    float pos = (float)(((double)y - low) / delta);
    if (pos > (float)(K - 1)) pos = (float)(K - 1);   // (the division's last bit)
    t.bad = pos != pos;
    // the float -> int conversion sees a finite value in [0, K - 2] only; a NaN row takes k0 = 0 and a NaN target below
    t.k0 = t.bad ? 0 : (int)fminf(floorf(fmaxf(pos, 0.f)), (float)(K - 2));
    t.f = pos - (float)t.k0;
    t.nanv = pos;
  } else {
    // the RAW target between the end bins, the bin below it through symlog on the uniform grid; symlog and the float B_k
    // each round, so the guess can sit one bin off: it moves by at most one bin, the neighbours' B_k read again.  The end
    // bins b_lo = B_0, b_hi = B_{K-1} are the same for every row: the kernel forms them once, ahead of its row loop
    float y = R;
    if (y < b_lo) y = b_lo;
    if (y > b_hi) y = b_hi;
    t.bad = y != y;
    const float pos = (float)(((double)copysignf(log1pf(fabsf(y)), y) - low) / delta);
    int k0 = t.bad ? 0 : (int)fminf(floorf(fmaxf(pos, 0.f)), (float)(K - 2));
    float b0 = symexp(bins.at(k0)), b1 = symexp(bins.at(k0 + 1));
    if (y < b0 && k0 > 0) {
      --k0;
      b1 = b0;
      b0 = symexp(bins.at(k0));
    } else if (y > b1 && k0 < K - 2) {
      ++k0;
      b0 = b1;
      b1 = symexp(bins.at(k0 + 1));
    }
    float f = (y - b0) / (b1 - b0);
    if (f < 0.f) f = 0.f;
    if (f > 1.f) f = 1.f;
    t.k0 = k0;
    t.f = f;
    t.nanv = y;
  }
  t.f0 = 1.f - t.f;
  return t;
}
__device__ __forceinline__ float th_weight(const ThTarget& t, int k) {
  return t.bad ? t.nanv : k == t.k0 ? t.f0 : k == t.k0 + 1 ? t.f : 0.f;
}

// parts[0][blk] = sum w CE_a ; parts[1][blk] = sum w ; with nvals == 3, parts[2][blk] = sum w CE_b (0 without a target_b).
// <SPACE 0, PAIR false> is repo_twohot_nll's kernel, expression for expression.
template <int NC, int SPACE, bool PAIR>
__global__ __launch_bounds__(256) void twohot_nll_kernel(long rows, int K, const float* __restrict__ logits, long ld,
                                                         const float* __restrict__ returns,
                                                         const float* __restrict__ target_b, float reg,
                                                         const float* __restrict__ weights, float lowf, float highf,
                                                         double low, double delta, const ThBins bins, float scale,
                                                         int vec, float* __restrict__ dlogits, long ldd, int vec_d,
                                                         float* __restrict__ parts, int nvals,
                                                         float* __restrict__ red_out, unsigned* __restrict__ ticket) {
  __shared__ float red[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float a = 0.f, wsum = 0.f, ab = 0.f;
  const float b_lo = SPACE ? symexp(bins.at(0)) : 0.f, b_hi = SPACE ? symexp(bins.at(K - 1)) : 0.f;
  for (long row = (long)blockIdx.x * kThRowsPerBlock + wid; row < rows; row += (long)gridDim.x * kThRowsPerBlock) {
    float z[NC][4];
    th_load<NC>(logits + (size_t)row * ld, K, lane, vec, z);
    const ThTarget ta = th_target<SPACE>(returns[row], K, lowf, highf, low, delta, bins, b_lo, b_hi);
    ThTarget tb = ta;
    if constexpr (PAIR) tb = th_target<SPACE>(target_b[row], K, lowf, highf, low, delta, bins, b_lo, b_hi);
    const float w = weights ? weights[row] : 1.f;
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) mx = fmaxf(mx, z[j][e]);
    mx = wave_max(mx);
    float s = 0.f, tz = 0.f, tzb = 0.f;
    float t[NC][4], t2[PAIR ? NC : 1][4];
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 256 * j + 4 * lane + e;
        const float zc = z[j][e] - mx;
        const float tk = th_weight(ta, k);
        t[j][e] = tk;
        if (ta.bad || k == ta.k0 || k == ta.k0 + 1) tz = fmaf(tk, zc, tz);   // (never 0 * -inf of the lanes past K)
        if constexpr (PAIR) {
          const float tkb = th_weight(tb, k);
          t2[j][e] = tkb;
          if (tb.bad || k == tb.k0 || k == tb.k0 + 1) tzb = fmaf(tkb, zc, tzb);
        }
        const float ex = expf(zc);
        z[j][e] = ex;
        s += ex;
      }
    const float den = wave_sum(s);
    tz = wave_sum(tz);
    if constexpr (PAIR) tzb = wave_sum(tzb);
    if (lane == 0) {
      const float lden = logf(den);
      a = fmaf(w, lden - tz, a);   // CE = -sum t log_softmax(z) = log den - sum t (z - max), sum t = 1
      wsum += w;
      if constexpr (PAIR) ab = fmaf(w, lden - tzb, ab);
    }
    if (dlogits) {
      const float sw = scale * w, inv = 1.f / den;
#pragma unroll
      for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if constexpr (PAIR) {   // (p - t_a) + reg (p - t_b): reg == 0 leaves the unpaired gradient's bits
            const float qa = z[j][e] * inv - t[j][e], qb = z[j][e] * inv - t2[j][e];
            z[j][e] = sw * fmaf(reg, qb, qa);
          } else {
            z[j][e] = sw * (z[j][e] * inv - t[j][e]);
          }
        }
      th_store<NC>(dlogits + (size_t)row * ldd, K, lane, vec_d, z);
    }
  }
  const float s0 = block_sum(a, red);
  const float s1 = block_sum(wsum, red);
  float s2 = 0.f;
  if constexpr (PAIR) s2 = block_sum(ab, red);
  if (threadIdx.x == 0) {
    parts[blockIdx.x] = s0;
    parts[gridDim.x + blockIdx.x] = s1;
    if (nvals == 3) parts[2 * gridDim.x + blockIdx.x] = s2;
  }
  last_block_finishes(parts, nvals, red_out, ticket, red);
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

// The cross-entropy's one launch path: repo_twohot_nll is (space 0, no target_b, two sums), repo_twohot_nll_x the rest.
static int th_nll_launch(int64_t rows, int64_t K, const float* logits, int64_t ld, const float* target_a,
                         const float* target_b, float reg, const float* weights, float low, float high, int space,
                         float scale, float* dlogits, int64_t ldd, float* sums, int nvals, void* ws, hipStream_t stream) {
  const double delta = ((double)high - (double)low) / (double)(K - 1);
  const ThBins bins = th_bins(low, high, K);
  const int blocks = red_blocks(rows, kThRowsPerBlock);
  const int sel = 2 * (space != 0) + (target_b != nullptr);
#define LAUNCH_AS(NC, SPACE, PAIR)                                                                                      \
  hipLaunchKernelGGL((twohot_nll_kernel<NC, SPACE, PAIR>), dim3(blocks), dim3(256), 0, stream, (long)rows, (int)K,      \
                     logits, (long)ld, target_a, target_b, reg, weights, low, high, (double)low, delta, bins, scale,    \
                     th_vec(logits, ld), dlogits, (long)ldd, dlogits ? th_vec(dlogits, ldd) : 0, red_parts(ws), nvals,  \
                     sums, red_ticket(ws, blocks))
#define LAUNCH(NC)                                       \
  do {                                                   \
    if (sel == 0) LAUNCH_AS(NC, 0, false);               \
    else if (sel == 1) LAUNCH_AS(NC, 0, true);           \
    else if (sel == 2) LAUNCH_AS(NC, 1, false);          \
    else LAUNCH_AS(NC, 1, true);                         \
  } while (0)
  TH_DISPATCH((int)K, LAUNCH);
#undef LAUNCH
#undef LAUNCH_AS
  REPO_CHECK_LAUNCH();
  return red_finish(ws, blocks, nvals, sums, stream);
}

extern "C" int repo_twohot_nll(int64_t rows, int64_t K, const float* logits, int64_t ld, const float* returns,
                               const float* weights, float low, float high, float scale, float* dlogits, int64_t ldd,
                               float* sums2, void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(rows > 0 && rows < kMaxIdx && K >= 2 && K <= kThMaxK && ld >= K && (!dlogits || ldd >= K), REPO_E_SHAPE);
  REPO_REQUIRE(logits && returns && sums2 && th_bounds_ok(low, high), REPO_E_BADARG);
  REPO_REQUIRE(ws && ws_bytes >= repo_reduce_workspace_bytes(), REPO_E_WS_TOO_SMALL);
  return th_nll_launch(rows, K, logits, ld, returns, nullptr, 0.f, weights, low, high, 0, scale, dlogits, ldd, sums2, 2, ws,
                       stream);
}

// ---- the _x siblings
// space 1 puts bins at symexp(low) and symexp(high): both must be finite floats
static inline bool th_space_ok(int space, float low, float high) {
  if (space == 0) return true;
  return space == 1 && std::isfinite(expm1f(fabsf(low))) && std::isfinite(expm1f(fabsf(high)));
}

extern "C" size_t repo_twohot_nll_x_workspace_bytes(void) { return kRedHeaderBytes + 3 * kRedBlocks * sizeof(float); }

extern "C" int repo_twohot_decode_x(int64_t rows, int64_t K, const float* logits, int64_t ld, float low, float high,
                                    int space, float* v_out, float* m_out, hipStream_t stream) {
  if (space == 0) return repo_twohot_decode(rows, K, logits, ld, low, high, v_out, m_out, stream);
  REPO_ARCH_GUARD();
  REPO_REQUIRE(rows > 0 && rows < kMaxIdx && K >= 2 && K <= kThMaxK && ld >= K, REPO_E_SHAPE);
  REPO_REQUIRE(logits && v_out && th_bounds_ok(low, high) && th_space_ok(space, low, high), REPO_E_BADARG);
  const ThBins bins = th_bins(low, high, K);
  const int blocks = red_blocks(rows, kThRowsPerBlock);
#define LAUNCH(NC)                                                                                                   \
  hipLaunchKernelGGL(twohot_decode_s1_kernel<NC>, dim3(blocks), dim3(256), 0, stream, (long)rows, (int)K, logits,    \
                     (long)ld, bins, th_vec(logits, ld), v_out, m_out)
  TH_DISPATCH((int)K, LAUNCH);
#undef LAUNCH
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_twohot_decode_bwd_x(int64_t rows, int64_t K, const float* logits, int64_t ld, float low, float high,
                                        int space, const float* g, float* dlogits, int64_t ldd, const float* gmul,
                                        hipStream_t stream) {
  if (space == 0) return repo_twohot_decode_bwd(rows, K, logits, ld, low, high, g, dlogits, ldd, gmul, stream);
  REPO_ARCH_GUARD();
  REPO_REQUIRE(rows > 0 && rows < kMaxIdx && K >= 2 && K <= kThMaxK && ld >= K && ldd >= K, REPO_E_SHAPE);
  REPO_REQUIRE(logits && g && dlogits && th_bounds_ok(low, high) && th_space_ok(space, low, high), REPO_E_BADARG);
  const ThBins bins = th_bins(low, high, K);
  const int blocks = red_blocks(rows, kThRowsPerBlock);
#define LAUNCH(NC)                                                                                                      \
  hipLaunchKernelGGL(twohot_decode_bwd_s1_kernel<NC>, dim3(blocks), dim3(256), 0, stream, (long)rows, (int)K, logits,   \
                     (long)ld, bins, th_vec(logits, ld), g, dlogits, (long)ldd, th_vec(dlogits, ldd), gmul)
  TH_DISPATCH((int)K, LAUNCH);
#undef LAUNCH
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_twohot_nll_x(int64_t rows, int64_t K, const float* logits, int64_t ld, const float* target_a,
                                 const float* target_b, float reg, const float* weights, float low, float high, int space,
                                 float scale, float* dlogits, int64_t ldd, float* sums3, void* ws, size_t ws_bytes,
                                 hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(rows > 0 && rows < kMaxIdx && K >= 2 && K <= kThMaxK && ld >= K && (!dlogits || ldd >= K), REPO_E_SHAPE);
  REPO_REQUIRE(logits && target_a && sums3 && th_bounds_ok(low, high) && th_space_ok(space, low, high), REPO_E_BADARG);
  REPO_REQUIRE(!target_b || (std::isfinite(reg) && reg >= 0.f), REPO_E_BADARG);
  REPO_REQUIRE(ws && ws_bytes >= repo_twohot_nll_x_workspace_bytes(), REPO_E_WS_TOO_SMALL);
  return th_nll_launch(rows, K, logits, ld, target_a, target_b, target_b ? reg : 0.f, weights, low, high, space, scale,
                       dlogits, ldd, sums3, 3, ws, stream);
}
