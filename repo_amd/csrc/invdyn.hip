// The inverse-dynamics auxiliary (config.inv_dynamics; reference dreamer.py:220-239, models/utils.py:84-109): the two
// passes around its dense chain.  repo_inv_dyn_pack forms the model's input rows from the observe scan's output
// (repo_inv_dyn_pack_pair from two column blocks of it, repo_inv_dyn_unpack_pair is that pack's adjoint), and
// repo_normal_nll_rows is the masked Normal NLL of the action head with its gradient and the data-dependent row count.
// Both are HBM-bound streaming kernels; the reduction follows loss.hip (wave64 shuffles, one partial per workgroup,
// the launch's last block sums them in a fixed order: common.h, last_block_finishes -- no float atomics).
#include "common.h"

namespace repo {

template <int V>
struct PackVec;
template <>
struct PackVec<1> { using type = float; };
template <>
struct PackVec<2> { using type = float2; };
template <>
struct PackVec<4> { using type = float4; };

// x[r] = [feat[r][0:F] | feat[r + B][0:D]], r < N: both halves of a row are runs of consecutive floats, copied V floats
// per thread.  The host picks the largest V in {4, 2, 1} for which every run starts on a V-float boundary (F, D, ldfeat,
// ldx multiples of V and both bases V * 4 bytes aligned), so a V-wide access never straddles the seam at column F and
// never leaves its alignment: D + S = 230 copies as float2, odd widths float by float.
template <int V>
__global__ __launch_bounds__(256) void inv_dyn_pack_kernel(long total, int wv, int F, int B, const float* __restrict__ feat,
                                                           long ldfeat, float* __restrict__ x, long ldx) {
  using T = typename PackVec<V>::type;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / wv;
    const int c = (int)(i - r * wv) * V;
    const float* src = c < F ? feat + r * ldfeat + c : feat + (r + B) * ldfeat + (c - F);
    *reinterpret_cast<T*>(x + r * ldx + c) = *reinterpret_cast<const T*>(src);
  }
}

// The same rows from TWO column blocks of a wider scan output (CalibratedRePo's "pair" step):
// x[t * B + b] = [cur[t][b][0:F] | next[t + 1][b][0:D]], each block with its own row pitch (ld) and time pitch (td).
template <int V>
__global__ __launch_bounds__(256) void inv_dyn_pack_pair_kernel(long total, int wv, int F, int B,
                                                                const float* __restrict__ cur, long ldc, long tdc,
                                                                const float* __restrict__ next, long ldn, long tdn,
                                                                float* __restrict__ x, long ldx) {
  using T = typename PackVec<V>::type;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / wv;
    const int c = (int)(i - r * wv) * V;
    const long t = r / B, b = r - t * B;
    const float* src = c < F ? cur + t * tdc + b * ldc + c : next + (t + 1) * tdn + b * ldn + (c - F);
    *reinterpret_cast<T*>(x + r * ldx + c) = *reinterpret_cast<const T*>(src);
  }
}

// The adjoint of the pack in gather form: one thread per element (t, b, c) of the (T, B, F) block dfeat, no atomics.
//   c < F, t <= T-2 (and dx_cur given):  scale_cur  * dx_cur[(t, b)][c]          the row's own [belief_t | state_t]
//   c < D, t >= 1:                       scale_next * dx_next[(t-1, b)][F + c]   belief_t as the row before's "next"
// Each term is one rounded multiply and their sum one rounded add (no contraction into an fma); an element neither term
// reaches gets an exact zero, written.
__global__ __launch_bounds__(256) void inv_dyn_unpack_pair_kernel(long total, int T, int B, int D, int F,
                                                                  const float* __restrict__ dx_cur, long ldxc,
                                                                  const float* __restrict__ dx_next, long ldxn,
                                                                  float scale_cur, float scale_next,
                                                                  float* __restrict__ dfeat, long ldf, long tdf,
                                                                  int accumulate) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long tb = i / F;
    const int c = (int)(i - tb * F);
    const long t = tb / B, b = tb - t * B;
    const bool has_cur = dx_cur && t <= T - 2, has_next = c < D && t >= 1;
    float v = 0.f;
    if (has_cur) v = __fmul_rn(scale_cur, dx_cur[(t * B + b) * ldxc + c]);
    if (has_next) {
      const float nx = __fmul_rn(scale_next, dx_next[((t - 1) * B + b) * ldxn + F + c]);
      v = has_cur ? __fadd_rn(v, nx) : nx;
    }
    float* dst = dfeat + t * tdf + b * ldf + c;
    *dst = accumulate ? __fadd_rn(*dst, v) : v;
  }
}

// F.softplus(beta=1, threshold=20) and its derivative.  The per-element math of this kernel runs in fp64 and is rounded
// once: N * A elements (14400 per update at the workload) make it a launch-latency kernel whatever the arithmetic costs,
// and z^2 / std near std = min_std amplifies every fp32 rounding of std into the gradient.  Sums accumulate in fp32.
__device__ __forceinline__ double softplus_d(double x) { return x > 20.0 ? x : log1p(exp(x)); }
__device__ __forceinline__ double softplus_grad_d(double x) { return x > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-x)); }

// Element e = row * A + j of the (N, A) action block.  raw[row] = [mean (A) | pre-softplus std (A)].
//   parts[0][blk] = sum over selected elements of 0.5 z^2 + log std + 0.5 log 2 pi
//   parts[1][blk] = selected rows (counted once per row, at j == 0)
//   draw[row]     = d(mean over the selected rows of the row NLL) / d raw[row]; exact zeros on unselected rows
// The divisor of the gradient is *count_in, or (count_in == nullptr) the number of selected rows, which EVERY block
// counts for itself from the whole mask before its element loop: a sum of zeros and ones below 2^24 is exact in fp32
// in any order (the entry point takes N <= 2^20: 64 blocks then read 4 MB of mask each, from L2), so all blocks hold the bits of sums[1] without a second launch or a grid-wide wait.
__global__ __launch_bounds__(256) void normal_nll_rows_kernel(int N, int A, const float* __restrict__ raw, long ldraw,
                                                              const float* __restrict__ target, long ldt,
                                                              const float* __restrict__ mask,
                                                              const float* __restrict__ count_in, float min_std,
                                                              float* __restrict__ draw, long lddraw,
                                                              float* __restrict__ parts, float* __restrict__ red_out,
                                                              unsigned* __restrict__ ticket) {
  __shared__ float red[16];
  __shared__ float s_inv;
  if (draw) {   // (kernel argument: uniform)
    float cnt;
    if (count_in) {
      cnt = *count_in;
    } else {
      float c = 0.f;
      for (int r = threadIdx.x; r < N; r += blockDim.x) c += mask[r] == 1.f ? 1.f : 0.f;
      cnt = block_sum(c, red);   // valid in thread 0
    }
    if (threadIdx.x == 0) s_inv = cnt > 0.f ? 1.f / cnt : 0.f;
    __syncthreads();
  }
  const float inv = draw ? s_inv : 0.f;
  const long n = (long)N * A;
  float acc = 0.f, rows = 0.f;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const int row = (int)(e / A), j = (int)(e - (long)row * A);
    const bool sel = mask[row] == 1.f;
    float gm = 0.f, gs = 0.f;
    if (sel) {
      const double m = raw[row * ldraw + j], rs = raw[row * ldraw + A + j];
      const double sd = softplus_d(rs) + (double)min_std;
      const double z = ((double)target[row * ldt + j] - m) / sd;
      acc += (float)(0.5 * z * z + log(sd) + 0.9189385332046727);   // 0.5 log 2 pi
      if (j == 0) rows += 1.f;
      gm = (float)(-z / sd * (double)inv);
      gs = (float)((1.0 - z * z) / sd * softplus_grad_d(rs) * (double)inv);
    }
    if (draw) {
      draw[row * lddraw + j] = gm;
      draw[row * lddraw + A + j] = gs;
    }
  }
  const float s0 = block_sum(acc, red);
  const float s1 = block_sum(rows, red);
  if (threadIdx.x == 0) {
    parts[blockIdx.x] = s0;
    parts[gridDim.x + blockIdx.x] = s1;
  }
  last_block_finishes(parts, 2, red_out, ticket, red);
}

static inline bool aligned_to(const void* p, size_t bytes) { return (uintptr_t)p % bytes == 0; }

}  // namespace repo

using namespace repo;

extern "C" int repo_inv_dyn_pack(int64_t T, int64_t B, int64_t D, int64_t S, const float* featx, int64_t ldfeat, float* x,
                                 int64_t ldx, hipStream_t stream) {
  REPO_ARCH_GUARD();
  const int64_t F = D + S, W = F + D, N = (T - 1) * B;
  REPO_REQUIRE(T >= 2 && B > 0 && D > 0 && S > 0 && ldfeat >= F && ldx >= W, REPO_E_SHAPE);
  REPO_REQUIRE(T * B * ldfeat < kMaxIdx && N * ldx < kMaxIdx, REPO_E_SHAPE);
  REPO_REQUIRE(featx && x, REPO_E_BADARG);
  int V = 1;
  for (int v = 4; v > 1 && V == 1; v >>= 1)
    if (F % v == 0 && D % v == 0 && ldfeat % v == 0 && ldx % v == 0 && aligned_to(featx, 4 * v) && aligned_to(x, 4 * v))
      V = v;
  const int wv = (int)(W / V);
  const long total = (long)N * wv;
  const int blocks = (int)(cdiv(total, 256) > 4096 ? 4096 : cdiv(total, 256));
  if (V == 4)
    hipLaunchKernelGGL(inv_dyn_pack_kernel<4>, dim3(blocks), dim3(256), 0, stream, total, wv, (int)F, (int)B, featx,
                       (long)ldfeat, x, (long)ldx);
  else if (V == 2)
    hipLaunchKernelGGL(inv_dyn_pack_kernel<2>, dim3(blocks), dim3(256), 0, stream, total, wv, (int)F, (int)B, featx,
                       (long)ldfeat, x, (long)ldx);
  else
    hipLaunchKernelGGL(inv_dyn_pack_kernel<1>, dim3(blocks), dim3(256), 0, stream, total, wv, (int)F, (int)B, featx,
                       (long)ldfeat, x, (long)ldx);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_inv_dyn_pack_pair(int64_t T, int64_t B, int64_t D, int64_t S, const float* cur, int64_t ldcur,
                                      int64_t tdcur, const float* next, int64_t ldnext, int64_t tdnext, float* x,
                                      int64_t ldx, hipStream_t stream) {
  REPO_ARCH_GUARD();
  const int64_t F = D + S, W = F + D, N = (T - 1) * B;
  REPO_REQUIRE(T >= 2 && B > 0 && D > 0 && S > 0 && ldcur >= F && ldnext >= F && tdcur >= B * ldcur &&
                   tdnext >= B * ldnext && ldx >= W,
               REPO_E_SHAPE);
  REPO_REQUIRE(T * tdcur < kMaxIdx && T * tdnext < kMaxIdx && N * ldx < kMaxIdx, REPO_E_SHAPE);
  REPO_REQUIRE(cur && next && x, REPO_E_BADARG);
  // the rule of repo_inv_dyn_pack with the column offsets (in the bases) and the time pitches included
  int V = 1;
  for (int v = 4; v > 1 && V == 1; v >>= 1)
    if (F % v == 0 && D % v == 0 && ldcur % v == 0 && tdcur % v == 0 && ldnext % v == 0 && tdnext % v == 0 &&
        ldx % v == 0 && aligned_to(cur, 4 * v) && aligned_to(next, 4 * v) && aligned_to(x, 4 * v))
      V = v;
  const int wv = (int)(W / V);
  const long total = (long)N * wv;
  const int blocks = (int)(cdiv(total, 256) > 4096 ? 4096 : cdiv(total, 256));
  auto go = [&](auto k) {
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, stream, total, wv, (int)F, (int)B, cur, (long)ldcur, (long)tdcur,
                       next, (long)ldnext, (long)tdnext, x, (long)ldx);
  };
  if (V == 4)
    go(inv_dyn_pack_pair_kernel<4>);
  else if (V == 2)
    go(inv_dyn_pack_pair_kernel<2>);
  else
    go(inv_dyn_pack_pair_kernel<1>);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_inv_dyn_unpack_pair(int64_t T, int64_t B, int64_t D, int64_t S, const float* dx_cur, int64_t lddx_cur,
                                        const float* dx_next, int64_t lddx_next, float scale_cur, float scale_next,
                                        float* dfeat, int64_t lddfeat, int64_t tddfeat, int accumulate,
                                        hipStream_t stream) {
  REPO_ARCH_GUARD();
  const int64_t F = D + S, W = F + D, N = (T - 1) * B;
  REPO_REQUIRE(T >= 2 && B > 0 && D > 0 && S > 0 && lddfeat >= F && tddfeat >= B * lddfeat && lddx_next >= W &&
                   (!dx_cur || lddx_cur >= W),
               REPO_E_SHAPE);
  REPO_REQUIRE(T * tddfeat < kMaxIdx && N * lddx_next < kMaxIdx && (!dx_cur || N * lddx_cur < kMaxIdx), REPO_E_SHAPE);
  REPO_REQUIRE(dx_next && dfeat, REPO_E_BADARG);
  const long total = (long)(T * B * F);
  const int blocks = (int)(cdiv(total, 256) > 4096 ? 4096 : cdiv(total, 256));
  hipLaunchKernelGGL(inv_dyn_unpack_pair_kernel, dim3(blocks), dim3(256), 0, stream, total, (int)T, (int)B, (int)D, (int)F,
                     dx_cur, (long)lddx_cur, dx_next, (long)lddx_next, scale_cur, scale_next, dfeat, (long)lddfeat,
                     (long)tddfeat, accumulate != 0);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" size_t repo_normal_nll_rows_workspace_bytes(void) {
  return kRedHeaderBytes + 2 * kLastBlockMaxGrid * sizeof(float);
}

extern "C" int repo_normal_nll_rows(int64_t N, int64_t A, const float* raw, int64_t ldraw, const float* target,
                                    int64_t ldt, const float* mask, const float* count_in, float min_std, float* sums,
                                    float* draw, int64_t lddraw, void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  // N <= 2^20: the row counts are fp32 sums of ones and must stay exact, and every block reads the whole mask once for
  // its divisor (kernel comment) -- at most 64 blocks x 4 MB, from L2; the update's N is (L - 2) * B = 2400
  REPO_REQUIRE(N > 0 && N <= (1 << 20) && A > 0 && ldraw >= 2 * A && ldt >= A && (!draw || lddraw >= 2 * A), REPO_E_SHAPE);
  REPO_REQUIRE(N * ldraw < kMaxIdx && N * ldt < kMaxIdx && (!draw || N * lddraw < kMaxIdx), REPO_E_SHAPE);
  REPO_REQUIRE(raw && target && mask && sums, REPO_E_BADARG);
  REPO_REQUIRE(ws && ws_bytes >= repo_normal_nll_rows_workspace_bytes(), REPO_E_WS_TOO_SMALL);
  // at most kLastBlockMaxGrid blocks, so that the launch always finishes its own sums (common.h)
  int blocks = cdiv(N * A, 1024);
  if (blocks > kLastBlockMaxGrid) blocks = kLastBlockMaxGrid;
  hipLaunchKernelGGL(normal_nll_rows_kernel, dim3(blocks), dim3(256), 0, stream, (int)N, (int)A, raw, (long)ldraw, target,
                     (long)ldt, mask, count_in, min_std, draw, (long)lddraw, (float*)((char*)ws + kRedHeaderBytes), sums,
                     (unsigned*)ws);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}
