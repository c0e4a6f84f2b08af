// Return normalisation (config.return_norm): two exact order statistics of the imagined lambda-returns by
// radix select, the running percentile range they feed, and the device-side scalar that carries 1 / max(limit, range)
// into the actor's gradients without a host read.
#include "common.h"

namespace repo {

// ------------------------------------------------------------------ radix select of two ranks
// ONE workgroup of kSelThreads walks x once per 8-bit digit, most significant first: four passes over an array of a few
// hundred KB that the lambda-return launch has just left in L2.  Each pass counts, per rank, the digit of every element
// whose higher digits equal the rank's prefix (LDS integer atomics only), then one wave per rank scans its 256 counts and
// extends the prefix by the digit its rank falls into.  While both ranks still share a prefix (always in pass 0) one
// histogram serves both.  Counts are integers: the result is THE k-th smallest key whatever the schedule.
// Four passes of fixed length and no data-dependent loop: the kernel ends on any input.
constexpr int kSelThreads = 1024;
// elements per thread per trip of the walk (kSelThreads * kSelUnroll elements per trip).  The walk is bound by the one
// CU's instruction issue (about 30 instructions per element and pass), not by its loads: 16 per trip measured slower than
// 4 at the flagship update's 34300 returns.
constexpr int kSelUnroll = 4;

// order-preserving key of the fp32 bits: -0 and +0 share the key of +0, every NaN gets the largest key
__device__ __forceinline__ unsigned sel_key(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if ((u << 1) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_val(unsigned k) {
  if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// ++h[d] for the lanes with m set.  Imagined returns share their sign and most of their exponent, so in the first passes
// most of a wave hits one counter: the lanes that share the first counting lane's digit add their number once, the rest add
// one each.  Called by whole waves.
__device__ __forceinline__ void sel_count(unsigned* h, bool m, unsigned d) {
  const unsigned long long act = __ballot(m);
  if (!act) return;   // (wave-uniform)
  const int lead = __ffsll((long long)act) - 1;
  const unsigned dl = (unsigned)__shfl((int)d, lead, 64);
  const unsigned long long eq = __ballot(m && d == dl);
  if ((int)(threadIdx.x & 63) == lead) atomicAdd(&h[dl], (unsigned)__popcll(eq));
  else if (m && d != dl) atomicAdd(&h[d], 1u);
}

// The guard, the EMA, the scale and its inverse (one thread).  out4 = {lo_b, hi_b, scale, inv}.
__device__ __forceinline__ void return_scale_epilogue(float lo_b, float hi_b, float decay, float limit,
                                                      float* __restrict__ state2, float* __restrict__ out4,
                                                      int update_state, const unsigned* __restrict__ skip) {
  float lo = state2[0], hi = state2[1];
  // a non-finite batch statistic or a faulted update leaves the state alone: a NaN in the EMA would never leave it
  const bool ok = isfinite(lo_b) && isfinite(hi_b) && !(skip && *skip);
  if (ok && update_state) {
    const float om = 1.f - decay;
    lo = fmaf(decay, lo, om * lo_b);
    hi = fmaf(decay, hi, om * hi_b);
    state2[0] = lo;
    state2[1] = hi;
  }
  const float scale = fmaxf(limit, hi - lo);
  out4[0] = lo_b;
  out4[1] = hi_b;
  out4[2] = scale;
  out4[3] = 1.f / scale;
}

__global__ __launch_bounds__(kSelThreads) void return_scale_kernel(long n, const float* __restrict__ x, unsigned k_lo,
                                                                   unsigned k_hi, float decay, float limit,
                                                                   float* __restrict__ state2, float* __restrict__ out4,
                                                                   int update_state, const unsigned* __restrict__ skip) {
  __shared__ unsigned hist[2][256];
  __shared__ unsigned s_prefix[2], s_k[2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) {
    s_prefix[0] = s_prefix[1] = 0u;
    s_k[0] = k_lo;
    s_k[1] = k_hi;
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 512) (&hist[0][0])[tid] = 0u;
    __syncthreads();
    const unsigned p0 = s_prefix[0], p1 = s_prefix[1];
    const unsigned himask = pass ? 0xffffffffu << (shift + 8) : 0u;   // the digits above this pass's
    const bool same = p0 == p1;                                        // (block-uniform) one histogram serves both ranks
    for (long base = 0; base < n; base += kSelThreads * kSelUnroll) {
      unsigned key[kSelUnroll];
      bool in[kSelUnroll];
#pragma unroll
      for (int u = 0; u < kSelUnroll; ++u) {
        const long i = base + u * kSelThreads + tid;
        in[u] = i < n;
        key[u] = in[u] ? sel_key(x[i]) : 0u;
      }
#pragma unroll
      for (int u = 0; u < kSelUnroll; ++u) {
        const unsigned d = (key[u] >> shift) & 255u;
        sel_count(hist[0], in[u] && ((key[u] ^ p0) & himask) == 0u, d);
        if (!same) sel_count(hist[1], in[u] && ((key[u] ^ p1) & himask) == 0u, d);
      }
    }
    __syncthreads();
    if (wid < 2) {   // wave r extends rank r's prefix: lane l owns counts 4l .. 4l+3
      const unsigned* h = hist[same ? 0 : wid];
      const unsigned k = s_k[wid];
      unsigned c[4], s = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[j] = h[4 * lane + j];
        s += c[j];
      }
      unsigned incl = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)incl, o, 64);
        if (lane >= o) incl += t;
      }
      const unsigned excl = incl - s;
      // the counted elements number more than k (n > k at the start, then by construction): exactly one lane holds it
      if (excl <= k && k < incl) {
        unsigned kk = k - excl;
        int j = 0;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          if (j == t && kk >= c[t]) {
            kk -= c[t];
            j = t + 1;
          }
        }
        const unsigned d = 4u * lane + j;
        s_prefix[wid] = (wid ? p1 : p0) | (d << shift);
        s_k[wid] = kk;
      }
    }
    __syncthreads();
  }
  if (tid == 0)
    return_scale_epilogue(sel_val(s_prefix[0]), sel_val(s_prefix[1]), decay, limit, state2, out4, update_state, skip);
}

// the epilogue alone, on batch statistics that were averaged over the ranks of a data-parallel job
__global__ void return_scale_finish_kernel(const float* __restrict__ batch2, float decay, float limit,
                                           float* __restrict__ state2, float* __restrict__ out4, int update_state,
                                           const unsigned* __restrict__ skip) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  return_scale_epilogue(batch2[0], batch2[1], decay, limit, state2, out4, update_state, skip);
}

// a, b, c (b, c nullable) *= *gmul, n elements each
__global__ __launch_bounds__(256) void scale_by_kernel(long n, float* __restrict__ a, float* __restrict__ b,
                                                       float* __restrict__ c, const float* __restrict__ gmul) {
  const float g = *gmul;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    a[i] *= g;
    if (b) b[i] *= g;
    if (c) c[i] *= g;
  }
}

}  // namespace repo

using namespace repo;

extern "C" int repo_return_scale_geometry(int* threads, int* per_trip) {
  REPO_REQUIRE(threads && per_trip, REPO_E_BADARG);
  *threads = kSelThreads;
  *per_trip = kSelThreads * kSelUnroll;
  return REPO_OK;
}

extern "C" int repo_return_scale(int64_t n, const float* x, int64_t k_lo, int64_t k_hi, float decay, float limit,
                                 float* state2, float* out4, int update_state, const unsigned* skip_if_nonzero, void* ws,
                                 size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(n > 0 && n < kMaxIdx && k_lo >= 0 && k_hi < n && k_lo <= k_hi, REPO_E_SHAPE);
  REPO_REQUIRE(x && state2 && out4, REPO_E_BADARG);
  // the reduction workspace's contract, like the streaming reductions beside it: a several-workgroup form can take this
  // kernel's place behind the same signature.  The one-workgroup kernel does not touch it.
  REPO_REQUIRE(ws && ws_bytes >= repo_reduce_workspace_bytes(), REPO_E_WS_TOO_SMALL);
  hipLaunchKernelGGL(return_scale_kernel, dim3(1), dim3(kSelThreads), 0, stream, (long)n, x, (unsigned)k_lo,
                     (unsigned)k_hi, decay, limit, state2, out4, update_state, skip_if_nonzero);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_return_scale_finish(const float* batch2, float decay, float limit, float* state2, float* out4,
                                        int update_state, const unsigned* skip_if_nonzero, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(batch2 && state2 && out4, REPO_E_BADARG);
  hipLaunchKernelGGL(return_scale_finish_kernel, dim3(1), dim3(64), 0, stream, batch2, decay, limit, state2, out4,
                     update_state, skip_if_nonzero);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_scale_by(int64_t n, float* a, float* b, float* c, const float* gmul, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(n > 0 && n < kMaxIdx, REPO_E_SHAPE);
  REPO_REQUIRE(a && gmul, REPO_E_BADARG);
  long blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(scale_by_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (long)n, a, b, c, gmul);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}
