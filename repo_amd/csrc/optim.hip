// Flat-buffer optimiser: global gradient norm + fused clip_grad_norm_ and Adam.
// Replaces nn.utils.clip_grad_norm_ + torch.optim.Adam.step over 40 / 10 / 8 tensors
// (algorithms/repo/repo.py:87-90, dreamer.py:356-359,370-373) with two HBM-bound passes
// over one contiguous parameter / gradient / moment buffer.
#include "common.h"

namespace repo {

__global__ __launch_bounds__(256) void sqnorm_kernel(int64_t n, const float* __restrict__ g, float* __restrict__ parts) {
  __shared__ float red[16];
  float acc = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      const float4 v = *reinterpret_cast<const float4*>(g + i);
      acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    } else {
      for (int64_t j = i; j < n; ++j) acc += g[j] * g[j];
    }
  }
  const float s = block_sum(acc, red);
  if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

__global__ void sqnorm_final_kernel(const float* __restrict__ parts, int n, float* __restrict__ out) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += parts[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) *out = s;
}

// clip_coef = min(1, max_norm / (sqrt(sqnorm) + 1e-6)); g *= clip_coef; Adam (no weight decay, no amsgrad)
__global__ __launch_bounds__(256) void clip_adam_kernel(int64_t n, float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        const float* __restrict__ sqnorm, float max_norm, float lr_bc1,
                                                        float b1, float b2, float eps, float inv_bc2_sqrt,
                                                        const unsigned* __restrict__ skip) {
  if (skip && *skip) return;   // a faulted update (scan timeout: NaN gradients) must not touch the model
  float coef = 1.f;
  if (sqnorm) {
    coef = max_norm / (sqrtf(*sqnorm) + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;
  }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gg = g[i] * coef;
    const float mm = b1 * m[i] + (1.f - b1) * gg;
    const float vv = b2 * v[i] + (1.f - b2) * gg * gg;
    m[i] = mm;
    v[i] = vv;
    p[i] = p[i] - lr_bc1 * (mm / (sqrtf(vv) * inv_bc2_sqrt + eps));
  }
}

// clip_adam_kernel's update (the same expressions, so the same bits in p, m, v) and, in the same pass, the slow target's
// mix from the parameter value just written: t += fraction * (p_new - t); fraction == 1 stores p_new itself
// (config.slow_value_target).  One skip word for all four buffers: they move together or not at all.
__global__ __launch_bounds__(256) void clip_adam_target_kernel(int64_t n, float* __restrict__ p, const float* __restrict__ g,
                                                               float* __restrict__ m, float* __restrict__ v,
                                                               const float* __restrict__ sqnorm, float max_norm,
                                                               float lr_bc1, float b1, float b2, float eps,
                                                               float inv_bc2_sqrt, const unsigned* __restrict__ skip,
                                                               float* __restrict__ t, float fraction) {
  if (skip && *skip) return;
  float coef = 1.f;
  if (sqnorm) {
    coef = max_norm / (sqrtf(*sqnorm) + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;
  }
  const bool copy = fraction == 1.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gg = g[i] * coef;
    const float mm = b1 * m[i] + (1.f - b1) * gg;
    const float vv = b2 * v[i] + (1.f - b2) * gg * gg;
    m[i] = mm;
    v[i] = vv;
    const float pn = p[i] - lr_bc1 * (mm / (sqrtf(vv) * inv_bc2_sqrt + eps));
    p[i] = pn;
    const float tt = t[i];
    const float d = pn - tt;
    t[i] = copy ? pn : fmaf(fraction, d, tt);
  }
}

// ---------------------------------------------------------------------------------------------------- AGC + LaProp (6p)
// Per-tensor adaptive gradient clipping (config.grad_clip = "agc") and the LaProp update (config.optimizer = "laprop"),
// DESIGN.md 6p.  The flat buffer is cut into CHUNKS of at most kAgcChunk elements that never cross a tensor: the table
// (int4 {offset, numel, segment, 0} per chunk, built once by the caller) is what both kernels walk.
constexpr int kAgcChunk = 4096;       // elements per chunk (a multiple of 4: every chunk starts 16-byte aligned)
constexpr int kAgcMaxBlocks = 1024;   // agc_parts_kernel's grid cap: a block takes chunks b, b + grid, ...
constexpr int kAgcFinishThreads = 256;   // agc_finish_kernel: one block, one WAVE (64 lanes) per segment at a time
constexpr int kStepMaxBlocks = 2048;  // the step kernel's grid cap (clip_adam_kernel's)
constexpr int kAgcMaxChunks = 1 << 30;   // 2 * chunk + 1 and 2 * segment + 1 index the partials and the norms as ints

// parts[2 c] = sum g^2, parts[2 c + 1] = sum p^2 over chunk c's own `numel` elements (never the padding behind a tensor).
// A table entry outside [0, n) poisons its partials with NaN and reads nothing.
__global__ __launch_bounds__(256) void agc_parts_kernel(int nchunk, const int4* __restrict__ chunks, int64_t n,
                                                        const float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ parts) {
  __shared__ float red[16];
  for (int c = blockIdx.x; c < nchunk; c += gridDim.x) {
    const int4 ch = chunks[c];
    const int64_t off = ch.x;
    const int len = ch.y;
    float ag = 0.f, ap = 0.f;
    const bool ok = ch.x >= 0 && len > 0 && len <= kAgcChunk && off + len <= n && (ch.x & 3) == 0;
    if (ok) {
      for (int i = threadIdx.x * 4; i < len; i += 256 * 4) {
        if (i + 3 < len) {
          const float4 a = *reinterpret_cast<const float4*>(g + off + i);
          const float4 b = *reinterpret_cast<const float4*>(p + off + i);
          ag += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
          ap += b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
        } else {
          for (int j = i; j < len; ++j) {
            ag += g[off + j] * g[off + j];
            ap += p[off + j] * p[off + j];
          }
        }
      }
    } else {
      ag = ap = __builtin_nanf("");
    }
    const float sg = block_sum(ag, red);
    const float sp = block_sum(ap, red);
    if (threadIdx.x == 0) {
      parts[2 * c] = sg;
      parts[2 * c + 1] = sp;
    }
  }
}

// One block.  Wave w takes segments w, w + 4, ...: its lanes stride the segment's chunks [seg_first[s], seg_first[s + 1])
// and a wave_sum closes them (a fixed order for a given table).  norms[2 s] = |g_s|^2, norms[2 s + 1] = |p_s|^2,
//   upper = clip * max(pmin, |p_s|);  coef[s] = |g_s| <= upper ? 1 : upper / |g_s|   (a NaN norm: a NaN coefficient)
// then stats[0] = sum_s |g_s|^2 in thread order over s (the pre-clip global squared norm), stats[1] = #{s: coef < 1}.
__global__ __launch_bounds__(kAgcFinishThreads) void agc_finish_kernel(int nseg, int nchunk,
                                                                       const int* __restrict__ seg_first,
                                                                       const float* __restrict__ parts, float clip,
                                                                       float pmin, float* __restrict__ norms,
                                                                       float* __restrict__ coef,
                                                                       float* __restrict__ stats) {
  __shared__ float red[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int s = wid; s < nseg; s += nw) {
    const int c0 = seg_first[s], c1 = seg_first[s + 1];
    float ag = 0.f, ap = 0.f;
    if (c0 < 0 || c1 > nchunk || c1 <= c0) ag = ap = __builtin_nanf("");   // (a table that is not one: poison, read nothing)
    else for (int c = c0 + lane; c < c1; c += 64) {
      ag += parts[2 * c];
      ap += parts[2 * c + 1];
    }
    ag = wave_sum(ag);
    ap = wave_sum(ap);
    if (lane == 0) {
      const float unorm = sqrtf(ag), pnorm = sqrtf(ap);
      const float floor = (pnorm >= pmin || pnorm != pnorm) ? pnorm : pmin;
      const float upper = clip * floor;
      norms[2 * s] = ag;
      norms[2 * s + 1] = ap;
      coef[s] = unorm <= upper ? 1.f : upper / unorm;
    }
  }
  __syncthreads();   // (one block: its own global writes are visible to it behind the barrier)
  float tg = 0.f, tc = 0.f;
  for (int s = threadIdx.x; s < nseg; s += blockDim.x) {
    tg += norms[2 * s];
    tc += coef[s] < 1.f ? 1.f : 0.f;
  }
  const float sg = block_sum(tg, red);
  const float sc = block_sum(tc, red);
  if (threadIdx.x == 0) {
    stats[0] = sg;
    stats[1] = sc;
  }
}

// The one step launch of DESIGN.md 6p.  RULE 0: Adam (clip_adam_kernel's expressions, so its bits), 1: LaProp.  CLIP 0:
// none, 1: the global coefficient of clip_adam_kernel from *sqnorm, 2: the per-tensor table.  TARGET: clip_adam_target_kernel's
// mix behind the parameter write.  One skip word for every buffer.
// Every product, sum and fused multiply-add is spelled out and contraction is off, so that all twelve instantiations
// round alike; the Adam branch spells what clip_adam_kernel compiles to (tests/test_optim_rules_gpu.py holds the two equal).
template <int RULE>
__device__ __forceinline__ float rule_step(float pp, float gg, float& mm, float& vv, float lr_bc1, float b1, float b2,
                                           float eps, float inv_bc2_sqrt) {
#pragma clang fp contract(off)
  const float g2 = ((1.f - b2) * gg) * gg;
  vv = b2 * vv + g2;
  const float den = fmaf(sqrtf(vv), inv_bc2_sqrt, eps);
  if (RULE == 0) {
    mm = fmaf(1.f - b1, gg, b1 * mm);
    return fmaf(-lr_bc1, mm / den, pp);
  }
  const float u = gg / den;
  mm = fmaf(1.f - b1, u, b1 * mm);
  return fmaf(-lr_bc1, mm, pp);
}

template <int RULE, int CLIP, bool TARGET>
__global__ __launch_bounds__(256) void optim_step_kernel(int64_t n, float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v,
                                                         const float* __restrict__ sqnorm, float max_norm,
                                                         int nchunk, int nseg, const int4* __restrict__ chunks,
                                                         const float* __restrict__ coefs, float lr_bc1, float b1, float b2,
                                                         float eps, float inv_bc2_sqrt, const unsigned* __restrict__ skip,
                                                         float* __restrict__ t, float fraction) {
  if (skip && *skip) return;
  const bool copy = fraction == 1.f;
  auto one = [&](int64_t i, float coef) {
    const float gg = CLIP == 0 ? g[i] : g[i] * coef;
    float mm = m[i], vv = v[i];
    const float pn = rule_step<RULE>(p[i], gg, mm, vv, lr_bc1, b1, b2, eps, inv_bc2_sqrt);
    m[i] = mm;
    v[i] = vv;
    p[i] = pn;
    if (TARGET) {
      const float tt = t[i];
      const float d = pn - tt;
      t[i] = copy ? pn : fmaf(fraction, d, tt);
    }
  };
  if (CLIP == 2) {
    // chunk by chunk, the padding lanes behind a tensor's last chunk included (zero gradient, the tensor's coefficient)
    for (int c = blockIdx.x; c < nchunk; c += gridDim.x) {
      const int4 ch = chunks[c];
      const int64_t off = ch.x;
      const int len4 = (ch.y + 3) & ~3;
      if (ch.x < 0 || ch.y <= 0 || ch.y > kAgcChunk || off + len4 > n || ch.z < 0 || ch.z >= nseg) continue;
      const float coef = coefs[ch.z];
      for (int i = threadIdx.x; i < len4; i += 256) one(off + i, coef);
    }
  } else {
    float coef = 1.f;
    if (CLIP == 1) {
      coef = max_norm / (sqrtf(*sqnorm) + 1e-6f);
      coef = coef > 1.f ? 1.f : coef;
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) one(i, coef);
  }
}

template <int RULE, int CLIP>
static void launch_step(bool target, dim3 grid, hipStream_t stream, int64_t n, float* p, const float* g, float* m, float* v,
                        const float* sqnorm, float max_norm, int nchunk, int nseg, const int4* chunks, const float* coefs, float lr_bc1,
                        float b1, float b2, float eps, float ibc2, const unsigned* skip, float* t, float fraction) {
  if (target)
    hipLaunchKernelGGL((optim_step_kernel<RULE, CLIP, true>), grid, dim3(256), 0, stream, n, p, g, m, v, sqnorm, max_norm,
                       nchunk, nseg, chunks, coefs, lr_bc1, b1, b2, eps, ibc2, skip, t, fraction);
  else
    hipLaunchKernelGGL((optim_step_kernel<RULE, CLIP, false>), grid, dim3(256), 0, stream, n, p, g, m, v, sqnorm, max_norm,
                       nchunk, nseg, chunks, coefs, lr_bc1, b1, b2, eps, ibc2, skip, t, fraction);
}

}  // namespace repo

using namespace repo;

// a reduction workspace (include/repo_hip.h, "losses and regularisers"): its 256-byte header belongs to the single-launch
// reductions' ticket and stays untouched (zero) here -- this grid (up to 1024 blocks) keeps its follow-up launch
extern "C" size_t repo_grad_sqnorm_workspace_bytes(void) { return kRedHeaderBytes + 1024 * sizeof(float); }

extern "C" int repo_grad_sqnorm(int64_t n, const float* g, float* sqnorm, void* ws, size_t ws_bytes,
                                hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(n > 0, REPO_E_SHAPE);
  REPO_REQUIRE(g && sqnorm, REPO_E_BADARG);
  REPO_REQUIRE(((uintptr_t)g & 15) == 0, REPO_E_ALIGN);
  REPO_REQUIRE(ws && ws_bytes >= repo_grad_sqnorm_workspace_bytes(), REPO_E_WS_TOO_SMALL);
  long blocks = (n + 4095) / 4096;
  if (blocks > 1024) blocks = 1024;
  float* parts = (float*)((char*)ws + kRedHeaderBytes);
  hipLaunchKernelGGL(sqnorm_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, n, g, parts);
  REPO_CHECK_LAUNCH();
  hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, stream, (const float*)parts, (int)blocks, sqnorm);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_clip_adam(int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                              const float* sqnorm, float max_norm, float lr, float beta1, float beta2, float eps,
                              int64_t step, const unsigned* skip_if_nonzero, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(n > 0 && step >= 1, REPO_E_SHAPE);
  REPO_REQUIRE(params && grads && exp_avg && exp_avg_sq, REPO_E_BADARG);
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(clip_adam_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, n, params, grads, exp_avg,
                     exp_avg_sq, sqnorm, max_norm, (float)((double)lr / bc1), beta1, beta2, eps,
                     (float)(1.0 / sqrt(bc2)), skip_if_nonzero);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_clip_adam_target(int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                     const float* sqnorm, float max_norm, float lr, float beta1, float beta2, float eps,
                                     int64_t step, const unsigned* skip_if_nonzero, float* target, float fraction,
                                     hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(n > 0 && step >= 1, REPO_E_SHAPE);
  REPO_REQUIRE(params && grads && exp_avg && exp_avg_sq && target, REPO_E_BADARG);
  REPO_REQUIRE(fraction > 0.f && fraction <= 1.f, REPO_E_BADARG);   // (a NaN fails both comparisons)
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(clip_adam_target_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, n, params, grads, exp_avg,
                     exp_avg_sq, sqnorm, max_norm, (float)((double)lr / bc1), beta1, beta2, eps,
                     (float)(1.0 / sqrt(bc2)), skip_if_nonzero, target, fraction);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_agc_geometry(int* chunk, int* parts_max_blocks, int* finish_threads, int* step_max_blocks) {
  REPO_REQUIRE(chunk && parts_max_blocks && finish_threads && step_max_blocks, REPO_E_BADARG);
  *chunk = kAgcChunk;
  *parts_max_blocks = kAgcMaxBlocks;
  *finish_threads = kAgcFinishThreads;
  *step_max_blocks = kStepMaxBlocks;
  return REPO_OK;
}

extern "C" int repo_agc_coef(int64_t n, int64_t nseg, int64_t nchunk, const int* chunks, const int* seg_first,
                             const float* params, const float* grads, float clip, float pmin, float* parts, float* norms,
                             float* coef, float* stats, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(n > 0 && n <= kMaxIdx && nseg > 0 && nchunk >= nseg && nchunk <= n && nchunk <= kAgcMaxChunks, REPO_E_SHAPE);
  REPO_REQUIRE(chunks && seg_first && params && grads && parts && norms && coef && stats, REPO_E_BADARG);
  REPO_REQUIRE(std::isfinite(clip) && clip > 0.f && std::isfinite(pmin) && pmin > 0.f, REPO_E_BADARG);
  REPO_REQUIRE((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)chunks) & 15) == 0, REPO_E_ALIGN);
  const long blocks = nchunk < kAgcMaxBlocks ? (long)nchunk : kAgcMaxBlocks;
  hipLaunchKernelGGL(agc_parts_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (int)nchunk, (const int4*)chunks, n,
                     params, grads, parts);
  REPO_CHECK_LAUNCH();
  hipLaunchKernelGGL(agc_finish_kernel, dim3(1), dim3(kAgcFinishThreads), 0, stream, (int)nseg, (int)nchunk,
                     seg_first, (const float*)parts, clip, pmin, norms, coef, stats);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_optim_step(int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int rule,
                               int clip_mode, const float* sqnorm, float max_norm, int64_t nseg, int64_t nchunk, const int* chunks,
                               const float* coef, float lr, float beta1, float beta2, float eps, int64_t step,
                               const unsigned* skip_if_nonzero, float* target, float fraction, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(n > 0 && step >= 1, REPO_E_SHAPE);
  REPO_REQUIRE(params && grads && exp_avg && exp_avg_sq, REPO_E_BADARG);
  REPO_REQUIRE((rule == REPO_OPT_ADAM || rule == REPO_OPT_LAPROP) && clip_mode >= REPO_CLIP_NONE && clip_mode <= REPO_CLIP_TABLE,
               REPO_E_BADARG);
  REPO_REQUIRE(clip_mode != REPO_CLIP_GLOBAL || sqnorm, REPO_E_BADARG);
  if (clip_mode == REPO_CLIP_TABLE) {
    REPO_REQUIRE(n <= kMaxIdx && nseg > 0 && nchunk >= nseg && nchunk <= n && nchunk <= kAgcMaxChunks, REPO_E_SHAPE);
    REPO_REQUIRE(chunks && coef, REPO_E_BADARG);
    REPO_REQUIRE(((uintptr_t)chunks & 15) == 0, REPO_E_ALIGN);
  }
  REPO_REQUIRE(!target || (fraction > 0.f && fraction <= 1.f), REPO_E_BADARG);   // (a NaN fails both comparisons)
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  long blocks = clip_mode == REPO_CLIP_TABLE ? (long)nchunk : (long)((n + 255) / 256);
  if (blocks > kStepMaxBlocks) blocks = kStepMaxBlocks;
  const dim3 grid((unsigned)blocks);
  const float lr_bc1 = (float)((double)lr / bc1), ibc2 = (float)(1.0 / sqrt(bc2));
  const int4* ch = (const int4*)chunks;
#define REPO_STEP(R, C)                                                                                                  \
  launch_step<R, C>(target != nullptr, grid, stream, n, params, grads, exp_avg, exp_avg_sq, sqnorm, max_norm, (int)nchunk, \
                    (int)nseg, ch, coef, lr_bc1, beta1, beta2, eps, ibc2, skip_if_nonzero, target, fraction)
  if (rule == REPO_OPT_ADAM) {
    if (clip_mode == REPO_CLIP_NONE) REPO_STEP(0, 0);
    else if (clip_mode == REPO_CLIP_GLOBAL) REPO_STEP(0, 1);
    else REPO_STEP(0, 2);
  } else {
    if (clip_mode == REPO_CLIP_NONE) REPO_STEP(1, 0);
    else if (clip_mode == REPO_CLIP_GLOBAL) REPO_STEP(1, 1);
    else REPO_STEP(1, 2);
  }
#undef REPO_STEP
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}
