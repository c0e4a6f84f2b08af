// The VDB discriminator of CalibratedRePo (reference common/models/gans.py:56-156): everything behind its dense chain.
// The chain itself is repo_gemm (REPO_EPI_LEAKY / REPO_EPI_MUL_DLEAKY, dense_epi.h) and repo_gemm_wgrad; here are the
// reparameterised bottleneck head with the prior KL, the four losses, the head's reverse pass, the dual step on beta, and
// the head-side pieces of the zero-centred gradient penalty (include/repo_hip.h states each contract; DESIGN.md 6h derives
// the penalty's parameter gradient).  All of them are HBM / launch-latency bound passes over (N, 2Z) = 2500 x 128 floats.
// Reductions follow loss.hip: wave64 shuffles, one partial per workgroup, summed in a fixed order by the launch's last
// block (common.h, last_block_finishes) or, for the column sums, by a one-block follow-up launch -- no float atomics.
#include "common.h"

namespace repo {

__device__ __forceinline__ float leaky(float x) { return x > 0.f ? x : kLeakySlope * x; }
__device__ __forceinline__ float leaky_grad(float x) { return x > 0.f ? 1.f : kLeakySlope; }

// Rows are dealt to the 4 waves of a block (row = 4 * block + wave, stride 4 * grid), lanes run over the Z columns: both
// halves of a row of z are read as runs of consecutive floats.
__global__ __launch_bounds__(256) void vdb_head_fwd_kernel(int N, int Z, const float* __restrict__ z, long ldz, NoiseSrc eps,
                                                           const float* __restrict__ fc_w, const float* __restrict__ fc_b,
                                                           float* __restrict__ lat, float* __restrict__ d,
                                                           float* __restrict__ parts, float* __restrict__ kl_out,
                                                           unsigned* __restrict__ ticket) {
  __shared__ float red[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float kl = 0.f;
  for (long n = (long)blockIdx.x * 4 + wid; n < N; n += (long)gridDim.x * 4) {
    const float* zr = z + n * ldz;
    float dot = 0.f;
    for (int j = lane; j < Z; j += 64) {
      const float m = zr[j], ls = zr[Z + j], sd = expf(ls);
      const float l = m + eps.at((size_t)n * Z + j) * sd;
      lat[n * Z + j] = l;
      dot += fc_w[j] * leaky(l);
      kl += -ls + 0.5f * (sd * sd + m * m) - 0.5f;
    }
    dot = wave_sum(dot);
    if (lane == 0) d[n] = dot + fc_b[0];
  }
  if (!kl_out) return;   // (kernel argument: uniform)
  const float s = block_sum(kl, red);
  if (threadIdx.x == 0) parts[blockIdx.x] = s;
  last_block_finishes(parts, 1, kl_out, ticket, red);
}

__global__ __launch_bounds__(256) void vdb_loss_kernel(int N, const float* __restrict__ d, int mode,
                                                       const float* __restrict__ tau, float gscale, float* __restrict__ dd,
                                                       float* __restrict__ parts, float* __restrict__ out,
                                                       unsigned* __restrict__ ticket) {
  __shared__ float red[16];
  float acc = 0.f;
  for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
    const float x = d[n];
    float f, g;
    if (mode == REPO_VDB_BCE0 || mode == REPO_VDB_BCE1) {
      // torch's stable form: max(x, 0) - x t + log1p(exp(-|x|)); derivative sigmoid(x) - t
      const float t = mode == REPO_VDB_BCE1 ? 1.f : 0.f;
      f = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
      g = 1.f / (1.f + expf(-x)) - t;
    } else if (mode == REPO_VDB_NEG_TAU) {
      f = -tau[n] * x;
      g = -tau[n];
    } else {
      f = x + 0.25f * x * x;
      g = 1.f + 0.5f * x;
      if (mode == REPO_VDB_NEG_CHI) { f = -f; g = -g; }
    }
    acc += f;
    if (dd) dd[n] = g * gscale;
  }
  const float s = block_sum(acc, red);
  if (threadIdx.x == 0) parts[blockIdx.x] = s;
  last_block_finishes(parts, 1, out, ticket, red);
}

// The two column-sum passes.  Block b owns the rows [b * rpb, (b + 1) * rpb); for each 64-column slab its 4 waves walk those
// rows (stride 4), lane = column, and the block leaves ONE partial per column: parts[column][b] (row pitch = grid).
// GP = false (repo_vdb_head_bwd): up = dd (N), writes dz (N, 2Z); partials of dfc_w (Z) and dfc_b (column Z).
// GP = true  (repo_vdb_gp_head):  up = a5 (N, 2Z), writes extra (N, Z); partials of dfc_w (Z).
template <bool GP>
__global__ __launch_bounds__(256) void vdb_colsum_kernel(int N, int Z, int rpb, const float* __restrict__ z, long ldz,
                                                         NoiseSrc eps, const float* __restrict__ lat,
                                                         const float* __restrict__ fc_w, const float* __restrict__ up, long ldup,
                                                         const float* __restrict__ beta, float kl_coef,
                                                         const float* __restrict__ extra_in, float* __restrict__ out, long ldout,
                                                         float* __restrict__ parts) {
  __shared__ float sm[4][64];
  __shared__ float smb[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rpb, r1 = r0 + rpb < N ? r0 + rpb : N;
  const float c = (!GP && beta) ? *beta * kl_coef : 0.f;
  const int G = gridDim.x;
  for (int jb = 0; jb < Z; jb += 64) {
    const int j = jb + lane;
    float acc = 0.f, accb = 0.f;
    if (j < Z) {
      const float w = fc_w[j];
      for (long n = r0 + wid; n < r1; n += 4) {
        const float m = z[n * ldz + j], sd = expf(z[n * ldz + Z + j]);
        const float l = lat[n * Z + j], es = eps.at((size_t)n * Z + j) * sd, gl = leaky_grad(l);
        if constexpr (GP) {
          const float am = up[n * ldup + j], as = up[n * ldup + Z + j];
          acc += (am + as * es) * gl;
          out[n * ldout + j] = as * w * gl * es;
        } else {
          const float u = up[n], dl = u * w * gl;
          acc += u * leaky(l);
          if (j == 0) accb += u;
          out[n * ldout + j] = dl + c * m;
          out[n * ldout + Z + j] = dl * es + c * (sd * sd - 1.f) + (extra_in ? extra_in[n * Z + j] : 0.f);
        }
      }
    }
    if (!parts) continue;   // (kernel argument: uniform)
    sm[wid][lane] = acc;
    if (!GP && jb == 0 && lane == 0) smb[wid] = accb;
    __syncthreads();
    if (wid == 0 && j < Z) parts[(size_t)j * G + blockIdx.x] = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
    if (!GP && jb == 0 && threadIdx.x == 0) parts[(size_t)Z * G + blockIdx.x] = (smb[0] + smb[1]) + (smb[2] + smb[3]);
    __syncthreads();
  }
}

// out[v] (+)= parts[v][0] + parts[v][1] + ... in that order; v < nw goes to dw, v == nw (if db) to db[0]
__global__ __launch_bounds__(256) void vdb_colsum_finish_kernel(int nw, int G, const float* __restrict__ parts,
                                                                float* __restrict__ dw, float* __restrict__ db, int accumulate) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nw + (db ? 1 : 0)) return;
  float s = 0.f;
  for (int i = 0; i < G; ++i) s += parts[(size_t)v * G + i];
  float* o = v < nw ? dw + v : db;
  *o = accumulate ? *o + s : s;
}

__global__ void vdb_beta_step_kernel(float* __restrict__ beta, const float* __restrict__ klr, float inv_nr,
                                     const float* __restrict__ klf, float inv_nf, float beta_lr, float target_kl,
                                     float* __restrict__ kl_out) {
  if (threadIdx.x || blockIdx.x) return;
  const float kl = 0.5f * (*klr * inv_nr + *klf * inv_nf);
  if (kl_out) *kl_out = kl;
  *beta = fmaxf(*beta + beta_lr * (kl - target_kl), 0.f);
}

__global__ __launch_bounds__(256) void vdb_gp_delta_kernel(long total, int Z, const float* __restrict__ z, long ldz, NoiseSrc eps,
                                                           const float* __restrict__ lat, const float* __restrict__ fc_w,
                                                           float* __restrict__ delta, long ldd) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / Z;
    const int j = (int)(i - n * Z);
    const float r = fc_w[j] * leaky_grad(lat[i]);
    delta[n * ldd + j] = r;
    delta[n * ldd + Z + j] = r * eps.at((size_t)i) * expf(z[n * ldz + Z + j]);
  }
}

__global__ __launch_bounds__(256) void vdb_gp_norm_kernel(long n, float* __restrict__ g, float scale, float* __restrict__ parts,
                                                          float* __restrict__ out, unsigned* __restrict__ ticket) {
  __shared__ float red[16];
  float acc = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = g[i];
    acc += v * v;
    g[i] = v * scale;
  }
  const float s = block_sum(acc, red);
  if (threadIdx.x == 0) parts[blockIdx.x] = s;
  last_block_finishes(parts, 1, out, ticket, red);
}

__global__ __launch_bounds__(256) void vdb_tau_kernel(int N, const float* __restrict__ lt, const float* __restrict__ d,
                                                      const float* __restrict__ u, float* __restrict__ tau_out,
                                                      float* __restrict__ dlt, float* __restrict__ parts,
                                                      float* __restrict__ out, unsigned* __restrict__ ticket) {
  __shared__ float red[16];
  const float uv = u ? *u : 0.f, inv = 1.f / (float)N;
  float a0 = 0.f, a1 = 0.f;
  for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
    const float t = expf(lt[n]), dv = d ? d[n] : 0.f;
    a0 += t * dv;
    a1 += t - 1.f;
    if (tau_out) tau_out[n] = t;
    if (dlt) dlt[n] = t * (dv + uv) * inv;
  }
  const float s0 = block_sum(a0, red);
  const float s1 = block_sum(a1, red);
  if (threadIdx.x == 0) {
    parts[blockIdx.x] = s0;
    parts[gridDim.x + blockIdx.x] = s1;
  }
  last_block_finishes(parts, 2, out, ticket, red);
}

static inline int small_grid(long work, long per_block) {
  const int b = cdiv(work, per_block);
  return b > kLastBlockMaxGrid ? kLastBlockMaxGrid : (b < 1 ? 1 : b);
}
static inline bool red_ws_ok(const void* ws, size_t bytes) {
  return ws && bytes >= kRedHeaderBytes + 2 * kLastBlockMaxGrid * sizeof(float);
}
static inline bool head_shape_ok(int64_t N, int64_t Z, int64_t ld) {
  return N >= 1 && Z >= 1 && ld >= 2 * Z && N * ld < kMaxIdx;
}

// the two column-sum entry points
static int colsum_launch(bool gp, int64_t N, int64_t Z, const float* z, int64_t ldz, NoiseSrc eps, const float* lat,
                         const float* fc_w, const float* up, int64_t ldup, const float* beta, float kl_coef,
                         const float* extra_in, float* out, int64_t ldout, float* dw, float* db, int accumulate, void* ws,
                         size_t ws_bytes, hipStream_t stream) {
  const int G = small_grid(N, 32);
  const int rpb = cdiv(N, G);
  float* parts = dw ? (float*)ws : nullptr;
  if (dw) REPO_REQUIRE(ws && ws_bytes >= repo_vdb_colsum_workspace_bytes(Z), REPO_E_WS_TOO_SMALL);
  if (gp)
    hipLaunchKernelGGL(vdb_colsum_kernel<true>, dim3(G), dim3(256), 0, stream, (int)N, (int)Z, rpb, z, (long)ldz, eps, lat,
                       fc_w, up, (long)ldup, beta, kl_coef, extra_in, out, (long)ldout, parts);
  else
    hipLaunchKernelGGL(vdb_colsum_kernel<false>, dim3(G), dim3(256), 0, stream, (int)N, (int)Z, rpb, z, (long)ldz, eps, lat,
                       fc_w, up, (long)ldup, beta, kl_coef, extra_in, out, (long)ldout, parts);
  REPO_CHECK_LAUNCH();
  if (dw) {
    const int nv = (int)Z + (db ? 1 : 0);
    hipLaunchKernelGGL(vdb_colsum_finish_kernel, dim3(cdiv(nv, 256)), dim3(256), 0, stream, (int)Z, G, parts, dw, db,
                       accumulate);
    REPO_CHECK_LAUNCH();
  }
  return REPO_OK;
}

}  // namespace repo

using namespace repo;

extern "C" int repo_vdb_head_fwd(int64_t N, int64_t Z, const float* z, int64_t ldz, const float* eps, uint64_t noise_seed,
                                 uint64_t noise_offset, const float* fc_w, const float* fc_b, float* lat, float* d,
                                 float* kl_sum, void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(head_shape_ok(N, Z, ldz), REPO_E_SHAPE);
  REPO_REQUIRE(z && fc_w && fc_b && lat && d, REPO_E_BADARG);
  REPO_REQUIRE(!kl_sum || red_ws_ok(ws, ws_bytes), REPO_E_WS_TOO_SMALL);
  hipLaunchKernelGGL(vdb_head_fwd_kernel, dim3(small_grid(N, 4)), dim3(256), 0, stream, (int)N, (int)Z, z, (long)ldz,
                     NoiseSrc{eps, noise_seed, noise_offset}, fc_w, fc_b, lat, d,
                     kl_sum ? (float*)((char*)ws + kRedHeaderBytes) : nullptr, kl_sum, (unsigned*)ws);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_vdb_loss(int64_t N, const float* d, int mode, const float* tau, float gscale, float* dd, float* loss_sum,
                             void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(N >= 1 && N < kMaxIdx, REPO_E_SHAPE);
  REPO_REQUIRE(d && loss_sum && mode >= REPO_VDB_BCE0 && mode <= REPO_VDB_NEG_CHI && (mode != REPO_VDB_NEG_TAU || tau),
               REPO_E_BADARG);
  REPO_REQUIRE(red_ws_ok(ws, ws_bytes), REPO_E_WS_TOO_SMALL);
  hipLaunchKernelGGL(vdb_loss_kernel, dim3(small_grid(N, 256)), dim3(256), 0, stream, (int)N, d, mode, tau, gscale, dd,
                     (float*)((char*)ws + kRedHeaderBytes), loss_sum, (unsigned*)ws);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" size_t repo_vdb_colsum_workspace_bytes(int64_t Z) {
  return Z < 0 ? 0 : (size_t)(Z + 1) * kLastBlockMaxGrid * sizeof(float);
}

extern "C" int repo_vdb_head_bwd(int64_t N, int64_t Z, const float* z, int64_t ldz, const float* eps, uint64_t noise_seed,
                                 uint64_t noise_offset, const float* lat, const float* fc_w, const float* dd,
                                 const float* beta, float kl_coef, const float* extra, float* dz, int64_t lddz, float* dfc_w,
                                 float* dfc_b, int accumulate, void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(head_shape_ok(N, Z, ldz) && head_shape_ok(N, Z, lddz), REPO_E_SHAPE);
  REPO_REQUIRE(z && lat && fc_w && dd && dz && (!dfc_w == !dfc_b), REPO_E_BADARG);
  return colsum_launch(false, N, Z, z, ldz, NoiseSrc{eps, noise_seed, noise_offset}, lat, fc_w, dd, 0, beta, kl_coef, extra,
                       dz, lddz, dfc_w, dfc_b, accumulate, ws, ws_bytes, stream);
}

extern "C" int repo_vdb_beta_step(float* beta, const float* kl_real_sum, int64_t n_real, const float* kl_fake_sum,
                                  int64_t n_fake, float beta_lr, float target_kl, float* kl_out, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(n_real >= 1 && n_fake >= 1, REPO_E_SHAPE);
  REPO_REQUIRE(beta && kl_real_sum && kl_fake_sum, REPO_E_BADARG);
  hipLaunchKernelGGL(vdb_beta_step_kernel, dim3(1), dim3(64), 0, stream, beta, kl_real_sum, 1.f / (float)n_real,
                     kl_fake_sum, 1.f / (float)n_fake, beta_lr, target_kl, kl_out);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_vdb_gp_delta(int64_t N, int64_t Z, const float* z, int64_t ldz, const float* eps, uint64_t noise_seed,
                                 uint64_t noise_offset, const float* lat, const float* fc_w, float* delta5, int64_t lddelta,
                                 hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(head_shape_ok(N, Z, ldz) && head_shape_ok(N, Z, lddelta), REPO_E_SHAPE);
  REPO_REQUIRE(z && lat && fc_w && delta5, REPO_E_BADARG);
  const long total = (long)N * Z;
  const int blocks = cdiv(total, 256) > 2048 ? 2048 : cdiv(total, 256);
  hipLaunchKernelGGL(vdb_gp_delta_kernel, dim3(blocks), dim3(256), 0, stream, total, (int)Z, z, (long)ldz,
                     NoiseSrc{eps, noise_seed, noise_offset}, lat, fc_w, delta5, (long)lddelta);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_vdb_gp_norm(int64_t n, float* g, float scale, float* sq_sum, void* ws, size_t ws_bytes,
                                hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(n >= 1, REPO_E_SHAPE);
  REPO_REQUIRE(g && sq_sum, REPO_E_BADARG);
  REPO_REQUIRE(red_ws_ok(ws, ws_bytes), REPO_E_WS_TOO_SMALL);
  hipLaunchKernelGGL(vdb_gp_norm_kernel, dim3(small_grid(n, 4096)), dim3(256), 0, stream, (long)n, g, scale,
                     (float*)((char*)ws + kRedHeaderBytes), sq_sum, (unsigned*)ws);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_vdb_gp_head(int64_t N, int64_t Z, const float* a5, int64_t lda5, const float* z, int64_t ldz,
                                const float* eps, uint64_t noise_seed, uint64_t noise_offset, const float* lat,
                                const float* fc_w, float* extra, float* dfc_w, int accumulate, void* ws, size_t ws_bytes,
                                hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(head_shape_ok(N, Z, ldz) && head_shape_ok(N, Z, lda5), REPO_E_SHAPE);
  REPO_REQUIRE(a5 && z && lat && fc_w && extra && dfc_w, REPO_E_BADARG);
  return colsum_launch(true, N, Z, z, ldz, NoiseSrc{eps, noise_seed, noise_offset}, lat, fc_w, a5, lda5, nullptr, 0.f,
                       nullptr, extra, Z, dfc_w, nullptr, accumulate, ws, ws_bytes, stream);
}

extern "C" int repo_vdb_tau(int64_t N, const float* lt, const float* d, const float* u, float* tau_out, float* dlt,
                            float* sums, void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(N >= 1 && N < kMaxIdx, REPO_E_SHAPE);
  REPO_REQUIRE(lt && sums, REPO_E_BADARG);
  REPO_REQUIRE(red_ws_ok(ws, ws_bytes), REPO_E_WS_TOO_SMALL);
  hipLaunchKernelGGL(vdb_tau_kernel, dim3(small_grid(N, 256)), dim3(256), 0, stream, (int)N, lt, d, u, tau_out, dlt,
                     (float*)((char*)ws + kRedHeaderBytes), sums, (unsigned*)ws);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}
