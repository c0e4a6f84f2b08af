// RSSM observe scan: fused per-timestep GRU + prior/posterior cell, persistent over T.
//
// Reference: TransitionModel.observe / compute_belief / compute_prior_state /
// compute_posterior_state, /root/reference/algorithms/repo/models/rssm.py:34-64,76-146.
//
// Structure (MI355X-first, not a per-op translation):
//  * The posterior's observation half, embed_t @ W_bq[:, D:]^T, does not depend on the
//    recurrence and is hoisted out of the scan as ONE (T*B, E) x (E, Hd) MFMA GEMM.
//  * The scan itself is a latency-bound chain of T dependent steps on B rows.  One
//    persistent workgroup owns R batch rows for all T steps; the deterministic belief and
//    the stochastic state stay in LDS between steps, and each thread owns one output
//    feature of the current stage, so weights stream through coalesced, transposed copies
//    ([k][feature]) that stay L2-resident, with the row vectors broadcast from LDS.
//  * Everything the backward needs is written once per step; weight gradients are NOT
//    formed inside the scan: the reverse scan emits per-step pre-activation deltas and the
//    weight/bias gradients become seven (T*B)-row MFMA GEMMs afterwards.
#include "common.h"
#include "scan_cs.h"

namespace repo {

constexpr int kMaxW = 256;   // max belief / hidden width (one thread per feature)
constexpr int kMaxS2 = 128;  // max 2*state
constexpr int kMaxX = 64;    // max state + action

struct ObsDims {
  int T, B, A, D, Hd, S;
};

// dst[c][r] = src[r*ld + c]   (rows x cols -> cols x rows)
__global__ void transpose_kernel(const float* __restrict__ src, int rows, int cols, int ld, float* __restrict__ dst) {
  __shared__ float tile[32][33];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  for (int i = threadIdx.y; i < 32; i += blockDim.y) {
    const int r = r0 + i, c = c0 + threadIdx.x;
    tile[i][threadIdx.x] = (r < rows && c < cols) ? src[(size_t)r * ld + c] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += blockDim.y) {
    const int c = c0 + i, r = r0 + threadIdx.x;
    if (c < cols && r < rows) dst[(size_t)c * rows + r] = tile[threadIdx.x][i];
  }
}

static int transpose_to(const float* src, int rows, int cols, int ld, float* dst, hipStream_t s) {
  dim3 grid((cols + 31) / 32, (rows + 31) / 32), block(32, 8);
  hipLaunchKernelGGL(transpose_kernel, grid, block, 0, s, src, rows, cols, ld, dst);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? REPO_OK : (int)e;
}

// k4-interleaved weights for the scan's GEMV stages: dst[(kg*N + n)*4 + u] = W(n, k = 4kg + u), 0 for k >= K,
// with W(n, k) = src[n*sn + k*sk].  Thread n of a stage then reads FOUR consecutive k of its output with one
// coalesced 16-byte load (1 KB per wave) instead of four dword loads: the scan was bound by the CU's
// vector-memory issue rate (~5.5k wave-level dword loads per step, ~12 cycles each), not by L2 latency.
struct K4Job {
  const float* src;
  float* dst;
  int N, K, sn, sk;
};
constexpr int kMaxK4Jobs = 8;
struct K4Jobs {
  K4Job job[kMaxK4Jobs];
  int n;
};
// one launch for all the matrices of a scan: blockIdx.y = job
__global__ void pack_k4_kernel(K4Jobs js) {
  const K4Job j = js.job[blockIdx.y];
  const int total = ((j.K + 3) >> 2) * 4 * j.N;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int u = i & 3, q = i >> 2;
    const int n = q % j.N, kg = q / j.N;
    const int k = 4 * kg + u;
    j.dst[i] = k < j.K ? j.src[(size_t)n * j.sn + (size_t)k * j.sk] : 0.f;
  }
}

static size_t packed_k4_floats(int64_t N, int64_t K) { return (size_t)((K + 3) / 4) * 4 * N; }

// queue a pack; returns where the next pack may start
static float* pack_k4_add(K4Jobs& js, const float* src, int N, int K, int sn, int sk, float* dst) {
  js.job[js.n++] = K4Job{src, dst, N, K, sn, sk};
  return dst + packed_k4_floats(N, K);
}
static int pack_k4_launch(const K4Jobs& js, hipStream_t s) {
  int mx = 1;
  for (int i = 0; i < js.n; ++i) {
    const int blocks = (int)((packed_k4_floats(js.job[i].N, js.job[i].K) + 255) / 256);
    if (blocks > mx) mx = blocks;
  }
  if (mx > 512) mx = 512;
  hipLaunchKernelGGL(pack_k4_kernel, dim3(mx, js.n), dim3(256), 0, s, js);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? REPO_OK : (int)e;
}

__device__ __forceinline__ float fma4(const float4 w, const float* __restrict__ x, float acc) {
  const float4 v = *reinterpret_cast<const float4*>(x);  // same address in every lane: LDS broadcast
  acc = fmaf(w.x, v.x, acc);
  acc = fmaf(w.y, v.y, acc);
  acc = fmaf(w.z, v.z, acc);
  return fmaf(w.w, v.w, acc);
}

struct ObsFwdArgs {
  ObsDims d;
  // k4-interleaved weights (pack_k4_kernel) and biases
  const float *WsaT, *bsa, *WihT, *WhhT, *bih, *bhh, *WbpT, *bbp, *WspT, *bsp, *WbqT, *bbq, *WsqT, *bsq;
  const float *prev_belief, *prev_state;  // (B,D), (B,S)
  const float *actions, *nonterms;        // (T,B,A), (T,B)
  const float* eemb;                      // (T,B,Hd) hoisted embed contribution (no bias)
  NoiseSrc eps_prior, eps_post;           // (T,B,S)
  float* featx;                           // (T+1,B,D+S): slot 0 = [prev_belief|prev_state], slot t+1 = [belief_t|post_t]
  float *prior_state, *prior_mean, *prior_std, *post_mean, *post_std;  // (T,B,S)
  float *xsa, *e, *gates, *hp, *hq;       // saved for backward: (T,B,S+A) (T,B,D) (T,B,4D) (T,B,Hd) (T,B,Hd)
  float min_std;
  int prior_only;  // the NEXT step is fed the prior sample (observe without observations, rssm.py:118)
  int skip_prior;  // the prior head is not evaluated here (repo_rssm_prior_head does it for all steps at once)
};

struct ObsBwdArgs {
  ObsDims d;
  // k4-interleaved weights (pack_k4_kernel) with the reduction over the layer's OUTPUT index:
  // W(n = input index, k = output index) = native[k*ld + n]
  const float *Wsa, *Wih, *Whh, *Wbp, *Wsp, *Wbq, *Wsq;
  // saved by forward
  const float *featx, *nonterms, *e, *gates, *hp, *hq, *prior_std, *post_std;
  NoiseSrc eps_prior, eps_post;
  // upstream gradients, each nullable: d featx[1:] (T,B,D+S); prior_state, and the four (mean,std) (T,B,S)
  const float *dfeat, *dprior_state, *dpm, *dps, *dqm, *dqs;
  // per-step deltas (outputs)
  float *doutp, *doutq;  // (T,B,2S)
  float *dhp, *dhq;      // (T,B,Hd)   d pre-activation of the hidden layers
  float *dgi, *dgh;      // (T,B,3D)
  float* de;             // (T,B,D)    d pre-activation of fc_embed_state_action
  float *dprev_belief, *dprev_state;  // (B,D) (B,S), nullable
  float min_std;
};

// the scan kernels, one copy per dense activation (rssm_scan.h)
#define REPO_SCAN_ACT REPO_ACT_ELU
#define REPO_SCAN_FWD_KERNEL observe_fwd_kernel
#define REPO_SCAN_BWD_KERNEL observe_bwd_kernel
#include "rssm_scan.h"
#undef REPO_SCAN_ACT
#undef REPO_SCAN_FWD_KERNEL
#undef REPO_SCAN_BWD_KERNEL
#define REPO_SCAN_ACT REPO_ACT_RELU
#define REPO_SCAN_FWD_KERNEL observe_fwd_relu_kernel
#define REPO_SCAN_BWD_KERNEL observe_bwd_relu_kernel
#include "rssm_scan.h"
#undef REPO_SCAN_ACT
#undef REPO_SCAN_FWD_KERNEL
#undef REPO_SCAN_BWD_KERNEL

static bool dims_ok(int64_t T, int64_t B, int64_t A, int64_t D, int64_t Hd, int64_t S) {
  return T >= 0 && B > 0 && A >= 0 && D > 0 && Hd > 0 && S > 0 && D <= kMaxW && Hd <= kMaxW && 2 * S <= kMaxS2 &&
         4 * S <= 256 && S + A <= kMaxX && T * B * 4 * D < kMaxIdx;
}

static size_t bwd_pack_floats(int64_t A, int64_t D, int64_t Hd, int64_t S) {
  (void)A;
  return 2 * packed_k4_floats(Hd, 2 * S) + 2 * packed_k4_floats(D, Hd) + 2 * packed_k4_floats(D, 3 * D) +
         packed_k4_floats(S, D);
}

static size_t fwd_ws_floats(int64_t A, int64_t D, int64_t Hd, int64_t S) {
  return packed_k4_floats(D, S + A) + 2 * packed_k4_floats(3 * D, D) + 2 * packed_k4_floats(Hd, D) +
         2 * packed_k4_floats(2 * S, Hd);
}

}  // namespace repo

using namespace repo;

extern "C" size_t repo_rssm_observe_fwd_workspace_bytes(int64_t T, int64_t B, int64_t A, int64_t D, int64_t Hd,
                                                        int64_t S, int64_t E) {
  (void)E;
  size_t f = fwd_ws_floats(A, D, Hd, S);
  if (scan_cs_ok(T, B, A, D, Hd, S)) f = std::max(f, scan_cs_fwd_ws_floats(B, A, D, Hd, S));  // prior_only = 3
  return f * sizeof(float);
}

extern "C" int repo_rssm_observe_fwd_act(int64_t T, int64_t B, int64_t A, int64_t D, int64_t Hd, int64_t S, int64_t E,
                                     const float* const* params, const float* prev_belief, const float* prev_state,
                                     const float* actions, const float* nonterms, const float* embeds,
                                     const float* eps_prior, const float* eps_post, uint64_t noise_seed,
                                     uint64_t noise_offset, float min_std, float* featx,
                                     float* prior_state, float* prior_mean, float* prior_std, float* post_mean,
                                     float* post_std, float* xsa, float* e, float* gates, float* hp, float* hq,
                                     float* eemb, int prior_only, unsigned* status, void* ws, size_t ws_bytes,
                                     hipStream_t stream, int act) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(act_ok(act), REPO_E_BADARG);
  REPO_REQUIRE(dims_ok(T, B, A, D, Hd, S) && E > 0, REPO_E_SHAPE);
  REPO_REQUIRE(params && prev_belief && prev_state && actions && nonterms && embeds && !eps_prior == !eps_post,
               REPO_E_BADARG);
  REPO_REQUIRE(featx && prior_state && prior_mean && prior_std && post_mean && post_std && xsa && e && gates && hp &&
                   hq && eemb,
               REPO_E_BADARG);
  REPO_REQUIRE(ws && ws_bytes >= fwd_ws_floats(A, D, Hd, S) * sizeof(float), REPO_E_WS_TOO_SMALL);
  const float* const* P = params;
  if (prior_only == 3) {
    // the column-split, weight-stationary engine (scan_cs.hip): prior head left out as with prior_only = 2
    REPO_REQUIRE(scan_cs_ok(T, B, A, D, Hd, S), REPO_E_SHAPE);
    if (T == 0) return REPO_OK;
    int rc3 = repo_gemm(0, 1, T * B, Hd, E, embeds, E, P[10] + D, D + E, nullptr, 1, eemb, Hd, REPO_EPI_NONE, nullptr,
                        0, 0, stream);
    if (rc3) return rc3;
    ScanCsFwd q{T, B, A, D, Hd, S, E, params, prev_belief, prev_state, actions, nonterms, eemb,
                NoiseSrc{eps_post, noise_seed, noise_offset + (uint64_t)(T * B * S)}, min_std,
                featx, post_mean, post_std, xsa, e, gates, hq, status, act};
    return scan_cs_fwd(q, ws, ws_bytes, stream);
  }
  float* w = (float*)ws;
  // W(n, k) = P[n*ld + k] (native (out, in) layout) -> k4-interleaved [k/4][n][4]
  const int X = (int)(S + A), d = (int)D, h = (int)Hd, s2 = (int)(2 * S);
  float* WsaT = w;  w += packed_k4_floats(d, X);
  float* WihT = w;  w += packed_k4_floats(3 * d, d);
  float* WhhT = w;  w += packed_k4_floats(3 * d, d);
  float* WbpT = w;  w += packed_k4_floats(h, d);
  float* WbqT = w;  w += packed_k4_floats(h, d);
  float* WspT = w;  w += packed_k4_floats(s2, h);
  float* WsqT = w;
  int rc;
  K4Jobs packs;
  packs.n = 0;
  pack_k4_add(packs, P[0], d, X, X, 1, WsaT);
  pack_k4_add(packs, P[2], 3 * d, d, d, 1, WihT);
  pack_k4_add(packs, P[3], 3 * d, d, d, 1, WhhT);
  pack_k4_add(packs, P[6], h, d, d, 1, WbpT);
  pack_k4_add(packs, P[10], h, d, (int)(D + E), 1, WbqT);
  pack_k4_add(packs, P[8], s2, h, h, 1, WspT);
  pack_k4_add(packs, P[12], s2, h, h, 1, WsqT);
  if ((rc = pack_k4_launch(packs, stream))) return rc;
  if (T == 0) return REPO_OK;
  // hoisted: eemb = embeds @ W_bq[:, D:]^T
  if ((rc = repo_gemm(0, 1, T * B, Hd, E, embeds, E, P[10] + D, D + E, nullptr, 1, eemb, Hd, REPO_EPI_NONE, nullptr, 0,
                      0, stream)))
    return rc;
  ObsFwdArgs a;
  a.d = ObsDims{(int)T, (int)B, (int)A, (int)D, (int)Hd, (int)S};
  a.WsaT = WsaT; a.bsa = P[1]; a.WihT = WihT; a.WhhT = WhhT; a.bih = P[4]; a.bhh = P[5];
  a.WbpT = WbpT; a.bbp = P[7]; a.WspT = WspT; a.bsp = P[9]; a.WbqT = WbqT; a.bbq = P[11]; a.WsqT = WsqT; a.bsq = P[13];
  a.prev_belief = prev_belief; a.prev_state = prev_state; a.actions = actions; a.nonterms = nonterms;
  a.eemb = eemb;
  a.prior_only = prior_only == 1;
  a.skip_prior = prior_only == 2;
  a.eps_prior = NoiseSrc{eps_prior, noise_seed, noise_offset};
  a.eps_post = NoiseSrc{eps_post, noise_seed, noise_offset + (uint64_t)(T * B * S)};
  a.featx = featx; a.prior_state = prior_state; a.prior_mean = prior_mean; a.prior_std = prior_std;
  a.post_mean = post_mean; a.post_std = post_std; a.xsa = xsa; a.e = e; a.gates = gates; a.hp = hp; a.hq = hq;
  a.min_std = min_std;
  // rows per workgroup: spread B over as many CUs as possible (the scan is latency-bound)
  auto go = [&](auto elu_k, auto relu_k, dim3 grid, dim3 block) {   // the instantiation of `act`
    hipLaunchKernelGGL(act == REPO_ACT_RELU ? relu_k : elu_k, grid, block, 0, stream, a);
  };
  if (B >= 512) {
    go(observe_fwd_kernel<4, 1>, observe_fwd_relu_kernel<4, 1>, dim3(cdiv(B, 4)), dim3(256));
  } else if (B >= 128) {
    go(observe_fwd_kernel<2, 2>, observe_fwd_relu_kernel<2, 2>, dim3(cdiv(B, 2)), dim3(512));
  } else if (B >= 32) {
    // two rows per workgroup: every streamed weight feeds two FMAs, which halves the scan's L2 traffic.
    // Alone the scan is no faster, but beside the convolution kernels it (and they) lose less to L2
    // contention: 11.1 -> 10.7 ms per pipelined update at B=50 (3 or 4 rows per workgroup: slower)
    go(observe_fwd_kernel<2, 4>, observe_fwd_relu_kernel<2, 4>, dim3(cdiv(B, 2)), dim3(1024));
  } else {
    go(observe_fwd_kernel<1, 4>, observe_fwd_relu_kernel<1, 4>, dim3((unsigned)B), dim3(1024));
  }
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

// ---- the prior head of all T steps at once (repo_rssm_observe_fwd with prior_only = 2 leaves it out of the scan)
__global__ void prior_sample_kernel(int n, int S, const float* __restrict__ outp, NoiseSrc eps, float min_std,
                                    float* __restrict__ mean_o, float* __restrict__ std_o, float* __restrict__ state_o) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int row = i / S, s = i % S;
    const float mean = outp[(size_t)row * 2 * S + s];
    const float sd = softplus(outp[(size_t)row * 2 * S + S + s]) + min_std;
    mean_o[i] = mean;
    std_o[i] = sd;
    state_o[i] = fmaf(sd, eps.at(i), mean);
  }
}

extern "C" size_t repo_rssm_prior_head_workspace_bytes(int64_t T, int64_t B, int64_t S) {
  return (size_t)(T * B * 2 * S) * sizeof(float);
}

extern "C" int repo_rssm_prior_head_act(int64_t T, int64_t B, int64_t D, int64_t Hd, int64_t S, const float* const* params,
                                    const float* featx, const float* eps_prior, uint64_t noise_seed,
                                    uint64_t noise_offset, float min_std, float* hp, float* prior_state,
                                    float* prior_mean, float* prior_std, void* ws, size_t ws_bytes,
                                    hipStream_t stream, int act) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(act_ok(act), REPO_E_BADARG);
  REPO_REQUIRE(T >= 0 && B > 0 && D > 0 && Hd > 0 && S > 0 && T * B * (int64_t)(D + S) < kMaxBufElems, REPO_E_SHAPE);
  REPO_REQUIRE(params && featx && hp && prior_state && prior_mean && prior_std, REPO_E_BADARG);
  if (T == 0) return REPO_OK;
  REPO_REQUIRE(ws && ws_bytes >= repo_rssm_prior_head_workspace_bytes(T, B, S), REPO_E_WS_TOO_SMALL);
  const int64_t rows = T * B, F = D + S;
  const float* bel = featx + (size_t)B * F;  // belief_t = featx[t + 1][:, :D]
  float* outp = (float*)ws;
  int rc;
  // hp = act(belief @ W_bp^T + b);  out = hp @ W_sp^T + b   (fc_embed_belief_prior, fc_state_prior: rssm.py:42-50)
  if ((rc = repo_gemm(0, 1, rows, Hd, D, bel, F, params[6], D, params[7], 1, hp, Hd, act_epi(act), nullptr, 0, 0, stream)))
    return rc;
  if ((rc = repo_gemm(0, 1, rows, 2 * S, Hd, hp, Hd, params[8], Hd, params[9], 1, outp, 2 * S, REPO_EPI_NONE, nullptr,
                      0, 0, stream)))
    return rc;
  const int n = (int)(rows * S);
  hipLaunchKernelGGL(prior_sample_kernel, dim3(cdiv(n, 256) < 1024 ? cdiv(n, 256) : 1024), dim3(256), 0, stream, n, (int)S,
                     (const float*)outp, NoiseSrc{eps_prior, noise_seed, noise_offset}, min_std, prior_mean, prior_std,
                     prior_state);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

// The deferred weight / bias gradients of the scan as (T*B)-row GEMM jobs (G = dparams in plist order).
static void obs_wgrad_jobs(WgradDesc* j, int64_t R_, int64_t B, int64_t A, int64_t D, int64_t Hd, int64_t S, int64_t E,
                           const float* featx, const float* xsa, const float* e, const float* hp, const float* hq,
                           const float* doutp, const float* doutq, const float* dhp, const float* dhq,
                           const float* dgi, const float* dgh, const float* de, float* const* G) {
  const int64_t F = D + S, X = S + A;
  auto g = [&](int i) -> float* { return G ? G[i] : nullptr; };
  const float* bel = featx ? featx + (size_t)B * F : nullptr;  // belief_t = featx[t+1][:, :D]
  // fc_state_prior / fc_state_posterior
  j[0] = WgradDesc{R_, 2 * S, Hd, doutp, 2 * S, hp, Hd, g(8), Hd, g(9)};
  j[1] = WgradDesc{R_, 2 * S, Hd, doutq, 2 * S, hq, Hd, g(12), Hd, g(13)};
  // fc_embed_belief_prior; fc_embed_belief_posterior's belief columns [0, D) of its (Hd, D + E) weight
  j[2] = WgradDesc{R_, Hd, D, dhp, Hd, bel, F, g(6), D, g(7)};
  j[3] = WgradDesc{R_, Hd, D, dhq, Hd, bel, F, g(10), D + E, g(11)};
  // GRU: weight_ih sees e, weight_hh sees belief_{t-1} = featx[t][:, :D]
  j[4] = WgradDesc{R_, 3 * D, D, dgi, 3 * D, e, D, g(2), D, g(4)};
  j[5] = WgradDesc{R_, 3 * D, D, dgh, 3 * D, featx, F, g(3), D, g(5)};
  // fc_embed_state_action
  j[6] = WgradDesc{R_, D, X, de, D, xsa, X, g(0), X, g(1)};
}

// output deltas of the PRIOR head for all steps (they depend on upstream gradients only, not on the recurrence)
__global__ void prior_delta_kernel(int n, int S, const float* __restrict__ dstate, const float* __restrict__ dpm,
                                   const float* __restrict__ dps, const float* __restrict__ prior_std, NoiseSrc eps,
                                   float min_std, float* __restrict__ doutp) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int row = i / S, s = i % S;
    const float dsmp = dstate ? dstate[i] : 0.f;
    const float dm = (dpm ? dpm[i] : 0.f) + dsmp;
    const float dsd = fmaf(dsmp, eps.at(i), dps ? dps[i] : 0.f);
    doutp[(size_t)row * 2 * S + s] = dm;
    doutp[(size_t)row * 2 * S + S + s] = dsd * (-expm1f(-(prior_std[i] - min_std)));
  }
}

// want_wgrad = false (repo_rssm_observe_bwd_frozen): the deltas, and a slab that holds the scan's own packs only
static size_t obs_bwd_ws_bytes(int64_t T, int64_t B, int64_t A, int64_t D, int64_t Hd, int64_t S, int64_t E,
                               bool want_wgrad) {
  // deltas + the largest wgrad slab
  const size_t rows = (size_t)T * B;
  size_t deltas = rows * (size_t)(4 * S + 2 * Hd + 6 * D + D);
  size_t slab = 0;
  if (want_wgrad) {
    // the seven recurrent-path weight gradients share one launch pair (one slab each); the (Hd x E) one runs alone
    WgradDesc jobs[7];
    obs_wgrad_jobs(jobs, T * B, B, A, D, Hd, S, E, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                   nullptr, nullptr, nullptr, nullptr, nullptr);
    slab = gemm_wgrad_group_ws_bytes(jobs, 7);
    const size_t big = repo_gemm_wgrad_workspace_bytes(T * B, Hd, E);
    if (big > slab) slab = big;
  }
  const size_t packs = bwd_pack_floats(A, D, Hd, S) * sizeof(float);  // live only during the scan kernel
  if (packs > slab) slab = packs;
  if (scan_cs_ok(T, B, A, D, Hd, S)) {  // column-split engine: its packs and exchange buffers + the prior head's d belief
    const size_t cs = (scan_cs_bwd_ws_floats(B, A, D, Hd, S) + rows * (size_t)D) * sizeof(float) + 256;
    if (cs > slab) slab = cs;
  }
  return deltas * sizeof(float) + slab + 256;
}

extern "C" size_t repo_rssm_observe_bwd_workspace_bytes(int64_t T, int64_t B, int64_t A, int64_t D, int64_t Hd,
                                                        int64_t S, int64_t E) {
  return obs_bwd_ws_bytes(T, B, A, D, Hd, S, E, true);
}

extern "C" size_t repo_rssm_observe_bwd_frozen_workspace_bytes(int64_t T, int64_t B, int64_t A, int64_t D, int64_t Hd,
                                                               int64_t S, int64_t E) {
  return obs_bwd_ws_bytes(T, B, A, D, Hd, S, E, false);
}

// The reverse scan behind repo_rssm_observe_bwd_act (want_wgrad: the eight deferred weight-gradient products follow the
// scan, dparams required) and repo_rssm_observe_bwd_frozen (the scan and d embeds only: dparams is not read).
static int obs_bwd_run(int64_t T, int64_t B, int64_t A, int64_t D, int64_t Hd, int64_t S, int64_t E,
                       const float* const* params, const float* nonterms, const float* embeds,
                       const float* eps_prior, const float* eps_post, uint64_t noise_seed,
                       uint64_t noise_offset, float min_std, const float* featx,
                       const float* prior_std, const float* post_std, const float* xsa, const float* e,
                       const float* gates, const float* hp, const float* hq, const float* dfeat,
                       const float* dprior_state, const float* dpm, const float* dps, const float* dqm,
                       const float* dqs, float* const* dparams, float* dembeds, float* dprev_belief,
                       float* dprev_state, int accumulate, unsigned* status, void* ws,
                       size_t ws_bytes, hipStream_t stream, int act, bool want_wgrad) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(act_ok(act), REPO_E_BADARG);
  REPO_REQUIRE(dims_ok(T, B, A, D, Hd, S) && E > 0 && T > 0, REPO_E_SHAPE);
  REPO_REQUIRE(params && nonterms && embeds && !eps_prior == !eps_post && featx && prior_std && post_std && xsa && e &&
                   gates && hp && hq && (dparams || !want_wgrad),
               REPO_E_BADARG);
  REPO_REQUIRE(ws && ws_bytes >= obs_bwd_ws_bytes(T, B, A, D, Hd, S, E, want_wgrad), REPO_E_WS_TOO_SMALL);
  const size_t rows = (size_t)T * B;
  float* w = (float*)ws;
  float* doutp = w;  w += rows * 2 * S;
  float* doutq = w;  w += rows * 2 * S;
  float* dhp = w;    w += rows * Hd;
  float* dhq = w;    w += rows * Hd;
  float* dgi = w;    w += rows * 3 * D;
  float* dgh = w;    w += rows * 3 * D;
  float* de = w;     w += rows * D;
  // align the slab region to 256 B
  uintptr_t sl = ((uintptr_t)w + 255) & ~(uintptr_t)255;
  void* slab = (void*)sl;
  const size_t slab_bytes = ws_bytes - (sl - (uintptr_t)ws);

  const float* const* P = params;
  const bool cs_engine = (accumulate & 2) != 0;
  accumulate &= 1;
  if (cs_engine) {
    // column-split, weight-stationary reverse scan (scan_cs.hip).  The prior head is off the recurrence: its output
    // deltas, its hidden delta and its share of d belief_t are three launches over all T*B rows, in front of the scan
    REPO_REQUIRE(scan_cs_ok(T, B, A, D, Hd, S), REPO_E_SHAPE);
    // no upstream on the prior head and nobody to read its deltas: the three launches would hand the scan zeros
    const bool prior_dead = !want_wgrad && !dprior_state && !dpm && !dps;
    int rc1 = REPO_OK;
    float* dbx = nullptr;
    void* cws = slab;
    if (!prior_dead) {
      const int n = (int)(rows * S);
      hipLaunchKernelGGL(prior_delta_kernel, dim3(cdiv(n, 256) > 1024 ? 1024 : cdiv(n, 256)), dim3(256), 0, stream, n, (int)S,
                         dprior_state, dpm, dps, prior_std, NoiseSrc{eps_prior, noise_seed, noise_offset}, min_std, doutp);
      REPO_CHECK_LAUNCH();
      rc1 = repo_gemm(0, 0, (int64_t)rows, Hd, 2 * S, doutp, 2 * S, P[8], Hd, nullptr, 1, dhp, Hd, act_epi_mul_d(act), hp,
                      Hd, 0, stream);
      if (rc1) return rc1;
      dbx = (float*)slab;
      if ((rc1 = repo_gemm(0, 0, (int64_t)rows, D, Hd, dhp, Hd, P[6], D, nullptr, 1, dbx, D, REPO_EPI_NONE, nullptr, 0, 0,
                           stream)))
        return rc1;
      cws = (void*)(((uintptr_t)(dbx + rows * D) + 255) & ~(uintptr_t)255);
    }
    ScanCsBwd q{T, B, A, D, Hd, S, E, params, nonterms,
                NoiseSrc{eps_post, noise_seed, noise_offset + (uint64_t)(T * B * S)}, min_std,
                featx, post_std, e, gates, hq, dfeat, dqm, dqs, dbx, doutq, dhq, dgi, dgh, de, dprev_belief, dprev_state, status, act};
    if ((rc1 = scan_cs_bwd(q, cws, slab_bytes - ((uintptr_t)cws - (uintptr_t)slab), stream))) return rc1;
  } else {
  ObsBwdArgs a;
  a.d = ObsDims{(int)T, (int)B, (int)A, (int)D, (int)Hd, (int)S};
  {  // packed weights at the head of the slab region: dead before the first weight-gradient GEMM uses it
    float* pw = (float*)slab;
    const int d = (int)D, h = (int)Hd, s2 = (int)(2 * S), X_ = (int)(S + A);
    K4Jobs packs;
    packs.n = 0;
    auto put = [&](const float* src, int N, int K, int ld, const float** dstp) {
      *dstp = pw;
      pw = pack_k4_add(packs, src, N, K, 1, ld, pw);
    };
    put(P[8], h, s2, h, &a.Wsp);
    put(P[12], h, s2, h, &a.Wsq);
    put(P[6], d, h, d, &a.Wbp);
    put(P[10], d, h, (int)(D + E), &a.Wbq);
    put(P[3], d, 3 * d, d, &a.Whh);
    put(P[2], d, 3 * d, d, &a.Wih);
    put(P[0], (int)S, d, X_, &a.Wsa);
    const int rc0 = pack_k4_launch(packs, stream);
    if (rc0) return rc0;
  }
  a.featx = featx; a.nonterms = nonterms; a.e = e; a.gates = gates; a.hp = hp; a.hq = hq;
  a.prior_std = prior_std; a.post_std = post_std;
  a.eps_prior = NoiseSrc{eps_prior, noise_seed, noise_offset};
  a.eps_post = NoiseSrc{eps_post, noise_seed, noise_offset + (uint64_t)(T * B * S)};
  a.dfeat = dfeat; a.dprior_state = dprior_state; a.dpm = dpm; a.dps = dps; a.dqm = dqm; a.dqs = dqs;
  a.doutp = doutp; a.doutq = doutq; a.dhp = dhp; a.dhq = dhq; a.dgi = dgi; a.dgh = dgh; a.de = de;
  a.dprev_belief = dprev_belief; a.dprev_state = dprev_state; a.min_std = min_std;
  // the output-delta role takes one thread per (row, 2S column): R * 2S <= blockDim.  Four rows on 256 threads hold
  // S <= 32 only; wider states (up to 64) take two rows on 512
  auto go = [&](auto elu_k, auto relu_k, dim3 grid, dim3 block) {   // the instantiation of `act`
    hipLaunchKernelGGL(act == REPO_ACT_RELU ? relu_k : elu_k, grid, block, 0, stream, a);
  };
  if (B >= 512 && 4 * 2 * S <= 256) {
    go(observe_bwd_kernel<4, 1>, observe_bwd_relu_kernel<4, 1>, dim3(cdiv(B, 4)), dim3(256));
  } else if (B >= 128) {
    go(observe_bwd_kernel<2, 2>, observe_bwd_relu_kernel<2, 2>, dim3(cdiv(B, 2)), dim3(512));
  } else if (B >= 32) {
    go(observe_bwd_kernel<2, 4>, observe_bwd_relu_kernel<2, 4>, dim3(cdiv(B, 2)), dim3(1024));
  } else {
    go(observe_bwd_kernel<1, 4>, observe_bwd_relu_kernel<1, 4>, dim3((unsigned)B), dim3(1024));
  }
  REPO_CHECK_LAUNCH();

  }
  const int64_t R_ = (int64_t)rows;
  int rc;
  if (want_wgrad) {
    // deferred weight/bias gradients: (T*B)-row MFMA GEMMs
    float* const* G = dparams;
    WgradDesc jobs[7];
    obs_wgrad_jobs(jobs, R_, B, A, D, Hd, S, E, featx, xsa, e, hp, hq, doutp, doutq, dhp, dhq, dgi, dgh, de, G);
    if ((rc = gemm_wgrad_group(jobs, 7, accumulate, slab, slab_bytes, stream))) return rc;
    // fc_embed_belief_posterior, columns [D, D+E): the embedding's share
    if ((rc = repo_gemm_wgrad(R_, Hd, E, dhq, Hd, embeds, E, G[10] + D, D + E, nullptr, accumulate, slab, slab_bytes, stream))) return rc;
  }
  // gradient into the encoder embedding: d embeds = dhq @ W_bq[:, D:]
  if (dembeds)
    if ((rc = repo_gemm(0, 0, R_, E, Hd, dhq, Hd, P[10] + D, D + E, nullptr, 1, dembeds, E, REPO_EPI_NONE, nullptr, 0, 0, stream))) return rc;
  return REPO_OK;
}

extern "C" int repo_rssm_observe_bwd_act(int64_t T, int64_t B, int64_t A, int64_t D, int64_t Hd, int64_t S, int64_t E,
                                         const float* const* params, const float* nonterms, const float* embeds,
                                         const float* eps_prior, const float* eps_post, uint64_t noise_seed,
                                         uint64_t noise_offset, float min_std, const float* featx,
                                         const float* prior_std, const float* post_std, const float* xsa, const float* e,
                                         const float* gates, const float* hp, const float* hq, const float* dfeat,
                                         const float* dprior_state, const float* dpm, const float* dps, const float* dqm,
                                         const float* dqs, float* const* dparams, float* dembeds, float* dprev_belief,
                                         float* dprev_state, int accumulate, unsigned* status, void* ws,
                                         size_t ws_bytes, hipStream_t stream, int act) {
  return obs_bwd_run(T, B, A, D, Hd, S, E, params, nonterms, embeds, eps_prior, eps_post, noise_seed, noise_offset,
                     min_std, featx, prior_std, post_std, xsa, e, gates, hp, hq, dfeat, dprior_state, dpm, dps, dqm, dqs,
                     dparams, dembeds, dprev_belief, dprev_state, accumulate, status, ws, ws_bytes, stream, act, true);
}

// ABI v13: the same reverse scan for FROZEN weights -- no weight-gradient product, no slab for one
extern "C" int repo_rssm_observe_bwd_frozen(int64_t T, int64_t B, int64_t A, int64_t D, int64_t Hd, int64_t S, int64_t E,
                                            const float* const* params, const float* nonterms, const float* embeds,
                                            const float* eps_prior, const float* eps_post, uint64_t noise_seed,
                                            uint64_t noise_offset, float min_std, const float* featx,
                                            const float* prior_std, const float* post_std, const float* xsa, const float* e,
                                            const float* gates, const float* hp, const float* hq, const float* dfeat,
                                            const float* dprior_state, const float* dpm, const float* dps, const float* dqm,
                                            const float* dqs, float* dembeds, float* dprev_belief, float* dprev_state,
                                            int engine, unsigned* status, void* ws, size_t ws_bytes, hipStream_t stream,
                                            int act) {
  REPO_REQUIRE(engine == 0 || engine == 2, REPO_E_BADARG);
  return obs_bwd_run(T, B, A, D, Hd, S, E, params, nonterms, embeds, eps_prior, eps_post, noise_seed, noise_offset,
                     min_std, featx, prior_std, post_std, xsa, e, gates, hp, hq, dfeat, dprior_state, dpm, dps, dqm, dqs,
                     nullptr, dembeds, dprev_belief, dprev_state, engine, status, ws, ws_bytes, stream, act, false);
}

// ---- the pre-v9 entry points: the ELU instantiations
extern "C" int repo_rssm_observe_fwd(int64_t T, int64_t B, int64_t A, int64_t D, int64_t Hd, int64_t S, int64_t E,
                                     const float* const* params, const float* prev_belief, const float* prev_state,
                                     const float* actions, const float* nonterms, const float* embeds,
                                     const float* eps_prior, const float* eps_post, uint64_t noise_seed,
                                     uint64_t noise_offset, float min_std, float* featx,
                                     float* prior_state, float* prior_mean, float* prior_std, float* post_mean,
                                     float* post_std, float* xsa, float* e, float* gates, float* hp, float* hq,
                                     float* eemb, int prior_only, unsigned* status, void* ws, size_t ws_bytes,
                                     hipStream_t stream) {
  return repo_rssm_observe_fwd_act(T, B, A, D, Hd, S, E, params, prev_belief, prev_state, actions, nonterms, embeds,
                                   eps_prior, eps_post, noise_seed, noise_offset, min_std, featx, prior_state, prior_mean,
                                   prior_std, post_mean, post_std, xsa, e, gates, hp, hq, eemb, prior_only, status, ws,
                                   ws_bytes, stream, REPO_ACT_ELU);
}

extern "C" int repo_rssm_prior_head(int64_t T, int64_t B, int64_t D, int64_t Hd, int64_t S, const float* const* params,
                                    const float* featx, const float* eps_prior, uint64_t noise_seed,
                                    uint64_t noise_offset, float min_std, float* hp, float* prior_state,
                                    float* prior_mean, float* prior_std, void* ws, size_t ws_bytes,
                                    hipStream_t stream) {
  return repo_rssm_prior_head_act(T, B, D, Hd, S, params, featx, eps_prior, noise_seed, noise_offset, min_std, hp,
                                  prior_state, prior_mean, prior_std, ws, ws_bytes, stream, REPO_ACT_ELU);
}

extern "C" int repo_rssm_observe_bwd(int64_t T, int64_t B, int64_t A, int64_t D, int64_t Hd, int64_t S, int64_t E,
                                     const float* const* params, const float* nonterms, const float* embeds,
                                     const float* eps_prior, const float* eps_post, uint64_t noise_seed,
                                     uint64_t noise_offset, float min_std, const float* featx,
                                     const float* prior_std, const float* post_std, const float* xsa, const float* e,
                                     const float* gates, const float* hp, const float* hq, const float* dfeat,
                                     const float* dprior_state, const float* dpm, const float* dps, const float* dqm,
                                     const float* dqs, float* const* dparams, float* dembeds, float* dprev_belief,
                                     float* dprev_state, int accumulate, unsigned* status, void* ws,
                                     size_t ws_bytes, hipStream_t stream) {
  return repo_rssm_observe_bwd_act(T, B, A, D, Hd, S, E, params, nonterms, embeds, eps_prior, eps_post, noise_seed,
                                   noise_offset, min_std, featx, prior_std, post_std, xsa, e, gates, hp, hq, dfeat,
                                   dprior_state, dpm, dps, dqm, dqs, dparams, dembeds, dprev_belief, dprev_state,
                                   accumulate, status, ws, ws_bytes, stream, REPO_ACT_ELU);
}
