// The row scan's two kernels (forward, reverse).  NOT a header with a guard: rssm.hip includes this text once per dense
// activation, with REPO_SCAN_ACT (REPO_ACT_*) and the two kernel names defined -- the activation is a compile-time
// constant of each copy, and the ELU copy is the kernel pair observe_fwd_kernel<R, KQ> / observe_bwd_kernel<R, KQ> under
// the names and template arguments traces and profiles are matched on.
#if !defined(REPO_SCAN_ACT) || !defined(REPO_SCAN_FWD_KERNEL) || !defined(REPO_SCAN_BWD_KERNEL)
#error "rssm_scan.h is included by rssm.hip with REPO_SCAN_ACT and the kernel names defined"
#endif

// R rows per workgroup, KQ-way split of every reduction (k) range over thread groups of 256:
// thread (kq, j) accumulates feature j over its quarter of k, partials meet in LDS.  The scan is
// bound by the latency of streaming ~1.4 MB of L2-resident weights per step through ONE CU; the
// k-split multiplies the loads in flight (memory-level parallelism), which is what that needs.
template <int R, int KQ>
__global__ __launch_bounds__(256 * KQ) void REPO_SCAN_FWD_KERNEL(ObsFwdArgs p) {
  constexpr int ACT = REPO_SCAN_ACT;
  const int T = p.d.T, B = p.d.B, A = p.d.A, D = p.d.D, Hd = p.d.Hd, S = p.d.S;
  const int X = S + A, F = D + S;
  __shared__ __attribute__((aligned(16))) float xs[R][kMaxX];
  __shared__ __attribute__((aligned(16))) float es[R][kMaxW];
  __shared__ __attribute__((aligned(16))) float hs[2][R][kMaxW];
  __shared__ __attribute__((aligned(16))) float hps[R][kMaxW];
  __shared__ __attribute__((aligned(16))) float hqs[R][kMaxW];
  __shared__ float outs[R][2 * kMaxS2];  // [0,2S) prior raw, [2S,4S) posterior raw
  __shared__ float st[R][kMaxS2];
  __shared__ float part[KQ][6][R][kMaxW];  // k-split partial sums

  const int tid = threadIdx.x;
  const int j = tid & 255;
  const int kq = __builtin_amdgcn_readfirstlane(tid >> 8);
  const int b0 = blockIdx.x * R;
  int nr = B - b0;
  if (nr > R) nr = R;
  // this thread group's range of k GROUPS (4 consecutive k each) of a K-long reduction
  auto krange = [&](int K, int& g0, int& g1) {
    const int KG = (K + 3) >> 2, per = (KG + KQ - 1) / KQ;
    g0 = kq * per;
    g1 = min(KG, g0 + per);
  };
  // rows of the operand vectors beyond their width are read by the zero-padded last k group
  for (int i = tid; i < R * kMaxX; i += blockDim.x) (&xs[0][0])[i] = 0.f;
  for (int i = tid; i < R * kMaxW; i += blockDim.x) {
    (&es[0][0])[i] = 0.f;
    (&hs[0][0][0])[i] = 0.f;
    (&hs[1][0][0])[i] = 0.f;
    (&hps[0][0])[i] = 0.f;
    (&hqs[0][0])[i] = 0.f;
  }
  __syncthreads();

  // slot 0 of featx and the carried state
  for (int i = tid; i < R * D; i += blockDim.x) {
    const int r = i / D, c = i % D;
    const float v = r < nr ? p.prev_belief[(size_t)(b0 + r) * D + c] : 0.f;
    hs[0][r][c] = v;
    if (r < nr) p.featx[(size_t)(b0 + r) * F + c] = v;
  }
  for (int i = tid; i < R * S; i += blockDim.x) {
    const int r = i / S, c = i % S;
    const float v = r < nr ? p.prev_state[(size_t)(b0 + r) * S + c] : 0.f;
    st[r][c] = v;
    if (r < nr) p.featx[(size_t)(b0 + r) * F + D + c] = v;
  }
  __syncthreads();

  // Every step is a chain of ten dependent stages; a global load issued where its value is needed adds its
  // whole latency (an L2 / HBM round trip, longer when other kernels share the chip) to that chain.  So: the
  // biases live in registers for the whole scan, and the per-step operands (nonterminal / action of the x
  // vector, the hoisted embed contribution) are fetched one step AHEAD, while the previous step computes.
  const bool feat_thr = tid < D, hid_thr = tid < Hd, out_thr = tid < 4 * S;
  const float b_sa = feat_thr ? p.bsa[tid] : 0.f;
  float b_g[6];
#pragma unroll
  for (int g = 0; g < 6; ++g) b_g[g] = feat_thr ? (g < 3 ? p.bih[g * D + tid] : p.bhh[(g - 3) * D + tid]) : 0.f;
  const float b_bp = hid_thr ? p.bbp[tid] : 0.f, b_bq = hid_thr ? p.bbq[tid] : 0.f;
  const float b_out = out_thr ? (tid >= 2 * S ? p.bsq[tid - 2 * S] : p.bsp[tid]) : 0.f;
  // x-vector role of this thread (R * X <= blockDim): element (xr, xk)
  const int xr = tid / X, xk = tid % X;
  const bool x_thr = tid < R * X && xr < nr;
  auto load_x = [&](int t) __attribute__((always_inline)) {
    const size_t row = (size_t)t * B + b0 + xr;
    return x_thr ? (xk < S ? p.nonterms[row] : p.actions[row * A + (xk - S)]) : 0.f;
  };
  float em_next[R];
  auto load_em = [&](int t) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      em_next[r] = (hid_thr && r < nr) ? p.eemb[((size_t)t * B + b0 + r) * Hd + tid] : 0.f;
  };
  float x_next = T > 0 ? load_x(0) : 0.f;
  if (T > 0) load_em(0);

  int cur = 0;
  for (int t = 0; t < T; ++t) {
    const size_t row0 = (size_t)t * B + b0;  // flattened (t, b0)
    const float x_in = x_next;
    float em[R];
#pragma unroll
    for (int r = 0; r < R; ++r) em[r] = em_next[r];
    if (t + 1 < T) {
      x_next = load_x(t + 1);
      load_em(t + 1);
    }
    // ---- x = [state * nonterm, action]
    if (tid < R * X) {
      float v = 0.f;
      if (x_thr) {
        v = xk < S ? st[xr][xk] * x_in : x_in;
        p.xsa[(row0 + xr) * X + xk] = v;
      }
      xs[xr][xk] = v;
    }
    __syncthreads();
    // ---- e = act(W_sa x + b)
    if (j < D) {
      float acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = 0.f;
      int k0, k1;
      krange(X, k0, k1);
      const float4* W4 = reinterpret_cast<const float4*>(p.WsaT);
#pragma unroll 2
      for (int g = k0; g < k1; ++g) {
        const float4 w = W4[g * D + j];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fma4(w, &xs[r][4 * g], acc[r]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) part[kq][0][r][j] = acc[r];
    }
    __syncthreads();
    if (tid < D) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float acc = b_sa;
#pragma unroll
        for (int q = 0; q < KQ; ++q) acc += part[q][0][r][tid];
        const float v = act_fn<ACT>(acc);
        es[r][tid] = v;
        if (r < nr) p.e[(row0 + r) * D + tid] = v;
      }
    }
    __syncthreads();
    // ---- GRU cell (gate order r,z,n): partial sums over this thread's k range
    if (j < D) {
      float gi[3][R], gh[3][R];
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < R; ++r) gi[g][r] = gh[g][r] = 0.f;
      const float* hc = &hs[cur][0][0];
      int k0, k1;
      krange(D, k0, k1);
      const float4* Wi4 = reinterpret_cast<const float4*>(p.WihT);
      const float4* Wh4 = reinterpret_cast<const float4*>(p.WhhT);
#pragma unroll 2
      for (int g = k0; g < k1; ++g) {
        const float4* wi = Wi4 + (size_t)g * 3 * D + j;
        const float4* wh = Wh4 + (size_t)g * 3 * D + j;
        const float4 wi0 = wi[0], wi1 = wi[D], wi2 = wi[2 * D];
        const float4 wh0 = wh[0], wh1 = wh[D], wh2 = wh[2 * D];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float* ev = &es[r][4 * g];
          const float* hv = hc + r * kMaxW + 4 * g;
          gi[0][r] = fma4(wi0, ev, gi[0][r]);
          gi[1][r] = fma4(wi1, ev, gi[1][r]);
          gi[2][r] = fma4(wi2, ev, gi[2][r]);
          gh[0][r] = fma4(wh0, hv, gh[0][r]);
          gh[1][r] = fma4(wh1, hv, gh[1][r]);
          gh[2][r] = fma4(wh2, hv, gh[2][r]);
        }
      }
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          part[kq][g][r][j] = gi[g][r];
          part[kq][3 + g][r][j] = gh[g][r];
        }
    }
    __syncthreads();
    if (tid < D) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float g6[6];
#pragma unroll
        for (int g = 0; g < 6; ++g) {
          float sacc = b_g[g];
#pragma unroll
          for (int q = 0; q < KQ; ++q) sacc += part[q][g][r][tid];
          g6[g] = sacc;
        }
        const float rg = sigmoidf(g6[0] + g6[3]);
        const float zg = sigmoidf(g6[1] + g6[4]);
        const float ng = tanh_fast(g6[2] + rg * g6[5]);
        const float hprev = hs[cur][r][tid];
        const float hn = (1.f - zg) * ng + zg * hprev;
        hs[cur ^ 1][r][tid] = hn;
        if (r < nr) {
          float* g = p.gates + (row0 + r) * 4 * D;
          g[tid] = rg;
          g[D + tid] = zg;
          g[2 * D + tid] = ng;
          g[3 * D + tid] = g6[5];
          p.featx[((size_t)(t + 1) * B + b0 + r) * F + tid] = hn;
        }
      }
    }
    __syncthreads();
    cur ^= 1;
    // ---- hidden layers of the prior and the posterior heads
    if (j < Hd) {
      float ap[R], aq[R];
#pragma unroll
      for (int r = 0; r < R; ++r) ap[r] = aq[r] = 0.f;
      const float* hc = &hs[cur][0][0];
      int k0, k1;
      krange(D, k0, k1);
      const float4* Wp4 = reinterpret_cast<const float4*>(p.WbpT);
      const float4* Wq4 = reinterpret_cast<const float4*>(p.WbqT);
      if (p.skip_prior) {  // the prior head depends on belief_t only: off the recurrence, done for all steps afterwards
#pragma unroll 2
        for (int g = k0; g < k1; ++g) {
          const float4 wq = Wq4[(size_t)g * Hd + j];
#pragma unroll
          for (int r = 0; r < R; ++r) aq[r] = fma4(wq, hc + r * kMaxW + 4 * g, aq[r]);
        }
      } else {
#pragma unroll 2
        for (int g = k0; g < k1; ++g) {
          const float4 wp = Wp4[(size_t)g * Hd + j];
          const float4 wq = Wq4[(size_t)g * Hd + j];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float* hv = hc + r * kMaxW + 4 * g;
            ap[r] = fma4(wp, hv, ap[r]);
            aq[r] = fma4(wq, hv, aq[r]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        part[kq][0][r][j] = ap[r];
        part[kq][1][r][j] = aq[r];
      }
    }
    __syncthreads();
    if (tid < Hd) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float ap = b_bp, aq = b_bq + em[r];
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          ap += part[q][0][r][tid];
          aq += part[q][1][r][tid];
        }
        const float vp = act_fn<ACT>(ap), vq = act_fn<ACT>(aq);
        hps[r][tid] = vp;
        hqs[r][tid] = vq;
        if (r < nr) {
          if (!p.skip_prior) p.hp[(row0 + r) * Hd + tid] = vp;
          p.hq[(row0 + r) * Hd + tid] = vq;
        }
      }
    }
    __syncthreads();
    // ---- output layers: columns [0,2S) prior, [2S,4S) posterior; k split as above
    if (j < 4 * S && (j >= 2 * S || !p.skip_prior)) {
      const bool post = j >= 2 * S;
      const int o = post ? j - 2 * S : j;
      const float* Wt = post ? p.WsqT : p.WspT;
      const float* hsrc = post ? &hqs[0][0] : &hps[0][0];
      float acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = 0.f;
      int k0, k1;
      krange(Hd, k0, k1);
      const float4* W4 = reinterpret_cast<const float4*>(Wt);
#pragma unroll 2
      for (int g = k0; g < k1; ++g) {
        const float4 w = W4[(size_t)g * 2 * S + o];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fma4(w, hsrc + r * kMaxW + 4 * g, acc[r]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) part[kq][0][r][j] = acc[r];
    }
    __syncthreads();
    if (tid < 4 * S) {
      const bool post = tid >= 2 * S;
      const int o = post ? tid - 2 * S : tid;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float acc = b_out;
#pragma unroll
        for (int q = 0; q < KQ; ++q) acc += part[q][0][r][tid];
        outs[r][tid] = acc;
      }
    }
    __syncthreads();
    // ---- softplus + reparameterised samples
    for (int i = tid; i < R * 2 * S; i += blockDim.x) {
      const int r = i / (2 * S), q = i % (2 * S);
      const bool post = q >= S;
      const int s = post ? q - S : q;
      const int base = post ? 2 * S : 0;
      const float mean = outs[r][base + s];
      const float sd = softplus(outs[r][base + S + s]) + p.min_std;
      if (r < nr && (post || !p.skip_prior)) {
        const size_t o = (row0 + r) * S + s;
        const float eps = post ? p.eps_post.at(o) : p.eps_prior.at(o);
        const float smp = fmaf(sd, eps, mean);
        if (post) {
          p.post_mean[o] = mean;
          p.post_std[o] = sd;
          if (!p.prior_only) {
            p.featx[((size_t)(t + 1) * B + b0 + r) * F + D + s] = smp;
            st[r][s] = smp;
          }
        } else {
          p.prior_mean[o] = mean;
          p.prior_std[o] = sd;
          p.prior_state[o] = smp;
          if (p.prior_only) {
            p.featx[((size_t)(t + 1) * B + b0 + r) * F + D + s] = smp;
            st[r][s] = smp;
          }
        }
      }
    }
    __syncthreads();
  }
}

template <int R, int KQ>
__global__ __launch_bounds__(256 * KQ) void REPO_SCAN_BWD_KERNEL(ObsBwdArgs p) {
  constexpr int ACT = REPO_SCAN_ACT;
  const int T = p.d.T, B = p.d.B, A = p.d.A, D = p.d.D, Hd = p.d.Hd, S = p.d.S;
  const int X = S + A, F = D + S;
  __shared__ float dh[R][kMaxW];      // carried d belief
  __shared__ float dst[R][kMaxS2];    // carried d posterior state
  __shared__ float dbel[R][kMaxW];
  __shared__ __attribute__((aligned(16))) float douts[R][2 * kMaxS2];
  __shared__ __attribute__((aligned(16))) float dhps[R][kMaxW];
  __shared__ __attribute__((aligned(16))) float dhqs[R][kMaxW];
  __shared__ __attribute__((aligned(16))) float dgis[R][3 * kMaxW];
  __shared__ __attribute__((aligned(16))) float dghs[R][3 * kMaxW];
  __shared__ __attribute__((aligned(16))) float des[R][kMaxW];
  __shared__ float part[KQ][2][R][kMaxW];  // k-split partial sums

  const int tid = threadIdx.x;
  const int j = tid & 255;
  const int kq = __builtin_amdgcn_readfirstlane(tid >> 8);
  const int b0 = blockIdx.x * R;
  int nr = B - b0;
  if (nr > R) nr = R;
  // this thread group's range of k GROUPS (4 consecutive k each) of a K-long reduction
  auto krange = [&](int K, int& g0, int& g1) {
    const int KG = (K + 3) >> 2, per = (KG + KQ - 1) / KQ;
    g0 = kq * per;
    g1 = min(KG, g0 + per);
  };
  for (int i = tid; i < R * kMaxW; i += blockDim.x) {
    (&dhps[0][0])[i] = 0.f;
    (&dhqs[0][0])[i] = 0.f;
    (&des[0][0])[i] = 0.f;
  }
  for (int i = tid; i < R * 3 * kMaxW; i += blockDim.x) {
    (&dgis[0][0])[i] = 0.f;
    (&dghs[0][0])[i] = 0.f;
  }
  for (int i = tid; i < R * 2 * kMaxS2; i += blockDim.x) (&douts[0][0])[i] = 0.f;
  for (int i = tid; i < R * kMaxW; i += blockDim.x) (&dh[0][0])[i] = 0.f;
  for (int i = tid; i < R * kMaxS2; i += blockDim.x) (&dst[0][0])[i] = 0.f;
  __syncthreads();

  // The saved activations and upstream gradients a step reads (each a dependent global load in front of one of
  // its eight stages) are fetched one step AHEAD into registers: in the update this scan shares the chip with the
  // decoder's backward, and a load issued where its value is needed then costs 1-2 us of the chain.
  struct StepIn {
    float dfb[R], g_r[R], g_z[R], g_n[R], g_hn[R], hprev[R], ev[R];  // feature threads (tid < D)
    float hp[R], hq[R];                                              // hidden threads (tid < Hd)
    float o_dsmp, o_dm, o_dsd, o_sd;                                 // output-delta role (tid < R * 2S)
    float nt[R];                                                     // tid < S
  };
  const int orr = tid / (2 * S), oq = tid % (2 * S);
  const bool o_thr = tid < R * 2 * S && orr < nr, o_post = oq >= S;
  const int o_s = o_post ? oq - S : oq;
  // one register set: each group of fields is re-loaded for step t-1 right after step t's last use of it
  StepIn in;
  auto load_top = [&](int t) __attribute__((always_inline)) {  // consumed by the first stage
    const size_t row0 = (size_t)t * B + b0;
#pragma unroll
    for (int r = 0; r < R; ++r) in.dfb[r] = (tid < D && r < nr && p.dfeat) ? p.dfeat[(row0 + r) * F + tid] : 0.f;
    in.o_dsmp = in.o_dm = in.o_dsd = in.o_sd = 0.f;
    if (o_thr) {
      const size_t o = (row0 + orr) * S + o_s;
      if (o_post) {
        in.o_dsmp = p.dfeat ? p.dfeat[(row0 + orr) * F + D + o_s] : 0.f;
        in.o_dm = p.dqm ? p.dqm[o] : 0.f;
        in.o_dsd = p.dqs ? p.dqs[o] : 0.f;
        in.o_sd = p.post_std[o];
      } else {
        in.o_dsmp = p.dprior_state ? p.dprior_state[o] : 0.f;
        in.o_dm = p.dpm ? p.dpm[o] : 0.f;
        in.o_dsd = p.dps ? p.dps[o] : 0.f;
        in.o_sd = p.prior_std[o];
      }
    }
  };
  auto load_hid = [&](int t) __attribute__((always_inline)) {
    const size_t row0 = (size_t)t * B + b0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool ha = tid < Hd && r < nr;
      in.hp[r] = ha ? p.hp[(row0 + r) * Hd + tid] : 0.f;
      in.hq[r] = ha ? p.hq[(row0 + r) * Hd + tid] : 0.f;
    }
  };
  auto load_gru = [&](int t) __attribute__((always_inline)) {
    const size_t row0 = (size_t)t * B + b0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool fa = tid < D && r < nr;
      const float* g = p.gates + (row0 + r) * 4 * D;
      in.g_r[r] = fa ? g[tid] : 0.f;
      in.g_z[r] = fa ? g[D + tid] : 0.f;
      in.g_n[r] = fa ? g[2 * D + tid] : 0.f;
      in.g_hn[r] = fa ? g[3 * D + tid] : 0.f;
      in.hprev[r] = fa ? p.featx[((size_t)t * B + b0 + r) * F + tid] : 0.f;
    }
  };
  auto load_e = [&](int t) __attribute__((always_inline)) {
    const size_t row0 = (size_t)t * B + b0;
#pragma unroll
    for (int r = 0; r < R; ++r) in.ev[r] = (tid < D && r < nr) ? p.e[(row0 + r) * D + tid] : 0.f;
  };
  auto load_nt = [&](int t) __attribute__((always_inline)) {
    const size_t row0 = (size_t)t * B + b0;
#pragma unroll
    for (int r = 0; r < R; ++r) in.nt[r] = (tid < S && r < nr) ? p.nonterms[row0 + r] : 0.f;
  };
  if (T > 0) {
    load_top(T - 1);
    load_hid(T - 1);
    load_gru(T - 1);
    load_e(T - 1);
    load_nt(T - 1);
  }

  for (int t = T - 1; t >= 0; --t) {
    const size_t row0 = (size_t)t * B + b0;
    const int tn = t > 0 ? t - 1 : 0;  // the step whose operands are fetched behind each stage (t = 0: a harmless re-read)
    // ---- total gradient on belief_t; heads' output-layer deltas
    if (tid < D) {
#pragma unroll
      for (int r = 0; r < R; ++r) dbel[r][tid] = dh[r][tid] + in.dfb[r];
    }
    if (tid < R * 2 * S) {
      const int r = orr, s = o_s;
      const bool post = o_post;
      float dm = 0.f, draw = 0.f;
      if (r < nr) {
        const size_t o = (row0 + r) * S + s;
        float dsmp = in.o_dsmp + (post ? dst[r][s] : 0.f), dsd = in.o_dsd;
        const float sd = in.o_sd;
        const float eps = post ? p.eps_post.at(o) : p.eps_prior.at(o);
        dm = in.o_dm;
        dm += dsmp;
        dsd = fmaf(dsmp, eps, dsd);
        // d softplus(raw)/d raw = sigmoid(raw) = 1 - exp(-softplus(raw))
        draw = dsd * (-expm1f(-(sd - p.min_std)));
        float* dst_out = post ? p.doutq : p.doutp;
        dst_out[(row0 + r) * 2 * S + s] = dm;
        dst_out[(row0 + r) * 2 * S + S + s] = draw;
      }
      const int base = post ? 2 * S : 0;
      douts[r][base + s] = dm;
      douts[r][base + S + s] = draw;
    }
    load_top(tn);
    __syncthreads();
    // ---- back through the output layers to the hidden pre-activations
    if (j < Hd) {
      float ap[R], aq[R];
#pragma unroll
      for (int r = 0; r < R; ++r) ap[r] = aq[r] = 0.f;
      int k0, k1;
      krange(2 * S, k0, k1);
      const float4* Wp4 = reinterpret_cast<const float4*>(p.Wsp);
      const float4* Wq4 = reinterpret_cast<const float4*>(p.Wsq);
#pragma unroll 2
      for (int g = k0; g < k1; ++g) {
        const float4 wp = Wp4[(size_t)g * Hd + j];
        const float4 wq = Wq4[(size_t)g * Hd + j];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          ap[r] = fma4(wp, &douts[r][4 * g], ap[r]);
          aq[r] = fma4(wq, &douts[r][2 * S + 4 * g], aq[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        part[kq][0][r][j] = ap[r];
        part[kq][1][r][j] = aq[r];
      }
    }
    __syncthreads();
    if (tid < Hd) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float ap = 0.f, aq = 0.f;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          ap += part[q][0][r][tid];
          aq += part[q][1][r][tid];
        }
        float vp = 0.f, vq = 0.f;
        if (r < nr) {
          vp = ap * act_grad_from_out<ACT>(in.hp[r]);
          vq = aq * act_grad_from_out<ACT>(in.hq[r]);
          p.dhp[(row0 + r) * Hd + tid] = vp;
          p.dhq[(row0 + r) * Hd + tid] = vq;
        }
        dhps[r][tid] = vp;
        dhqs[r][tid] = vq;
      }
    }
    load_hid(tn);
    __syncthreads();
    // ---- into belief_t (k-split partial sums over the hidden index)
    if (j < D) {
      float acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = 0.f;
      int k0, k1;
      krange(Hd, k0, k1);
      const float4* Wp4 = reinterpret_cast<const float4*>(p.Wbp);
      const float4* Wq4 = reinterpret_cast<const float4*>(p.Wbq);
#pragma unroll 2
      for (int g = k0; g < k1; ++g) {
        const float4 wp = Wp4[(size_t)g * D + j];
        const float4 wq = Wq4[(size_t)g * D + j];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fma4(wp, &dhps[r][4 * g], fma4(wq, &dhqs[r][4 * g], acc[r]));
      }
#pragma unroll
      for (int r = 0; r < R; ++r) part[kq][0][r][j] = acc[r];
    }
    __syncthreads();
    // ---- through the GRU gates (pointwise in the feature index)
    if (tid < D) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float db_ = dbel[r][tid];
#pragma unroll
        for (int q = 0; q < KQ; ++q) db_ += part[q][0][r][tid];
        float g_r = 0.f, g_z = 0.f, g_n = 0.f, g_hn = 0.f, dhprev = 0.f;
        if (r < nr) {
          const float rg = in.g_r[r], zg = in.g_z[r], ng = in.g_n[r], ghn = in.g_hn[r];
          const float hprev = in.hprev[r];
          const float dn = db_ * (1.f - zg);
          const float dz = db_ * (hprev - ng);
          dhprev = db_ * zg;
          g_n = dn * (1.f - ng * ng);
          g_hn = g_n * rg;
          g_r = g_n * ghn * rg * (1.f - rg);
          g_z = dz * zg * (1.f - zg);
          float* gi = p.dgi + (row0 + r) * 3 * D;
          float* gh = p.dgh + (row0 + r) * 3 * D;
          gi[tid] = g_r;
          gi[D + tid] = g_z;
          gi[2 * D + tid] = g_n;
          gh[tid] = g_r;
          gh[D + tid] = g_z;
          gh[2 * D + tid] = g_hn;
        }
        dgis[r][tid] = g_r;
        dgis[r][D + tid] = g_z;
        dgis[r][2 * D + tid] = g_n;
        dghs[r][tid] = g_r;
        dghs[r][D + tid] = g_z;
        dghs[r][2 * D + tid] = g_hn;
        dh[r][tid] = dhprev;
      }
    }
    load_gru(tn);
    __syncthreads();
    // ---- through W_hh into belief_{t-1}, through W_ih into e (k-split over the 3D gate index)
    if (j < D) {
      float ah[R], ae[R];
#pragma unroll
      for (int r = 0; r < R; ++r) ah[r] = ae[r] = 0.f;
      int k0, k1;
      krange(3 * D, k0, k1);
      const float4* Wh4 = reinterpret_cast<const float4*>(p.Whh);
      const float4* Wi4 = reinterpret_cast<const float4*>(p.Wih);
#pragma unroll 2
      for (int g = k0; g < k1; ++g) {
        const float4 wh = Wh4[(size_t)g * D + j];
        const float4 wi = Wi4[(size_t)g * D + j];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          ah[r] = fma4(wh, &dghs[r][4 * g], ah[r]);
          ae[r] = fma4(wi, &dgis[r][4 * g], ae[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        part[kq][0][r][j] = ah[r];
        part[kq][1][r][j] = ae[r];
      }
    }
    __syncthreads();
    if (tid < D) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float ah = dh[r][tid], ae = 0.f;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          ah += part[q][0][r][tid];
          ae += part[q][1][r][tid];
        }
        dh[r][tid] = ah;
        float v = 0.f;
        if (r < nr) {
          v = ae * act_grad_from_out<ACT>(in.ev[r]);
          p.de[(row0 + r) * D + tid] = v;
        }
        des[r][tid] = v;
      }
    }
    load_e(tn);
    __syncthreads();
    // ---- through W_sa into the previous posterior state (masked by nonterminal)
    if (j < S) {
      float acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = 0.f;
      int k0, k1;
      krange(D, k0, k1);
      const float4* W4 = reinterpret_cast<const float4*>(p.Wsa);
#pragma unroll 2
      for (int g = k0; g < k1; ++g) {
        const float4 w = W4[(size_t)g * S + j];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fma4(w, &des[r][4 * g], acc[r]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) part[kq][0][r][j] = acc[r];
    }
    __syncthreads();
    if (tid < S) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < KQ; ++q) acc += part[q][0][r][tid];
        dst[r][tid] = r < nr ? acc * in.nt[r] : 0.f;
      }
    }
    load_nt(tn);
    __syncthreads();
  }
  if (p.dprev_belief)
    for (int i = tid; i < nr * D; i += blockDim.x) p.dprev_belief[(size_t)(b0 + i / D) * D + i % D] = dh[i / D][i % D];
  if (p.dprev_state)
    for (int i = tid; i < nr * S; i += blockDim.x) p.dprev_state[(size_t)(b0 + i / S) * S + i % S] = dst[i / S][i % S];
}
