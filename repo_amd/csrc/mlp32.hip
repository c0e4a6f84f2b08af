// Fused dense heads on 32-row tiles and the bf16 matrix pipe (rowtile32.h): the chains of mlp16.hip -- same operands,
// same saved activations, same pre-activation gradients -- with every product formed as the exact three-way bf16
// split's six partial products ("bf16x6", bgemm.h) accumulated in fp32.
//
// A persistent workgroup (8 waves) takes 32 rows at a time through the whole chain.  Waves 0..6 own one 32-column tile
// of a 200-wide layer each; wave 7 is the STORE WAVE: behind a layer's barrier it writes that layer's tile to its
// row-major fp32 matrix (the saved activation / the pre-activation gradient) while the others multiply the next layer.
//
// LDS holds ONE plane triple (forward: 240 columns, 46 080 B; reverse: 208 columns, 39 936 B), used IN PLACE: a layer's
// outputs wait in the accumulators for the barrier behind which nobody reads the layer's input, and are then split over
// it.  Two plane triples (86 016 B) would leave one workgroup per CU; with one, two workgroups are resident and one's
// barrier / epilogue phases run beside the other's MFMAs.  The weight stream has ONE register window of 3 blocks per
// wave, re-opened for the next layer as soon as the current product has consumed it (before the epilogue and both
// barriers), which keeps a wave within the 128 registers that four waves per SIMD leave.
//
// Reference: the nn.Sequential heads of models/actor_critic.py:10-60 and models/reward.py and autograd's backward.
#include <cstdlib>

#include "rowtile32.h"

namespace repo {

bool rowtile32_enabled();  // imagine32.hip

constexpr int kMPD = 3;
typedef WWin32<kMPD> WinM;
constexpr int kM32MaxL = 5;

struct Mlp32FwdArgs {
  int rows, in_dim, hidden, out_dim, ldx, ldo;
  const float* x;
  const char* wpack;
  unsigned wbytes;
  unsigned W[kM32MaxL], B[kM32MaxL];
  float* hid[kM32MaxL - 1];
  float* out;
};

struct Mlp32BwdArgs {
  int rows, in_dim, hidden, out_dim, lddout, lddx, accumulate_dx, rows_w, ldw;
  const float* dout;
  // The bf16 pipe's accumulation error has a part that does NOT follow the sign of what is summed (measured: ~ 7e-9 of a
  // row's scale, the same way whatever the upstream's sign).  Element by element that is far below fp32 rounding, but
  // in a column sum over tens of thousands of rows whose terms cancel (a bias gradient under random-sign upstreams) it
  // adds up: 2.6e-6 .. 3.9e-6 against the fp32 engine's 3e-7 .. 5e-7 with the upstream simply folded into the chain.
  // So the chain never runs on the upstream as it comes:
  //   * a SCALAR head (out_dim == 1) runs on the UNIT upstream; the input gradient leaves scaled by dout[row], the
  //     saved pre-activation gradients by dout_w[row * ldw] (rows >= rows_w: 0) -- the second upstream of mlp16.hip's
  //     MlpBwdArgs, or dout itself.  The error is then a factor's worth of the signal and cancels with it (3e-7);
  //   * a wider head (dout_w null) runs every ODD row on the negated upstream and negates what leaves (exact both
  //     ways): the error alternates in sign from row to row.
  const float* dout_w;
  const char* wpack;    // transposed packs: layer l as (N' = k_l, K' = n_l)
  unsigned wbytes;
  unsigned W[kM32MaxL];
  const float* hid[kM32MaxL - 1];
  float* dsave[kM32MaxL - 1];
  float* dx;
};

// The 32-row tiles a workgroup owns: a contiguous run (the grid is at most two workgroups per CU).
struct Tiles32 {
  int first, count;
};
__device__ __forceinline__ Tiles32 my_tiles32(int rows) {
  const int nt = (rows + kR32 - 1) / kR32, g = gridDim.x, b = blockIdx.x;
  const int base = nt / g, rem = nt % g;
  return Tiles32{b * base + min(b, rem), base + (b < rem ? 1 : 0)};
}

template <int NBLK, bool BIAS>
__device__ __forceinline__ void mopen32(WinM& w, __amdgpu_buffer_rsrc_t rw, unsigned W, unsigned B, int N, int wave,
                                        int lane) {
  const int nt = (N + 31) >> 5;
  wopen32<NBLK, kMPD, BIAS>(w, rw, wave < nt, W, B, N, min(wave, nt - 1), lane);
}

// Input rows -> registers -> planes.  A lane takes column PAIRS (one split, one 4-byte LDS store per plane): per
// instruction a wave covers 8 rows x 16 columns.  Columns at and beyond in_dim are stored as zeros; rows beyond the
// tile's last are copies of its last row (rows never mix: a lane's accumulators belong to one row).
template <int BI>
struct XLoad32 {
  float v[16];
  __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rx, int ldx, int r0, int nr, int wave, int lane) {
    const int row = 8 * (wave & 3) + (lane >> 3);
    const int f0 = 16 * (wave >> 2) + 2 * (lane & 7);
    const unsigned vo = 4u * ((unsigned)(r0 + min(row, nr - 1)) * (unsigned)ldx + (unsigned)f0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[2 * j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, vo + 128u * j, 0, 0));
      v[2 * j + 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, vo + 128u * j + 4u, 0, 0));
    }
  }
  __device__ __forceinline__ void land(char* T, int ps, int F, int wave, int lane) {
    const int row = 8 * (wave & 3) + (lane >> 3);
    const int f0 = 16 * (wave >> 2) + 2 * (lane & 7);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = f0 + 32 * j;
      if (f < 16 * BI) {
        unsigned p1, p2, p3;
        rt_split3(f < F ? v[2 * j] : 0.f, f + 1 < F ? v[2 * j + 1] : 0.f, p1, p2, p3);
        char* d = T + pofs(f, row);
        *reinterpret_cast<unsigned*>(d) = p1;
        *reinterpret_cast<unsigned*>(d + ps) = p2;
        *reinterpret_cast<unsigned*>(d + 2 * ps) = p3;
      }
    }
  }
};

// store_tile32 (rowtile32.h) with a per-row factor (SCALE: the two-upstream mode's weight-side scalar) and the
// destination given as the TILE's first row: offsets stay far below the 2 GB window whatever the row count.
template <bool SCALE>
__device__ __forceinline__ void store_rows32(const char* T, int ps, int ncols, const float* dst_tile, int nr,
                                             unsigned ld, const float (&sc)[4], int lane, int g0, int gstep) {
  asm volatile("" : "+v"(lane));  // this call's lane arithmetic stays here: hoisted out of the tile loop it spills
  unsigned long long da = reinterpret_cast<unsigned long long>(dst_tile);
  unsigned dlo = (unsigned)da, dhi = (unsigned)(da >> 32);
  asm volatile("" : "+s"(dlo), "+s"(dhi));
  dlo = __builtin_amdgcn_readfirstlane(dlo), dhi = __builtin_amdgcn_readfirstlane(dhi);
  const __amdgpu_buffer_rsrc_t q = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<float*>(((unsigned long long)dhi << 32) | dlo), 0, 0x7fffffff, 0x00020000);
  const int piece = lane & 7, rsub = lane >> 3;
  unsigned vo[4];
  const char* src[4];
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int row = rg * 8 + rsub;
    vo[rg] = row < nr ? 4u * ((unsigned)row * ld + 4u * (unsigned)piece) : 0x80000000u;  // no row: out of range, dropped
    src[rg] = T + pofs(4 * piece, row);
  }
  const int ng = (ncols + 31) >> 5;
  const bool mine_last = (ng - 1) * 32 + 4 * piece < ncols;  // the last group may be ragged (ncols % 4 == 0)
  for (int g = g0; g < ng; g += gstep) {
    f32x4v q4[4];
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      q4[rg] = ldq32(src[rg] + 2048 * g, ps, 0, 0);
      if (SCALE) q4[rg] = q4[rg] * sc[rg];
    }
    const bool ok = g + 1 < ng || mine_last;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, q4[rg]), q,
                                             ok ? vo[rg] + 128u * (unsigned)g : 0x80000000u, 0, 0);
  }
}

// ROWS (= 32) tells these instantiations from the 16-row engine's in a device trace.
template <int BI, int BH, int L, int ACT, int ROWS>
__global__ __launch_bounds__(512, 4) void mlp_fwd_kernel(Mlp32FwdArgs p) {
  static_assert(ROWS == kR32 && BI >= BH, "one plane triple of the input's width");
  extern __shared__ __attribute__((aligned(16))) char lds32[];
  constexpr int ps = 1024 * BI;
  char* T = lds32;
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  const int F = p.in_dim, Hd = p.hidden, O = p.out_dim;
  const __amdgpu_buffer_rsrc_t rw = wrsrc(reinterpret_cast<const float*>(p.wpack), p.wbytes);
  const __amdgpu_buffer_rsrc_t rx = wrsrc(p.x, 4u * ((unsigned)(p.rows - 1) * (unsigned)p.ldx + (unsigned)p.in_dim));
  const bool swave = wave == kW - 1;
  const float one[4] = {1.f, 1.f, 1.f, 1.f};

  Tiles32 mt = my_tiles32(p.rows);
  if (mt.count <= 0) return;
  XLoad32<BI> xl;
  xl.issue(rx, p.ldx, mt.first * kR32, min(kR32, p.rows - mt.first * kR32), wave, tid0 & 63);
  WinM w;
  mopen32<BI, true>(w, rw, p.W[0], p.B[0], Hd, wave, tid0 & 63);
  while (mt.count > 0) {
    const int r0 = mt.first * kR32;
    const int nr = min(kR32, p.rows - r0);
    mt.first += 1, mt.count -= 1;
    int lane = tid0 & 63;
    asm volatile("" : "+v"(lane));  // per-tile lane arithmetic stays inside the tile: hoisted out of this loop it spills
    const int li = lane & 31, lh = lane >> 5;
    const int xf = xfrag32(lane);
    const int c0 = wave * 32 + 4 * lh;  // first column of this lane's quad 0 in a layer tile
    xl.land(T, ps, F, wave, lane);
    lds_barrier();
#pragma unroll
    for (int l = 0; l < L - 1; ++l) {
      const bool act = w.act;
      f32x16v c = zero16();
      if (act) {
        c = bias_acc(w);
        if (l == 0)
          wrun32<BI, kMPD>(c, T + xf, ps, w, rw);
        else
          wrun32<BH, kMPD>(c, T + xf, ps, w, rw);
      }
      // the window is consumed: the next layer's first blocks (and its bias) fly during the epilogue and the barriers
      mopen32<BH, true>(w, rw, p.W[l + 1], p.B[l + 1], l + 1 == L - 1 ? O : Hd, wave, lane);
      lds_barrier();  // nobody reads this layer's input any more (the store wave has read the previous layer's tile)
      if (act) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (wave * 32 + 8 * i < 16 * BH) {  // columns [hidden, 16 BH): act(0) = 0, and they meet zero weight rows
            const f32x4v a = quad(c, i);
            f32x4v v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = act_fn<ACT>(a[r]);
            stq32(T, ps, c0 + 8 * i, li, v);
          }
        }
      }
      lds_barrier();
      if (l < L - 2 && swave)
        store_rows32<false>(T, ps, Hd, p.hid[l] + (size_t)r0 * Hd, nr, (unsigned)Hd, one, lane, 0, 1);
    }
    // the output layer: one column tile (wave 0); the other waves share the last hidden tile's store
    const bool act = w.act;
    if (mt.count > 0) xl.issue(rx, p.ldx, mt.first * kR32, min(kR32, p.rows - mt.first * kR32), wave, lane);
    if (wave >= 1)
      store_rows32<false>(T, ps, Hd, p.hid[L - 2] + (size_t)r0 * Hd, nr, (unsigned)Hd, one, lane, wave - 1, kW - 1);
    f32x16v c = zero16();
    if (act) {
      c = bias_acc(w);
      wrun32<BH, kMPD>(c, T + xf, ps, w, rw);
    }
    mopen32<BI, true>(w, rw, p.W[0], p.B[0], Hd, wave, lane);  // the next tile's first layer
    if (act && li < nr) {
      float* o = p.out + (size_t)(r0 + li) * p.ldo;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = c0 + 8 * (e >> 2) + (e & 3);
        if (n < O) o[n] = c[e];
      }
    }
    lds_barrier();  // the tile is free for the next rows
  }
}

// stage s = 0 .. L-1 handles layer l = L-1-s: T = D_l * W_l; s < L-1: D_{l-1} = T * act'(h_{l-1}); s = L-1: dx = T.
template <int BI, int BH, int L, int ACT, int ROWS>
__global__ __launch_bounds__(512, 4) void mlp_bwd_kernel(Mlp32BwdArgs p) {
  static_assert(ROWS == kR32, "32-row tiles");
  extern __shared__ __attribute__((aligned(16))) char lds32[];
  constexpr int ps = 1024 * BH;
  char* T = lds32;
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  const int F = p.in_dim, Hd = p.hidden, O = p.out_dim;
  const __amdgpu_buffer_rsrc_t rw = wrsrc(reinterpret_cast<const float*>(p.wpack), p.wbytes);
  const bool swave = wave == kW - 1;
  const bool dual = p.dout_w != nullptr;  // (uniform; out_dim == 1): unit upstream, scalars behind the chain
  const bool do_dx = p.dx != nullptr;

  Tiles32 mt = my_tiles32(p.rows);
  if (mt.count <= 0) return;
  WinM w;
  mopen32<1, false>(w, rw, p.W[L - 1], 0, Hd, wave, tid0 & 63);
  while (mt.count > 0) {
    const int r0 = mt.first * kR32;
    const int nr = min(kR32, p.rows - r0);
    mt.first += 1, mt.count -= 1;
    int tid = tid0;
    asm volatile("" : "+v"(tid));  // per-tile lane arithmetic stays inside the tile: hoisted out of this loop it spills
    const int lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int xf = xfrag32(lane);
    const int c0 = wave * 32 + 4 * lh;
    {  // upstream gradient -> columns 0..15 of the tile (512 threads: one element each)
      const int row = tid & 31, f = tid >> 5;
      float v = 0.f;
      if (row < nr && f < O) v = dual ? 1.f : ((row & 1) ? -1.f : 1.f) * p.dout[(size_t)(r0 + row) * p.lddout + f];
      st1_32(T, ps, f, row, v);
    }
    lds_barrier();
#pragma unroll
    for (int s = 0; s < L - 1; ++s) {
      const int l = L - 1 - s;  // the layer whose transposed weights this stage multiplies by; its input is hid[l - 1]
      const bool act = w.act;
      f32x4v h[4];
      f32x16v c = zero16();
      if (act) {
        // the activations the epilogue multiplies by, requested ahead of the MFMA chain
        const __amdgpu_buffer_rsrc_t qh = arsrc(p.hid[l - 1] + (size_t)r0 * Hd);
        const unsigned lrow = (unsigned)min(li, nr - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = bldq(qh, 4u * (lrow * (unsigned)Hd + (unsigned)min(c0 + 8 * i, Hd - 4)), 0);
        if (s == 0)
          wrun32<1, kMPD>(c, T + xf, ps, w, rw);
        else
          wrun32<BH, kMPD>(c, T + xf, ps, w, rw);
      }
      mopen32<BH, false>(w, rw, p.W[l - 1], 0, l - 1 == 0 ? F : Hd, wave, lane);
      lds_barrier();  // nobody reads this stage's input any more
      if (act) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (wave * 32 + 8 * i < 16 * BH) {
            const f32x4v a = quad(c, i);
            f32x4v v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (c0 + 8 * i < Hd) ? a[r] * act_grad_from_out<ACT>(h[i][r]) : 0.f;
            stq32(T, ps, c0 + 8 * i, li, v);
          }
        }
      }
      lds_barrier();
      if (swave && p.dsave[l - 1]) {
        float sw[4];  // what this lane's four rows leave scaled by: the weight side's scalar / the row's sign
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int row = r0 + rg * 8 + (lane >> 3);
          sw[rg] = dual ? (row < p.rows_w ? p.dout_w[(size_t)row * p.ldw] : 0.f) : ((lane >> 3) & 1) ? -1.f : 1.f;
        }
        store_rows32<true>(T, ps, Hd, p.dsave[l - 1] + (size_t)r0 * Hd, nr, (unsigned)Hd, sw, lane, 0, 1);
      }
    }
    // the input gradient: 8 column tiles of in_dim, every wave one; leaves from the accumulators (lddx is the caller's)
    const bool act = w.act;
    // what this lane's accumulator row leaves scaled by: dx's upstream scalar / the row's sign
    float sx = (li & 1) ? -1.f : 1.f;
    if (dual) sx = (do_dx && li < nr) ? p.dout[(size_t)(r0 + li) * p.lddout] : 1.f;
    f32x16v c = zero16();
    if (do_dx && act) wrun32<BH, kMPD>(c, T + xf, ps, w, rw);
    mopen32<1, false>(w, rw, p.W[L - 1], 0, Hd, wave, lane);  // the next tile's first stage
    if (do_dx && act && li < nr) {
      float* d = p.dx + (size_t)(r0 + li) * p.lddx;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = c0 + 8 * (e >> 2) + (e & 3);
        if (n < F) d[n] = p.accumulate_dx ? fmaf(c[e], sx, d[n]) : c[e] * sx;
      }
    }
    lds_barrier();  // the tile is free for the next upstream rows
  }
}

// ------------------------------------------------------------------------------------------ host side
constexpr int kBI32 = 15, kBH32 = 13;  // mlp_fused_ok's shapes: in_dim 225..240, hidden 193..208, out_dim <= 16

// Rows from which a fused head call runs on this engine (below: the 16-row fp32 engine of mlp16.hip).  Measured, chain
// kernel alone, fp32 / bf16x6 in us (profiles/mlp32_threshold.txt): forward 20.6 / 21.1 at 4096 rows, 33.6 / 24.3 at 8192,
// 110 / 78 at 34 300; reverse 19.0 / 23.0, 31.9 / 28.4, 112 / 86.  Up to 4096 rows the fp32 engine has one 16-row block
// per workgroup and at most one workgroup per CU, and wins or ties; from 4097 rows some CU carries two of its workgroups
// (the step to 32-34 us) while this engine stays at one 32-row tile per workgroup up to 16 384 rows.
// REPO_MLP32_MIN_ROWS, read at every call, overrides both.
#ifndef REPO_MLP32_FWD_MIN_ROWS
#define REPO_MLP32_FWD_MIN_ROWS 4097
#endif
#ifndef REPO_MLP32_BWD_MIN_ROWS
#define REPO_MLP32_BWD_MIN_ROWS 4097
#endif
bool mlp32_routed(int64_t rows, bool reverse, const void* ws) {
  if (!rowtile32_enabled() || ((uintptr_t)ws & 15) != 0) return false;
  long long min_rows = reverse ? REPO_MLP32_BWD_MIN_ROWS : REPO_MLP32_FWD_MIN_ROWS;
  if (const char* e = std::getenv("REPO_MLP32_MIN_ROWS")) {
    char* end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    if (end != e && v >= 0) min_rows = v;
  }
  return rows >= min_rows;
}

size_t mlp32_ws_bytes(int64_t in_dim, int64_t hidden, int64_t out_dim, int n_layers) {
  const size_t f = pack32_bytes(hidden, in_dim) + (n_layers - 2) * pack32_bytes(hidden, hidden) +
                   pack32_bytes(out_dim, hidden) + (n_layers - 1) * vec32_bytes(hidden) + vec32_bytes(out_dim);
  const size_t b = pack32_bytes(in_dim, hidden) + (n_layers - 2) * pack32_bytes(hidden, hidden) + pack32_bytes(hidden, out_dim);
  return (f > b ? f : b) + 256;
}

// two workgroups per CU (2 x 46 KB LDS, <= 128 VGPRs)
static int grid32_for(int rows) {
  static int slots = 0;
  if (!slots) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    slots = 2 * cus;
  }
  const int nt = (rows + kR32 - 1) / kR32;
  return nt < slots ? nt : slots;
}

template <int L, int ACT>
static int launch_fwd32(const Mlp32FwdArgs& a, hipStream_t s) {
  constexpr int lds = 3 * 1024 * kBI32;
  hipLaunchKernelGGL((mlp_fwd_kernel<kBI32, kBH32, L, ACT, kR32>), dim3(grid32_for(a.rows)), dim3(512), lds, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? REPO_OK : (int)e;
}

int mlp32_fwd(int64_t rows, int64_t in_dim, int64_t hidden, int64_t out_dim, int L, const float* x, int64_t ldx,
              const float* const* params, float* const* hidden_out, float* out, int64_t ldo, void* ws,
              hipStream_t stream, int act) {
  Mlp32FwdArgs a;
  a.rows = (int)rows, a.in_dim = (int)in_dim, a.hidden = (int)hidden, a.out_dim = (int)out_dim;
  a.ldx = (int)ldx, a.ldo = (int)ldo;
  a.x = x, a.out = out;
  char* w = (char*)ws;
  a.wpack = w;
  Pack32Args pa;
  pa.njobs = 0;
  for (int l = 0; l < L; ++l) {
    const int n = l == L - 1 ? (int)out_dim : (int)hidden, k = l == 0 ? (int)in_dim : (int)hidden;
    pa.job[pa.njobs++] = Pack32Job{params[2 * l], w, n, k, k, 1, 0, nullptr};
    a.W[l] = (unsigned)(w - a.wpack);
    w += pack32_bytes(n, k);
    pa.job[pa.njobs++] = Pack32Job{params[2 * l + 1], w, n, 0, 0, 0, 1, nullptr};
    a.B[l] = (unsigned)(w - a.wpack);
    w += vec32_bytes(n);
    if (l < L - 1) a.hid[l] = hidden_out[l];
  }
  a.wbytes = (unsigned)(w - a.wpack);
  int rc = launch_pack32(pa, stream);
  if (rc) return rc;
  if (act == REPO_ACT_RELU) return L == 4 ? launch_fwd32<4, REPO_ACT_RELU>(a, stream) : launch_fwd32<5, REPO_ACT_RELU>(a, stream);
  return L == 4 ? launch_fwd32<4, REPO_ACT_ELU>(a, stream) : launch_fwd32<5, REPO_ACT_ELU>(a, stream);
}

template <int L, int ACT>
static int launch_bwd32(const Mlp32BwdArgs& a, hipStream_t s) {
  constexpr int lds = 3 * 1024 * kBH32;
  hipLaunchKernelGGL((mlp_bwd_kernel<kBI32, kBH32, L, ACT, kR32>), dim3(grid32_for(a.rows)), dim3(512), lds, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? REPO_OK : (int)e;
}

int mlp32_bwd(int64_t rows, int64_t in_dim, int64_t hidden, int64_t out_dim, int L, const float* const* params,
              const float* const* hidden_acts, const float* dout, int64_t lddout, float* const* dsave, float* dx,
              int64_t lddx, int accumulate_dx, void* ws, hipStream_t stream, int act, const float* dout_w, int64_t rows_w) {
  Mlp32BwdArgs a;
  a.dout_w = dout_w, a.rows_w = (int)rows_w, a.ldw = 1;
  if (out_dim == 1 && !dout_w) a.dout_w = dout, a.rows_w = (int)rows, a.ldw = (int)lddout;  // one upstream, both sides
  a.rows = (int)rows, a.in_dim = (int)in_dim, a.hidden = (int)hidden, a.out_dim = (int)out_dim;
  a.lddout = (int)lddout, a.lddx = (int)lddx, a.accumulate_dx = accumulate_dx;
  a.dout = dout, a.dx = dx;
  char* w = (char*)ws;
  a.wpack = w;
  Pack32Args pa;
  pa.njobs = 0;
  for (int l = (dx ? 0 : 1); l < L; ++l) {
    const int n = l == L - 1 ? (int)out_dim : (int)hidden, k = l == 0 ? (int)in_dim : (int)hidden;
    // transposed: pack column n' = k index, reduction k' = n index
    pa.job[pa.njobs++] = Pack32Job{params[2 * l], w, k, n, 1, k, 0, nullptr};
    a.W[l] = (unsigned)(w - a.wpack);
    w += pack32_bytes(k, n);
  }
  if (!dx) a.W[0] = a.W[1];  // (opened, never multiplied by)
  for (int l = 0; l < L - 1; ++l) {
    a.hid[l] = hidden_acts[l];
    a.dsave[l] = dsave ? dsave[l] : nullptr;
  }
  a.wbytes = (unsigned)(w - a.wpack);
  int rc = launch_pack32(pa, stream);
  if (rc) return rc;
  if (act == REPO_ACT_RELU) return L == 4 ? launch_bwd32<4, REPO_ACT_RELU>(a, stream) : launch_bwd32<5, REPO_ACT_RELU>(a, stream);
  return L == 4 ? launch_bwd32<4, REPO_ACT_ELU>(a, stream) : launch_bwd32<5, REPO_ACT_ELU>(a, stream);
}

}  // namespace repo
