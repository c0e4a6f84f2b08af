// Stride-2 convolution family of the reference's encoder/decoder: three passes (down, up, weight gradient) of 14 layer
// geometries over eleven engine headers.  Which engine a layer's pass takes is written down once, in the table under
// "host-side dispatch" (Layer<G>), and decided per call by down_plan / up_plan / wgrad_plan there.
//
// A layer is a (big, small) pair with big = 2*small + KS - 2 and one weight tensor w[cs][cb][ky][kx] (nn.Conv2d
// (out,in,kh,kw) for the encoder, nn.ConvTranspose2d (in,out,kh,kw) for the decoder -- the same indexing).
//   down : small[img][cs][sy][sx] = sum_{cb,ky,kx} big[img][cb][2sy+ky][2sx+kx] w[cs][cb][ky][kx]
//   up   : big[img][cb][2y+py][2x+px] = sum_{cs,jy,jx} small[img][cs][y-jy][x-jx] w[cs][cb][py+2jy][px+2jx] per output
//          parity class (py,px): only the taps that exist, no zero-stuffing
//   wgrad: dw[cs][cb][ky][kx] = sum_{img,sy,sx} small[img][cs][sy][sx] big[img][cb][2sy+ky][2sx+kx]
//          (+ the bias gradient of `small`), split over images into slabs, reduced in fixed order
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "igemm.h"
#include "dconv.h"
#include "uconv.h"
#include "dconv_up.h"
#include "bconv.h"
#include "buconv.h"
#include "bwgrad.h"
#include "bdec4.h"
#include "twgrad.h"
#include "tconv_up.h"
#include "tconv_down.h"

namespace repo {

// Test aid (repo_debug_bconv): 0 keeps every conv layer on the fp32-MFMA kernels.  Thread-local (api.hip): the setting
// of the calling host thread, read at launch time.
static thread_local int t_bconv_enabled = 1;

// Convolution precision (repo_conv_precision): REPO_CONV_PRECISION_HIGHEST forms the six products of the three-way bf16 split,
// REPO_CONV_PRECISION_HIGH the three of a two-way split (bgemm.h, BgProd).  Thread-local like the switch above; a thread that has
// not set it takes the process's REPO_CONV_PRECISION (read once).  An unknown name there is an error of every conv entry point
// (REPO_E_ENV), not a fall-back.  Read by the three plans and the repo_decoder_out_nll decision, by nothing else.
static thread_local int t_conv_precision = -1;
static int env_conv_precision() {
  static const int mode = [] {
    const char* e = getenv("REPO_CONV_PRECISION");
    if (!e || !*e || !strcmp(e, "highest")) return REPO_CONV_PRECISION_HIGHEST;
    return !strcmp(e, "high") ? REPO_CONV_PRECISION_HIGH : REPO_E_ENV;
  }();
  return mode;
}
static int conv_precision() { return t_conv_precision >= 0 ? t_conv_precision : env_conv_precision(); }
static bool conv_precision_high() { return conv_precision() == REPO_CONV_PRECISION_HIGH; }
#define REPO_CONV_PRECISION_GUARD() \
  do {                              \
    if (conv_precision() < 0) return REPO_E_ENV; \
  } while (0)

template <int CB_, int CS_, int HB_, int KS_>
struct Geo {
  static constexpr int CB = CB_, CS = CS_, HB = HB_, WB = HB_, KS = KS_;
  static constexpr int HS = (HB - KS) / 2 + 1, WS = HS;
  static constexpr int PB = HB * WB, PS = HS * WS, KK = KS * KS;
};
using GEnc1 = Geo<3, 32, 64, 4>;
using GEnc2 = Geo<32, 64, 31, 4>;
using GEnc3 = Geo<64, 128, 14, 4>;
using GEnc4 = Geo<128, 256, 6, 4>;
using GDec2 = Geo<64, 128, 13, 5>;
using GDec3 = Geo<32, 64, 30, 6>;
using GDec4 = Geo<3, 32, 64, 6>;
static_assert(GEnc1::HS == 31 && GEnc2::HS == 14 && GEnc3::HS == 6 && GEnc4::HS == 2, "encoder geometry");
static_assert(GDec2::HS == 5 && GDec3::HS == 13 && GDec4::HS == 30, "decoder geometry");
// The 128 x 128 stack (BASELINE config 4's frame size; build-defined: the reference's encoder hard-codes the 64 x 64
// flatten, encoder.py:39).  Same kernel sizes and strides, one more decoder layer (layers 7..12 of the ABI):
//   encoder  3x128x128 -> 32x63x63 -> 64x30x30 -> 128x14x14 -> 256x6x6 (k4), then a build-defined fc 9216 -> 1024
//   decoder  ... -> 32x30x30 (layers 4, 5 as at 64 x 64) -> 16x64x64 (k6) -> 3x128x128 (k2)
using GX1 = Geo<3, 32, 128, 4>;
using GX2 = Geo<32, 64, 63, 4>;
using GX3 = Geo<64, 128, 30, 4>;
using GX4 = Geo<128, 256, 14, 4>;
using GY4 = Geo<16, 32, 64, 6>;
using GY5 = Geo<3, 16, 128, 2>;
using GT4 = Geo<6, 32, 64, 6>;  // TIAObservationModel.conv4 (models/decoder.py:165): 32 -> 6 = [recon | mask]
static_assert(GX1::HS == 63 && GX2::HS == 30 && GX3::HS == 14 && GX4::HS == 6 && GY4::HS == 30 && GY5::HS == 64,
              "128 x 128 geometry");

__device__ __forceinline__ float epi_apply(float v, int epi, const float* bias, int ch, const float* aux, int o) {
  if (bias) v += bias[ch];
  if (epi == REPO_EPI_RELU) v = fmaxf(v, 0.f);
  else if (epi == REPO_EPI_MUL_DRELU) v = aux[o] > 0.f ? v : 0.f;
  return v;
}

// Compile-time k -> address-offset tables (one per geometry), read with scalar loads: inside the K
// loop k is wave-uniform for the n-major operands, so the (channel, ky, kx) decode -- ~10 scalar ALU
// instructions per element when done with div/mod by constants -- becomes one s_load per element.
template <class G, int JY, int JX>
struct UpKTab {
  int off[G::CS * JY * JX];
  int sh[G::CS * JY * JX];
  constexpr UpKTab() : off(), sh() {
    for (int k = 0; k < G::CS * JY * JX; ++k) {
      const int cs = k / (JY * JX), r = k % (JY * JX);
      const int jy = r / JX, jx = r % JX;
      off[k] = cs * G::PS - jy * G::WS - jx;
      sh[k] = jy | ((4 + jx) << 8);
    }
  }
};
template <class G, int JY, int JX>
__device__ const UpKTab<G, JY, JX> g_up_ktab{};

// ------------------------------------------------------------------------------- down
template <class G, class TgtT, int MODE>
struct ConvUpMergedOp {
  static constexpr bool A_KMAJOR = true, B_KMAJOR = false;
  static constexpr int NY = (G::HB + 1) / 2, NX = (G::WB + 1) / 2;
  static constexpr int J = (G::KS + 1) / 2, JJ = J * J;
  const float* small;
  const float* w;
  const float* bias;
  const float* aux;
  float* out;  // MODE 0: output; MODE 1: recon (nullable)
  int nimg, epi;
  // MODE 1
  const TgtT* target;
  float* dpre;       // nullable
  float* partials;   // one per workgroup
  float grad_scale;
  float lsum;

  struct AM {
    int off;
    int py, px;
  };
  struct AK {
    int off;
    int jy2, jx2;  // 2*jy, 2*jx
  };
  struct BN {
    int off;
    unsigned mask;
  };
  struct BK {
    int off;
    int sh;
  };
  __device__ void init(int) { lsum = 0.f; }
  __device__ int M() const { return 4 * G::CB; }
  __device__ int N() const { return nimg * NY * NX; }
  __device__ int kbeg() const { return 0; }
  __device__ int kend() const { return G::CS * JJ; }
  // M index = (py, cb, px) with px fastest: two consecutive accumulator registers of a lane are the
  // two horizontally adjacent output pixels, so the epilogue stores them as one 8-byte word and a
  // wave writes whole 256-byte runs (the separate px classes wrote every line twice, half each:
  // WRITE_SIZE was 2.0x the tensor).
  __device__ AM a_m(int m) const {
    const int py = m / (2 * G::CB), rem = m % (2 * G::CB);
    const int cb = rem >> 1, px = rem & 1;
    return AM{cb * G::KK + py * G::KS + px, py, px};
  }
  __device__ AK a_k(int k) const {
    const int cs = k / JJ, r = k % JJ;
    const int jy2 = 2 * (r / J), jx2 = 2 * (r % J);
    return AK{cs * (G::CB * G::KK) + jy2 * G::KS + jx2, jy2, jx2};
  }
  __device__ float a(const AM& m, const AK& k) const {
    const bool ok = (m.py + k.jy2 < G::KS) && (m.px + k.jx2 < G::KS);
    const float v = w[(unsigned)(ok ? m.off + k.off : 0)];
    return ok ? v : 0.f;
  }
  __device__ BN b_n(int n) const {
    const int img = n / (NY * NX), q = n % (NY * NX);
    const int y = q / NX, x = q % NX;
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mask |= ((y - j >= 0 && y - j < G::HS) ? 1u : 0u) << j;
      mask |= ((x - j >= 0 && x - j < G::WS) ? 1u : 0u) << (4 + j);
    }
    return BN{(img * G::CS * G::HS + y) * G::WS + x, mask};
  }
  __device__ BK b_k(int k) const { return BK{g_up_ktab<G, J, J>.off[k], g_up_ktab<G, J, J>.sh[k]}; }
  __device__ float b(const BK& k, const BN& n) const {
    const bool ok = ((n.mask >> (k.sh & 0xff)) & (n.mask >> (k.sh >> 8)) & 1u) != 0;
    const float v = small[(unsigned)(ok ? n.off + k.off : 0)];
    return ok ? v : 0.f;
  }
  __device__ void store_col(int mb, int n, const f32x16& acc, int M) {
    const int img = n / (NY * NX), q = n % (NY * NX);
    const int y2 = 2 * (q / NX), x2 = 2 * (q % NX);
    const int obase = img * G::CB * G::PB;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const int m = mb + (r & 3) + 8 * (r >> 2);  // even: px = 0; register r+1 is px = 1
      if (m < M) {
        const int py = m / (2 * G::CB), cb = (m % (2 * G::CB)) >> 1;
        const int by = y2 + py;
        if (by < G::HB && x2 < G::WB) {
          const int o = obase + (cb * G::HB + by) * G::WB + x2;
          const bool two = x2 + 1 < G::WB;
          float v0 = acc[r], v1 = acc[r + 1];
          if (MODE == 0) {
            v0 = epi_apply(v0, epi, bias, cb, aux, o);
            if (two) v1 = epi_apply(v1, epi, bias, cb, aux, o + 1);
          } else {
            const float bv = bias ? bias[cb] : 0.f;
            v0 += bv;
            v1 += bv;
            const float d0 = v0 - load_as_float(target, (unsigned)o);
            const float d1 = two ? v1 - load_as_float(target, (unsigned)(o + 1)) : 0.f;
            lsum += 0.5f * (d0 * d0 + d1 * d1);
            if (dpre) {
              if (G::WB % 2 == 0) {
                *reinterpret_cast<float2*>(dpre + o) = make_float2(d0 * grad_scale, d1 * grad_scale);
              } else {
                dpre[o] = d0 * grad_scale;
                if (two) dpre[o + 1] = d1 * grad_scale;
              }
            }
          }
          if (out) {
            if (G::WB % 2 == 0) {
              *reinterpret_cast<float2*>(out + o) = make_float2(v0, v1);
            } else {
              out[o] = v0;
              if (two) out[o + 1] = v1;
            }
          }
        }
      }
    }
  }
  __device__ void finish() {
    if (MODE == 1) {
      __shared__ float red[16];
      const float s = block_sum(lsum, red);
      if (threadIdx.x == 0)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
    }
  }
};

// ------------------------------------------------------------------------------- wgrad
__global__ void conv_slab_reduce_kernel(const float* __restrict__ slab, int splits, int Mrows, int Ncols,
                                        float* __restrict__ dw, float* __restrict__ db, int accumulate) {
  const int total = Mrows * (Ncols + 1);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int m = i / (Ncols + 1), n = i % (Ncols + 1);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;  // fixed-order independent chains
    int z = 0;
    for (; z + 4 <= splits; z += 4) {
      s0 += slab[(size_t)z * total + i];
      s1 += slab[(size_t)(z + 1) * total + i];
      s2 += slab[(size_t)(z + 2) * total + i];
      s3 += slab[(size_t)(z + 3) * total + i];
    }
    for (; z < splits; ++z) s0 += slab[(size_t)z * total + i];
    const float s = (s0 + s1) + (s2 + s3);
    if (n < Ncols) {
      float* p = dw + (size_t)m * Ncols + n;
      *p = accumulate ? *p + s : s;
    } else if (db) {
      db[m] = accumulate ? db[m] + s : s;
    }
  }
}

// Many splits, few outputs (the 3-channel layers: 613 slabs of 32 x 49): a workgroup of 1024 threads owns 64 consecutive
// outputs; thread (o, g) adds slabs g, g + 16, ... of output o -- the 64 lanes of a wave read 256 contiguous bytes of
// one slab, four loads in flight per thread -- and the 16 partial sums of an output meet in LDS in a fixed order
// (bit-reproducible).  (Round 4's one-wave-per-output form read 64 different slabs per load instruction, one cache line
// each: 70-80 us inside the update for 3.8 MB of slabs.)
// SLAB_REDUCE_WAVES waves per workgroup walk the 16 slab groups (16: the round-4 form, one group per wave; 4: each wave takes
// four groups in turn -- the same 16 partial sums in the same order, bit for bit, from a 256-thread workgroup that finds a
// place on a busy chip; a 1024-thread workgroup needs a CU with 16 free wave slots, and inside the update these launches
// waited for one: 78-135 us each in the trace against ~15 us alone).
#ifndef SLAB_REDUCE_WAVES
#define SLAB_REDUCE_WAVES 4
#endif
__global__ __launch_bounds__(64 * SLAB_REDUCE_WAVES) void conv_slab_reduce_wave_kernel(const float* __restrict__ slab, int splits, int Mrows,
                                                                     int Ncols, float* __restrict__ dw,
                                                                     float* __restrict__ db, int accumulate, int tkk,
                                                                     int tcb, float* __restrict__ dbig) {
  // tkk > 0: the slabs are twgrad.h's [tap][row][channel] (+ db[row] at the end) instead of [row][channel * tkk + tap | db]
  // and, behind them, the two row-parity halves of the channel sums of `big` (2 x tcb: one aligned block of 64 outputs)
  __shared__ float red[16][64];
  const int total = Mrows * (Ncols + 1) + (tkk > 0 ? 2 * tcb : 0);
  const int o = threadIdx.x & 63, gw = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + o;
  for (int g = gw; g < 16; g += SLAB_REDUCE_WAVES) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (i < total) {
      int z = g;
      for (; z + 48 < splits; z += 64) {
        s0 += slab[(size_t)z * total + i];
        s1 += slab[(size_t)(z + 16) * total + i];
        s2 += slab[(size_t)(z + 32) * total + i];
        s3 += slab[(size_t)(z + 48) * total + i];
      }
      for (; z < splits; z += 16) s0 += slab[(size_t)z * total + i];
    }
    red[g][o] = (s0 + s1) + (s2 + s3);
  }
  __syncthreads();
  const int g = gw;
  if (g == 0 && i < total) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += red[q][o];
    int m = i / (Ncols + 1), n = i % (Ncols + 1);
    if (tkk > 0) {
      const int body = Mrows * Ncols;
      if (i >= body + Mrows) {   // channel sums of `big`: output c = half 0 + half 1 (both in this block's `red`)
        const int c = i - body - Mrows;
        if (dbig && c < tcb) {
          float s2 = 0.f;
#pragma unroll
          for (int q = 0; q < 16; ++q) s2 += red[q][o + tcb];
          dbig[c] = accumulate ? dbig[c] + (s + s2) : s + s2;
        }
        return;
      }
      if (i < body) m = (i / tcb) % Mrows, n = (i % tcb) * tkk + i / (tcb * Mrows);
      else m = i - body, n = Ncols;
    }
    if (n < Ncols) {
      float* p = dw + (size_t)m * Ncols + n;
      *p = accumulate ? *p + s : s;
    } else if (db) {
      db[m] = accumulate ? db[m] + s : s;
    }
  }
}

// out[c] (+)= scale * sum of parts[c][0 .. n): one workgroup per c
__global__ void partial_sum_rows_kernel(const float* __restrict__ parts, int n, float* __restrict__ out, float scale,
                                        int accumulate) {
  __shared__ float red[16];
  const float* row = parts + (size_t)blockIdx.x * n;
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += row[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = accumulate ? out[blockIdx.x] + scale * s : scale * s;
}

__global__ void partial_sum_kernel(const float* __restrict__ parts, int n, float* __restrict__ out, int accumulate) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += parts[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) *out = accumulate ? *out + s : s;
}

// x[n][c][p] -> partial[s][c] over image chunk s.  Threads walk the flattened (image, pixel) index of
// the chunk with an incremental (img, p) carry, so small planes (P = 25, 169) keep all lanes busy.
__global__ void channel_sum_kernel(const float* __restrict__ x, int nimg, int C, int P, int imgs_per_split,
                                   float* __restrict__ parts) {
  __shared__ float red[16];
  const int c = blockIdx.x, s = blockIdx.y;
  const int i0 = s * imgs_per_split, i1 = min(nimg, i0 + imgs_per_split);
  const int nt = blockDim.x;
  const int dq = nt / P, dr = nt % P;
  int img = i0 + (int)threadIdx.x / P, p = (int)threadIdx.x % P;
  float a0 = 0.f, a1 = 0.f;
  const size_t cstride = (size_t)C * P;
  const float* base = x + (size_t)c * P;
  while (img < i1) {
    a0 += base[img * cstride + p];
    p += dr;
    img += dq;
    if (p >= P) {
      p -= P;
      ++img;
    }
    if (img >= i1) break;
    a1 += base[img * cstride + p];
    p += dr;
    img += dq;
    if (p >= P) {
      p -= P;
      ++img;
    }
  }
  const float acc = block_sum(a0 + a1, red);
  if (threadIdx.x == 0) parts[s * C + c] = acc;
}
// one wave per channel: lanes stride over the splits, fixed-order shuffle reduction (bit-reproducible)
__global__ void channel_sum_final_kernel(const float* __restrict__ parts, int splits, int C, float* __restrict__ out,
                                         int accumulate) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= C) return;
  float s = 0.f;
  for (int z = lane; z < splits; z += 64) s += parts[z * C + c];
  s = wave_sum(s);
  if (lane == 0) out[c] = accumulate ? out[c] + s : s;
}

__global__ void relu_mask_kernel(int64_t n, const float* __restrict__ dy, const float* __restrict__ h,
                                 float* __restrict__ y) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = h[i] > 0.f ? dy[i] : 0.f;
}

// ------------------------------------------------------------------------------- host-side dispatch
// What is chosen per LAYER is one table entry, Layer<G> below.  What is chosen per CALL is one plan per pass (down_plan,
// up_plan, wgrad_plan): a plain struct computed from the run-time arguments, which the workspace-size query, the pack and
// the launcher all consume.  Moving a layer's pass to another engine = editing its entry; nothing else derives a tile
// count, a pack size or a workspace offset.
struct Off {};   // "not on this engine"
template <class T> constexpr bool kOn = !std::is_same<T, Off>::value;

// Every layer has the fp32-MFMA kernels of dconv.h: the down pass's throughput tile DTile <BM, BN, CK, WM, WN>, the weight
// gradient's WTile <BM, BN, WM, WN, images per chunk, small rows per chunk> and WGT, the workgroups its split-K over image
// groups aims at.  The other engines are off unless the entry names them.
template <class Down_, class Wgrad_, int WGT_>
struct LayerFp32 {
  using Down = Down_; using Wgrad = Wgrad_; static constexpr int WGT = WGT_;
  // -- down.  A handful of frames (the acting path encodes ONE per environment step): the throughput tiles leave 1-2
  // workgroups walking 16-64 dependent channel chunks (enc4: 147 us for one frame).  Latency tiles (nimg * PS <= 512) use 32
  // output channels per workgroup (4-8x more workgroups) and 4x larger channel chunks (4x fewer barriers).  Off = `Down`.
  using DownLat = Off;
  // bconv.h (bf16x6) for the MFMA-bound geometries with an even big-row pitch; the 3-channel layers are bandwidth bound ...
  using DownBf = Off;
  // ... but for uint8 frames (the encoder's first layer as train_agent() feeds it): the bytes are exact in ONE bf16, so the
  // product needs three MFMAs per block instead of six and no split of the activation (bconv.h, U8)
  using DownBfU8 = Off;
  // tconv_down.h (staging waves beside multiplying waves): its geometry.  It takes a call of the bf16x6 kernel's, and its
  // pack that kernel's place, if nimg >= 32, no channel sums are wanted and down_tcd_takes(epi, has_bias, wants_cmask).
  using DownTcd = Off;
  static bool down_tcd_takes(int, bool, bool) { return false; }
  // -- up: with none of these, the merged gather engine (igemm.h, ConvUpMergedOp)
  using UpScatter = Off;   // uconv.h: SConf <images per workgroup, resident N tiles>
  // buconv.h, the scatter kernel in bf16x6 (the decoder's conv3 forward is the update's largest launch).  The weight pack's
  // format follows the kernel: repo_debug_bconv toggles both, a pack written under one setting is void under the other.
  using UpBfScatter = Off;
  // dconv_up.h (direct, register-accumulating): its tile, instead of a scatter configuration.  A/B on one box (round 3, us):
  //   enc2@128 data gradient  gather engine 1634 -> direct 1243 (8 waves; 4 waves 1424)
  //   dec4@128 forward        gather engine  717 -> direct  535
  //   TIA conv4 forward       gather engine  775 -> direct  434
  //   enc2 data gradient      scatter        425 vs direct  606 (its K loop alone runs 424, staging +76, epilogue
  //                           +106; staggered starts, 16-byte-aligned stores and prefetching the ReLU operand under
  //                           the last chunk's MFMAs each changed nothing): the scatter kernel stays
  using DirectUp = Off;
  // tconv_up.h (gather form): takes the encoder backward's epilogues at nimg >= 4; its pack sits behind the scatter kernels'
  static constexpr bool UpTconv = false;
  // -- weight gradient
  // bwgrad.h (bf16x6, on the fp32 kernel's split-K) for the layers whose bands fill whole 16-k blocks reasonably (enc4's
  // 2 x 2 planes would run 4 real k in a block of 16; the 3-channel layers are not MFMA-bound).  Measured and left on the fp32
  // kernel: enc2 (31 x 31 planes: 343-445 us against 320) and dec2 (232-244 against 247) -- with one or two waves per SIMD the
  // in-register split of the B fragments (44 dependent vector instructions per 8 elements) is not hidden behind 12 MFMAs
  using WgradBf = Off;
  // twgrad.h (both operands split at staging, `big` read through the LDS's transposing load): k-blocks per chunk, 0 = not
  // on this engine; staging waves: 8 where the multiplying waves (4 taps: 64 accumulator registers) fit three waves per
  // SIMD.  A PAIR of workgroups (the two row parities of the taps) owns the whole dw of its images: images per split =
  // ceil(nimg / 128), one slab per pair.  TwDbig: the channel sums of `big` ride along where the taps cover it.
  static constexpr int TwNBK = 0, TwNPW = 4;
  static constexpr bool TwDbig = true;
};

template <class G> struct Layer;
// WGT: sweep of 768 / 1024 / 1536 / 2048 / 3072 on one box, round 3: enc2 371 -> 335 us at 768, enc3 239 -> 226 at 1024,
// dec3 542 -> 531 at 2048; fewer splits also mean smaller slabs to reduce.
// The 3-channel layers are one channel chunk per workgroup (no pipelining inside it): 8 waves per tile and short
// weight-gradient bands measured best (tile sweep, round 2: enc1 fwd 148 -> 140 us, enc1 wgrad 224 -> 171,
// dec4 dgrad 311-338 -> 247, dec4 wgrad 210 -> 201)
template <> struct Layer<GEnc1> : LayerFp32<DTile<32, 512, 3, 1, 8>, WTile<32, 64, 1, 2, 1, 4, 2>, 3072> {
  using DownBfU8 = BTile<32, 512, 4, 1, 8>;
};
template <> struct Layer<GEnc2> : LayerFp32<DTile<64, 128, 2, 2, 2>, WTile<64, 128, 2, 2, 1, 7, 2>, 768> {
  using DownLat = DTile<32, 128, 4, 1, 4>;
  // 31 x 31 planes, k4: with the element-wise staging of its padded pitch it measured equal on both kernels (312 vs 309 us,
  // round 4); staged by LDS quads (bconv.h, QROW) it is on the bf16 pipe
  using DownBf = BTile<64, 256, 4, 1, 4>;
  // its forward (ReLU) runs on tconv_down.h since round 6 (242 -> 203 us alone, results within 3e-6 of fp64, masks identical
  // to the fp32 engine's on random data).  Round 5 built it and left it un-routed: on the TIA oracle test's frames its 5e-7
  // differences flip ONE ReLU decision of conv3 at a pre-activation 5e-7 from zero, and that pixel alone takes the encoder's
  // gradient 5e-3 from the oracle's -- the test now hands the oracle the kernels' decision inside a 1e-5 band around zero
  // (tests/test_tia_gpu.py, _TIE_BAND).
  using DownTcd = TcdGeoE2;
  static bool down_tcd_takes(int epi, bool, bool) { return epi == REPO_EPI_RELU; }
  using UpScatter = SConf<GEnc2, 1, 8>;
  using UpBfScatter = BSConf<GEnc2, 1, 4>;
  static constexpr bool UpTconv = true;
  static constexpr int TwNBK = 2, TwNPW = 8;
};
template <> struct Layer<GEnc3> : LayerFp32<DTile<128, 128, 2, 2, 2>, WTile<64, 128, 2, 2, 2, 6>, 1024> {
  using DownLat = DTile<32, 128, 8, 1, 4>;
  // enc3 / enc4: ONE M tile per workgroup (the patch is staged and split once): 169 -> 146 us, 112 -> 101 (round 5)
  using DownBf = BTile<128, 128, 4, 2, 2>;
  using UpScatter = SConf<GEnc3, 4, 2>;
  using UpBfScatter = BSConf<GEnc3, 4, 4>;      // CS = 128: two K-slices
  using WgradBf = WTile<64, 256, 1, 4, 1, 6>;   // 215 -> 172-182 us
};
// enc4 forward has only 9800 output pixels: 128 x 128 tiles are 154 workgroups on 256 CUs (171 us); 32 x 64: 125 us
template <> struct Layer<GEnc4> : LayerFp32<DTile<32, 64, 2, 1, 2>, WTile<64, 128, 2, 2, 8, 2>, 768> {
  using DownLat = DTile<32, 128, 8, 1, 4>;
  using DownBf = BTile<128, 64, 4, 2, 2>;
  using UpScatter = SConf<GEnc4, 8, 1>;
  using UpBfScatter = BSConf<GEnc4, 8, 2>;   // CS = 256: four
};
// (dec2 down: 8 waves, 306 -> 274 us, A/B on one box)
template <> struct Layer<GDec2> : LayerFp32<DTile<128, 128, 4, 2, 4, 1>, WTile<64, 128, 2, 2, 4, 5>, 1536> {
  using DownBf = BTile<64, 128, 2, 1, 4>;    // 13 x 13 planes, k5 (32 slots for 25 taps)
  using UpScatter = SConf<GDec2, 5, 2>;
  using UpBfScatter = BSConf<GDec2, 5, 4>;   // CS = 128, k5: per-class tap sets
};
template <> struct Layer<GDec3> : LayerFp32<DTile<64, 128, 2, 2, 2>, WTile<64, 128, 2, 2, 1, 7>, 2048> {
  using DownBf = BTile<64, 256, 2, 1, 4>;
  using DownTcd = TcdGeo;   // its data gradient: plain or times the ReLU derivative, nothing else
  static bool down_tcd_takes(int epi, bool has_bias, bool wants_cmask) {
    return (epi == REPO_EPI_NONE || epi == REPO_EPI_MUL_DRELU) && !has_bias && !wants_cmask;
  }
  using UpScatter = SConf<GDec3, 1, 6>;
  using UpBfScatter = BSConf<GDec3, 1, 4>;
  using WgradBf = WTile<64, 128, 1, 4, 1, 7>;   // 531 -> 465 us (64 x 64 wave tiles: 551)
  static constexpr int TwNBK = 2;
};
template <> struct Layer<GDec4> : LayerFp32<DTile<32, 256, 3, 1, 8>, WTile<32, 128, 1, 4, 1, 2>, 1536> {};
// 128 x 128 stack: tiles by analogy with the 64 x 64 layer of the same role (not swept).  Up: the parity-class planes of a
// 16-channel group must fit LDS (<= 80 KB: two workgroups per CU), which 30 x 30 and 14 x 14 outputs do; 63 x 63 / 64 x 64
// / 128 x 128 outputs (262 KB) take the direct kernel or the gather engine.
// (GX1's weight gradient walks 2-row bands: with 4 rows of 63 pixels the 126 k-pairs of a band exceed what the
// compiler unrolls, the chunk-ahead loads then index their registers at run time: 1935 us instead of ~400)
template <> struct Layer<GX1> : LayerFp32<DTile<32, 512, 3, 1, 8>, WTile<32, 64, 1, 2, 1, 2, 2>, 3072> {};
template <> struct Layer<GX2> : LayerFp32<DTile<64, 128, 2, 2, 2>, WTile<64, 128, 2, 2, 1, 3, 2>, 1536> {
  using DirectUp = DTile<128, 128, 8, 2, 4>;
};
template <> struct Layer<GX3> : LayerFp32<DTile<128, 128, 2, 2, 2>, WTile<64, 128, 2, 2, 1, 7>, 1024> {
  using UpScatter = SConf<GX3, 1, 2>;
};
template <> struct Layer<GX4> : LayerFp32<DTile<64, 128, 2, 2, 2>, WTile<64, 128, 2, 2, 2, 6>, 1024> {
  using UpScatter = SConf<GX4, 4, 1>;
};
template <> struct Layer<GY4> : LayerFp32<DTile<32, 256, 2, 1, 4>, WTile<32, 128, 1, 4, 1, 2>, 1536> {
  using DirectUp = DTile<64, 256, 4, 2, 4>;
};
template <> struct Layer<GY5> : LayerFp32<DTile<32, 512, 3, 1, 8>, WTile<32, 64, 1, 2, 1, 2>, 1536> {};
template <> struct Layer<GT4> : LayerFp32<DTile<32, 256, 3, 1, 8>, WTile<32, 128, 1, 4, 1, 2>, 1536> {
  using DirectUp = DTile<32, 256, 4, 1, 8>;
};

// What the plans read: the table entry under the A/B builds' overrides (tools/build_variant.sh).  -DTCD_DISABLE: bconv.h
// instead of tconv_down.h, -DTCD_NO_ENC2: for encoder conv2 only; -DTCU_DISABLE: the scatter kernel instead of tconv_up.h;
// -DTW_DISABLE: the previous weight-gradient engines instead of twgrad.h; -DTW_NO_DBIG: the separate channel-sum pass.
template <class G> struct Route : Layer<G> {
#if defined(TCD_DISABLE)
  using DownTcd = Off;
#elif defined(TCD_NO_ENC2)
  using DownTcd = std::conditional_t<std::is_same<G, GEnc2>::value, Off, typename Layer<G>::DownTcd>;
#endif
#ifdef TCU_DISABLE
  static constexpr bool UpTconv = false;
#endif
#ifdef TW_DISABLE
  static constexpr int TwNBK = 0;
#endif
#ifdef TW_NO_DBIG
  static constexpr bool TwDbig = false;
#endif
};
template <class G> using DownLatTile = std::conditional_t<kOn<typename Route<G>::DownLat>, typename Route<G>::DownLat, typename Route<G>::Down>;
template <class G, class BigT> using DownBfTile = std::conditional_t<std::is_same<BigT, float>::value, typename Route<G>::DownBf, typename Route<G>::DownBfU8>;

constexpr size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- down.  Workspace: [weight pack of the bf16x6 kernel | channel-sum partials]; without room for the pack the layer
// runs on the fp32-MFMA kernel (ws stays optional for callers that want no dbias).  Test aid repo_debug_bconv(0) keeps
// every layer on the fp32 kernel.
enum class DownEngine { Fp32Lat, Fp32, Bf16, Tcd };
struct DownPlan {
  DownEngine engine;
  long tiles;          // pixel tiles of the engine's grid = rows of the channel-sum partials (repo_conv_down's dbias)
  size_t pack_bytes;   // the weight pack at the head of the workspace = offset of the partials
  size_t parts_bytes;  // 0 unless the channel sums are wanted
  bool high;           // repo_conv_precision: the bf16 engines' three-product instantiation (two against uint8 frames)
  size_t need() const { return pack_bytes + parts_bytes; }
};
template <class G, class BigT>
static DownPlan down_plan(int64_t nimg, int epi, bool has_bias, bool wants_dbias, bool wants_cmask, size_t ws_have) {
  using R = Route<G>;
  using BT = DownBfTile<G, BigT>;
  const long px = nimg * (long)G::PS;
  auto plan = [&](DownEngine e, long bn, size_t pack) {
    const long tiles = (px + bn - 1) / bn;
    return DownPlan{e, tiles, pack, wants_dbias ? (size_t)tiles * G::CS * sizeof(float) : 0, conv_precision_high()};
  };
  if constexpr (kOn<BT>) {
    if (t_bconv_enabled && px > 512) {
      using P = BPack<G, BT>;
      constexpr size_t pack = round256(std::is_same<BigT, float>::value ? P::BYTES : P::BYTES_U8);
      DownPlan b = plan(DownEngine::Bf16, BT::BN, pack);
      if constexpr (kOn<typename R::DownTcd>) {
        static_assert(std::is_same<BigT, float>::value && R::DownTcd::PACK_BYTES <= pack,
                      "tconv_down: float frames; its pack fits the room of the bf16x6 kernel's");
        if (nimg >= 32 && !wants_dbias && R::down_tcd_takes(epi, has_bias, wants_cmask)) b.engine = DownEngine::Tcd;
      }
      if (ws_have >= b.need()) return b;
    }
  }
  return px <= 512 ? plan(DownEngine::Fp32Lat, DownLatTile<G>::BN, 0) : plan(DownEngine::Fp32, R::Down::BN, 0);
}
// (the frame type is not known to the size query: the larger pack and the larger partials of the float / uint8 plans)
template <class G>
static size_t conv_down_ws_bytes(int64_t nimg) {
  const DownPlan f = down_plan<G, float>(nimg, REPO_EPI_NONE, false, true, false, SIZE_MAX);
  const DownPlan u = down_plan<G, uint8_t>(nimg, REPO_EPI_NONE, false, true, false, SIZE_MAX);
  return std::max(f.pack_bytes, u.pack_bytes) + std::max(f.parts_bytes, u.parts_bytes);
}

template <class G, class BigT>
static int conv_down_t(int64_t nimg, const BigT* big, const float* w, const float* bias, float* small, int epi,
                       const float* aux, float* dbias, int accumulate_dbias, unsigned char* cmask, void* ws,
                       size_t ws_bytes, hipStream_t s) {
  if (cmask && G::CS % 4 != 0) return REPO_E_BADARG;
  if (nimg * (int64_t)G::CB * G::PB >= kMaxBufElems || nimg * (int64_t)G::CS * G::PS >= kMaxBufElems) return REPO_E_SHAPE;
  const size_t ws_have = ws ? ws_bytes : 0;
  const DownPlan p = down_plan<G, BigT>(nimg, epi, bias != nullptr, dbias != nullptr, cmask != nullptr, ws_have);
  if (ws_have < p.need()) return REPO_E_WS_TOO_SMALL;
  float* parts = dbias ? (float*)((char*)ws + p.pack_bytes) : nullptr;
  DownArgs a{big, w, bias, aux, small, (int)nimg, epi, (unsigned)(nimg * G::CB * G::PB * sizeof(BigT)),
             (unsigned)(G::CS * G::CB * G::KK * sizeof(float)), parts, cmask};
  int rc = REPO_E_BADARG;
  switch (p.engine) {
    case DownEngine::Tcd:
      if constexpr (kOn<typename Route<G>::DownTcd>)
        rc = p.high ? launch_tconv_down<typename Route<G>::DownTcd, 3>(a, w, (char*)ws, s)
                    : launch_tconv_down<typename Route<G>::DownTcd, 6>(a, w, (char*)ws, s);
      break;
    case DownEngine::Bf16:
      if constexpr (kOn<DownBfTile<G, BigT>>) {
        constexpr int NFULL = std::is_same<BigT, float>::value ? 6 : 3;   // uint8 frames are exact in one bf16
        rc = p.high ? launch_bconv_down<G, DownBfTile<G, BigT>, BigT, NFULL == 6 ? 3 : 2>(a, w, (char*)ws, s)
                    : launch_bconv_down<G, DownBfTile<G, BigT>, BigT, NFULL>(a, w, (char*)ws, s);
      }
      break;
    case DownEngine::Fp32Lat: rc = launch_dconv_down<G, BigT, DownLatTile<G>>(a, s); break;
    case DownEngine::Fp32: rc = launch_dconv_down<G, BigT, typename Route<G>::Down>(a, s); break;
  }
  if (rc || !dbias) return rc;
  hipLaunchKernelGGL(channel_sum_final_kernel, dim3(cdiv(G::CS, 4)), dim3(256), 0, s, (const float*)parts, (int)p.tiles,
                     (int)G::CS, dbias, accumulate_dbias);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

// ---- up.  Workspace: [weight pack of the layer's scatter / direct kernel (room for either form of the scatter kernel: the
// debug switch is thread-local) | pack of the gather-form kernel]; the merged gather engine reads the native weights.
enum class UpEngine { Tconv, BfScatter, Direct, Scatter, Merged };
struct UpPlan {
  UpEngine engine;   // this call's
  UpEngine base;     // the layer's where the gather-form kernel does not take the call: whose pack sits at offset 0
  bool tcu_live;     // the gather-form kernel is in use (under the current debug switch): packing ahead writes its pack too
  size_t tcu_off;    // ... at this offset
  size_t need;       // bytes this call's engine reads
  size_t total;      // bytes of the layer's packs together (repo_conv_up_workspace_bytes)
  bool high;         // repo_conv_precision: the bf16 engines' three-product instantiation (the packs are the same)
};
template <class G>
static UpPlan up_plan(int64_t nimg, int epi, size_t ws_have) {
  using R = Route<G>;
  using UC = typename R::UpScatter;
  using BC = typename R::UpBfScatter;
  static_assert(!kOn<BC> || kOn<UC>, "the bf16x6 scatter kernel has an fp32 twin (repo_debug_bconv(0))");
  static_assert(!kOn<typename R::DirectUp> || !kOn<UC>, "the direct kernel or the scatter kernels");
  static_assert(!R::UpTconv || kOn<BC>, "the gather-form kernel follows the debug switch of the bf16x6 kernels");
  UpPlan p{UpEngine::Merged, UpEngine::Merged, false, 0, 0, 0, conv_precision_high()};
  size_t room = 0;
  if constexpr (kOn<BC>) {
    p.base = t_bconv_enabled ? UpEngine::BfScatter : UpEngine::Scatter;
    p.need = t_bconv_enabled ? BC::PACK_BYTES : UC::PACK_FLOATS * sizeof(float);
    room = std::max(BC::PACK_BYTES, UC::PACK_FLOATS * sizeof(float));
  } else if constexpr (kOn<typename R::DirectUp>) {
    p.base = UpEngine::Direct, p.need = room = UpGeo<G>::PACK_FLOATS * sizeof(float);
  } else if constexpr (kOn<UC>) {
    p.base = UpEngine::Scatter, p.need = room = UC::PACK_FLOATS * sizeof(float);
  }
  p.engine = p.base;
  p.tcu_off = round256(room);
  p.total = R::UpTconv ? p.tcu_off + kTcuPackBytes : room;
  p.tcu_live = R::UpTconv && t_bconv_enabled;
  // the encoder backward's epilogues; ReLU / FiLM: the scatter kernel
  const bool epi_ok = epi == REPO_EPI_NONE || epi == REPO_EPI_MUL_DRELU || epi == REPO_EPI_MUL_CMASK;
  if (p.tcu_live && epi_ok && nimg >= 4 && ws_have >= p.total) {
    p.engine = UpEngine::Tconv;
    p.need = p.total;
  }
  return p;
}

template <class G>
static int conv_up_pack_t(const float* w, void* ws, size_t ws_bytes, hipStream_t s) {
  using R = Route<G>;
  const size_t ws_have = ws ? ws_bytes : 0;
  const UpPlan p = up_plan<G>(0, REPO_EPI_NONE, ws_have);
  if (ws_have < (p.tcu_live ? p.total : p.need)) return REPO_E_WS_TOO_SMALL;
  if (p.tcu_live)   // both packs: which kernel a later call takes depends on its epilogue and batch
    if (const int rc = launch_tconv_up_pack(w, (char*)ws + p.tcu_off, s)) return rc;
  if constexpr (kOn<typename R::UpBfScatter>)
    if (p.base == UpEngine::BfScatter) return launch_buconv_pack<G, typename R::UpBfScatter>(w, ws, ws_bytes, s);
  if constexpr (kOn<typename R::DirectUp>) return launch_dconv_up_pack<G>(w, ws, ws_bytes, s);
  else if constexpr (kOn<typename R::UpScatter>) return launch_uconv_pack<G, typename R::UpScatter>(w, ws, ws_bytes, s);
  else return REPO_OK;  // the merged gather engine reads the native weights
}

template <class G>
static int conv_up_t(int64_t nimg, const float* small, const float* w, const float* bias, float* big, int epi,
                     const float* aux, int packed, void* ws, size_t ws_bytes, hipStream_t s) {
  if (nimg * (int64_t)G::CB * G::PB >= kMaxBufElems || nimg * (int64_t)G::CS * G::PS >= kMaxBufElems) return REPO_E_SHAPE;
  using R = Route<G>;
  // the channel-quad mask and FiLM are what the scatter kernels' drains read (a pixel's four channels per item)
  if (epi == REPO_EPI_MUL_CMASK && (!kOn<typename R::UpScatter> || G::CB % 4 != 0)) return REPO_E_BADARG;
  if (epi == REPO_EPI_FILM_RELU && !kOn<typename R::UpScatter>) return REPO_E_BADARG;
  const size_t ws_have = ws ? ws_bytes : 0;
  const UpPlan p = up_plan<G>(nimg, epi, ws_have);
  if (ws_have < p.need) return REPO_E_WS_TOO_SMALL;
  if constexpr (R::UpTconv)
    if (p.engine == UpEngine::Tconv) {
      char* pack = (char*)ws + p.tcu_off;
      if (!packed)
        if (const int rc = launch_tconv_up_pack(w, pack, s)) return rc;
      return p.high ? launch_tconv_up<3>(small, pack, bias, aux, big, nimg, epi, s)
                    : launch_tconv_up<6>(small, pack, bias, aux, big, nimg, epi, s);
    }
  if constexpr (kOn<typename R::UpBfScatter>)
    if (p.engine == UpEngine::BfScatter)
      return p.high ? launch_buconv_scatter<G, typename R::UpBfScatter, 3>(small, w, bias, aux, big, nimg, epi, packed, ws, ws_bytes, s)
                    : launch_buconv_scatter<G, typename R::UpBfScatter, 6>(small, w, bias, aux, big, nimg, epi, packed, ws, ws_bytes, s);
  if constexpr (kOn<typename R::DirectUp>) {
    return launch_dconv_up<G, typename R::DirectUp>(small, w, bias, aux, big, nimg, epi, packed, ws, ws_bytes, s);
  } else if constexpr (kOn<typename R::UpScatter>) {
    return launch_uconv_scatter<G, typename R::UpScatter>(small, w, bias, aux, big, nimg, epi, packed, ws, ws_bytes, s);
  } else {
    // UpEngine::Merged: 3-channel outputs (encoder conv1 data-gradient, plain decoder conv4) and, in the 128 x 128 stack,
    // the outputs whose class planes do not fit LDS: the four output parity classes read the same (J x J) input taps, so
    // they are merged on M (4 * CB rows) in the gather engine of igemm.h
    static_assert(G::KS % 2 == 0, "the gather engine pairs horizontally adjacent output pixels");
    ConvUpMergedOp<G, float, 0> op{small, w, bias, aux, big, (int)nimg, epi, nullptr, nullptr, nullptr, 0.f, 0.f};
    if constexpr (G::CB < 8) return launch_igemm<T32x256>(op, 4 * G::CB, nimg * (int64_t)op.NY * op.NX, 1, s);
    else return launch_igemm<T64x128>(op, 4 * G::CB, nimg * (int64_t)op.NY * op.NX, 1, s);
  }
}

// ---- weight gradient.  Workspace: [one slab per split (room for the larger of the engines' sets: the engine is a
// thread-local switch) | the channel sums' partials for dbias_big where the engine does not produce them]
static inline int chansum_splits(int64_t nimg, int64_t C, int64_t P) {
  long want = (4096 + C - 1) / C;
  long min_imgs = (8192 + P - 1) / P;
  long maxs = (nimg + min_imgs - 1) / min_imgs;
  if (want > maxs) want = maxs;
  if (want < 1) want = 1;
  long ips = (nimg + want - 1) / want;
  return (int)((nimg + ips - 1) / ips);
}
static int channel_sum_launch(int64_t nimg, int64_t C, int64_t P, const float* x, float* out, int accumulate, float* ws,
                              hipStream_t stream) {
  const int splits = chansum_splits(nimg, C, P);
  const int ips = (int)((nimg + splits - 1) / splits);
  hipLaunchKernelGGL(channel_sum_kernel, dim3((unsigned)C, (unsigned)splits), dim3(256), 0, stream, x, (int)nimg, (int)C,
                     (int)P, ips, ws);
  REPO_CHECK_LAUNCH();
  hipLaunchKernelGGL(channel_sum_final_kernel, dim3(cdiv(C, 4)), dim3(256), 0, stream, (const float*)ws, splits, (int)C,
                     out, accumulate);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

enum class WgradEngine { Transposing, Bf16, Fp32 };
struct WgradPlan {
  WgradEngine engine;
  int ips, splits;      // images per split, splits (= slabs)
  int slab_floats;      // one slab
  bool dbig_in_slabs;   // the channel sums of `big` ride along (behind each slab) and leave through the slab reduce
  bool wave_reduce;     // conv_slab_reduce_wave_kernel (many splits, few outputs) or conv_slab_reduce_kernel
  size_t chan_off;      // offset of the separate channel-sum pass's partials
  size_t need;
  bool high;            // repo_conv_precision: the bf16 engines' three-product instantiation
};
template <class G, class BigT>
static WgradPlan wgrad_plan(int64_t nimg, bool wants_dbig) {
  using R = Route<G>;
  using T = typename R::Wgrad;
  constexpr bool kFloat = std::is_same<BigT, float>::value;
  const long tiles = ((G::CS + T::BM - 1) / T::BM) * ((G::CB * G::KK + T::BN - 1) / T::BN);
  const long want = (R::WGT + tiles - 1) / tiles;
  const long min_ips = T::GI * ((G::PS >= 512) ? 1 : (G::PS >= 64 ? 2 : 4));
  const long ips = (std::max((long)(nimg + want - 1) / want, min_ips) + T::GI - 1) / T::GI * T::GI;
  constexpr int row = G::CS * (G::CB * G::KK + 1);
  WgradPlan p{WgradEngine::Fp32, (int)ips, (int)((nimg + ips - 1) / ips), row, false, false, 0, 0, conv_precision_high()};
  p.wave_reduce = p.splits >= 64 && row <= 65536;
  size_t slabs = (size_t)p.splits * row * sizeof(float);
  if constexpr (kOn<typename R::WgradBf> && kFloat) {
    static_assert(T::GI % R::WgradBf::GI == 0, "images per split: a multiple of both kernels' chunks");
    if (t_bconv_enabled) p.engine = WgradEngine::Bf16;
  }
  if constexpr (R::TwNBK > 0) {
    using TG = TWGeo<G, R::TwNBK, R::TwNPW>;
    const int tips = (int)((nimg + 127) / 128), tsplits = (int)((nimg + tips - 1) / tips);
    slabs = std::max(slabs, (size_t)tsplits * TG::SLAB * sizeof(float));
    // where the taps reach every row and column of `big` (decoder conv3; not the 31 x 31 planes of encoder conv2, whose
    // last row and column no window touches) every element is staged exactly once and its channel sums ride along
    constexpr bool covers = R::TwDbig && G::HB == 2 * (G::HS - 1) + G::KS;
    if (kFloat && t_bconv_enabled) p = WgradPlan{WgradEngine::Transposing, tips, tsplits, TG::SLAB, covers && wants_dbig, true, 0, 0, p.high};
  }
  p.chan_off = round256(slabs);
  p.need = p.chan_off + (size_t)chansum_splits(nimg, G::CB, G::PB) * G::CB * sizeof(float);
  return p;
}

template <class G, class BigT>
static int conv_wgrad_t(int64_t nimg, const float* small, const BigT* big, float* dw, float* db, float* dbig,
                        int accumulate, void* ws, size_t ws_bytes, hipStream_t s) {
  if (nimg * (int64_t)G::CB * G::PB >= kMaxBufElems || nimg * (int64_t)G::CS * G::PS >= kMaxBufElems) return REPO_E_SHAPE;
  using R = Route<G>;
  constexpr bool kFloat = std::is_same<BigT, float>::value;
  const WgradPlan p = wgrad_plan<G, BigT>(nimg, dbig != nullptr);
  if (!ws || ws_bytes < p.need) return REPO_E_WS_TOO_SMALL;
  WgradArgs a{small, big, (float*)ws, (int)nimg, p.ips, db != nullptr,
              (unsigned)(nimg * G::CS * G::PS * sizeof(float)), (unsigned)(nimg * G::CB * G::PB * sizeof(BigT))};
  a.want_dbig = p.dbig_in_slabs;
  int rc = REPO_E_BADARG;
  switch (p.engine) {
    case WgradEngine::Transposing:
      if constexpr (R::TwNBK > 0 && kFloat)
        rc = p.high ? launch_tconv_wgrad<G, R::TwNBK, R::TwNPW, 3>(a, p.splits, s) : launch_tconv_wgrad<G, R::TwNBK, R::TwNPW, 6>(a, p.splits, s);
      break;
    case WgradEngine::Bf16:
      if constexpr (kOn<typename R::WgradBf> && kFloat)
        rc = p.high ? launch_bconv_wgrad<G, typename R::WgradBf, 3>(a, p.splits, s) : launch_bconv_wgrad<G, typename R::WgradBf, 6>(a, p.splits, s);
      break;
    case WgradEngine::Fp32: rc = launch_dconv_wgrad<G, BigT, typename R::Wgrad>(a, p.splits, s); break;
  }
  if (rc) return rc;
  if (p.wave_reduce) {
    // the transposing engine's slabs are [tap][row][channel] (+ db, + the channel sums of `big`): the kernel's tkk / tcb
    const bool tw = p.engine == WgradEngine::Transposing;
    hipLaunchKernelGGL(conv_slab_reduce_wave_kernel, dim3(cdiv(p.slab_floats, 64)), dim3(64 * SLAB_REDUCE_WAVES), 0, s,
                       (const float*)ws, p.splits, G::CS, G::CB * G::KK, dw, db, accumulate, tw ? G::KK : 0, tw ? G::CB : 0,
                       p.dbig_in_slabs ? dbig : (float*)nullptr);
  } else {
    const int blocks = cdiv(p.slab_floats, 256) < 2048 ? cdiv(p.slab_floats, 256) : 2048;
    hipLaunchKernelGGL(conv_slab_reduce_kernel, dim3(blocks), dim3(256), 0, s, (const float*)ws, p.splits, G::CS, G::CB * G::KK, dw, db,
                       accumulate);
  }
  REPO_CHECK_LAUNCH();
  if (dbig && !p.dbig_in_slabs) {
    if constexpr (kFloat) return channel_sum_launch(nimg, G::CB, G::PB, big, dbig, accumulate, (float*)((char*)ws + p.chan_off), s);
    else return REPO_E_BADARG;
  }
  return REPO_OK;
}

}  // namespace repo

using namespace repo;

#define REPO_LAYER_SWITCH(layer, CALL)                 \
  switch (layer) {                                     \
    case 0: { using G = GEnc1; CALL; }                 \
    case 1: { using G = GEnc2; CALL; }                 \
    case 2: { using G = GEnc3; CALL; }                 \
    case 3: { using G = GEnc4; CALL; }                 \
    case 4: { using G = GDec2; CALL; }                 \
    case 5: { using G = GDec3; CALL; }                 \
    case 6: { using G = GDec4; CALL; }                 \
    case 7: { using G = GX1; CALL; }                   \
    case 8: { using G = GX2; CALL; }                   \
    case 9: { using G = GX3; CALL; }                   \
    case 10: { using G = GX4; CALL; }                  \
    case 11: { using G = GY4; CALL; }                  \
    case 12: { using G = GY5; CALL; }                  \
    case 13: { using G = GT4; CALL; }                  \
    default: return REPO_E_BADARG;                     \
  }

extern "C" int repo_conv_down(int layer, int64_t nimg, const void* big, int big_is_u8, const float* w,
                              const float* bias, float* small, int epi, const void* aux_, float* dbias_small,
                              int accumulate_dbias, unsigned char* relu_cmask, void* ws, size_t ws_bytes,
                              hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_CONV_PRECISION_GUARD();
  REPO_REQUIRE(nimg >= 0, REPO_E_SHAPE);
  if (nimg == 0) return REPO_OK;
  REPO_REQUIRE(big && w && small, REPO_E_BADARG);
  REPO_REQUIRE(epi == REPO_EPI_NONE || epi == REPO_EPI_RELU ||
                   ((epi == REPO_EPI_MUL_DRELU || epi == REPO_EPI_MUL_MASK4 || epi == REPO_EPI_FILM_RELU) && aux_), REPO_E_BADARG);
  REPO_REQUIRE(!relu_cmask || epi == REPO_EPI_RELU, REPO_E_BADARG);
  REPO_REQUIRE(epi != REPO_EPI_FILM_RELU || !dbias_small, REPO_E_BADARG);
  const float* aux = (const float*)aux_;  // fp32 activations, or the quad mask's bytes (REPO_EPI_MUL_MASK4)
  if (big_is_u8) {
    REPO_REQUIRE(layer == 0 || layer == 7, REPO_E_BADARG);
    if (layer == 7)
      return conv_down_t<GX1, uint8_t>(nimg, (const uint8_t*)big, w, bias, small, epi, aux, dbias_small,
                                       accumulate_dbias, relu_cmask, ws, ws_bytes, stream);
    return conv_down_t<GEnc1, uint8_t>(nimg, (const uint8_t*)big, w, bias, small, epi, aux, dbias_small,
                                       accumulate_dbias, relu_cmask, ws, ws_bytes, stream);
  }
  REPO_LAYER_SWITCH(layer, return (conv_down_t<G, float>(nimg, (const float*)big, w, bias, small, epi, aux, dbias_small,
                                                         accumulate_dbias, relu_cmask, ws, ws_bytes, stream)))
}

extern "C" size_t repo_conv_down_workspace_bytes(int layer, int64_t nimg) {
  if (nimg <= 0) return 0;
  REPO_LAYER_SWITCH(layer, return (conv_down_ws_bytes<G>(nimg)))
}

extern "C" int repo_debug_bconv(int enable) {
  const int prev = t_bconv_enabled;
  t_bconv_enabled = enable ? 1 : 0;
  return prev;
}

extern "C" int repo_conv_precision(int mode) {
  if (mode != REPO_CONV_PRECISION_HIGHEST && mode != REPO_CONV_PRECISION_HIGH) return REPO_E_BADARG;
  const int prev = conv_precision();
  if (prev < 0) return prev;   // REPO_CONV_PRECISION names no mode: nothing is set over it
  t_conv_precision = mode;
  return prev;
}

extern "C" size_t repo_conv_up_workspace_bytes(int layer) {
  REPO_LAYER_SWITCH(layer, return (up_plan<G>(0, REPO_EPI_NONE, 0).total))
}

extern "C" int repo_conv_up_pack(int layer, const float* w, void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_CONV_PRECISION_GUARD();
  REPO_REQUIRE(w, REPO_E_BADARG);
  REPO_LAYER_SWITCH(layer, return (conv_up_pack_t<G>(w, ws, ws_bytes, stream)))
}

extern "C" int repo_conv_up(int layer, int64_t nimg, const float* small, const float* w, const float* bias,
                            float* big, int epi, const float* aux, int ws_is_packed, void* ws, size_t ws_bytes,
                            hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_CONV_PRECISION_GUARD();
  REPO_REQUIRE(nimg >= 0, REPO_E_SHAPE);
  if (nimg == 0) return REPO_OK;
  REPO_REQUIRE(small && w && big, REPO_E_BADARG);
  REPO_REQUIRE(epi == REPO_EPI_NONE || epi == REPO_EPI_RELU ||
                   ((epi == REPO_EPI_MUL_DRELU || epi == REPO_EPI_MUL_CMASK || epi == REPO_EPI_FILM_RELU) && aux), REPO_E_BADARG);
  REPO_LAYER_SWITCH(layer, return (conv_up_t<G>(nimg, small, w, bias, big, epi, aux, ws_is_packed, ws, ws_bytes, stream)))
}

extern "C" size_t repo_conv_wgrad_workspace_bytes(int layer, int64_t nimg) {
  if (nimg <= 0) return 0;
  REPO_LAYER_SWITCH(layer, return (wgrad_plan<G, float>(nimg, false).need))
}

extern "C" int repo_conv_wgrad(int layer, int64_t nimg, const float* small, const void* big, int big_is_u8,
                               float* dw, float* dbias_small, float* dbias_big, int accumulate, void* ws,
                               size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_CONV_PRECISION_GUARD();
  REPO_REQUIRE(nimg > 0, REPO_E_SHAPE);
  REPO_REQUIRE(small && big && dw, REPO_E_BADARG);
  if (big_is_u8) {
    REPO_REQUIRE((layer == 0 || layer == 7) && !dbias_big, REPO_E_BADARG);
    if (layer == 7)
      return conv_wgrad_t<GX1, uint8_t>(nimg, small, (const uint8_t*)big, dw, dbias_small, nullptr, accumulate, ws,
                                        ws_bytes, stream);
    return conv_wgrad_t<GEnc1, uint8_t>(nimg, small, (const uint8_t*)big, dw, dbias_small, nullptr, accumulate, ws,
                                        ws_bytes, stream);
  }
  REPO_LAYER_SWITCH(layer, return (conv_wgrad_t<G, float>(nimg, small, (const float*)big, dw, dbias_small, dbias_big,
                                                          accumulate, ws, ws_bytes, stream)))
}

// loss partials, then either the kernel's per-channel partials or the channel-sum pass's (the fp32 twin)
static size_t dec4_nll_ws_floats(int64_t nimg) {
  const size_t n = (size_t)dec4_nll_grid(nimg);
  const size_t cs = (size_t)chansum_splits(nimg, GDec4::CB, GDec4::PB) * GDec4::CB;
  return n + (3 * n > cs ? 3 * n : cs);
}
extern "C" size_t repo_decoder_out_nll_workspace_bytes(int64_t nimg) {
  return nimg <= 0 ? 0 : dec4_nll_ws_floats(nimg) * sizeof(float);
}

template <class TgtT>
static int decoder_out_nll_t(int64_t nimg, const float* h3, const float* w, const float* bias, const TgtT* target,
                             float grad_scale, float* recon, float* dpre, unsigned char* mask4, float* loss_sum,
                             float* dbias, int accumulate_dbias, void* ws, hipStream_t stream) {
  using G = GDec4;
  const int nparts = dec4_nll_grid(nimg);
  float* chan = (float*)ws + nparts;
  NllArgs a{h3, w, bias, target, recon, dpre, mask4, (float*)ws, grad_scale, (int)nimg,
            (unsigned)(nimg * G::CS * G::PS * sizeof(float))};
  // ONE decision: the bf16x6 kernel (bdec4.h), whose per-channel partials are the bias gradient's, or -- repo_debug_bconv(0)
  // -- the fp32-MFMA twin with a channel-sum pass over dpre
  // ... and, on the bf16 kernel, its six- or three-product instantiation (repo_conv_precision)
  const bool bf = t_bconv_enabled != 0;
  a.chan_partials = bf && dbias ? chan : nullptr;
  if (bf && conv_precision_high()) hipLaunchKernelGGL((bdec4_nll_kernel<TgtT, 3>), dim3(nparts), dim3(256), 0, stream, a);
  else if (bf) hipLaunchKernelGGL((bdec4_nll_kernel<TgtT, 6>), dim3(nparts), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((dconv_dec4_nll_kernel<TgtT>), dim3(nparts), dim3(256), 0, stream, a);
  REPO_CHECK_LAUNCH();
  if (loss_sum) {
    hipLaunchKernelGGL(partial_sum_kernel, dim3(1), dim3(1024), 0, stream, (const float*)ws, nparts, loss_sum, 0);
    REPO_CHECK_LAUNCH();
  }
  if (!dbias) return REPO_OK;
  // the output layer's bias gradient = the channel sums of dpre
  if (!bf) return dpre ? channel_sum_launch(nimg, G::CB, G::PB, dpre, dbias, accumulate_dbias, chan, stream) : REPO_E_BADARG;
  hipLaunchKernelGGL(partial_sum_rows_kernel, dim3(3), dim3(256), 0, stream, (const float*)chan, nparts, dbias, grad_scale,
                     accumulate_dbias);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}

extern "C" int repo_decoder_out_nll(int64_t nimg, const float* h3, const float* w, const float* bias,
                                    const void* target, int target_is_u8, float grad_scale, float* recon, float* dpre,
                                    unsigned char* relu_mask4, float* loss_sum, float* dbias, int accumulate_dbias,
                                    void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_CONV_PRECISION_GUARD();
  REPO_REQUIRE(nimg > 0, REPO_E_SHAPE);
  REPO_REQUIRE(h3 && w && target, REPO_E_BADARG);
  REPO_REQUIRE(nimg * (int64_t)GDec4::CS * GDec4::PS < kMaxBufElems, REPO_E_SHAPE);
  REPO_REQUIRE(ws && ws_bytes >= repo_decoder_out_nll_workspace_bytes(nimg), REPO_E_WS_TOO_SMALL);
  if (target_is_u8)
    return decoder_out_nll_t<uint8_t>(nimg, h3, w, bias, (const uint8_t*)target, grad_scale, recon, dpre, relu_mask4,
                                      loss_sum, dbias, accumulate_dbias, ws, stream);
  return decoder_out_nll_t<float>(nimg, h3, w, bias, (const float*)target, grad_scale, recon, dpre, relu_mask4, loss_sum,
                                  dbias, accumulate_dbias, ws, stream);
}

// ---- a 3-channel transposed conv fused with the pixel likelihood on the gather engine (any output size): what the
//      128 x 128 stack's output layer (layer 12) runs on; layer 6 goes through it too in the tests, as a second
//      implementation of repo_decoder_out_nll.
template <class G>
static long up_nll_parts(int64_t nimg) {
  constexpr int NY = (G::HB + 1) / 2, NX = (G::WB + 1) / 2;
  return (nimg * (long)NY * NX + T32x256::BN - 1) / T32x256::BN;  // one workgroup row (M = 12 <= 32)
}
template <class G, class TgtT>
static int conv_up_nll_t(int64_t nimg, const float* small, const float* w, const float* bias, const TgtT* target,
                         float grad_scale, float* recon, float* dpre, float* loss_sum, void* ws, size_t ws_bytes,
                         hipStream_t stream) {
  static_assert(G::CB < 8 && G::KS % 2 == 0, "output layers only");
  if (nimg * (int64_t)G::CB * G::PB >= kMaxBufElems || nimg * (int64_t)G::CS * G::PS >= kMaxBufElems) return REPO_E_SHAPE;
  const long nparts = up_nll_parts<G>(nimg);
  if (!ws || ws_bytes < (size_t)nparts * sizeof(float)) return REPO_E_WS_TOO_SMALL;
  ConvUpMergedOp<G, TgtT, 1> op{small, w, bias, nullptr, recon, (int)nimg, REPO_EPI_NONE, target, dpre, (float*)ws,
                                grad_scale, 0.f};
  const int rc = launch_igemm<T32x256>(op, 4 * G::CB, nimg * (int64_t)op.NY * op.NX, 1, stream);
  if (rc) return rc;
  if (loss_sum) {
    hipLaunchKernelGGL(partial_sum_kernel, dim3(1), dim3(1024), 0, stream, (const float*)ws, (int)nparts, loss_sum, 0);
    REPO_CHECK_LAUNCH();
  }
  return REPO_OK;
}

extern "C" size_t repo_conv_up_nll_workspace_bytes(int layer, int64_t nimg) {
  if (nimg <= 0) return 0;
  if (layer == 6) return (size_t)up_nll_parts<GDec4>(nimg) * sizeof(float);
  if (layer == 12) return (size_t)up_nll_parts<GY5>(nimg) * sizeof(float);
  return 0;
}

extern "C" int repo_conv_up_nll(int layer, int64_t nimg, const float* small, const float* w, const float* bias,
                                const void* target, int target_is_u8, float grad_scale, float* recon, float* dpre,
                                float* loss_sum, void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(nimg > 0, REPO_E_SHAPE);
  REPO_REQUIRE(small && w && target, REPO_E_BADARG);
  REPO_REQUIRE(layer == 6 || layer == 12, REPO_E_BADARG);
#define REPO_UPNLL(G)                                                                                                  \
  return target_is_u8 ? conv_up_nll_t<G, uint8_t>(nimg, small, w, bias, (const uint8_t*)target, grad_scale, recon, dpre, \
                                                  loss_sum, ws, ws_bytes, stream)                                         \
                      : conv_up_nll_t<G, float>(nimg, small, w, bias, (const float*)target, grad_scale, recon, dpre,      \
                                                loss_sum, ws, ws_bytes, stream)
  if (layer == 6) { REPO_UPNLL(GDec4); }
  REPO_UPNLL(GY5);
#undef REPO_UPNLL
}

extern "C" size_t repo_channel_sum_workspace_bytes(int64_t nimg, int64_t C, int64_t P) {
  if (nimg <= 0 || C <= 0 || P <= 0) return 0;
  return (size_t)chansum_splits(nimg, C, P) * C * sizeof(float);
}

extern "C" int repo_channel_sum(int64_t nimg, int64_t C, int64_t P, const float* x, float* out, int accumulate,
                                void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(nimg > 0 && C > 0 && P > 0, REPO_E_SHAPE);
  REPO_REQUIRE(x && out, REPO_E_BADARG);
  REPO_REQUIRE(C <= 65535, REPO_E_SHAPE);
  const int splits = chansum_splits(nimg, C, P);
  REPO_REQUIRE(ws && ws_bytes >= (size_t)splits * C * sizeof(float), REPO_E_WS_TOO_SMALL);
  return channel_sum_launch(nimg, C, P, x, out, accumulate, (float*)ws, stream);
}

extern "C" int repo_relu_mask(int64_t n, const float* dy, const float* h, float* y, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(n >= 0, REPO_E_SHAPE);
  if (n == 0) return REPO_OK;
  REPO_REQUIRE(dy && h && y, REPO_E_BADARG);
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(relu_mask_kernel, dim3(blocks), dim3(256), 0, stream, n, dy, h, y);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}
