// The epilogue of every dense product (repo_gemm; include/repo_hip.h states each REPO_EPI_*):
//   C[m][n] (+)= epi( acc + bias[n / bias_div] )
// written once for the fp32 tile engines (GemmOp / VGemmOp in gemm.hip), the bf16x6 engine (bgemm.h) and the <= 8-row
// vector kernel (gemm.hip).
#pragma once
#include "igemm.h"

namespace repo {

struct DenseEpi {
  const float* bias;
  const float* aux;
  float* C;
  int ldc, ldaux, bias_div, epi, accumulate;

  __device__ __forceinline__ float bias_of(int n) const {   // bias_div < 0: one bias per output column (FiLM: header)
    return bias ? bias[bias_div > 1 ? n / bias_div : n] : 0.f;
  }
  // v = accumulator of C[m][n] plus its bias -> the value stored there.  Each engine keeps the addressing it was tuned with
  // (register counts: profiles/*_dense_refactor_resources.txt).  COL (the fp32 tile ops, 32-bit offsets): c and ax point
  // at row m - dm of column n and dm * ld is added; else (size_t offsets): c = C, ax = aux and m * ld + n is added.
  // FILM = false leaves the FiLM branch out (the <= 8-row kernel, which repo_gemm keeps out of FiLM).
  template <bool FILM, bool COL>
  __device__ __forceinline__ void put(float v, int m, int n, int dm, const float* ax, float* c) const {
    if (epi == REPO_EPI_ELU) v = elu(v);
    else if (epi == REPO_EPI_RELU) v = fmaxf(v, 0.f);
    else if (epi == REPO_EPI_MUL_DELU) v *= elu_grad_from_out(COL ? ax[dm * ldaux] : ax[(size_t)m * ldaux + n]);
    else if (epi == REPO_EPI_MUL_DRELU) v = (COL ? ax[dm * ldaux] : ax[(size_t)m * ldaux + n]) > 0.f ? v : 0.f;
    else if (epi == REPO_EPI_LEAKY) v = v > 0.f ? v : kLeakySlope * v;
    else if (epi == REPO_EPI_MUL_DLEAKY) v = (COL ? ax[dm * ldaux] : ax[(size_t)m * ldaux + n]) > 0.f ? v : kLeakySlope * v;
    else if (FILM && epi == REPO_EPI_FILM_RELU) {   // row m's FiLM table: [scale (C) | shift (C)], C = ldaux / 2, channel n / |bias_div|
      const int ch = bias_div == 1 ? n : n / (bias_div < 0 ? -bias_div : bias_div);
      const float* tb = aux + (size_t)m * ldaux;
      v = fmaxf(fmaf(tb[ch], v, tb[(ldaux >> 1) + ch]), 0.f);
    }
    float* d = COL ? c + dm * ldc : c + (size_t)m * ldc + n;
    if (accumulate) v += *d;
    *d = v;
  }
  // one lane's 16 accumulators of a 32 x 32 MFMA tile: column n, rows mb + (r & 3) + 8 * (r >> 2) below M
  template <bool COL>
  __device__ __forceinline__ void store_col(int mb, int n, const f32x16& acc, int M) const {
    const float bv = bias_of(n);
    float* c = COL ? C + mb * ldc + n : C;
    const float* ax = COL ? (aux ? aux + mb * ldaux + n : nullptr) : aux;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dm = (r & 3) + 8 * (r >> 2);
      if (mb + dm < M) put<true, COL>(acc[r] + bv, mb + dm, n, dm, ax, c);
    }
  }
};

}  // namespace repo
