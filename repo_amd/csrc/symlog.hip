// symlog(x) = sign(x) log1p(|x|) over a flat fp32 buffer (config.obs_symlog): the state-vector frames of a
// batch, transformed once into the buffer that is both the encoder's input and the decoder's target.  HBM-bound streaming:
// 16-byte accesses where both bases allow, dwords for a misaligned base and for the ragged tail, a grid-stride loop under a
// block cap.  x and y are not __restrict__: y == x (in place) is part of the contract -- every element is read and written
// by the same thread, the read first.
#include "common.h"

namespace repo {

constexpr int kSymThreads = 256;
constexpr int kSymVec = 4;          // floats per 16-byte access
constexpr int kSymMaxBlocks = 1024;

// Odd in bits: the magnitude is a function of |x| alone and the sign bit is copied, so symlog(-x) == -symlog(x), -0 -> -0;
// NaN -> NaN, +-inf -> +-inf.  Below 2^-24, log1p(a) = a (1 - a / 2 + ...) rounds to a: returned as it is, which also keeps
// denormals out of log1pf.
__device__ __forceinline__ float symlog1(float x) {
  const float a = fabsf(x);
  return copysignf(a < 0x1p-24f ? a : log1pf(a), x);
}

// vec != 0: both bases are 16-byte aligned; nvec = n / 4 whole vectors, then the n % 4 tail elements as dwords.
__global__ __launch_bounds__(kSymThreads) void symlog_kernel(long n, const float* x, float* y, int vec) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (long)gridDim.x * blockDim.x;
  long done = 0;
  if (vec) {
    const long nvec = n / kSymVec;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    float4* y4 = reinterpret_cast<float4*>(y);
    for (long i = tid; i < nvec; i += nthreads) {
      float4 v = x4[i];
      v.x = symlog1(v.x);
      v.y = symlog1(v.y);
      v.z = symlog1(v.z);
      v.w = symlog1(v.w);
      y4[i] = v;
    }
    done = nvec * kSymVec;
  }
  for (long i = done + tid; i < n; i += nthreads) y[i] = symlog1(x[i]);
}

}  // namespace repo

using namespace repo;

extern "C" int repo_symlog_geometry(int* threads, int* vec_floats, int* max_blocks) {
  REPO_REQUIRE(threads && vec_floats && max_blocks, REPO_E_BADARG);
  *threads = kSymThreads;
  *vec_floats = kSymVec;
  *max_blocks = kSymMaxBlocks;
  return REPO_OK;
}

extern "C" int repo_symlog(int64_t n, const float* x, float* y, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(n >= 0, REPO_E_SHAPE);
  REPO_REQUIRE(x && y, REPO_E_BADARG);
  if (n == 0) return REPO_OK;
  const int vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0 && n >= kSymVec;
  const long items = vec ? n / kSymVec : n;   // (the tail of the vector form is at most 3 elements: the first threads')
  long blocks = (items + kSymThreads - 1) / kSymThreads;
  if (blocks > kSymMaxBlocks) blocks = kSymMaxBlocks;
  hipLaunchKernelGGL(symlog_kernel, dim3((unsigned)blocks), dim3(kSymThreads), 0, stream, (long)n, x, y, vec);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}
