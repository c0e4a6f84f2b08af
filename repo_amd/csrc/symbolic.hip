// State-vector observations (config.pixel_obs = False; reference models/decoder.py SymbolicObservationModel with the
// obs-loss line dreamer.py:262-267): the output head of the symbolic decoder.  repo_linear_unit_nll applies the last
// Linear, takes the unit-variance Normal NLL against the observation vectors and emits the pre-activation gradient, without
// storing the reconstruction -- the ending repo_decoder_out_nll gives the pixel decoder.
//
// The product runs on the fp32 matrix pipe through the vector-load tile engine (vgemm.h: 16-byte buffer loads along k for
// both operands, LDS slices [k][m] / [k][n], v_mfma_f32_32x32x2_f32); the fusion is the operator's epilogue: every lane
// holds 16 predictions of one output column in registers, turns them into 0.5 d^2 and d * scale there, and the workgroup
// leaves ONE partial sum.  Sums follow loss.hip: wave64 shuffles, one partial per workgroup, a fixed-order final sum by the
// launch's last block (common.h, last_block_finishes) or, for grids above kLastBlockMaxGrid, by a one-block follow-up
// launch -- no float atomics, two runs give the same bits.
#include "vgemm.h"

namespace repo {

// Test / measurement aid (repo_debug_linear_nll): 0 = the dispatch below, 1 = the fused kernel wherever its operands allow
// it, 2 = the composition everywhere.  Thread-local like the other debug switches (api.hip).
static thread_local int t_linear_nll_mode = 0;

// 32 rows x 64 outputs per 128-thread workgroup, K slices of 32: the product is a thin one (O = 17 .. 67 outputs at the
// workload against K = 1024), so its time is the chain of dependent K slices of each workgroup -- 32-row tiles give 77
// workgroups at 2450 rows where 64-row tiles give 39, and 32-deep slices halve the barriers per workgroup.
using NllTile = T32x64k32;
constexpr int kNllMaxGrid = 2048;   // partials the reduction workspace holds (repo_reduce_workspace_bytes)

struct LinearNllOp {
  static constexpr bool A_VK = true;   // h[m][k]
  static constexpr bool B_VK = true;   // W[o][k]
  static constexpr int VW = 4;
  Dense2D A, B;
  const float* bias;
  const float* target;
  float* dpre;
  float* recon;   // nullable
  float* parts;
  float* out;
  unsigned* ticket;   // nullable: the follow-up launch sums the partials
  int M_, N_, K_, ldt, lddp, ldr, ntiles_n;
  float scale;
  float lsum;   // this thread's share of the workgroup's partial

  __device__ void init(int) { lsum = 0.f; }
  __device__ void decode(int t, int& bx, int& by, int& bz) const {   // 1-D grid: gridDim.x workgroups = partials
    bx = t % ntiles_n;
    by = t / ntiles_n;
    bz = 0;
  }
  __device__ int M() const { return M_; }
  __device__ int N() const { return N_; }
  __device__ int kbeg() const { return 0; }
  __device__ int kend() const { return K_; }
  template <class V>
  __device__ void fix_b(V&, int) const {}
  // one lane's 16 accumulators of a 32 x 32 MFMA tile: column n, rows mb + (r & 3) + 8 * (r >> 2) below M
  __device__ void store_col(int mb, int n, const f32x16& acc, int M) {
    const float bv = bias[n];
    const float* t = target + mb * ldt + n;
    float* d = dpre + mb * lddp + n;
    float* rc = recon ? recon + mb * ldr + n : nullptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dm = (r & 3) + 8 * (r >> 2);
      if (mb + dm < M) {
        const float p = acc[r] + bv;
        const float e = p - t[dm * ldt];
        lsum += 0.5f * e * e;
        d[dm * lddp] = e * scale;
        if (rc) rc[dm * ldr] = p;
      }
    }
  }
  __device__ void finish() {
    __shared__ float red[16];
    const float s = block_sum(lsum, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = s;
    last_block_finishes(parts, 1, out, ticket, red);
  }
};

// out[0] = sum of parts[0 .. n) in last_block_finishes' order (grids above kLastBlockMaxGrid)
__global__ __launch_bounds__(256) void nll_parts_sum_kernel(const float* __restrict__ parts, int n, float* __restrict__ out) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += parts[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

// The NLL pass of the composition: scalar_nll_kernel's arithmetic (loss.hip) over a (rows, O) block whose three operands
// have row pitches -- pred is repo_gemm's output.  At most kLastBlockMaxGrid workgroups: the launch finishes its own sum.
__global__ __launch_bounds__(256) void unit_nll_rows_kernel(long n, int O, const float* __restrict__ pred, long ldp,
                                                            const float* __restrict__ target, long ldt, float scale,
                                                            float* __restrict__ dpre, long lddp, float* __restrict__ parts,
                                                            float* __restrict__ out, unsigned* __restrict__ ticket) {
  __shared__ float red[16];
  float a = 0.f;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const long row = e / O;
    const int j = (int)(e - row * O);
    const float d = pred[row * ldp + j] - target[row * ldt + j];
    a += 0.5f * d * d;
    dpre[row * lddp + j] = d * scale;
  }
  const float s = block_sum(a, red);
  if (threadIdx.x == 0) parts[blockIdx.x] = s;
  last_block_finishes(parts, 1, out, ticket, red);
}

static inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }
static inline long nll_grid(int64_t rows, int64_t O) {
  return (long)((rows + NllTile::BM - 1) / NllTile::BM) * (long)((O + NllTile::BN - 1) / NllTile::BN);
}
// what the fused kernel asks of its operands: 16-byte vectors along k for h and W, a grid whose partials fit
static bool nll_fused_legal(int64_t rows, int64_t O, int64_t K, const float* h, int64_t ldh, const float* W, int64_t ldw) {
  return K % 4 == 0 && ldh % 4 == 0 && ldw % 4 == 0 && aligned16(h) && aligned16(W) && nll_grid(rows, O) <= kNllMaxGrid;
}
static bool nll_takes_fused(int64_t rows, int64_t O, int64_t K, const float* h, int64_t ldh, const float* W, int64_t ldw) {
  if (t_linear_nll_mode == 2 || !nll_fused_legal(rows, O, K, h, ldh, W, ldw)) return false;
  return true;   // (no shape measured yet at which the composition is the faster form: DESIGN.md 6g)
}

}  // namespace repo

using namespace repo;

extern "C" int repo_debug_linear_nll(int mode) {
  const int prev = t_linear_nll_mode;
  if (mode >= 0 && mode <= 2) t_linear_nll_mode = mode;
  return prev;
}

extern "C" int repo_linear_unit_nll_fused(int64_t rows, int64_t O, int64_t K, const float* h, int64_t ldh, const float* W,
                                          int64_t ldw) {
  return rows > 0 && O > 0 && K > 0 && nll_takes_fused(rows, O, K, h, ldh, W, ldw) ? 1 : 0;
}

extern "C" int repo_linear_unit_nll(int64_t rows, int64_t O, int64_t K, const float* h, int64_t ldh, const float* W,
                                    int64_t ldw, const float* bias, const float* target, int64_t ldt, float grad_scale,
                                    float* sums, float* dpre, int64_t lddpre, float* recon, int64_t ldrecon, float* scratch,
                                    size_t scratch_bytes, void* ws, size_t ws_bytes, hipStream_t stream) {
  REPO_ARCH_GUARD();
  REPO_REQUIRE(rows >= 1 && O >= 1 && O <= 1024 && K >= 1, REPO_E_SHAPE);
  REPO_REQUIRE(ldh >= K && ldw >= K && ldt >= O && lddpre >= O && (!recon || ldrecon >= O), REPO_E_SHAPE);
  REPO_REQUIRE(h && W && bias && target && sums && dpre, REPO_E_BADARG);
  // 32-bit offsets inside the kernels (and repo_gemm's own bounds for the composition)
  REPO_REQUIRE(rows < kMaxIdx && K < kMaxIdx && ldh < kMaxIdx && ldw < kMaxIdx, REPO_E_SHAPE);
  REPO_REQUIRE((rows - 1) * ldh + K < kMaxBufElems && (O - 1) * ldw + K < kMaxBufElems, REPO_E_SHAPE);
  REPO_REQUIRE(rows * ldt < kMaxIdx && rows * lddpre < kMaxIdx && (!recon || rows * ldrecon < kMaxIdx) && rows * O < kMaxIdx,
               REPO_E_SHAPE);
  REPO_REQUIRE(ws && ws_bytes >= repo_reduce_workspace_bytes(), REPO_E_WS_TOO_SMALL);
  float* parts = (float*)((char*)ws + kRedHeaderBytes);
  unsigned* ticket = (unsigned*)ws;

  if (nll_takes_fused(rows, O, K, h, ldh, W, ldw)) {
    const long blocks = nll_grid(rows, O);
    LinearNllOp op;
    op.A = Dense2D{h, 4u * (unsigned)((rows - 1) * ldh + K), (int)ldh};
    op.B = Dense2D{W, 4u * (unsigned)((O - 1) * ldw + K), (int)ldw};
    op.bias = bias, op.target = target, op.dpre = dpre, op.recon = recon, op.parts = parts, op.out = sums;
    op.ticket = blocks <= kLastBlockMaxGrid ? ticket : nullptr;
    op.M_ = (int)rows, op.N_ = (int)O, op.K_ = (int)K, op.ldt = (int)ldt, op.lddp = (int)lddpre, op.ldr = (int)ldrecon;
    op.ntiles_n = (int)((O + NllTile::BN - 1) / NllTile::BN);
    op.scale = grad_scale, op.lsum = 0.f;
    const int rc = launch_vgemm_flat<NllTile>(op, blocks, stream);
    if (rc) return rc;
    if (blocks > kLastBlockMaxGrid) {
      hipLaunchKernelGGL(nll_parts_sum_kernel, dim3(1), dim3(256), 0, stream, parts, (int)blocks, sums);
      REPO_CHECK_LAUNCH();
    }
    return REPO_OK;
  }

  // the composition: repo_gemm (any K, any alignment: its plan falls back to 8-byte loads or gathers) into the
  // reconstruction, or into the caller's scratch when nobody wants it, then the NLL pass over the pitched block
  float* pred = recon;
  int64_t ldp = ldrecon;
  if (!pred) {
    REPO_REQUIRE(scratch && scratch_bytes >= (size_t)rows * O * sizeof(float), REPO_E_WS_TOO_SMALL);
    pred = scratch, ldp = O;
  }
  const int rc = repo_gemm(0, 1, rows, O, K, h, ldh, W, ldw, bias, 1, pred, ldp, REPO_EPI_NONE, nullptr, 0, 0, stream);
  if (rc) return rc;
  const long n = (long)rows * O;
  int blocks = cdiv(n, 1024);
  if (blocks > kLastBlockMaxGrid) blocks = kLastBlockMaxGrid;
  hipLaunchKernelGGL(unit_nll_rows_kernel, dim3(blocks), dim3(256), 0, stream, n, (int)O, pred, (long)ldp, target, (long)ldt,
                     grad_scale, dpre, (long)lddpre, parts, sums, ticket);
  REPO_CHECK_LAUNCH();
  return REPO_OK;
}
