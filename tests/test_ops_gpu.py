"""Op-level parity of the HIP kernels (through the C ABI) against fp64 PyTorch on CPU.

fp32 tolerance: the kernels accumulate in fp32 (v_mfma_f32_32x32x2_f32 = chained fmaf),
so the normwise error against an fp64 reference is bounded by ~K * 2^-24 * sum|a*b|;
1e-5 relative to the largest output is used throughout (stated per assert).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import CONV_ENGINE_KERNELS, DENSE_ENGINE_KERNELS, has, log, relerr, rnd, traced

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from repo_amd import ops as o

    return o


def dev(t):
    return t.cuda()


@pytest.mark.parametrize("ta,tb", [(False, True), (False, False), (True, False), (True, True)])
@pytest.mark.parametrize("M,N,K", [(50, 200, 36), (2450, 200, 230), (784, 1024, 230), (33, 60, 200), (700, 640, 130), (1, 1, 1), (65, 129, 17), (3000, 200, 1), (300, 7, 1), (1, 200, 230), (5, 60, 200), (8, 600, 1224)])
def test_gemm_layouts(ops, ta, tb, M, N, K):
    rs = np.random.RandomState(M * 7 + N * 3 + K)
    A = rnd(rs, K, M) if ta else rnd(rs, M, K)
    B = rnd(rs, N, K) if tb else rnd(rs, K, N)
    bias = rnd(rs, N)
    want = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double()) + bias.double()
    got = ops.gemm(dev(A), dev(B), ta, tb, bias=dev(bias))
    e = relerr(got, want)
    log(f"gemm ta={ta} tb={tb} {M}x{N}x{K}: relerr {e:.2e}")
    assert e < TOL


def test_gemm_strided_and_epilogues(ops):
    rs = np.random.RandomState(5)
    M, N, K = 300, 200, 230
    feat = rnd(rs, M, 260)  # x is a column slice of a wider buffer
    x = feat[:, 10:240]
    W, b = rnd(rs, N, K, scale=0.1), rnd(rs, N)
    pre = x.double() @ W.double().t() + b.double()
    fd = dev(feat)
    for epi, fn in [(ops.EPI_ELU, F.elu), (ops.EPI_RELU, F.relu), (ops.EPI_NONE, lambda v: v)]:
        got = ops.gemm(fd[:, 10:240], dev(W), transb=True, bias=dev(b), epi=epi)
        e = relerr(got, fn(pre))
        log(f"gemm epi={epi}: relerr {e:.2e}")
        assert e < TOL
    # backward-data with the activation derivative fused + accumulate into a strided slice
    h = F.elu(pre).float()
    dy = rnd(rs, M, N)
    want = (dy.double() * torch.where(h > 0, torch.ones_like(h), h + 1).double()) 
    got = ops.gemm(dev(dy), dev(torch.eye(N)), epi=ops.EPI_MUL_DELU, aux=dev(h))
    assert relerr(got, want) < TOL
    dx_want = dy.double() @ W.double()
    outbuf = torch.ones(M, 260).cuda()
    ops.gemm(dev(dy), dev(W), out=outbuf[:, 10:240], accumulate=True)
    assert relerr(outbuf[:, 10:240], dx_want + 1) < TOL
    assert float((outbuf[:, :10] - 1).abs().max()) == 0 and float((outbuf[:, 240:] - 1).abs().max()) == 0
    hr = F.relu(pre).float()
    got = ops.gemm(dev(dy), dev(torch.eye(N)), epi=ops.EPI_MUL_DRELU, aux=dev(hr))
    assert relerr(got, dy.double() * (hr > 0)) < TOL
    # bias_div (channel bias over 25 pixels)
    W2, b2 = rnd(rs, K, 75), rnd(rs, 3)
    got = ops.gemm(fd[:, 10:240], dev(W2), bias=dev(b2), bias_div=25, epi=ops.EPI_RELU)
    want = F.relu(x.double() @ W2.double() + b2.double().repeat_interleave(25))
    assert relerr(got, want) < TOL


BG_SHAPES = [
    # (ta, tb, M, N, K): the decoder's three big products and ragged variants of each operand layout
    (False, False, 2450, 3200, 1024),   # conv1 forward: h1 = h0 @ W1            (10 x 25 = 250 < 400 tiles of 256 x 128: 128 x 128 tiles)
    (False, True, 2450, 1024, 3200),    # conv1 data gradient: dh0 = d1 @ W1^T   (128 x 128 tiles, K 32 per stage)
    (True, False, 1024, 3200, 2450),    # conv1 weight gradient through repo_gemm's layout: A[k][m], B[k][n]
    (False, True, 1301, 1932, 1001),    # nothing divides anything: M, N ragged in the last tiles, K % 16 = 9, K % 4 = 1
    (False, False, 1300, 1940, 130),     # shortest K the engine takes (two register sets, 5 stages of 32)
    (True, True, 1284, 1937, 777),       # A[k][m] with B[n][k]
    (True, False, 1280, 2048, 16),      # below the engine's K: stays on the fp32 tiles (dispatch boundary)
]


@pytest.mark.parametrize("ta,tb,M,N,K", BG_SHAPES)
def test_bgemm_matches_fp64_and_the_fp32_engine(ops, ta, tb, M, N, K):
    """The bf16x6 dense engine (csrc/bgemm.h: six exact bf16 partial products per fp32 multiply, fp32 accumulation) on
    every operand layout, ragged tiles and K tails, with bias / bias_div / ReLU / accumulate, against fp64 -- and against
    the fp32-MFMA tile engine on the SAME operands (repo_debug_bgemm(0)): its error is not allowed to exceed that
    engine's by more than 25 % (measured: equal or smaller; both are set by the fp32 accumulation over K)."""
    from repo_amd._lib import lib

    rs = np.random.RandomState(M + 3 * N + 7 * K)
    A = rnd(rs, K, M) if ta else rnd(rs, M, K)
    B = rnd(rs, N, K) if tb else rnd(rs, K, N)
    A[::7] *= 40.0      # a wide dynamic range inside every dot product
    bias = rnd(rs, (N + 24) // 25)
    opA, opB = (A.double().t() if ta else A.double()), (B.double().t() if tb else B.double())
    pre = opA @ opB + bias.double().repeat_interleave(25)[:N]
    mag = opA.abs() @ opB.abs()
    # k-contiguous operands as column slices of wider buffers: the leading dimension stays a multiple of 4 (what the
    # engine asks for) while K itself is ragged
    def widen(t):
        wide = torch.zeros(t.shape[0], (t.shape[1] + 7) // 4 * 4)
        wide[:, : t.shape[1]] = t
        return dev(wide)[:, : t.shape[1]]

    dA = dev(A) if ta else widen(A)
    dB = widen(B) if tb else dev(B)
    dbias = dev(bias)
    errs = {}
    for engine in (1, 0):
        prev = lib().repo_debug_bgemm(engine)
        try:
            got = ops.gemm(dA, dB, ta, tb, bias=dbias, bias_div=25, epi=ops.EPI_RELU)
            acc = torch.full((M, N), 0.5).cuda()
            ops.gemm(dA, dB, ta, tb, out=acc, accumulate=True)
        finally:
            lib().repo_debug_bgemm(prev)
        assert relerr(got, F.relu(pre)) < TOL
        assert relerr(acc, opA @ opB + 0.5) < TOL
        errs[engine] = float(((acc.double().cpu() - (opA @ opB + 0.5)).abs() / mag).max())
    log(f"bgemm ta={ta} tb={tb} {M}x{N}x{K}: max |err| / sum|a||b|  bf16x6 {errs[1]:.2e}  fp32 MFMA {errs[0]:.2e}")
    assert errs[1] <= 1.25 * errs[0] + 1e-9, errs


def _tile(*cfg):
    return r"TileCfg<" + r",\s*".join(str(c) for c in cfg) + ">"


# (id, ta, tb, M, N, K, engine kernel, its instantiation): the smallest shape that reaches each engine and tile of
# csrc/gemm.hip's dense_plan.  K = 36 / 20: vector loads; K = 17: odd, gathers; K = 130: the bf16x6 engine's shortest K,
# 176 tiles of 128 x 128 (>= 150) and 20 x 20 = 400 tiles of 256 x 128 with both edges ragged.
DENSE_ENGINE_CASES = [
    ("gemv-nt", False, True, 5, 60, 200, "gemv_small_kernel", r"gemv_small_kernel<true>"),
    ("gemv-nn", False, False, 5, 60, 200, "gemv_small_kernel", r"gemv_small_kernel<false>"),
    ("vec-32x128", False, True, 20, 60, 36, "vgemm_kernel", r"vgemm_kernel<.*VGemmOp<.*" + _tile(1, 4, 1, 1, 16, 2)),
    ("vec-64x64", False, True, 65, 129, 36, "vgemm_kernel", r"vgemm_kernel<.*VGemmOp<.*" + _tile(2, 2, 1, 1, 16, 2)),
    ("vec-128x128s1", False, True, 1536, 2048, 20, "vgemm_kernel", r"vgemm_kernel<.*VGemmOp<.*" + _tile(2, 2, 2, 2, 16, 1)),
    ("gather-32x128", False, True, 20, 60, 17, "igemm_kernel", r"igemm_kernel<.*GemmOp<.*" + _tile(1, 4, 1, 1, 16, 2)),
    ("gather-64x64", False, True, 65, 129, 17, "igemm_kernel", r"igemm_kernel<.*GemmOp<.*" + _tile(2, 2, 1, 1, 16, 2)),
    ("gather-128x128", False, True, 1536, 2048, 17, "igemm_kernel", r"igemm_kernel<.*GemmOp<.*" + _tile(2, 2, 2, 2, 16, 2)),
    ("bf16-mid", False, False, 1300, 1940, 130, "bgemm_kernel", r"bgemm_kernel<.*BgTile<128,\s*128,\s*32>"),
    ("bf16-big", False, True, 4865, 2450, 130, "bgemm_kernel", r"bgemm_kernel<.*BgTile<256,\s*128,\s*16>"),
]


@pytest.mark.parametrize("ta,tb,M,N,K,engine,kernel", [c[1:] for c in DENSE_ENGINE_CASES], ids=[c[0] for c in DENSE_ENGINE_CASES])
def test_gemm_every_engine_every_epilogue(ops, ta, tb, M, N, K, engine, kernel):
    """Every engine and tile dense_plan can choose, at the smallest shape that reaches it, with every epilogue it accepts,
    against fp64 (TOL: the fp32-accumulation bound at the top of this file) -- and the device trace of each call lists
    that engine's kernel and no other dense engine's.  k-contiguous operands, aux and the accumulate destination are
    column slices of wider buffers (leading dimensions that differ from the extents)."""
    rs = np.random.RandomState(M + 3 * N + 7 * K + tb)

    def sliced(t, lead=0):      # t as columns [lead, lead + cols) of a buffer whose row pitch is a multiple of 4
        wide = torch.zeros(t.shape[0], (lead + t.shape[1] + 7) // 4 * 4)
        wide[:, lead : lead + t.shape[1]] = t
        return dev(wide)[:, lead : lead + t.shape[1]]

    A = rnd(rs, K, M) if ta else rnd(rs, M, K)
    B = rnd(rs, N, K, scale=0.1) if tb else rnd(rs, K, N, scale=0.1)
    prod = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    dA, dB = (dev(A) if ta else sliced(A)), (sliced(B) if tb else dev(B))
    bias, bias25 = rnd(rs, N), rnd(rs, (N + 24) // 25)
    b25 = bias25.double().repeat_interleave(25)[:N]
    h = F.elu(rnd(rs, M, N))            # a saved ELU output: in (-1, inf), both signs
    hr = F.relu(h)                      # a saved ReLU output
    base = rnd(rs, M, N + 16)           # accumulate destination: columns [8, 8 + N) of it
    C = (N + 24) // 25
    table = torch.cat([1 + rnd(rs, M, C, scale=0.5), rnd(rs, M, C)], dim=1)      # FiLM: row m = [scale (C) | shift (C)]
    scale, shift = (table[:, i * C : (i + 1) * C].double().repeat_interleave(25, dim=1)[:, :N] for i in (0, 1))

    def check(what, want, **kw):
        out = kw.get("out")
        got, names = traced(lambda: ops.gemm(dA, dB, ta, tb, **kw))
        e = relerr(got, want)
        log(f"gemm engine {kernel} {M}x{N}x{K} {what}: relerr {e:.2e}")
        assert e < TOL, (what, e)
        assert has(names, kernel), (what, names)
        assert not any(has(names, rf"\b{k}\b") for k in set(DENSE_ENGINE_KERNELS) - {engine}), (what, names)
        return out

    dbias = dev(bias)
    check("none", prod + bias.double(), bias=dbias)
    check("elu", F.elu(prod + bias.double()), bias=dbias, epi=ops.EPI_ELU)
    check("relu", F.relu(prod + bias.double()), bias=dbias, epi=ops.EPI_RELU)
    check("mul_delu", prod * torch.where(h > 0, torch.ones_like(h), h + 1).double(), epi=ops.EPI_MUL_DELU, aux=sliced(h, 3))
    check("mul_drelu", prod * (hr > 0), epi=ops.EPI_MUL_DRELU, aux=sliced(hr, 3))
    check("bias_div 25", F.relu(prod + b25), bias=dev(bias25), bias_div=25, epi=ops.EPI_RELU)
    buf = dev(base)
    check("accumulate", prod + base[:, 8 : 8 + N].double(), out=buf[:, 8 : 8 + N], accumulate=True)
    assert torch.equal(buf[:, :8].cpu(), base[:, :8]) and torch.equal(buf[:, 8 + N :].cpu(), base[:, 8 + N :])
    if engine != "gemv_small_kernel":   # (repo_gemm keeps FiLM off the <= 8-row kernel)
        dtab = dev(table)
        check("film, bias per channel", F.relu(scale * (prod + b25) + shift), bias=dev(bias25), bias_div=25,
              epi=ops.EPI_FILM_RELU, aux=dtab)
        check("film, bias per column", F.relu(scale * (prod + bias.double()) + shift), bias=dbias, bias_div=-25,
              epi=ops.EPI_FILM_RELU, aux=dtab)


def test_bgemm_weight_gradient_without_slabs(ops):
    """repo_gemm_wgrad without a bias column at the decoder conv1's size takes the bf16x6 engine (one product, no
    split-K slabs): value, accumulate into a strided destination, and bit-reproducibility."""
    rs = np.random.RandomState(9)
    M, N, K = 2450, 1024, 3200
    dY, X = rnd(rs, M, N), rnd(rs, M, K)
    want = dY.double().t() @ X.double()
    dW, _ = ops.gemm_wgrad(dev(dY), dev(X), want_bias=False)
    assert relerr(dW, want) < TOL
    wide = torch.full((N, K + 8), 2.0).cuda()
    ops.gemm_wgrad(dev(dY), dev(X), dW=wide[:, 4 : 4 + K], db=None, accumulate=True, want_bias=False)
    assert relerr(wide[:, 4 : 4 + K], want + 2) < TOL
    assert float((wide[:, :4] - 2).abs().max()) == 0 and float((wide[:, 4 + K :] - 2).abs().max()) == 0
    again, _ = ops.gemm_wgrad(dev(dY), dev(X), want_bias=False)
    assert torch.equal(again, dW)


@pytest.mark.parametrize("M,N,K", [(2450, 200, 230), (50, 60, 200), (3000, 200, 1024), (7, 12, 200), (343, 1, 200)])
def test_gemm_wgrad(ops, M, N, K):
    rs = np.random.RandomState(M + N + K)
    dY, X = rnd(rs, M, N), rnd(rs, M, K)
    dW, db = ops.gemm_wgrad(dev(dY), dev(X))
    e1 = relerr(dW, dY.double().t() @ X.double())
    e2 = relerr(db, dY.double().sum(0))
    log(f"gemm_wgrad {M}x{N}x{K}: dW {e1:.2e} db {e2:.2e}")
    assert e1 < TOL and e2 < TOL
    # accumulate + strided destination (dW is a column block of a wider gradient)
    wide = torch.full((N, K + 50), 2.0).cuda()
    dbacc = torch.full((N,), 3.0).cuda()
    ops.gemm_wgrad(dev(dY), dev(X), dW=wide[:, 20 : 20 + K], db=dbacc, accumulate=True)
    assert relerr(wide[:, 20 : 20 + K], dY.double().t() @ X.double() + 2) < TOL
    assert relerr(dbacc, dY.double().sum(0) + 3) < TOL
    assert float((wide[:, :20] - 2).abs().max()) == 0


def test_gemm_nt_transposition_is_gated_like_the_engine(ops, monkeypatch):
    """ops.gemm / ops.gemm_wgrad make their transposing copy (the bf16x6 engine's NT form) only for products that engine
    takes and from operands repo_transpose accepts: N = 513 (ldb % 4 != 0), a misaligned view and a data-parallel
    shard's 637 rows (125 tiles < 150) stay on the untransposed forms -- and all of them still compute the product."""
    calls = []
    real = ops.transpose
    monkeypatch.setattr(ops, "transpose", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    rs = np.random.RandomState(11)

    def product(M, N, K, view=False):
        A, B = rnd(rs, M, K), rnd(rs, K, N + (1 if view else 0))
        Bd = dev(B)[:, 1:] if view else dev(B)      # view: same ld, data pointer 4 bytes off a 16-byte boundary
        Bh = B[:, 1:] if view else B
        got = ops.gemm(dev(A), Bd)
        assert relerr(got, A.double() @ Bh.double()) < TOL, (M, N, K, view)

    n0 = len(calls)
    product(2450, 3200, 1024)                  # the decoder's first layer: transposed
    assert len(calls) == n0 + 1
    for M, N, K, view in [(640, 513, 512, False), (2560, 1027, 512, True), (637, 3200, 1024, False), (600, 600, 100, False)]:
        n0 = len(calls)
        product(M, N, K, view)
        assert len(calls) == n0, (M, N, K, view, calls[n0:])
    # the switched-off engine: no copy either
    prev = ops.lib().repo_debug_bgemm(0)
    try:
        n0 = len(calls)
        product(2450, 3200, 1024)
        assert len(calls) == n0
    finally:
        ops.lib().repo_debug_bgemm(prev)
    # weight gradient without a bias column: both operands transposed, or none
    for M, N, K, want in [(2450, 1024, 3200, 2), (637, 1024, 3200, 2), (2450, 513, 640, 0)]:
        dY, X = rnd(rs, M, N), rnd(rs, M, K)
        n0 = len(calls)
        dW, _ = ops.gemm_wgrad(dev(dY), dev(X), want_bias=False)
        assert relerr(dW, dY.double().t() @ X.double()) < TOL, (M, N, K)
        assert len(calls) - n0 == want, (M, N, K, calls[n0:])


def test_debug_switches_follow_an_autograd_function_into_its_backward_thread(ops):
    """The repo_debug_* switches are thread-local; torch.autograd runs a Function's backward on its device thread.  The nn
    wrappers record the forward thread's settings and re-apply them around their backward (ops.debug_scope)."""
    import threading

    from repo_amd import functional as Fn
    from repo_amd.algorithms.repo.models.encoder import VisualEncoder

    torch.manual_seed(0)
    enc = VisualEncoder(1024).cuda()
    seen = {}
    real = Fn.encoder_bwd

    def spy(*a, **k):
        seen["thread"], seen["state"] = threading.get_ident(), ops.debug_snapshot()
        return real(*a, **k)

    prev = (ops.lib().repo_debug_scan_spin_limit(12345), ops.lib().repo_debug_bconv(0))
    try:
        Fn.encoder_bwd = spy
        want = ops.debug_snapshot()
        assert want[0] == 12345 and want[2] == 0
        out = enc(torch.rand(3, 3, 64, 64, device="cuda") - 0.5)
        out.sum().backward()
        torch.cuda.synchronize()
    finally:
        Fn.encoder_bwd = real
        ops.lib().repo_debug_scan_spin_limit(prev[0])
        ops.lib().repo_debug_bconv(prev[1])
    assert seen["state"] == want, (seen, want)
    assert ops.debug_snapshot()[0] == prev[0]
    if seen["thread"] != threading.get_ident():      # the backward thread is back on ITS defaults afterwards
        assert all(torch.isfinite(p.grad).all() for p in enc.parameters())


def _layer_tensors(ops, layer, nimg, seed):
    rs = np.random.RandomState(seed)
    (cb, hb, _), (cs, hs, _) = ops.conv_shapes(layer)
    ks = ops.CONV_GEO[layer][3]
    big = rnd(rs, nimg, cb, hb, hb)
    small = rnd(rs, nimg, cs, hs, hs)
    w = rnd(rs, cs, cb, ks, ks, scale=0.1)
    return big, small, w, rs


ALL_LAYERS = list(range(14))  # 0..6: the reference's 64 x 64 stack; 7..12: the build-defined 128 x 128 stack; 13: TIA conv4


@pytest.mark.parametrize("layer", ALL_LAYERS)
@pytest.mark.parametrize("nimg", [1, 5, 37])  # 37: pixel tiles that straddle several images / ragged last tile
def test_conv_down(ops, layer, nimg):
    if layer >= 7 and nimg == 37:
        nimg = 11
    big, small, w, rs = _layer_tensors(ops, layer, nimg, 100 + layer)
    cs = small.shape[1]
    bias = rnd(rs, cs)
    want = F.conv2d(big.double(), w.double(), bias.double(), stride=2)
    got = ops.conv_down(layer, dev(big), dev(w), dev(bias), epi=ops.EPI_RELU)
    e = relerr(got, F.relu(want))
    log(f"conv_down layer {layer} n={nimg}: {e:.2e}")
    assert e < TOL
    # backward-data form: no bias, masked by a saved activation
    h = F.relu(rnd(rs, *small.shape))
    got = ops.conv_down(layer, dev(big), dev(w), None, epi=ops.EPI_MUL_DRELU, aux=dev(h))
    assert relerr(got, F.conv2d(big.double(), w.double(), None, stride=2) * (h > 0)) < TOL


@pytest.mark.parametrize("nimg", [37, 600])   # 600: workgroups that take two or three images each (persistent grid), ragged
def test_conv_down_decoder_conv3_staging_and_multiplying_waves(ops, nimg):
    """Decoder conv3's data gradient from 32 images up runs on csrc/tconv_down.h (one persistent workgroup per CU: four waves
    stage image b + 1's channel chunks and the weight ring while four multiply image b): against fp64, without and with the
    ReLU mask of the saved activation, and the images must not leak into each other (an image's result is the same alone)."""
    layer = 5
    big, small, w, rs = _layer_tensors(ops, layer, nimg, 4100 + nimg)
    big[::7] *= 20.0
    want = F.conv2d(big.double(), w.double(), None, stride=2)
    got = ops.conv_down(layer, dev(big), dev(w), None, epi=ops.EPI_NONE)
    assert relerr(got, want) < TOL
    h = F.relu(rnd(rs, *small.shape))
    got_m = ops.conv_down(layer, dev(big), dev(w), None, epi=ops.EPI_MUL_DRELU, aux=dev(h))
    assert relerr(got_m, want * (h > 0)) < TOL
    assert torch.equal(got_m.cpu(), torch.where(h > 0, got.cpu(), torch.zeros(())))   # the mask selects, bit for bit
    sub = [0, 1, nimg // 2, nimg - 1] + list(range(3, 3 + 32))    # >= 32 images: the same kernel, other workgroup <-> image map
    got_s = ops.conv_down(layer, dev(big[sub]), dev(w), None, epi=ops.EPI_NONE)
    assert torch.equal(got_s.cpu(), got.cpu()[sub])


def test_conv_down_u8(ops):
    rs = np.random.RandomState(3)
    obs = torch.from_numpy(rs.randint(0, 256, size=(6, 3, 64, 64)).astype(np.uint8))
    w, b = rnd(rs, 32, 3, 4, 4, scale=0.1), rnd(rs, 32)
    x = ((obs.numpy().astype(np.float32) / 255) * 2) - 1.0
    want = F.relu(F.conv2d(torch.from_numpy(x).double(), w.double(), b.double(), stride=2))
    got = ops.conv_down(ops.ENC1, dev(obs), dev(w), dev(b), epi=ops.EPI_RELU)
    assert relerr(got, want) < TOL


@pytest.mark.parametrize("layer", ALL_LAYERS)
@pytest.mark.parametrize("nimg", [1, 5, 37])
def test_conv_up(ops, layer, nimg):
    if layer >= 7 and nimg == 37:
        nimg = 11
    big, small, w, rs = _layer_tensors(ops, layer, nimg, 200 + layer)
    cb = big.shape[1]
    bias = rnd(rs, cb)
    hb = big.shape[2]

    def up(bias_):
        # encoder conv2 (31 -> 14) never reads the last input row/col, so its backward-data
        # (the "up" form) leaves them at zero: pad torch's 30x30 result to the 31x31 buffer
        r = F.conv_transpose2d(small.double(), w.double(), None, stride=2)
        r = F.pad(r, (0, hb - r.shape[3], 0, hb - r.shape[2]))
        return r if bias_ is None else r + bias_.double().view(1, -1, 1, 1)

    want = up(bias)
    got = ops.conv_up(layer, dev(small), dev(w), dev(bias), epi=ops.EPI_RELU)
    e = relerr(got, F.relu(want))
    log(f"conv_up layer {layer} n={nimg}: {e:.2e}")
    assert e < TOL
    h = F.relu(rnd(rs, *big.shape))
    got = ops.conv_up(layer, dev(small), dev(w), None, epi=ops.EPI_MUL_DRELU, aux=dev(h))
    assert relerr(got, up(None) * (h > 0)) < TOL
    got = ops.conv_up(layer, dev(small), dev(w), dev(bias))
    assert relerr(got, want) < TOL


@pytest.mark.parametrize("nimg", [4, 600])
def test_conv_up_gather_form_many_images_per_workgroup(ops, nimg):
    """Encoder conv2's data gradient in gather form (csrc/tconv_up.h) where a workgroup walks SEVERAL images (600 images: three
    per workgroup, the accumulators and the weight / relu-operand prefetch carried across images, the last workgroup ragged)
    and at its smallest batch: all three of its epilogues against fp64, the mask and activation forms bit-identical."""
    import repo_amd.ops as rops
    layer = 1
    big, small, w, rs = _layer_tensors(ops, layer, nimg, 321)
    hb = big.shape[2]
    r = F.conv_transpose2d(small.double(), w.double(), None, stride=2)
    want = F.pad(r, (0, hb - r.shape[3], 0, hb - r.shape[2]))
    bias = rnd(rs, big.shape[1])
    got = ops.conv_up(layer, dev(small), dev(w), dev(bias))
    assert relerr(got, want + bias.double().view(1, -1, 1, 1)) < TOL
    h = F.relu(rnd(rs, *big.shape))
    a = ops.conv_up(layer, dev(small), dev(w), None, epi=ops.EPI_MUL_DRELU, aux=dev(h))
    assert relerr(a, want * (h > 0)) < TOL
    bits = (h > 0).to(torch.uint8).view(nimg, -1, 4, hb * hb)   # channel-quad mask: byte (image, quad, pixel), bit = channel & 3
    cmask = (bits[:, :, 0] | (bits[:, :, 1] << 1) | (bits[:, :, 2] << 2) | (bits[:, :, 3] << 3)).contiguous().view(-1)
    m = ops.conv_up(layer, dev(small), dev(w), None, epi=rops.EPI_MUL_CMASK, aux=dev(cmask))
    assert torch.equal(a, m)


# (layer, pass, images, the kernel a device trace must show with repo_debug_bconv on).  41 images fill several pixel tiles
# and straddle images; where conv.hip's plans hand 41 images of that call to another engine, the count that keeps the
# call on the kernel the case is about: decoder conv3's plain data gradient goes to tconv_down.h from 32 images (29),
# encoder conv4's 2 x 2 planes stay on the latency tiles up to 128 images (150); encoder conv2's plain data gradient goes
# to tconv_up.h from 4 images, so its buconv.h case keeps the 41 images and takes the epilogue that stays there (ReLU with
# bias: the decoder's forward form).  Those engines have cases of their own (-tcd, -tcu); both weight gradients on the
# transposing engine are twgrad.h's (decoder conv3 on bwgrad.h is shadowed by it in the default build).
_BF16X6_CASES = [
    pytest.param(5, "down", 29, "bconv_down_kernel", id="5-down"), pytest.param(1, "down", 41, "bconv_down_kernel", id="1-down"),
    pytest.param(2, "down", 41, "bconv_down_kernel", id="2-down"), pytest.param(3, "down", 150, "bconv_down_kernel", id="3-down"),
    pytest.param(4, "down", 41, "bconv_down_kernel", id="4-down"), pytest.param(5, "up", 41, "buconv_scatter_kernel", id="5-up"),
    pytest.param(1, "up", 41, "buconv_scatter_kernel", id="1-up"), pytest.param(2, "up", 41, "buconv_scatter_kernel", id="2-up"),
    pytest.param(3, "up", 41, "buconv_scatter_kernel", id="3-up"), pytest.param(4, "up", 41, "buconv_scatter_kernel", id="4-up"),
    pytest.param(5, "wgrad", 41, "tconv_wgrad_kernel", id="5-wgrad"), pytest.param(2, "wgrad", 41, "bconv_wgrad_kernel", id="2-wgrad"),
    pytest.param(1, "wgrad", 41, "tconv_wgrad_kernel", id="1-wgrad"),
    pytest.param(5, "down", 41, "tconv_down_kernel", id="5-down-tcd"), pytest.param(1, "up", 41, "tconv_up_kernel", id="1-up-tcu"),
]
_BF16X6_FP32_TWIN = {"down": "dconv_down_kernel", "up": "uconv_scatter_kernel", "wgrad": "dconv_wgrad_kernel"}


@pytest.mark.parametrize("layer,kind,nimg,kernel", _BF16X6_CASES)
def test_bf16x6_conv_kernels_match_fp64_and_the_fp32_kernels(ops, layer, kind, nimg, kernel):
    """The bf16x6 conv kernels (csrc/bconv.h: decoder conv3 / conv2 data gradients, encoder conv2 / conv3 / conv4 forward;
    csrc/buconv.h: decoder conv3 / conv2 forward, encoder conv2 / conv3 / conv4 data gradients; csrc/bwgrad.h: encoder conv3's
    weight gradient; csrc/twgrad.h: decoder conv3's and encoder conv2's; csrc/tconv_down.h and csrc/tconv_up.h: the -tcd / -tcu
    cases) against fp64 at a batch that fills several
    pixel tiles and straddles images -- and against the fp32-MFMA kernel of the same layer on the SAME operands
    (repo_debug_bconv(0)): the error relative to sum |a||b| may not exceed that kernel's by more than 25 % (measured: at or
    below it), i.e. the six-product split is an fp32-accurate way of feeding the bf16 pipe, not a reduced precision.  A
    device trace shows that the kernel the case names ran, and its fp32 twin with the switch off."""
    from repo_amd._lib import lib

    big, small, w, rs = _layer_tensors(ops, layer, nimg, 900 + layer)
    big[::3] *= 25.0
    small[::3] *= 25.0
    if kind == "down":
        want = F.conv2d(big.double(), w.double(), None, stride=2)
        mag = F.conv2d(big.double().abs(), w.double().abs(), None, stride=2)
        run = lambda: ops.conv_down(layer, dev(big), dev(w), None, epi=ops.EPI_NONE)  # noqa: E731
    elif kind == "wgrad":
        def corr(a, b):   # dw[cs][cb][ky][kx] = sum_n corr(small, big)
            ks = w.shape[-1]
            cols = F.unfold(b, ks, stride=2).view(b.shape[0], b.shape[1], ks * ks, -1)       # (n, cb, kk, pix)
            return torch.einsum("nsp,nckp->sck", a.flatten(2), cols).view(a.shape[1], b.shape[1], ks, ks)

        want = corr(small.double(), big.double())
        mag = corr(small.double().abs(), big.double().abs())
        run = lambda: ops.conv_wgrad(layer, dev(small), dev(big), want_bias=False)[0]  # noqa: E731
    else:
        hb = big.shape[2]
        pad = lambda r: F.pad(r, (0, hb - r.shape[3], 0, hb - r.shape[2]))  # noqa: E731
        want = pad(F.conv_transpose2d(small.double(), w.double(), None, stride=2))
        mag = pad(F.conv_transpose2d(small.double().abs(), w.double().abs(), None, stride=2)) + 1e-30
        run = lambda: ops.conv_up(layer, dev(small), dev(w), None, epi=ops.EPI_NONE)  # noqa: E731
        if (layer, kernel) == (1, "buconv_scatter_kernel"):   # ReLU with bias: the |bias| joins the magnitude
            bias = rnd(rs, big.shape[1])
            want = F.relu(want + bias.double().view(1, -1, 1, 1))
            mag = mag + bias.double().abs().view(1, -1, 1, 1)
            run = lambda: ops.conv_up(layer, dev(small), dev(w), dev(bias), epi=ops.EPI_RELU)  # noqa: E731
    errs = {}
    for engine in (1, 0):
        prev = lib().repo_debug_bconv(engine)
        try:
            got, names = traced(run)
        finally:
            lib().repo_debug_bconv(prev)
        ran = kernel if engine else _BF16X6_FP32_TWIN[kind]
        assert has(names, rf"\b{ran}\b"), (layer, kind, nimg, engine, names)
        assert not any(has(names, rf"\b{k}\b") for k in set(CONV_ENGINE_KERNELS) - {ran}), (layer, kind, nimg, engine, names)
        assert relerr(got, want) < TOL
        errs[engine] = float(((got.double().cpu() - want).abs() / (mag + 1e-30)).max())
    log(f"bf16x6 conv layer {layer} {kind}: max |err| / sum|a||b|  bf16x6 {errs[1]:.2e}  fp32 MFMA {errs[0]:.2e}")
    assert errs[1] <= 1.25 * errs[0] + 1e-9, errs


@pytest.mark.parametrize("layer", ALL_LAYERS)
@pytest.mark.parametrize("nimg", [1, 9, 75])  # 75: several image groups per split, ragged last group and split
def test_conv_wgrad(ops, layer, nimg):
    if layer >= 7 and nimg == 75:
        nimg = 21
    big, small, w, rs = _layer_tensors(ops, layer, nimg, 300 + layer)
    bigd = big.double().requires_grad_(False)
    wd = w.double().requires_grad_(True)
    out = F.conv2d(bigd, wd, None, stride=2)
    (out * small.double()).sum().backward()
    dw, db = ops.conv_wgrad(layer, dev(small), dev(big))
    e1 = relerr(dw, wd.grad)
    e2 = relerr(db, small.double().sum((0, 2, 3)))
    log(f"conv_wgrad layer {layer} n={nimg}: dw {e1:.2e} db {e2:.2e}")
    assert e1 < TOL and e2 < TOL
    dw2 = torch.ones_like(dw)
    ops.conv_wgrad(layer, dev(small), dev(big), dw=dw2, db=None, accumulate=True, want_bias=False)
    assert relerr(dw2, wd.grad + 1) < TOL


@pytest.mark.parametrize("layer", [1, 2, 4, 5, 6])
@pytest.mark.parametrize("nimg", [3, 300])
def test_conv_wgrad_channel_sums_of_big(ops, layer, nimg):
    """repo_conv_wgrad's dbias_big: the channel sums of `big` (the bias gradient of a transposed conv) -- fused into the
    weight-gradient kernel where it stages every element once (decoder conv3: 300 images are 3 per workgroup pair, ragged),
    the channel-sum pass elsewhere; the same numbers from both engines, with and without accumulation."""
    from repo_amd._lib import lib

    big, small, w, rs = _layer_tensors(ops, layer, nimg, 700 + layer)
    want = big.double().sum((0, 2, 3))
    for engine in (1, 0):
        prev = lib().repo_debug_bconv(engine)
        try:
            dbig = torch.full((big.shape[1],), 2.0, device="cuda")
            dw, _ = ops.conv_wgrad(layer, dev(small), dev(big), want_bias=False, dbig=dbig, accumulate=False)
            assert relerr(dbig, want) < TOL
            dw2 = dw.clone()
            ops.conv_wgrad(layer, dev(small), dev(big), dw=dw2, db=None, want_bias=False, dbig=dbig, accumulate=True)
            assert relerr(dbig, 2 * want) < TOL and relerr(dw2, 2 * dw.double().cpu()) < TOL
        finally:
            lib().repo_debug_bconv(prev)


def test_conv_wgrad_u8(ops):
    rs = np.random.RandomState(4)
    obs = torch.from_numpy(rs.randint(0, 256, size=(7, 3, 64, 64)).astype(np.uint8))
    x = torch.from_numpy(((obs.numpy().astype(np.float32) / 255) * 2) - 1.0).double()
    small = rnd(rs, 7, 32, 31, 31)
    wd = torch.zeros(32, 3, 4, 4, dtype=torch.float64, requires_grad=True)
    (F.conv2d(x, wd, None, stride=2) * small.double()).sum().backward()
    dw, db = ops.conv_wgrad(ops.ENC1, dev(small), dev(obs))
    assert relerr(dw, wd.grad) < TOL


@pytest.mark.parametrize("u8,nimg", [(True, 6), (False, 6), (True, 300)])  # 300 images: persistent tile loop
def test_decoder_out_nll(ops, u8, nimg):
    rs = np.random.RandomState(9)
    h3 = F.relu(rnd(rs, nimg, 32, 30, 30))
    w, b = rnd(rs, 32, 3, 6, 6, scale=0.05), rnd(rs, 3)
    obs = torch.from_numpy(rs.randint(0, 256, size=(nimg, 3, 64, 64)).astype(np.uint8))
    tgt = torch.from_numpy(((obs.numpy().astype(np.float32) / 255) * 2) - 1.0)
    recon = F.conv_transpose2d(h3.double(), w.double(), b.double(), stride=2)
    d = recon - tgt.double()
    loss, dpre, rec = ops.decoder_out_nll(dev(h3), dev(w), dev(b), dev(obs if u8 else tgt), 0.25, want_recon=True)
    e0, e1, e2 = relerr(rec, recon), relerr(dpre, d * 0.25), abs(loss.item() - (0.5 * d * d).sum().item()) / (0.5 * d * d).sum().item()
    log(f"decoder_out_nll u8={u8}: recon {e0:.2e} dpre {e1:.2e} loss {e2:.2e}")
    assert e0 < TOL and e1 < TOL and e2 < 1e-5
    # the quad mask of h3 (REPO_EPI_MUL_MASK4): bit (o & 3) of byte (o >> 2) is h3.flat[o] > 0, every byte written
    sentinel = torch.full((h3.numel() // 4,), 0xAA, dtype=torch.uint8)
    import repo_amd.ops as rops
    loss2, dpre2, _, mask = ops.decoder_out_nll(dev(h3), dev(w), dev(b), dev(obs if u8 else tgt), 0.25, want_mask=True)
    assert mask.dtype == torch.uint8 and mask.numel() == h3.numel() // 4
    bits = (h3.reshape(-1, 4) > 0).to(torch.uint8)
    want = bits[:, 0] | (bits[:, 1] << 1) | (bits[:, 2] << 2) | (bits[:, 3] << 3)
    assert torch.equal(mask.cpu(), want)
    assert torch.equal(dpre2, dpre) and loss2.item() == loss.item()
    # dbias: the channel sums of dpre (the output layer's bias gradient), both engines, overwrite and accumulate
    from repo_amd._lib import lib
    for engine in (1, 0):
        prev = lib().repo_debug_bconv(engine)
        try:
            db = torch.full((3,), 5.0, device="cuda")
            ops.decoder_out_nll(dev(h3), dev(w), dev(b), dev(obs if u8 else tgt), 0.25, dbias=db)
            assert relerr(db, (d * 0.25).sum((0, 2, 3))) < 2e-5
            ops.decoder_out_nll(dev(h3), dev(w), dev(b), dev(obs if u8 else tgt), 0.25, dbias=db, accumulate_dbias=True)
            assert relerr(db, 2 * (d * 0.25).sum((0, 2, 3))) < 2e-5
        finally:
            lib().repo_debug_bconv(prev)
    # ... and the data gradient that reads it equals the one that reads h3 itself, bit for bit
    d4 = dev(rnd(rs, nimg, 3, 64, 64))
    a = ops.conv_down(rops.DEC4, d4, dev(w), None, epi=rops.EPI_MUL_DRELU, aux=dev(h3))
    m = ops.conv_down(rops.DEC4, d4, dev(w), None, epi=rops.EPI_MUL_MASK4, aux=mask)
    assert torch.equal(a, m)
    assert float((a == 0).float().mean()) > 0.3  # the mask really masks
    del sentinel


@pytest.mark.parametrize("layer", ALL_LAYERS)
def test_conv_down_channel_sums(ops, layer):
    """repo_conv_down's dbias: the per-channel sum of the values it writes (the bias gradient of the transposed-conv
    layer below, taken in the epilogue) == a second pass over the output; throughput and latency tiles (<= 512
    output pixels), ragged last tiles, accumulation, run-to-run bit-identical."""
    import repo_amd.ops as rops
    rs = np.random.RandomState(70 + layer)
    (cb, hb, _), (cs, hs, _) = rops.conv_shapes(layer)
    ks = rops.CONV_GEO[layer][3]
    for nimg in (1, 9):
        big = dev(rnd(rs, nimg, cb, hb, hb))
        w = dev(rnd(rs, cs, cb, ks, ks, scale=0.1))
        h = dev(F.relu(rnd(rs, nimg, cs, hs, hs)))
        db = torch.full((cs,), 3.0, device="cuda")
        out = ops.conv_down(layer, big, w, None, epi=rops.EPI_MUL_DRELU, aux=h, dbias=db, accumulate_dbias=True)
        want = out.double().sum((0, 2, 3)) + 3.0
        assert relerr(db, want) < TOL, (layer, nimg, relerr(db, want))
        db2 = torch.empty(cs, device="cuda")
        out2 = ops.conv_down(layer, big, w, None, epi=rops.EPI_MUL_DRELU, aux=h, dbias=db2)
        db3 = torch.empty(cs, device="cuda")
        ops.conv_down(layer, big, w, None, epi=rops.EPI_MUL_DRELU, aux=h, dbias=db3)
        assert torch.equal(out2, out) and torch.equal(db2, db3)
        assert relerr(db2, out.double().sum((0, 2, 3))) < TOL


@pytest.mark.parametrize("layer", [1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12])
def test_conv_down_quad_mask_any_geometry(ops, layer):
    """REPO_EPI_MUL_MASK4 on every geometry (pixel planes of 196, 36, 4, 25, 169 and 900 elements: quads that are
    unaligned in the mask's bytes and quads that run over an image's end) equals REPO_EPI_MUL_DRELU bit for bit."""
    import repo_amd.ops as rops
    rs = np.random.RandomState(40 + layer)
    (cb, hb, _), (cs, hs, _) = rops.conv_shapes(layer)
    ks = rops.CONV_GEO[layer][3]
    for nimg in (1, 7):
        big = dev(rnd(rs, nimg, cb, hb, hb))
        w = dev(rnd(rs, cs, cb, ks, ks, scale=0.1))
        h = F.relu(rnd(rs, nimg, cs, hs, hs))
        flat = h.reshape(-1)
        pad = (-flat.numel()) % 4
        bits = (torch.cat([flat, torch.zeros(pad)]).reshape(-1, 4) > 0).to(torch.uint8)
        mask = (bits[:, 0] | (bits[:, 1] << 1) | (bits[:, 2] << 2) | (bits[:, 3] << 3)).cuda()
        a = ops.conv_down(layer, big, w, None, epi=rops.EPI_MUL_DRELU, aux=dev(h))
        m = ops.conv_down(layer, big, w, None, epi=rops.EPI_MUL_MASK4, aux=mask)
        assert torch.equal(a, m), (layer, nimg)


@pytest.mark.parametrize("layer", [0, 1, 2])
@pytest.mark.parametrize("engine", [1, 0], ids=["bf16x6", "fp32"])
def test_channel_quad_mask_written_by_conv_down_read_by_conv_up(ops, layer, engine):
    """REPO_EPI_MUL_CMASK: the encoder layer's forward writes the channel-quad mask of its ReLU from the accumulators
    (repo_conv_down relu_cmask: byte ((n * C/4 + c/4) * P + p), bit c % 4 <=> relu > 0), the data gradient of the
    layer above (repo_conv_up on the scatter kernels: enc2 / enc3 / enc4, 961- / 196- / 36-pixel planes, both
    drains) multiplies by it: the mask equals the activation's signs and the gradient equals REPO_EPI_MUL_DRELU's bit
    for bit; ragged image counts; a 3-channel layer has no channel quads (REPO_E_BADARG)."""
    import repo_amd.ops as rops
    from repo_amd._lib import RepoHipError, lib

    rs = np.random.RandomState(90 + layer)
    (cb, hb, _), (cs, hs, _) = rops.conv_shapes(layer)
    ks = rops.CONV_GEO[layer][3]
    up = layer + 1   # the layer whose data gradient lands on this layer's output
    (ucb, uhb, _), (ucs, uhs, _) = rops.conv_shapes(up)
    assert (ucb, uhb) == (cs, hs)
    uks = rops.CONV_GEO[up][3]
    prev = lib().repo_debug_bconv(engine)
    try:
        for nimg in (1, 5, 37):
            big = dev(rnd(rs, nimg, cb, hb, hb))
            w = dev(rnd(rs, cs, cb, ks, ks, scale=0.2))
            b = dev(rnd(rs, cs, scale=0.1))
            h, cmask = ops.conv_down(layer, big, w, b, epi=rops.EPI_RELU, want_cmask=True)
            assert torch.equal(h, ops.conv_down(layer, big, w, b, epi=rops.EPI_RELU))
            bits = (h > 0).to(torch.uint8).view(nimg, cs // 4, 4, hs * hs)
            want = bits[:, :, 0] | (bits[:, :, 1] << 1) | (bits[:, :, 2] << 2) | (bits[:, :, 3] << 3)
            assert torch.equal(cmask.view(nimg, cs // 4, hs * hs), want), (layer, nimg)
            assert 0.2 < float((h > 0).float().mean()) < 0.8
            d = dev(rnd(rs, nimg, ucs, uhs, uhs))
            uw = dev(rnd(rs, ucs, ucb, uks, uks, scale=0.1))
            a = ops.conv_up(up, d, uw, None, epi=rops.EPI_MUL_DRELU, aux=h)
            m = ops.conv_up(up, d, uw, None, epi=rops.EPI_MUL_CMASK, aux=cmask)
            assert torch.equal(a, m), (layer, nimg)
    finally:
        lib().repo_debug_bconv(prev)
    if layer == 0:
        with pytest.raises(RepoHipError):   # the 3-channel data gradient runs on the gather engine: no channel quads
            ops.conv_up(0, dev(rnd(rs, 1, 32, 31, 31)), dev(rnd(rs, 32, 3, 4, 4)), None, epi=rops.EPI_MUL_CMASK,
                        aux=torch.zeros(64, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("layer,u8", [(6, True), (6, False), (12, True), (12, False)])
def test_conv_up_nll(ops, layer, u8):
    """The gather engine's fused output layer + pixel NLL (layer 12: the 128 x 128 stack's; layer 6: a second
    implementation of repo_decoder_out_nll) vs fp64 torch, and at layer 6 vs the specialised kernel."""
    import repo_amd.ops as rops
    rs = np.random.RandomState(60 + layer)
    (cb, hb, _), (cs, hs, _) = rops.conv_shapes(layer)
    ks = rops.CONV_GEO[layer][3]
    nimg = 5
    h = F.relu(rnd(rs, nimg, cs, hs, hs))
    w, b = rnd(rs, cs, cb, ks, ks, scale=0.05), rnd(rs, cb)
    obs = torch.from_numpy(rs.randint(0, 256, size=(nimg, cb, hb, hb)).astype(np.uint8))
    tgt = torch.from_numpy(((obs.numpy().astype(np.float32) / 255) * 2) - 1.0)
    recon = F.conv_transpose2d(h.double(), w.double(), b.double(), stride=2)
    d = recon - tgt.double()
    loss, dpre, rec = ops.conv_up_nll(layer, dev(h), dev(w), dev(b), dev(obs if u8 else tgt), 0.25, want_recon=True)
    want_loss = (0.5 * d * d).sum().item()
    assert relerr(rec, recon) < TOL and relerr(dpre, d * 0.25) < TOL and abs(loss.item() - want_loss) / want_loss < 1e-5
    if layer == 6:
        loss2, dpre2, rec2 = ops.decoder_out_nll(dev(h), dev(w), dev(b), dev(obs if u8 else tgt), 0.25, want_recon=True)
        assert relerr(rec2, rec.double()) < TOL and relerr(dpre2, dpre.double()) < TOL


def test_channel_sum_relu_mask(ops):
    rs = np.random.RandomState(1)
    x = rnd(rs, 37, 3, 64, 64)
    assert relerr(ops.channel_sum(dev(x)), x.double().sum((0, 2, 3))) < TOL
    x = rnd(rs, 50, 128, 25)
    acc = torch.ones(128).cuda()
    ops.channel_sum(dev(x), out=acc, accumulate=True)
    assert relerr(acc, x.double().sum((0, 2)) + 1) < TOL
    dy, h = rnd(rs, 1000, 33), F.relu(rnd(rs, 1000, 33))
    assert float((ops.relu_mask(dev(dy), dev(h)).cpu() - dy * (h > 0)).abs().max()) == 0


def test_no_uninitialised_lds(ops):
    """Every direct-conv / GEMM kernel must give the same bits after the LDS of all CUs has been filled
    with NaN patterns: a kernel that reads LDS it did not write (even to multiply it by zero) fails here
    deterministically instead of once in a dozen runs."""
    from repo_amd._lib import lib

    def poison():
        assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0

    rs = np.random.RandomState(77)
    for layer in range(7):
        for nimg in (3, 37):
            big, small, w, _ = _layer_tensors(ops, layer, nimg, 900 + layer)
            big, small, w = dev(big), dev(small), dev(w)
            outs = []
            for p in (False, True):
                if p:
                    poison()
                d = ops.conv_down(layer, big, w)
                if p:
                    poison()
                u = ops.conv_up(layer, small, w)
                if p:
                    poison()
                dw, db = ops.conv_wgrad(layer, small, big)
                outs.append((d, u, dw, db))
            for a, b in zip(*outs):
                assert torch.isfinite(b).all(), (layer, nimg)
                assert torch.equal(a, b), (layer, nimg)
    h3, w4, b4 = dev(rnd(rs, 9, 32, 30, 30)), dev(rnd(rs, 32, 3, 6, 6, scale=0.05)), dev(rnd(rs, 3))
    tgt = dev(torch.from_numpy(rs.randint(0, 256, size=(9, 3, 64, 64)).astype(np.uint8)))
    ref = ops.decoder_out_nll(h3, w4, b4, tgt, 0.5)
    poison()
    got = ops.decoder_out_nll(h3, w4, b4, tgt, 0.5)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
    for (M, N, K) in ((333, 200, 230), (70, 1024, 36), (500, 7, 1)):
        A, B = dev(rnd(rs, M, K)), dev(rnd(rs, K, N))
        ref = ops.gemm(A, B)
        poison()
        assert torch.equal(ref, ops.gemm(A, B))
        dy = dev(rnd(rs, M, N))
        r1 = ops.gemm_wgrad(dy, A)
        poison()
        r2 = ops.gemm_wgrad(dy, A)
        assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


def test_no_uninitialised_lds_row_tile_kernels(ops):
    """The persistent row-tile kernels (rollout forward / reverse on both engines, the fused heads) after the LDS of every
    CU has been filled with NaN patterns: same bits as before -- their tiles' padding columns meet zero weights, so they
    must hold finite values the kernels wrote themselves."""
    from repo_amd._lib import lib
    from oracle import fixtures as fx

    def poison():
        assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0

    rs = np.random.RandomState(78)
    Hm, N, A, D, S = 3, 75, 6, 200, 30
    P = fx.make_params(A, 7)
    rp = [torch.tensor(v).cuda() for v in P["transition_model"].values()]
    ap = [torch.tensor(v).cuda() for v in P["actor_model"].values()]
    vp = [torch.tensor(v).cuda() for v in P["value_model"].values()]
    b0, s0 = dev(rnd(rs, N, D, scale=0.3)), dev(rnd(rs, N, S))
    ea, ep = dev(rnd(rs, Hm, N, A)), dev(rnd(rs, Hm, N, S))
    dfeat = dev(rnd(rs, Hm, N, D + S, scale=0.01))
    for engine in (1, 0):
        prev = lib().repo_debug_rowtile32(engine)
        try:
            outs = []
            for p in (False, True):
                if p:
                    poison()
                sv = ops.rssm_imagine_fwd(rp, ap, b0, s0, ea, ep)
                if p:
                    poison()
                d_araw, dfeat0 = ops.rssm_imagine_bwd(rp, sv, dfeat, want_dfeat0=True)
                outs.append((sv.featx.clone(), sv.gates.clone(), sv.a_hidden.clone(), d_araw.clone(), dfeat0.clone()))
            for a, b in zip(*outs):
                assert torch.isfinite(b).all() and torch.equal(a, b), engine
        finally:
            lib().repo_debug_rowtile32(prev)
    x = dev(rnd(rs, 1000, D + S))
    ref, rh = ops.mlp_fwd(vp, x)
    dx_ref = torch.empty_like(x)
    ops.mlp_bwd(vp, x, rh, dev(rnd(np.random.RandomState(1), 1000, 1)), dparams=None, dx=dx_ref)
    poison()
    got, gh = ops.mlp_fwd(vp, x)
    poison()
    dx = torch.empty_like(x)
    ops.mlp_bwd(vp, x, gh, dev(rnd(np.random.RandomState(1), 1000, 1)), dparams=None, dx=dx)
    assert torch.equal(ref, got) and all(torch.equal(a, b) for a, b in zip(rh, gh)) and torch.equal(dx_ref, dx)


def test_device_check_and_arch_guard():
    """repo_device_check: the MI355X passes, an ordinal that does not exist is a bad argument; every entry
    point runs the same (cached) check before launching (REPO_E_ARCH on anything that is not gfx950)."""
    from repo_amd._lib import lib

    L = lib()
    assert L.repo_device_check(0) == 0
    assert L.repo_device_check(torch.cuda.device_count()) == -1  # REPO_E_BADARG
    assert L.repo_strerror(-5).decode() == "device is not gfx950"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


# ----------------------------------------------------------------------------- the decoder through its composed head
# From functional._DEC_COMPOSE_MIN_ROWS rows up the decoder's fc1 and its 1x1 -> 5x5 transposed conv1 run as ONE layer
# (functional.dec_head_compose: W01 = W1^T W0, its bias column padded to DecHead.pad) and their gradients come out of
# (G | s) = d1^T (feat | 1).  These tests run the whole decoder at composing row counts and latent widths against the
# reference's TWO-layer form (oracle/repo_oracle.py: decoder_fwd / cond_decoder_fwd) in float64, tensor by tensor, with
# the same shapes under REPO_DEC_COMPOSE=0 so that both forms stay pinned.
def _dec64(P, feat, gates=None, film=None):
    """float64 restatement of oracle decoder_fwd (film = (gammas, betas): cond_decoder_fwd) -> (fc1 output, [h1, h2, ...],
    output layer).  gates: None (ReLU), or one fixed 0/1 tensor per ReLU -- the GPU forward's own `h > 0` -- so that a
    pre-activation within rounding of zero takes the GPU's side of the ReLU in the backward."""
    rows = feat.shape[0]
    h0 = F.linear(feat, P["fc1.weight"], P["fc1.bias"])
    x = h0.view(rows, -1, 1, 1)
    convs = [k[: -len(".weight")] for k in P if k.startswith("conv") and k.endswith(".weight")]
    hs = []
    for i, name in enumerate(convs[:-1]):
        pre = F.conv_transpose2d(x, P[f"{name}.weight"], P[f"{name}.bias"], stride=2)
        if film is not None:
            pre = (1 + film[0][i][..., None, None]) * pre + film[1][i][..., None, None]
        x = F.relu(pre) if gates is None else pre * gates[i]
        hs.append(x)
    return h0, hs, F.conv_transpose2d(x, P[f"{convs[-1]}.weight"], P[f"{convs[-1]}.bias"], stride=2)


def _dec_case_params(F_, image, tia, seed):
    from oracle import fixtures as fx

    # fc1 is F_ = belief + state wide; the remaining modules are drawn too (make_params' order) and not used here
    return fx.make_params(6, seed, image=image, tia=tia, belief=F_ - 30, state=30)["obs_model"]


def _dec_frames(rs, rows, image):
    u8 = torch.from_numpy(rs.randint(0, 256, size=(rows, 3, image, image)).astype(np.uint8))
    return u8, (u8.double() / 255) * 2 - 1


DEC_CASES = [
    # (rows, F = belief + state, stack): 511 stays two-layer, 512 is the first composing row count, 637 a data-parallel
    # shard's, 2450 the headline update's; F 229 / 231: odd K into the padded leading dimension; 232 / 264: a pad past 232
    (511, 230, "64"), (512, 230, "64"), (637, 230, "64"), (2450, 230, "64"),
    (512, 130, "64"), (512, 229, "64"), (512, 231, "64"), (512, 232, "64"), (512, 264, "64"),
    (512, 230, "128"),   # the build-defined 128 x 128 stack (12 tensors: functional._decoder_bwd_128)
    (512, 230, "tia"),   # TIA's 6-channel output layer (T_DEC4; decoder_fwd + an outside cotangent, as tia.py runs it)
]


@pytest.mark.parametrize("compose", ["1", "0"])
@pytest.mark.parametrize("rows,F_,stack", DEC_CASES)
def test_decoder_matches_fp64_two_layer_form_per_tensor(ops, monkeypatch, rows, F_, stack, compose):
    """Fn.decoder_fwd(_nll) / Fn.decoder_bwd against fp64 autograd of the two-layer decoder: every activation, the
    output, the NLL and its gradient, each of the ten (twelve) parameter gradients and d feat, each within TOL; then the
    same backward accumulating into pre-filled gradients, on a side stream (RePo's call) and deferred (Dreamer's call) --
    the last two bit-identical to the serial run."""
    import repo_amd.functional as Fn

    monkeypatch.setenv("REPO_DEC_COMPOSE", compose)
    image, tia = (128 if stack == "128" else 64), stack == "tia"
    rs = np.random.RandomState(rows + 7 * F_ + len(stack))
    P = _dec_case_params(F_, image, tia, seed=rows + F_)
    p = [dev(torch.from_numpy(v)) for v in P.values()]
    feat = rnd(rs, rows, F_, scale=0.7)
    u8, tgt = _dec_frames(rs, rows, image)
    gs = 1.0 / rows
    # -- forward (the GPU's), then the engagement of the composed head
    if tia:
        out, saved = Fn.decoder_fwd(p, dev(feat))
        cot = rnd(rs, *out.shape, scale=gs)
        saved = (*saved, dev(cot))
    else:
        loss, saved = Fn.decoder_fwd_nll(p, dev(feat), dev(u8), gs)
        out, _ = Fn.decoder_fwd(p, dev(feat))
    composed = isinstance(saved[0], Fn.DecHead)
    assert composed == (rows >= 512 and compose == "1"), (rows, compose, type(saved[0]))
    nrelu = 4 if image == 128 else 3
    hs_gpu = saved[1 : 1 + nrelu]
    # -- fp64: the plain forward (values), then the gated one (gradients)
    P64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in P.items()}
    feat64 = feat.double().requires_grad_(True)
    errs = {}
    with torch.no_grad():
        h0w, hsw, outw = _dec64(P64, feat64)
    if not composed:
        errs["h0"] = relerr(saved[0], h0w)
    for i, (hg, hw) in enumerate(zip(hs_gpu, hsw), 1):
        errs[f"h{i}"] = relerr(hg, hw)
    errs["out"] = relerr(out, outw)
    if not tia:
        d = outw - tgt
        want_loss = (0.5 * d * d).sum().item()
        errs["nll"] = abs(loss.item() - want_loss) / want_loss
        errs["dpre"] = relerr(saved[4] if image == 64 else saved[5], d * gs)
    del h0w, hsw, outw
    gates = [(h > 0).double().cpu() for h in hs_gpu]
    _, _, out64 = _dec64(P64, feat64, gates=gates)
    if tia:
        (out64 * cot.double()).sum().backward()
    else:
        (0.5 * gs * (out64 - tgt).pow(2)).sum().backward()
    del out64, gates
    names = list(P)
    wants = [P64[k].grad for k in names] + [feat64.grad]

    def bwd(**kw):
        g = [torch.empty_like(t) for t in p]
        dfeat = torch.empty(rows, F_, device="cuda")
        Fn.decoder_bwd(p, dev(feat), saved, g, dfeat=dfeat, **kw)
        return g + [dfeat]

    got = bwd()
    torch.cuda.synchronize()
    for k, a, w in zip(names + ["dfeat"], got, wants):
        errs[f"d {k}"] = relerr(a, w)
    log(f"decoder {stack} rows={rows} F={F_} compose={compose} (composed {composed}): "
        + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if e >= TOL}
    assert not bad, bad
    # accumulate into pre-filled gradients (and d feat): want + prefill
    pre = [dev(rnd(rs, *w.shape, scale=0.5 * float(w.abs().max()))) for w in wants]
    g = [t.clone() for t in pre[:-1]]
    dfeat = pre[-1].clone()
    Fn.decoder_bwd(p, dev(feat), saved, g, dfeat=dfeat, accumulate=True, accumulate_dfeat=True)
    for k, a, w, b in zip(names + ["dfeat"], g + [dfeat], wants, pre):
        e = relerr(a, w + b.double().cpu())
        assert e < TOL, ("accumulate", k, e)
    # RePo's call (weight gradients on a side stream) and Dreamer's (deferred closures): the serial run's bits
    side = torch.cuda.Stream()
    assert all(torch.equal(a, b) for a, b in zip(bwd(side=side), got)), "side stream"
    closures = []
    res = bwd(deferred=closures)
    assert closures, "nothing was deferred"
    for fn in closures:
        fn()
    assert all(torch.equal(a, b) for a, b in zip(res, got)), "deferred"


@pytest.mark.parametrize("compose", ["1", "0"])
@pytest.mark.parametrize("F_", [230, 232])
def test_cond_decoder_matches_fp64_two_layer_form_per_tensor(ops, monkeypatch, F_, compose):
    """The multitask decoder (Fm.cond_decoder_fwd_nll / cond_decoder_bwd: FiLM on conv1..conv3) at 512 rows against fp64
    autograd of oracle cond_decoder_fwd, tensor by tensor (twelve parameter gradients incl. the FiLM pair, and d feat into
    a strided view, as dreamer_mt.py writes it).  Task 0 gates one conv1 plane off (1 + gamma = 0 up to rounding, beta > 0:
    the plane is active) and task 1 another to 1 + gamma = 1e-4: the composed head's exact FiLM pass (FILM_DENSE over W01^T
    with one bias per output element) must recover both planes' gamma gradients; task 2 does the same to a conv2 plane."""
    import repo_amd.functional as Fn
    import repo_amd.functional_mt as Fm
    from oracle import fixtures as fx
    from oracle import repo_oracle as ro

    monkeypatch.setenv("REPO_DEC_COMPOSE", compose)
    rows, C = 512, 3
    rs = np.random.RandomState(F_ + 31)
    P = fx.make_params(6, 7, cond=C, belief=F_ - 30, state=30)["obs_model"]
    fw, fb = P["film.weight"], P["film.bias"]
    tot = 128 + 64 + 32
    for task, ch, one_plus_gamma in ((0, 5, 0.0), (1, 77, 1e-4), (2, 128 + 9, 0.0)):
        fw[ch, task] = np.float32(-1.0 + one_plus_gamma) - fb[ch]
        fw[tot + ch, task] = np.float32(0.5) - fb[tot + ch]
    p = [dev(torch.from_numpy(v)) for v in P.values()]
    feat = rnd(rs, rows, F_, scale=0.7)
    cond = torch.from_numpy(np.eye(C, dtype=np.float32)[rs.randint(0, C, size=rows)])
    u8, tgt = _dec_frames(rs, rows, 64)
    gs = 1.0 / rows
    loss, saved = Fm.cond_decoder_fwd_nll(p, dev(feat), dev(cond), dev(u8), gs)
    out, _ = Fm.cond_decoder_fwd(p, dev(feat), dev(cond))
    composed = isinstance(saved[1], Fn.DecHead)
    assert composed == (compose == "1"), (compose, type(saved[1]))
    gam = saved[0][:, :tot].cpu()
    assert float((1 + gam[:, 5]).abs().min()) < 1e-6 and float((1 + gam[:, 77]).abs().min()) < 2e-4
    assert float((1 + gam[:, 128 + 9]).abs().min()) < 1e-6
    hs_gpu = saved[3]
    P64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in P.items()}
    feat64 = feat.double().requires_grad_(True)
    errs = {}
    with torch.no_grad():
        _, hsw, outw = _dec64(P64, feat64, film=ro._film(P64, cond.double(), (128, 64, 32)))
    for i, (hg, hw) in enumerate(zip(hs_gpu, hsw), 1):
        errs[f"h{i}"] = relerr(hg, hw)
    errs["out"] = relerr(out, outw)
    d = outw - tgt
    want_loss = (0.5 * d * d).sum().item()
    errs["nll"] = abs(loss.item() - want_loss) / want_loss
    errs["dpre"] = relerr(saved[4], d * gs)
    del hsw, outw, d
    gates = [(h > 0).double().cpu() for h in hs_gpu]
    _, _, out64 = _dec64(P64, feat64, gates=gates, film=ro._film(P64, cond.double(), (128, 64, 32)))
    (0.5 * gs * (out64 - tgt).pow(2)).sum().backward()
    del out64, gates
    names = list(P)
    wants = [P64[k].grad for k in names] + [feat64.grad]
    ld = F_ + C + 1   # d feat lands in the first F_ columns of a wider row (dreamer_mt.py: [belief | state | task])

    def bwd(accumulate=False, side=None, fill=None):
        g = [torch.empty_like(t) for t in p] if fill is None else [t.clone() for t in fill[:-1]]
        buf = torch.full((rows, ld), 7.0, device="cuda")
        if fill is not None:
            buf[:, :F_] = fill[-1]
        Fm.cond_decoder_bwd(p, dev(feat), dev(cond), saved, g, dfeat=buf[:, :F_], accumulate_dfeat=fill is not None,
                            accumulate=accumulate, side=side)
        assert bool((buf[:, F_:] == 7.0).all()), "d feat wrote past its columns"
        return g + [buf[:, :F_]]

    got = bwd()
    torch.cuda.synchronize()
    for k, a, w in zip(names + ["dfeat"], got, wants):
        errs[f"d {k}"] = relerr(a, w)
    log(f"cond decoder rows={rows} F={F_} compose={compose} (composed {composed}): "
        + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if e >= TOL}
    assert not bad, bad
    pre = [dev(rnd(rs, *w.shape, scale=0.5 * float(w.abs().max()))) for w in wants]
    for k, a, w, b in zip(names + ["dfeat"], bwd(accumulate=True, fill=pre), wants, pre):
        e = relerr(a, w + b.double().cpu())
        assert e < TOL, ("accumulate", k, e)
    assert all(torch.equal(a, b) for a, b in zip(bwd(side=torch.cuda.Stream()), got)), "side stream"
