"""conv_precision="high"  on every bf16 conv engine, where csrc/conv.hip's plans send it.

The cases come from tests/test_conv_engines_gpu.py's TABLE, plan mirrors and image counts (imported, not copied): for every
(layer, pass, frame type) the mirrors send to a bf16 engine -- bconv.h (float and uint8 frames), tconv_down.h, buconv.h,
tconv_up.h, bwgrad.h, twgrad.h -- the smallest count of that module's lists that selects the engine and one count that leaves
a ragged last tile / image group / split (ragged_count below says which and why); plus repo_decoder_out_nll (bdec4.h).

Each case, in "high":
  (a) the device trace lists the engine's kernel in its three-product instantiation (two-product against uint8 frames)
      and no six-product one;
  (b) the result is within TOL = 1e-5 of the float64 model a1 b1 + a1 b2 + a2 b1 (tests/conv_precision_ref.py), per image
      (down, up) or per output row (weight gradient): what separates kernel and model is the fp32 accumulation over K, the
      bound the existing module applies to the six-product kernels against the exact product;
  (c) it is componentwise within K_HIGH * sum |a||b| (K_HIGH_U8 for uint8 frames) + TOL * max |exact| of the exact product;
  (d) it differs in at least one bit from the "highest" result;
  (e) no bias enters any case: image i (row r) on operands scaled by 2^k_i equals 2^k_i times the unscaled result, bit for bit.
In "highest", set explicitly and on a thread that never set it: the six-product instantiation (three against uint8 frames),
bit-identical results.
"""
import functools
from collections import namedtuple
import os
import re
import threading

import pytest
import torch
import torch.nn.functional as F

from repo_amd.ops import EPI_RELU
from tests import conv_precision_ref as ref
from tests import test_conv_engines_gpu as ce
from tests.util import has, log, traced

TOL = ce.TOL
BF_ENGINES = {"down": ("Bf16", "Tcd"), "up": ("BfScatter", "Tconv"), "wgrad": ("Bf16", "Transposing")}
COUNTS = {"down": ce.DOWN_COUNTS, "up": ce.UP_COUNTS, "wgrad": ce.WGRAD_COUNTS}
NLL_KERNEL = "bdec4_nll_kernel"
DEFAULT = os.environ.get("REPO_CONV_PRECISION") or "highest"   # what a thread that never set the mode runs at

Case = namedtuple("PCase", "kind layer nimg epi u8 engine")


def engine_at(kind, layer, n, epi, u8):
    e = ce.EPIS[epi][0]
    if kind == "down":
        return ce.down_plan(layer, n, e, False, False, False, u8, "full", 1).engine
    if kind == "up":
        return ce.up_plan(layer, n, e, 1)
    return ce.wgrad_plan(layer, n, False, u8, 1).engine


def ragged_count(kind, layer, engine, u8):
    """One count that leaves the engine's last unit of work partly filled, and the property that says so."""
    cb, cs, hb, ks, hs, ps = ce.geo(layer)
    lay = ce.TABLE[layer]
    if kind == "down" and engine == "Bf16":     # the last pixel tile of BN pixels: the module's largest small count
        n, bn = max(COUNTS[kind][layer]), lay.down_bf_u8 if u8 else lay.down_bf
        assert (n * ps) % bn != 0
    elif engine in ("Tcd", "Tconv"):            # one workgroup per CU (256), images dealt round: one workgroup gets a second
        n = 257
    elif kind == "up":                          # buconv.h: GI images per workgroup (GI = 1: several workgroups, nothing ragged)
        n = 37
        assert lay.up_bf == 1 or n % lay.up_bf != 0
    elif engine == "Transposing":               # twgrad.h: two images per split, the last split has one
        n = 129
        p = ce.wgrad_plan(layer, n)
        assert p.ips == 2 and n % p.ips == 1
    else:                                       # bwgrad.h: the last split of `ips` images
        n = 75
        assert n % ce.wgrad_plan(layer, n).ips != 0
    return n


def _cases():
    out = []
    for layer in ce.TABLE:
        for kind, engines in BF_ENGINES.items():
            for u8 in ((False, True) if layer in ce.U8_LAYERS and kind != "up" else (False,)):
                for engine in engines:
                    # the first (count, epilogue) of the module's lists that the mirror sends to this engine
                    hits = [(n, epi) for n in sorted(COUNTS[kind][layer]) for epi in ("none", "relu")
                            if (kind != "wgrad" or epi == "none") and engine_at(kind, layer, n, epi, u8) == engine]
                    if not hits:
                        continue
                    n0, epi0 = hits[0]
                    nr = ragged_count(kind, layer, engine, u8)
                    epir = next(epi for epi in ("none", "relu") if engine_at(kind, layer, nr, epi, u8) == engine)
                    assert nr != ce.FULL[layer] and n0 != ce.FULL[layer]
                    out.append(Case(kind, layer, n0, epi0, u8, engine))
                    if nr != n0:
                        out.append(Case(kind, layer, nr, epir, u8, engine))
    return out


CASES = _cases()


def case_id(c):
    return f"{ce.TABLE[c.layer].name}-{c.kind}-n{c.nimg}-{c.epi}{'-u8' if c.u8 else ''}-{c.engine}"


def kernel_of(c):
    return ce.WGRAD_KERNEL_OF[c.engine] if c.kind == "wgrad" else ce.KERNEL_OF[c.engine]


def products(names, kernel):
    """The product counts (last template argument) of the kernel's instantiations in a device trace."""
    out = set()
    for n in names:
        if re.search(rf"\b{kernel}\b", n):
            m = re.search(r",(\d+)>(\(|$)", n.replace(" ", ""))
            assert m, ("no product count in the kernel's name", n)
            out.add(int(m.group(1)))
    return out


def n_products(mode, u8=False):
    return {("highest", False): 6, ("high", False): 3, ("highest", True): 3, ("high", True): 2}[(mode, u8)]


@functools.lru_cache(maxsize=1)
def reference(kind, layer, nimg, u8):
    """(model, exact, bound) of the UNSCALED operands, float64 on the device; one (kind, layer, count) at a time."""
    d = ce.data(layer, nimg)
    hb = ce.geo(layer)[2]
    if kind == "down":
        r = ref.down_u8(d.u8, d.w) if u8 else ref.down(d.big0, d.w)
    elif kind == "up":
        r = ref.up(d.small0, d.w, hb)
    else:
        r = ref.wgrad(d.small_w, (d.u8.float() / 255.0) * 2.0 - 1.0 if u8 else d.big0, tuple(d.w.shape))
    return tuple(t.cuda() for t in r)


def run(ops, c):
    """The case's call on the scaled and on the unscaled operands -> (result, result0, per-slice scale, extras)."""
    d = ce.data(c.layer, c.nimg)
    epi = ce.EPIS[c.epi][0]
    if c.kind == "down":
        s = d.dev("simg")
        if c.u8:
            return ops.conv_down(c.layer, d.dev("u8"), d.dev("w"), None, epi=epi), None, None
        return (ops.conv_down(c.layer, d.dev("big0") * ce._view(s, d.big0), d.dev("w"), None, epi=epi),
                ops.conv_down(c.layer, d.dev("big0"), d.dev("w"), None, epi=epi), s)
    if c.kind == "up":
        s = d.dev("simg")
        return (ops.conv_up(c.layer, d.dev("small0") * ce._view(s, d.small0), d.dev("w"), None, epi=epi),
                ops.conv_up(c.layer, d.dev("small0"), d.dev("w"), None, epi=epi), s)
    s = d.dev("srow")
    big = d.dev("u8") if c.u8 else d.dev("big0")
    small0 = d.dev("small_w")
    return (ops.conv_wgrad(c.layer, small0 * s.view(1, -1, 1, 1), big), ops.conv_wgrad(c.layer, small0, big), s)


def excess(got, exact, bound):
    """max over components of |got - exact| - bound - TOL * max |exact| of the slice (<= 0: inside)."""
    allow = TOL * exact.abs().flatten(1).amax(1)
    return float(((got.double() - exact).abs() - bound - ce._view(allow, exact)).max())


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from repo_amd import ops as o

    return o


@pytest.fixture(autouse=True)
def _poison_lds(request):
    if "gpu" in request.keywords:
        from repo_amd._lib import lib

        assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
    yield


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    reference.cache_clear()
    ce._cache.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def on_fresh_thread(fn):
    """fn() on a host thread that never set a mode (the library's thread-local default), on the caller's stream."""
    box, stream = {}, torch.cuda.current_stream()

    def body():
        try:
            with torch.cuda.stream(stream):
                box["out"] = fn()
        except BaseException as e:   # noqa: BLE001 (handed to the caller)
            box["err"] = e

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if "err" in box:
        raise box["err"]
    return box["out"]


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_engine_in_high_and_highest(ops, c):
    what, kernel = case_id(c), kernel_of(c)
    model0, exact0, bound0 = reference(c.kind, c.layer, c.nimg, c.u8)
    with ops.conv_precision("high"):
        assert ops.get_conv_precision() == "high"
        (got, got0, s), names = traced(lambda: run(ops, c))
    assert ops.get_conv_precision() == DEFAULT
    # (a)
    assert products(names, kernel) == {n_products("high", c.u8)}, (what, names)
    db = None
    if c.kind == "wgrad":
        (got, db), (got0, _) = got, got0
    if s is None:   # uint8 frames carry no scale
        model, exact, bound = model0, exact0, bound0
    else:
        sv = ce._view(s.double(), model0)
        model, exact, bound = model0 * sv, exact0 * sv, bound0 * sv
    if ce.EPIS[c.epi][0] == EPI_RELU:   # |relu(x) - relu(y)| <= |x - y|: the bound carries over
        model, exact = F.relu(model), F.relu(exact)
    # (b), (c)
    e_model, e_exact, ex = ce.per_slice(got, model), ce.per_slice(got, exact), excess(got, exact, bound)
    log(f"conv_precision {what}: high {n_products('high', c.u8)} products; worst slice {e_model:.2e} of the model, "
        f"{e_exact:.2e} of the exact product, bound excess {ex:.2e}")
    assert e_model < TOL, (what, e_model)
    assert ex <= 0.0, (what, ex)
    # (e)
    if s is not None:
        assert torch.equal(got, got0 * ce._view(s, got0)), (what, "a slice's result depends on another slice's scale")
    # "highest", explicit and on a thread that never set a mode
    with ops.conv_precision("highest"):
        (hi, _, _), names_hi = traced(lambda: run(ops, c))
    (dflt, _, _), names_d = traced(lambda: on_fresh_thread(lambda: run(ops, c)))
    assert products(names_hi, kernel) == {n_products("highest", c.u8)}, (what, names_hi)
    assert products(names_d, kernel) == {n_products(DEFAULT, c.u8)}, (what, names_d)
    db_hi = None
    if c.kind == "wgrad":
        (hi, db_hi), (dflt, _) = hi, dflt
    if DEFAULT == "highest":
        assert torch.equal(hi, dflt), (what, "explicit and default highest differ")
    assert ce.per_slice(hi, exact) < TOL, what
    # (d)
    assert not torch.equal(got, hi), (what, "high and highest agree in every bit")
    if db is not None:   # the bias gradient is no product: the same bits in both modes
        assert torch.equal(db, db_hi), (what, "db")


def _nll_inputs(nimg, u8):
    g = torch.Generator().manual_seed(77 + nimg)
    h3 = F.relu(torch.randn(nimg, 32, 30, 30, generator=g))
    w = torch.randn(32, 3, 6, 6, generator=g) * 0.05
    bias = torch.randn(3, generator=g) * 0.1
    tgt = torch.randint(0, 256, (nimg, 3, 64, 64), generator=g, dtype=torch.uint8)
    return h3, w, bias, tgt if u8 else (tgt.float() / 255.0) * 2.0 - 1.0


@gpu
@pytest.mark.parametrize("nimg,u8", [(1, False), (5, True)], ids=["n1-float", "n5-u8"])
def test_decoder_out_nll_in_high_and_highest(ops, nimg, u8):
    """The fused output layer + NLL (bdec4.h): one image = four tiles on four workgroups; five = twenty."""
    h3, w, bias, tgt = _nll_inputs(nimg, u8)
    model, exact, bound = (t.cuda() for t in ref.up(h3, w, 64))
    bd = bias.double().cuda().view(1, -1, 1, 1)
    model, exact = model + bd, exact + bd
    args = (h3.cuda(), w.cuda(), bias.cuda(), tgt.cuda(), 0.25)
    tgt64 = ((tgt.float() / 255.0) * 2.0 - 1.0 if u8 else tgt).double().cuda()
    with ops.conv_precision("high"):
        (loss, dpre, recon), names = traced(lambda: ops.decoder_out_nll(*args, want_recon=True))
    assert products(names, NLL_KERNEL) == {3}, names
    e_model, ex = ce.per_slice(recon, model), excess(recon, exact, bound)
    log(f"conv_precision decoder_out_nll n{nimg}: recon {e_model:.2e} of the model, bound excess {ex:.2e}")
    assert e_model < TOL and ex <= 0.0, (e_model, ex)
    want_loss = float((0.5 * (model - tgt64) ** 2).sum())
    assert abs(float(loss) - want_loss) <= TOL * want_loss
    assert ce.per_slice(dpre, (model - tgt64) * 0.25) < TOL
    with ops.conv_precision("highest"):
        (_, _, recon_hi), names_hi = traced(lambda: ops.decoder_out_nll(*args, want_recon=True))
    (_, _, recon_d), names_d = traced(lambda: on_fresh_thread(lambda: ops.decoder_out_nll(*args, want_recon=True)))
    assert products(names_hi, NLL_KERNEL) == {6} and products(names_d, NLL_KERNEL) == {n_products(DEFAULT)}
    if DEFAULT == "highest":
        assert torch.equal(recon_hi, recon_d)
    assert ce.per_slice(recon_hi, exact) < TOL
    assert not torch.equal(recon, recon_hi)


TWIN_CASES = [Case("down", 2, 15, "none", False, "Fp32"), Case("up", 2, 5, "none", False, "Scatter"),
              Case("wgrad", 2, 9, "none", False, "Fp32")]


@gpu
@pytest.mark.parametrize("c", TWIN_CASES, ids=case_id)
def test_debug_bconv_off_selects_the_fp32_twin_in_either_mode(ops, c):
    from repo_amd._lib import lib

    first = lambda r: r[0][0] if c.kind == "wgrad" else r[0]   # noqa: E731
    prev = lib().repo_debug_bconv(0)
    try:
        with ops.conv_precision("high"):
            r_high, names = traced(lambda: run(ops, c))
        with ops.conv_precision("highest"):
            r_hi = run(ops, c)
    finally:
        lib().repo_debug_bconv(prev)
    assert has(names, rf"\b{kernel_of(c)}\b"), names
    for k in ("bconv_down_kernel", "tconv_down_kernel", "buconv_scatter_kernel", "tconv_up_kernel", "bconv_wgrad_kernel",
              "tconv_wgrad_kernel"):
        assert not has(names, rf"\b{k}\b"), (k, names)
    assert torch.equal(first(r_high), first(r_hi))


@gpu
def test_debug_bconv_off_nll_runs_the_fp32_twin_in_either_mode(ops):
    from repo_amd._lib import lib

    h3, w, bias, tgt = _nll_inputs(1, False)
    args = (h3.cuda(), w.cuda(), bias.cuda(), tgt.cuda(), 0.25)
    prev = lib().repo_debug_bconv(0)
    try:
        with ops.conv_precision("high"):
            (_, _, r_high), names = traced(lambda: ops.decoder_out_nll(*args, want_recon=True))
        with ops.conv_precision("highest"):
            r_hi = ops.decoder_out_nll(*args, want_recon=True)[2]
    finally:
        lib().repo_debug_bconv(prev)
    assert has(names, r"\bdconv_dec4_nll_kernel\b") and not has(names, rf"\b{NLL_KERNEL}\b"), names
    assert torch.equal(r_high, r_hi)


@gpu
@pytest.mark.parametrize("layer,nimg,kernel", [(2, 5, "buconv_scatter_kernel"), (1, 4, "tconv_up_kernel")],
                         ids=["enc3-buconv", "enc2-tconv_up"])
def test_a_pack_written_under_one_mode_serves_the_other(ops, layer, nimg, kernel):
    d = ce.data(layer, nimg)
    small, w = d.dev("small0"), d.dev("w")
    with ops.conv_precision("highest"):
        pack_hi = ops.conv_up_pack(layer, w)
        own_hi = ops.conv_up(layer, small, w)
    with ops.conv_precision("high"):
        pack_high = ops.conv_up_pack(layer, w)
        own_high = ops.conv_up(layer, small, w)
        got, names = traced(lambda: ops.conv_up(layer, small, w, pack=pack_hi))
    assert torch.equal(pack_hi, pack_high), "the pack depends on the mode"
    assert products(names, kernel) == {3} and not any(has(names, rf"\b{k}\b") for k in ce.PACKERS), names
    assert torch.equal(got, own_high)
    with ops.conv_precision("highest"):
        assert torch.equal(ops.conv_up(layer, small, w, pack=pack_high), own_hi)
    assert not torch.equal(own_hi, own_high)


@gpu
def test_setter_returns_the_previous_mode_and_an_unknown_mode_is_refused(ops):
    """On the device box too (tests/test_conv_precision_cpu.py has the full version): a refused value leaves the mode, and
    the kernels that then run, as they were."""
    from repo_amd._lib import lib

    c = Case("down", 2, 15, "none", False, "Bf16")
    assert ops.set_conv_precision("high") == DEFAULT
    try:
        assert ops.set_conv_precision("high") == "high"
        assert lib().repo_conv_precision(2) == -1 and lib().repo_conv_precision(-1) == -1
        with pytest.raises(ValueError, match='"highest" or "high"'):
            ops.set_conv_precision("tf32")
        _, names = traced(lambda: run(ops, c))
        assert products(names, kernel_of(c)) == {3}, names
    finally:
        assert ops.set_conv_precision(DEFAULT) == "high"
    assert ops.get_conv_precision() == DEFAULT


@gpu
def test_backward_thread_follows_its_forwards_mode(ops):
    """torch.autograd runs a Function's backward on its device thread; the wrappers carry the forward thread's mode there
    (ops.debug_snapshot / debug_scope), so the backward's conv kernels are three-product ones too."""
    from repo_amd import functional as Fn
    from repo_amd.algorithms.repo.models.encoder import VisualEncoder

    torch.manual_seed(0)
    enc = VisualEncoder(1024).cuda()
    x = torch.rand(40, 3, 64, 64, device="cuda") - 0.5
    seen, real = {}, Fn.encoder_bwd

    def spy(*a, **k):
        seen["thread"], seen["mode"] = threading.get_ident(), ops.get_conv_precision()
        return real(*a, **k)

    def step():
        enc(x).sum().backward()

    try:
        Fn.encoder_bwd = spy
        with ops.conv_precision("high"):
            assert ops.debug_snapshot()[-1] == ops.CONV_PRECISIONS.index("high")
            _, names = traced(step)
    finally:
        Fn.encoder_bwd = real
    assert seen["mode"] == "high", seen
    assert ops.get_conv_precision() == DEFAULT
    ran = {k: products(names, k) for k in ("bconv_down_kernel", "tconv_down_kernel", "buconv_scatter_kernel", "tconv_up_kernel",
                                           "bconv_wgrad_kernel", "tconv_wgrad_kernel")}
    assert any(ran.values()), names
    assert all(v <= {3} for v in ran.values()), ran
    assert all(torch.isfinite(p.grad).all() for p in enc.parameters())
