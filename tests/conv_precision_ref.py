"""CPU model of conv_precision="high"  and the bound it is held to.

The bf16 conv kernels split an fp32 operand with csrc/bgemm.h's bg_split3 (twgrad.h's tw_split3 is the same arithmetic):
a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2), each conversion a `__builtin_convertvector` float -> __bf16, which
on gfx950 is v_cvt_pk_bf16_f32: ROUND TO NEAREST EVEN (not truncation), the subtractions exact.  torch's
float32 -> bfloat16 conversion rounds to nearest even too, so `split2` below restates the first two parts bit for bit.

"high" forms a1 b1 + a1 b2 + a2 b1 where "highest" forms the six products with i + j <= 4.  Every bf16 x bf16 product is exact
in fp32, so what the kernels add to this model is the fp32 accumulation over K -- common to both modes and what the existing
conv tests bound with TOL = 1e-5 against the exact product.  The model is evaluated in float64.

The bound.  Round to nearest with 8 significand bits: u = 2^-8, |a - a1| <= u |a|, |a2| <= u (1 + u) |a|, and
r_a = a - a1 - a2 has |r_a| <= u |a - a1| <= u^2 |a|.  Then
    a b - (a1 b1 + a1 b2 + a2 b1) = a2 b2 + r_a b + (a - r_a) r_b,
    |.| <= (u^2 (1 + u)^2 + u^2 + (1 + u^2) u^2) |a||b| <= 3 u^2 (1 + u) |a||b|,
summed over K: componentwise at most K_HIGH * sum |a||b| with K_HIGH = 3 * 2^-16 * (1 + 2^-8).
uint8 frames are exact in ONE bf16 (bconv.h, U8): "highest" is x w1 + x w2 + x w3, "high" x w1 + x w2, and
    x w - x (w1 + w2) = x r_w,  |.| <= u^2 |x||w|:  K_HIGH_U8 = 2^-16  (w = the weights as the pack scales them, 2 w / 255).
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -8
K_HIGH = 3 * U * U * (1 + U)
K_HIGH_U8 = U * U


def bf16(x):
    """float32 -> bf16 (round to nearest even) -> float32."""
    assert x.dtype == torch.float32
    return x.to(torch.bfloat16).to(torch.float32)


def split2(x):
    """(a1, a2) of bg_split3, as float32 tensors whose values are bf16 numbers; a - a1 is exact in float32."""
    a1 = bf16(x)
    a2 = bf16(x - a1)
    return a1, a2


def _three(op, a, b):
    """a1 b1 + a1 b2 + a2 b1 through the bilinear `op`, in float64 (b1 + b2 is exact there)."""
    a1, a2 = split2(a)
    b1, b2 = split2(b)
    return op(a1.double(), (b1.double() + b2.double())) + op(a2.double(), b1.double())


def _chunks(n, step=64):
    return [(i, min(n, i + step)) for i in range(0, n, step)]


# ---- the three passes: model, exact product and bound, float64, images in chunks
def down(big, w):
    """-> (model, exact, bound) of small = conv2d(big, w, stride 2)."""
    op = lambda x, ww: torch.cat([F.conv2d(x[i:j], ww, None, stride=2) for i, j in _chunks(x.shape[0])])   # noqa: E731
    return _three(op, big, w), op(big.double(), w.double()), K_HIGH * op(big.double().abs(), w.double().abs())


def down_u8(u8, w, bias=None):
    """uint8 frames: the kernel multiplies the raw bytes v with w' = float32(w * (2 / 255)) split in two, and adds the folded
    bias float32(b - sum_k w_k) (bconv_pack_kernel: the sum in float64).  exact = conv2d(((v / 255) * 2) - 1, w) on the
    float32 frames the reference normalises to."""
    ws = w * torch.tensor(2.0 / 255.0, dtype=torch.float32)
    w1, w2 = split2(ws)
    v = u8.double()
    op = lambda x, ww: torch.cat([F.conv2d(x[i:j], ww, None, stride=2) for i, j in _chunks(x.shape[0])])   # noqa: E731
    fb = ((bias.double() if bias is not None else 0.0) - w.double().sum((1, 2, 3))).float().double()
    model = op(v, w1.double() + w2.double()) + fb.view(1, -1, 1, 1)
    frames = ((u8.float() / 255.0) * 2.0 - 1.0).double()
    exact = op(frames, w.double())
    if bias is not None:
        exact = exact + bias.double().view(1, -1, 1, 1)
    return model, exact, K_HIGH_U8 * op(v, ws.double().abs())


def down_u8_own_exact(u8, w, bias=None):
    """The exact value of the product the uint8 kernel forms: bytes x w' (unsplit) + the folded bias."""
    ws = (w * torch.tensor(2.0 / 255.0, dtype=torch.float32)).double()
    fb = ((bias.double() if bias is not None else 0.0) - w.double().sum((1, 2, 3))).float().double()
    v = u8.double()
    return torch.cat([F.conv2d(v[i:j], ws, None, stride=2) for i, j in _chunks(v.shape[0])]) + fb.view(1, -1, 1, 1)


def up(small, w, hb):
    """-> (model, exact, bound) of big = conv_transpose2d(small, w, stride 2), padded to hb x hb (encoder conv2's 31)."""
    def op(x, ww):
        r = torch.cat([F.conv_transpose2d(x[i:j], ww, None, stride=2) for i, j in _chunks(x.shape[0])])
        return F.pad(r, (0, hb - r.shape[3], 0, hb - r.shape[2]))
    return _three(op, small, w), op(small.double(), w.double()), K_HIGH * op(small.double().abs(), w.double().abs())


def wgrad(small, big, wshape):
    """-> (model, exact, bound) of dw = sum over images and pixels of small x big windows."""
    def op(s, b):
        r = torch.zeros(wshape, dtype=torch.float64)
        for i, j in _chunks(s.shape[0], 50):
            r += torch.nn.grad.conv2d_weight(b[i:j], wshape, s[i:j], stride=2)
        return r
    return _three(op, small, big), op(small.double(), big.double()), K_HIGH * op(small.double().abs(), big.double().abs())
