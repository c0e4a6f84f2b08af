"""Every conv engine where csrc/conv.hip's plans send it, judged per image / per row against float64, with proof it ran.

csrc/conv.hip routes three passes (down, up, weight gradient) of 14 layer geometries to eleven engine headers.  Which
engine a call takes is decided by Layer<G> / Route<G> and one plan per pass (down_plan, up_plan, wgrad_plan).  This module

  * mirrors the table and the three plans in Python (TABLE, down_plan, up_plan, wgrad_plan below),
  * lists its cases once (CASES) and checks WITHOUT a GPU that they reach every (layer, pass, engine) the default build
    can select and both sides of every routing threshold (test_cases_cover_every_engine_and_threshold),
  * runs every case under a device trace and asserts that exactly the kernels of the mirrored engine ran, so a mirror
    that drifts from conv.hip fails on the device,
  * compares with float64 torch on the CPU of the same operation, the bound being tests/test_ops_gpu.py's TOL = 1e-5 applied
    PER IMAGE (down, up) or PER OUTPUT ROW (weight gradient: dw[r], db[r], dbig[c] alike), on inputs whose images (rows)
    differ by up to 2^16 in scale -- standard normal, except that the weight gradient's `small` (and, where dbig is asked
    for, `big`) carries a per-channel offset so that the single sums db[r] / dbig[c] do not cancel (class Data),
  * and, where no bias enters, asserts the exact law that scaling gives: image i of the result on the scaled batch equals
    2^k_i times image i of the result on the unscaled batch, bit for bit (no arithmetic crosses images in down / up, none
    crosses rows in the weight gradient, and a power of two commutes with every fp32 and bf16-split rounding in this range).

When a layer's pass is re-routed: edit its TABLE entry (and the plan mirror if a threshold moved) as conv.hip's Layer<G>
entry was edited; run the CPU test -- it names every (layer, pass, engine) and threshold side that CASES no longer
reaches; add the image counts on both sides of a new threshold to DOWN_COUNTS / UP_COUNTS / WGRAD_COUNTS (and the threshold
to thresholds()).  An engine only a tools/build_variant.sh define can reach goes into NOT_REACHABLE by name.
"""
import re
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from repo_amd.ops import CONV_GEO, EPI_MUL_CMASK, EPI_MUL_DRELU, EPI_MUL_MASK4, EPI_NONE, EPI_RELU
from tests.util import CONV_ENGINE_KERNELS, CONV_REDUCE_KERNELS, has, log, traced

TOL = 1e-5               # tests/test_ops_gpu.py's, here per image / per row
OK, E_SHAPE, E_WS_TOO_SMALL = 0, -2, -4


# ----------------------------------------------------------------------------- the table (conv.hip: Layer<G>), in Python
def _never(epi, has_bias, wants_cmask):
    return False


# down: DTile <BM, BN, CK, WM, WN> of the throughput tile; down_lat: the latency tile (None: the same tile);
# down_bf / down_bf_u8: BN of bconv.h's tile for float / uint8 frames; tcd(epi, has_bias, wants_cmask): tconv_down.h takes it;
# up_scatter / up_bf: images per workgroup of uconv.h / buconv.h; direct: dconv_up.h; tconv: tconv_up.h;
# wtile: (BM, BN, GI) of dconv.h's weight-gradient tile; wgt: the workgroups its split-K aims at; wgrad_bf: GI of bwgrad.h's
# tile; tw_nbk: twgrad.h's k-blocks per chunk (0: not on it)
Lay = namedtuple("Lay", "name down down_lat down_bf down_bf_u8 tcd up_scatter up_bf direct tconv wtile wgt wgrad_bf tw_nbk",
                 defaults=(None, None, None, _never, None, None, False, False, None, 0, None, 0))
TABLE = {
    0: Lay("enc1", (32, 512, 3, 1, 8), down_bf_u8=512, wtile=(32, 64, 1), wgt=3072),
    1: Lay("enc2", (64, 128, 2, 2, 2), down_lat=(32, 128, 4, 1, 4), down_bf=256,
           tcd=lambda epi, has_bias, wants_cmask: epi == EPI_RELU, up_scatter=1, up_bf=1, tconv=True,
           wtile=(64, 128, 1), wgt=768, tw_nbk=2),
    2: Lay("enc3", (128, 128, 2, 2, 2), down_lat=(32, 128, 8, 1, 4), down_bf=128, up_scatter=4, up_bf=4,
           wtile=(64, 128, 2), wgt=1024, wgrad_bf=1),
    3: Lay("enc4", (32, 64, 2, 1, 2), down_lat=(32, 128, 8, 1, 4), down_bf=64, up_scatter=8, up_bf=8,
           wtile=(64, 128, 8), wgt=768),
    4: Lay("dec2", (128, 128, 4, 2, 4), down_bf=128, up_scatter=5, up_bf=5, wtile=(64, 128, 4), wgt=1536),
    5: Lay("dec3", (64, 128, 2, 2, 2), down_bf=256,
           tcd=lambda epi, has_bias, wants_cmask: epi in (EPI_NONE, EPI_MUL_DRELU) and not has_bias and not wants_cmask,
           up_scatter=1, up_bf=1, wtile=(64, 128, 1), wgt=2048, wgrad_bf=1, tw_nbk=2),
    6: Lay("dec4", (32, 256, 3, 1, 8), wtile=(32, 128, 1), wgt=1536),
    7: Lay("x_enc1", (32, 512, 3, 1, 8), wtile=(32, 64, 1), wgt=3072),
    8: Lay("x_enc2", (64, 128, 2, 2, 2), direct=True, wtile=(64, 128, 1), wgt=1536),
    9: Lay("x_enc3", (128, 128, 2, 2, 2), up_scatter=1, wtile=(64, 128, 1), wgt=1024),
    10: Lay("x_enc4", (64, 128, 2, 2, 2), up_scatter=4, wtile=(64, 128, 2), wgt=1024),
    11: Lay("x_dec4", (32, 256, 2, 1, 4), direct=True, wtile=(32, 128, 1), wgt=1536),
    12: Lay("x_dec5", (32, 512, 3, 1, 8), wtile=(32, 64, 1), wgt=1536),
    13: Lay("tia_dec4", (32, 256, 3, 1, 8), direct=True, wtile=(32, 128, 1), wgt=1536),
}
# (layer, pass, engine) the table names but the default build never selects
NOT_REACHABLE = [
    (5, "wgrad", "Bf16"),   # decoder conv3 on bwgrad.h: shadowed by the transposing engine (tools/build_variant.sh -DTW_DISABLE)
]
U8_LAYERS = (0, 7)


def geo(layer):
    cb, cs, hb, ks = CONV_GEO[layer]
    hs = (hb - ks) // 2 + 1
    return cb, cs, hb, ks, hs, hs * hs


def cdiv(a, b):
    return (a + b - 1) // b


# ----------------------------------------------------------------------------- the three plans, in Python
DownPlan = namedtuple("DownPlan", "engine tile tiles rc")


def down_plan(layer, nimg, epi=EPI_NONE, has_bias=False, wants_dbias=False, wants_cmask=False, u8=False, ws="full", bconv=1):
    """conv.hip down_plan + conv_down_t's workspace check.  ws: "full" (what repo_conv_down_workspace_bytes asks for),
    "none", or "short" (one byte less than the bf16x6 kernel's weight pack; without channel sums only)."""
    lay, ps = TABLE[layer], geo(layer)[5]
    assert not (ws == "short" and wants_dbias)
    px = nimg * ps
    bn = lay.down_bf_u8 if u8 else lay.down_bf
    if bn and bconv and px > 512 and ws == "full":
        engine = "Bf16"
        if not u8 and nimg >= 32 and not wants_dbias and lay.tcd(epi, has_bias, wants_cmask):
            engine = "Tcd"
        return DownPlan(engine, None, cdiv(px, bn), OK)
    lat = px <= 512
    tile = (lay.down_lat or lay.down) if lat else lay.down
    return DownPlan("Fp32Lat" if lat else "Fp32", tile, cdiv(px, tile[1]), E_WS_TOO_SMALL if wants_dbias and ws != "full" else OK)


def up_plan(layer, nimg, epi=EPI_NONE, bconv=1):
    lay = TABLE[layer]
    if lay.up_bf:
        base = "BfScatter" if bconv else "Scatter"
    elif lay.direct:
        base = "Direct"
    elif lay.up_scatter:
        base = "Scatter"
    else:
        base = "Merged"
    if lay.tconv and bconv and epi in (EPI_NONE, EPI_MUL_DRELU, EPI_MUL_CMASK) and nimg >= 4:
        return "Tconv"
    return base


def up_has_pack(layer):
    lay = TABLE[layer]
    return bool(lay.up_bf or lay.direct or lay.up_scatter)


def up_takes_cmask(layer):
    return bool(TABLE[layer].up_scatter) and geo(layer)[0] % 4 == 0


def chansum_splits(nimg, c, p):
    want = min(cdiv(4096, c), cdiv(nimg, cdiv(8192, p)))
    want = max(want, 1)
    return cdiv(nimg, cdiv(nimg, want))


WgradPlan = namedtuple("WgradPlan", "engine ips splits wave_reduce dbig_in_slabs need")


def round256(b):
    return (b + 255) & ~255


def wgrad_plan(layer, nimg, wants_dbig=False, u8=False, bconv=1):
    lay = TABLE[layer]
    cb, cs, hb, ks, hs, ps = geo(layer)
    bm, bnw, gi = lay.wtile
    tiles = cdiv(cs, bm) * cdiv(cb * ks * ks, bnw)
    want = cdiv(lay.wgt, tiles)
    min_ips = gi * (1 if ps >= 512 else 2 if ps >= 64 else 4)
    ips = cdiv(max(cdiv(nimg, want), min_ips), gi) * gi
    row = cs * (cb * ks * ks + 1)
    splits = cdiv(nimg, ips)
    engine, wave, in_slabs = "Fp32", splits >= 64 and row <= 65536, False
    slabs = splits * row * 4
    if lay.wgrad_bf and not u8 and bconv:
        engine = "Bf16"
    if lay.tw_nbk:
        tips = cdiv(nimg, 128)
        tsplits = cdiv(nimg, tips)
        slabs = max(slabs, tsplits * (row + 2 * cb) * 4)
        covers = hb == 2 * (hs - 1) + ks
        if not u8 and bconv:
            engine, ips, splits, wave, in_slabs = "Transposing", tips, tsplits, True, covers and wants_dbig
    need = round256(slabs) + chansum_splits(nimg, cb, hb * hb) * cb * 4
    return WgradPlan(engine, ips, splits, wave, in_slabs, need)


# ----------------------------------------------------------------------------- the cases
# The default bench.py update (B = 50, L = 50) feeds every 64 x 64 layer and TIA's conv4 (L - 1) * B = 2450 images; the
# 128 x 128 stack's config (B = 32) feeds its layers 1568.
FULL = {**{layer: 2450 for layer in range(7)}, **{layer: 1568 for layer in range(7, 13)}, 13: 2450}

# image counts per layer beside FULL: both sides of each threshold the layer has, one ragged count per images-per-workgroup
# factor.  nimg * PS <= 512 (latency | throughput / bf16x6 tiles); nimg >= 32 (tconv_down.h); 37: pixel tiles straddle images
DOWN_COUNTS = {0: [1, 5], 1: [2, 3, 31, 32, 37], 2: [14, 15, 37], 3: [128, 129, 150], 4: [20, 21, 37], 5: [3, 4, 31, 32, 37],
               6: [1, 5], 7: [1, 3], 8: [1, 3], 9: [2, 3], 10: [14, 15], 11: [1, 3], 12: [1, 3], 13: [1, 5]}
# nimg >= 4 (tconv_up.h; 600: several images per workgroup, ragged); nimg % GI of the scatter configurations (4, 5, 8)
UP_COUNTS = {0: [1, 5], 1: [3, 4, 37, 600], 2: [3, 4, 5, 37], 3: [7, 8, 13, 37], 4: [4, 5, 7, 37], 5: [1, 5, 37], 6: [1, 5],
             7: [1, 3], 8: [1, 3], 9: [1, 3], 10: [3, 4, 6], 11: [1, 3], 12: [1, 3], 13: [1, 5]}
# twgrad.h's images per workgroup pair (128 | 129, 256 | 257; 300: three per pair, ragged); splits >= 64 (the slab-reduce
# kernel: 63 | 64 where a split is one image, 126 | 127 for enc2's fp32 engine); 9 / 75: ragged image groups and splits
WGRAD_COUNTS = {0: [1, 63, 64], 1: [9, 126, 127, 128, 129, 256, 257, 300], 2: [9, 75, 300], 3: [9, 75, 600],
                4: [9, 75, 300], 5: [9, 75, 128, 129, 256, 257, 300], 6: [1, 63, 64], 7: [1, 63, 64], 8: [9, 63, 64],
                9: [9, 21], 10: [9, 21], 11: [9, 63, 64], 12: [1, 63, 64], 13: [9, 63, 64]}
MASK4_LAYERS = (1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12)   # the layers whose data gradient reads a quad mask

# kind: down | up | wgrad.  epi: the epilogue's name (EPIS); opt: the pass's extras (down: "", "cmask", "dbias", "dbias_acc";
# up: "", "pack"; wgrad: "db", "dbig_acc", "db_dbig"); ws (down): "full", "none", "short"
Case = namedtuple("Case", "kind layer nimg epi opt u8 ws bconv")
EPIS = {"none": (EPI_NONE, False), "bias": (EPI_NONE, True), "relu": (EPI_RELU, False), "relu_bias": (EPI_RELU, True),
        "drelu": (EPI_MUL_DRELU, False), "mask4": (EPI_MUL_MASK4, False), "cmask": (EPI_MUL_CMASK, False)}


def _bconv_settings(layer, kind):
    lay = TABLE[layer]
    on = {"down": lay.down_bf or lay.down_bf_u8, "up": lay.up_bf, "wgrad": lay.wgrad_bf or lay.tw_nbk}[kind]
    return (1, 0) if on else (1,)


def _cases():
    out = []
    for layer in TABLE:
        full = FULL[layer]
        for bconv in _bconv_settings(layer, "down"):
            for n in DOWN_COUNTS[layer] + [full]:
                small_n = n != full
                variants = [("none", ""), ("relu_bias", ""), ("relu_bias", "cmask"), ("drelu", ""), ("drelu", "dbias")]
                if small_n:
                    variants += [("relu", ""), ("drelu", "dbias_acc"), ("none", "dbias")]
                if layer in MASK4_LAYERS:
                    variants.append(("mask4", ""))
                for epi, opt in variants:
                    if not (bconv == 0 and layer in U8_LAYERS):   # float frames of the 3-channel layers: no bf16x6 engine
                        out.append(Case("down", layer, n, epi, opt, False, "full", bconv))
                if layer in U8_LAYERS:
                    for epi, opt in [("relu_bias", ""), ("relu_bias", "dbias"), ("none", "")]:
                        out.append(Case("down", layer, n, epi, opt, True, "full", bconv))
        # repo_conv_down without room for the weight pack: the fp32 engine, or REPO_E_WS_TOO_SMALL where channel sums
        # need a workspace
        if TABLE[layer].down_bf or TABLE[layer].down_bf_u8:
            u8 = layer in U8_LAYERS
            n = DOWN_COUNTS[layer][-1]
            out += [Case("down", layer, n, "relu_bias", "", u8, "none", 1), Case("down", layer, n, "relu_bias", "", u8, "short", 1),
                    Case("down", layer, n, "relu_bias", "dbias", u8, "none", 1)]
        for bconv in _bconv_settings(layer, "up"):
            for n in UP_COUNTS[layer] + [full]:
                variants = [("none", ""), ("bias", ""), ("relu_bias", ""), ("drelu", "")]
                if up_takes_cmask(layer):
                    variants.append(("cmask", ""))
                if up_has_pack(layer):
                    variants += [("none", "pack"), ("relu_bias", "pack")]
                for epi, opt in variants:
                    out.append(Case("up", layer, n, epi, opt, False, "full", bconv))
        for bconv in _bconv_settings(layer, "wgrad"):
            for n in WGRAD_COUNTS[layer] + [full]:
                for opt in ("db", "dbig_acc", "db_dbig"):
                    out.append(Case("wgrad", layer, n, "none", opt, False, "full", bconv))
        if layer in U8_LAYERS:
            for n in WGRAD_COUNTS[layer] + [full]:
                out.append(Case("wgrad", layer, n, "none", "db", True, "full", 1))
    # cases that share a (layer, count) are neighbours: the float64 references are cached per (layer, count)
    return sorted(out, key=lambda c: (c.layer, c.nimg, c.kind, c.u8, -c.bconv))


CASES = _cases()


def case_id(c):
    return f"{TABLE[c.layer].name}-{c.kind}-n{c.nimg}-{c.epi}{'-' + c.opt if c.opt else ''}{'-u8' if c.u8 else ''}" \
           f"{'' if c.ws == 'full' else '-ws_' + c.ws}-{'bf' if c.bconv else 'fp32'}"


def plan_of(c):
    epi, has_bias = EPIS[c.epi]
    if c.kind == "down":
        return down_plan(c.layer, c.nimg, epi, has_bias, c.opt.startswith("dbias"), c.opt == "cmask", c.u8, c.ws, c.bconv)
    if c.kind == "up":
        return up_plan(c.layer, c.nimg, epi, c.bconv)
    return wgrad_plan(c.layer, c.nimg, "dbig" in c.opt, c.u8, c.bconv)


def engine_of(c):
    p = plan_of(c)
    return p if isinstance(p, str) else p.engine


def selectable():
    """Every (layer, pass, engine) the mirrored plans select for SOME arguments: counts 1 .. 700 and the update's, every
    epilogue and flag, both settings of the switch, both frame types."""
    out = set()
    for layer in TABLE:
        for n in list(range(1, 701)) + [FULL[layer]]:
            for bconv in (1, 0):
                for epi in (EPI_NONE, EPI_RELU, EPI_MUL_DRELU, EPI_MUL_MASK4, EPI_MUL_CMASK):
                    out.add((layer, "up", up_plan(layer, n, epi, bconv)))
                    for flags in range(8):
                        for u8 in ((False, True) if layer in U8_LAYERS else (False,)):
                            out.add((layer, "down", down_plan(layer, n, epi, bool(flags & 1), bool(flags & 2), bool(flags & 4), u8,
                                                              "full", bconv).engine))
                for u8 in ((False, True) if layer in U8_LAYERS else (False,)):
                    out.add((layer, "wgrad", wgrad_plan(layer, n, False, u8, bconv).engine))
    return out


def thresholds():
    """(what, kind, layer, bconv, count below, count above, the plan's property that changes, a filter on the case)."""
    anycase = lambda c: True   # noqa: E731
    eng = lambda p: p if isinstance(p, str) else p.engine   # noqa: E731
    out = []
    for layer, (lo, hi) in {1: (2, 3), 9: (2, 3), 2: (14, 15), 10: (14, 15), 3: (128, 129), 4: (20, 21), 5: (3, 4)}.items():
        for bconv in _bconv_settings(layer, "down"):
            out.append(("nimg * PS <= 512", "down", layer, bconv, lo, hi, eng, anycase))
    out.append(("nimg >= 32: tconv_down.h", "down", 1, 1, 31, 32, eng, lambda c: c.epi.startswith("relu") and "dbias" not in c.opt))
    out.append(("nimg >= 32: tconv_down.h", "down", 5, 1, 31, 32, eng, lambda c: c.epi in ("none", "drelu") and not c.opt))
    out.append(("nimg >= 4: tconv_up.h", "up", 1, 1, 3, 4, eng, lambda c: c.epi in ("none", "drelu", "cmask")))
    for layer in (1, 5):
        for lo, hi in ((128, 129), (256, 257)):
            out.append(("twgrad.h images per pair", "wgrad", layer, 1, lo, hi, lambda p: p.ips, anycase))
    for layer, bconv, lo, hi in [(0, 1, 63, 64), (1, 0, 126, 127), (6, 1, 63, 64), (7, 1, 63, 64), (8, 1, 63, 64), (11, 1, 63, 64),
                                 (12, 1, 63, 64), (13, 1, 63, 64)]:
        out.append(("splits >= 64: the slab-reduce kernel", "wgrad", layer, bconv, lo, hi, lambda p: p.wave_reduce, anycase))
    return out


def test_cases_cover_every_engine_and_threshold():
    """CPU-side.  CASES reaches every (layer, pass, engine) the plans can select in the default build with the bconv
    switch on and off, both sides of every routing threshold of every layer that has it, a ragged image count for every
    images-per-workgroup factor of the scatter configurations, and the update's own count for every (layer, pass, engine)
    that count can reach."""
    reached = {(c.layer, c.kind, engine_of(c)) for c in CASES}
    want = selectable()
    assert not (want - reached), f"no case reaches {sorted(want - reached)}"
    assert not (reached - want), sorted(reached - want)
    for layer, kind, engine in NOT_REACHABLE:
        assert (layer, kind, engine) not in want, "reachable after all: give it cases and take it off NOT_REACHABLE"
    # the engines are table entries: NOT_REACHABLE names what the table holds and the plans never return
    assert TABLE[5].wgrad_bf and TABLE[5].tw_nbk
    for layer in TABLE:   # both settings of the switch wherever it changes anything
        for kind in ("down", "up", "wgrad"):
            for bconv in _bconv_settings(layer, kind):
                assert any(c.layer == layer and c.kind == kind and c.bconv == bconv for c in CASES), (layer, kind, bconv)
    for what, kind, layer, bconv, lo, hi, prop, keep in thresholds():
        sides = {}
        for c in CASES:
            if (c.kind, c.layer, c.bconv, c.ws) == (kind, layer, bconv, "full") and c.nimg in (lo, hi) and keep(c):
                sides.setdefault(c._replace(nimg=0), {})[c.nimg] = prop(plan_of(c))
        pairs = [s for s in sides.values() if len(s) == 2 and s[lo] != s[hi]]
        assert pairs, f"{what}: layer {layer} {kind} (bconv {bconv}) has no pair of cases at {lo} | {hi} images that differ"
    for layer, gi in ((2, 4), (10, 4), (4, 5), (3, 8)):
        assert gi in (TABLE[layer].up_scatter, TABLE[layer].up_bf)
        for bconv in _bconv_settings(layer, "up"):
            assert any(c.kind == "up" and c.layer == layer and c.bconv == bconv and c.nimg > gi and c.nimg % gi for c in CASES), (layer, gi)
    # the update's count: every engine it can select there
    for layer in TABLE:
        n = FULL[layer]
        at_full = {(c.kind, engine_of(c)) for c in CASES if c.layer == layer and c.nimg == n}
        for kind in ("down", "up", "wgrad"):
            for bconv in (1, 0):
                for epi in (EPI_NONE, EPI_RELU, EPI_MUL_DRELU):
                    e = {"down": lambda: down_plan(layer, n, epi, epi == EPI_RELU, False, False, False, "full", bconv).engine,
                         "up": lambda: up_plan(layer, n, epi, bconv),
                         "wgrad": lambda: wgrad_plan(layer, n, False, False, bconv).engine}[kind]()
                    assert (kind, e) in at_full, (layer, kind, e, n)
    # the plan of the issue's figures: images per split at the update's count
    assert wgrad_plan(5, 2450, bconv=0).ips == 11 and wgrad_plan(2, 2450).ips == 40 and wgrad_plan(4, 2450).ips == 44
    assert wgrad_plan(0, 2450).splits == 2450 and wgrad_plan(13, 2450).splits == 613
    assert wgrad_plan(1, 300).ips == 3 and wgrad_plan(1, 129).ips == 2 and wgrad_plan(1, 128).ips == 1


# ----------------------------------------------------------------------------- GPU side
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from repo_amd import ops as o

    return o


@pytest.fixture(autouse=True)
def _poison_lds(request):
    """Start every GPU test from NaN-filled LDS on all CUs: reads of never-written LDS cannot hide."""
    if "gpu" in request.keywords:
        from repo_amd._lib import lib

        assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
    yield


FAMILY = list(CONV_ENGINE_KERNELS) + list(CONV_REDUCE_KERNELS)   # tests/util.py: the one list of these names
PACKERS = ["bconv_pack_kernel", "tconv_down_pack_kernel", "uconv_pack_kernel", "buconv_pack_kernel", "dconv_up_pack_kernel",
           "tconv_up_pack_kernel"]
KERNEL_OF = {"Fp32Lat": "dconv_down_kernel", "Fp32": "dconv_down_kernel", "Bf16": "bconv_down_kernel", "Tcd": "tconv_down_kernel",
             "Tconv": "tconv_up_kernel", "BfScatter": "buconv_scatter_kernel", "Scatter": "uconv_scatter_kernel",
             "Direct": "dconv_up_kernel", "Merged": "igemm_kernel"}
WGRAD_KERNEL_OF = {"Transposing": "tconv_wgrad_kernel", "Bf16": "bconv_wgrad_kernel", "Fp32": "dconv_wgrad_kernel"}


def family_ran(names):
    return {k for k in FAMILY if has(names, rf"\b{k}\b")}


def assert_kernels(names, expected, what, tile=None):
    """Exactly the conv kernels of the expected engine ran; where the layer has a latency and a throughput tile, the
    DTile<...> of the instantiation is the expected one."""
    ran = family_ran(names)
    assert ran == set(expected), (what, "expected", sorted(expected), "ran", sorted(ran), names)
    if tile is not None:
        spelled = "DTile<" + ",".join(str(v) for v in tile) + ","
        inst = [n.replace(" ", "") for n in names if re.search(r"\bdconv_down_kernel\b", n)]
        assert inst and all(spelled in n for n in inst), (what, spelled, inst)


def per_slice(got, want):
    """max |got - want| over a slice (dim 0) / max |want| over that slice, the worst slice; NaN-propagating."""
    got, want = got.double().flatten(1), want.flatten(1)
    err = (got - want).abs().amax(1) / (want.abs().amax(1) + 1e-300)
    return float(err.max()) if not bool(torch.isnan(err).any()) else float("nan")


def _chunks(n, step=64):
    return [(i, min(n, i + step)) for i in range(0, n, step)]


class Data:
    """Inputs of one (layer, count), and the float64 references of the UNSCALED operands, each computed once on the CPU in
    image chunks and kept on the device (a power-of-two scale per image / row carries over to the reference exactly)."""

    def __init__(self, layer, nimg):
        cb, cs, hb, ks, hs, ps = geo(layer)
        self.layer, self.nimg = layer, nimg
        g = torch.Generator().manual_seed(1000 * layer + nimg)
        self.big0 = torch.randn(nimg, cb, hb, hb, generator=g)
        self.small0 = torch.randn(nimg, cs, hs, hs, generator=g)
        self.w = torch.randn(cs, cb, ks, ks, generator=g) * 0.1
        self.bias_s, self.bias_b = torch.randn(cs, generator=g), torch.randn(cb, generator=g)
        # powers of two from 2^-8 .. 2^8: one per image (down, up), one per channel of `small` (weight gradient)
        self.simg = torch.pow(2.0, torch.randint(-8, 9, (nimg,), generator=g).float())
        self.srow = torch.pow(2.0, torch.randint(-8, 9, (cs,), generator=g).float())
        self.h_s = F.relu(torch.randn(nimg, cs, hs, hs, generator=g))   # saved activations: the epilogues' operand
        self.h_b = F.relu(torch.randn(nimg, cb, hb, hb, generator=g))
        self.u8 = torch.randint(0, 256, (nimg, cb, hb, hb), generator=g, dtype=torch.uint8) if layer in U8_LAYERS else None
        # the weight gradient's operands: db[r] and dbig[c] are ONE sum each, and a sum of zero-mean terms cancels to anywhere
        # between 0 and a few roots of its sum of squares -- no fp32 summation is bounded relative to such a sum (torch's own
        # float32 sum of standard-normal `small`: 6.5e-4 of |want| on encoder conv2's worst row at 128 images).  So `small`
        # carries an offset of +-(1 .. 2) per channel, and in the cases that ask for dbig `big` does too: the sums do not
        # cancel and are judged per row against |want| like dw.  dw itself stays a sum of zero-mean products wherever
        # `big` has no offset (every "db" case, at every count and engine).
        sign = lambda k: torch.randint(0, 2, (k,), generator=g).float() * 2 - 1   # noqa: E731
        self.off_s = sign(cs) * (1 + torch.rand(cs, generator=g))
        self.off_b = sign(cb) * (1 + torch.rand(cb, generator=g))
        self._dev, self._ref = {}, {}

    @property
    def small_w(self):
        return self.small0 + self.off_s.view(1, -1, 1, 1)

    @property
    def big_w(self):
        return self.big0 + self.off_b.view(1, -1, 1, 1)

    def dev(self, name):
        if name not in self._dev:
            self._dev[name] = getattr(self, name).cuda()
        return self._dev[name]

    def frames(self):   # the uint8 frames as the kernels read them: ((x / 255) * 2) - 1 in float32
        return (self.u8.float() / 255.0) * 2.0 - 1.0

    def ref(self, what):
        if what not in self._ref:
            w64, n = self.w.double(), self.nimg
            hb = geo(self.layer)[2]
            if what in ("down", "down_u8"):
                big = self.big0 if what == "down" else self.frames()
                r = torch.cat([F.conv2d(big[i:j].double(), w64, None, stride=2) for i, j in _chunks(n)])
            elif what == "up":
                r = torch.cat([F.conv_transpose2d(self.small0[i:j].double(), w64, None, stride=2) for i, j in _chunks(n)])
                r = F.pad(r, (0, hb - r.shape[3], 0, hb - r.shape[2]))   # encoder conv2: row / column 30 of 31 stay zero
            elif what in ("dw", "dw_ob", "dw_u8"):   # _ob: `big` with its channel offsets
                big = {"dw": self.big0, "dw_u8": None, "dw_ob": None}[what]
                big = self.frames() if what == "dw_u8" else self.big_w if what == "dw_ob" else big
                small, r = self.small_w, torch.zeros_like(w64)
                for i, j in _chunks(n, 50):
                    r += torch.nn.grad.conv2d_weight(big[i:j].double(), w64.shape, small[i:j].double(), stride=2)
            elif what == "db":
                r = self.small_w.double().sum((0, 2, 3))
            elif what == "dbig":
                r = self.big_w.double().sum((0, 2, 3))
            self._ref[what] = r.cuda()
        return self._ref[what]


_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    """The last (layer, count)'s device tensors do not outlive the module."""
    yield
    _cache.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def data(layer, nimg):
    if (layer, nimg) not in _cache:
        _cache.clear()   # one (layer, count) at a time: the update's counts are gigabytes of float64
        torch.cuda.empty_cache()
        _cache[(layer, nimg)] = Data(layer, nimg)
    return _cache[(layer, nimg)]


@pytest.fixture
def bconv():
    from repo_amd._lib import lib

    prev = lib().repo_debug_bconv(1)
    lib().repo_debug_bconv(prev)
    yield lambda on: lib().repo_debug_bconv(int(on))
    lib().repo_debug_bconv(prev)


def quad_mask(h):
    flat = h.reshape(-1)
    bits = (torch.cat([flat, torch.zeros((-flat.numel()) % 4)]).reshape(-1, 4) > 0).to(torch.uint8)
    return bits[:, 0] | (bits[:, 1] << 1) | (bits[:, 2] << 2) | (bits[:, 3] << 3)


def channel_quad_mask(h):
    n, c = h.shape[:2]
    bits = (h > 0).to(torch.uint8).view(n, c // 4, 4, -1)
    return (bits[:, :, 0] | (bits[:, :, 1] << 1) | (bits[:, :, 2] << 2) | (bits[:, :, 3] << 3)).contiguous().view(-1)


def _view(s, t):
    return s.view(-1, *([1] * (t.dim() - 1)))


def _down_raw(ops, c, d, big, bias, out, ws_bytes):
    """repo_conv_down through lib() with a workspace of exactly ws_bytes (0: none)."""
    from repo_amd._lib import lib

    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda") if ws_bytes else None
    dbias = torch.empty(geo(c.layer)[1], device="cuda") if c.opt == "dbias" else None
    rc = lib().repo_conv_down(c.layer, c.nimg, big.data_ptr(), int(c.u8), d.dev("w").data_ptr(), bias.data_ptr(), out.data_ptr(),
                              EPIS[c.epi][0], None, dbias.data_ptr() if dbias is not None else None, 0, None,
                              ws.data_ptr() if ws is not None else None, ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def run_down(ops, c):
    from repo_amd._lib import lib

    d, plan = data(c.layer, c.nimg), plan_of(c)
    cb, cs, hb, ks, hs, ps = geo(c.layer)
    epi, has_bias = EPIS[c.epi]
    what = case_id(c)
    bias = d.dev("bias_s") if has_bias else None
    s = d.dev("simg")
    big = d.dev("u8") if c.u8 else d.dev("big0") * _view(s, d.big0)
    ref0 = d.ref("down_u8" if c.u8 else "down")
    want = ref0 if c.u8 else ref0 * _view(s.double(), ref0)
    if has_bias:
        want = want + d.dev("bias_s").double().view(1, -1, 1, 1)
    if epi == EPI_RELU:
        want = F.relu(want)
    aux = None
    if epi in (EPI_MUL_DRELU, EPI_MUL_MASK4):
        want = want * (d.dev("h_s") > 0)
        aux = d.dev("h_s") if epi == EPI_MUL_DRELU else quad_mask(d.h_s).cuda()
    expected = [KERNEL_OF[plan.engine]]
    if c.ws != "full":
        # no room for the weight pack: the plan's fp32 engine and a correct result, or REPO_E_WS_TOO_SMALL
        full = lib().repo_conv_down_workspace_bytes(c.layer, c.nimg)
        lay, px = TABLE[c.layer], c.nimg * ps   # the query: the larger pack + the larger partials of the float / uint8 plans
        pack = full - max(cdiv(px, lay.down_bf or lay.down[1]), cdiv(px, lay.down_bf_u8 or lay.down[1])) * cs * 4
        assert 0 < pack < full
        out = torch.full((c.nimg, cs, hs, hs), float("nan"), device="cuda")
        if plan.rc == E_WS_TOO_SMALL:
            assert _down_raw(ops, c, d, big, bias, out, 0) == E_WS_TOO_SMALL
            assert bool(torch.isnan(out).all()), "a refused call wrote its output"
            log(f"conv {what}: REPO_E_WS_TOO_SMALL as planned, output untouched")
            return
        rc, names = traced(lambda: _down_raw(ops, c, d, big, bias, out, pack - 1 if c.ws == "short" else 0))
        assert rc == OK
        assert_kernels(names, expected, what, plan.tile)
        e = per_slice(out, want)
        log(f"conv {what}: engine {plan.engine} ran; worst per-image error {e:.2e}")
        assert e < TOL
        return
    kw = {}
    if c.opt.startswith("dbias"):
        kw = dict(dbias=torch.full((cs,), 3.0, device="cuda") if c.opt == "dbias_acc" else torch.empty(cs, device="cuda"),
                  accumulate_dbias=c.opt == "dbias_acc")
    if c.opt == "cmask":
        kw = dict(want_cmask=True)
    got, names = traced(lambda: ops.conv_down(c.layer, big, d.dev("w"), bias, epi=epi, aux=aux, **kw))
    assert_kernels(names, expected, what, plan.tile)
    cmask = None
    if c.opt == "cmask":
        got, cmask = got
    e = per_slice(got, want)
    log(f"conv {what}: engine {plan.engine} ran; worst per-image error {e:.2e}")
    assert e < TOL, (what, e)
    if cmask is not None:   # the mask is the written activation's signs, bit for bit
        assert torch.equal(cmask, channel_quad_mask(got)), what
    if c.opt.startswith("dbias"):   # the channel sums of what it wrote (+ 3 when accumulating), per channel
        # one sum per channel of what the call wrote.  Where it does not cancel (ReLU outputs) it is judged against |want|;
        # where it does (zero-mean outputs: no fp32 summation is bounded relative to such a sum) against the root of the
        # sum of squares of the written values, the size the sum has when it does not cancel: the larger of the two per
        # channel.  A channel ReLU switched off entirely must sum to exactly 0.  The figure against |want| is logged.
        pre = 3.0 if c.opt == "dbias_acc" else 0.0
        sums = got.double().sum((0, 2, 3)) + pre
        err = (kw["dbias"].double() - sums).abs()
        scale = torch.maximum(sums.abs(), got.double().pow(2).sum((0, 2, 3)).sqrt() + pre)
        eb = float((err / (scale + 1e-300)).max()) if not bool(torch.isnan(err).any()) else float("nan")
        log(f"conv {what}: channel sums, worst channel {eb:.2e} of max(|want|, root of the sum of squares), "
            f"{float((err / (sums.abs() + 1e-300)).max()):.2e} of |want|")
        assert eb < TOL, (what, "dbias", eb)
    # a twin call stays on THIS call's engine: channel sums are a routing input (tconv_down.h takes neither them nor the
    # quad mask), so the twin asks for them wherever the plan says that keeps the engine
    def twin_kw(twin_epi, wants):
        for dbias in (wants, not wants):
            if down_plan(c.layer, c.nimg, twin_epi, False, dbias, False, False, "full", c.bconv).engine == plan.engine:
                return dict(dbias=torch.empty(cs, device="cuda")) if dbias else {}
        raise AssertionError((what, "no twin call on the same engine"))

    if epi == EPI_MUL_MASK4:   # the quad mask selects what the activation selects, bit for bit
        twin = ops.conv_down(c.layer, big, d.dev("w"), None, epi=EPI_MUL_DRELU, aux=d.dev("h_s"), **twin_kw(EPI_MUL_DRELU, False))
        assert torch.equal(got, twin), what
    if not has_bias and not c.u8:
        # the scaling law: image i on the scaled batch = 2^k_i x image i on the unscaled batch, bit for bit
        got0 = ops.conv_down(c.layer, d.dev("big0"), d.dev("w"), None, epi=epi, aux=aux, **twin_kw(epi, c.opt.startswith("dbias")))
        assert torch.equal(got, got0 * _view(s, got0)), (what, "an image's result depends on another image's scale")


def run_up(ops, c):
    d, engine = data(c.layer, c.nimg), plan_of(c)
    cb, cs, hb, ks, hs, ps = geo(c.layer)
    epi, has_bias = EPIS[c.epi]
    what = case_id(c)
    bias = d.dev("bias_b") if has_bias else None
    s = d.dev("simg")
    small = d.dev("small0") * _view(s, d.small0)
    ref0 = d.ref("up")
    want = ref0 * _view(s.double(), ref0)
    if has_bias:
        want = want + d.dev("bias_b").double().view(1, -1, 1, 1)
    if epi == EPI_RELU:
        want = F.relu(want)
    aux = None
    if epi in (EPI_MUL_DRELU, EPI_MUL_CMASK):
        want = want * (d.dev("h_b") > 0)
        aux = d.dev("h_b") if epi == EPI_MUL_DRELU else channel_quad_mask(d.h_b).cuda()
    pack = ops.conv_up_pack(c.layer, d.dev("w")) if c.opt == "pack" else None
    if c.opt == "pack":
        assert pack is not None
    got, names = traced(lambda: ops.conv_up(c.layer, small, d.dev("w"), bias, epi=epi, aux=aux, pack=pack))
    assert_kernels(names, [KERNEL_OF[engine]], what)
    if pack is not None:   # packed ahead: the call packs nothing, and gives the bits of the call that packs itself
        assert not any(has(names, rf"\b{k}\b") for k in PACKERS), (what, names)
        assert torch.equal(got, ops.conv_up(c.layer, small, d.dev("w"), bias, epi=epi, aux=aux)), what
    e = per_slice(got, want)
    log(f"conv {what}: engine {engine} ran; worst per-image error {e:.2e}")
    assert e < TOL, (what, e)
    if hb != 2 * (hs - 1) + ks and not has_bias:   # encoder conv2's 31 x 31 data gradient: no window reaches row / column 30
        assert float(got[:, :, -1, :].abs().max()) == 0.0 and float(got[:, :, :, -1].abs().max()) == 0.0, what
    if epi == EPI_MUL_CMASK:
        assert torch.equal(got, ops.conv_up(c.layer, small, d.dev("w"), None, epi=EPI_MUL_DRELU, aux=d.dev("h_b"))), what
    if not has_bias:
        got0 = ops.conv_up(c.layer, d.dev("small0"), d.dev("w"), None, epi=epi, aux=aux)
        assert torch.equal(got, got0 * _view(s, got0)), (what, "an image's result depends on another image's scale")


def run_wgrad(ops, c):
    from repo_amd._lib import lib

    d, plan = data(c.layer, c.nimg), plan_of(c)
    cb, cs, hb, ks, hs, ps = geo(c.layer)
    what = case_id(c)
    s = d.dev("srow")
    wants_dbig = "dbig" in c.opt
    small0 = d.dev("small_w")
    small = small0 * s.view(1, -1, 1, 1)
    big = d.dev("u8") if c.u8 else d.dev("big_w" if wants_dbig else "big0")
    want_dw = d.ref("dw_u8" if c.u8 else "dw_ob" if wants_dbig else "dw") * _view(s.double(), d.w)
    want_db = d.ref("db") * s.double()
    # the mirror's splits against the library's own plan: the workspace it asks for
    assert lib().repo_conv_wgrad_workspace_bytes(c.layer, c.nimg) == wgrad_plan(c.layer, c.nimg, False, False, c.bconv).need, what
    acc = c.opt == "dbig_acc"
    want_bias = "db" in c.opt.split("_")
    dbig = (torch.full((cb,), 2.0, device="cuda") if acc else torch.empty(cb, device="cuda")) if wants_dbig else None
    dw = torch.ones(cs, cb, ks, ks, device="cuda") if acc else None
    (dw, db), names = traced(lambda: ops.conv_wgrad(c.layer, small, big, dw=dw, accumulate=acc, want_bias=want_bias, dbig=dbig))
    expected = [WGRAD_KERNEL_OF[plan.engine], "conv_slab_reduce_wave_kernel" if plan.wave_reduce else "conv_slab_reduce_kernel"]
    if dbig is not None and not plan.dbig_in_slabs:
        expected.append("channel_sum_kernel")
    assert_kernels(names, expected, what)
    errs = {"dw": per_slice(dw, want_dw + (1.0 if acc else 0.0))}
    if want_bias:
        errs["db"] = per_slice(db.view(-1, 1), want_db.view(-1, 1))
    if dbig is not None:
        errs["dbig"] = per_slice(dbig.view(-1, 1), (d.ref("dbig") + (2.0 if acc else 0.0)).view(-1, 1))
    log(f"conv {what}: engine {plan.engine} ran ({plan.ips} images per split, {plan.splits} slabs, "
        f"{'wave' if plan.wave_reduce else 'plain'} reduce); worst per-row error " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < TOL for v in errs.values()), (what, errs)
    if not acc:
        # the scaling law: row r with `small`'s channel r scaled = 2^k_r x the unscaled row, bit for bit
        dw0, db0 = ops.conv_wgrad(c.layer, small0, big, want_bias=want_bias)
        assert torch.equal(dw, dw0 * _view(s, dw0)), (what, "a row of dw depends on another row's scale")
        if want_bias:
            assert torch.equal(db, db0 * s), (what, "db")


# One test per (layer, count, pass, switch): its epilogues and extras run one after the other, each under its own device
# trace and from freshly poisoned LDS, and every failing case is reported, not only the first.
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault((_c.layer, _c.nimg, _c.kind, _c.bconv), []).append(_c)


def group_id(key):
    layer, nimg, kind, on = key
    return f"{TABLE[layer].name}-{kind}-n{nimg}-{'bf' if on else 'fp32'}"


@gpu
@pytest.mark.parametrize("key", list(GROUPS), ids=group_id)
def test_conv_engine(ops, bconv, key):
    """The cases of CASES at one (layer, count, pass, switch).  For each: the mirrored plan's engine ran (device trace), the
    result is within TOL of float64 per image (down, up) or per row (weight gradient), masks and packs agree bit for bit,
    and the power-of-two law holds."""
    from repo_amd._lib import lib

    bconv(key[3])
    failed = []
    for c in GROUPS[key]:
        assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
        try:
            {"down": run_down, "up": run_up, "wgrad": run_wgrad}[c.kind](ops, c)
        except AssertionError as e:
            failed.append(f"{case_id(c)}: {str(e)[:1500]}")
    assert not failed, f"{len(failed)} of {len(GROUPS[key])} cases failed:\n" + "\n".join(failed)


@gpu
@pytest.mark.parametrize("layer", sorted(TABLE))
def test_no_images_is_ok_and_writes_nothing(ops, layer):
    """nimg == 0: repo_conv_down / repo_conv_up return REPO_OK, repo_conv_wgrad refuses it with REPO_E_SHAPE (a gradient over
    no images is the caller's mistake), and all three leave a NaN-filled output as it was."""
    from repo_amd._lib import lib

    cb, cs, hb, ks, hs, ps = geo(layer)
    w = torch.randn(cs, cb, ks, ks).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    small = torch.full((1, cs, hs, hs), float("nan"), device="cuda")
    big = torch.full((1, cb, hb, hb), float("nan"), device="cuda")
    assert lib().repo_conv_down(layer, 0, big.data_ptr(), 0, w.data_ptr(), None, small.data_ptr(), EPI_NONE, None, None, 0, None,
                                None, 0, stream) == OK
    assert lib().repo_conv_up(layer, 0, small.data_ptr(), w.data_ptr(), None, big.data_ptr(), EPI_NONE, None, 0, None, 0, stream) == OK
    dw = torch.full((cs, cb, ks, ks), float("nan"), device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    assert lib().repo_conv_wgrad(layer, 0, small.data_ptr(), big.data_ptr(), 0, dw.data_ptr(), None, None, 0, ws.data_ptr(),
                                 ws.numel(), stream) == E_SHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(small).all()) and bool(torch.isnan(big).all()) and bool(torch.isnan(dw).all())
