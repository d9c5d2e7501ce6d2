"""Bit-exact integer probes of the conv kernels (test_exact_probe_cpu.py, test_gpu_conv_exact.py, test_gpu_ops_exact.py).  Plain module, no fixtures.

When every stored activation, weight, bias and PReLU slope of a layer is a small integer times a power of two, every fp16 x fp16 product and
every partial sum of its convolution is exactly representable in fp32: the fp32 accumulator then holds the same number whatever the summation
order, the tile shape, the K split or the MFMA shape, and the stored fp16 value is the round-to-nearest-even of ONE exact number.  A float64
reference that rounds every node to fp16 states it bit for bit -- for every kernel variant, whichever variant runs the layers in front.

  int_params       such weights, biases (where a node has one) and slopes for a Net
  bn_params        BatchNorm parameters whose fold is such a layer again: scale = +-2 ** k, zero running mean, integer shift (below)
  reference        the net in float64, every fp16 tensor rounded with numpy's astype(np.float16) and every BatchNorm evaluated as its ideal
                   affine (oracle.nets.run_net(dtype, store, bn))
  check_exactness  the CONDITIONS under which the comparison may be exact and can see a fault, asserted on the reference alone
  assert_same_bits the comparator: finite, then equality of the fp16 values (+0 == -0), with positions / bit patterns / ulp histogram on failure
  PROBES           the probe nets: a 3 -> 64 stem, a 1x1 widening conv where the op needs more channels, then the op under test
  split_mirror     the split-K plan a net that does not autotune launches (csrc/conv.hip conv_plan, FID_CONV_FORCE, gemm_launch), SPLIT_CASES

Two node kinds besides convs: an FC (fold_fc, fc_columns, eval_fc: an fp32 tensor of exact sums on the activation's stored HWC order with padded
channels; every K-step must change an output of every image, CHW-ordered columns must give another result) and a max pool (eval_pool: the
source's grid; every window position is somewhere the strict maximum, and zero padding shows where the source is negative).

BatchNorm with a zero running mean is in scope.  gamma / sqrt(var + eps) is no exact power of two, but exactness only needs the constants the
device RECEIVES to be the ideal ones: with var = float32(1 - 1e-5) and gamma = +-2 ** k the scale is 2 ** k (1 + d), |d| < 2 ** -26, and the fp16
folded weights W a1 a2 and the fp32 bias rows round to the values of the ideal affine x * gamma + beta (test_exact_probe_cpu.py lowers every BN
probe both ways and compares the blobs byte for byte).  Two constraints keep a bias row from cancelling down to a ~1e-7 residue where the
ideal value is 0: running means are 0, and a conv with a BatchNorm in front has a post-BN whose shift is 0.  The BN nodes carry no conv bias
(as in IResNet).  A BatchNorm in front of a zero-padded 3x3 conv folds into NINE bias rows, one per border class (lower.py fold_conv): fold_node
states that fold, eval_node applies it per pixel, and check_exactness asserts that a wrong class at any border pixel changes a stored value.
Nonzero running means stay with the tolerance tests."""
import functools
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np
import torch
import torch.nn.functional as F

from oracle import align, nets as onets
from scrfd_arcface_facerecognition_amd.archs import Conv, Net
from scrfd_arcface_facerecognition_amd.lower import OP_DWCONV, T_CP, T_H, T_W, W_DST, W_KH, W_KW, W_PAD, W_SRC, W_TYPE

IN_MEAN, IN_SCALE = 127.5, 2.0        # the first conv reads 2 p - 255 with weights W * in_scale / 2 = W (lower.py): exact as well
PIXELS = (120, 136)                   # |2 p - 255| <= 15
GUARD = 2.0 ** 22                     # partial sums stay two bits under fp32's 24 (an MFMA may align its addends to the largest exponent)
F16_MAX = 65504.0


# ---- parameters --------------------------------------------------------------------------------------------------------------------------

def int_params(net, seed, layers=None):
    """{name: float32 array} for every conv node of `net`: weights = signed integers from `mags` at `density`, times 2 ** `exp`; integer biases
    in +-`bias` times 2 ** `exp`; PReLU slopes from {0.5, 0.25}.  layers: {node name: overrides of density / mags / exp / bias}.  Every value is
    exactly representable in fp16."""
    rng = np.random.default_rng(seed)
    P = {}
    for n in net.nodes:
        if n.kind == "dethead":                               # integer weights and biases, bbox.scale = 1: the fp32 bbox / kps channels are exact sums
            for part, c in (("cls", n.num_anchors), ("bbox", 4 * n.num_anchors), ("kps", 10 * n.num_anchors)):
                shape = (c, n.cin, n.k, n.k)
                P[f"{n.wname}.{part}.weight"] = (rng.choice((1, 2), shape) * rng.choice([-1, 1], shape)).astype(np.float32)     # dense: every column reaches each of the few couts' block
                P[f"{n.wname}.{part}.bias"] = rng.integers(-64, 65, c).astype(np.float32)
            P[n.wname + ".bbox.scale"] = np.ones(1, np.float32)
            continue
        if n.kind == "maxpool":
            continue
        if n.kind == "fc":                                    # integer weights [cout, c * h * w] (CHW columns, as the graph holds them) and biases
            o = dict(density=1.0 / 3.0, mags=(1, 2), exp=0, bias=8)
            o.update((layers or {}).get(n.name, {}))
            shape = (n.cout, n.c * n.h * n.w)
            w = rng.choice(o["mags"], shape) * rng.choice([-1, 1], shape) * (rng.random(shape) < o["density"])
            P[n.wname + ".weight"] = (w * 2.0 ** o["exp"]).astype(np.float32)
            if n.bias:
                P[n.wname + ".bias"] = (rng.integers(-o["bias"], o["bias"] + 1, n.cout) * 2.0 ** o["exp"]).astype(np.float32)
            continue
        assert n.kind == "conv", n.name                       # (a node's BatchNorms: bn_params)
        o = dict(density=1.0 if (n.src == "input" or n.groups > 1) else 1.0 / 3.0, mags=(1,) if n.src == "input" else (1, 2), exp=0, bias=8,
                 slopes=(0.5, 0.25))
        o.update((layers or {}).get(n.name, {}))
        shape = (n.cout, n.cin // n.groups, n.k, n.k)
        w = rng.choice(o["mags"], shape) * rng.choice([-1, 1], shape) * (rng.random(shape) < o["density"])
        P[n.wname + ".weight"] = (w * 2.0 ** o["exp"]).astype(np.float32)
        if n.bias:
            P[n.wname + ".bias"] = (rng.integers(-o["bias"], o["bias"] + 1, n.cout) * 2.0 ** o["exp"]).astype(np.float32)
        if n.act == "prelu":
            P[n.wname + ".prelu"] = rng.choice(o["slopes"], n.cout).astype(np.float32)
    for k, v in P.items():
        assert np.array_equal(v.astype(np.float16).astype(np.float32), v), k
    return P


BN_VAR = np.float32(1.0 - 1e-5)         # + BN_EPS = 1 + d, |d| < 2 ** -25: the scale gamma / sqrt(var + eps) is gamma (1 + d / 2)


def bn_params(net, seed, layers=None):
    """{name: float32 array} for every BatchNorm of `net` (prefix <wname>.pre_bn / <wname>.post_bn): gamma = a signed power of two from `scales`
    per channel, var = BN_VAR, mean = 0, beta = integers in +-`beta` -- on the BN in front as well, so that the nine bias rows differ -- and 0
    on the post-BN of a conv that has a BN in front.  layers: {"<node name>.pre_bn" | "<node name>.post_bn": overrides of scales / beta}."""
    rng = np.random.default_rng(seed)
    P = {}
    for n in net.nodes:
        if n.kind not in ("conv", "fc"):
            continue
        for which, c in (("pre_bn", n.cin if n.kind == "conv" else n.c), ("post_bn", n.cout)):
            if not getattr(n, which):
                continue
            assert n.kind == "fc" or not n.bias, n.name       # (bias a2 (1 + d) + beta2 would cancel: see the module docstring; an FC's bias is
                                                              #  summed with the shift of the BN in front BEFORE the scale, and its post-BN shift is 0)
            o = dict(scales=(1.0, 0.5), beta=8)
            o.update((layers or {}).get(f"{n.name}.{which}", {}))
            pre = f"{n.wname}.{which}"
            P[pre + ".gamma"] = (rng.choice(o["scales"], c) * rng.choice([-1, 1], c)).astype(np.float32)
            P[pre + ".var"] = np.full(c, BN_VAR, np.float32)
            P[pre + ".mean"] = np.zeros(c, np.float32)
            beta = rng.integers(-o["beta"], o["beta"] + 1, c)
            P[pre + ".beta"] = (beta * (0 if which == "post_bn" and n.pre_bn else 1)).astype(np.float32)
    return P


def ideal_affine(P, prefix):
    """(A, B) of a bn_params BatchNorm as the affine x * A + B it stands for, float64"""
    assert (P[prefix + ".mean"] == 0).all() and (P[prefix + ".var"] == BN_VAR).all(), prefix
    a = P[prefix + ".gamma"].astype(np.float64)
    m, e = np.frexp(np.abs(a))
    assert (m == 0.5).all(), prefix                           # signed powers of two
    return a, P[prefix + ".beta"].astype(np.float64)


INTERIOR, TOP_LEFT, TOP = 4, 0, 1       # border classes (row class * 3 + column class; 0: first row / column, 2: last, 1: between)


def border_classes(H, W):
    """int [H, W]: the border class of every pixel of a zero-padded 3x3 / stride-1 conv's map"""
    assert H >= 2 and W >= 2
    yc = np.where(np.arange(H) == 0, 0, np.where(np.arange(H) == H - 1, 2, 1))
    xc = np.where(np.arange(W) == 0, 0, np.where(np.arange(W) == W - 1, 2, 1))
    return yc[:, None] * 3 + xc[None, :]


def fold_node(n, P):
    """(W [cout, cin / groups, k, k], bias rows [1 or 9, cout]) of a conv node, float64: the layer the device is given.  A BatchNorm in front
    scales the input channels and shifts every tap that lies INSIDE the map: one bias row per border class where the conv pads; the BatchNorm
    behind scales the output channels and shifts the rows.  (An average pool in front stays with the caller.)"""
    W = P[n.wname + ".weight"].astype(np.float64)
    rows = (P[n.wname + ".bias"].astype(np.float64) if n.bias else np.zeros(n.cout))[None, :]
    if n.pre_bn:
        assert n.groups == 1 and not n.pre_avgpool, n.name
        a1, b1 = ideal_affine(P, n.wname + ".pre_bn")
        shift = np.einsum("oikl,i->okl", W, b1)                # what the shift adds through every tap
        W = W * a1[None, :, None, None]
        if n.pad == 0:
            rows = rows + shift.sum(axis=(1, 2))[None, :]
        else:
            assert n.k == 3 and n.pad == 1 and n.stride == 1, n.name
            inside = np.ones((9, 3, 3))
            for cls in range(9):
                yc, xc = divmod(cls, 3)
                if yc != 1:
                    inside[cls, yc, :] = 0                    # the first row has no row above it, the last one none below
                if xc != 1:
                    inside[cls, :, xc] = 0
            rows = rows + np.einsum("okl,ckl->co", shift, inside)
    if n.post_bn:
        a2, b2 = ideal_affine(P, n.wname + ".post_bn")
        W = W * a2[:, None, None, None]
        rows = rows * a2[None, :] + b2[None, :]
    return W, rows


def fold_fc(n, P):
    """(W [cout, c, h, w], bias [cout]) of an FC node, float64: lower.py's fold stated again.  The BatchNorm in front scales the input channels
    and its shift goes through every column into the bias; the BatchNorm behind scales the rows and shifts the bias."""
    W = P[n.wname + ".weight"].astype(np.float64).reshape(n.cout, n.c, n.h, n.w)
    b = P[n.wname + ".bias"].astype(np.float64) if n.bias else np.zeros(n.cout)
    if n.pre_bn:
        a1, b1 = ideal_affine(P, n.wname + ".pre_bn")
        b = b + np.einsum("ochw,c->o", W, b1)
        W = W * a1[None, :, None, None]
    if n.post_bn:
        a2, b2 = ideal_affine(P, n.wname + ".post_bn")
        W = W * a2[:, None, None, None]
        b = b * a2 + b2
    return W, b


def int_images(seed, batch, hw, pixels=None):
    lo, hi = pixels or PIXELS
    return np.random.default_rng(seed).integers(lo, hi, (batch,) + tuple(hw) + (3,), dtype=np.uint8)



# ---- the exact reference -----------------------------------------------------------------------------------------------------------------

def _r16(y):
    """float64 tensor -> its fp16 rounding (nearest even), as float64"""
    return torch.from_numpy(y.numpy().astype(np.float16).astype(np.float64))


def reference(net, P, images, raw=None):
    """{node name: float64 [B, H, W, C] holding fp16 values} for every conv and max-pool node ([B, cout] float64 for an FC).  raw: a dict that receives the values BEFORE the rounding"""
    out = {}

    def store(name, y):
        if raw is not None:
            raw[name] = y.permute(0, 2, 3, 1).numpy().copy()
        with np.errstate(over="ignore"):
            r = _r16(y)
        out[name] = r.permute(0, 2, 3, 1).numpy().copy()
        return r

    def bn(x, prefix):                                       # the ideal affine, not x / sqrt(var + eps): that lies 1e-9 off the grid and breaks ties
        a, b = ideal_affine(P, prefix)
        sh = (1, -1) + (1,) * (x.dim() - 2)                   # ([B, C, H, W], or [B, C] behind an FC)
        return x * torch.from_numpy(a).view(sh) + torch.from_numpy(b).view(sh)

    blob = align.blob_from_images(list(images), net.in_scale, net.in_mean)
    res = onets.run_net(net, P, blob, keep=[n.name for n in net.nodes], dtype=torch.float64, store=store, bn=bn)
    for n in net.nodes:
        if n.kind == "dethead":                               # an fp32 tensor on the device: (scores, bbox, kps) as float64, not rounded
            out[n.name] = res[n.name]
        elif n.kind == "fc":                                  # fp32 as well: [B, cout] exact sums
            out[n.name] = res[n.name]
            if raw is not None:
                raw[n.name] = res[n.name]
    out["input"] = np.transpose(blob, (0, 2, 3, 1)).astype(np.float64)
    return out


def _nchw(a):
    return torch.from_numpy(np.array(np.transpose(a, (0, 3, 1, 2)), order="C"))       # (always a copy: the cached references are read-only)


def _chunks(n):
    """the pieces the K axis of a conv node is summed in: 32-channel chunks (one kernel row each for a depthwise layer), as weight masks"""
    cin_g = n.cin // n.groups
    masks = []
    if n.groups == 1:
        for c0 in range(0, cin_g, 32):
            m = torch.zeros(1, cin_g, 1, 1, dtype=torch.bool)
            m[:, c0:c0 + 32] = True
            masks.append(m)
    else:
        for r in range(n.k):
            m = torch.zeros(1, 1, n.k, 1, dtype=torch.bool)
            m[:, :, r] = True
            masks.append(m)
    return masks


def eval_node(n, ref, P, mode="exact", rounded=True, arg=None):
    """One conv node from the reference's STORED inputs, [B, H, W, C] as float64 holding fp16 values, in its FOLDED form (fold_node: the weights
    and the bias row of every pixel's border class, as the device computes it; the reference applies the BatchNorms as they stand).  mode:
      exact          float64, one conv
      f32_fwd        float32, the K axis in 32-channel chunks, first to last
      f32_rev        float32, the chunks last to first, the channels of every chunk flipped
      fault_tap      the centre tap does not reach pixel (0, 0) of image 0
      fault_f16acc   the partial sum is rounded to fp16 between the chunks
      fault_rtz      the store rounds toward zero
      fault_border   every pixel takes the interior bias row (a node with border classes)
      fault_class    the top-left corner pixel of the LAST image takes the top-edge row
      fault_kstep    a split-K slab loses one K-step: arg = (bk, Cin_p, step), the columns [step bk, (step + 1) bk) of the (tap, stored channel) axis
      fault_bias_slabs  the bias row is added once per slab: arg = the number of slabs
      fault_row      kernel row `arg` of every filter is missing (the global depthwise conv's row lanes)
    rounded=False: the float64 value before the store (the f32 modes always return the fp32 accumulator's value)"""
    dt = torch.float32 if mode.startswith("f32") else torch.float64
    x = _nchw(ref[n.src]).to(dt)
    if n.pre_avgpool:
        x = F.avg_pool2d(x, 2, 2)
    wf, rows = fold_node(n, P)
    if mode == "fault_kstep":
        bk, cin_p, step = arg
        assert n.groups == 1 and not n.pre_avgpool and (step + 1) * bk <= n.k * n.k * cin_p, (n.name, arg)
        wf = wf.copy()
        for col in range(step * bk, (step + 1) * bk):
            tap, ci = divmod(col, cin_p)
            if ci < wf.shape[1]:                              # (a padded channel multiplies a zero weight anyway)
                wf[:, ci, tap // n.k, tap % n.k] = 0
    elif mode == "fault_bias_slabs":
        rows = rows * arg
    elif mode == "fault_row":
        wf = wf.copy()
        wf[:, :, arg, :] = 0
    w = torch.from_numpy(wf).to(dt)
    conv = lambda xx, ww: F.conv2d(xx, ww, None, n.stride, n.pad, 1, n.groups)
    if mode in ("exact", "fault_rtz", "fault_border", "fault_class", "fault_kstep", "fault_bias_slabs", "fault_row"):
        y = conv(x, w)
    elif mode == "fault_tap":
        y = conv(x, w)
        x0 = torch.zeros_like(x)
        at = n.k // 2 - n.pad                                 # the input pixel under the centre tap of output pixel (0, 0): (0, 0) where the conv pads
        x0[0, :, at, at] = x[0, :, at, at]
        w0 = torch.zeros_like(w)
        w0[:, :, n.k // 2, n.k // 2] = w[:, :, n.k // 2, n.k // 2]
        y = y - conv(x0, w0)                                  # (that product only reaches output pixel (0, 0) of image 0)
    else:
        masks = _chunks(n)
        if mode == "f32_rev":
            masks = masks[::-1]
        y = torch.zeros_like(conv(x, w))
        for m in masks:
            if mode == "f32_rev" and n.groups == 1:
                idx = torch.nonzero(m.flatten()).flatten().flip(0)
                part = F.conv2d(x[:, idx], w[:, idx], None, n.stride, n.pad)
            else:
                part = conv(x, w * m)
            y = y + part
            if mode == "fault_f16acc":
                y = _r16(y)
    if rows.shape[0] == 1:
        assert not mode.startswith("fault_border") and mode != "fault_class", n.name
        y = y + torch.from_numpy(rows[0]).to(dt)[None, :, None, None]
    else:
        cls = np.broadcast_to(border_classes(y.shape[2], y.shape[3]), (y.shape[0], y.shape[2], y.shape[3])).copy()
        if mode == "fault_border":
            cls[:] = INTERIOR
        elif mode == "fault_class":
            assert cls[-1, 0, 0] == TOP_LEFT
            cls[-1, 0, 0] = TOP
        y = y + torch.from_numpy(rows[cls]).to(dt).permute(0, 3, 1, 2)
    if n.res is not None:
        r = _nchw(ref[n.res]).to(dt)
        if n.res_up2:
            r = F.interpolate(r, scale_factor=2, mode="nearest")
        y = y + r
    if n.act == "relu":
        y = F.relu(y)
    elif n.act == "prelu":
        y = F.prelu(y, torch.from_numpy(P[n.wname + ".prelu"]).to(dt))
    y = y.permute(0, 2, 3, 1).numpy()
    if mode.startswith("f32"):
        return y                                              # the fp32 accumulator's value, before the store
    if not rounded:
        return y
    h = y.astype(np.float16)
    if mode == "fault_rtz":
        away = np.abs(h.astype(np.float64)) > np.abs(y)
        h = np.where(away, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float64)


# ---- the conditions ----------------------------------------------------------------------------------------------------------------------

def lsb_of(a):
    """the largest power of two that divides every entry of `a` (1.0 for an all-zero array)"""
    a = np.asarray(a, dtype=np.float64)
    a = a[a != 0]
    if a.size == 0:
        return 1.0
    m, e = np.frexp(np.abs(a))                                # a = m * 2 ** e, 0.5 <= m < 1: m * 2 ** 53 is an integer
    mi = (m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((mi & -mi).astype(np.float64))               # trailing zero bits of the integer significand
    return float(2.0 ** np.min(e - 53 + tz))


def _on_grid(a, g):
    q = np.asarray(a, dtype=np.float64) / g
    return bool(np.all(q == np.round(q)))


def _is_f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a).astype(np.float16).astype(np.float64) == np.asarray(a, dtype=np.float64)


def check_exactness(net, P, images, probed, onchip=(), ref=None, raw=None):
    """Asserts, on the reference alone, that the nodes `probed` of the net may be compared bit for bit and that the comparison has power;
    `onchip`: the nodes a fused op never stores.  ref / raw: reference()'s results where the caller already has them.  Returns the figures
    per node ({name: dict})."""
    if ref is None:
        raw = {}
        ref = reference(net, P, images, raw)
    grid = {"input": 1.0}                                     # 2 p - 255: odd integers
    stats = {}
    for n in net.nodes:
        if n.kind == "dethead":
            stats[n.name] = _check_dethead(n, P, ref, grid[n.src])
            continue
        if n.kind == "fc":
            stats[n.name] = _check_fc(n, P, ref, grid[n.src])
            continue
        if n.kind == "maxpool":                               # a selection: the source's grid, no sum, no rounding
            grid[n.name] = grid[n.src]
            assert np.array_equal(raw[n.name], ref[n.name]) and np.isfinite(ref[n.name]).all(), n.name
            if n.name in probed:
                stats[n.name] = _check_pool(n, ref, grid[n.src])
            continue
        w, b = fold_node(n, P)                                # through both BatchNorms: the folded weights W a1 a2 and the bias rows
        if n.pre_bn or n.post_bn:
            assert _is_f16(w).all() and (np.abs(b) < 2.0 ** 24).all(), (n.name, "folded weights are not fp16 values")
        g = grid[n.src] * lsb_of(w) * (0.25 if n.pre_avgpool else 1.0)
        g = min(g, lsb_of(b))
        if n.pre_bn or n.post_bn:                             # the same grid through both affines as they stand: x A1 + B1, conv, y A2 + B2
            ga = grid[n.src]
            if n.pre_bn:
                a1, b1 = ideal_affine(P, n.wname + ".pre_bn")
                ga = min(ga * lsb_of(a1), lsb_of(b1))
            ga *= lsb_of(P[n.wname + ".weight"]) * (0.25 if n.pre_avgpool else 1.0)
            if n.post_bn:
                a2, b2 = ideal_affine(P, n.wname + ".post_bn")
                ga = min(ga * lsb_of(a2), lsb_of(b2))
            assert ga <= g and _on_grid(g, ga), (n.name, g, ga)     # (the fold can only be coarser: it multiplies the scales channel by channel)
            g = ga
        if n.res is not None:
            g = min(g, grid[n.res])
        g_pre = g
        if n.act == "prelu":
            g *= lsb_of(P[n.wname + ".prelu"])
        grid[n.name] = g
        assert 2.0 ** -24 <= g <= 1.0, (n.name, g)
        # finite values, everywhere
        assert np.abs(raw[n.name]).max() < F16_MAX and np.isfinite(ref[n.name]).all(), (n.name, np.abs(raw[n.name]).max())
        if n.name in onchip:                            # kept on chip by a fused op: the same number as fp16 and as fp32
            assert _is_f16(raw[n.name]).all(), (n.name, "on-chip intermediate needs rounding", np.abs(raw[n.name]).max() / g)
        border = _check_border(n, ref, P, b) if b.shape[0] == 9 else None      # (every border-class node, probed or not)
        if n.name not in probed and n.name not in onchip:
            continue
        # dyadic grid: every operand of the node is a multiple of its tracked lsb
        assert _on_grid(ref[n.src], grid[n.src]) and _on_grid(w, lsb_of(w)) and _on_grid(b, g_pre), n.name
        assert n.res is None or _on_grid(ref[n.res], grid[n.res]), n.name
        assert _on_grid(raw[n.name], g), n.name
        # partial sums: no subset of the addends, in any order, leaves the 24-bit window
        x = _nchw(np.abs(ref[n.src]))
        if n.pre_avgpool:
            x = F.avg_pool2d(x, 2, 2)
        S = F.conv2d(x, torch.from_numpy(np.abs(w)), torch.from_numpy(np.abs(b).max(axis=0)), n.stride, n.pad, 1, n.groups)     # (the largest |bias row|)
        if n.res is not None:
            r = _nchw(np.abs(ref[n.res]))
            S = S + (F.interpolate(r, scale_factor=2, mode="nearest") if n.res_up2 else r)
        bits = float(np.log2(S.max().item() / g))
        assert S.max().item() / g < GUARD, (n.name, bits)
        st = dict(grid=g, sum_bits=bits, max=float(np.abs(raw[n.name]).max()))
        if border is not None:
            st["border"] = border
        if n.name in probed:
            y, h = raw[n.name], ref[n.name]
            inexact = h != y
            with np.errstate(over="ignore"):
                h16 = h.astype(np.float16)
                up = np.nextafter(h16, np.float16(np.inf)).astype(np.float64)
                dn = np.nextafter(h16, np.float16(-np.inf)).astype(np.float64)
            tie = inexact & ((np.abs(y - h) * 2 == np.abs(up - h)) | (np.abs(y - h) * 2 == np.abs(h - dn)))
            st.update(inexact=float(inexact.mean()), ties=float(tie.mean()), nonzero=float((h != 0).mean()))
            assert st["inexact"] >= 0.10 and st["ties"] >= 0.01 and st["nonzero"] >= 0.20, (n.name, st)
            if n.act == "prelu":
                pre = eval_node(_no_act(n), ref, P)
                st["negative"] = float((pre < 0).mean())
                assert (pre < 0).any() and (pre > 0).any(), n.name
            if n.groups == 1:                                 # every (tap, input channel) column reaches some cout of every 64-cout block
                for c0 in range(0, n.cout, 64):
                    assert (np.abs(w[c0:c0 + 64]).sum(axis=0) > 0).all(), (n.name, c0)
            else:
                assert (w != 0).all(), n.name
        stats[n.name] = st
    return stats


def _check_border(n, ref, P, rows):
    """a node with nine border-class bias rows: the rows tell the classes apart, and a wrong class shows.  Every pair of rows differs in at
    least a quarter of the output channels; at every border pixel of every image the interior row in place of the pixel's own changes the stored
    fp16 value of some channel."""
    share = min(float((rows[i] != rows[j]).mean()) for i in range(9) for j in range(i))
    assert share >= 0.25, (n.name, "bias rows too much alike", share)
    good, bad = eval_node(n, ref, P), eval_node(n, ref, P, "fault_border")
    changed = (good != bad).any(axis=3)                       # [B, H, W]
    is_border = border_classes(*changed.shape[1:]) != INTERIOR
    assert not changed[:, ~is_border].any() and changed[:, is_border].all(), (n.name, "a border pixel the interior row does not change",
                                                                             np.argwhere(~changed & is_border[None])[:4].tolist())
    return dict(row_pairs_differ=share, border_pixels=int(is_border.sum()), pixels=int(is_border.size),
                channels_changed=float((good != bad)[:, is_border].mean()))


def _check_dethead(n, P, ref, g_src):
    """the bbox / kps channels of a DetHead: fp32 stores of exact sums (no rounding to see, so only grid, partial sums and coverage)"""
    st = {}
    for part in ("bbox", "kps"):
        w, b = P[f"{n.wname}.{part}.weight"].astype(np.float64), P[f"{n.wname}.{part}.bias"].astype(np.float64)
        g = min(g_src * lsb_of(w), lsb_of(b))
        assert _on_grid(ref[n.src], g_src) and float(P[n.wname + ".bbox.scale"][0]) == 1.0
        S = F.conv2d(_nchw(np.abs(ref[n.src])), torch.from_numpy(np.abs(w)), torch.from_numpy(np.abs(b)), 1, n.k // 2)
        assert S.max().item() / g < GUARD, (n.name, part)
        y = ref[n.name][1 if part == "bbox" else 2]
        assert _on_grid(y, g) and (y != 0).mean() >= 0.20 and (np.abs(w).sum(axis=0) > 0).all(), (n.name, part)
        st[part] = dict(grid=g, sum_bits=float(np.log2(S.max().item() / g)), max=float(np.abs(y).max()))
    return st


def fc_columns(n, ref, P, order="hwc"):
    """(x [B, K], W [cout, K], bias [cout]) of an FC node as the device multiplies them, float64: K = h w Cp, the activation's stored HWC order
    with the channels padded to a multiple of 32 (zeros on both sides).  order="chw": the weight columns left in the graph's CHW order
    (a lowering that forgot the permutation; Cp = c only)."""
    W4, b = fold_fc(n, P)
    x = ref[n.src]                                            # [B, h, w, c]
    B, cp = x.shape[0], (n.c + 31) // 32 * 32
    xk = np.zeros((B, n.h, n.w, cp))
    xk[..., :n.c] = x
    Wk = np.zeros((n.cout, n.h, n.w, cp))
    if order == "chw":
        assert cp == n.c
        Wk = W4.reshape(n.cout, -1)
    else:
        Wk[..., :n.c] = W4.transpose(0, 2, 3, 1)
    return xk.reshape(B, -1), Wk.reshape(n.cout, -1), b


def fc_bk(n):
    """the K-step of the implicit GEMM on the FC's flattened input (csrc/conv.hip conv_plan: 64 where the row length allows it)"""
    K = n.h * n.w * ((n.c + 31) // 32 * 32)
    return 64 if K % 64 == 0 else 32


def eval_fc(n, ref, P, mode="exact", arg=None):
    """One FC node from the reference's stored input, in its folded form and the device's column order; [B, cout] float64.  mode:
      exact          float64
      f32_fwd / f32_rev   float32, K-step by K-step (fc_bk columns each), first to last / last to first
      chw            the weight columns in CHW order
      fault_kstep    K-step `arg` is missing (a slab that drops a step)
      fault_kstep_twice   K-step `arg` is added twice (two slabs that overlap)
      fault_bias_slabs    the bias is added once per slab: arg = the number of slabs"""
    x, W, b = fc_columns(n, ref, P, "chw" if mode == "chw" else "hwc")
    bk = fc_bk(n)
    if mode in ("f32_fwd", "f32_rev"):
        steps = list(range(x.shape[1] // bk))
        y = np.zeros((x.shape[0], n.cout), np.float32)
        for s_ in (steps if mode == "f32_fwd" else steps[::-1]):
            y = y + x[:, s_ * bk:(s_ + 1) * bk].astype(np.float32) @ W[:, s_ * bk:(s_ + 1) * bk].astype(np.float32).T
        return y + b.astype(np.float32)
    y = x @ W.T + b
    if mode in ("fault_kstep", "fault_kstep_twice"):
        part = x[:, arg * bk:(arg + 1) * bk] @ W[:, arg * bk:(arg + 1) * bk].T
        y = y - part if mode == "fault_kstep" else y + part
    elif mode == "fault_bias_slabs":
        y = y + b * (arg - 1)
    else:
        assert mode in ("exact", "chw"), mode
    return y


def _check_fc(n, P, ref, g_src):
    """an FC node: an fp32 store of exact sums (grid, partial sums, coverage), and the two conditions that give the comparison power over a
    split-K plan and over the column order: every K-step changes some output of EVERY image, and CHW-ordered columns give another result"""
    W4, b = fold_fc(n, P)
    assert _is_f16(W4).all() and (np.abs(b) < 2.0 ** 24).all(), (n.name, "folded weights are not fp16 values")
    g = min(g_src * lsb_of(W4), lsb_of(b))
    x, W, _ = fc_columns(n, ref, P)
    assert _on_grid(ref[n.src], g_src) and np.isfinite(x).all(), n.name
    S = np.abs(x) @ np.abs(W).T + np.abs(b)
    bits = float(np.log2(S.max() / g))
    assert 2.0 ** -24 <= g <= 1.0 and S.max() / g < GUARD, (n.name, g, bits)
    y = ref[n.name]
    assert y.shape == (x.shape[0], n.cout) and np.array_equal(y, eval_fc(n, ref, P)), n.name     # (the fold IS the BatchNorms as they stand)
    assert _on_grid(y, g) and np.array_equal(y.astype(np.float32).astype(np.float64), y), n.name
    assert (y != 0).mean() >= 0.20 and (np.abs(W).sum(axis=0)[np.abs(x).sum(axis=0) > 0] > 0).all(), n.name
    bk = fc_bk(n)
    steps = x.shape[1] // bk
    assert steps * bk == x.shape[1]
    part = np.einsum("bsk,osk->bso", x.reshape(x.shape[0], steps, bk), W.reshape(n.cout, steps, bk))
    dead = np.argwhere(~(part != 0).any(axis=2))
    assert dead.size == 0, (n.name, "a K-step that changes no output of an image (image, step)", dead[:4].tolist())
    if (n.c + 31) // 32 * 32 == n.c:
        assert (eval_fc(n, ref, P, "chw") != y).mean() >= 0.5, (n.name, "CHW-ordered columns give the same result")
    return dict(grid=g, sum_bits=bits, max=float(np.abs(y).max()), nonzero=float((y != 0).mean()), ksteps=steps, bk=bk,
                outputs_per_step=float((part != 0).mean()))


def eval_pool(n, ref, mode="exact", arg=None):
    """One max-pool node from the reference's stored input; [B, Ho, Wo, C] float64.  mode:
      exact      taps outside the map are ignored
      fault_pad0 the map is padded with 0 and every tap counts
      fault_row_off   output row `arg` is taken one input row further down (a pooled row from the wrong tile at a seam)"""
    x = _nchw(ref[n.src])
    y = F.max_pool2d(x, n.k, n.stride, n.pad)
    if mode == "fault_pad0":
        y = F.max_pool2d(F.pad(x, (n.pad,) * 4, value=0.0), n.k, n.stride, 0)
    elif mode == "fault_row_off":
        down = torch.cat([x[:, :, 1:], torch.full_like(x[:, :, :1], -np.inf)], dim=2)
        y = y.clone()
        y[:, :, arg] = F.max_pool2d(down, n.k, n.stride, n.pad)[:, :, arg]
    else:
        assert mode == "exact", mode
    return y.permute(0, 2, 3, 1).numpy()


def _check_pool(n, ref, g_src):
    """a max pool: each of the k x k window positions is the STRICT maximum of some interior output and channel (a tap that is never read
    shows), and where the source has negative values, padding with 0 instead of ignoring the taps outside changes a border output"""
    x = _nchw(ref[n.src])
    assert np.array_equal(eval_pool(n, ref), ref[n.name]) and _on_grid(ref[n.name], g_src), n.name
    off = -(-n.pad // n.stride) * n.stride - n.pad            # the first window that lies inside the map
    inner = x[:, :, off:, off:]
    B, C = inner.shape[:2]
    win = F.unfold(inner, n.k, stride=n.stride).view(B, C, n.k * n.k, -1)
    top = win.max(dim=2, keepdim=True).values
    strict = (win == top) & ((win == top).sum(dim=2, keepdim=True) == 1)
    won = strict.any(dim=3).any(dim=1).any(dim=0).numpy()
    assert won.all(), (n.name, "window positions that never hold the strict maximum", np.flatnonzero(~won).tolist())
    st = dict(grid=g_src, positions=float(strict.float().sum(dim=2).mean()), negative=float((ref[n.src] < 0).mean()))
    if (ref[n.src] < 0).any() and n.pad > 0:
        bad = eval_pool(n, ref, "fault_pad0") != ref[n.name]
        Ho, Wo = bad.shape[1:3]
        H, W = ref[n.src].shape[1:3]
        clipped = np.zeros((Ho, Wo), bool)
        for oy in range(Ho):
            for ox in range(Wo):
                clipped[oy, ox] = (oy * n.stride - n.pad < 0 or ox * n.stride - n.pad < 0 or oy * n.stride - n.pad + n.k > H
                                   or ox * n.stride - n.pad + n.k > W)
        assert bad[:, clipped].any() and not bad[:, ~clipped].any(), (n.name, "zero padding changes no border output")
        st["pad0_changes"] = float(bad[:, clipped].mean())
    return st


def _no_act(n):
    import dataclasses
    return dataclasses.replace(n, act="none")


# ---- the comparator ----------------------------------------------------------------------------------------------------------------------

def _ordered(h16):
    b = h16.view(np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def assert_same_bits(got, ref, what=""):
    """got, ref: [B, H, W, C] arrays holding fp16 values.  Both finite, then equal as fp16 (+0 == -0); no tolerance."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all(), f"{what}: not finite"
    g, r = got.astype(np.float16), ref.astype(np.float16)
    assert np.array_equal(g.astype(got.dtype), got) and np.array_equal(r.astype(ref.dtype), ref), f"{what}: not fp16 values"
    if np.array_equal(g, r):
        return
    bad = np.argwhere(g != r)
    ulps = _ordered(g) - _ordered(r)
    vals, counts = np.unique(ulps[g != r], return_counts=True)
    first = ", ".join(f"(n={i}, y={y}, x={x}, c={c}): got 0x{int(g[i, y, x, c].view(np.uint16)):04x} ref 0x{int(r[i, y, x, c].view(np.uint16)):04x}"
                      for i, y, x, c in bad[:6])
    hist = ", ".join(f"{int(v):+d}: {int(k)}" for v, k in zip(vals[:12], counts[:12]))
    raise AssertionError(f"{what}: {len(bad)} of {g.size} values differ; first {first}; difference in fp16 ulps {{{hist}}}")


def assert_same_values(got, ref, what=""):
    """fp32 tensors (the detector head's bbox / kps channels): finite and equal, no tolerance"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all(), f"{what}: not finite"
    bad = np.argwhere(got != ref)
    if len(bad):
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ; first at {i}: got {float(got[i])!r} ref {float(ref[i])!r}")


# ---- the probe nets ----------------------------------------------------------------------------------------------------------------------

@dataclass
class Probe:
    name: str
    net: Net
    P: Dict[str, np.ndarray]
    images: np.ndarray
    probed: List[str]                        # nodes compared bit for bit whose conditions check_exactness asserts
    onchip: List[str] = field(default_factory=list)     # nodes a fused op keeps on chip
    env: Dict[str, str] = field(default_factory=dict)
    through: List[str] = field(default_factory=list)    # nodes held to the probed nodes' conditions that a fused form only shows through a later node

    @property
    def batch(self):
        return self.images.shape[0]


KW = dict(bias=True, post_bn=False)


def _net(hw):
    return Net("t", tuple(hw), IN_MEAN, IN_SCALE)


def _front(net, cin, layers):
    """s (3 -> 64, 3x3, ReLU) [-> x (1x1, 64 -> cin, PReLU)]: the name of the tensor the op under test reads"""
    net.add(Conv("s", "input", 3, 64, act="relu", **KW))
    if cin == 64:
        return "s"
    net.add(Conv("x", "s", 64, cin, k=1, pad=0, act="prelu", **KW))
    layers.setdefault("x", dict(density=0.25, mags=(1,)))
    return "x"


def family_probe(hw, cin, cout, batch, stride=1):
    """both forms of a 3x3 conv on one input: c (cin -> cout, PReLU) and r (ReLU, + residual: the input itself at stride 1, a 1x1 / stride-2
    conv d of it at stride 2)"""
    net, layers = _net(hw), {}
    x = _front(net, cin, layers)
    net.add(Conv("c", x, cin, cout, stride=stride, act="prelu", **KW))
    if stride == 1:
        net.add(Conv("r", x, cin, cin, act="relu", res=x, **KW))
        outs = [x, "c", "r"]
    else:
        net.add(Conv("d", x, cin, cout, k=1, stride=2, pad=0, **KW))
        net.add(Conv("r", x, cin, cout, stride=2, act="relu", res="d", **KW))
        outs = [x, "d", "c", "r"]
    net.outputs = outs
    dense = dict(density=1.0, mags=(1, 2, 3, 4, 5, 6, 7)) if cin == 64 else {}     # (576 taps on integers: larger factors, so that most sums need rounding)
    layers.update(c=dict(bias=64, **dense), r=dict(bias=64, **dense))
    name = f"conv{'.s2' if stride == 2 else ''}-{hw[0]}x{hw[1]}-{cin}-{cout}x{batch}"
    return Probe(name, net, int_params(net, 7, layers), int_images(3, batch, hw), ["c", "r"])


FAMILY_SHAPES = [((37, 21), 64, 64, 3), ((14, 14), 128, 128, 5), ((20, 20), 224, 224, 3), ((28, 28), 128, 256, 5), ((40, 24), 88, 224, 2)]
MOSAIC_SHAPES = [((7, 7), 128, 128, 9)]
STRIDE2_SHAPES = [((37, 45), 64, 96, 2), ((30, 18), 96, 64, 3)]


@functools.lru_cache(maxsize=None)
def get_family_probe(hw, cin, cout, batch, stride=1):
    return family_probe(hw, cin, cout, batch, stride)


@functools.lru_cache(maxsize=None)
def cached_reference(probe_key):
    """(ref, raw) of a probe built by PROBES[probe_key]: computed once, shared by every test that needs it, never written to"""
    p = PROBES[probe_key]()
    raw = {}
    ref = reference(p.net, p.P, p.images, raw)
    for a in list(ref.values()) + list(raw.values()):
        for b in (a if isinstance(a, tuple) else (a,)):
            b.setflags(write=False)
    return ref, raw


PROBES = {}


def _register(fn, *args):
    p = fn(*args)
    PROBES[p.name] = functools.partial(fn, *args)
    return p.name


FAMILY_KEYS = {sh: _register(get_family_probe, *sh) for sh in FAMILY_SHAPES + MOSAIC_SHAPES}
STRIDE2_KEYS = {sh: _register(get_family_probe, *sh, 2) for sh in STRIDE2_SHAPES}


# ---- fused ops ---------------------------------------------------------------------------------------------------------------------------
# An intermediate map that a fused op keeps on chip (Probe.onchip) must be the same number as fp16 and as fp32: the layers in front of it are
# sparse (few +-1 taps) and the images of these nets come from a narrower band, so that it stays inside fp16's 11 bits.  The last conv of the
# op is dense with factors up to 7: most of ITS sums need rounding.

DENSE = dict(density=1.0, mags=(1, 2, 3, 4, 5, 6, 7), bias=64)
FINE = dict(density=1.0, mags=tuple(range(1, 32)), exp=-2, bias=64)     # quarters up to 7.75: for a 1x1 conv on small integers
NARROW = (126, 130)                   # |2 p - 255| <= 3


def _narrow_images(seed, batch, hw):
    return np.random.default_rng(seed).integers(NARROW[0], NARROW[1], (batch,) + tuple(hw) + (3,), dtype=np.uint8)


def bb_probe(hw, planes, batch):
    """a residual BasicBlock (conv3x3 + ReLU, conv3x3, + block input, ReLU): csrc/conv_bb.hip keeps b.conv1 on chip"""
    net = _net(hw)
    net.add(Conv("s", "input", 3, planes, act="relu", **KW))
    net.add(Conv("b.conv1", "s", planes, planes, act="relu", **KW))
    net.add(Conv("b.conv2", "b.conv1", planes, planes, act="relu", res="s", **KW))
    net.outputs = ["s", "b.conv2"]
    layers = {"s": dict(density=1.0 / 3.0), "b.conv1": dict(density=8.0 / planes, mags=(1,)), "b.conv2": dict(density=1.0, mags=(1, 2, 3), bias=64)}
    return Probe(f"bb-{hw[0]}x{hw[1]}-{planes}x{batch}", net, int_params(net, 11, layers), int_images(5, batch, hw), ["b.conv2"], ["b.conv1"])


def mbf_probe(hw, cin, g, cout, stride, res, act3, batch):
    """MobileFaceNet's bottleneck (1x1 -> depthwise 3x3 -> 1x1 [+ block input]): csrc/mbf_block.hip keeps b.pw1 and b.dw on chip"""
    net = _net(hw)
    net.add(Conv("s", "input", 3, 64, act="relu", **KW))
    x = "s"
    if cin != 64:
        x = net.add(Conv("x", "s", 64, cin, k=1, pad=0, act="relu", **KW))
    net.add(Conv("b.pw1", x, cin, g, k=1, pad=0, act="relu", **KW))
    net.add(Conv("b.dw", "b.pw1", g, g, stride=stride, groups=g, act="relu", **KW))
    net.add(Conv("b.pw2", "b.dw", g, cout, k=1, pad=0, act=act3, res=x if res else None, **KW))
    net.outputs = [x, "b.pw2"]
    sparse = lambda c: dict(density=8.0 / c, mags=(1,))
    layers = {"s": dict(density=1.0 / 3.0), "x": sparse(64), "b.pw1": sparse(cin), "b.dw": dict(mags=(1,)), "b.pw2": FINE}
    return Probe(f"mbf-{hw[0]}x{hw[1]}-{cin}-{g}-{cout}s{stride}x{batch}", net, int_params(net, 13, layers), _narrow_images(6, batch, hw),
                 ["b.pw2"], ["b.pw1", "b.dw"], {})


def dwpw_probe(hw, g, cout, stride, act1, batch):
    """depthwise 3x3 + the pointwise 1x1 behind it: csrc/dwpw.hip (FID_DWPW_FUSE=1) keeps dw on chip"""
    net = _net(hw)
    net.add(Conv("s", "input", 3, 64, act="relu", **KW))
    net.add(Conv("p1", "s", 64, g, k=1, pad=0, act="relu", **KW))
    net.add(Conv("dw", "p1", g, g, stride=stride, groups=g, act=act1, **KW))
    net.add(Conv("pw", "dw", g, cout, k=1, pad=0, act="prelu", **KW))
    net.outputs = ["p1", "pw"]
    layers = {"s": dict(density=1.0 / 3.0), "p1": dict(density=1.0 / 8.0, mags=(1,)), "dw": dict(mags=(1, 2)), "pw": FINE}
    return Probe(f"dwpw-{hw[0]}x{hw[1]}-{g}-{cout}s{stride}x{batch}", net, int_params(net, 15, layers), _narrow_images(7, batch, hw),
                 ["pw"], ["dw"], {"FID_NO_MBF_FUSE": "1"})


def dual_probe(hw, planes, batch):
    """the block shortcut (2x2 average pool + 1x1 conv: the weights become quarters) beside the stride-2 conv on the same input: conv_s2.hip DUAL"""
    net = _net(hw)
    net.add(Conv("s", "input", 3, 64, act="relu", **KW))
    net.add(Conv("b.down", "s", 64, planes, k=1, stride=1, pad=0, pre_avgpool=True, **KW))
    net.add(Conv("b.conv1", "s", 64, planes, stride=2, act="relu", **KW))
    net.outputs = ["s", "b.down", "b.conv1"]
    return Probe(f"dual-{hw[0]}x{hw[1]}-{planes}x{batch}", net, int_params(net, 17, {"b.down": DENSE, "b.conv1": DENSE}), int_images(8, batch, hw),
                 ["b.down", "b.conv1"])


def stem_probe(hw, act, batch):
    """IResNet's stem + the 3x3 conv on it + the block's 1x1 / stride-2 shortcut: csrc/stem_block.hip keeps the stem's map on chip and stores
    its even pixels"""
    net = _net(hw)
    net.add(Conv("stem", "input", 3, 64, act=act, **KW))
    net.add(Conv("b.down", "stem", 64, 64, k=1, stride=2, pad=0, **KW))
    net.add(Conv("b.conv1", "stem", 64, 64, act=act, **KW))
    net.outputs = ["b.down", "b.conv1"]
    return Probe(f"stem-{hw[0]}x{hw[1]}-{act}x{batch}", net, int_params(net, 19, {"b.down": FINE, "b.conv1": DENSE}), int_images(9, batch, hw),
                 ["b.down", "b.conv1"], ["stem"])


def dw_probe(hw, batch):
    """a depthwise 3x3 layer of its own (net.hip: dwconv_nhwc; dwconv3x3_lds from 50 000 pixels per launch)"""
    net = _net(hw)
    net.add(Conv("s", "input", 3, 64, act="relu", **KW))
    net.add(Conv("p", "s", 64, 64, k=1, pad=0, act="prelu", **KW))
    net.add(Conv("d", "p", 64, 64, groups=64, act="prelu", **KW))
    net.outputs = ["p", "d"]
    return Probe(f"dw-{hw[0]}x{hw[1]}x{batch}", net, int_params(net, 21, {"p": dict(density=0.25, mags=(1,)), "d": DENSE}), int_images(10, batch, hw), ["d"])


def latfpn_probe(hw, batch):
    """two PAFPN levels and the coarsest one (lateral 1x1 [+ the upsampled coarser lateral] -> 3x3): csrc/lat_fpn.hip keeps the laterals on chip
    and stores the ones a finer level adds.  The laterals are compared as well, but only the 3x3 convs are held to the power conditions."""
    net = _net(hw)
    net.add(Conv("s", "input", 3, 32, act="relu", **KW))
    net.add(Conv("c3", "s", 32, 88, act="relu", **KW))
    net.add(Conv("c4", "c3", 88, 88, stride=2, act="relu", **KW))
    net.add(Conv("c5", "c4", 88, 88, stride=2, act="relu", **KW))
    net.add(Conv("lat2", "c5", 88, 56, k=1, pad=0, **KW))
    net.add(Conv("lat1", "c4", 88, 56, k=1, pad=0, res="lat2", res_up2=True, **KW))
    net.add(Conv("lat0", "c3", 88, 56, k=1, pad=0, res="lat1", res_up2=True, **KW))
    for i in range(3):
        net.add(Conv(f"fpn{i}", f"lat{i}", 56, 56, **KW))
    net.outputs = ["c3", "c4", "c5", "fpn0", "fpn1", "fpn2"]
    few = lambda taps: dict(density=4.0 / taps, mags=(1,))
    layers = {"s": dict(density=1.0 / 3.0), "c3": few(288), "c4": few(792), "c5": few(792), "lat0": few(88), "lat1": few(88), "lat2": few(88)}
    layers.update({f"fpn{i}": dict(density=1.0, mags=(1, 2, 3), bias=64) for i in range(3)})
    return Probe(f"latfpn-{hw[0]}x{hw[1]}x{batch}", net, int_params(net, 23, layers), _narrow_images(11, batch, hw),
                 ["fpn0", "fpn1", "fpn2"], ["lat0", "lat1", "lat2"])


def shortcut_probe(hw, cin, cout, batch):
    """a downsampling block whose 1x1 / stride-2 shortcut conv2 may absorb as extra K-steps (a generation-12 pick; conv_s2.hip NX = 2 with ns = 10):
    the absorbed form never rounds b.down, so b.down counts as kept on chip"""
    net, layers = _net(hw), {}
    x = _front(net, cin, layers)
    net.add(Conv("b.down", x, cin, cout, k=1, stride=2, pad=0, **KW))
    net.add(Conv("b.conv1", x, cin, cout, act="prelu", **KW))
    net.add(Conv("b.conv2", "b.conv1", cout, cout, stride=2, res="b.down", **KW))
    net.outputs = [x, "b.conv1", "b.conv2"]
    layers.update({"b.down": dict(density=8.0 / cin, mags=(1,)), "b.conv1": dict(density=8.0 / (9 * cin), mags=(1,))})
    return Probe(f"shortcut-{hw[0]}x{hw[1]}-{cin}-{cout}x{batch}", net, int_params(net, 25, layers), int_images(12, batch, hw), ["b.conv2"], ["b.down"])


def dethead_probe(hw, cin, batch):
    """the detector head conv (2 + 8 + 20 fp32 channels): the bbox and kps channels are exact sums; the sigmoid scores stay with the tolerance test"""
    from scrfd_arcface_facerecognition_amd.archs import DetHead
    net, layers = _net(hw), {}
    x = _front(net, cin, layers)
    net.add(DetHead("h", x, cin, 8))
    net.outputs = [x, "h"]
    return Probe(f"dethead-{hw[0]}x{hw[1]}-{cin}x{batch}", net, int_params(net, 27, layers), int_images(13, batch, hw), [])


BB_SHAPES = [((37, 45), 64, 2), ((12, 20), 64, 5), ((37, 45), 32, 2), ((12, 20), 24, 5)]
MBF_SHAPES = [((30, 22), 64, 96, 64, 1, True, "relu", 1), ((37, 21), 64, 128, 96, 2, False, "prelu", 2), ((14, 14), 256, 512, 256, 2, False, "none", 3)]
DWPW_SHAPES = [((37, 21), 64, 96, 1, "relu", 1), ((16, 24), 32, 48, 2, "none", 4)]
DUAL_SHAPES = [((74, 50), 96, 2)]
STEM_SHAPES = [((50, 44), "relu", 2), ((16, 16), "prelu", 1)]
DW_SHAPES = [((113, 75), 6), ((37, 21), 2)]            # 6 x 113 x 75 = 50 850 pixels: the LDS-tiled kernel, ragged tiles both ways

LATFPN_SHAPES = [((40, 56), 3), ((16, 16), 1)]
SHORTCUT_SHAPES = [((37, 45), 64, 96, 2), ((28, 28), 64, 128, 3)]

DETHEAD_SHAPES = [((24, 40), 80, 2), ((26, 26), 64, 3)]
BB_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(bb_probe), *sh) for sh in BB_SHAPES}
MBF_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(mbf_probe), *sh) for sh in MBF_SHAPES}
DWPW_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(dwpw_probe), *sh) for sh in DWPW_SHAPES}
DUAL_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(dual_probe), *sh) for sh in DUAL_SHAPES}
STEM_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(stem_probe), *sh) for sh in STEM_SHAPES}
DW_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(dw_probe), *sh) for sh in DW_SHAPES}
LATFPN_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(latfpn_probe), *sh) for sh in LATFPN_SHAPES}
SHORTCUT_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(shortcut_probe), *sh) for sh in SHORTCUT_SHAPES}
DETHEAD_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(dethead_probe), *sh) for sh in DETHEAD_SHAPES}


# ---- BatchNorm-folded forms --------------------------------------------------------------------------------------------------------------
# IResNet's layers: no conv bias, BatchNorm behind every conv and in front of a block's first one.  The conv behind a BN in front is zero-padded,
# so its bias is one of nine rows by the pixel's border class (lower.py: CF_BORDER); every kernel family decodes that class from its own tile
# coordinates.  Parameters: bn_params (see the module docstring for what makes the lowered constants the ideal ones).

BN = dict(bias=False, post_bn=True)
TINY_SHAPES = [((3, 5), 64, 64, 7)]      # 13 of 15 pixels are border pixels and every class occurs; seven images side by side on a STRIP tile


def _bn_probe(name, net, seed, layers, bn_layers, images, probed, onchip=()):
    P = int_params(net, seed, layers)
    P.update(bn_params(net, seed + 1, bn_layers))
    return Probe(name, net, P, images, list(probed), list(onchip))


def family_bn_probe(hw, cin, cout, batch):
    """both BatchNorm forms of a 3x3 conv on one input: c (BN - conv - BN - PReLU, cin -> cout) and r (BN - conv - BN, + the input, no activation)"""
    net, layers = _net(hw), {}
    x = _front(net, cin, layers)
    net.add(Conv("c", x, cin, cout, act="prelu", pre_bn=True, **BN))
    net.add(Conv("r", x, cin, cin, res=x, pre_bn=True, **BN))
    net.outputs = [x, "c", "r"]
    dense = dict(density=1.0, mags=(1, 2, 3, 4, 5, 6, 7)) if cin == 64 else {}
    layers.update(c=dict(dense), r=dict(dense))
    one = {"c.post_bn": dict(scales=(1.0,))} if cin > 128 else {}     # (2016 taps: one magnitude behind c keeps its partial sums inside GUARD)
    return _bn_probe(f"convbn-{hw[0]}x{hw[1]}-{cin}-{cout}x{batch}", net, 29, layers, one, int_images(14, batch, hw), ["c", "r"])


def ir_probe(hw, planes, batch):
    """IResNet's residual block (BN - conv - BN - PReLU - conv - BN, + block input): csrc/conv_bb.hip keeps b.conv1 on chip and picks its bias
    row by border class"""
    net = _net(hw)
    net.add(Conv("s", "input", 3, planes, act="relu", **KW))
    net.add(Conv("b.conv1", "s", planes, planes, act="prelu", pre_bn=True, **BN))
    net.add(Conv("b.conv2", "b.conv1", planes, planes, res="s", **BN))
    net.outputs = ["s", "b.conv2"]
    layers = {"s": dict(density=1.0 / 3.0), "b.conv1": dict(density=8.0 / planes, mags=(1,), slopes=(0.5,)),
              "b.conv2": dict(density=1.0, mags=(1, 2, 3))}
    return _bn_probe(f"ir-{hw[0]}x{hw[1]}-{planes}x{batch}", net, 31, layers, {}, int_images(15, batch, hw), ["b.conv2"], ["b.conv1"])


def shortcut_bn_probe(hw, cin, cout, batch):
    """the first block of an IResNet stage as it is: b.down (1x1 / stride 2 + BN), b.conv1 (BN - conv - BN - PReLU), b.conv2 (stride 2 + BN, + b.down).
    As in shortcut_probe the absorbed form never rounds b.down."""
    net, layers = _net(hw), {}
    x = _front(net, cin, layers)
    net.add(Conv("b.down", x, cin, cout, k=1, stride=2, pad=0, **BN))
    net.add(Conv("b.conv1", x, cin, cout, act="prelu", pre_bn=True, **BN))
    net.add(Conv("b.conv2", "b.conv1", cout, cout, stride=2, res="b.down", **BN))
    net.outputs = [x, "b.conv1", "b.conv2"]
    layers.update({"b.down": dict(density=8.0 / cin, mags=(1,)), "b.conv1": dict(density=8.0 / (9 * cin), mags=(1,))})
    return _bn_probe(f"shortcutbn-{hw[0]}x{hw[1]}-{cin}-{cout}x{batch}", net, 33, layers, {}, int_images(16, batch, hw), ["b.conv2"], ["b.down"])


def stem_bn_probe(hw, act, batch):
    """stem_probe with IResNet's BatchNorms: one in front of and one behind the 3x3 conv on the stem's map, one behind the shortcut"""
    net = _net(hw)
    net.add(Conv("stem", "input", 3, 64, act=act, **KW))
    net.add(Conv("b.down", "stem", 64, 64, k=1, stride=2, pad=0, **BN))
    net.add(Conv("b.conv1", "stem", 64, 64, act=act, pre_bn=True, **BN))
    net.outputs = ["b.down", "b.conv1"]
    return _bn_probe(f"stembn-{hw[0]}x{hw[1]}-{act}x{batch}", net, 35, {"b.down": FINE, "b.conv1": DENSE}, {}, int_images(17, batch, hw),
                     ["b.down", "b.conv1"], ["stem"])


FAMILY_BN_SHAPES = FAMILY_SHAPES + TINY_SHAPES
FAMILY_BN_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(family_bn_probe), *sh) for sh in FAMILY_BN_SHAPES + MOSAIC_SHAPES}
IR_SHAPES = [sh for sh in BB_SHAPES if sh[1] == 64]
IR_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(ir_probe), *sh) for sh in IR_SHAPES}
SHORTCUT_BN_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(shortcut_bn_probe), *sh) for sh in SHORTCUT_SHAPES}
STEM_BN_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(stem_bn_probe), *sh) for sh in STEM_SHAPES}
BN_KEYS = sorted(list(FAMILY_BN_KEYS.values()) + list(IR_KEYS.values()) + list(SHORTCUT_BN_KEYS.values()) + list(STEM_BN_KEYS.values()))


# ---- the split-K plan of the implicit GEMM, mirrored ---------------------------------------------------------------------------------------
# What a net that does not autotune (FID_AUTOTUNE=0) launches for a conv the direct kernel does not take: csrc/conv.hip conv_plan's generation-2
# branch, its FID_CONV_FORCE="bm,bn,ksplit" hook, and gemm_launch's recomputation of the split count from whole K-steps per slab.
# tests/test_exact_probe_cpu.py holds it against the library's own conv_plan on a grid of shapes; tests/test_gpu_ops_exact.py against what runs.

GEMM2_TILES = {64: ((128, 128), (128, 64), (64, 64)), 32: ((128, 128), (128, 96), (128, 64), (128, 32))}      # GEMM_TILES, generation 2, four ring slots


def _cdiv(a, b):
    return -(-a // b)


def split_mirror(M, cin_p, cout_p, taps, cus, force=None, allow_split=True):
    """dict(bm, bn, bk, ksteps, ksplit = the plan's split count, per = K-steps per slab, slabs = the K-steps of every launched slab).
    force: FID_CONV_FORCE as (bm, bn, ksplit)."""
    bk = 64 if cin_p % 64 == 0 else 32
    tiles = lambda bm, bn: _cdiv(M, bm) * _cdiv(cout_p, bn)
    bm = 128
    bn = 128 if cout_p % 128 == 0 else 96 if cout_p % 96 == 0 else 128 if cout_p > 64 else 64 if cout_p > 32 else 32
    if tiles(bm, bn) < cus and bn == 128:
        bn = 64
    if tiles(bm, bn) < cus and bn == 64 and bk == 64:
        bm = 64
    if bk == 64 and bn not in (128, 64):
        bn = 128 if cout_p > 64 else 64
    ksteps = _cdiv(taps * cin_p, bk)
    t, ks = tiles(bm, bn), 1
    if allow_split and t * 2 <= cus and ksteps >= 16:
        ks = max(1, min(_cdiv(cus, t), ksteps // 8))
    if force is not None:
        fbm, fbn, fks = force
        if (fbm, fbn) in GEMM2_TILES[bk]:
            bm, bn = fbm, fbn
        if fks >= 1 and allow_split:
            ks = max(1, min(fks, ksteps // 2))
    per = _cdiv(ksteps, ks)                                   # gemm_launch: whole K-steps per slab, then the slabs that are not empty
    n = _cdiv(ksteps, per)
    return dict(bm=bm, bn=bn, bk=bk, ksteps=ksteps, ksplit=ks, per=per, slabs=[min(per, ksteps - i * per) for i in range(n)])


def conv_geometry(low, name, batch):
    """(M, Cin_p, Cout_p, taps) of the OP_CONV record `name` of a lowered net, as csrc/net.hip run_op hands them to conv_plan"""
    r = low.ops[low.op_names.index(name)]
    src, dst = low.tensors[int(r[W_SRC])], low.tensors[int(r[W_DST])]
    return batch * int(dst[T_H]) * int(dst[T_W]), int(src[T_CP]), int(dst[T_CP]), int(r[W_KH]) * int(r[W_KW])


def takes_gdc_rows(low, name):
    """csrc/net.hip OP_DWCONV: the record `name` meets the condition under which gdc_rows runs instead of dwconv_nhwc"""
    r = low.ops[low.op_names.index(name)]
    src, dst = low.tensors[int(r[W_SRC])], low.tensors[int(r[W_DST])]
    return (int(r[W_TYPE]) == OP_DWCONV and int(r[W_KH]) == int(r[W_KW]) <= 8 and int(r[W_PAD]) == 0 and int(src[T_H]) == int(r[W_KH])
            and int(src[T_W]) == int(r[W_KW]) and int(dst[T_H]) == 1 and int(dst[T_W]) == 1)


# ---- split-K probes: the family nets under a forced split, and a 1x1 conv with an up-sampled residual ---------------------------------------

def up2_probe(hw, cin, cout, batch):
    """a 1x1 conv on `cin` channels that adds a map of half the size, up-sampled (CF_RES_UP2), PReLU: with cin = 1024 its K axis is 16 steps of
    64, which the heuristic plan already splits"""
    net = _net(hw)
    net.add(Conv("s", "input", 3, 64, act="relu", **KW))
    net.add(Conv("x", "s", 64, cin, k=1, pad=0, act="relu", **KW))
    net.add(Conv("d", "s", 64, cout, stride=2, **KW))
    net.add(Conv("u", "x", cin, cout, k=1, pad=0, act="prelu", res="d", res_up2=True, **KW))
    net.outputs = ["x", "d", "u"]
    layers = {"s": dict(density=1.0 / 3.0), "x": dict(density=8.0 / 64, mags=(1,)), "d": dict(density=4.0 / 576, mags=(1,)),
              "u": dict(density=1.0 / 8.0, mags=(1, 2, 3, 4, 5, 6, 7), bias=64)}
    return Probe(f"up2-{hw[0]}x{hw[1]}-{cin}-{cout}x{batch}", net, int_params(net, 37, layers), int_images(18, batch, hw), ["u"])


UP2_SHAPES = [((8, 8), 1024, 56, 3)]
UP2_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(up2_probe), *sh) for sh in UP2_SHAPES}

# (probe key, node names, FID_CONV_FORCE, the K-steps of every slab) -- the slabs follow from the forced split alone, whatever the device
SPLIT_CASES = [
    (FAMILY_KEYS[((14, 14), 128, 128, 5)], ("c", "r"), "128,64,2", [9, 9]),                     # 3x3 on 128 channels: 18 steps of 64
    (FAMILY_KEYS[((14, 14), 128, 128, 5)], ("c", "r"), "64,64,9", [2] * 9),                     # fewer steps than the ring's prologue
    (FAMILY_KEYS[((14, 14), 128, 128, 5)], ("c", "r"), "128,128,4", [5, 5, 5, 3]),              # a ragged last slab
    (FAMILY_KEYS[((14, 14), 128, 128, 5)], ("c", "r"), "128,64,7", [3] * 6),                    # a request the launcher reduces: 7 -> 6 slabs
    (FAMILY_KEYS[((40, 24), 88, 224, 2)], ("c",), "128,64,7", [4] * 6 + [3]),                   # 96 stored channels: 27 steps of 32, three per tap; slabs begin inside a tap
    (FAMILY_KEYS[((40, 24), 88, 224, 2)], ("c", "r"), "128,128,2", [14, 13]),
    (FAMILY_BN_KEYS[((3, 5), 64, 64, 7)], ("c", "r"), "64,64,4", [3, 3, 3]),                    # border-class bias rows behind the slab sum
    (FAMILY_BN_KEYS[((3, 5), 64, 64, 7)], ("c", "r"), "128,64,2", [5, 4]),
    (UP2_KEYS[UP2_SHAPES[0]], ("u",), None, None),                                              # the heuristic's own split (by the device's CU count)
    (UP2_KEYS[UP2_SHAPES[0]], ("u",), "64,64,5", [4, 4, 4, 4]),                                 # up-sampled residual behind the slab sum
]


# ---- FC ----------------------------------------------------------------------------------------------------------------------------------------

def fc_probe(c, hw_map, cout, batch):
    """IResNet's last op on a small map: stem, [1x1 to c channels], two 3x3 / stride-2 convs down to the map, BN - FC - BN with a bias"""
    from scrfd_arcface_facerecognition_amd.archs import FC
    h, w = hw_map
    net = _net((4 * h, 4 * w))
    net.add(Conv("s", "input", 3, 64, act="relu", **KW))
    x = "s"
    if c != 64:
        x = net.add(Conv("x", "s", 64, c, k=1, pad=0, act="relu", **KW))
    net.add(Conv("a", x, c, c, stride=2, act="relu", **KW))
    net.add(Conv("b", "a", c, c, stride=2, **KW))
    net.add(FC("fc", "b", c, h, w, cout))
    net.outputs = ["b", "fc"]
    few = lambda taps: dict(density=4.0 / taps, mags=(1,))
    layers = {"s": dict(density=1.0 / 3.0), "x": few(64), "a": few(9 * c), "b": few(9 * c), "fc": dict(density=1.0 / 4.0, mags=(1, 2), bias=64)}
    P = int_params(net, 41, layers)
    P.update(bn_params(net, 42))
    return Probe(f"fc-{c}x{h}x{w}-{cout}x{batch}", net, P, _narrow_images(19, batch, net.in_hw), ["fc"])


FC_SHAPES = [(64, (5, 5), 512, 1), (64, (5, 5), 512, 3), (64, (5, 5), 512, 130), (128, (7, 7), 512, 2), (88, (5, 5), 128, 3)]
FC_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(fc_probe), *sh) for sh in FC_SHAPES}


# ---- the fused detector stem -----------------------------------------------------------------------------------------------------------------
# conv / stride 2 - conv - conv - max pool 3 / 2 / 1, all ReLU.  Every form of it (csrc/stem_rows.hip with 8 or 6 pooled rows and with wave roles,
# csrc/stem_fused.hip) keeps stem.0 and stem.1 in LDS as fp16, rounded from the fp32 accumulator exactly as the unfused convs store them
# (__builtin_convertvector to half, ReLU after the rounding: the same bits), and rounds stem.2 once: the row kernels pool the fp32 accumulators and
# round the maximum, the flat kernel rounds and then pools -- rounding is monotone, so both are max(round(.)).  The reference therefore rounds
# all three maps and nothing is listed as kept on chip; stem.2 is held to the power conditions and seen through the pool.

def stemfused_probe(hw, c0, c2, batch):
    from scrfd_arcface_facerecognition_amd.archs import MaxPool
    net = _net(hw)
    net.add(Conv("stem.0", "input", 3, c0, stride=2, act="relu", **KW))
    net.add(Conv("stem.1", "stem.0", c0, c0, act="relu", **KW))
    net.add(Conv("stem.2", "stem.1", c0, c2, act="relu", **KW))
    net.add(MaxPool("stem.pool", "stem.2", c2))
    net.outputs = ["stem.pool"]
    layers = {"stem.1": dict(density=1.0 / 3.0, mags=(1, 2), exp=-4, bias=64), "stem.2": dict(DENSE)}
    return Probe(f"stemfused-{hw[0]}x{hw[1]}-{c0}-{c2}x{batch}", net, int_params(net, 43, layers), int_images(20, batch, hw), ["stem.pool"],
                 through=["stem.2"])


STEMFUSED_SHAPES = [((72, 100), 12, 24, 2), ((64, 64), 28, 56, 3), ((100, 76), 24, 24, 3)]
STEMFUSED_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(stemfused_probe), *sh) for sh in STEMFUSED_SHAPES}


# ---- the first conv of a net on its own ---------------------------------------------------------------------------------------------------------
# 27 taps: the whole pixel range (|2 p - 255| <= 255) and factors up to 7 make most sums need rounding; at most 27 * 255 * 7 + 64 < 65504.

def first_probe(hw, cout, stride, batch):
    net = _net(hw)
    net.add(Conv("s", "input", 3, cout, stride=stride, act="prelu" if stride == 2 else "relu", **KW))
    net.outputs = ["s"]
    P = int_params(net, 45, {"s": dict(mags=(1, 2, 3, 4, 5, 6, 7), bias=64)})
    return Probe(f"first-{hw[0]}x{hw[1]}-{cout}s{stride}x{batch}", net, P, int_images(21, batch, hw, (0, 256)), ["s"])


FIRST_SHAPES = [(hw, cout, st, 2) for hw in ((36, 52), (36, 50)) for cout in (12, 28, 64, 128) for st in (1, 2)]
FIRST_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(first_probe), *sh) for sh in FIRST_SHAPES}


# ---- max pool and the global depthwise conv ------------------------------------------------------------------------------------------------------

def pool_probe(hw, c, batch):
    """max pool 3 / 2 / 1 behind a PReLU conv: negative values, so a tap outside the map that counted as 0 would win at the border"""
    from scrfd_arcface_facerecognition_amd.archs import MaxPool
    net = _net(hw)
    net.add(Conv("s", "input", 3, c, act="prelu", **KW))
    net.add(MaxPool("pool", "s", c))
    net.outputs = ["s", "pool"]
    return Probe(f"pool-{hw[0]}x{hw[1]}-{c}x{batch}", net, int_params(net, 47, {"s": dict(bias=64)}), int_images(22, batch, hw), ["pool"])


def gdc_probe(k, c, batch, act):
    """MobileFaceNet's global depthwise conv: k x k, no padding, on a k x k map (csrc/net.hip gdc_rows: lane r of eight sums kernel row r)"""
    net = _net((k, k))
    net.add(Conv("s", "input", 3, 64, act="relu", **KW))
    x = "s"
    if c != 64:
        x = net.add(Conv("x", "s", 64, c, k=1, pad=0, act="relu", **KW))
    net.add(Conv("g", x, c, c, k=k, pad=0, groups=c, act=act, **KW))
    net.outputs = [x, "g"]
    layers = {"s": dict(density=1.0 / 3.0 if c != 64 else 1.0), "x": dict(density=8.0 / 64, mags=(1,)), "g": dict(FINE)}       # (k k taps on integers: quarters, so that most sums need rounding)
    return Probe(f"gdc-{k}x{k}-{c}-{act}x{batch}", net, int_params(net, 49, layers), int_images(23, batch, (k, k)), ["g"])


POOL_SHAPES = [((37, 21), 56, 3), ((16, 16), 56, 3), ((37, 21), 24, 3), ((16, 16), 24, 3)]
GDC_SHAPES = [(7, 512, 1, "prelu"), (7, 512, 3, "none"), (7, 512, 5, "prelu"), (7, 128, 1, "none"), (5, 64, 3, "prelu")]
POOL_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(pool_probe), *sh) for sh in POOL_SHAPES}
GDC_KEYS = {sh: _register(functools.lru_cache(maxsize=None)(gdc_probe), *sh) for sh in GDC_SHAPES}
OPS_KEYS = sorted(list(UP2_KEYS.values()) + list(FC_KEYS.values()) + list(STEMFUSED_KEYS.values()) + list(FIRST_KEYS.values())
                  + list(POOL_KEYS.values()) + list(GDC_KEYS.values()))
