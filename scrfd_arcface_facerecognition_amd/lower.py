"""Lowering: archs.Net + raw fp32 parameters  ->  the layer table libfaceid executes.

This is the work onnxruntime's graph optimiser does invisibly inside InferenceSession (reference
models/scrfd.py:59-62, models/arcface.py:18-21), written down:

  * BatchNorm after a conv is folded into the conv's weights and bias;
  * BatchNorm BEFORE a zero-padded conv (IResNet's bn1) is folded exactly: scale into the weights,
    shift into a 9-entry border-class bias table (a border pixel's missing taps contribute no shift);
  * AvgPool(2)+Conv1x1 ("avg_down" shortcut) becomes one 2x2/stride-2 conv with weights/4;
  * nearest-2x upsample + add (PAFPN top-down) and the residual add become epilogue flags;
  * a residual BasicBlock on 64 (padded) channels -- conv3x3+ReLU, conv3x3, + block input, activation -- becomes ONE op whose
    intermediate map never leaves the CU (csrc/conv_bb.hip; FID_NO_BB_FUSE=1 keeps the two convs);
  * a depthwise 3x3 conv whose only consumer is a pointwise 1x1 conv (MobileFaceNet bottlenecks, SCRFD-500M) becomes ONE op with the
    depthwise result in LDS (csrc/dwpw.hip) when FID_DWPW_FUSE=1 asks for it (measured slower than the two launches: off by default);
  * the three SCRFD output convs of a level become one conv with 2+8+20 output channels, sigmoid on
    the first two, bbox scale folded in, fp32 output;
  * blobFromImage's (x-127.5)*scale and BGR->RGB swap are folded into the first conv's weights;
  * a PAFPN level's 1x1 lateral conv (+ the upsampled coarser lateral) and the 3x3 conv on it become ONE op (csrc/lat_fpn.hip): the lateral is
    stored only when a finer level adds it (FID_NO_LATFPN_FUSE=1 keeps the two convs apart);
  * IResNet's first conv (3 -> 64, stride 1) and the 3x3 conv on 64 channels that consumes it become ONE op (csrc/stem_block.hip): the first
    conv's map only exists in LDS; the block's 1x1 / stride-2 shortcut reads a compact copy of it at the even pixels (FID_NO_STEMBLOCK_FUSE=1
    keeps the two convs apart);
  * FC consumes the NHWC activation directly (weight columns permuted from CHW order).

Weights are packed fp16 [Cout_p][tap][Cin_p] (channels padded to multiples of 32 with zeros), all
epilogue tables fp32.  Activation buffers are assigned to slots by liveness.
Word layout of the op / tensor records: csrc/net.h, mirrored name by name in net_layout.py (OP_*, W_*, T_*, CF_*, ACT); every record here is
written by _Builder.emit / new_tensor and read through those names.

lower() walks the graph once and tries the fused patterns in a fixed priority order; each pattern is a predicate (_stem_fused, _stem_block,
_dual_ok, _bblock, _mbf_block, _latfpn, _dwpw) and an emitter (_emit_*) that writes its tables into the blob and one record into the table.
"""
from __future__ import annotations

import copy
import dataclasses
import os
from typing import Dict, List, Tuple

import numpy as np

from . import net_layout
from .archs import BN_EPS, Net, infer_shapes
from .net_layout import *  # noqa: F401,F403  (OP_*, W_*, T_*, CF_*, ACT, OP_WORDS, TENSOR_WORDS, record_tensors: re-exported)

CPAD = 32
_WORD = {k[2:].lower(): v for k, v in vars(net_layout).items() if k.startswith("W_")}     # emit()'s keywords: woff=... writes rec[W_WOFF]


def _rup(x, m):
    return (x + m - 1) // m * m


def _bn_affine(P, prefix):
    a = P[prefix + ".gamma"].astype(np.float64) / np.sqrt(P[prefix + ".var"].astype(np.float64) + BN_EPS)
    b = P[prefix + ".beta"].astype(np.float64) - P[prefix + ".mean"].astype(np.float64) * a
    return a, b


class _Blob:
    def __init__(self):
        self.parts: List[bytes] = []
        self.size = 0

    def add(self, arr: np.ndarray) -> Tuple[int, int]:
        raw = np.ascontiguousarray(arr).tobytes()
        off = self.size
        pad = (-len(raw)) % 256
        self.parts.append(raw + b"\0" * pad)
        self.size += len(raw) + pad
        return off, len(raw)

    def bytes(self) -> bytes:
        return b"".join(self.parts)


class Lowered:
    """Result of lower(): numpy tables + name maps."""

    def __init__(self):
        self.ops: np.ndarray = None          # int32 [n_ops, 32]
        self.tensors: np.ndarray = None      # int32 [n_tensors, 8]
        self.blob: bytes = b""
        self.tensor_id: Dict[str, int] = {}
        self.op_names: List[str] = []
        self.op_nodes: List[List[str]] = []
        self.outputs: List[str] = []
        self.in_hw = (0, 0)
        self.macs = 0
        self.heads: Dict[str, dict] = {}     # DetHead name -> channel layout of the fused tensor
        self.fused_groups: Dict[str, list] = {}   # fused op name -> graph nodes it covers


def _pack_weights(W4, cin_p, cout_p):
    """[cout, cin, kh, kw] float64 -> fp16 [cout_p][kh*kw][cin_p]"""
    cout, cin, kh, kw = W4.shape
    Wp = np.zeros((cout_p, kh * kw, cin_p), dtype=np.float32)
    Wp[:cout, :, :cin] = W4.transpose(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    h = Wp.astype(np.float16)
    if not np.isfinite(h).all():
        raise ValueError("weights overflow fp16")
    return h


def _repack_kind2(Wp):
    """fp16 [cout_p <= 128][9][cin_p] -> csrc/repack.hip kind 2 (conv3x3_wr's MFMA A fragments in lane order):
    [32-channel chunk][cout fragment 0..7][dx][dy][lane][8 halfs], lane = (channel group of 8) * 16 + (cout & 15)"""
    cout_p, taps, cin_p = Wp.shape
    assert taps == 9 and cout_p <= 128 and cin_p % 32 == 0
    full = np.zeros((128, 9, cin_p), dtype=np.float16)
    full[:cout_p] = Wp
    x = full.reshape(8, 16, 3, 3, cin_p // 32, 4, 8)          # [cf][cout & 15][dy][dx][ck][group][e]
    return np.ascontiguousarray(x.transpose(4, 0, 3, 2, 5, 1, 6))   # [ck][cf][dx][dy][group][cout & 15][e]


def _padded(vec, n, fill=0.0):
    o = np.full(n, fill, dtype=np.float32)
    o[: len(vec)] = vec
    return o


def _avg_down(W):
    """the 2x2 average pool in front of a 1x1 conv, folded: a 2x2 / stride-2 kernel with W / 4"""
    return np.repeat(np.repeat(W, 2, axis=2), 2, axis=3) / 4.0


class _Builder:
    """What the emitters share: the graph and its parameters, and the blob, tensor records and op records being written."""

    def __init__(self, net: Net, P: Dict[str, np.ndarray]):
        self.net, self.P = net, P
        self.shp = infer_shapes(net)
        self.blob = _Blob()
        self.ops, self.tensors, self.tid = [], [], {}      # op records, tensor records, tensor name -> id
        self.op_names, self.op_nodes = [], []              # per op: its name, the graph nodes it covers (several for fused ops)
        self.fused_groups, self.heads = {}, {}
        self.skip = set()                          # node indices an earlier fused op has covered
        self.pending_sc = {}                       # conv2 name -> (its block's shortcut conv node, that op's index): fused as extra K-steps

    def new_tensor(self, name, C, H, W, dtype=0, Cp=None):
        rec = [0] * TENSOR_WORDS
        rec[T_C], rec[T_CP], rec[T_H], rec[T_W], rec[T_DTYPE], rec[T_SLOT] = C, _rup(C, CPAD) if Cp is None else Cp, H, W, dtype, -1
        self.tid[name] = len(self.tensors)
        self.tensors.append(rec)
        return self.tid[name]

    def src(self, n):
        """the tensor record a node reads"""
        return self.tensors[self.tid[n.src]]

    def res(self, n):
        return self.tid[n.res] if n.res else -1

    def emit(self, name, nodes=None, macs=None, **words):
        """append one op record: `words` by their csrc/net.h names without the W_ (type=, src=, woff=, b_w1=, x_src2= ...), `macs` = the algorithmic
        MACs per image of a fused group, `nodes` = the graph nodes a fused op covers"""
        rec = [0] * OP_WORDS
        rec[W_RES] = rec[W_WOFF] = rec[W_BOFF] = rec[W_SOFF] = -1
        rec[W_GROUPS] = 1
        for k, v in words.items():
            rec[_WORD[k]] = int(v)
        if macs is not None:                       # a 64-bit count in two int32 words
            lo = macs & 0xFFFFFFFF
            rec[W_F_MACS_LO], rec[W_F_MACS_HI] = lo - 2 ** 32 if lo >= 2 ** 31 else lo, macs >> 32
        self.ops.append(rec)
        self.op_names.append(name)
        self.op_nodes.append(list(nodes) if nodes else [name])
        if nodes:
            self.fused_groups[name] = list(nodes)

    def put(self, arr):
        """blob offset of a table"""
        return self.blob.add(arr)[0]

    def slopes(self, n, width):
        """blob offset of a node's PReLU slopes, or -1"""
        return self.put(_padded(self.P[n.wname + ".prelu"], width)) if n.act == "prelu" else -1

    def folded(self, n, W=None):
        """conv weights/bias with the trailing BatchNorm folded in (float64)"""
        W = self.P[n.wname + ".weight"].astype(np.float64) if W is None else W
        b = self.P[n.wname + ".bias"].astype(np.float64) if n.bias else np.zeros(n.cout)
        if n.post_bn:
            a2, b2 = _bn_affine(self.P, n.wname + ".post_bn")
            W = W * a2.reshape((-1,) + (1,) * (W.ndim - 1))
            b = b * a2 + b2
        return W, b

    def fold_conv(self, n, src_hw):
        """full fold of a conv node: (W [cout, cin, k, k] f64, bias table [ncls, cout] f64, k, stride) with a BatchNorm in FRONT of a zero-padded
        conv folded exactly (scale into the weights, shift into 9 border-class bias rows: a border pixel's missing taps contribute no shift), the
        avg-pool of an "avg_down" shortcut as a 2x2 / stride-2 kernel and the trailing BatchNorm"""
        P = self.P
        W = P[n.wname + ".weight"].astype(np.float64)            # [cout, cin, k, k]
        b = P[n.wname + ".bias"].astype(np.float64) if n.bias else np.zeros(n.cout)
        k, stride, pad = n.k, n.stride, n.pad
        if n.pre_avgpool:
            assert k == 1 and pad == 0 and stride == 1
            W = _avg_down(W)
            k, stride = 2, 2
        bias_tab = None
        if n.pre_bn:
            a1, b1 = _bn_affine(P, n.wname + ".pre_bn")
            shift = np.einsum("oikl,i->okl", W, b1)                # per-tap contribution of the BN shift
            W = W * a1[None, :, None, None]
            if pad == 0:
                b = b + shift.sum(axis=(1, 2))
            else:
                assert k == 3 and pad == 1 and stride == 1 and src_hw[0] >= 2 and src_hw[1] >= 2, n.name
                bias_tab = np.zeros((9, n.cout))
                for yc in range(3):
                    for xc in range(3):
                        m = np.ones((3, 3))
                        if yc != 1: m[yc, :] = 0                   # (the taps outside the image)
                        if xc != 1: m[:, xc] = 0
                        bias_tab[yc * 3 + xc] = b + (shift * m[None]).sum(axis=(1, 2))
        if bias_tab is None:
            bias_tab = b[None, :]
        if n.post_bn:
            a2, b2 = _bn_affine(P, n.wname + ".post_bn")
            W = W * a2[:, None, None, None]
            bias_tab = bias_tab * a2[None, :] + b2[None, :]
        return W, bias_tab, k, stride


def _users(net, name, but=None):
    """the nodes that read tensor `name` as input or residual (other than node `but`)"""
    return [x for x in net.nodes if x is not but and (getattr(x, "src", None) == name or getattr(x, "res", None) == name)]


# ---- which pattern applies at a node ------------------------------------------------------------------------------------------------------

def _stem_fused(net):
    """nodes 0..3 = SCRFD's deep stem: conv / stride 2 - conv - conv (3x3, ReLU, at most 32 / 32 / 64 couts) - maxpool 3x3 / stride 2 on an input
    whose sides are multiples of 4, the three conv maps read by nothing else (csrc/stem_fused.hip)"""
    nd = net.nodes
    inner = [x.name for x in nd[:3]]
    return (len(nd) >= 4 and nd[0].kind == "conv" and nd[0].src == "input"
            and all(x.kind == "conv" and x.k == 3 and x.pad == 1 and x.groups == 1 and x.act == "relu" and not x.pre_bn
                    and x.res is None and not x.pre_avgpool for x in nd[0:3])
            and nd[0].stride == 2 and nd[1].stride == 1 and nd[2].stride == 1 and nd[1].src == nd[0].name
            and nd[2].src == nd[1].name and nd[3].kind == "maxpool" and nd[3].src == nd[2].name
            and (nd[3].k, nd[3].stride, nd[3].pad) == (3, 2, 1) and nd[0].cout <= 32 and nd[1].cout <= 32
            and nd[2].cout <= 64 and net.in_hw[0] % 4 == 0 and net.in_hw[1] % 4 == 0
            and not any(getattr(x, "src", None) in inner or getattr(x, "res", None) in inner for x in nd[4:])
            and not any(o in inner for o in net.outputs))


def _stem_block(net):
    """node 0 = IResNet's first conv (3 -> 64, 3x3 / stride 1, ReLU / PReLU) whose consumers are ONE 3x3 / stride-1 conv on 64 channels and at most
    one 1x1 / stride-2 shortcut conv (csrc/stem_block.hip): (index of the 3x3 conv, that node, [(index, shortcut node)] or []) or None"""
    nd = net.nodes
    if len(nd) < 2:
        return None
    st = nd[0]
    users = [(i, x) for i, x in enumerate(nd) if getattr(x, "src", None) == st.name or getattr(x, "res", None) == st.name]
    c1s = [(i, x) for i, x in users if x.kind == "conv" and x.src == st.name and x.k == 3 and x.stride == 1 and x.pad == 1 and x.groups == 1
           and x.cin == 64 and x.cout == 64 and x.res is None and x.act in ("relu", "prelu") and not x.pre_avgpool and not x.res_up2]
    others = [(i, x) for i, x in users if not c1s or x is not c1s[0][1]]
    sc_ok = all(x.kind == "conv" and x.src == st.name and x.res != st.name and x.k == 1 and x.stride == 2 and x.pad == 0 and x.groups == 1
                and not x.pre_bn and not x.pre_avgpool for _, x in others)
    H0, W0 = net.in_hw
    if not (st.kind == "conv" and st.src == "input" and st.k == 3 and st.stride == 1 and st.pad == 1 and st.groups == 1 and st.cout == 64
            and st.act in ("relu", "prelu") and st.res is None and not st.pre_bn and len(c1s) == 1 and sc_ok and len(others) <= 1
            and st.name not in net.outputs and W0 % 4 == 0 and H0 >= 3 and abs(net.in_mean - 127.5) < 1e-12):
        return None
    return c1s[0][0], c1s[0][1], others


def _dual_ok(net, i, tensors, tid, shp):
    """nodes i, i+1 = an "avg_down" shortcut conv and the block's 3x3 / stride-2 conv1 on the same input, in the shapes csrc/conv_s2.hip's DUAL
    variant takes (64 stored input channels, 96 padded couts each): lowered as ONE op with two outputs"""
    n = net.nodes[i]
    nxt = net.nodes[i + 1] if i + 1 < len(net.nodes) else None
    return (n.kind == "conv" and n.groups == 1 and n.pre_avgpool and not os.environ.get("FID_NO_DOWN_FUSE")
            and nxt is not None and nxt.kind == "conv" and nxt.groups == 1 and nxt.src == n.src and nxt.k == 3 and nxt.stride == 2
            and nxt.pad == 1 and nxt.res is None and not nxt.pre_bn and not n.pre_bn and not nxt.pre_avgpool
            and nxt.act in ("none", "relu") and n.act == "none" and n.res is None and not n.res_up2 and not nxt.res_up2
            and tensors[tid[n.src]][T_CP] == 64 and _rup(n.cout, CPAD) == 96 and _rup(nxt.cout, CPAD) == 96
            and shp[n.name][1:] == shp[nxt.name][1:])


def _shortcut_target(net, i, tensors, tid, shp):
    """node i = a residual block's shortcut conv whose only consumer is the residual add of a later 3x3 conv of the same output shape that the
    implicit-GEMM kernel can extend by K-steps on the block input: that conv node, or None.  Two forms:
      * IResNet: 1x1 / stride s + BN feeding the block's stride-s conv2 (one extra tap at (s oy, s ox));
      * ResNetV1e "avg_down" (SCRFD): 2x2 average pool + 1x1 + BN = a 2x2 / stride-2 conv feeding the block's stride-1 conv2 (four extra taps at
        (2 oy + {0,1}, 2 ox + {0,1})) -- unless csrc/conv_s2.hip's DUAL launch already computes it beside conv1 (_dual_ok)."""
    n = net.nodes[i]
    if not (n.k == 1 and n.pad == 0 and n.act == "none" and n.res is None and not n.pre_bn and not n.res_up2 and n.src != "input"
            and n.name not in net.outputs and n.groups == 1):
        return None
    avg = bool(n.pre_avgpool)
    if (avg and n.stride != 1) or (not avg and n.stride not in (1, 2)) or (avg and _dual_ok(net, i, tensors, tid, shp)):
        return None
    s_eff, taps = (2, 2) if avg else (n.stride, 1)
    users = _users(net, n.name)
    if len(users) != 1:
        return None
    m = users[0]
    if not (m.kind == "conv" and m.res == n.name and m.src != n.name and m.groups == 1 and m.k == 3 and m.pad == 1 and not m.pre_bn
            and m.stride == (1 if avg else 2) and not m.pre_avgpool and not m.res_up2 and net.nodes.index(m) > i and shp[m.name] == shp[n.name]):
        return None
    x_t = tensors[tid[n.src]]
    # (when conv2's input is lowered after the shortcut, its padded width is its own cout rounded up)
    cin_p = tensors[tid[m.src]][T_CP] if m.src in tid else _rup(next(x for x in net.nodes if x.name == m.src).cout, CPAD)
    # every sampled pixel (oy * s + dy, ox * s + dx) must exist, the channel counts must suit a 32- or 64-wide K-step of the LDS-DMA implicit GEMM
    _, ho, wo = shp[m.name]
    if (x_t[T_DTYPE] != 0 or x_t[T_CP] % 32 or cin_p % 32 or (ho - 1) * s_eff + taps - 1 >= x_t[T_H]
            or (wo - 1) * s_eff + taps - 1 >= x_t[T_W]):
        return None
    if not avg and n.stride != m.stride and not getattr(n, "_even_src", False):   # (_even_src: the shortcut reads the fused stem block's even-pixel copy of x with stride 1)
        return None
    return m


def _bblock(net, i, tensors, tid):
    """nodes i, i+1 = a residual BasicBlock, conv 3x3 + ReLU / PReLU -> conv 3x3 -> + block input -> ReLU / none, on 64 stored channels (or 32
    with a plain ReLU conv1), conv1's map read by nothing else, in the shapes csrc/conv_bb.hip takes"""
    n = net.nodes[i]
    m = net.nodes[i + 1] if i + 1 < len(net.nodes) else None
    if not (n.kind == "conv" and n.groups == 1 and m is not None and m.kind == "conv" and m.groups == 1 and n.k == 3 and m.k == 3
            and n.stride == 1 and m.stride == 1 and n.pad == 1 and m.pad == 1 and n.act in ("relu", "prelu") and m.act in ("relu", "none")
            and n.res is None and m.res == n.src and m.src == n.name and not n.res_up2 and not m.res_up2 and not m.pre_bn
            and not n.pre_avgpool and not m.pre_avgpool and n.src != "input"):
        return False
    src_t = tensors[tid[n.src]]
    cp = src_t[T_CP]
    return (cp in (32, 64) and src_t[T_DTYPE] == 0 and _rup(n.cout, CPAD) == cp and _rup(m.cout, CPAD) == cp
            and (cp == 64 or (n.act == "relu" and not n.pre_bn)) and n.name not in net.outputs and src_t[T_H] >= 3 and src_t[T_W] >= 3
            and not _users(net, n.name, but=m))


def _mbf_block(net, i, tensors, tid, shp):
    """nodes i, i+1, i+2 = pointwise 1x1 -> depthwise 3x3 -> pointwise 1x1 [+ the first one's input] in the shapes csrc/mbf_block.hip takes
    (mbf_block_applicable): (depthwise node, second pointwise node) or None"""
    if i + 2 >= len(net.nodes):
        return None
    n, d, m = net.nodes[i], net.nodes[i + 1], net.nodes[i + 2]
    if not (d.kind == "conv" and m.kind == "conv" and n.k == 1 and n.pad == 0 and n.stride == 1 and n.src != "input" and n.res is None
            and not n.pre_bn and not n.pre_avgpool and not n.res_up2
            and d.groups == d.cin == d.cout == n.cout and d.groups > 1 and d.k == 3 and d.pad == 1 and d.stride in (1, 2) and d.src == n.name
            and d.res is None and not d.pre_bn and not d.pre_avgpool
            and m.groups == 1 and m.k == 1 and m.pad == 0 and m.stride == 1 and m.src == d.name and m.res in (None, n.src)
            and not m.pre_bn and not m.pre_avgpool and not m.res_up2):
        return None
    if n.name in net.outputs or d.name in net.outputs or _users(net, n.name, but=d) or _users(net, d.name, but=m):   # the two expanded maps feed nothing else
        return None
    src_t = tensors[tid[n.src]]
    cin_p, gp, cout_p = src_t[T_CP], _rup(n.cout, CPAD), _rup(m.cout, CPAD)
    if (src_t[T_DTYPE] != 0 or cin_p % 32 or cin_p > 256 or gp % 32 or gp > 512 or cout_p % 16 or cout_p > 256
            or (m.res is not None and (d.stride != 1 or cin_p != cout_p))):
        return None
    to = 7 if d.stride == 1 else 4                        # LDS: the 9 x 9 region + both expanded maps (csrc/mbf_block.hip mbf_lds_bytes; the kernel
    rup = lambda v: (v + 1023) // 1024 * 1024            #  takes 7 x 7 tiles at stride 2 as well when their 15 x 15 region fits)
    if rup(81 * (cin_p * 2 + 16)) + rup(81 * (gp * 2 + 16)) + ((to * to + 15) // 16 * 16) * (gp * 2 + 16) > 160 * 1024:
        return None
    return d, m


def _latfpn(net, i, tensors, tid):
    """node i = a 1x1 lateral conv (bias / BN, no activation, optionally + the nearest-2x upsampled coarser lateral) on 64 / 96 stored channels whose
    consumers are ONE 3x3 / stride-1 conv without activation or residual (64 stored couts each) and otherwise only finer laterals that add it
    (res_up2): (index of the 3x3 conv, that node, lateral stored?) or None (csrc/lat_fpn.hip)"""
    n = net.nodes[i]
    if os.environ.get("FID_NO_LATFPN_FUSE") or not (n.kind == "conv" and n.k == 1 and n.pad == 0 and n.stride == 1 and n.groups == 1 and n.act == "none"
                                                    and not n.pre_bn and not n.pre_avgpool and n.src != "input" and n.name not in net.outputs
                                                    and (n.res is None or n.res_up2) and _rup(n.cout, CPAD) == 64):
        return None
    src_t = tensors[tid[n.src]]
    if src_t[T_DTYPE] != 0 or src_t[T_CP] not in (64, 96) or src_t[T_H] < 3 or src_t[T_W] < 3:
        return None
    if n.res is not None:
        r_t = tensors[tid[n.res]]
        if r_t[T_DTYPE] != 0 or r_t[T_CP] != 64 or src_t[T_H] != 2 * r_t[T_H] or src_t[T_W] != 2 * r_t[T_W]:      # exact 2x levels only (see the CF_RES_UP2 note below)
            return None
    convs, adders = [], 0
    for j, x in enumerate(net.nodes):
        if getattr(x, "src", None) == n.name:
            convs.append((j, x))
        if getattr(x, "res", None) == n.name:
            if not (x.kind == "conv" and x.res_up2 and x.src != n.name):
                return None
            adders += 1
    if len(convs) != 1:
        return None
    j, m = convs[0]
    if not (j > i and m.kind == "conv" and m.k == 3 and m.stride == 1 and m.pad == 1 and m.groups == 1 and m.act == "none" and m.res is None and not m.pre_bn
            and not m.pre_avgpool and m.cin == n.cout and _rup(m.cout, CPAD) == 64):
        return None
    return j, m, adders > 0


def _dwpw(net, i, cp):
    """nodes i, i+1 = a depthwise 3x3 conv on cp stored channels and the pointwise 1x1 conv that alone consumes it, in the shapes csrc/dwpw.hip
    takes.  Opt-in, FID_DWPW_FUSE=1: measured SLOWER than the two launches -- MobileFaceNet at 32 faces 0.532 vs 0.502 ms, one face 0.350 vs
    0.299 ms: these layers are a few hundred 2-us items, two wide launches hide their load latencies better than one deep one"""
    n = net.nodes[i]
    m = net.nodes[i + 1] if i + 1 < len(net.nodes) else None
    return bool(os.environ.get("FID_DWPW_FUSE") and m is not None and m.kind == "conv" and m.groups == 1 and m.k == 1 and m.pad == 0
                and m.stride == 1 and m.src == n.name and not m.pre_bn and not m.pre_avgpool and not m.res_up2 and n.k == 3 and n.pad == 1
                and n.stride in (1, 2) and cp in (32, 64, 128, 256, 512) and n.name not in net.outputs and m.res != n.name
                and not _users(net, n.name, but=m))


# ---- one emitter per pattern: tables into the blob, tensors, one op record ----------------------------------------------------------------

def _emit_stem_fused(b):
    """SCRFD deep stem (conv/s2 - conv - conv - maxpool, all ReLU): one fused kernel (csrc/stem_fused.hip)"""
    c0, c1, c2, pool = b.net.nodes[:4]
    (W0, b0), (W1, b1), (W2, b2) = (b.folded(c) for c in (c0, c1, c2))
    w0 = np.zeros((32, 32), dtype=np.float32)                      # [co][k = (dy*3+dx)*3 + c_bgr]
    w0[: c0.cout, :27] = (W0[:, ::-1] * (b.net.in_scale / 2.0)).transpose(0, 2, 3, 1).reshape(c0.cout, 27)
    c2p = _rup(c2.cout, CPAD)
    offs = dict(f_w0=b.put(w0.astype(np.float16)), f_b0=b.put(_padded(b0, 32)),
                f_w1=b.put(_pack_weights(W1, 32, 32)), f_b1=b.put(_padded(b1, 32)),
                f_w2=b.put(_pack_weights(W2, 32, c2p)), f_b2=b.put(_padded(b2, c2p)))
    _, hp, wp = b.shp[pool.name]
    dst = b.new_tensor(pool.name, c2.cout, hp, wp)
    b.emit("stem.fused", nodes=[c0.name, c1.name, c2.name, pool.name], type=OP_STEMFUSED, src=-1, dst=dst, kh=3, kw=3,
           macs=sum(b.shp[x.name][1] * b.shp[x.name][2] * x.cout * x.cin * 9 for x in (c0, c1, c2)), **offs)
    b.skip.update(range(4))


def _emit_stem_block(b, ci, c1, others):
    """IResNet's stem + the first 3x3 conv on its result: one fused op (csrc/stem_block.hip)"""
    st = b.net.nodes[0]
    H0, W0 = b.net.in_hw
    W, bias = b.folded(st)                                         # [64, 3(RGB), 3, 3]
    Wd = np.ascontiguousarray((W[:, ::-1] * (b.net.in_scale / 2.0)).transpose(0, 2, 3, 1), dtype=np.float32)   # [co][dy][dx][c_bgr]: the kernel's input is 2 p - 255
    w0off, w0bytes = b.blob.add(Wd)
    b0off = b.put(_padded(bias, 64))
    s0off = b.slopes(st, 64)
    W1, bt1, _, _ = b.fold_conv(c1, (H0, W0))
    # stem_block.hip is built with -fno-honor-nans (its max(v, 0) then needs no canonicalising second v_max): a folded weight or bias that
    # is inf / NaN, or overflows fp16, would be undefined behaviour there instead of propagating -- refused here
    for nm_, arr_ in (("stem weights", Wd), ("stem bias", bias), ("conv1 weights", W1), ("conv1 bias", bt1)):
        if not np.isfinite(np.asarray(arr_, dtype=np.float64)).all() or np.abs(np.asarray(arr_, dtype=np.float64)).max() > 65504.0:
            raise ValueError(f"{st.name} / {c1.name}: folded {nm_} are not finite fp16 values; the fused stem block cannot take them")
    b1t = np.zeros((bt1.shape[0], 64), dtype=np.float32)
    b1t[:, :64] = bt1
    w1off = b.put(_repack_kind2(_pack_weights(W1, 64, 64)))
    b1off = b.put(b1t)
    s1off = b.slopes(c1, 64)
    dst = b.new_tensor(c1.name, 64, H0, W0)
    dst2 = 0
    if others:                                                  # the block's stride-2 shortcut reads x at the even pixels only: a compact second output
        even = st.name + ".even"
        dst2 = b.new_tensor(even, 64, (H0 + 1) // 2, (W0 + 1) // 2) + 1
        b.shp[even] = (64, (H0 + 1) // 2, (W0 + 1) // 2)
        oi_, sc_node = others[0]
        sc2 = dataclasses.replace(sc_node, src=even, stride=1)
        sc2._even_src = True
        b.net = copy.copy(b.net)
        b.net.nodes = list(b.net.nodes)
        b.net.nodes[oi_] = sc2
    b.emit(c1.name, nodes=[st.name, c1.name], type=OP_STEMBLOCK, src=-1, dst=dst, kh=3, kw=3, stride=1, pad=1, cin=3, cout=64, act=ACT[c1.act],
           flags=CF_BORDER if bt1.shape[0] == 9 else 0, woff=w0off, wbytes=w0bytes, boff=b0off, soff=s0off, wrows=64,
           s_w1=w1off, s_b1=b1off, s_s1=s1off, s_act0=ACT[st.act], s_dst2=dst2, macs=H0 * W0 * 64 * 27 + H0 * W0 * 64 * 64 * 9)
    b.skip.update({0, ci})


def _emit_stem(b, n):
    """the first conv on the uint8 frame"""
    assert n.k == 3 and n.pad == 1 and n.groups == 1 and not n.pre_bn and n.res is None
    cout, (_, ho, wo) = n.cout, b.shp[n.name]
    cp = _rup(cout, CPAD)
    assert cp in (32, 64, 128), cp
    W, bias = b.folded(n)                                        # [cout, 3(RGB), 3, 3]
    # kernel input is (2*pixel - 255) in BGR order: fold scale/2 and the channel swap
    Wd = np.zeros((cp, 3, 3, 3), dtype=np.float32)            # [co][dy][dx][c_bgr]
    Wd[:cout] = (W[:, ::-1] * (b.net.in_scale / 2.0)).transpose(0, 2, 3, 1)
    assert abs(b.net.in_mean - 127.5) < 1e-12
    woff, wbytes = b.blob.add(Wd)
    boff = b.put(_padded(bias, cp))
    soff = b.slopes(n, cp)
    dst = b.new_tensor(n.name, cout, ho, wo)
    b.emit(n.name, type=OP_STEM, src=-1, dst=dst, kh=3, kw=3, stride=n.stride, pad=1, cin=3, cout=cout,
           act=ACT[n.act], woff=woff, wbytes=wbytes, boff=boff, soff=soff, wrows=cp)


def _emit_dual(b, i):
    """The block's shortcut (2x2 average pool + 1x1 conv + BN = a 2x2 / stride-2 conv with W/4) reads the tensor the block's
    first conv (3x3 / stride 2 / pad 1) reads, and its window is taps (1..2, 1..2) of that conv's window: ONE launch of the
    stride-2 kernel with twice the couts and two outputs fetches the (large) input once instead of twice (csrc/conv_s2.hip,
    twelve waves: fragments 0..5 = the conv, 6..11 = the shortcut).  Op record: the conv's, with 192 weight / bias rows;
    W_X_DST2 = second output's tensor id + 1, W_X_ACT2 = its activation, W_X_COUT1P = padded couts of the first output, W_F_MACS_* = the MACs
    of the shortcut (cost accounting)."""
    n, m = b.net.nodes[i], b.net.nodes[i + 1]
    cin_p = b.src(n)[T_CP]
    _, ho, wo = b.shp[m.name]
    W1, b1 = b.folded(m)                                                          # [cout, cin, 3, 3]
    Wd, b2 = b.folded(n, _avg_down(b.P[n.wname + ".weight"].astype(np.float64)))  # [cout, cin, 1, 1], avgpool2 folded: 2x2 / stride 2
    W2 = np.zeros((n.cout, n.cin, 3, 3))
    W2[:, :, 1:3, 1:3] = Wd
    Wp = np.concatenate([_pack_weights(W1, cin_p, 96), _pack_weights(W2, cin_p, 96)], axis=0)
    woff, wbytes = b.blob.add(Wp)
    bt = np.zeros((1, 192), dtype=np.float32)
    bt[0, :m.cout] = b1
    bt[0, 96:96 + n.cout] = b2
    boff = b.put(bt)
    dst2 = b.new_tensor(n.name, n.cout, ho, wo)
    dst = b.new_tensor(m.name, m.cout, ho, wo)
    macs2 = ho * wo * n.cout * n.cin * 4
    assert macs2 < 2 ** 31
    b.emit(m.name, nodes=[n.name, m.name], type=OP_CONV, src=b.tid[n.src], dst=dst, res=-1, kh=3, kw=3, stride=2, pad=1, cin=m.cin, cout=m.cout,
           act=ACT[m.act], flags=0, woff=woff, wbytes=wbytes, boff=boff, soff=-1, wrows=192,
           x_dst2=dst2 + 1, x_act2=ACT[n.act], x_cout1p=96, macs=macs2)
    b.skip.add(i + 1)


def _emit_bblock(b, i):
    """A residual BasicBlock on 64 stored channels (SCRFD-10G layer1): conv1 + ReLU -> conv2 -> + block input -> activation as ONE
    launch (csrc/conv_bb.hip): conv1's output only feeds conv2, so it is never materialised.  Both filter banks go into the blob
    in the register-fragment order the kernel loads (repack.hip kind 2).
    IResNet's form of the block (BN - conv - BN - PReLU - conv - BN, + input: arcface_r50 layer1.1 / 1.2) is covered too: the leading
    BatchNorm folds into conv1 with 9 border-class bias rows (flag CF_BORDER), PReLU slopes travel in W_B_S1."""
    n, m = b.net.nodes[i], b.net.nodes[i + 1]
    src_t = b.src(n)
    W1, bt1, _, _ = b.fold_conv(n, (src_t[T_H], src_t[T_W]))
    W2, bt2, _, _ = b.fold_conv(m, (src_t[T_H], src_t[T_W]))
    assert bt2.shape[0] == 1
    cpb = src_t[T_CP]                                         # 64 stored channels, or 32 (conv_bb32: SCRFD-2.5G layer1)
    b1t = np.zeros((bt1.shape[0], cpb), dtype=np.float32)
    b1t[:, :n.cout] = bt1
    offs = dict(b_w1=b.put(_repack_kind2(_pack_weights(W1, cpb, cpb))), b_b1=b.put(b1t),
                b_w2=b.put(_repack_kind2(_pack_weights(W2, cpb, cpb))), b_b2=b.put(_padded(bt2[0], cpb)))
    s1_off = b.slopes(n, cpb)
    _, ho, wo = b.shp[m.name]
    dst = b.new_tensor(m.name, m.cout, ho, wo)
    b.emit(m.name, nodes=[n.name, m.name], type=OP_BBLOCK, src=b.tid[n.src], dst=dst, kh=3, kw=3, stride=1, pad=1, cin=n.cin, cout=m.cout,
           act=ACT[m.act], flags=CF_BORDER if bt1.shape[0] == 9 else 0, b_s1=s1_off, b_act1=ACT[n.act],
           macs=ho * wo * 9 * (n.cout * n.cin + m.cout * m.cin), **offs)
    b.skip.add(i + 1)


def _emit_mbf_block(b, i, d, m):
    """MobileFaceNet's bottleneck: 1x1 (cin -> G, act) -> depthwise 3x3 / stride 1 | 2 (G, act) -> 1x1 (G -> cout) [+ block input] as ONE launch
    (csrc/mbf_block.hip): both expanded maps stay in LDS.  The record is the second pointwise conv's; the W_M_* words hold the first
    pointwise conv's and the depthwise layer's tables, W_F_MACS_* the MACs of the three layers."""
    n = b.net.nodes[i]
    cin_p, gp, cout_p = b.src(n)[T_CP], _rup(n.cout, CPAD), _rup(m.cout, CPAD)
    W1, b1 = b.folded(n)
    w1_off = b.put(_pack_weights(W1, cin_p, gp))
    b1_off = b.put(_padded(b1, gp))
    s1_off = b.slopes(n, gp)
    Wdw, bdw = b.folded(d)                                      # [G, 1, 3, 3]
    Wd = np.zeros((9, gp), dtype=np.float32)
    Wd[:, :d.cout] = Wdw[:, 0].reshape(d.cout, 9).T
    dw_off = b.put(Wd)
    dwb_off = b.put(_padded(bdw, gp))
    dws_off = b.slopes(d, gp)
    W2, b2 = b.folded(m)
    w2_off, w2_bytes = b.blob.add(_pack_weights(W2, gp, cout_p))
    b2_off = b.put(_padded(b2, cout_p)[None, :])
    s2_off = b.slopes(m, cout_p)
    _, ho, wo = b.shp[m.name]
    _, h1, w1_ = b.shp[n.name]
    dst = b.new_tensor(m.name, m.cout, ho, wo)
    b.emit(m.name, nodes=[n.name, d.name, m.name], type=OP_MBBLOCK, src=b.tid[n.src], dst=dst, res=b.res(m), kh=3, kw=3, stride=d.stride, pad=1,
           cin=n.cin, cout=m.cout, act=ACT[m.act], flags=0, woff=w2_off, wbytes=w2_bytes, boff=b2_off, soff=s2_off, wrows=cout_p,
           m_w1=w1_off, m_b1=b1_off, m_s1=s1_off, m_act1=ACT[n.act], m_dw=dw_off, m_dwb=dwb_off, m_dws=dws_off, m_dwact=ACT[d.act], m_gp=gp,
           macs=h1 * w1_ * n.cout * n.cin + ho * wo * d.cout * 9 + ho * wo * m.cout * m.cin)
    b.skip.update({i + 1, i + 2})


def _emit_latfpn(b, i, mj, m, keep_lat):
    """A PAFPN level: lateral 1x1 (+ upsampled coarser lateral) and the 3x3 conv on it as ONE launch (csrc/lat_fpn.hip); the lateral is a
    tensor of its own only when a finer level adds it.  The record is the 3x3 conv's; W_L_*: the lateral's weights / bias / tensor."""
    n = b.net.nodes[i]
    cin_p = b.src(n)[T_CP]
    W0, b0 = b.folded(n)
    w0off = b.put(_pack_weights(W0, cin_p, 64).reshape(64, cin_p))
    b0off = b.put(_padded(b0, 64))
    W1, b1 = b.folded(m)
    w1off, w1bytes = b.blob.add(_repack_kind2(_pack_weights(W1, 64, 64)))
    b1off = b.put(_padded(b1, 64)[None, :])
    _, ho, wo = b.shp[m.name]
    lat_t = b.new_tensor(n.name, n.cout, ho, wo) + 1 if keep_lat else 0
    dst = b.new_tensor(m.name, m.cout, ho, wo)
    b.emit(m.name, nodes=[n.name, m.name], type=OP_LATFPN, src=b.tid[n.src], dst=dst, res=b.res(n), kh=3, kw=3, stride=1, pad=1, cin=m.cin,
           cout=m.cout, act=0, flags=0, woff=w1off, wbytes=w1bytes, boff=b1off, soff=-1, wrows=64, l_w0=w0off, l_b0=b0off, l_lat=lat_t,
           macs=ho * wo * (n.cout * n.cin + m.cout * m.cin * 9))
    b.skip.add(mj)


def _emit_conv(b, n):
    """a dense conv; when it is the conv2 a block's shortcut conv can ride on (pending_sc), with the second weight image that holds both"""
    cin, cout = n.cin, n.cout
    _, ho, wo = b.shp[n.name]
    src_t = b.src(n)
    cin_p, cout_p = src_t[T_CP], _rup(cout, CPAD)
    W, bias_tab, k, stride = b.fold_conv(n, (src_t[T_H], src_t[T_W]))
    ncls = bias_tab.shape[0]
    Wp = _pack_weights(W, cin_p, cout_p)
    sc, sc_op = b.pending_sc.pop(n.name, (None, -1))
    woff, wbytes = b.blob.add(Wp)
    bt = np.zeros((ncls, cout_p), dtype=np.float32)
    bt[:, :cout] = bias_tab
    boff = b.put(bt)
    sc_words = {}
    if sc is not None:                                        # second image: weight rows [9 * Cin_p | Cin2_p], one bias row = both biases
        Wsc, bsc = b.folded(sc)
        if sc.pre_avgpool:                                    # average pool + 1x1 = a 2x2 / stride-2 kernel with W / 4: four taps (dy2, dx2)
            Wsc = _avg_down(Wsc)
        assert ncls == 1 and b.ops[sc_op][W_DST] == b.tid[sc.name]
        W2p = np.concatenate([Wp.reshape(cout_p, -1), _pack_weights(Wsc, b.src(sc)[T_CP], cout_p).reshape(cout_p, -1)], axis=1)
        w2off = b.put(W2p)
        bt2 = np.zeros((1, cout_p), dtype=np.float32)
        bt2[0, :cout] = bias_tab[0] + bsc
        # block input, taps, row length, stride, second images, the shortcut's op
        t2, kw2, s2 = (4, 2, 2) if sc.pre_avgpool else (1, 1, sc.stride)
        sc_words = dict(x_src2=b.tid[sc.src] + 1, x_t2=t2, x_kw2=kw2, x_s2=s2, x_w2off=w2off, x_b2off=b.put(bt2), x_scop=sc_op + 1)
    soff = b.slopes(n, cout_p)
    flags = (CF_BORDER if ncls == 9 else 0) | (CF_RES_UP2 if n.res_up2 else 0)
    if n.res_up2:
        # the kernels read the coarser lateral at (y >> 1, x >> 1): nearest 2x.  The reference PAFPN interpolates to the finer level's
        # exact SIZE, which differs for odd or non-2x levels -- unpinned here (the oracle upsamples by scale 2 too), so refused
        r_t = b.tensors[b.tid[n.res]]
        if (ho, wo) != (2 * r_t[T_H], 2 * r_t[T_W]):
            raise ValueError(f"{n.name}: top-down add of a {r_t[T_H]}x{r_t[T_W]} level onto {ho}x{wo}: only exact 2x levels are supported "
                             "(input sizes that are multiples of 32)")
    dst = b.new_tensor(n.name, cout, ho, wo)
    b.emit(n.name, type=OP_CONV, src=b.tid[n.src], dst=dst, res=b.res(n), kh=k, kw=k, stride=stride, pad=n.pad, cin=cin, cout=cout,
           act=ACT[n.act], flags=flags, woff=woff, wbytes=wbytes, boff=boff, soff=soff, wrows=cout_p, **sc_words)
    if sc is not None:
        b.ops[sc_op][W_X_W2OFF] = len(b.ops)                  # the shortcut op knows the conv that may absorb it (index + 1; csrc/net.h)


def _emit_depthwise(b, i):
    """a depthwise conv, or (_dwpw) the depthwise 3x3 + the pointwise 1x1 that consumes it as one op, the depthwise result in LDS
    (csrc/dwpw.hip): that record is the pointwise conv's; the W_D_* words hold the depthwise tables / activation, W_F_MACS_* the MACs of both."""
    n = b.net.nodes[i]
    assert n.groups == n.cin == n.cout and not n.pre_bn and not n.pre_avgpool and n.res is None
    c = n.cin
    _, ho, wo = b.shp[n.name]
    cp = b.src(n)[T_CP]
    W, bias = b.folded(n)                                       # [c, 1, k, k]
    Wd = np.zeros((n.k * n.k, cp), dtype=np.float32)
    Wd[:, :c] = W[:, 0].reshape(c, -1).T
    woff, wbytes = b.blob.add(Wd)
    boff = b.put(_padded(bias, cp))
    soff = b.slopes(n, cp)
    if not _dwpw(b.net, i, cp):
        dst = b.new_tensor(n.name, c, ho, wo, Cp=cp)
        b.emit(n.name, type=OP_DWCONV, src=b.tid[n.src], dst=dst, kh=n.k, kw=n.k, stride=n.stride, pad=n.pad,
               cin=c, cout=c, act=ACT[n.act], woff=woff, wbytes=wbytes, boff=boff, soff=soff, wrows=cp, groups=c)
        return
    m = b.net.nodes[i + 1]
    Wm, bm = b.folded(m)
    cout_p = _rup(m.cout, CPAD)
    pw_off, pw_bytes = b.blob.add(_pack_weights(Wm, cp, cout_p))
    pb_off = b.put(_padded(bm, cout_p)[None, :])
    ps_off = b.slopes(m, cout_p)
    _, mho, mwo = b.shp[m.name]
    dst = b.new_tensor(m.name, m.cout, mho, mwo)
    b.emit(m.name, nodes=[n.name, m.name], type=OP_DWPW, src=b.tid[n.src], dst=dst, res=b.res(m), kh=3, kw=3, stride=n.stride, pad=1, cin=c,
           cout=m.cout, act=ACT[m.act], flags=0, woff=pw_off, wbytes=pw_bytes, boff=pb_off, soff=ps_off, wrows=cout_p,
           d_woff=woff, d_boff=boff, d_soff=soff, d_act=ACT[n.act], macs=ho * wo * c * n.k * n.k + mho * mwo * m.cout * m.cin)
    b.skip.add(i + 1)


def _emit_maxpool(b, n):
    c, ho, wo = b.shp[n.name]
    dst = b.new_tensor(n.name, c, ho, wo, Cp=b.src(n)[T_CP])
    b.emit(n.name, type=OP_MAXPOOL, src=b.tid[n.src], dst=dst, kh=n.k, kw=n.k, stride=n.stride, pad=n.pad, cin=c, cout=c)


def _emit_fc(b, n):
    """the embedding layer: a 1x1 conv on a [H W Cp] x 1 x 1 view of its source tensor"""
    P = b.P
    src_t = b.src(n)
    C_, Cp_, H_, W_ = src_t[T_C], src_t[T_CP], src_t[T_H], src_t[T_W]
    assert (C_, H_, W_) == (n.c, n.h, n.w)
    Wm = P[n.wname + ".weight"].astype(np.float64).reshape(n.cout, n.c, n.h, n.w)
    bias = P[n.wname + ".bias"].astype(np.float64) if n.bias else np.zeros(n.cout)
    if n.pre_bn:
        a1, b1 = _bn_affine(P, n.wname + ".pre_bn")
        bias = bias + np.einsum("ochw,c->o", Wm, b1)
        Wm = Wm * a1[None, :, None, None]
    if n.post_bn:
        a2, b2 = _bn_affine(P, n.wname + ".post_bn")
        Wm = Wm * a2[:, None, None, None]
        bias = bias * a2 + b2
    K = H_ * W_ * Cp_
    cout_p = _rup(n.cout, CPAD)
    Wk = np.zeros((cout_p, H_, W_, Cp_), dtype=np.float32)     # NHWC flatten order of the activation
    Wk[: n.cout, :, :, : n.c] = Wm.transpose(0, 2, 3, 1)
    woff, wbytes = b.blob.add(Wk.reshape(cout_p, 1, K).astype(np.float16))
    boff = b.put(_padded(bias, cout_p)[None, :])
    view = b.new_tensor(n.name + ".in_view", K, 1, 1, Cp=K)     # alias of the source tensor
    b.tensors[view][T_SLOT] = -2 - b.tid[n.src]                 # resolved to the source's slot by _assign_slots
    dst = b.new_tensor(n.name, n.cout, 1, 1, dtype=1)
    b.emit(n.name, type=OP_CONV, src=view, dst=dst, kh=1, kw=1, stride=1, pad=0, cin=n.c * n.h * n.w,
           cout=n.cout, act=0, flags=0, woff=woff, wbytes=wbytes, boff=boff, wrows=cout_p)


def _emit_dethead(b, n):
    """the three SCRFD output convs of a level as one conv: [scores | boxes * scale | landmarks], sigmoid on the scores, fp32"""
    P = b.P
    A = n.num_anchors
    _, h_, w_ = b.shp[n.name]
    s = float(P[n.wname + ".bbox.scale"][0])
    W = np.concatenate([P[n.wname + ".cls.weight"], P[n.wname + ".bbox.weight"] * s, P[n.wname + ".kps.weight"]], axis=0).astype(np.float64)
    bias = np.concatenate([P[n.wname + ".cls.bias"], P[n.wname + ".bbox.bias"] * s, P[n.wname + ".kps.bias"]]).astype(np.float64)
    cout = 15 * A
    cout_p = _rup(cout, CPAD)
    woff, wbytes = b.blob.add(_pack_weights(W, b.src(n)[T_CP], cout_p))
    boff = b.put(_padded(bias, cout_p)[None, :])
    dst = b.new_tensor(n.name, cout, h_, w_, dtype=1)
    b.emit(n.name, type=OP_CONV, src=b.tid[n.src], dst=dst, kh=n.k, kw=n.k, stride=1, pad=n.k // 2, cin=n.cin,
           cout=cout, act=0, flags=0, nsig=A, woff=woff, wbytes=wbytes, boff=boff, wrows=cout_p)
    b.heads[n.name] = dict(stride=n.stride, anchors=A, cp=cout_p, h=h_, w=w_, score=(0, 1), bbox=(A, 4), kps=(5 * A, 10))


def _assign_slots(ops, tensors, keep):
    """liveness-based slot assignment: writes T_SLOT of every tensor record (an alias takes its base tensor's) and T_FLAGS = 1 of the kept ones"""
    n_t = len(tensors)
    base = [-2 - r[T_SLOT] if r[T_SLOT] <= -2 else t for t, r in enumerate(tensors)]      # alias -> base tensor
    last_use = [-1] * n_t
    for oi, rec in enumerate(ops):
        for t in record_tensors(rec)[0]:
            last_use[base[t]] = oi
    slot_of = [-1] * n_t
    slot_size, free = [], []
    nbytes = lambda t: tensors[t][T_CP] * tensors[t][T_H] * tensors[t][T_W] * (4 if tensors[t][T_DTYPE] == 1 else 2)
    for oi, rec in enumerate(ops):
        dsts = record_tensors(rec)[1]
        for d in dsts:
            need = nbytes(d)
            if d in keep or not free:
                slot_size.append(need)
                slot_of[d] = len(slot_size) - 1
            else:
                best = min(free, key=lambda s: (slot_size[s] < need, abs(slot_size[s] - need)))
                free.remove(best)
                slot_size[best] = max(slot_size[best], need)
                slot_of[d] = best
        for t in range(n_t):
            if base[t] == t and slot_of[t] >= 0 and last_use[t] == oi and t not in keep and t not in dsts:
                free.append(slot_of[t])
        for d in dsts:
            if last_use[d] < 0 and d not in keep:      # produced but never read
                free.append(slot_of[d])
    for t in range(n_t):
        tensors[t][T_SLOT] = slot_of[base[t]]
        if t in keep:
            tensors[t][T_FLAGS] = 1
        assert tensors[t][T_SLOT] >= 0, t


def lower(net: Net, P: Dict[str, np.ndarray]) -> Lowered:
    b = _Builder(net, P)
    off = lambda switch: not os.environ.get(switch)
    if off("FID_NO_STEM_FUSE") and _stem_fused(net):
        _emit_stem_fused(b)
    elif off("FID_NO_STEMBLOCK_FUSE") and _stem_block(net) is not None:
        _emit_stem_block(b, *_stem_block(net))        # (may replace b.net: the block's shortcut then reads the even-pixel copy)
    for i, n in enumerate(b.net.nodes):
        if i in b.skip:
            continue
        at = (b.net, i, b.tensors, b.tid)
        dense = n.kind == "conv" and n.groups == 1
        if dense and n.src != "input" and off("FID_NO_SC_FUSE") and _shortcut_target(*at, b.shp) is not None:
            # A block's shortcut conv CAN run as extra K-steps of the block's conv2 (one more "tap" that reads x at (2 oy, 2 ox): csrc/conv.hip
            # generation 2, ConvArgs::in2).  Both forms are lowered -- this op as it is, and conv2 with a second weight image [9 Cin | Cx] + summed
            # bias -- and the autotuner decides per batch size (the fused form is a generation-12 pick of conv2; this op is then skipped): at 64
            # faces every fused pair wins 5-12 us, at 500 the weights-in-registers kernels the fused form cannot use win instead.
            b.pending_sc[_shortcut_target(*at, b.shp).name] = (n, len(b.ops))     # (this op is emitted next: its index)
        if n.kind == "conv" and n.src == "input":
            _emit_stem(b, n)
        elif _dual_ok(*at, b.shp):
            _emit_dual(b, i)
        elif off("FID_NO_BB_FUSE") and _bblock(*at):
            _emit_bblock(b, i)
        elif dense and off("FID_NO_MBF_FUSE") and _mbf_block(*at, b.shp) is not None:
            _emit_mbf_block(b, i, *_mbf_block(*at, b.shp))
        elif dense and _latfpn(*at) is not None:
            _emit_latfpn(b, i, *_latfpn(*at))
        elif dense:
            _emit_conv(b, n)
        elif n.kind == "conv":
            _emit_depthwise(b, i)
        elif n.kind == "maxpool":
            _emit_maxpool(b, n)
        elif n.kind == "fc":
            _emit_fc(b, n)
        elif n.kind == "dethead":
            _emit_dethead(b, n)
        else:
            raise ValueError(f"cannot lower node {n}")
    _assign_slots(b.ops, b.tensors, keep={b.tid[o] for o in b.net.outputs})

    out = Lowered()
    out.ops = np.asarray(b.ops, dtype=np.int32).reshape(-1, OP_WORDS)
    out.tensors = np.asarray(b.tensors, dtype=np.int32).reshape(-1, TENSOR_WORDS)
    out.blob, out.tensor_id, out.outputs, out.in_hw = b.blob.bytes(), b.tid, list(b.net.outputs), b.net.in_hw
    out.op_names, out.op_nodes, out.fused_groups, out.heads = b.op_names, b.op_nodes, b.fused_groups, b.heads
    return out
