"""Oracle: the two conv nets behind session.run (reference models/scrfd.py:83, arcface.py:51),
interpreted layer by layer in fp32 with torch-CPU from the unfused graph in
scrfd_arcface_facerecognition_amd/archs.py.  BatchNorm is applied as BatchNorm (not folded), so
this checks the product's folding / packing / fusion as well as its kernels.
Test infrastructure only.  PARITY UNPINNED against onnxruntime (no .onnx, no ORT offline)."""
import numpy as np
import torch
import torch.nn.functional as F

from scrfd_arcface_facerecognition_amd.archs import BN_EPS


def _bn(x, P, prefix):
    g, b = torch.from_numpy(P[prefix + ".gamma"]).to(x.dtype), torch.from_numpy(P[prefix + ".beta"]).to(x.dtype)
    m, v = torch.from_numpy(P[prefix + ".mean"]).to(x.dtype), torch.from_numpy(P[prefix + ".var"]).to(x.dtype)
    if x.dim() == 4:
        return F.batch_norm(x, m, v, g, b, False, 0.0, BN_EPS)
    return (x - m) / torch.sqrt(v + BN_EPS) * g + b


@torch.no_grad()
def run_net(net, P, blob, keep=None, dtype=torch.float32, store=None, bn=None):
    """blob: float32 [N,3,H,W] (already normalised, RGB).  Returns {name: np.ndarray} for the net
    outputs (plus any tensor named in `keep`).  DetHead outputs are (scores[N,HWA,1],
    bbox[N,HWA,4], kps[N,HWA,10]) like the 9 ONNX outputs of SCRFD.
    dtype: the precision the net is evaluated in.  store: None, or store(name, y) -> y applied to the result of
    every conv / maxpool node, the tensors the executor keeps as fp16 (tests/exact_probe.py rounds them there, in
    float64: the exact reference).  FC and DetHead results are fp32 tensors on the device and do not pass through it.
    bn: None (BatchNorm as BatchNorm), or bn(x, prefix) -> y in its place (tests/exact_probe.py: the ideal affine of its probe parameters)."""
    t = {"input": torch.from_numpy(np.ascontiguousarray(blob)).to(dtype)}
    par = lambda k: torch.from_numpy(P[k]).to(dtype)
    stored = (lambda name, y: y) if store is None else store
    norm = (lambda x, prefix: _bn(x, P, prefix)) if bn is None else bn
    for n in net.nodes:
        x = t[n.src]
        if n.kind == "conv":
            w = n.wname
            if n.pre_bn:
                x = norm(x, w + ".pre_bn")
            if n.pre_avgpool:
                x = F.avg_pool2d(x, 2, 2)
            b = par(w + ".bias") if n.bias else None
            y = F.conv2d(x, par(w + ".weight"), b, n.stride, n.pad, 1, n.groups)
            if n.post_bn:
                y = norm(y, w + ".post_bn")
            if n.res is not None:
                r = t[n.res]
                if n.res_up2:
                    r = F.interpolate(r, scale_factor=2, mode="nearest")
                y = y + r
            if n.act == "relu":
                y = F.relu(y)
            elif n.act == "prelu":
                y = F.prelu(y, par(w + ".prelu"))
            t[n.name] = stored(n.name, y)
        elif n.kind == "maxpool":
            t[n.name] = stored(n.name, F.max_pool2d(x, n.k, n.stride, n.pad))
        elif n.kind == "fc":
            w = n.wname
            if n.pre_bn:
                x = norm(x, w + ".pre_bn")
            y = x.flatten(1) @ par(w + ".weight").T
            if n.bias:
                y = y + par(w + ".bias")
            if n.post_bn:
                y = norm(y, w + ".post_bn")
            t[n.name] = y
        elif n.kind == "dethead":
            w, A = n.wname, n.num_anchors
            pad = n.k // 2
            cls = torch.sigmoid(F.conv2d(x, par(w + ".cls.weight"),
                                         par(w + ".cls.bias"), 1, pad))
            bb = F.conv2d(x, par(w + ".bbox.weight"),
                          par(w + ".bbox.bias"), 1, pad) * float(P[w + ".bbox.scale"][0])
            kp = F.conv2d(x, par(w + ".kps.weight"),
                          par(w + ".kps.bias"), 1, pad)
            N = x.shape[0]
            t[n.name] = (cls.permute(0, 2, 3, 1).reshape(N, -1, 1),
                         bb.permute(0, 2, 3, 1).reshape(N, -1, 4),
                         kp.permute(0, 2, 3, 1).reshape(N, -1, 10))
        else:
            raise ValueError(n.kind)
    names = list(net.outputs) + list(keep or [])
    out = {}
    for k in names:
        v = t[k]
        out[k] = tuple(a.numpy() for a in v) if isinstance(v, tuple) else v.numpy()
    return out


def scrfd_session_outputs(net, P, blob):
    """The 9 arrays SCRFD's session.run returns for ONE image (scrfd.py:83-94 order):
    scores(8,16,32), bbox(8,16,32), kps(8,16,32)."""
    o = run_net(net, P, blob)
    heads = [o[k] for k in net.outputs]
    return ([h[0][0] for h in heads] + [h[1][0] for h in heads] + [h[2][0] for h in heads])
