"""Numpy restatement of tiled detection (fid_tile_cut / fid_scrfd_postprocess_tiled): the cut and the per-frame merge, built on the oracle's
own decode, sort and NMS.  Test infrastructure only."""
import numpy as np

from oracle import align as oalign
from oracle import postprocess as pp


def tile_det_scale(row, in_hw):
    """what the post-process divides tile `row`'s coordinates by: exactly 1 for a native tile, the letterbox's new_h / h otherwise"""
    _, _, _, w, h, kind = (int(v) for v in row)
    return 1.0 if kind == 0 else pp.letterbox_geometry(h, w, (in_hw[1], in_hw[0]))[2]


def cut_tiles(frames, tiles, in_hw):
    """frames uint8 [B,H,W,3], tiles int32 [T,6] -> uint8 [T,in_h,in_w,3]: kind 0 is the slice at the top-left of a zero input, kind 1 the
    oracle's letterbox of the slice"""
    in_h, in_w = in_hw
    out = np.zeros((len(tiles), in_h, in_w, 3), np.uint8)
    for t, (b, x0, y0, w, h, kind) in enumerate(np.asarray(tiles).tolist()):
        region = frames[b, y0:y0 + h, x0:x0 + w]
        assert region.shape[:2] == (h, w), (t, region.shape)
        if kind == 0:
            out[t, :h, :w] = region
        else:
            out[t] = oalign.letterbox(region, (in_w, in_h))[0]
    return out


def tile_candidates(heads, row, img_hw, in_hw, conf, edge_margin):
    """one tile's candidates in frame coordinates, in anchor order, after the edge rule: scores [n,1], bboxes [n,4], kpss [n,5,2] (fp32)"""
    _, x0, y0, w, h, _ = (int(v) for v in row)
    s, b, k = pp.decode_heads(heads, in_hw, conf)
    ds = np.float32(tile_det_scale(row, in_hw))
    scores = np.vstack(s).astype(np.float32)
    bboxes = np.vstack(b).astype(np.float32) / ds
    kpss = np.vstack(k).astype(np.float32) / ds
    bboxes = bboxes + np.array([x0, y0, x0, y0], np.float32)
    kpss = kpss + np.array([x0, y0], np.float32)
    assert bboxes.dtype == np.float32 and kpss.dtype == np.float32
    if edge_margin >= 0:
        m = int(edge_margin)
        drop = np.zeros(len(bboxes), bool)
        if x0 > 0:
            drop |= bboxes[:, 0] < np.float32(x0 + m)
        if y0 > 0:
            drop |= bboxes[:, 1] < np.float32(y0 + m)
        if x0 + w < img_hw[1]:
            drop |= bboxes[:, 2] > np.float32(x0 + w - m)
        if y0 + h < img_hw[0]:
            drop |= bboxes[:, 3] > np.float32(y0 + h - m)
        scores, bboxes, kpss = scores[~drop], bboxes[~drop], kpss[~drop]
    return scores, bboxes, kpss


def merge_tiles(heads_per_tile, tiles, img_hw, in_hw, conf=0.5, iou=0.4, edge_margin=8, max_num=0, metric="max", batch=None):
    """-> [(det [K,5], kpss [K,5,2])] per frame: every tile's candidates (oracle.postprocess.decode_heads, / np.float32(det_scale),
    + np.float32(x0 / y0), edge rule) concatenated in table order, then detect_from_heads' sort / nms / max_num statements."""
    tiles = np.asarray(tiles)
    B = int(tiles[:, 0].max()) + 1 if batch is None else int(batch)
    out = []
    for f in range(B):
        parts = [tile_candidates(heads_per_tile[t], tiles[t], img_hw, in_hw, conf, edge_margin) for t in range(len(tiles)) if tiles[t, 0] == f]
        if not parts:
            out.append((np.zeros((0, 5), np.float32), np.zeros((0, 5, 2), np.float32)))
            continue
        scores = np.vstack([p[0] for p in parts])
        bboxes = np.vstack([p[1] for p in parts])
        kpss = np.vstack([p[2] for p in parts])
        # oracle/postprocess.py detect_from_heads, from the sort on
        order = scores.ravel().argsort(kind="stable")[::-1]
        pre_det = np.hstack((bboxes, scores)).astype(np.float32, copy=False)
        pre_det = pre_det[order, :]
        keep = pp.nms(pre_det, iou)
        det = pre_det[keep, :]
        kpss = kpss[order, :, :][keep, :, :]
        if 0 < max_num < det.shape[0]:
            area = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
            center = int(img_hw[0]) // 2, int(img_hw[1]) // 2
            offsets = np.vstack([(det[:, 0] + det[:, 2]) / 2 - center[1],
                                 (det[:, 1] + det[:, 3]) / 2 - center[0]])
            dist2 = np.sum(np.power(offsets, 2.0), 0)
            values = area if metric == "max" else (area - dist2 * 2.0)
            bindex = np.argsort(values, kind="stable")[::-1][0:max_num]
            det = det[bindex, :]
            kpss = kpss[bindex, :]
        out.append((det.astype(np.float32), kpss.astype(np.float32)))
    return out


def random_heads(rng, K, in_hw=(64, 64), lo=0.5, hi=0.99):
    """the nine head arrays of one detector input with exactly K anchors >= 0.5 (distinct scores), in the ONNX output order"""
    ns = [(in_hw[0] // s) * (in_hw[1] // s) * 2 for s in (8, 16, 32)]
    total = sum(ns)
    scores = rng.uniform(0.0, 0.45, total).astype(np.float32)
    pos = rng.choice(total, K, replace=False)
    scores[pos] = rng.permutation(np.linspace(lo, hi, max(K, 1)))[:K].astype(np.float32)
    bbox = rng.uniform(-0.25, 2.0, (total, 4)).astype(np.float32)
    kps = rng.uniform(-1.5, 1.5, (total, 10)).astype(np.float32)
    o = np.cumsum([0] + ns)
    return ([np.ascontiguousarray(scores[o[i]:o[i + 1], None]) for i in range(3)] + [np.ascontiguousarray(bbox[o[i]:o[i + 1]]) for i in range(3)]
            + [np.ascontiguousarray(kps[o[i]:o[i + 1]]) for i in range(3)])
