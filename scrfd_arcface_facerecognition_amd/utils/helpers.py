"""Geometry / similarity helpers with the names and signatures of reference utils/helpers.py
(:6-123).  Each one is a thin host wrapper: upload, one libfaceid call, download.  There is no
numpy implementation behind them -- without the HIP library they raise."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .._lib import Context, check, default_context

reference_alignment = np.array(
    [[[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]]],
    dtype=np.float32)


def _ctx(ctx) -> Context:
    return ctx or default_context(0)


def _align(image, landmark, ctx, want_crop):
    landmark = np.asarray(landmark, dtype=np.float32)
    assert landmark.shape == (5, 2)
    ctx = _ctx(ctx)
    image = np.ascontiguousarray(image, dtype=np.uint8)
    H, W = image.shape[:2]
    fr = ctx.to_device(image[None])
    kp = ctx.to_device(landmark.reshape(1, 1, 10))
    cn = ctx.to_device(np.array([1], np.int32))
    crop = ctx.empty((1, 112, 112, 3), np.uint8)
    M = ctx.empty((1, 6), np.float64)
    check(ctx.lib.fid_align_crops(ctx.handle, C.c_void_p(fr.ptr), 1, H, W, C.c_void_p(kp.ptr), C.c_void_p(cn.ptr), 1, 1,
                                  C.c_void_p(crop.ptr), C.c_void_p(M.ptr)))
    return (crop.download()[0] if want_crop else None), M.download().reshape(2, 3)


def estimate_norm(landmark, image_size=112, *, ctx=None):
    """helpers.py:18-53 -> (M float64 [2,3], 0)."""
    if image_size != 112:
        raise NotImplementedError("only the 112x112 ArcFace template is implemented on the device")
    _, M = _align(np.zeros((2, 2, 3), np.uint8), landmark, ctx, False)
    return M, 0


def norm_crop_image(image, landmark, image_size=112, mode="arcface", *, ctx=None):
    """helpers.py:56-59 -> uint8 [112,112,3]."""
    if image_size != 112:
        raise NotImplementedError("only 112x112 crops are implemented on the device")
    crop, _ = _align(image, landmark, ctx, True)
    return crop


def _decode(points, distance, ncol, ctx):
    ctx = _ctx(ctx)
    points = np.ascontiguousarray(points, dtype=np.float32)
    distance = np.ascontiguousarray(distance, dtype=np.float32)
    n = points.shape[0]
    if n == 0:
        return np.zeros((0, ncol), np.float32)
    p, d = ctx.to_device(points), ctx.to_device(distance)
    o = ctx.empty((n, ncol), np.float32)
    if ncol == 4:
        check(ctx.lib.fid_distance2bbox(ctx.handle, C.c_void_p(p.ptr), C.c_void_p(d.ptr), n, C.c_void_p(o.ptr)))
    else:
        check(ctx.lib.fid_distance2kps(ctx.handle, C.c_void_p(p.ptr), C.c_void_p(d.ptr), n, ncol, C.c_void_p(o.ptr)))
    return o.download()


def distance2bbox(points, distance, max_shape=None, *, ctx=None):
    """helpers.py:62-83"""
    if max_shape is not None:
        raise NotImplementedError("max_shape clamping is unused on the reference path")
    return _decode(points, distance, 4, ctx)


def distance2kps(points, distance, max_shape=None, *, ctx=None):
    """helpers.py:86-107"""
    if max_shape is not None:
        raise NotImplementedError("max_shape clamping is unused on the reference path")
    return _decode(points, distance, np.asarray(distance).shape[1], ctx)


def compute_similarity(feat1: np.ndarray, feat2: np.ndarray, *, ctx=None) -> np.float32:
    """helpers.py:110-123: cosine of two feature vectors (np.float32)."""
    idx, score, cos = match_gallery(np.asarray(feat2).reshape(1, -1), np.asarray(feat1).reshape(1, -1), -2.0, ctx=ctx,
                                    return_matrix=True)
    return np.float32(cos[0, 0])


def compute_similarities(feats1, feats2, *, ctx=None) -> np.ndarray:
    """The cosine of reference smart_face_recognition.py:965-982 (the same formula as helpers.py:110-123) for P pairs at once, in fp32 on the
    raw rows (fid_pair_verify; no fp16 unit rows in between): feats1, feats2 [P, D] -> float32 [P].  A zero row gives NaN, as numpy does."""
    from ..engine import verify_pairs
    score, _, _ = verify_pairs(_ctx(ctx), feats1, feats2, threshold=0.0)
    return score


def match_gallery(embeddings, gallery, thresh, *, ctx=None, return_matrix=False):
    """The gallery scan of reference main.py:136-142 for many faces at once.
    embeddings [N,D], gallery [G,D] (raw, un-normalised) -> (idx int32 [N] (-1 = Unknown), score float32 [N])."""
    from ..engine import Gallery
    ctx = _ctx(ctx)
    emb = np.ascontiguousarray(embeddings, dtype=np.float32)
    n, dim = emb.shape
    gal = gallery if isinstance(gallery, Gallery) else Gallery(ctx, np.asarray(gallery, dtype=np.float32))
    e = ctx.to_device(emb)
    q = ctx.empty((n, dim), np.float16)
    check(ctx.lib.fid_l2_normalize_f16(ctx.handle, C.c_void_p(e.ptr), n, dim, C.c_void_p(q.ptr)))
    idx, sc = ctx.empty((n,), np.int32), ctx.empty((n,), np.float32)
    gal.match_device(q, n, thresh, idx, sc)
    out = (idx.download(), sc.download())
    if return_matrix:
        cm = ctx.empty((n, gal.Gp), np.float32)
        check(ctx.lib.fid_cosine_matrix(ctx.handle, gal.handle, C.c_void_p(q.ptr), n, C.c_void_p(cm.ptr)))
        out = out + (cm.download()[:, :gal.G],)
    if not isinstance(gallery, Gallery):
        gal.close()
    return out


# ---- measured face quality (no reference analogue: its blur and lighting scores read no pixel) ----
def measure_crops(crops, kps=None, M=None):
    """fid_face_measure_host on numpy arrays, no device: crops uint8 [n,112,112,3] (or one [112,112,3]) BGR as norm_crop_image returns them;
    optionally the landmarks [n,5,2] and the matrices estimate_norm returns [n,2,3], both or neither.
    -> per crop a dict keyed by MEASURE_KEYS (python floats holding the float32 words) plus "pose_valid"."""
    from .._lib import MEASURE_KEYS, MEASURE_POSE_VALID, load
    crops = np.ascontiguousarray(crops, dtype=np.uint8)
    if crops.ndim == 3:
        crops = crops[None]
    if crops.ndim != 4 or crops.shape[1:] != (112, 112, 3):
        raise ValueError(f"measure_crops needs uint8 [n,112,112,3] crops, not {crops.shape}")
    if (kps is None) != (M is None):
        raise ValueError("measure_crops: landmarks and M come together or not at all")
    n = len(crops)
    k = None if kps is None else np.ascontiguousarray(kps, dtype=np.float32).reshape(n, 10)
    m = None if M is None else np.ascontiguousarray(M, dtype=np.float64).reshape(n, 6)
    stats, meas = np.zeros((n, 8), np.int64), np.zeros((n, 8), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    check(load().fid_face_measure_host(p(crops), n, p(k), None, p(m), p(stats), p(meas)))
    return [dict({key: float(meas[i, j]) for j, key in enumerate(MEASURE_KEYS)}, pose_valid=bool(stats[i, 7] & MEASURE_POSE_VALID))
            for i in range(n)]


# ---- coasting tracks through missed frames (no reference analogue: the reference draws what it detects) ----
def coast_tracks(entries, stream, det, counts, track, ident_idx=None, ident_score=None, config=None):
    """fid_track_coast_host on numpy arrays, no device: entries int32 [S,T,COAST_WORDS] (updated in place; a fresh state is id -1, every
    other word 0), the step's stream [B], det [B,cap,5], counts [B], track [B,cap,2] and optionally fid_track_identify's ident_idx /
    ident_score [B,cap]; config: _lib.CoastConfig (default: its UNCALIBRATED defaults).
    -> (det [B,cap+T,5], counts [B], track [B,cap+T,2], idx [B,cap+T], score [B,cap+T]): every frame's detections, then its coasted tracks."""
    from .._lib import COAST_WORDS, CoastConfig, load
    if not (isinstance(entries, np.ndarray) and entries.dtype == np.int32 and entries.ndim == 3 and entries.shape[2] == COAST_WORDS
            and entries.flags.c_contiguous):
        raise ValueError(f"coast_tracks needs contiguous int32 [S,T,{COAST_WORDS}] entries")
    S, T = entries.shape[:2]
    det = np.ascontiguousarray(det, dtype=np.float32)
    if det.ndim != 3 or det.shape[2] != 5:
        raise ValueError(f"coast_tracks needs det [B,cap,5], not {det.shape}")
    B, cap = det.shape[:2]
    stream = np.ascontiguousarray(stream, dtype=np.int32).reshape(B)
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(B)
    track = np.ascontiguousarray(track, dtype=np.int32).reshape(B, cap, 2)
    if (ident_idx is None) != (ident_score is None):
        raise ValueError("coast_tracks: ident_idx and ident_score come together or not at all")
    ii = None if ident_idx is None else np.ascontiguousarray(ident_idx, dtype=np.int32).reshape(B, cap)
    sc = None if ident_score is None else np.ascontiguousarray(ident_score, dtype=np.float32).reshape(B, cap)
    cfg = config if config is not None else CoastConfig()
    cap2 = cap + T
    outs = (np.empty((B, cap2, 5), np.float32), np.empty(B, np.int32), np.empty((B, cap2, 2), np.int32), np.empty((B, cap2), np.int32),
            np.empty((B, cap2), np.float32))
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    check(load().fid_track_coast_host(i32(entries), S, T, i32(stream), B, cap, p(det), p(counts), p(track), p(ii), p(sc), C.byref(cfg),
                                      *[p(o) for o in outs]))
    return outs


# ---- re-linking a returning face to its earlier track (no reference analogue: the reference re-identifies against a gallery only) ----
def relink_tracks(state, stream, counts, track, offsets, src, q, n_rows=None, config=None, max_age=15):
    """fid_track_relink_host on numpy arrays, no device: state = dict(live int32 [S,T,8], pool int32 [S,L,8], frames int32 [S],
    live_q fp16 [S,T,dim], pool_q fp16 [S,L,dim]), updated in place (relink_state() makes a fresh one); the step's stream [B], counts [B],
    track [B,cap,2], offsets [B+1], src [row_cap] and the unit fp16 rows q [>= n_rows, dim] (n_rows: default len(q)); config:
    _lib.RelinkConfig (default: its UNCALIBRATED defaults; its pool must be the state's); max_age: the tracker's.
    -> person int32 [B,cap,2] = {person id, word | TRACK_RELINKED}."""
    from .._lib import RELINK_WORDS, RelinkConfig, load
    live, pool, frames, live_q, pool_q = (state[k] for k in ("live", "pool", "frames", "live_q", "pool_q"))
    for a, dt, nd in ((live, np.int32, 3), (pool, np.int32, 3), (frames, np.int32, 1), (live_q, np.float16, 3), (pool_q, np.float16, 3)):
        if not (isinstance(a, np.ndarray) and a.dtype == dt and a.ndim == nd and a.flags.c_contiguous):
            raise ValueError("relink_tracks needs the contiguous state arrays of relink_state()")
    S, T = live.shape[:2]
    L, dim = pool.shape[1], live_q.shape[2]
    if live.shape[2] != RELINK_WORDS or pool.shape != (S, L, RELINK_WORDS) or frames.shape != (S,) or live_q.shape != (S, T, dim) or \
            pool_q.shape != (S, L, dim):
        raise ValueError("relink_tracks: the state arrays do not belong together")
    cfg = config if config is not None else RelinkConfig(pool=L)
    if cfg.pool != L:
        raise ValueError(f"relink_tracks: config.pool = {cfg.pool}, the state's pool has {L} entries")
    track = np.ascontiguousarray(track, dtype=np.int32)
    if track.ndim != 3 or track.shape[2] != 2:
        raise ValueError(f"relink_tracks needs track [B,cap,2], not {track.shape}")
    B, cap = track.shape[:2]
    stream = np.ascontiguousarray(stream, dtype=np.int32).reshape(B)
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(B)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(B + 1)
    src = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
    q = np.ascontiguousarray(q, dtype=np.float16).reshape(-1, dim)
    n = len(q) if n_rows is None else int(n_rows)
    if n > len(q):
        raise ValueError(f"relink_tracks: n_rows = {n}, q has {len(q)} rows")
    person = np.empty((B, cap, 2), np.int32)
    c = cfg.c(max_age)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    check(load().fid_track_relink_host(i32(live), p(live_q), i32(pool), p(pool_q), i32(frames), S, T, L, dim, i32(stream), B, cap, p(counts),
                                       p(track), p(offsets), p(src), len(src), n, p(q), C.byref(c), p(person)))
    return person


def relink_state(streams, max_tracks, pool, dim):
    """a fresh relinker state for relink_tracks: every live entry empty, every pool entry free"""
    from .._lib import RELINK_WORDS
    st = dict(live=np.zeros((streams, max_tracks, RELINK_WORDS), np.int32), pool=np.zeros((streams, pool, RELINK_WORDS), np.int32),
              frames=np.zeros(streams, np.int32), live_q=np.zeros((streams, max_tracks, dim), np.float16),
              pool_q=np.zeros((streams, pool, dim), np.float16))
    st["live"][..., 0] = -1
    st["pool"][..., 0] = -1
    return st


# ---- density clusters of embeddings (no reference analogue: its clustering_results/ come from the greedy visit loop) ----
def cluster_embeddings(embeddings, threshold: float = 0.45, min_samples: int = 2):
    """fid_cluster_host on numpy arrays, no device: embeddings [n, dim] (any scale; a zero row takes no part) are normalised in float64 and
    rounded to fp16 as the gallery stores them, then clustered by the rule of fid_gallery_cluster (include/faceid.h): two rows hit at a cosine
    >= threshold (and > 0), a row with `min_samples` rows within the threshold, itself counted, is a core, clusters are connected cores plus
    their borders, labelled by their lowest core.  The answer does not depend on the order of the rows.  The default threshold is the
    reference's `grouping_threshold`; it is UNCALIBRATED for clustering (score_distribution below measures labelled rows).  -> engine.ClusterResult
    keyed by the row index."""
    from .._lib import load
    from ..engine import cluster_result
    x = np.asarray(embeddings, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"cluster_embeddings needs embeddings [n, dim], not {x.shape}")
    n, dim = x.shape
    nrm = np.sqrt((x * x).sum(1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.ascontiguousarray(np.where(nrm > 0, x / np.where(nrm > 0, nrm, 1), 0).astype(np.float16))
    label, degree, via = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
    score, summary = np.empty(n, np.float32), np.empty(6, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    check(load().fid_cluster_host(p(unit), n, dim, None, n, C.c_float(threshold), int(min_samples), p(label), p(degree), p(via), p(score), p(summary)))
    return cluster_result(list(range(n)), label, degree, via, score, summary)


# ---- genuine / impostor score distributions of labelled embeddings (no reference analogue: its thresholds are constants of config.json) ----
def score_distribution(embeddings, labels, bins: int = 512):
    """fid_score_hist_host on numpy arrays, no device: embeddings [n, dim] (any scale; a zero row takes no part) are normalised in float64 and
    rounded to fp16 as the gallery stores them (as cluster_embeddings does); labels: the person of every row, a sequence of n hashables (None =
    unlabelled) or a mapping row index -> person.  Every pair of labelled rows is counted once into the genuine or the impostor histogram by the
    rule of fid_gallery_score_hist (include/faceid.h).  -> engine.ScoreDistribution keyed by the row index."""
    from .._lib import load
    from ..engine import HIST_MAX_BINS, ScoreDistribution, label_codes
    x = np.asarray(embeddings, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"score_distribution needs embeddings [n, dim], not {x.shape}")
    n, dim = x.shape
    bins = int(bins)
    if bins < 2 or bins > HIST_MAX_BINS or bins % 2:
        raise ValueError(f"score_distribution: bins = {bins} must be even, 2 .. {HIST_MAX_BINS}")
    if not hasattr(labels, "get"):
        if len(labels) != n:
            raise ValueError(f"score_distribution: {len(labels)} labels for {n} rows")
        labels = dict(enumerate(labels))
    codes = label_codes(range(n), labels)
    nrm = np.sqrt((x * x).sum(1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.ascontiguousarray(np.where(nrm > 0, x / np.where(nrm > 0, nrm, 1), 0).astype(np.float16))
    hist, summary = np.empty((2, bins), np.uint64), np.empty(4, np.uint64)
    imp_via, gen_via = np.empty(n, np.int32), np.empty(n, np.int32)
    imp_score, gen_score = np.empty(n, np.float32), np.empty(n, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    check(load().fid_score_hist_host(p(unit), n, dim, None, p(codes), n, bins, p(hist), p(imp_via), p(imp_score), p(gen_via), p(gen_score), p(summary)))
    return ScoreDistribution(list(range(n)), hist, imp_via, imp_score, gen_via, gen_score, summary)


# ---- identity templates: one row per person from many embeddings (no reference analogue: its build_targets takes one photograph per name) ----
def identity_templates(embeddings, labels, weights=None, min_score=None):
    """fid_templates_host on numpy arrays, no device: embeddings [n, dim] (any scale; a zero row takes no part) are normalised in float64 and
    rounded to fp16 as the gallery stores them (as score_distribution does); labels: the person of every row, a sequence of n hashables (None
    = unlabelled) or a mapping row index -> person; weights: None (equal), or the quality in [0, 1] of every row as a sequence or a mapping
    (engine.weight_codes has the mapping to 1 .. 255); min_score: None drops nothing.  The rule of fid_gallery_templates (include/faceid.h):
    exact integer sums, the same bytes as the device.  -> engine.TemplateResult keyed by the row index."""
    from .._lib import load
    from ..engine import TEMPLATE_KEEP_ALL, TEMPLATE_MAX_ROWS, TemplateResult, label_codes, persons_of, weight_codes
    x = np.asarray(embeddings, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"identity_templates needs embeddings [n, dim], not {x.shape}")
    n, dim = x.shape
    if n > TEMPLATE_MAX_ROWS:
        raise ValueError(f"identity_templates: {n} rows exceed the {TEMPLATE_MAX_ROWS} of one call")
    as_map = lambda v, what: v if v is None or hasattr(v, "get") else dict(enumerate(_same_len(v, n, what)))
    labels, weights = as_map(labels, "labels"), as_map(weights, "weights")
    ids = list(range(n))
    codes = label_codes(ids, labels)
    persons = persons_of(ids, labels, codes)
    P = len(persons)
    if P == 0:
        return TemplateResult(ids, [], np.zeros((0, dim), np.float16), np.zeros(n, np.float32), np.full(n, -1, np.int32), np.zeros((0, 4), np.int32),
                              np.zeros(0, np.float32), np.zeros(6, np.int64))
    w = weight_codes(ids, weights)
    nrm = np.sqrt((x * x).sum(1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.ascontiguousarray(np.where(nrm > 0, x / np.where(nrm > 0, nrm, 1), 0).astype(np.float16))
    tpl, score, kept = np.empty((P, dim), np.float16), np.empty(n, np.float32), np.empty(n, np.int32)
    person, cohesion, summary = np.empty((P, 4), np.int32), np.empty(P, np.float32), np.empty(6, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    check(load().fid_templates_host(p(unit), n, dim, None, p(codes), p(w), n, P, C.c_float(TEMPLATE_KEEP_ALL if min_score is None else float(min_score)),
                                    p(tpl), p(score), p(kept), p(person), p(cohesion), p(summary)))
    return TemplateResult(ids, persons, tpl, score, kept, person, cohesion, summary)


def _same_len(v, n, what):
    if len(v) != n:
        raise ValueError(f"identity_templates: {len(v)} {what} for {n} rows")
    return v


# ---- drawing (reference utils/helpers.py:126-179): with OpenCV on the host, cv2's primitives; without it, the library's host rasteriser
# (fid_draw_faces_host: the raster rules of include/faceid.h -- the same pixels fid_draw_faces writes on the device) ----
def _cv2():
    try:
        import cv2
        return cv2
    except ImportError:
        return None


def _draw_host(image, boxes, idx=None, score=None, names=None, colors=None, track=None, style=None):
    """fid_draw_faces_host on one uint8 [H,W,3] image in place: boxes [n,4], optional identities / label table / track ids"""
    from .._lib import DrawStyle, label_arrays, load
    if getattr(image, "dtype", None) != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"drawing needs a uint8 [H,W,3] image, not {getattr(image, 'dtype', None)} {getattr(image, 'shape', None)}")
    n = len(boxes)
    if n == 0:
        return image
    buf = image if image.flags.c_contiguous and image.flags.writeable else np.ascontiguousarray(image)
    H, W = buf.shape[:2]
    det = np.zeros((n, 5), np.float32)
    det[:, :4] = np.asarray(boxes, dtype=np.float32).reshape(n, 4)
    counts = np.array([n], np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    idx = None if idx is None else np.ascontiguousarray(idx, np.int32)
    score = None if score is None else np.ascontiguousarray(score, np.float32)
    trk = None
    if track is not None:
        trk = np.zeros((n, 2), np.int32)
        trk[:, 0] = track
    raw, offsets, bgr = (None, None, None) if names is None else label_arrays(names, colors)
    style = style if style is not None else DrawStyle()
    check(load().fid_draw_faces_host(p(buf), 1, H, W, p(det), p(counts), n, p(idx), p(score), n, None, 0, p(trk), raw, p(offsets), p(bgr),
                                     0 if names is None else len(names), C.byref(style)))
    if buf is not image:
        image[...] = buf
    return image


def _face_names(faces):
    """the label table of one face list: (names in order of first appearance, per face its row or -1 for "Unknown")"""
    names, idx = [], []
    for face in faces:
        name = face[3]
        if name == "Unknown":
            idx.append(-1)
            continue
        if name not in names:
            names.append(name)
        idx.append(names.index(name))
    return names, idx


def draw_faces(image, faces, colors=None, style=None):
    """Draw one frame's face list -- an entry of `results()` / `results_tracked()`: (bbox, det_score, kps, name, similarity[, track id, ...])
    per face -- onto `image` (uint8 [H,W,3], in place; returned) on the host, in list order (a later face shows over an earlier one).
    colors: {name: (b, g, r)} or None (a fixed colour per name, in order of first appearance); "Unknown" is drawn in style.unknown_bgr."""
    names, idx = _face_names(faces)
    bgr = [colors[n] for n in names] if colors is not None and names else None
    track = [face[5] for face in faces] if faces and all(len(face) > 5 for face in faces) else None
    return _draw_host(image, [np.asarray(face[0], np.float32)[:4] for face in faces], idx, [face[4] for face in faces], names or None, bgr,
                      track, style)


def redact_faces(image, faces, known=None, style=None):
    """Redact one frame's faces on `image` (uint8 [H,W,3], in place; returned) on the host (fid_redact_faces_host): a mosaic or a solid fill
    over every face `style` (_lib.RedactStyle; default: an 8-cell mosaic over the unknown ones) selects.  faces: boxes (x1, y1, x2, y2, ...)
    or entries of `results()` (bbox, det_score, kps, name, similarity, ...).  known: one truth value per face; None: an entry whose name is
    not "Unknown" is known, a plain box is not.  Redact before draw_faces, so that boxes and names stay legible on top."""
    from .._lib import RedactStyle, load
    if getattr(image, "dtype", None) != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"redaction needs a uint8 [H,W,3] image, not {getattr(image, 'dtype', None)} {getattr(image, 'shape', None)}")
    n = len(faces)
    if n == 0:
        return image
    entries = [np.ndim(face[0]) > 0 for face in faces]
    if known is None:
        known = [e and face[3] != "Unknown" for e, face in zip(entries, faces)]
    if len(known) != n:
        raise ValueError(f"redact_faces: {len(known)} known flags for {n} faces")
    buf = image if image.flags.c_contiguous and image.flags.writeable else np.ascontiguousarray(image)
    H, W = buf.shape[:2]
    det = np.zeros((n, 5), np.float32)
    det[:, :4] = [np.asarray(face[0] if e else face, np.float32)[:4] for e, face in zip(entries, faces)]
    counts = np.array([n], np.int32)
    idx = np.array([0 if k else -1 for k in known], np.int32)
    score = np.zeros(n, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    style = style if style is not None else RedactStyle()
    check(load().fid_redact_faces_host(p(buf), 1, H, W, p(det), p(counts), n, p(idx), p(score), n, None, 0, C.byref(style)))
    if buf is not image:
        image[...] = buf
    return image


def draw_bbox(image, bbox, color=(0, 255, 0), thickness=3, proportion=0.2):
    cv2 = _cv2()
    if cv2 is None:
        from .._lib import DrawStyle
        return _draw_host(image, [np.asarray(bbox, np.float32)[:4]],
                          style=DrawStyle(proportion, thickness, 0, 0, 0, tuple(int(c) for c in color[:3])))
    x1, y1, x2, y2 = map(int, bbox)
    cv2.rectangle(image, (x1, y1), (x2, y2), color, max(1, thickness // 3))
    L = int(min(x2 - x1, y2 - y1) * proportion)
    for (cx, cy, sx, sy) in ((x1, y1, 1, 1), (x2, y1, -1, 1), (x1, y2, 1, -1), (x2, y2, -1, -1)):
        cv2.line(image, (cx, cy), (cx + sx * L, cy), color, thickness)
        cv2.line(image, (cx, cy), (cx, cy + sy * L), color, thickness)
    return image


def draw_bbox_info(frame, bbox, similarity, name, color):
    cv2 = _cv2()
    if cv2 is None:                     # name, two-decimal similarity, box and similarity bar in `color`
        return _draw_host(frame, [np.asarray(bbox, np.float32)[:4]], [0], [similarity], [name], [tuple(int(c) for c in color[:3])])
    x1, y1, _, _ = map(int, bbox)
    cv2.putText(frame, f"{name}: {similarity:.2f}", (x1, y1 - 10), cv2.FONT_HERSHEY_SIMPLEX, 1, color, 2)
    draw_bbox(frame, bbox, color)


# ---- NV12 -> BGR on the host (no reference analogue: cv2.VideoCapture converts before the reference sees a frame).  fid_nv12_to_bgr_host:
# the integer definition of include/faceid.h -- the bytes the device's fid_nv12_to_bgr and the fused *_nv12 readers see ----
def nv12_to_bgr(nv12, H, W, standard="bt601", *, pitch=None, uv_offset=None, frame_stride=None):
    """One NV12 frame (uint8 [H*3//2, W]: H rows of Y, then H/2 rows of interleaved U, V) or a batch of them ([B, H*3//2, W]) -> uint8
    [H,W,3] / [B,H,W,3] BGR.  standard: "bt601" (limited range, OpenCV's COLOR_YUV2BGR_NV12), "bt709", "bt601_full".  A pitched layout is
    given by pitch / uv_offset / frame_stride (fid_nv12_desc) with `nv12` the flat allocation of ONE frame unless frame_stride says more."""
    from .._lib import load, nv12_desc
    H, W = int(H), int(W)
    buf = np.ascontiguousarray(nv12, dtype=np.uint8)
    desc = nv12_desc(H, W, pitch, uv_offset, frame_stride, standard)
    frame_bytes = desc.uv_offset + desc.pitch * (H // 2)
    single = buf.ndim <= 2 and buf.size < desc.frame_stride + frame_bytes
    B = 1 if single else (buf.size - frame_bytes) // max(int(desc.frame_stride), 1) + 1
    if buf.size < (B - 1) * desc.frame_stride + frame_bytes:
        raise ValueError(f"nv12_to_bgr: {buf.size} bytes cannot hold a {W}x{H} NV12 frame of {frame_bytes} bytes")
    out = np.empty((B, H, W, 3), np.uint8)
    check(load().fid_nv12_to_bgr_host(buf.ctypes.data_as(C.c_void_p), C.byref(desc), B, H, W, out.ctypes.data_as(C.c_void_p)))
    return out[0] if single else out


# ---- BGR -> NV12 on the host, and the overlay on NV12 frames (no reference analogue: cv2.VideoWriter converts BGR frames on the host).
# fid_bgr_to_nv12_host / fid_draw_faces_nv12_host: the integer definitions of include/faceid.h, the bytes the device calls write ----
def bgr_to_nv12(image_or_batch, standard="bt601", *, pitch=None, uv_offset=None, frame_stride=None):
    """One BGR image (uint8 [H,W,3], H and W even) or a batch ([B,H,W,3]) -> NV12, the twin of nv12_to_bgr: uint8 [H*3//2, W] / [B, H*3//2, W]
    in the dense layout; with pitch / uv_offset / frame_stride (fid_nv12_desc) the flat allocation of the pitched layout, B * frame_stride
    bytes, whose padding is zero.  Luma per pixel, chroma the box-filtered sample of each 2 x 2 group."""
    from .._lib import load, nv12_desc
    img = np.ascontiguousarray(image_or_batch, dtype=np.uint8)
    single = img.ndim == 3
    if img.ndim not in (3, 4) or img.shape[-1] != 3:
        raise ValueError(f"bgr_to_nv12 needs uint8 [H,W,3] or [B,H,W,3], not {img.shape}")
    B, H, W = (1,) + img.shape[:2] if single else img.shape[:3]
    desc = nv12_desc(H, W, pitch, uv_offset, frame_stride, standard)
    dense = pitch is None and uv_offset is None and frame_stride is None
    out = np.zeros(max(B * int(desc.frame_stride), 1), np.uint8)
    check(load().fid_bgr_to_nv12_host(img.ctypes.data_as(C.c_void_p), B, H, W, out.ctypes.data_as(C.c_void_p), C.byref(desc)))
    if not dense:
        return out
    out = out.reshape(B, H * 3 // 2, W)
    return out[0] if single else out


def draw_faces_nv12(nv12, H, W, faces, colors=None, style=None, standard="bt601"):
    """draw_faces on one dense NV12 frame (uint8 [H*3//2, W], in place; returned): the same boxes, names and scores, painted on the Y plane
    pixel by pixel and on the UV plane pair by pair (a pair takes the colour of the last face that covers any pixel of its 2 x 2 group)."""
    from .._lib import DrawStyle, label_arrays, load, nv12_desc
    H, W = int(H), int(W)
    if getattr(nv12, "dtype", None) != np.uint8 or nv12.size != H * W * 3 // 2:
        raise ValueError(f"drawing needs a dense uint8 [{H * 3 // 2}, {W}] NV12 frame, not {getattr(nv12, 'dtype', None)} {getattr(nv12, 'shape', None)}")
    n = len(faces)
    if n == 0:
        return nv12
    names, idx = _face_names(faces)
    bgr = [colors[m] for m in names] if colors is not None and names else None
    buf = nv12 if nv12.flags.c_contiguous and nv12.flags.writeable else np.ascontiguousarray(nv12)
    det = np.zeros((n, 5), np.float32)
    det[:, :4] = np.asarray([np.asarray(face[0], np.float32)[:4] for face in faces], np.float32).reshape(n, 4)
    counts, idx = np.array([n], np.int32), np.ascontiguousarray(idx, np.int32)
    score = np.ascontiguousarray([face[4] for face in faces], np.float32)
    trk = None
    if all(len(face) > 5 for face in faces):
        trk = np.zeros((n, 2), np.int32)
        trk[:, 0] = [face[5] for face in faces]
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    raw, offsets, cols = (None, None, None) if not names else label_arrays(names, bgr)
    style = style if style is not None else DrawStyle()
    desc = nv12_desc(H, W, standard=standard)
    check(load().fid_draw_faces_nv12_host(p(buf), C.byref(desc), 1, H, W, p(det), p(counts), n, p(idx), p(score), n, None, 0, p(trk), raw, p(offsets),
                                          p(cols), len(names), C.byref(style)))
    if buf is not nv12:
        nv12[...] = buf.reshape(nv12.shape)
    return nv12
