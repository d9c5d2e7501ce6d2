"""`FaceAnalysis`-style front end: what the reference's product layer gets from
`insightface.app.FaceAnalysis(...).get(image)` (smart_face_recognition.py:356-358,1473-1519,
compare_face_from_api.py:69-70,157-174): a list of faces, each with `bbox`, `kps`, `det_score`,
`embedding` and `normed_embedding`, plus the product layer's quality scores, side-face test and best-face
selection with its rejections (smart_face_recognition.py:1145-1216,1218-1297,1299-1399) -- `fid_face_gates`.
All faces of an image are aligned and embedded in ONE batch on the device."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np

from ._lib import MEASURE_KEYS, GateConfig, MeasureConfig, check
from .models import ArcFace, SCRFD

VERDICTS = ("accepted", "no face", "confidence too low", "side face", "quality too low")      # FID_GATE_* (include/faceid.h)
QUALITY_KEYS = ("overall", "blur", "pose", "lighting", "size")


def face_measure(ctx, crops, n_rows: int, kps=None, src=None, M=None):
    """fid_face_measure on device buffers: sharpness, exposure and pose of the first `n_rows` aligned crops (uint8 [*,112,112,3] as the
    fid_align_crops* calls write them).  src: the row table (int32, a row < 0 is no face); kps / M: the landmarks the rows pick from and
    the rows' similarity matrices, both or neither.  Asynchronous.  -> (stats int64 [n_rows,8], measure float32 [n_rows,8]) on the device"""
    from ._lib import _ptr
    stats, measure = ctx.empty((n_rows, 8), np.int64), ctx.empty((n_rows, 8), np.float32)
    check(ctx.lib.fid_face_measure(ctx.handle, _ptr(crops), n_rows, _ptr(kps) if kps is not None else None,
                                   _ptr(src) if src is not None else None, _ptr(M) if M is not None else None, C.c_void_p(stats.ptr),
                                   C.c_void_p(measure.ptr)))
    return stats, measure


def measured_dicts(stats: np.ndarray, measure: np.ndarray):
    """host copies of fid_face_measure's outputs -> per row a dict keyed by MEASURE_KEYS, or None for a row that is no face"""
    return [dict(zip(MEASURE_KEYS, (float(v) for v in measure[i, :7]))) if stats[i, 7] & 1 else None for i in range(len(stats))]


def face_gates(ctx, det_dev, kps_dev, counts_dev, batch: int, cap: int, faces_per_frame: int, config: Optional[GateConfig] = None, pose=None,
               measures=None, offsets=None, measure_config: Optional[MeasureConfig] = None):
    """The reference's quality / side-face gates and best-face selection (smart_face_recognition.py:1145-1216, 1218-1297, 1299-1399,
    1473-1519) for every face of a batch, on the post-process's device arrays (`PostProcessor.det / .kps / .counts`, cap = their
    second dimension).  pose: optional [batch, faces_per_frame, 2] yaw / pitch in radians (0 = not available), handed over as float64.
    measures: optional (stats, measure) device buffers of face_measure -- then fid_face_gates_measured decides, with blur, lighting, pose and
    the side test measured for every face whose row carries them: face f of frame b is row offsets[b] + f (offsets: the device table of
    fid_face_pack) or, without offsets, row b * faces_per_frame + f; measure_config: the MeasureConfig (its defaults are uncalibrated).
    -> quality [batch, F, 5] (QUALITY_KEYS), side score [batch, F], side flag [batch, F] (bool), best [batch, 2] = (face index or -1, verdict)"""
    cfg = config or GateConfig()
    F = faces_per_frame
    quality = ctx.empty((batch, F, 5), np.float32)
    side = ctx.empty((batch, F), np.int32)
    best = ctx.empty((batch, 2), np.int32)
    if measures is not None:
        if pose is not None:
            raise ValueError("face_gates: measured gates take no pose angles")
        stats, measure = measures
        mcfg = measure_config or MeasureConfig()
        check(ctx.lib.fid_face_gates_measured(ctx.handle, C.c_void_p(det_dev.ptr), C.c_void_p(kps_dev.ptr), C.c_void_p(counts_dev.ptr), batch, cap, F,
                                              C.c_void_p(stats.ptr), C.c_void_p(measure.ptr), C.c_void_p(offsets.ptr) if offsets is not None else None,
                                              min(stats.shape[0], measure.shape[0]), C.byref(cfg), C.byref(mcfg), C.c_void_p(quality.ptr),
                                              C.c_void_p(side.ptr), C.c_void_p(best.ptr)))
        sd = side.download()
        return quality.download(), sd & 0xFFFF, (sd >> 16).astype(bool), best.download()
    pose_dev = ctx.to_device(np.ascontiguousarray(pose, dtype=np.float64).reshape(batch, F, 2)) if pose is not None else None   # (float64 across the boundary: python floats in the reference)
    check(ctx.lib.fid_face_gates(ctx.handle, C.c_void_p(det_dev.ptr), C.c_void_p(kps_dev.ptr), C.c_void_p(counts_dev.ptr), batch, cap, F,
                                 C.c_void_p(pose_dev.ptr) if pose_dev is not None else None, C.byref(cfg), C.c_void_p(quality.ptr),
                                 C.c_void_p(side.ptr), C.c_void_p(best.ptr)))
    sd = side.download()
    return quality.download(), sd & 0xFFFF, (sd >> 16).astype(bool), best.download()


def _approve_label(approve) -> int:
    """a comparison record's `approve` as fid_pair_verify's label: 1 / 0 where `approve == True` / `approve == False` holds (bools, and the
    numbers 1 and 0 an API may send instead: what `record['approve'] == same_person`, smart_face_recognition.py:1082, can ever match), else -1"""
    if isinstance(approve, (bool, int, float, np.bool_, np.integer, np.floating)):
        return 1 if approve == 1 else 0 if approve == 0 else -1
    return -1


class Face(dict):
    """dict with attribute access, like insightface's Face"""
    __getattr__ = dict.get

    @property
    def embedding_norm(self):
        return float(np.linalg.norm(self["embedding"])) if self.get("embedding") is not None else None


class FaceAnalysis:
    def __init__(self, det_model: str = "synthetic:scrfd_10g", rec_model: str = "synthetic:arcface_r50", *, device: int = 0,
                 det_size=(640, 640), det_thresh: float = 0.5, max_faces: int = 64, gate_config: Optional[GateConfig] = None,
                 measured_quality: bool = False, measure_config: Optional[MeasureConfig] = None):
        """measured_quality: get / get_batch measure every aligned crop (fid_face_measure: sharpness, exposure, pose) right behind the warp,
        gate with the measured scores (fid_face_gates_measured, `measure_config`: a MeasureConfig, whose defaults are uncalibrated) and give
        each Face a `measured` dict keyed by MEASURE_KEYS; best_face / process_visits then reject on measured quality through the unchanged
        verdict path.  Off (the default): no `measured` key, nothing new is launched."""
        self.det = SCRFD(det_model, input_size=det_size, conf_thres=det_thresh, device=device)
        self.rec = ArcFace(rec_model, device=device, ctx=self.det.ctx, max_batch=max_faces)
        self.ctx = self.det.ctx
        self.max_faces = int(max_faces)
        self.gate_config = gate_config or GateConfig()       # the reference's config.json thresholds (GateConfig.from_reference_json)
        self.measured_quality = bool(measured_quality)
        self.measure_config = measure_config or MeasureConfig()
        self.last_verdict = None                              # of the last best_face(): one of VERDICTS
        self.last_batch_best = []                             # of the last get_batch(): per image (best face index, FID_GATE_* verdict)

    tiled, tile_overlap, tile_margin = False, 128, 8         # prepare(tiled=True, ...) changes them

    def prepare(self, ctx_id: int = 0, det_size=(640, 640), det_thresh: Optional[float] = None, tiled: bool = False, tile_overlap: int = 128,
                tile_margin: int = 8):
        """insightface API compatibility (smart_face_recognition.py:358).  tiled=True: get / get_batch on images of one size detect tiled
        (SCRFD.detect_tiled: native-resolution tiles `tile_overlap` pixels apart plus one overview tile, candidates within `tile_margin`
        pixels of a cut dropped); a get_batch list whose images differ in size keeps the mixed-size path, which letterboxes every image whole."""
        self.det.input_size = det_size
        if det_thresh is not None:
            self.det.conf_thres = det_thresh
        self.tiled, self.tile_overlap, self.tile_margin = bool(tiled), int(tile_overlap), int(tile_margin)

    def get(self, image: np.ndarray, max_num: int = 0) -> List[Face]:
        if self.tiled:
            det, kpss = self.det.detect_tiled(image, max_num=max_num, overlap=self.tile_overlap, edge_margin=self.tile_margin)
        else:
            det, kpss = self.det.detect(image, max_num=max_num)
        n = min(len(det), self.max_faces)
        if n == 0:
            return []
        ctx = self.ctx
        H, W = image.shape[:2]
        fr = ctx.to_device(np.ascontiguousarray(image, dtype=np.uint8)[None])
        kp = ctx.to_device(np.ascontiguousarray(kpss[:n], dtype=np.float32).reshape(1, n, 10))
        cn = ctx.to_device(np.array([n], np.int32))
        crops = ctx.empty((n, 112, 112, 3), np.uint8)
        Mm = ctx.empty((n, 6), np.float64) if self.measured_quality else None
        check(ctx.lib.fid_align_crops(ctx.handle, C.c_void_p(fr.ptr), 1, H, W, C.c_void_p(kp.ptr), C.c_void_p(cn.ptr), n, n,
                                      C.c_void_p(crops.ptr), C.c_void_p(Mm.ptr) if Mm is not None else None))
        measures = face_measure(ctx, crops, n, kps=kp, M=Mm) if self.measured_quality else None
        net = self.rec.session.compiled()
        net.run_device(crops, n)
        emb_ptr, _, _ = net.tensor(net.low.outputs[0])
        q = ctx.empty((n, 512), np.float16)
        check(ctx.lib.fid_l2_normalize_f16(ctx.handle, C.c_void_p(emb_ptr), n, 512, C.c_void_p(q.ptr)))
        emb = net.read(net.low.outputs[0], n).reshape(n, 512)
        normed = q.download().astype(np.float32)
        # quality scores, side-face flag and the best-face verdict of the reference's product layer, all faces in one launch
        dd = ctx.to_device(np.ascontiguousarray(det[:n], dtype=np.float32).reshape(1, n, 5))
        quality, side_score, side_flag, best = face_gates(ctx, dd, kp, cn, 1, n, n, self.gate_config, measures=measures,
                                                          measure_config=self.measure_config)
        self._best = (int(best[0, 0]), int(best[0, 1]))
        faces = [Face(bbox=det[i, :4].copy(), det_score=float(det[i, 4]), kps=kpss[i].copy(), embedding=emb[i].copy(),
                      normed_embedding=normed[i].copy(), quality={k: float(quality[0, i, j]) for j, k in enumerate(QUALITY_KEYS)},
                      is_side_face=bool(side_flag[0, i]), side_face_score=int(side_score[0, i])) for i in range(n)]
        if measures is not None:
            for f, m in zip(faces, measured_dicts(measures[0].download(), measures[1].download())):
                f["measured"] = m
        return faces

    def get_batch(self, images, max_num: int = 0) -> List[List[Face]]:
        """get() for a batch of images ([B,H,W,3], or a list whose images may differ in size: then every chunk is one mixed-size batch,
        fid_align_crops_packed_ragged in place of fid_align_crops_packed): the detector runs on the batch (`SCRFD.detect_batch`, in its
        chunks of `max_batch` images), and all faces of a chunk's images -- every one, the reference's max_num = 0 default, or its
        top-`max_num` per image -- go through alignment, recogniser and normalisation as one packed row list (fid_face_pack), in runs of
        at most `max_faces` rows: nothing is truncated.  Gates: `face_gates` on the chunk's detections.  -> per image its list of Face."""
        mixed = isinstance(images, (list, tuple)) and len({tuple(np.shape(im)) for im in images}) > 1
        if mixed:
            images = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        else:
            images = np.ascontiguousarray(np.stack([np.asarray(im, dtype=np.uint8) for im in images]) if isinstance(images, (list, tuple)) else images,
                                          dtype=np.uint8)
            assert images.ndim == 4 and images.shape[3] == 3, images.shape
            H, W = images.shape[1:3]
        ctx, lib = self.ctx, self.ctx.lib
        net = self.rec.session.compiled()
        out: List[List[Face]] = []
        bests: List[tuple] = []                               # per image (best face index or -1, FID_GATE_* verdict): process_visits reads it
        tiled = self.tiled and not mixed                      # (a mixed-size list keeps the ragged path: prepare's docstring)
        step = self.det.tiled_frames_per_chunk(H, W, self.tile_overlap) if tiled else self.det._max_batch
        for b0 in range(0, len(images), step):
            chunk = images[b0:b0 + step]
            B = len(chunk)
            batch = ctx.image_batch(chunk) if mixed else None
            dets = (self.det._detect_chunk_ragged(chunk, max_num, "max", batch) if mixed
                    else self.det._detect_chunk_tiled(chunk, max_num, "max", self.tile_overlap, self.tile_margin) if tiled
                    else self.det._detect_chunk(chunk, max_num, "max"))   # host results; the post-process's device arrays stay valid
            post = self.det._postprocessor()
            total = sum(len(d) for d, _ in dets)
            if total == 0:
                out += [[] for _ in range(B)]
                bests += [(-1, 1)] * B
                continue
            fr = None if mixed else ctx.to_device(chunk)
            offsets, src = ctx.empty((B + 1,), np.int32), ctx.empty((total,), np.int32)
            check(lib.fid_face_pack(ctx.handle, C.c_void_p(post.counts.ptr), B, post.cap, 0, C.c_void_p(offsets.ptr), C.c_void_p(src.ptr), total))
            emb = np.empty((total, 512), np.float32)
            normed = np.empty((total, 512), np.float32)
            rows = min(total, self.max_faces)
            crops, q = ctx.empty((rows, 112, 112, 3), np.uint8), ctx.empty((rows, 512), np.float16)
            measures = None
            if self.measured_quality:                         # M of one run; stats / measure of the whole chunk, filled run by run
                Mm = ctx.empty((rows, 6), np.float64)
                measures = (ctx.empty((total, 8), np.int64), ctx.empty((total, 8), np.float32))
            for r0 in range(0, total, self.max_faces):
                n = min(self.max_faces, total - r0)
                src_n = C.c_void_p(src.ptr + 4 * r0)
                M_n = C.c_void_p(Mm.ptr) if measures is not None else None
                if mixed:
                    check(lib.fid_align_crops_packed_ragged(ctx.handle, *batch.args(), B, C.c_void_p(post.kps.ptr), post.cap, src_n, n,
                                                            C.c_void_p(crops.ptr), M_n))
                else:
                    check(lib.fid_align_crops_packed(ctx.handle, C.c_void_p(fr.ptr), B, H, W, C.c_void_p(post.kps.ptr), post.cap, src_n, n,
                                                     C.c_void_p(crops.ptr), M_n))
                if measures is not None:                      # the crop buffer is reused per run: measure it before the next warp
                    check(lib.fid_face_measure(ctx.handle, C.c_void_p(crops.ptr), n, C.c_void_p(post.kps.ptr), src_n, M_n,
                                               C.c_void_p(measures[0].ptr + 64 * r0), C.c_void_p(measures[1].ptr + 32 * r0)))
                net.run_device(crops, n)
                emb_ptr, _, _ = net.tensor(net.low.outputs[0])
                check(lib.fid_l2_normalize_f16_packed(ctx.handle, C.c_void_p(emb_ptr), n, 512, src_n, C.c_void_p(q.ptr)))
                emb[r0:r0 + n] = net.read(net.low.outputs[0], n).reshape(n, 512)
                normed[r0:r0 + n] = q.download()[:n].astype(np.float32)
            F = max(len(d) for d, _ in dets)
            quality, side_score, side_flag, best = face_gates(ctx, post.det, post.kps, post.counts, B, post.cap, F, self.gate_config,
                                                              measures=measures, offsets=offsets if measures is not None else None,
                                                              measure_config=self.measure_config)
            bests += [(int(i), int(v)) for i, v in best]
            off = offsets.download()
            md = measured_dicts(measures[0].download(), measures[1].download()) if measures is not None else None
            for b, (det, kpss) in enumerate(dets):
                r = int(off[b])
                out.append([Face(bbox=det[i, :4].copy(), det_score=float(det[i, 4]), kps=kpss[i].copy(), embedding=emb[r + i].copy(),
                                 normed_embedding=normed[r + i].copy(), quality={k: float(quality[b, i, j]) for j, k in enumerate(QUALITY_KEYS)},
                                 is_side_face=bool(side_flag[b, i]), side_face_score=int(side_score[b, i])) for i in range(len(det))])
                if md is not None:
                    for i, f in enumerate(out[-1]):
                        f["measured"] = md[r + i]
        self.last_batch_best = bests
        return out

    def cluster_faces(self, images, similarity_threshold: float = 0.45, min_samples: int = 2, max_num: int = 0):
        """Which faces of these images are the same person: get_batch(images, max_num), every face's embedding into a temporary VectorGallery
        under the id (image index, face index), then VectorGallery.cluster.  Host glue only.  -> engine.ClusterResult keyed by those pairs;
        the answer does not depend on the order of the images beyond the names of the labels.  The default threshold is the reference's
        `grouping_threshold`; it is UNCALIBRATED for clustering (calibrate_faces / VectorGallery.score_distribution measure labelled faces)."""
        from .engine import VectorGallery
        faces = self.get_batch(images, max_num)
        ids = [(b, i) for b, fs in enumerate(faces) for i in range(len(fs))]
        store = VectorGallery(self.ctx, 512, capacity=max(128, len(ids)))
        try:
            if ids:
                store.upsert(ids, np.stack([faces[b][i]["embedding"] for b, i in ids]))
            return store.cluster(similarity_threshold, min_samples)
        finally:
            store._gal.close()

    def calibrate_faces(self, images, labels, bins: int = 512):
        """The genuine / impostor score distributions of a labelled set of images: get_batch(images, max_num=1), the one face of image b into a
        temporary VectorGallery under the id b with the person labels[b] (None = unlabelled), then VectorGallery.score_distribution.  Host
        glue only.  An image without a face is in no pair: its index is not among the ids of the result.  -> engine.ScoreDistribution keyed
        by image index."""
        from .engine import VectorGallery
        if len(labels) != len(images):
            raise ValueError(f"calibrate_faces: {len(labels)} labels for {len(images)} images")
        faces = self.get_batch(images, max_num=1)
        ids = [b for b, fs in enumerate(faces) if len(fs)]
        store = VectorGallery(self.ctx, 512, capacity=max(128, len(ids)))
        try:
            if ids:
                store.upsert(ids, np.stack([faces[b][0]["embedding"] for b in ids]))
            return store.score_distribution({b: labels[b] for b in ids}, bins)
        finally:
            store._gal.close()

    def enroll_faces(self, images, labels, min_score=None, weights=None):
        """One gallery row per person from a labelled set of images: get_batch(images, max_num=1), the one face of image b into a temporary
        VectorGallery under the id b with the person labels[b] (None = unlabelled), then VectorGallery.enroll_templates into a NEW store keyed
        by person.  Host glue only, shaped like calibrate_faces.  An image without a face takes no part.  weights: None, or the quality in
        [0, 1] of every image; min_score: None (the default) drops no face -- no value has been measured, calibrate_faces is the tool to
        choose one with.  -> (VectorGallery of the persons, engine.TemplateResult keyed by image index); the caller closes the store."""
        from .engine import VectorGallery
        if len(labels) != len(images) or (weights is not None and len(weights) != len(images)):
            raise ValueError(f"enroll_faces: {len(labels)} labels / {None if weights is None else len(weights)} weights for {len(images)} images")
        faces = self.get_batch(images, max_num=1)
        ids = [b for b, fs in enumerate(faces) if len(fs)]
        store = VectorGallery(self.ctx, 512, capacity=max(128, len(ids)))
        persons = VectorGallery(self.ctx, 512, capacity=max(128, len({labels[b] for b in ids if labels[b] is not None})))
        try:
            if ids:
                store.upsert(ids, np.stack([faces[b][0]["embedding"] for b in ids]))
            res = store.enroll_templates({b: labels[b] for b in ids}, persons, None if weights is None else {b: weights[b] for b in ids}, min_score)
        except Exception:
            persons._gal.close()
            raise
        finally:
            store._gal.close()
        return persons, res

    def process_visits(self, images, store, **thresholds):
        """The reference's process_visit_data (smart_face_recognition.py:1721-2005) for a list of images (sizes may differ), one visit each, in
        order: best face and its gates per image (the batch form of best_face, :1473-1519, through get_batch), then `store.group_visits` on the
        accepted embeddings -- a rejected image is a "no face" visit (:1796-1801).  thresholds: group_visits' duplicate_threshold /
        grouping_threshold / similarity_threshold (and via).  -> (records, counters): group_visits' record per image plus "gate" (one of
        VERDICTS), and the reference's counter dict (engine.visit_counters, :1772-1781)."""
        from .engine import visit_counters
        faces = self.get_batch(images)
        emb = np.zeros((len(faces), 512), np.float32)
        for b, (idx, verdict) in enumerate(self.last_batch_best):
            if verdict == 0 and 0 <= idx < len(faces[b]):
                emb[b] = faces[b][idx]["embedding"]
        records = store.group_visits(emb, **thresholds)
        for r, (_, verdict) in zip(records, self.last_batch_best):
            r["gate"] = VERDICTS[verdict]
        return records, visit_counters(records)

    def compare_pairs(self, images_a, images_b, threshold: float = 0.4, labels=None, return_embeddings: bool = False):
        """The reference's compare_face_images (smart_face_recognition.py:878-963) for P image pairs: pair p = (images_a[p], images_b[p]); an
        image may be None (its download failed, :896) and the images may differ in size.  Per chunk of `min(det max_batch, max_faces) // 2`
        pairs -- a chunk holds whole pairs -- the present images run as ONE batch: detect (max_num = 0; the mixed-size path when shapes differ,
        as get_batch chooses), fid_face_pack with max_per_frame = 1 (the first NMS survivor = `faces[0]`, :925-926: only that face is
        aligned and embedded), packed warp, recogniser, then fid_pair_verify on the recogniser's output tensor in place: fp32 cosine (:978),
        strict `> threshold` (:932), error verdicts and counters.  No embedding is downloaded unless `return_embeddings` is set; the chunk's
        detections still are (the detector's own fetch, which also reports a capacity overflow): they tell the host how many rows to embed.
        labels: optional [P] of True / False / None (or 1 / 0 / -1), the API's `approve`.
        -> (results, counters): per pair {"same_person", "confidence", "threshold_used", "error"} (:936-943; "error" is one of the reference's
        two messages or None) -- with return_embeddings also "embedding1" / "embedding2" (float32 [D] or None) and "bbox1" / "bbox2" (the chosen
        face's det row [5] or None) --, and engine.pair_counters' dict."""
        from .engine import PAIR_ERRORS, pair_counters
        from .pipeline import pair_image_table
        sides = (list(images_a), list(images_b))
        P = len(sides[0])
        if len(sides[1]) != P:
            raise ValueError(f"compare_pairs: {P} first images, {len(sides[1])} second images")
        step = min(self.det._max_batch, self.max_faces) // 2
        if step < 1:
            raise ValueError("compare_pairs: the detector's max_batch and max_faces must both be >= 2 (a chunk holds whole pairs)")
        if P == 0:
            return [], pair_counters(np.zeros(8, np.int32))
        sides = tuple([None if im is None else np.ascontiguousarray(im, dtype=np.uint8) for im in s] for s in sides)
        present = tuple([im is not None for im in s] for s in sides)
        ctx, lib = self.ctx, self.ctx.lib
        net = self.rec.session.compiled()
        chunks = [pair_image_table(present[0], present[1], p0, min(p0 + step, P)) for p0 in range(0, P, step)]
        pairs = ctx.to_device(np.concatenate([t for _, t in chunks]))
        lab = None
        if labels is not None:
            lab = np.array([-1 if v is None else int(v) for v in labels], np.int32)
            if lab.shape[0] != P:
                raise ValueError(f"compare_pairs: {lab.shape[0]} labels for {P} pairs")
            lab = ctx.to_device(lab)
        out = ctx.empty((2 * P + 8,), np.int32).zero()        # score [P] | verdict [P] | counters [8]: one download at the end
        offsets, src = ctx.empty((2 * step + 1,), np.int32).zero(), ctx.empty((2 * step,), np.int32)
        crops = ctx.empty((2 * step, 112, 112, 3), np.uint8)
        emb = [[None] * P, [None] * P]
        bbox = [[None] * P, [None] * P]
        for ci, (run, _) in enumerate(chunks):
            p0 = ci * step
            Pc = min(step, P - p0)
            imgs = [sides[side][p] for p, side in run]
            n, total, emb_ptr, dim, dets = len(imgs), 0, None, 512, []
            if n:
                mixed = len({im.shape for im in imgs}) > 1
                if mixed:
                    batch = ctx.image_batch(imgs)
                    dets = self.det._detect_chunk_ragged(imgs, 0, "max", batch)
                else:
                    chunk = np.stack(imgs)
                    fr = ctx.to_device(chunk)                 # one upload: the detector and the warp read the same frames
                    dets = self.det._detect_chunk(chunk, 0, "max", fr)
                post = self.det._postprocessor()
                total = sum(1 for d, _ in dets if len(d))
                check(lib.fid_face_pack(ctx.handle, C.c_void_p(post.counts.ptr), n, post.cap, 1, C.c_void_p(offsets.ptr), C.c_void_p(src.ptr), n))
            if total:
                if mixed:
                    check(lib.fid_align_crops_packed_ragged(ctx.handle, *batch.args(), n, C.c_void_p(post.kps.ptr), post.cap, C.c_void_p(src.ptr),
                                                            total, C.c_void_p(crops.ptr), None))
                else:
                    check(lib.fid_align_crops_packed(ctx.handle, C.c_void_p(fr.ptr), n, chunk.shape[1], chunk.shape[2], C.c_void_p(post.kps.ptr),
                                                     post.cap, C.c_void_p(src.ptr), total, C.c_void_p(crops.ptr), None))
                net.run_device(crops, total)
                emb_ptr, (eh, ew, ec, ecp), dt = net.tensor(net.low.outputs[0])
                if dt != np.float32 or (eh, ew) != (1, 1) or ec != ecp:
                    raise RuntimeError(f"compare_pairs: the recogniser's output {(eh, ew, ec, ecp)} {dt} is not a dense fp32 row per face")
                dim = ecp
            # (a chunk without any face, or without any image, still goes through the entry point: its errors are counted there)
            check(lib.fid_pair_verify(ctx.handle, C.c_void_p(emb_ptr) if total else None, total, dim, C.c_void_p(pairs.ptr + 8 * p0), Pc,
                                      C.c_void_p(offsets.ptr), n, C.c_void_p(lab.ptr + 4 * p0) if lab is not None else None,
                                      C.c_float(threshold), C.c_void_p(out.ptr + 4 * p0), C.c_void_p(out.ptr + 4 * (P + p0)),
                                      C.c_void_p(out.ptr + 8 * P)))
            if return_embeddings and total:
                e = net.read(net.low.outputs[0], total).reshape(total, -1)
                off = offsets.download()
                for i, (p, side) in enumerate(run):
                    if len(dets[i][0]):
                        emb[side][p], bbox[side][p] = e[off[i]].copy(), dets[i][0][0].copy()
        got = out.download()
        score, verdict = got[:P].view(np.float32), got[P:2 * P]
        results = []
        for p in range(P):
            r = {"same_person": bool(verdict[p] == 1), "confidence": float(score[p]), "threshold_used": threshold, "error": PAIR_ERRORS[verdict[p]]}
            if return_embeddings:
                r.update(embedding1=emb[0][p], embedding2=emb[1][p], bbox1=bbox[0][p], bbox2=bbox[1][p])
            results.append(r)
        return results, pair_counters(got[2 * P:])

    def process_face_comparisons(self, records, loader=None, max_comparisons: Optional[int] = None, threshold: float = 0.4):
        """The reference's process_face_comparisons (smart_face_recognition.py:1023-1143) on compare_pairs: records are its comparison records
        (`image1_url`, `image2_url`, `approve` and the metadata keys of :1067-1084; a missing metadata key reads None); loader(url) returns a uint8
        BGR image or None (default: pipeline._read_image on file paths -- fetching from the network is the caller's business).
        -> the summary dict of :1112-1122 (the empty form :1036-1043 for no records); per-record fields as :1067-1084.  The summary's
        `api_matches` / `total_with_api_data` are counted on the host exactly as :1108-1110 do (every record counts, `None == False` is no match);
        the device's labelled / label_matches counters take `approve` equal to True / 1 or False / 0 as a label and anything else as none."""
        from .pipeline import _read_image
        if not records:
            return {"total_comparisons": 0, "processed": 0, "same_person": 0, "different_person": 0, "errors": 0, "results": []}
        records = list(records)
        if max_comparisons and len(records) > max_comparisons:
            records = records[:max_comparisons]
        loader = loader or _read_image

        def load(url):
            im = loader(url) if url is not None else None
            return im if isinstance(im, np.ndarray) and im.ndim == 3 and im.shape[2] == 3 and im.size else None

        approve = [r.get("approve") for r in records]
        res, counters = self.compare_pairs([load(r.get("image1_url")) for r in records], [load(r.get("image2_url")) for r in records], threshold,
                                           labels=[_approve_label(a) for a in approve])
        results = []
        for r, c, v in zip(records, res, approve):
            out = {k: r.get(k) for k in ("comparison_id", "event_id", "branch_id", "created_at", "customer_info", "matched_info")}
            out.update(api_approve=v, our_result=c["same_person"], confidence=c["confidence"], threshold_used=c["threshold_used"],
                       image1_url=r.get("image1_url"), image2_url=r.get("image2_url"), error=c["error"],
                       match_status="SAME" if c["same_person"] else "DIFFERENT", api_vs_our_match=v == c["same_person"],
                       raw_data=r.get("raw_data", {}))
            results.append(out)
        api_matches = sum(1 for r in results if r.get("api_vs_our_match") is True)                                        # :1108-1110
        total_with_api_data = sum(1 for r in results if "api_vs_our_match" in r and r["api_vs_our_match"] is not None)
        return {"total_comparisons": len(records), "processed": len(results), "same_person": counters["same_person"],
                "different_person": counters["different_person"], "errors": counters["errors"],
                "accuracy_vs_api": (api_matches / total_with_api_data * 100) if total_with_api_data > 0 else 0, "api_matches": api_matches,
                "total_with_api_data": total_with_api_data, "results": results}

    def best_face(self, image: np.ndarray) -> Optional[Face]:
        """The reference's enrolment gate (smart_face_recognition.py:1473-1519): the first highest-det_score face, rejected (None, with
        `last_verdict` naming the reason) when its score is below `confidence_threshold`, when it is a side face, or when its overall
        quality is below `min_quality_threshold` -- decided on the device by fid_face_gates."""
        self._best = (-1, 1)
        faces = self.get(image)
        idx, verdict = self._best
        self.last_verdict = VERDICTS[verdict]
        return faces[idx] if verdict == 0 and faces else None
