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

from ._lib import GateConfig, check
from .models import ArcFace, SCRFD

VERDICTS = ("accepted", "no face", "confidence too low", "side face", "quality too low")      # FID_GATE_* (include/faceid.h)
QUALITY_KEYS = ("overall", "blur", "pose", "lighting", "size")


def face_gates(ctx, det_dev, kps_dev, counts_dev, batch: int, cap: int, faces_per_frame: int, config: Optional[GateConfig] = None, pose=None):
    """The reference's quality / side-face gates and best-face selection (smart_face_recognition.py:1145-1216, 1218-1297, 1299-1399,
    1473-1519) for every face of a batch, on the post-process's device arrays (`PostProcessor.det / .kps / .counts`, cap = their
    second dimension).  pose: optional [batch, faces_per_frame, 2] yaw / pitch in radians (0 = not available), handed over as float64.
    -> quality [batch, F, 5] (QUALITY_KEYS), side score [batch, F], side flag [batch, F] (bool), best [batch, 2] = (face index or -1, verdict)"""
    cfg = config or GateConfig()
    F = faces_per_frame
    quality = ctx.empty((batch, F, 5), np.float32)
    side = ctx.empty((batch, F), np.int32)
    best = ctx.empty((batch, 2), np.int32)
    pose_dev = ctx.to_device(np.ascontiguousarray(pose, dtype=np.float64).reshape(batch, F, 2)) if pose is not None else None   # (float64 across the boundary: python floats in the reference)
    check(ctx.lib.fid_face_gates(ctx.handle, C.c_void_p(det_dev.ptr), C.c_void_p(kps_dev.ptr), C.c_void_p(counts_dev.ptr), batch, cap, F,
                                 C.c_void_p(pose_dev.ptr) if pose_dev is not None else None, C.byref(cfg), C.c_void_p(quality.ptr),
                                 C.c_void_p(side.ptr), C.c_void_p(best.ptr)))
    sd = side.download()
    return quality.download(), sd & 0xFFFF, (sd >> 16).astype(bool), best.download()


class Face(dict):
    """dict with attribute access, like insightface's Face"""
    __getattr__ = dict.get

    @property
    def embedding_norm(self):
        return float(np.linalg.norm(self["embedding"])) if self.get("embedding") is not None else None


class FaceAnalysis:
    def __init__(self, det_model: str = "synthetic:scrfd_10g", rec_model: str = "synthetic:arcface_r50", *, device: int = 0,
                 det_size=(640, 640), det_thresh: float = 0.5, max_faces: int = 64, gate_config: Optional[GateConfig] = None):
        self.det = SCRFD(det_model, input_size=det_size, conf_thres=det_thresh, device=device)
        self.rec = ArcFace(rec_model, device=device, ctx=self.det.ctx, max_batch=max_faces)
        self.ctx = self.det.ctx
        self.max_faces = int(max_faces)
        self.gate_config = gate_config or GateConfig()       # the reference's config.json thresholds (GateConfig.from_reference_json)
        self.last_verdict = None                              # of the last best_face(): one of VERDICTS
        self.last_batch_best = []                             # of the last get_batch(): per image (best face index, FID_GATE_* verdict)

    def prepare(self, ctx_id: int = 0, det_size=(640, 640), det_thresh: Optional[float] = None):
        """insightface API compatibility (smart_face_recognition.py:358)"""
        self.det.input_size = det_size
        if det_thresh is not None:
            self.det.conf_thres = det_thresh

    def get(self, image: np.ndarray, max_num: int = 0) -> List[Face]:
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
        check(ctx.lib.fid_align_crops(ctx.handle, C.c_void_p(fr.ptr), 1, H, W, C.c_void_p(kp.ptr), C.c_void_p(cn.ptr), n, n,
                                      C.c_void_p(crops.ptr), None))
        net = self.rec.session.compiled()
        net.run_device(crops, n)
        emb_ptr, _, _ = net.tensor(net.low.outputs[0])
        q = ctx.empty((n, 512), np.float16)
        check(ctx.lib.fid_l2_normalize_f16(ctx.handle, C.c_void_p(emb_ptr), n, 512, C.c_void_p(q.ptr)))
        emb = net.read(net.low.outputs[0], n).reshape(n, 512)
        normed = q.download().astype(np.float32)
        # quality scores, side-face flag and the best-face verdict of the reference's product layer, all faces in one launch
        dd = ctx.to_device(np.ascontiguousarray(det[:n], dtype=np.float32).reshape(1, n, 5))
        quality, side_score, side_flag, best = face_gates(ctx, dd, kp, cn, 1, n, n, self.gate_config)
        self._best = (int(best[0, 0]), int(best[0, 1]))
        return [Face(bbox=det[i, :4].copy(), det_score=float(det[i, 4]), kps=kpss[i].copy(), embedding=emb[i].copy(),
                     normed_embedding=normed[i].copy(), quality={k: float(quality[0, i, j]) for j, k in enumerate(QUALITY_KEYS)},
                     is_side_face=bool(side_flag[0, i]), side_face_score=int(side_score[0, i])) for i in range(n)]

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
        step = self.det._max_batch
        for b0 in range(0, len(images), step):
            chunk = images[b0:b0 + step]
            B = len(chunk)
            batch = ctx.image_batch(chunk) if mixed else None
            dets = (self.det._detect_chunk_ragged(chunk, max_num, "max", batch) if mixed
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
            for r0 in range(0, total, self.max_faces):
                n = min(self.max_faces, total - r0)
                src_n = C.c_void_p(src.ptr + 4 * r0)
                if mixed:
                    check(lib.fid_align_crops_packed_ragged(ctx.handle, *batch.args(), B, C.c_void_p(post.kps.ptr), post.cap, src_n, n,
                                                            C.c_void_p(crops.ptr), None))
                else:
                    check(lib.fid_align_crops_packed(ctx.handle, C.c_void_p(fr.ptr), B, H, W, C.c_void_p(post.kps.ptr), post.cap, src_n, n,
                                                     C.c_void_p(crops.ptr), None))
                net.run_device(crops, n)
                emb_ptr, _, _ = net.tensor(net.low.outputs[0])
                check(lib.fid_l2_normalize_f16_packed(ctx.handle, C.c_void_p(emb_ptr), n, 512, src_n, C.c_void_p(q.ptr)))
                emb[r0:r0 + n] = net.read(net.low.outputs[0], n).reshape(n, 512)
                normed[r0:r0 + n] = q.download()[:n].astype(np.float32)
            F = max(len(d) for d, _ in dets)
            quality, side_score, side_flag, best = face_gates(ctx, post.det, post.kps, post.counts, B, post.cap, F, self.gate_config)
            bests += [(int(i), int(v)) for i, v in best]
            off = offsets.download()
            for b, (det, kpss) in enumerate(dets):
                r = int(off[b])
                out.append([Face(bbox=det[i, :4].copy(), det_score=float(det[i, 4]), kps=kpss[i].copy(), embedding=emb[r + i].copy(),
                                 normed_embedding=normed[r + i].copy(), quality={k: float(quality[b, i, j]) for j, k in enumerate(QUALITY_KEYS)},
                                 is_side_face=bool(side_flag[b, i]), side_face_score=int(side_score[b, i])) for i in range(len(det))])
        self.last_batch_best = bests
        return out

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

    def best_face(self, image: np.ndarray) -> Optional[Face]:
        """The reference's enrolment gate (smart_face_recognition.py:1473-1519): the first highest-det_score face, rejected (None, with
        `last_verdict` naming the reason) when its score is below `confidence_threshold`, when it is a side face, or when its overall
        quality is below `min_quality_threshold` -- decided on the device by fid_face_gates."""
        self._best = (-1, 1)
        faces = self.get(image)
        idx, verdict = self._best
        self.last_verdict = VERDICTS[verdict]
        return faces[idx] if verdict == 0 and faces else None
