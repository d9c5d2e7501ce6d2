"""Batched det -> align -> embed -> match harness: the logic of reference main.py `build_targets`
(:78-105) and `frame_processor` (:108-150) for a whole batch of frames, with every stage on the
device and no host round trip between stages.

Per step (one batch of B frames, F = max faces kept per frame = the reference's --max-num):

  frames u8 [B,H,W,3] --(letterbox if needed)--> SCRFD net --> post-process (top-F per frame)
       --> align (Umeyama + warp, B*F crops) --> ArcFace net --> L2-normalise (fp16 [B*F,512])
       --> [multi-GPU: ONE all-gather of the per-rank unit embeddings over RCCL/xGMI]
       --> cosine GEMM + arg-max against the gallery  --> (index, score) per face slot

Multi-GPU: frames shard by rank (independent units), weights and gallery are replicated, the only
collective is the embedding all-gather (BASELINE.json north_star).  `FacePipeline` itself is
single-device; `run_step_distributed` adds the collective through torch.distributed
(backend "nccl" = RCCL on ROCm, "gloo" in the CPU tests).

`PackedFacePipeline` is the same path on a dense face list: every detected face of the batch is one row
(the reference's default max_num = 0), sum-of-faces rows instead of B * F slots."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import Context, check
from .engine import CompiledNet, Gallery, HeadViews, PostProcessor


def shard_range(n_items: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous block partition of frames over ranks: rank r gets
    [r*n/world, (r+1)*n/world)."""
    return (rank * n_items) // world, ((rank + 1) * n_items) // world


def tile_origins(L: int, n: int, overlap: int) -> List[Tuple[int, int]]:
    """(origin, extent) of the tiles along one axis of length L for input length n: L <= n -> the single tile (0, L); else origins
    0, step, 2*step ... (step = n - overlap) while origin + n < L, then a last origin L - n, flush with the far edge; extent n."""
    L, n, overlap = int(L), int(n), int(overlap)
    if L <= n:
        return [(0, L)]
    step = n - overlap
    if overlap < 0 or step <= 0:
        raise ValueError(f"tile_plan: overlap {overlap} must lie in [0, {n})")
    out, x = [], 0
    while x + n < L:
        out.append((x, n))
        x += step
    out.append((L - n, n))
    return out


def tile_plan(H: int, W: int, in_hw, overlap: int = 128, overview: bool = True, batch: int = 1) -> np.ndarray:
    """The tile table of tiled detection (fid_tile_cut / fid_scrfd_postprocess_tiled, include/faceid.h): int32 [T,6], one row
    `frame, x0, y0, w, h, kind` per tile, for `batch` frames of H x W and a detector input in_hw = (in_h, in_w).

    Per frame: the native tiles (kind 0) are the cross product of `tile_origins` along y and x, y-major -- no tile leaves the frame and the
    last one of an axis is flush with its far edge --; with `overview` one letterboxed tile (kind 1) that covers the whole frame comes
    last.  A frame that fits the input (H <= in_h and W <= in_w) gets only that overview row, whatever `overview` says: the untiled path.
    1920x1080 into 640x640 at overlap 128: x origins [0, 512, 1024, 1280], y origins [0, 440], 8 + 1 tiles; 3840x2160: 8 x 4 + 1 = 33.

    Guarantee: along an axis longer than the input, every integer interval of length s <= overlap - 2 * margin lies inside some tile with
    `margin` pixels to spare on every interior side of that tile (a side on the frame's boundary needs no spare).  So with the edge rule at
    `edge_margin = margin`, a face up to overlap - 2 * margin pixels wide and high is found whole by a native tile wherever it stands;
    larger faces are the overview tile's job."""
    in_h, in_w = int(in_hw[0]), int(in_hw[1])
    H, W, batch = int(H), int(W), int(batch)
    if H <= 0 or W <= 0 or batch <= 0:
        raise ValueError(f"tile_plan: bad frame size {W}x{H} or batch {batch}")
    rows = []
    if H > in_h or W > in_w:
        ys, xs = tile_origins(H, in_h, overlap), tile_origins(W, in_w, overlap)
        rows = [(x0, y0, w, h, 0) for y0, h in ys for x0, w in xs]
    if overview or not rows:
        rows.append((0, 0, W, H, 1))
    return np.array([(b,) + r for b in range(batch) for r in rows], dtype=np.int32).reshape(-1, 6)


def frame_reader(name: str, frames, H: int, W: int):
    """The entry point that reads `frames` and its leading arguments: BGR frames (a device buffer uint8 [B,H,W,3]) -> (name, (frames_dev,));
    _lib.Nv12Frames -> (name + "_nv12", (nv12_dev, desc)), the twin that converts every tap on the fly and writes the same bytes."""
    if isinstance(frames, _lib.Nv12Frames):
        if (frames.H, frames.W) != (int(H), int(W)):
            raise ValueError(f"Nv12Frames of {frames.W}x{frames.H} passed as {W}x{H}")
        return name + "_nv12", frames.args()
    return name, (_lib._ptr(frames),)


class FacePipeline:
    """frames_dev of detect / embed / run_step / draw: BGR uint8 [B,H,W,3] on the device, or _lib.Nv12Frames (a decoder's NV12 frames as they
    are: the letterbox, the tile cut and the warp convert each tap, fid_*_nv12; no BGR frame is built, and every result is the one the BGR
    path gives on fid_nv12_to_bgr of the same frames)."""

    def __init__(self, ctx: Context, det: CompiledNet, rec: CompiledNet, *, batch: int, faces_per_frame: int = 1,
                 conf_thres: float = 0.5, iou_thres: float = 0.4, metric: int = 0, det_cap: int = 256,
                 q_buffer=None, tiling=None):
        assert rec.max_batch >= batch * faces_per_frame and det.max_batch >= batch
        self.ctx, self.det, self.rec = ctx, det, rec
        self.B, self.F = int(batch), int(faces_per_frame)
        self.conf, self.iou, self.metric = float(conf_thres), float(iou_thres), int(metric)
        self.in_hw = det.in_hw
        self.post = PostProcessor(det.ctx, batch, cap=det_cap)     # (the detector may live on another context / stream than the recogniser: the whole detect stage runs there)
        self.n_slots = self.B * self.F
        self.crops = ctx.empty((self.n_slots, 112, 112, 3), np.uint8)
        self.emb_dim = 512
        # unit embeddings: caller may supply the device buffer (e.g. a torch tensor for the all-gather)
        self.q = q_buffer if q_buffer is not None else ctx.empty((self.n_slots, self.emb_dim), np.float16)
        self.idx = ctx.empty((self.n_slots,), np.int32)
        self.score = ctx.empty((self.n_slots,), np.float32)
        self._det_in = None
        self._hv: Optional[HeadViews] = None
        self.bgr = None                                        # draw()'s BGR frames when the input is NV12
        self.nv12_out, self.nv12_standard = None, "bt601"      # draw(out="nv12")'s NV12 frames when the input is BGR, and their standard
        self._set_tiling(tiling)

    def _set_tiling(self, tiling):
        """tiling: None (every frame is letterboxed whole), or a dict / object with `overlap`, `edge_margin` and `overview` (defaults
        128, 8, True): detect() cuts every frame into tile_plan's tiles, runs the detector ONCE over the B * tiles-per-frame tiles
        (det.max_batch must hold them: splitting a step is the caller's choice of B) and merges them per frame on the device."""
        if tiling is not None:
            get = tiling.get if isinstance(tiling, dict) else (lambda k, d: getattr(tiling, k, d))
            tiling = dict(overlap=int(get("overlap", 128)), edge_margin=int(get("edge_margin", 8)), overview=bool(get("overview", True)))
        self.tiling = tiling
        self._tile_plans = {}                                  # (H, W) -> tile table
        self._tile_buf = None

    # -- stages ---------------------------------------------------------------------------------
    def _detect_tiled(self, frames_dev, H, W):
        ctx, (in_h, in_w) = self.det.ctx, self.in_hw
        tiles = self._tile_plans.get((H, W))
        if tiles is None:
            tiles = self._tile_plans[(H, W)] = tile_plan(H, W, self.in_hw, self.tiling["overlap"], self.tiling["overview"], self.B)
        T = len(tiles)
        assert self.det.max_batch >= T, f"tiling: {T} tiles per step exceed the detector's max_batch {self.det.max_batch}"
        if self._tile_buf is None or self._tile_buf.shape[0] < T:
            self._tile_buf = ctx.empty((T, in_h, in_w, 3), np.uint8)
        fn, lead = frame_reader("fid_tile_cut", frames_dev, H, W)
        check(getattr(ctx.lib, fn)(ctx.handle, *lead, self.B, H, W, tiles.ctypes.data_as(_lib.c_i32_p), T,
                                   C.c_void_p(self._tile_buf.ptr), in_h, in_w))
        self.det.run_device(self._tile_buf, T)
        if self._hv is None:
            self._hv = HeadViews.from_fused(self.det)
        self.post.run_tiled(self._hv, tiles, self.B, self.in_hw, (H, W), self.conf, self.iou, self.tiling["edge_margin"], self.F, self.metric)

    def detect(self, frames_dev, H, W):
        if self.tiling is not None:
            return self._detect_tiled(frames_dev, H, W)
        in_h, in_w = self.in_hw
        fn, lead = frame_reader("fid_letterbox", frames_dev, H, W)
        if (H, W) == (in_h, in_w) and fn == "fid_letterbox":
            det_in = frames_dev
        else:                                                 # (NV12 frames of the detector's own size: the letterbox's identity path converts them)
            if self._det_in is None:
                self._det_in = self.det.ctx.empty((self.B, in_h, in_w, 3), np.uint8)
            sc = C.c_double()
            check(getattr(self.det.ctx.lib, fn)(self.det.ctx.handle, *lead, self.B, H, W,
                                                C.c_void_p(self._det_in.ptr), in_h, in_w, C.byref(sc)))
            det_in = self._det_in
        self.det.run_device(det_in, self.B)
        if self._hv is None:
            self._hv = HeadViews.from_fused(self.det)
        self.post.run(self._hv, self.B, self.in_hw, (H, W), self.conf, self.iou, self.F, self.metric)

    def embed(self, frames_dev, H, W):
        fn, lead = frame_reader("fid_align_crops", frames_dev, H, W)
        check(getattr(self.ctx.lib, fn)(self.ctx.handle, *lead, self.B, H, W,
                                        C.c_void_p(self.post.kps.ptr), C.c_void_p(self.post.counts.ptr),
                                        self.post.cap, self.F, C.c_void_p(self.crops.ptr), None))
        self.rec.run_device(self.crops, self.n_slots)
        emb_ptr, _, _ = self.rec.tensor(self.rec.low.outputs[0])
        # empty face slots (f >= counts[b]) become zero rows marked by -0.0 in element 0: they never match, and the matrix the all-gather
        # moves tells every rank which slots of the other ranks hold faces (gathered_face_counts)
        check(self.ctx.lib.fid_l2_normalize_f16_slots(self.ctx.handle, C.c_void_p(emb_ptr), self.n_slots, self.emb_dim,
                                                      C.c_void_p(self.post.counts.ptr), self.F, _lib._ptr(self.q)))

    def match(self, gallery: Gallery, thresh: float, q=None, n=None, idx=None, score=None):
        gallery.match_device(self.q if q is None else q, self.n_slots if n is None else n, thresh,
                             self.idx if idx is None else idx, self.score if score is None else score)

    def match_keys(self, gallery: Gallery, q, n, first_row, keys):
        """this rank's shard of a row-sharded gallery: one packed (score, global index) key per query"""
        check(self.ctx.lib.fid_match_keys(self.ctx.handle, gallery.handle, _lib._ptr(q), int(n), int(first_row), _lib._ptr(keys)))

    def match_merge(self, keys_all, parts, n, gallery_total, thresh, idx, score):
        check(self.ctx.lib.fid_match_merge(self.ctx.handle, _lib._ptr(keys_all), int(parts), int(n), int(gallery_total),
                                           float(thresh), _lib._ptr(idx), _lib._ptr(score)))

    def topk_keys(self, gallery: Gallery, q, n, k, first_row, keys):
        """this rank's shard of a row-sharded gallery: the k best packed keys per query, keys [n, k] uint64, descending, 0 = no candidate"""
        check(self.ctx.lib.fid_topk_keys(self.ctx.handle, gallery.handle, _lib._ptr(q), int(n), int(k), int(first_row), _lib._ptr(keys)))

    def topk_merge(self, keys_all, parts, n, k, gallery_total, thresh, idx, score):
        """keys_all [parts, n, k] (the all-gathered shards) -> idx / score [n, k]: the answer of one top-k search over the whole gallery"""
        check(self.ctx.lib.fid_topk_merge(self.ctx.handle, _lib._ptr(keys_all), int(parts), int(n), int(k), int(gallery_total),
                                          float(thresh), _lib._ptr(idx), _lib._ptr(score)))

    def run_step(self, frames_dev, H, W, gallery: Gallery, thresh: float = 0.4):
        """One full pass over one batch; asynchronous (results stay on the device)."""
        if self.det.ctx is not self.ctx:
            # detect() runs on the detector's stream, embed() on this pipeline's: nothing orders the two.  A staged schedule calls
            # detect / embed / match itself and puts its own events between the streams (bench.py --schedule stages).
            raise ValueError("FacePipeline.run_step: the detector lives on another context / stream; call detect(), embed(), match() "
                             "with your own cross-stream events")
        self.detect(frames_dev, H, W)
        self.embed(frames_dev, H, W)
        self.match(gallery, thresh)

    # -- overlay -----------------------------------------------------------------------------------
    @staticmethod
    def _label_handle(labels):
        """a LabelTable, a Gallery (its cached table) or None (no names: every face is drawn as unknown)"""
        if labels is None:
            return None
        if hasattr(labels, "labels"):
            labels = labels.labels()
        return labels.handle

    def _redact(self, frames_dev, H, W, style, idx, score, id_stride, offsets=None, n_rows=0, det=None, counts=None, cap=None):
        """fid_redact_faces / fid_redact_faces_nv12 in place on frames_dev, with the identity arrays of the class's own draw; det / counts /
        cap: another detection table than the post-process's (a coaster's extended one)"""
        det = self.post.det if det is None else det
        counts = self.post.counts if counts is None else counts
        cap = self.post.cap if cap is None else int(cap)
        style = style if style is not None else _lib.RedactStyle()
        if not isinstance(style, _lib.RedactStyle):
            raise TypeError(f"redact: style must be a _lib.RedactStyle, not {type(style).__name__}")
        name, lead = frame_reader("fid_redact_faces", frames_dev, H, W)
        check(getattr(self.ctx.lib, name)(self.ctx.handle, *lead, self.B, int(H), int(W), C.c_void_p(det.ptr), C.c_void_p(counts.ptr), cap,
                                          _lib._ptr(idx), _lib._ptr(score), int(id_stride), _lib._ptr(offsets), int(n_rows), C.byref(style)))
        return frames_dev

    def _draw(self, frames_dev, H, W, labels, style, idx, score, id_stride, offsets=None, n_rows=0, track=None, out=None, redact=None,
              det=None, counts=None, cap=None):
        if out not in (None, "nv12"):
            raise ValueError(f"draw: out must be None or 'nv12', not {out!r}")
        if redact is not None and not isinstance(redact, _lib.RedactStyle):
            raise TypeError(f"draw: redact must be a _lib.RedactStyle or None, not {type(redact).__name__}")
        style = style if style is not None else _lib.DrawStyle()
        tables = dict(det=det, counts=counts, cap=cap)         # (None: the post-process's own)
        det = self.post.det if det is None else det
        counts = self.post.counts if counts is None else counts
        cap = self.post.cap if cap is None else int(cap)
        tail = (self.B, int(H), int(W), C.c_void_p(det.ptr), C.c_void_p(counts.ptr), cap, _lib._ptr(idx),
                _lib._ptr(score), int(id_stride), _lib._ptr(offsets), int(n_rows), _lib._ptr(track), self._label_handle(labels), C.byref(style))
        if isinstance(frames_dev, _lib.Nv12Frames):
            _, lead = frame_reader("fid_nv12_to_bgr", frames_dev, H, W)
            if out == "nv12":                                  # in place on the two planes: no BGR frame anywhere
                if redact is not None:
                    self._redact(frames_dev, H, W, redact, idx, score, id_stride, offsets, n_rows, **tables)
                check(self.ctx.lib.fid_draw_faces_nv12(self.ctx.handle, *lead, *tail))
                return frames_dev
            # a BGR overlay needs BGR pixels: convert into the pipeline's own buffer, draw there
            if self.bgr is None or self.bgr.shape != (self.B, int(H), int(W), 3):
                self.bgr = self.ctx.empty((self.B, int(H), int(W), 3), np.uint8)
            check(self.ctx.lib.fid_nv12_to_bgr(self.ctx.handle, *lead, self.B, int(H), int(W), C.c_void_p(self.bgr.ptr)))
            frames_dev = self.bgr
        if redact is not None:                                 # on the buffer about to be drawn on: boxes and names stay legible on top
            self._redact(frames_dev, H, W, redact, idx, score, id_stride, offsets, n_rows, **tables)
        check(self.ctx.lib.fid_draw_faces(self.ctx.handle, _lib._ptr(frames_dev), *tail))
        if out == "nv12":                                      # BGR frames, drawn in place above: one conversion, half the bytes to download
            if self.nv12_out is None or (self.nv12_out.H, self.nv12_out.W) != (int(H), int(W)):
                self.nv12_out = _lib.Nv12Frames(self.ctx.empty((self.B, int(H) * 3 // 2, int(W)), np.uint8), H, W, standard=self.nv12_standard)
            check(self.ctx.lib.fid_bgr_to_nv12(self.ctx.handle, _lib._ptr(frames_dev), self.B, int(H), int(W), *self.nv12_out.args()))
            return self.nv12_out
        return frames_dev

    def redact(self, frames_dev, H, W, style=None):
        """Redact the last step's faces on frames_dev -- BGR uint8 [B,H,W,3], or the two planes of _lib.Nv12Frames --, in place and on the
        device (fid_redact_faces / fid_redact_faces_nv12): a mosaic or a solid fill over every face `style` (_lib.RedactStyle; default: an
        8-cell mosaic over the faces the match did not name) selects.  A face is known iff its entry of the identity array the class's own
        `draw` uses is >= 0.  Enqueued behind the match; nothing is read back.  Redaction DESTROYS pixels: call it after the step's last
        reader of the clean frames -- the warp (embed), measure and the best-shot crops, all inside run_step -- and before the buffer is
        handed back to an upload.  Returns frames_dev."""
        return self._redact(frames_dev, H, W, style, self.idx, self.score, self.F)

    def draw(self, frames_dev, H, W, labels, style=None, out=None, redact=None):
        """Draw the last step's boxes, names and scores onto frames_dev uint8 [B,H,W,3], in place and on the device (fid_draw_faces): what
        frame_processor does with cv2 per face (main.py:132-148).  Enqueued behind the match; nothing is read back.  Call it after the
        step's last reader of the clean frames (run_step), and before the buffer is handed back to an upload.
        redact: a _lib.RedactStyle: the selected faces are redacted (`redact`) on the buffer that is about to be drawn on, immediately
        before the overlay, so that boxes and names stay legible on top of the mosaic -- on `self.bgr` for _lib.Nv12Frames with out=None
        (the input stays untouched), in place on the planes with out="nv12", on the BGR frames before their conversion otherwise.  The same
        ordering rule holds, the more so: redaction destroys pixels, so it runs after the step's last reader of the clean frames (the
        warp, measure, the best-shot crops).
        labels: a LabelTable, a Gallery, or None; style: _lib.DrawStyle (default: the reference's look).
        out=None returns the BGR buffer that was drawn on: frames_dev itself, or -- for _lib.Nv12Frames, which are left untouched -- the
        pipeline's own BGR buffer `self.bgr` [B,H,W,3], filled by fid_nv12_to_bgr just before (overwritten by the next draw).
        out="nv12" returns _lib.Nv12Frames, what an encoder takes: _lib.Nv12Frames are drawn IN PLACE on their two planes
        (fid_draw_faces_nv12; no BGR buffer is allocated) and returned; BGR frames are drawn in place as before and then converted once
        (fid_bgr_to_nv12, standard `self.nv12_standard`) into the pipeline's own dense buffer `self.nv12_out` (overwritten by the next
        draw; H and W even)."""
        return self._draw(frames_dev, H, W, labels, style, self.idx, self.score, self.F, out=out, redact=redact)

    # -- results -----------------------------------------------------------------------------------
    def results(self, gallery: Gallery):
        """Host view of the last step: per frame a list of (bbox[4], det_score, kps[5,2], name, similarity)
        -- what frame_processor draws (main.py:132-148)."""
        self.post.check()
        counts = self.post.counts.download()
        det = self.post.det.download()
        kps = self.post.kps.download()
        idx = self.idx.download().reshape(self.B, self.F)
        score = self.score.download().reshape(self.B, self.F)
        out = []
        for b in range(self.B):
            faces = []
            for f in range(min(int(counts[b]), self.F)):
                j = int(idx[b, f])
                faces.append((det[b, f, :4].copy(), float(det[b, f, 4]), kps[b, f].reshape(5, 2).copy(),
                              gallery.names[j] if j >= 0 else "Unknown", float(score[b, f])))
            out.append(faces)
        return out

    def embeddings(self) -> np.ndarray:
        """Raw (un-normalised) fp32 embeddings of the last step, [B*F, 512]."""
        return self.rec.read(self.rec.low.outputs[0], self.n_slots).reshape(self.n_slots, -1)


class GroupedFacePipeline(FacePipeline):
    """FacePipeline whose recogniser runs once per `group` consecutive steps (dynamic batching across steps, round 5).

    Every step still detects, post-processes and aligns ITS batch of B frames at once (the frames may be overwritten as soon as
    `run_step` has been enqueued); the B*F crops of the group's steps collect in one buffer and the last step of the group sends all
    group*B*F of them through IResNet, the L2 normalisation and ONE gallery match.  IResNet-50 at 64 crops has one tile per CU on its
    26 stage-3 layers (a launch = one latency chain); at 128 crops it runs at 810 instead of 664 TFLOP/s (profiles/r05/steady.txt): the same
    work per face, 18 % less time.  The price is latency: a step's identities exist when its group's last step has run
    (`flush` finishes a partial group).  Slots of step k of the group: [k*B*F, (k+1)*B*F) of `q`, `idx`, `score`."""

    def __init__(self, ctx: Context, det: CompiledNet, rec: CompiledNet, *, batch: int, faces_per_frame: int = 1, group: int = 2,
                 det_cap: int = 256, **kw):
        assert group >= 1 and rec.max_batch >= group * batch * faces_per_frame
        q_buffer = kw.pop("q_buffer", None)
        super().__init__(ctx, det, rec, batch=batch, faces_per_frame=faces_per_frame, det_cap=det_cap, **kw)
        self.group = int(group)
        self.posts = [self.post] + [PostProcessor(det.ctx, batch, cap=det_cap) for _ in range(self.group - 1)]
        n = self.n_slots
        self.crops = ctx.empty((self.group * n, 112, 112, 3), np.uint8)
        self.q = q_buffer if q_buffer is not None else ctx.empty((self.group * n, self.emb_dim), np.float16)
        self.idx = ctx.empty((self.group * n,), np.int32)
        self.score = ctx.empty((self.group * n,), np.float32)
        self.k = 0                                           # steps of the current group already detected + aligned

    def collect(self, frames_dev, H, W) -> bool:
        """detect + post-process + align one batch into the group's crop buffer; True when the group is full"""
        if self.det.ctx is not self.ctx:
            raise ValueError("GroupedFacePipeline: detector and recogniser must share one context / stream")
        k, n = self.k, self.n_slots
        if k >= self.group:
            raise RuntimeError("GroupedFacePipeline.collect: the group is full -- embed_collected() / flush() it first")
        self.post = self.posts[k]
        self.detect(frames_dev, H, W)
        fn, lead = frame_reader("fid_align_crops", frames_dev, H, W)
        check(getattr(self.ctx.lib, fn)(self.ctx.handle, *lead, self.B, H, W,
                                        C.c_void_p(self.post.kps.ptr), C.c_void_p(self.post.counts.ptr),
                                        self.post.cap, self.F, C.c_void_p(self.crops.ptr + k * n * 112 * 112 * 3), None))
        self.k += 1
        return self.k == self.group

    def run_step(self, frames_dev, H, W, gallery: Gallery, thresh: float = 0.4):
        if self.collect(frames_dev, H, W):
            self.flush(gallery, thresh)

    def embed_collected(self) -> int:
        """IResNet + L2 normalisation of the steps collected so far into q[0 : steps * B * F]; returns steps (0: nothing collected)"""
        steps, n = self.k, self.n_slots
        if steps == 0:
            return 0
        self.rec.run_device(self.crops, steps * n)
        emb_ptr, _, _ = self.rec.tensor(self.rec.low.outputs[0])
        q_ptr = _lib._ptr(self.q).value
        for j in range(steps):
            check(self.ctx.lib.fid_l2_normalize_f16_slots(self.ctx.handle, C.c_void_p(emb_ptr + j * n * self.emb_dim * 4), n, self.emb_dim,
                                                          C.c_void_p(self.posts[j].counts.ptr), self.F,
                                                          C.c_void_p(q_ptr + j * n * self.emb_dim * 2)))
        self.last_steps, self.k = steps, 0
        return steps

    def flush(self, gallery: Gallery, thresh: float = 0.4):
        """embed + match the steps collected so far (a whole group, or what a stream's end left of one)"""
        steps = self.embed_collected()
        if steps:
            self.match(gallery, thresh, n=steps * self.n_slots)

    def redact(self, frames_dev, H, W, style=None):
        """FacePipeline.redact without identities: a step's identities exist only when its group's last step has run, so every face of the
        step counts as unknown (the detections-only form).  A style that selects only known faces would silently redact nobody here and
        is refused."""
        style = style if style is not None else _lib.RedactStyle()
        if isinstance(style, _lib.RedactStyle) and not (style.who & _lib.REDACT_UNKNOWN):
            raise ValueError("GroupedFacePipeline.redact: no identities exist at the step; a style must select REDACT_UNKNOWN")
        return self._redact(frames_dev, H, W, style, None, None, 0)

    def draw(self, frames_dev, H, W, labels, style=None, out=None, redact=None):
        raise ValueError("GroupedFacePipeline.draw: a step's identities exist only when its group's last step has run, after its frames "
                         "may have been overwritten; draw from results() on the host (utils.helpers.draw_faces)")

    def results(self, gallery: Gallery):
        """per step of the last finished group: the list FacePipeline.results returns for one batch"""
        out = []
        idx_all, score_all = self.idx.download(), self.score.download()
        for j in range(getattr(self, "last_steps", 0)):
            post = self.posts[j]
            post.check()
            counts, det, kps = post.counts.download(), post.det.download(), post.kps.download()
            idx = idx_all[j * self.n_slots:(j + 1) * self.n_slots].reshape(self.B, self.F)
            score = score_all[j * self.n_slots:(j + 1) * self.n_slots].reshape(self.B, self.F)
            frames = []
            for b in range(self.B):
                faces = []
                for f in range(min(int(counts[b]), self.F)):
                    i = int(idx[b, f])
                    faces.append((det[b, f, :4].copy(), float(det[b, f, 4]), kps[b, f].reshape(5, 2).copy(),
                                  gallery.names[i] if i >= 0 else "Unknown", float(score[b, f])))
                frames.append(faces)
            out.append(frames)
        return out


def packed_layout(counts, cap: int, max_per_frame: int, row_cap: int) -> Tuple[np.ndarray, np.ndarray]:
    """The packed face layout, stated on the host (what fid_face_pack computes on the device; include/faceid.h).
    k_b = min(max(counts[b], 0), cap) and, when max_per_frame > 0, also min(., max_per_frame).
    -> offsets int32 [B+1]: exclusive prefix sum of k_b, offsets[B] = total faces (NOT clipped to row_cap);
       src int32 [row_cap]: src[i] = b * cap + f of the i-th face in (frame, rank) order for i < min(total, row_cap), -1 after them
       (faces beyond row_cap -- the last ones in that order -- are dropped)."""
    k = np.clip(np.asarray(counts, dtype=np.int64).reshape(-1), 0, int(cap))
    if max_per_frame > 0:
        k = np.minimum(k, int(max_per_frame))
    B = k.shape[0]
    offsets = np.zeros(B + 1, np.int64)
    offsets[1:] = np.cumsum(k)
    n = int(min(offsets[B], row_cap))
    frame = np.repeat(np.arange(B, dtype=np.int64), k)[:n]
    src = np.full(int(row_cap), -1, np.int32)
    src[:n] = frame * int(cap) + (np.arange(n, dtype=np.int64) - offsets[frame])
    return offsets.astype(np.int32), src


def pair_image_table(present_a, present_b, p0: int, p1: int) -> Tuple[List[Tuple[int, int]], np.ndarray]:
    """The images one chunk of a pair list runs, stated on the host (FaceAnalysis.compare_pairs): pairs p0 .. p1 - 1, present_a[p] / present_b[p]
    = "image a / b of pair p exists" (the reference's download succeeded, smart_face_recognition.py:893-896).
    -> run: [(p, side)] (side 0 = a, 1 = b) in the order a_p0, b_p0, a_p0+1 ... with absent images skipped: image i of the chunk's batch;
       table int32 [p1 - p0, 2]: the batch index of each side, -1 for an absent image -- fid_pair_verify's pair table in its image-index form."""
    run: List[Tuple[int, int]] = []
    table = np.full((max(p1 - p0, 0), 2), -1, np.int32)
    for p in range(p0, p1):
        for side, present in enumerate((present_a, present_b)):
            if present[p]:
                table[p - p0, side] = len(run)
                run.append((p, side))
    return run, table


class PackedFacePipeline(FacePipeline):
    """FacePipeline on a dense (packed) face list: EVERY face the detector returns for the batch -- `max_num = 0`, the reference's
    default (main.py:130-134 with models/scrfd.py:159-177), or its top-`max_num` per frame -- is one row of a row table
    (fid_face_pack / packed_layout), and alignment, recogniser, normalisation and match run on those rows instead of on
    B x faces_per_frame slots: a crowded frame no longer sets the price of every frame of the batch.

    row_cap   rows the buffers hold (<= rec.max_batch, <= 65535).  A batch with more faces loses the LAST faces of its last frames
              (`overflow`, read after results(), says how many); a reported face is never wrong.
    rows      "capacity": every step runs row_cap rows; fully asynchronous like FacePipeline.run_step.
              "count":    embed() reads the batch's face total back (4 bytes; this SYNCHRONISES the stream with the host) and runs the
                          smallest entry of `buckets` >= min(total, row_cap) rows; no face at all -> recogniser and match are skipped.
    buckets   ascending row counts ending in row_cap (default: the multiples of 64).  The executor tunes and plans per batch size, so
              the set of sizes it ever sees must be small and fixed; warm() runs each once.
    measure   True: embed() asks the warp for the similarity matrices and measures the rows right behind it on the same stream
              (fid_face_measure: sharpness, exposure, pose); `stats` / `measures` hold [row_cap, 8] on the device, results_measured() reads
              them.  results() is the same either way.
    More survivors than det_cap in one frame is FID_E_CAPACITY from results(), as in FacePipeline.  Rows of q / idx / score at or past
    the rows of the last step (`n_run`) are stale.  Single device: the distributed step and step grouping know nothing of row tables."""

    def __init__(self, ctx: Context, det: CompiledNet, rec: CompiledNet, *, batch: int, row_cap: int, max_num: int = 0,
                 rows: str = "capacity", buckets: Optional[Sequence[int]] = None, conf_thres: float = 0.5, iou_thres: float = 0.4,
                 metric: int = 0, det_cap: int = 256, q_buffer=None, tiling=None, measure: bool = False):
        assert det.max_batch >= batch and rec.max_batch >= row_cap and 0 < row_cap <= 65535 and max_num >= 0
        if rows not in ("capacity", "count"):
            raise ValueError(f"rows must be 'capacity' or 'count', not {rows!r}")
        self.ctx, self.det, self.rec = ctx, det, rec
        self.B, self.F = int(batch), int(max_num)             # F: the max_num detect() hands to the post-process (0 = every survivor)
        self.max_num, self.row_cap, self.rows = int(max_num), int(row_cap), rows
        if buckets is None:
            buckets = list(range(64, self.row_cap, 64)) + [self.row_cap]
        self.buckets = [int(v) for v in buckets]
        assert self.buckets == sorted(set(self.buckets)) and self.buckets[0] > 0 and self.buckets[-1] == self.row_cap, self.buckets
        self.conf, self.iou, self.metric = float(conf_thres), float(iou_thres), int(metric)
        self.in_hw = det.in_hw
        self.post = PostProcessor(det.ctx, batch, cap=det_cap)
        self.n_slots = self.row_cap
        self.emb_dim = 512
        self.offsets = ctx.empty((self.B + 1,), np.int32)
        self.src = ctx.empty((self.row_cap,), np.int32)
        self.crops = ctx.empty((self.row_cap, 112, 112, 3), np.uint8)
        self.q = q_buffer if q_buffer is not None else ctx.empty((self.row_cap, self.emb_dim), np.float16)
        self.idx = ctx.empty((self.row_cap,), np.int32)
        self.score = ctx.empty((self.row_cap,), np.float32)
        self.measure = bool(measure)
        self.M = self.stats = self.measures = None
        if self.measure:
            self.M = ctx.empty((self.row_cap, 6), np.float64)
            self.stats = ctx.empty((self.row_cap, 8), np.int64)
            self.measures = ctx.empty((self.row_cap, 8), np.float32)
        self._det_in = None
        self._hv: Optional[HeadViews] = None
        self.bgr = None
        self.nv12_out, self.nv12_standard = None, "bt601"
        self._set_tiling(tiling)                              # (FacePipeline: detect() tiles every frame when set)
        self.n_run = 0                                        # rows the last embed() ran
        self.rec_steps = 0                                    # recogniser runs so far (a step without a face adds none in rows="count")
        self._overflow = 0

    def _rows_for(self, total: int) -> int:
        need = min(int(total), self.row_cap)
        return 0 if need <= 0 else next(v for v in self.buckets if v >= need)

    def _pack(self):
        """the row table of the last detect(): offsets / src (a subclass may build another table in the same format)"""
        check(self.ctx.lib.fid_face_pack(self.ctx.handle, C.c_void_p(self.post.counts.ptr), self.B, self.post.cap, self.max_num,
                                         C.c_void_p(self.offsets.ptr), C.c_void_p(self.src.ptr), self.row_cap))

    def embed(self, frames_dev, H, W):
        lib, h = self.ctx.lib, self.ctx.handle
        self._pack()
        if self.rows == "count":
            total = int(self.ctx.borrow(self.offsets.ptr + 4 * self.B, (1,), np.int32).download()[0])     # the one read-back: synchronises
            self.n_run = self._rows_for(total)
            if self.n_run == 0:
                return
        else:
            self.n_run = self.row_cap
        n = self.n_run
        fn, lead = frame_reader("fid_align_crops_packed", frames_dev, H, W)
        check(getattr(lib, fn)(h, *lead, self.B, H, W, C.c_void_p(self.post.kps.ptr), self.post.cap,
                               C.c_void_p(self.src.ptr), n, C.c_void_p(self.crops.ptr), C.c_void_p(self.M.ptr) if self.measure else None))
        if self.measure:
            check(lib.fid_face_measure(h, C.c_void_p(self.crops.ptr), n, C.c_void_p(self.post.kps.ptr), C.c_void_p(self.src.ptr),
                                       C.c_void_p(self.M.ptr), C.c_void_p(self.stats.ptr), C.c_void_p(self.measures.ptr)))
        self.rec.run_device(self.crops, n)
        self.rec_steps += 1
        emb_ptr, _, _ = self.rec.tensor(self.rec.low.outputs[0])
        check(lib.fid_l2_normalize_f16_packed(h, C.c_void_p(emb_ptr), n, self.emb_dim, C.c_void_p(self.src.ptr), _lib._ptr(self.q)))

    def match(self, gallery: Gallery, thresh: float, q=None, n=None, idx=None, score=None):
        n = self.n_run if n is None else n
        if n > 0:
            super().match(gallery, thresh, q=q, n=n, idx=idx, score=score)

    def warm(self, frames_dev, H, W, gallery: Optional[Gallery] = None, thresh: float = 0.4):
        """Run the detector once and the recogniser (and the match, given a gallery) once per bucket, so that no later step meets a
        row count the executor has not tuned.  Synchronises."""
        self.detect(frames_dev, H, W)
        lib, h = self.ctx.lib, self.ctx.handle
        PackedFacePipeline._pack(self)                        # (every face, whatever table a subclass's steps build)
        fn, lead = frame_reader("fid_align_crops_packed", frames_dev, H, W)
        for n in (self.buckets if self.rows == "count" else [self.row_cap]):
            check(getattr(lib, fn)(h, *lead, self.B, H, W, C.c_void_p(self.post.kps.ptr), self.post.cap,
                                   C.c_void_p(self.src.ptr), n, C.c_void_p(self.crops.ptr), None))
            self.rec.run_device(self.crops, n)
            emb_ptr, _, _ = self.rec.tensor(self.rec.low.outputs[0])
            check(lib.fid_l2_normalize_f16_packed(h, C.c_void_p(emb_ptr), n, self.emb_dim, C.c_void_p(self.src.ptr), _lib._ptr(self.q)))
            if gallery is not None:
                FacePipeline.match(self, gallery, thresh, n=n)
        self.ctx.sync()

    def redact(self, frames_dev, H, W, style=None):
        """FacePipeline.redact on the row table (the row form, as `draw`): a face without a row is not a face of the call"""
        return self._redact(frames_dev, H, W, style, self.idx, self.score, 0, offsets=self.offsets, n_rows=min(self.n_run, self.row_cap))

    def draw(self, frames_dev, H, W, labels, style=None, out=None, redact=None):
        """FacePipeline.draw on the row table: face f of frame b is row offsets[b] + f; only the rows the last step ran carry an identity"""
        return self._draw(frames_dev, H, W, labels, style, self.idx, self.score, 0, offsets=self.offsets, n_rows=min(self.n_run, self.row_cap),
                          out=out, redact=redact)

    # -- results -----------------------------------------------------------------------------------
    def _download(self):
        """host copies of the last step: counts [B], det [B,cap,5], kps [B,cap,10], idx [row_cap], score [row_cap]"""
        self.post.check()
        return self.post.counts.download(), self.post.det.download(), self.post.kps.download(), self.idx.download(), self.score.download()

    def results(self, gallery: Gallery):
        """Host view of the last step: per frame the list FacePipeline.results gives -- (bbox[4], det_score, kps[5,2], name, similarity)
        in the detector's order -- for ALL faces of the frame that found a row; sets `overflow`."""
        counts, det, kps, idx, score = self._download()
        cap = det.shape[1]
        offsets, src = packed_layout(counts[:self.B], cap, self.max_num, self.row_cap)
        kept = min(int(offsets[self.B]), self.row_cap)
        self._overflow = int(offsets[self.B]) - kept
        out = []
        for b in range(self.B):
            faces = []
            for i in range(int(offsets[b]), min(int(offsets[b + 1]), kept)):
                f = int(src[i]) - b * cap
                j = int(idx[i])
                faces.append((det[b, f, :4].copy(), float(det[b, f, 4]), kps[b, f].reshape(5, 2).copy(),
                              gallery.names[j] if j >= 0 else "Unknown", float(score[i])))
            out.append(faces)
        return out

    def _measured_rows(self):
        """per row of the last step's table a MEASURE_KEYS dict, None for a row that holds no face or was not run"""
        if not self.measure:
            raise RuntimeError("results_measured needs a pipeline built with measure=True")
        n = min(self.n_run, self.row_cap)
        rows = [None] * self.row_cap
        if n > 0:
            stats, meas = self.stats.download()[:n], self.measures.download()[:n]
            for i in range(n):
                if stats[i, 7] & 1:
                    rows[i] = dict(zip(_lib.MEASURE_KEYS, (float(v) for v in meas[i, :7])))
        return rows

    def results_measured(self, gallery: Gallery):
        """(results(gallery), measured): measured[b][f] is the MEASURE_KEYS dict of face f of frame b as results() lists it"""
        res = self.results(gallery)
        rows = self._measured_rows()
        offsets, _ = packed_layout(self.post.counts.download()[:self.B], self.post.cap, self.max_num, self.row_cap)
        return res, [[rows[int(offsets[b]) + f] for f in range(len(res[b]))] for b in range(self.B)]

    @property
    def overflow(self) -> int:
        """faces of the last results() that found no row (batch total - row_cap, 0 if they all fit)"""
        return self._overflow

    def embeddings(self) -> Tuple[np.ndarray, np.ndarray]:
        """Raw (un-normalised) fp32 embeddings of the last step, [faces kept, 512] in row order, and offsets [B+1] (packed_layout:
        frame b owns rows offsets[b] : offsets[b+1], cut at the number of rows returned)."""
        offsets, _ = packed_layout(self.post.counts.download()[:self.B], self.post.cap, self.max_num, self.row_cap)
        kept = min(int(offsets[self.B]), self.row_cap, self.n_run)
        if kept == 0:
            return np.zeros((0, self.emb_dim), np.float32), offsets
        return self.rec.read(self.rec.low.outputs[0], kept).reshape(kept, -1), offsets


class TrackedFacePipeline(PackedFacePipeline):
    """PackedFacePipeline for video: faces are followed from frame to frame on the device (fid_track_step / fid_track_identify,
    include/faceid.h) and only the faces whose track is DUE go through alignment, recogniser and match -- a new track, a track without a
    name every `retry` matches, a named one every `refresh` matches.  Every detection still reports a name: its track's best gallery match
    so far.  A step's B frames are consecutive frames of the video (of several videos: `stream` of run_step); nothing is read back between
    the tracker and the recogniser.

    streams     cameras the tracker keeps apart (run_step's `stream[b]` in [0, streams)).
    max_tracks  slots per stream, 1 .. 64 (default 64: all a wavefront holds; a free slot costs nothing).  A detection that finds no slot
                is embedded and matched on its own every frame, exactly as PackedFacePipeline treats it.
    iou         overlap (the NMS's, with its +1 convention) above which a detection continues a track; 0.3 follows a face that moves up
                to about half its width between two frames and is still below the detector's own NMS threshold 0.4, so two detections
                that survived NMS in one frame rarely compete for one track.
    max_age     frames a track survives without a detection (default 15: half a second at 30 fps bridges a turned head or a passer-by
                without handing the name to the next face that appears in the same place much later).
    refresh     a NAMED track is embedded again every `refresh` matches (default 16: twice a second at 30 fps.  The name only ever
                moves to a better score, so refreshing corrects a wrong first match; it is not needed to keep a right one).
    retry       a track WITHOUT a name is embedded every `retry` matches (default 1: every frame, so an unknown face is never worse
                off than in PackedFacePipeline).
    rows / buckets / row_cap behave as in PackedFacePipeline, on the tracker's table; a due face that finds no row keeps what its track
    knows and asks again after its interval (`overflow`).

    best_shot   True (implies measure=True): match() follows identify() with fid_shot_score and fid_track_keep on the step's rows: of the
                faces a track embeds, the one with the best measured score stays on the device -- unit embedding, aligned crop (keep_crops),
                box, frame number -- and a track that ends becomes ONE finished record: finished() reads the records, group_finished() hands
                their embeddings to a VectorGallery where they lie, finish_all() ends every live track (the end of a video).  An unnamed
                track is embedded every `retry` matches (default: every frame), so the keeper normally sees a stranger's whole passage.
                The tracker still decides WHEN a face is embedded.  `finished_cap`: finished records the device holds between two
                finished() calls (further ones are dropped and counted); `measure_config`: _lib.MeasureConfig, the score's three
                normalisations (UNCALIBRATED defaults).  reset() needs no extra call: the next step's keep finishes what the reset orphaned.
                Off (the default), nothing of this is launched or allocated.

    coast       a _lib.CoastConfig: match() follows identify() (and the keeper) with fid_track_coast: every track that is alive but found no
                detection in a frame is appended to that frame's detections for up to `hold` frames -- at its last box, moved along its
                last velocity (`predict`) and grown by `grow` per missed frame -- with its track's name.  redact() and draw() then work on
                the extended tables [B, cap + max_tracks]: a redaction does not flicker off in the frames where the detector missed the
                face, a named person stays in the clear, and the overlay shows the held box with the track's name and id.  hold > max_age
                is a ValueError: the tracker has freed the track by then.  results() / results_tracked() are unchanged -- a coasted box is
                not a detection --; results_coasted() lists the coasted entries.  The config's defaults are UNCALIBRATED.  None (the
                default): nothing of this is launched or allocated.

    relink      a _lib.RelinkConfig: match() follows identify() with fid_track_relink on the step's unit rows (also with gallery=None): the
                relinker keeps every live track's latest embedding and, per stream, a pool of `pool` recently ended tracks for `window`
                frames; a new track whose first embedding scores above `thresh` against a pooled one inherits that track's PERSON ID (the
                id of the first track of the chain).  results_persons() adds (person id, relinked) to results_tracked()'s tuples,
                relinker_state() reads the tables, and draw() with DRAW_TRACK_ID prints the person id in place of the track id, so the
                drawn number stays when a stranger returns.  With a coaster the extended table keeps TRACK ids: mapping held boxes to
                persons is out of scope.  results() / results_tracked() are unchanged.  Only a track that has ENDED can be linked to: use
                a short max_age with the relinker.  The config's defaults are UNCALIBRATED.  None (the default): nothing of this is
                launched or allocated."""

    def __init__(self, ctx: Context, det: CompiledNet, rec: CompiledNet, *, batch: int, row_cap: int, streams: int = 1, max_tracks: int = 64,
                 iou: float = 0.3, max_age: int = 15, refresh: int = 16, retry: int = 1, best_shot: bool = False, finished_cap: int = 256,
                 keep_crops: bool = True, measure_config=None, coast=None, relink=None, **kw):
        if relink is not None and not isinstance(relink, _lib.RelinkConfig):
            raise TypeError(f"TrackedFacePipeline: relink must be a _lib.RelinkConfig or None, not {type(relink).__name__}")
        if coast is not None:
            if not isinstance(coast, _lib.CoastConfig):
                raise TypeError(f"TrackedFacePipeline: coast must be a _lib.CoastConfig or None, not {type(coast).__name__}")
            if coast.hold > int(max_age):
                raise ValueError(f"TrackedFacePipeline: coast.hold = {coast.hold} exceeds max_age = {int(max_age)}: the tracker frees a track "
                                 "after max_age missed frames, there is nothing left to hold")
        self.best_shot = bool(best_shot)
        if self.best_shot:
            kw["measure"] = True
        super().__init__(ctx, det, rec, batch=batch, row_cap=row_cap, **kw)
        if det.ctx is not ctx:
            raise ValueError("TrackedFacePipeline: detector and recogniser must share one context / stream")
        self.streams = int(streams)
        self.cfg = _lib.TrackConfig(float(iou), int(max_age), int(refresh), int(retry))
        h = C.c_void_p()
        check(ctx.lib.fid_tracker_create(ctx.handle, self.streams, int(max_tracks), C.byref(h)))
        self.tracker, self.max_tracks = h, int(max_tracks)
        cap = self.post.cap
        self.track = ctx.empty((self.B, cap, 2), np.int32)
        self.ident_idx = ctx.empty((self.B, cap), np.int32)
        self.ident_score = ctx.empty((self.B, cap), np.float32)
        self._stream = np.zeros(self.B, np.int32)
        self._identified = True                               # no step is waiting for its identify()
        self.shots, self.finished_dropped, self._names = None, 0, None
        if self.best_shot:
            self.mcfg = measure_config if measure_config is not None else _lib.MeasureConfig()
            self.finished_cap, self.keep_crops = int(finished_cap), bool(keep_crops)
            h = C.c_void_p()
            check(ctx.lib.fid_shots_create(ctx.handle, self.streams, self.max_tracks, self.emb_dim, self.finished_cap, int(self.keep_crops),
                                           C.byref(h)))
            self.shots = h
            self.shot_score = ctx.empty((self.row_cap,), np.float32)
        self.coast, self.coaster, self._coasted = coast, None, False
        if coast is not None:
            h = C.c_void_p()
            check(ctx.lib.fid_coaster_create(ctx.handle, self.streams, self.max_tracks, C.byref(h)))
            self.coaster = h
            cap2 = self.cap2 = cap + self.max_tracks
            self.coast_det = ctx.empty((self.B, cap2, 5), np.float32)
            self.coast_counts = ctx.empty((self.B,), np.int32)
            self.coast_track = ctx.empty((self.B, cap2, 2), np.int32)
            self.coast_idx = ctx.empty((self.B, cap2), np.int32)
            self.coast_score = ctx.empty((self.B, cap2), np.float32)
        self.relink, self.relinker, self._relinked = relink, None, False
        if relink is not None:
            h = C.c_void_p()
            check(ctx.lib.fid_relinker_create(ctx.handle, self.streams, self.max_tracks, relink.pool, self.emb_dim, C.byref(h)))
            self.relinker = h
            self.relink_cfg = relink.c(max_age)
            self.person = ctx.empty((self.B, cap, 2), np.int32)

    def _pack(self):
        check(self.ctx.lib.fid_track_step(self.ctx.handle, self.tracker, C.c_void_p(self.post.det.ptr), C.c_void_p(self.post.counts.ptr),
                                          self._stream.ctypes.data_as(_lib.c_i32_p), self.B, self.post.cap, C.byref(self.cfg),
                                          C.c_void_p(self.track.ptr), C.c_void_p(self.offsets.ptr), C.c_void_p(self.src.ptr), self.row_cap))
        self._identified = False
        self._coasted = False                                 # (the extended tables are the previous step's until match() has run)
        self._relinked = False

    def identify(self, n_rows: Optional[int] = None, idx=None, score=None):
        """fold the match of the last embed()'s rows back into the tracks (n_rows = 0: a step without a gallery or without a face)"""
        n = self.n_run if n_rows is None else int(n_rows)
        check(self.ctx.lib.fid_track_identify(self.ctx.handle, self.tracker, C.c_void_p(self.post.counts.ptr),
                                              self._stream.ctypes.data_as(_lib.c_i32_p), self.B, self.post.cap, C.c_void_p(self.track.ptr),
                                              C.c_void_p(self.offsets.ptr), C.c_void_p(self.src.ptr), self.row_cap,
                                              _lib._ptr(self.idx if idx is None else idx) if n else None,
                                              _lib._ptr(self.score if score is None else score) if n else None, n,
                                              C.c_void_p(self.ident_idx.ptr), C.c_void_p(self.ident_score.ptr)))
        self._identified = True

    def match(self, gallery: Optional[Gallery], thresh: float = 0.4, q=None, n=None, idx=None, score=None):
        """PackedFacePipeline.match, then identify(); gallery None: tracking alone"""
        n = self.n_run if n is None else n
        if gallery is None:
            n = 0
        super().match(gallery, thresh, q=q, n=n, idx=idx, score=score)
        self.identify(n, idx, score)
        if self.best_shot:
            self._names = gallery.names if gallery is not None else None
            self._keep(q)
        if self.coaster:
            self._coast()
        if self.relinker:
            self._relink(q)

    def _relink(self, q=None):
        """the step's person table: every tracked detection's person id (fid_track_relink; one launch, nothing is read back)"""
        check(self.ctx.lib.fid_track_relink(self.ctx.handle, self.relinker, self.tracker, self._stream.ctypes.data_as(_lib.c_i32_p), self.B,
                                            self.post.cap, C.c_void_p(self.post.counts.ptr), C.c_void_p(self.track.ptr),
                                            C.c_void_p(self.offsets.ptr), C.c_void_p(self.src.ptr), self.row_cap, min(self.n_run, self.row_cap),
                                            _lib._ptr(self.q if q is None else q), C.byref(self.relink_cfg), C.c_void_p(self.person.ptr)))
        self._relinked = True

    def _coast(self):
        """the step's detections plus the tracks that coast, into the extended tables (fid_track_coast; nothing is read back)"""
        check(self.ctx.lib.fid_track_coast(self.ctx.handle, self.coaster, self.tracker, self._stream.ctypes.data_as(_lib.c_i32_p), self.B,
                                           self.post.cap, C.c_void_p(self.post.det.ptr), C.c_void_p(self.post.counts.ptr),
                                           C.c_void_p(self.track.ptr), C.c_void_p(self.ident_idx.ptr), C.c_void_p(self.ident_score.ptr),
                                           C.byref(self.coast), C.c_void_p(self.coast_det.ptr), C.c_void_p(self.coast_counts.ptr),
                                           C.c_void_p(self.coast_track.ptr), C.c_void_p(self.coast_idx.ptr), C.c_void_p(self.coast_score.ptr)))
        self._coasted = True

    def _keep(self, q=None):
        """score the rows the last embed() ran and let the keeper see the step (with no row at all the keep still runs: ended tracks finish)"""
        lib, h, n = self.ctx.lib, self.ctx.handle, self.n_run
        if n > 0:
            check(lib.fid_shot_score(h, C.c_void_p(self.stats.ptr), C.c_void_p(self.measures.ptr), n, C.byref(self.mcfg),
                                     C.c_void_p(self.shot_score.ptr)))
        check(lib.fid_track_keep(h, self.shots, self.tracker, self._stream.ctypes.data_as(_lib.c_i32_p), self.B, self.post.cap,
                                 C.c_void_p(self.track.ptr), C.c_void_p(self.offsets.ptr), C.c_void_p(self.src.ptr), self.row_cap, n,
                                 C.c_void_p(self.shot_score.ptr), _lib._ptr(self.q if q is None else q),
                                 C.c_void_p(self.crops.ptr) if self.keep_crops else None, C.c_void_p(self.post.det.ptr),
                                 C.c_void_p(self.ident_idx.ptr), C.c_void_p(self.ident_score.ptr)))

    # -- finished tracks (best_shot=True) -------------------------------------------------------------
    def _need_shots(self):
        if self.shots is None:
            raise RuntimeError("TrackedFacePipeline: built without best_shot=True")

    def _finished_store(self):
        """(count, meta ptr, q ptr, crops ptr) of the finished store -- fid_shots_finished: synchronises, reads 8 bytes"""
        self._need_shots()
        count, dropped = C.c_int32(0), C.c_int32(0)
        meta, q, crops = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self.ctx.lib.fid_shots_finished(self.ctx.handle, self.shots, C.byref(count), C.byref(dropped), C.byref(meta), C.byref(q),
                                              C.byref(crops)))
        self.finished_dropped = int(dropped.value)
        return int(count.value), meta.value, q.value, crops.value

    def _finished_records(self, n, meta_ptr, names):
        meta = self.ctx.borrow(meta_ptr, (n, _lib.SHOT_META_WORDS), np.int32).download() if n else np.zeros((0, _lib.SHOT_META_WORDS), np.int32)
        f32 = meta.view(np.float32)
        return [dict(stream=int(m[0]), track_id=int(m[1]), name=names[int(m[2])] if m[2] >= 0 and names is not None else "Unknown",
                     similarity=float(f[3]), shot_score=float(f[4]), frame=int(m[5]), rows=int(m[6]), bbox=f[7:11].copy(), det_score=float(f[11]),
                     embedding=None, crop=None) for m, f in zip(meta, f32)]

    def finished(self, clear: bool = True, names=None):
        """The tracks that have ended since the last clear, in the order they ended: one dict each -- stream, track_id, name / similarity (the
        track's identity as of its last embedded face; names: default the last match()'s gallery's), shot_score, frame (of the stream, counted
        over the steps since the pipeline was built), rows (faces of the track that were embedded), bbox, det_score, embedding (unit fp16
        [512], the bits fid_gallery_group reads) and crop (uint8 [112,112,3] BGR, None without keep_crops) of the best shot.  Synchronises.
        `finished_dropped` says how many records found the store full."""
        n, meta, q, crops = self._finished_store()
        recs = self._finished_records(n, meta, self._names if names is None else names)
        if n:
            emb = self.ctx.borrow(q, (n, self.emb_dim), np.float16).download()
            img = self.ctx.borrow(crops, (n, 112, 112, 3), np.uint8).download() if crops else None
            for k, r in enumerate(recs):
                r["embedding"], r["crop"] = emb[k].copy(), (img[k].copy() if img is not None else None)
        if clear:
            check(self.ctx.lib.fid_shots_clear_finished(self.ctx.handle, self.shots))
        return recs

    def finish_all(self, stream: int = -1):
        """end every live track of one stream, or of all (-1): their best shots move to the finished store (the end of a video).  The
        tracker is not touched: a track that goes on afterwards begins a new record."""
        self._need_shots()
        check(self.ctx.lib.fid_shots_flush(self.ctx.handle, self.shots, int(stream)))

    def shots_state(self) -> np.ndarray:
        """the keeper's live entries, int32 [streams, max_tracks, 16] (include/faceid.h: the meta words) -- fid_shots_read; synchronises"""
        self._need_shots()
        meta = np.empty((self.streams, self.max_tracks, _lib.SHOT_META_WORDS), np.int32)
        check(self.ctx.lib.fid_shots_read(self.ctx.handle, self.shots, meta.ctypes.data_as(_lib.c_i32_p)))
        return meta

    def group_finished(self, store, ids=None, names=None, **thresholds):
        """The finished tracks as visits: store.group_device (engine.VectorGallery) on the finished embeddings where they lie -- only the
        count and the records' meta are read back -- then the finished store is cleared.  -> (finished records without embedding / crop,
        group_visits' records), both in finished order.  thresholds: duplicate_threshold, grouping_threshold, similarity_threshold."""
        n, meta, q, _ = self._finished_store()
        recs = self._finished_records(n, meta, self._names if names is None else names)
        groups = store.group_device(q, n, ids, **thresholds) if n else []
        check(self.ctx.lib.fid_shots_clear_finished(self.ctx.handle, self.shots))
        return recs, groups

    def run_step(self, frames_dev, H, W, gallery: Optional[Gallery], thresh: float = 0.4, stream=None):
        """One full pass over one batch of consecutive frames; stream: int [B], the camera of every frame (default: all 0), frames of one
        camera in time order, -1 = not a frame (it ages no track and gets no row).  Asynchronous when rows="capacity"."""
        st = np.zeros(self.B, np.int32) if stream is None else np.ascontiguousarray(stream, dtype=np.int32).reshape(-1)
        if st.shape[0] != self.B:
            raise ValueError(f"stream has {st.shape[0]} entries for a batch of {self.B}")
        self._stream = st
        self.detect(frames_dev, H, W)
        self.embed(frames_dev, H, W)
        self.match(gallery, thresh)

    def reset(self, stream: int = -1):
        """forget the tracks of one stream, or of all (-1: ids start at 0 again).  With best_shot=True the keeper is not touched here: the
        next step's keep finishes the tracks the reset orphaned (a stream's ids begin again at 0; a track that STARTS in an orphan's slot
        under the orphan's id still ends it)"""
        check(self.ctx.lib.fid_tracker_reset(self.ctx.handle, self.tracker, int(stream)))
        if stream < 0:
            self._identified = True
        if self.coaster:                                      # (a held box of a forgotten track would outlive it)
            check(self.ctx.lib.fid_coaster_reset(self.ctx.handle, self.coaster, int(stream)))
        if self.relinker:                                     # (a stream's ids begin again at 0: a pooled id would name somebody else)
            check(self.ctx.lib.fid_relinker_reset(self.ctx.handle, self.relinker, int(stream)))

    def tracker_state(self) -> Tuple[np.ndarray, np.ndarray]:
        """(slots int32 [streams, max_tracks, 10], per-stream int32 [streams, 2] = next id, lost) -- fid_tracker_read; synchronises"""
        slots = np.empty((self.streams, self.max_tracks, _lib.TRACK_SLOT_WORDS), np.int32)
        per_stream = np.empty((self.streams, 2), np.int32)
        check(self.ctx.lib.fid_tracker_read(self.ctx.handle, self.tracker, slots.ctypes.data_as(_lib.c_i32_p),
                                            per_stream.ctypes.data_as(_lib.c_i32_p)))
        return slots, per_stream

    @property
    def rows_embedded(self) -> int:
        """rows of the last step's table: the faces that went through the recogniser (reads 4 bytes back)"""
        total = int(self.ctx.borrow(self.offsets.ptr + 4 * self.B, (1,), np.int32).download()[0])
        return min(total, self.row_cap)

    def redact(self, frames_dev, H, W, style=None):
        """FacePipeline.redact for EVERY detection, by its TRACK's identity (ident_idx, id_stride = cap): a person named earlier in the track
        stays in the clear in the frames where the face was not embedded again"""
        self._need_coasted()
        if self.coaster:                                      # ... and for every coasted track, behind the frame's detections
            return self._redact(frames_dev, H, W, style, self.coast_idx, self.coast_score, self.cap2, det=self.coast_det,
                                counts=self.coast_counts, cap=self.cap2)
        return self._redact(frames_dev, H, W, style, self.ident_idx, self.ident_score, self.post.cap)

    def draw(self, frames_dev, H, W, labels, style=None, out=None, redact=None):
        """FacePipeline.draw for EVERY detection, with its track's name and score; a style with the DRAW_TRACK_ID flag prints the track id"""
        self._need_coasted()
        if self.coaster:                                      # a held box is drawn after the detections: it wins where they overlap
            return self._draw(frames_dev, H, W, labels, style, self.coast_idx, self.coast_score, self.cap2, track=self.coast_track, out=out,
                              redact=redact, det=self.coast_det, counts=self.coast_counts, cap=self.cap2)
        if self.relinker:                                     # the person table in place of the track table: the drawn number stays
            self._need_relinked()
            return self._draw(frames_dev, H, W, labels, style, self.ident_idx, self.ident_score, self.post.cap, track=self.person, out=out,
                              redact=redact)
        return self._draw(frames_dev, H, W, labels, style, self.ident_idx, self.ident_score, self.post.cap, track=self.track, out=out,
                          redact=redact)

    # -- results -----------------------------------------------------------------------------------
    def results_tracked(self, gallery: Optional[Gallery] = None):
        """Host view of the last step: per frame, for EVERY detection in the detector's order,
        (bbox[4], det_score, kps[5,2], name, similarity, track id, started) -- name / similarity are the track's (an untracked face's own
        match; "Unknown" / 0.0 without one), track id -1 = untracked, started = the track began with this detection.  Sets `overflow`."""
        if not self._identified:
            raise RuntimeError("TrackedFacePipeline: the last step has not been identified (match() / identify())")
        self.post.check()
        counts, det, kps = self.post.counts.download(), self.post.det.download(), self.post.kps.download()
        track, ii, sc = self.track.download(), self.ident_idx.download(), self.ident_score.download()
        self._overflow = max(int(self.offsets.download()[self.B]) - self.row_cap, 0)
        cap = det.shape[1]
        out = []
        for b in range(self.B):
            faces = []
            for f in range(0 if self._stream[b] < 0 else min(max(int(counts[b]), 0), cap)):
                j = int(ii[b, f])
                tid, word = int(track[b, f, 0]), int(track[b, f, 1])
                faces.append((det[b, f, :4].copy(), float(det[b, f, 4]), kps[b, f].reshape(5, 2).copy(),
                              gallery.names[j] if j >= 0 and gallery is not None else "Unknown", float(sc[b, f]), tid,
                              word >= 0 and bool(word & _lib.TRACK_STARTED)))
            out.append(faces)
        return out

    def _need_relinked(self):
        if self.relinker is None:
            raise RuntimeError("TrackedFacePipeline: built without relink=RelinkConfig(...)")
        if not self._relinked:
            raise RuntimeError("TrackedFacePipeline: the last step has not been relinked (match() runs fid_track_relink; identify() alone does not)")

    def results_persons(self, gallery: Optional[Gallery] = None):
        """results_tracked()'s tuples plus (person id, relinked): the person id is the id of the first track of the detection's chain (the
        track id itself for a track that was never linked, -1 for an untracked face), relinked = it is an earlier track's"""
        self._need_relinked()
        person = self.person.download()
        return [[face + (int(person[b, f, 0]), person[b, f, 1] >= 0 and bool(person[b, f, 1] & _lib.TRACK_RELINKED))
                 for f, face in enumerate(frame)] for b, frame in enumerate(self.results_tracked(gallery))]

    def relinker_state(self):
        """the relinker's tables (include/faceid.h: the words): dict of live int32 [streams, max_tracks, 8], pool int32 [streams, pool, 8],
        frames int32 [streams], live_q fp16 [streams, max_tracks, dim], pool_q fp16 [streams, pool, dim] -- fid_relinker_read; synchronises"""
        if self.relinker is None:
            raise RuntimeError("TrackedFacePipeline: built without relink=RelinkConfig(...)")
        S, T, L = self.streams, self.max_tracks, self.relink.pool
        st = dict(live=np.empty((S, T, _lib.RELINK_WORDS), np.int32), pool=np.empty((S, L, _lib.RELINK_WORDS), np.int32),
                  frames=np.empty(S, np.int32), live_q=np.empty((S, T, self.emb_dim), np.float16), pool_q=np.empty((S, L, self.emb_dim), np.float16))
        check(self.ctx.lib.fid_relinker_read(self.ctx.handle, self.relinker, st["live"].ctypes.data_as(_lib.c_i32_p),
                                             st["pool"].ctypes.data_as(_lib.c_i32_p), st["frames"].ctypes.data_as(_lib.c_i32_p),
                                             st["live_q"].ctypes.data_as(C.c_void_p), st["pool_q"].ctypes.data_as(C.c_void_p)))
        return st

    def _need_coaster(self):
        if self.coaster is None:
            raise RuntimeError("TrackedFacePipeline: built without coast=CoastConfig(...)")

    def _need_coasted(self):
        """redact / draw / results_coasted read the extended tables: they must be this step's"""
        if not self._identified:
            raise RuntimeError("TrackedFacePipeline: the last step has not been identified (match() / identify())")
        if self.coaster and not self._coasted:
            raise RuntimeError("TrackedFacePipeline: the last step has not been coasted (match() runs fid_track_coast; identify() alone does not)")

    def coaster_state(self) -> np.ndarray:
        """the coaster's entries, int32 [streams, max_tracks, 16] (include/faceid.h: the words) -- fid_coaster_read; synchronises"""
        self._need_coaster()
        entries = np.empty((self.streams, self.max_tracks, _lib.COAST_WORDS), np.int32)
        check(self.ctx.lib.fid_coaster_read(self.ctx.handle, self.coaster, entries.ctypes.data_as(_lib.c_i32_p)))
        return entries

    def results_coasted(self, gallery: Optional[Gallery] = None):
        """Host view of the last step's coasted tracks: per frame, in slot order, (bbox[4], det_score, name, similarity, track id, missed)
        -- the held box, the detection score and the name of the track's last matched frame, and the frames it has been missing for."""
        self._need_coaster()
        self._need_coasted()
        counts, det, track = self.coast_counts.download(), self.coast_det.download(), self.coast_track.download()
        ii, sc = self.coast_idx.download(), self.coast_score.download()
        out = []
        for b in range(self.B):
            rows = []
            for f in range(min(max(int(counts[b]), 0), self.cap2)):
                word, j = int(track[b, f, 1]), int(ii[b, f])
                if word >= 0 and word & _lib.TRACK_COASTED:
                    rows.append((det[b, f, :4].copy(), float(det[b, f, 4]), gallery.names[j] if j >= 0 and gallery is not None else "Unknown",
                                 float(sc[b, f]), int(track[b, f, 0]), word >> 16))
            out.append(rows)
        return out

    def results(self, gallery: Optional[Gallery] = None):
        """the list FacePipeline.results gives -- (bbox[4], det_score, kps[5,2], name, similarity) -- for every detection, name and
        similarity taken from its track"""
        return [[face[:5] for face in frame] for frame in self.results_tracked(gallery)]

    def results_measured(self, gallery: Optional[Gallery] = None):
        """(results(gallery), measured): measured[b][f] is the MEASURE_KEYS dict of detection f of frame b if it was embedded in this step (the
        tracker's rows are the faces embedded now), else None"""
        res = self.results(gallery)
        rows = self._measured_rows()
        src = self.src.download()
        n, cap = min(self.n_run, self.row_cap), self.post.cap
        row_of = {int(src[i]): i for i in range(n) if src[i] >= 0}
        return res, [[rows[row_of[b * cap + f]] if b * cap + f in row_of else None for f in range(len(res[b]))] for b in range(self.B)]

    def embeddings(self) -> Tuple[np.ndarray, np.ndarray]:
        """Raw fp32 embeddings of the rows the last step ran, [rows, 512] in table order, and the table's offsets [B+1] (src says whose)."""
        offsets = self.offsets.download()
        kept = min(int(offsets[self.B]), self.row_cap, self.n_run)
        if kept == 0:
            return np.zeros((0, self.emb_dim), np.float32), offsets
        return self.rec.read(self.rec.low.outputs[0], kept).reshape(kept, -1), offsets

    def close(self):
        if self.relinker:
            self.ctx.lib.fid_relinker_destroy(self.ctx.handle, self.relinker)
            self.relinker = None
        if self.coaster:
            self.ctx.lib.fid_coaster_destroy(self.ctx.handle, self.coaster)
            self.coaster = None
        if self.shots:
            self.ctx.lib.fid_shots_destroy(self.ctx.handle, self.shots)
            self.shots = None
        if self.tracker:
            self.ctx.lib.fid_tracker_destroy(self.ctx.handle, self.tracker)
            self.tracker = None


def calibrate_detector_bias(ctx: Context, net, params, frames: np.ndarray, target: int = 48, max_batch: int = 8):
    """Synthetic (random-init) detectors fire on ~half of all anchors.  Shift the shared cls bias so that
    the busiest-to-quietest calibration frame keeps at least `target` anchors >= 0.5 -- the job training
    does for a real detector.  Returns a NEW params dict; it feeds the HIP engine and the oracle alike."""
    cn = CompiledNet(ctx, net, params, max_batch=max_batch)
    kth = []
    for b0 in range(0, len(frames), max_batch):
        chunk = frames[b0:b0 + max_batch]
        cn.run(chunk)
        sc = np.concatenate([cn.read(name, len(chunk))[..., :2].reshape(len(chunk), -1) for name in cn.low.outputs], axis=1)
        sc = np.clip(sc.astype(np.float64), 1e-7, 1 - 1e-7)
        logit = np.log(sc / (1 - sc))
        kth += [np.sort(l)[-target] for l in logit]
    cn.close()
    shift = -float(min(kth))
    out = dict(params)
    for k in params:
        if k.endswith(".cls.bias"):
            out[k] = (params[k] + np.float32(shift)).astype(np.float32)
    return out, shift


# ---- gallery construction: reference main.py:78-105 ----------------------------------------------------

def _read_image(path: str) -> Optional[np.ndarray]:
    """cv2.imread stand-in for hosts without OpenCV: returns uint8 BGR [H,W,3] or None (like imread on a file
    it cannot decode).  Uses OpenCV when importable; otherwise understands .npy arrays and binary PPM (P6)."""
    try:
        import cv2
        return cv2.imread(path)
    except ImportError:
        pass
    try:
        if path.endswith(".npy"):
            a = np.load(path, allow_pickle=False)
            return np.ascontiguousarray(a, dtype=np.uint8) if a.ndim == 3 and a.shape[2] == 3 else None
        with open(path, "rb") as f:
            data = f.read()
        if data[:2] == b"P6":
            tok, pos = [], 2
            while len(tok) < 3:                          # width, height, maxval (comments allowed)
                while data[pos:pos + 1].isspace():
                    pos += 1
                if data[pos:pos + 1] == b"#":
                    pos = data.index(b"\n", pos) + 1
                    continue
                end = pos
                while not data[end:end + 1].isspace():
                    end += 1
                tok.append(int(data[pos:end])); pos = end
            w, h, mx = tok
            if mx != 255:
                return None
            rgb = np.frombuffer(data, np.uint8, count=w * h * 3, offset=pos + 1).reshape(h, w, 3)
            return np.ascontiguousarray(rgb[..., ::-1])
    except Exception:
        return None
    return None


def build_targets_from_images(detector, recognizer, images: Sequence[np.ndarray], names: Sequence[str],
                              paths: Optional[Sequence[str]] = None) -> List[Tuple[np.ndarray, str]]:
    """The body of reference build_targets (main.py:91-103) for images already in memory:
    per image `detect(image, max_num=1)` (:96), images without a face are skipped with a warning (:98-100),
    the best face is embedded (`recognizer(image, kpss[0])`, :102) and `(embedding, name)` collected (:103),
    in input order.  Images of one shape go through the detector, the alignment and the recogniser as ONE
    batch (detect_batch -> fid_align_crops -> get_feat); images of differing shapes go through them in chunks of
    the detector's `max_batch` consecutive images, each one mixed-size batch (fid_align_crops_ragged); objects
    without the batched surface are driven through the reference's per-image calls."""
    import logging
    assert len(images) == len(names)
    kps_of: List[Optional[np.ndarray]] = [None] * len(images)
    batched = hasattr(detector, "detect_batch") and hasattr(recognizer, "get_feat") and getattr(recognizer, "_native", False)
    by_shape = {}
    for i, im in enumerate(images):
        by_shape.setdefault(tuple(im.shape), []).append(i)
    emb_of: List[Optional[np.ndarray]] = [None] * len(images)
    if batched and len(by_shape) > 1 and hasattr(detector, "_detect_chunk_ragged"):
        ctx = recognizer.ctx
        step = detector._max_batch
        for b0 in range(0, len(images), step):
            ids = list(range(b0, min(b0 + step, len(images))))
            chunk = [np.ascontiguousarray(images[i], dtype=np.uint8) for i in ids]
            dets = detector.detect_batch(chunk, max_num=1)
            hit = [k for k, (_, kpss) in enumerate(dets) if len(kpss)]
            if not hit:
                continue
            n = len(hit)
            kps = np.stack([dets[k][1][0].reshape(10) for k in hit]).astype(np.float32).reshape(n, 1, 10)
            batch = ctx.image_batch([chunk[k] for k in hit])
            kp, cn = ctx.to_device(kps), ctx.to_device(np.ones(n, np.int32))
            crops = ctx.empty((n, 112, 112, 3), np.uint8)
            check(ctx.lib.fid_align_crops_ragged(ctx.handle, *batch.args(), n, C.c_void_p(kp.ptr), C.c_void_p(cn.ptr), 1, 1,
                                                 C.c_void_p(crops.ptr), None))
            feats = recognizer.get_feat(crops.download())
            for k, e in zip(hit, feats):
                emb_of[ids[k]] = np.ascontiguousarray(e, dtype=np.float32).reshape(-1)
        by_shape = {}
    for shape, ids in by_shape.items():
        if not batched:
            for i in ids:
                _, kpss = detector.detect(images[i], max_num=1)
                if len(kpss):
                    emb_of[i] = np.asarray(recognizer(images[i], kpss[0]), dtype=np.float32).reshape(-1)
            continue
        stack = np.ascontiguousarray(np.stack([images[i] for i in ids]), dtype=np.uint8)
        dets = detector.detect_batch(stack, max_num=1)
        hit = [k for k, (_, kpss) in enumerate(dets) if len(kpss)]
        if not hit:
            continue
        ctx = recognizer.ctx
        H, W = shape[:2]
        n = len(hit)
        kps = np.stack([dets[k][1][0].reshape(10) for k in hit]).astype(np.float32).reshape(n, 1, 10)
        fr = ctx.to_device(stack[hit])
        kp, cn = ctx.to_device(kps), ctx.to_device(np.ones(n, np.int32))
        crops = ctx.empty((n, 112, 112, 3), np.uint8)
        check(ctx.lib.fid_align_crops(ctx.handle, C.c_void_p(fr.ptr), n, H, W, C.c_void_p(kp.ptr), C.c_void_p(cn.ptr),
                                      1, 1, C.c_void_p(crops.ptr), None))
        feats = recognizer.get_feat(crops.download())
        for k, e in zip(hit, feats):
            emb_of[ids[k]] = np.ascontiguousarray(e, dtype=np.float32).reshape(-1)
    targets = []
    for i, name in enumerate(names):
        if emb_of[i] is None:
            logging.warning(f"No face detected in {paths[i] if paths else name}. Skipping...")
            continue
        targets.append((emb_of[i], name))
    return targets


def build_targets(detector, recognizer, params, *, loader=None) -> List[Tuple[np.ndarray, str]]:
    """reference main.py:78-105, same signature: `params.faces_dir` is scanned with os.listdir (:91),
    `name = filename[:-4]` (:92), every file is read (:95) and handed to build_targets_from_images.
    `params` may also be the directory path itself.  Files the loader cannot decode are skipped."""
    import logging
    import os
    faces_dir = params if isinstance(params, str) else params.faces_dir
    loader = loader or _read_image
    images, names, paths = [], [], []
    for filename in os.listdir(faces_dir):
        image_path = os.path.join(faces_dir, filename)
        image = loader(image_path)
        if image is None:
            logging.warning(f"Cannot read {image_path}. Skipping...")
            continue
        images.append(image); names.append(filename[:-4]); paths.append(image_path)
    return build_targets_from_images(detector, recognizer, images, names, paths)


def merge_targets(ctx: Optional[Context], targets: Sequence[Tuple[np.ndarray, str]], min_score=None) -> List[Tuple[np.ndarray, str]]:
    """The `(embedding, name)` list of build_targets with ONE entry per distinct name, in the order of first appearance: the entries of a name
    become its identity template (fid_gallery_templates: the mean of their unit embeddings, re-normalised; with `min_score` the entries that
    score below it against the mean are left out -- None, the default, drops nothing).  So a folder with ann_1.jpg, ann_2.jpg serves once the
    caller has mapped file names to persons.  ctx: the device context (a temporary VectorGallery), or None for the host twin
    (helpers.identity_templates: the same rule without a GPU).  A name whose entries cancel or are all dropped has no template and is left
    out with a warning.  build_targets and gallery_from_targets stay as they are."""
    import logging
    if not targets:
        return []
    emb = np.stack([np.asarray(t[0], np.float32).reshape(-1) for t in targets])
    names = [t[1] for t in targets]
    if ctx is None:
        from .utils.helpers import identity_templates
        res = identity_templates(emb, names, None, min_score)
    else:
        from .engine import VectorGallery
        store = VectorGallery(ctx, emb.shape[1], capacity=max(128, len(targets)))
        try:
            store.upsert(list(range(len(targets))), emb)
            res = store.templates(dict(enumerate(names)), None, min_score)
        finally:
            store._gal.close()
    out = []
    for p, name in enumerate(res.persons):
        if res.cohesion[p] > 0:
            out.append((res.templates[p].astype(np.float32), name))
        else:
            logging.warning(f"No template for {name}: its faces cancel or were all dropped. Skipping...")
    return out


def gallery_from_targets(ctx: Context, targets: Sequence[Tuple[np.ndarray, str]]) -> Gallery:
    """The `targets` list as a device-resident Gallery (what frame_processor scans, main.py:136-142)."""
    assert len(targets) > 0, "no targets: every gallery image was skipped"
    return Gallery(ctx, np.stack([t[0] for t in targets]).astype(np.float32), [t[1] for t in targets])


# ---- multi-GPU step: the single collective -----------------------------------------------------

class Communicator:
    """fid_comm: this rank's end of an RCCL communicator owned by libfaceid (include/faceid.h), so the collective runs
    behind the C-ABI on the context's stream.  `exchange_id(id_bytes_or_None) -> id_bytes` is how the host hands rank 0's
    128-byte rendezvous id to every rank (a torch.distributed broadcast, an MPI bcast, a file ...)."""

    def __init__(self, ctx: Context, world: int, rank: int, exchange_id):
        self.ctx, self.world, self.rank = ctx, int(world), int(rank)
        n = 128
        buf = (C.c_uint8 * n)()
        if rank == 0:
            check(ctx.lib.fid_comm_unique_id(buf, n))
        ident = exchange_id(bytes(buf) if rank == 0 else None)
        assert len(ident) == n
        h = C.c_void_p()
        check(ctx.lib.fid_comm_init_rank(ctx.handle, self.world, self.rank, ident, n, C.byref(h)))
        self.handle = h

    def get_rank(self):
        return self.rank

    def get_world_size(self):
        return self.world

    def all_gather_into_tensor(self, out, inp):
        """same call shape as torch.distributed's; `out` / `inp` are device buffers (anything _lib._ptr accepts)
        and `inp` carries .nbytes or (numel, element_size)"""
        nbytes = inp.nbytes if hasattr(inp, "nbytes") and not callable(inp.nbytes) else inp.numel() * inp.element_size()
        check(self.ctx.lib.fid_allgather(self.ctx.handle, self.handle, _lib._ptr(inp), _lib._ptr(out), int(nbytes)))

    def close(self):
        if self.handle:
            self.ctx.lib.fid_comm_destroy(self.ctx.handle, self.handle)
            self.handle = None


EMPTY_SLOT_MARK = 0x8000          # fp16 -0.0 in element 0 of an otherwise all +0.0 row (csrc/match.hip l2norm_rows)


def empty_slot_rows(q_all: np.ndarray) -> np.ndarray:
    """bool per row of a unit-embedding matrix (fp16, host copy): True = the row is the EMPTY-slot marker fid_l2_normalize_f16_slots writes
    for face slots f >= counts[b] (-0.0 then +0.0s).  A degenerate face inside a frame's valid prefix (zero / NaN / inf embedding) is an
    all +0.0 row instead: numerically the same zero row (never matches), but still a face."""
    u = np.ascontiguousarray(np.asarray(q_all)).view(np.uint16).reshape(-1, np.asarray(q_all).shape[-1])
    return (u[:, 0] == EMPTY_SLOT_MARK) & ~u[:, 1:].any(axis=1)


def gathered_face_counts(q_all: np.ndarray, frames_total: int, faces_per_frame: int) -> np.ndarray:
    """Face count of every frame of the WHOLE batch from the gathered unit-embedding matrix [frames_total * F, 512] (fp16 host copy):
    a slot holds a face iff its row is not the empty-slot marker (empty_slot_rows) -- so the one collective of SURVEY.md 8e also carries
    `counts[]` EXACTLY and idx_all / score_all can be read like the reference's per-face loop (main.py:132-134), which visits a detected
    face whether or not its embedding is degenerate.  (Round 3 counted non-zero rows: a degenerate face at slot f < count shifted every
    later slot of its frame by one.)"""
    q = np.asarray(q_all)
    assert q.dtype == np.float16, "the gathered matrix is fp16 (bit patterns matter: -0.0 marks an empty slot)"
    return (~empty_slot_rows(q)).reshape(frames_total, faces_per_frame).sum(axis=1).astype(np.int32)


def _slice_ptr(buf, row0: int, row_bytes: int):
    """device address of row `row0` of a 2-D device buffer (torch tensor / DeviceBuffer / raw int)"""
    base = buf.data_ptr() if hasattr(buf, "data_ptr") else (buf.ptr if hasattr(buf, "ptr") else int(buf))
    return base + row0 * row_bytes


def _first_rows(buf, rows: int):
    """the first `rows` rows of a device buffer the collective / match calls accept (torch tensor or numpy array: a view; else unchanged)"""
    if buf is None or not hasattr(buf, "shape") or int(buf.shape[0]) == rows:
        return buf
    return buf[:rows]


def run_step_distributed(pipe, frames_dev, H, W, gallery, thresh, q_local, q_all, dist, *, idx_all=None, score_all=None,
                         match_scope: str = "all", keys_local=None, keys_all=None, gallery_first_row: int = 0,
                         gallery_total: int = 0, flush: bool = False):
    """One multi-GPU step: local detect / align / embed on this rank's frames, ONE all-gather of the
    unit fp16 embeddings (the collective BASELINE.json's north_star names), then the gallery match on the gathered
    matrix.  `dist` is torch.distributed (RCCL as backend "nccl", gloo in the CPU tests) or a `Communicator`
    (the C-ABI's own RCCL communicator): anything with get_rank / get_world_size / all_gather_into_tensor.

    q_local [n,512] / q_all [world*n,512] fp16 device buffers (pipe.q aliases q_local).

    match_scope
      "all"      (default; replicated gallery) every rank matches ALL world*n gathered queries, so every rank holds the
                 whole batch's result list in idx_all / score_all [world*n] with no second collective -- the gather's
                 output is what the match reads.
      "own"      every rank matches only its own n rows of the gathered matrix into pipe.idx / pipe.score (the cheapest
                 form when the host collects per-rank results itself).
      "sharded"  gallery sharded by contiguous row blocks (the 1 M-entry variant): `gallery` holds rows
                 [gallery_first_row, +G_local) of a gallery_total-row gallery; every rank scans its shard for all
                 world*n queries (fid_match_keys), a second tiny all-gather exchanges the packed (score, index) keys
                 (keys_local [world*n] u64 -> keys_all [world, world*n]), fid_match_merge takes the arg-max.

    A GroupedFacePipeline (anything with collect / embed_collected) only detects + aligns until its group is full: the call returns False
    and nothing is exchanged.  The group's last step (or `flush=True`, which embeds what a stream's end left of a group without detecting
    anything) runs IResNet on all collected crops, then the SAME one all-gather and match on n = steps * B * F rows per rank -- the buffers
    are sized for a full group, a partial group uses their first rows (every rank holds the same number of steps).  Returns True when results
    were written.
    """
    if isinstance(pipe, PackedFacePipeline):
        # its rows are not B x F slots: the other ranks' per-frame offsets would have to travel too (a second small gather)
        raise TypeError("run_step_distributed works on face slots (FacePipeline / GroupedFacePipeline); a PackedFacePipeline is single-device")
    r, world = dist.get_rank(), dist.get_world_size()
    n = pipe.n_slots
    grouped = hasattr(pipe, "collect")
    n_cap = n * (pipe.group if grouped else 1)              # rows per rank the buffers must hold

    def rows(buf):                                   # entries of a result / key buffer (torch tensor, DeviceBuffer, numpy array)
        if buf is None:
            return 0
        return int(np.prod(tuple(buf.shape))) if hasattr(buf, "shape") else int(buf.nbytes // buf.itemsize)

    # the scopes that write world*n results must be given buffers of that size: falling back to pipe.idx / pipe.score (n entries)
    # would overrun them at world > 1 (a one-rank group may use them: world*n == n)
    if match_scope == "all" and idx_all is None and score_all is None and world == 1:
        idx_all, score_all = pipe.idx, pipe.score
    if match_scope in ("all", "sharded") and (rows(idx_all) < world * n_cap or rows(score_all) < world * n_cap):
        raise ValueError(f"match_scope={match_scope!r} writes {world * n_cap} results: pass idx_all / score_all with at least that many entries")
    if match_scope == "sharded" and (rows(keys_local) < world * n_cap or rows(keys_all) < world * world * n_cap or gallery_total <= 0):
        raise ValueError("match_scope='sharded' needs keys_local [world*n], keys_all [world*world*n] (uint64) and gallery_total")
    if grouped:
        if not flush and not pipe.collect(frames_dev, H, W):
            return False                    # the group is still open: this step's crops wait for the group's last step
        steps = pipe.embed_collected()      # writes q_local[0 : steps * B * F]
        if steps == 0:
            return False
        n = steps * pipe.n_slots
        q_local, q_all = _first_rows(q_local, n), _first_rows(q_all, world * n)
        idx_all, score_all = _first_rows(idx_all, world * n), _first_rows(score_all, world * n)
        keys_local, keys_all = _first_rows(keys_local, world * n), _first_rows(keys_all, world * world * n)
    else:
        pipe.detect(frames_dev, H, W)
        pipe.embed(frames_dev, H, W)        # writes q_local (pipe.q aliases it); empty face slots are zero rows
    dist.all_gather_into_tensor(q_all, q_local)
    if match_scope == "own":
        pipe.match(gallery, thresh, q=_slice_ptr(q_all, r * n, 512 * 2), n=n)
    elif match_scope == "all":
        pipe.match(gallery, thresh, q=q_all, n=world * n, idx=idx_all, score=score_all)
    elif match_scope == "sharded":
        pipe.match_keys(gallery, q_all, world * n, gallery_first_row, keys_local)
        dist.all_gather_into_tensor(keys_all, keys_local)
        pipe.match_merge(keys_all, world, world * n, gallery_total, thresh, idx_all, score_all)
    else:
        raise ValueError(f"unknown match_scope {match_scope!r}")
    return True
