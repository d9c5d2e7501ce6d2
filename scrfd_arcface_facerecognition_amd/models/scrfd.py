"""SCRFD detector with the call surface of reference models/scrfd.py (class SCRFD, :12-207):
same constructor arguments and defaults, same attributes, same `forward` / `detect` / `nms`
results -- computed by libfaceid on an MI355X instead of onnxruntime + numpy."""
from __future__ import annotations

import ctypes as C
from typing import List, Tuple

import numpy as np

from .. import _lib
from .._lib import check
from ..engine import HeadViews, PostProcessor
from ..session import HipSession

__all__ = ["SCRFD"]


class SCRFD:
    def __init__(self, model_path: str, input_size: Tuple[int] = (640, 640), conf_thres: float = 0.5,
                 iou_thres: float = 0.4, *, device: int = 0, ctx=None, max_batch: int = 8, max_det: int = 512,
                 session=None) -> None:
        self.input_size = input_size
        self.conf_thres = conf_thres
        self.iou_thres = iou_thres
        # SCRFD model params (reference scrfd.py:39-47)
        self.fmc = 3
        self._feat_stride_fpn = [8, 16, 32]
        self._num_anchors = 2
        self.use_kps = True
        self.mean = 127.5
        self.std = 128.0
        self.center_cache = {}
        self._device, self._ctx, self._max_batch, self._max_det = device, ctx, int(max_batch), int(max_det)
        self._post = None
        self._session = session        # keyword-only extension: a ready HipSession (like ArcFace(session=...), arcface.py:11-21)
        self._initialize_model(model_path=model_path)

    def _initialize_model(self, model_path: str):
        try:
            self.session = self._session or HipSession(model_path, ctx=self._ctx, device=self._device,
                                                       input_hw=(self.input_size[1], self.input_size[0]),
                                                       max_batch=self._max_batch)
            self.output_names = [x.name for x in self.session.get_outputs()]
            self.input_names = [x.name for x in self.session.get_inputs()]
        except Exception as e:                       # reference scrfd.py:66-68
            print(f"Failed to load the model: {e}")
            raise
        self.ctx = self.session.ctx

    # ------------------------------------------------------------------------------------
    def _postprocessor(self) -> PostProcessor:
        if self._post is None:
            self._post = PostProcessor(self.ctx, self._max_batch, cap=self._max_det)
        return self._post

    def _run_net(self, images_dev, B, hw):
        cn = self.session.compiled(hw)
        cn.run_device(images_dev, B)
        return cn

    def forward(self, image, threshold):
        """scrfd.py:70-120: (scores_list, bboxes_list, kpss_list) per stride, candidates >= threshold in
        anchor order, coordinates in the (letterboxed) input image."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        H, W = image.shape[:2]
        cn = self.session.compiled((H, W))
        cn.run(image[None])
        hv = HeadViews.from_fused(cn)
        post = self._postprocessor()
        rec = self.ctx.empty((1, post.cand_cap, 16), np.float32)
        cnt = self.ctx.empty((1,), np.int32)
        check(self.ctx.lib.fid_scrfd_decode(self.ctx.handle, C.cast(hv.ptrs, _lib.c_void_pp), hv.pix, hv.anc, hv.bstride,
                                            1, H, W, self._num_anchors, float(threshold), C.c_void_p(rec.ptr),
                                            C.c_void_p(cnt.ptr)))
        n = int(cnt.download()[0])
        if n > post.cand_cap:
            raise _lib.FaceIdError(-3, f"{n} candidates exceed the workspace ({post.cand_cap})")
        r = rec.download()[0, :n]
        flat = r[:, 15].view(np.int32)
        bounds = np.cumsum([(H // s) * (W // s) * self._num_anchors for s in self._feat_stride_fpn])
        level = np.searchsorted(bounds, flat, side="right")
        scores_list, bboxes_list, kpss_list = [], [], []
        for lv in range(self.fmc):
            m = level == lv
            scores_list.append(np.ascontiguousarray(r[m, 4:5]))
            bboxes_list.append(np.ascontiguousarray(r[m, 0:4]))
            kpss_list.append(np.ascontiguousarray(r[m, 5:15]).reshape(-1, 5, 2))
        return scores_list, bboxes_list, kpss_list

    def detect_batch(self, images, max_num=0, metric="max") -> List[Tuple[np.ndarray, np.ndarray]]:
        """Batched detect(): images uint8 [B,H,W,3], or a list of uint8 [H,W,3] images -> [(det[K,5], kpss[K,5,2])] per frame.
        A list whose images differ in shape runs in chunks of `max_batch` consecutive images, each ONE mixed-size batch
        (`_detect_chunk_ragged`); the reference detects such images one by one (main.py:96)."""
        if isinstance(images, (list, tuple)) and len({tuple(np.shape(im)) for im in images}) > 1:
            images = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
            results = []
            for b0 in range(0, len(images), self._max_batch):
                results += self._detect_chunk_ragged(images[b0:b0 + self._max_batch], max_num, metric)
            return results
        images = np.ascontiguousarray(images, dtype=np.uint8)
        assert images.ndim == 4 and images.shape[3] == 3
        results = []
        for b0 in range(0, images.shape[0], self._max_batch):
            chunk = images[b0:b0 + self._max_batch]
            results += self._detect_chunk(chunk, max_num, metric)
        return results

    def _detect_chunk(self, images, max_num, metric, frames=None):
        """`frames`: the chunk already on the device (a caller that reads the frames again, e.g. for the warp, uploads them once)"""
        B, H, W, _ = images.shape
        in_w, in_h = self.input_size
        frames = self.ctx.to_device(images) if frames is None else frames
        if (H, W) == (in_h, in_w):
            det_in = frames
        else:                                      # scrfd.py:123-138 on the device
            det_in = self.ctx.empty((B, in_h, in_w, 3), np.uint8)
            sc = C.c_double()
            check(self.ctx.lib.fid_letterbox(self.ctx.handle, C.c_void_p(frames.ptr), B, H, W, C.c_void_p(det_in.ptr),
                                             in_h, in_w, C.byref(sc)))
        cn = self._run_net(det_in, B, (in_h, in_w))
        post = self._postprocessor()
        post.run(HeadViews.from_fused(cn), B, (in_h, in_w), (H, W), self.conf_thres, self.iou_thres, max_num,
                 0 if metric == "max" else 1, self._num_anchors)
        return post.fetch(B)

    def _detect_chunk_ragged(self, images, max_num, metric, batch=None):
        """_detect_chunk for images of differing sizes (at most max_batch): pack, letterbox, ONE net run and post-process for the whole
        list.  `batch`: the list already on the device (Context.image_batch)."""
        batch = self.ctx.image_batch(images) if batch is None else batch
        B = batch.B
        in_w, in_h = self.input_size
        det_in = self.ctx.empty((B, in_h, in_w, 3), np.uint8)
        check(self.ctx.lib.fid_letterbox_ragged(self.ctx.handle, *batch.args(), B, C.c_void_p(det_in.ptr), in_h, in_w, None))
        cn = self._run_net(det_in, B, (in_h, in_w))
        post = self._postprocessor()
        post.run_ragged(HeadViews.from_fused(cn), B, (in_h, in_w), batch.hw, self.conf_thres, self.iou_thres, max_num,
                        0 if metric == "max" else 1, self._num_anchors)
        return post.fetch(B)

    # ---- tiled detection: frames larger than the input, seen at native resolution (no reference analogue) ---------------------------------
    def _detect_chunk_tiled(self, images, max_num, metric, overlap=128, edge_margin=8, overview=True, frames=None):
        """_detect_chunk with every frame cut into pipeline.tile_plan's tiles: fid_tile_cut, ONE net run over the B * tiles-per-frame tiles
        (at most max_batch), fid_scrfd_postprocess_tiled -> per frame its detections in frame coordinates.  The post-process's device arrays
        hold the B frames afterwards, as after _detect_chunk."""
        from ..pipeline import tile_plan
        B, H, W, _ = images.shape
        in_w, in_h = self.input_size
        tiles = tile_plan(H, W, (in_h, in_w), overlap, overview, B)
        T = len(tiles)
        assert T <= self._max_batch, f"{T} tiles exceed max_batch {self._max_batch}"
        frames = self.ctx.to_device(images) if frames is None else frames
        det_in = self.ctx.empty((T, in_h, in_w, 3), np.uint8)
        check(self.ctx.lib.fid_tile_cut(self.ctx.handle, C.c_void_p(frames.ptr), B, H, W, tiles.ctypes.data_as(_lib.c_i32_p), T,
                                        C.c_void_p(det_in.ptr), in_h, in_w))
        cn = self._run_net(det_in, T, (in_h, in_w))
        post = self._postprocessor()
        post.run_tiled(HeadViews.from_fused(cn), tiles, B, (in_h, in_w), (H, W), self.conf_thres, self.iou_thres, edge_margin, max_num,
                       0 if metric == "max" else 1, self._num_anchors)
        return post.fetch(B)

    def tiled_frames_per_chunk(self, H, W, overlap=128, overview=True) -> int:
        """whole frames of H x W whose tiles fit one detector run of max_batch"""
        from ..pipeline import tile_plan
        in_w, in_h = self.input_size
        per_frame = len(tile_plan(H, W, (in_h, in_w), overlap, overview, 1))
        if per_frame > self._max_batch:
            raise ValueError(f"a {W}x{H} frame has {per_frame} tiles at overlap {overlap}: more than max_batch = {self._max_batch}")
        return self._max_batch // per_frame

    def detect_batch_tiled(self, images, max_num=0, metric="max", overlap=128, edge_margin=8, overview=True):
        """detect_batch for uniform-size frames larger than the input: images uint8 [B,H,W,3] (or a list of equal shapes) ->
        [(det[K,5], kpss[K,5,2])] per frame.  Tiles run in chunks of whole frames that fit `max_batch`."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        assert images.ndim == 4 and images.shape[3] == 3, images.shape
        step = self.tiled_frames_per_chunk(images.shape[1], images.shape[2], overlap, overview)
        results = []
        for b0 in range(0, images.shape[0], step):
            results += self._detect_chunk_tiled(images[b0:b0 + step], max_num, metric, overlap, edge_margin, overview)
        return results

    def detect_tiled(self, image, max_num=0, metric="max", overlap=128, edge_margin=8, overview=True):
        """detect() with the frame cut into overlapping native-resolution tiles plus (overview) one letterboxed tile of the whole frame;
        (det, kpss) as detect returns them.  Faces up to overlap - 2 * edge_margin pixels are found whole by a native tile."""
        (det, kpss), = self.detect_batch_tiled(np.ascontiguousarray(image, dtype=np.uint8)[None], max_num, metric, overlap, edge_margin, overview)
        return det, kpss

    def detect(self, image, max_num=0, metric="max"):
        """scrfd.py:122-178: (det float32 [K,5], kpss float32 [K,5,2]); K may be 0."""
        (det, kpss), = self._detect_chunk(np.ascontiguousarray(image, dtype=np.uint8)[None], max_num, metric)
        return det, kpss

    def nms(self, dets, iou_thres):
        """scrfd.py:180-207: indices of the kept rows of dets [K,5], best score first."""
        dets = np.ascontiguousarray(dets, dtype=np.float32)
        K = dets.shape[0]
        if K == 0:
            return []
        d = self.ctx.to_device(dets)
        keep = self.ctx.empty((K,), np.int32)
        cnt = self.ctx.empty((1,), np.int32)
        check(self.ctx.lib.fid_nms(self.ctx.handle, C.c_void_p(d.ptr), K, float(iou_thres), C.c_void_p(keep.ptr),
                                   C.c_void_p(cnt.ptr)))
        n = int(cnt.download()[0])
        return [np.int64(i) for i in keep.download()[:n]]
