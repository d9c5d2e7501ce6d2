"""Host-side handles over the C-ABI: a compiled conv net, the SCRFD post-process, alignment and the
gallery.  Everything here only moves pointers and shapes; all arithmetic happens in libfaceid.so."""
from __future__ import annotations

import ctypes as C
import functools
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import Context, DeviceBuffer, check
from .archs import ARCHS, ONNX_BASENAMES, Net, synth_params
from .lower import Lowered, lower


class CompiledNet:
    """fid_net: layer table + packed weights resident on one device.  The session.run replacement
    (reference models/scrfd.py:83, models/arcface.py:51)."""

    def __init__(self, ctx: Context, net: Net, params: Dict[str, np.ndarray], max_batch: int = 64):
        self.ctx = ctx
        self.net = net
        self.low: Lowered = lower(net, params)
        self.max_batch = int(max_batch)
        ops = np.ascontiguousarray(self.low.ops, dtype=np.int32)
        tens = np.ascontiguousarray(self.low.tensors, dtype=np.int32)
        h = C.c_void_p()
        blob = self.low.blob
        check(ctx.lib.fid_net_create(ctx.handle, ops.ctypes.data_as(_lib.c_i32_p), ops.shape[0],
                                     tens.ctypes.data_as(_lib.c_i32_p), tens.shape[0], blob, len(blob),
                                     net.in_hw[0], net.in_hw[1], self.max_batch, C.byref(h)))
        self.handle = h
        self.in_hw = tuple(net.in_hw)
        self._in_buf: Optional[DeviceBuffer] = None

    # -- running ----------------------------------------------------------------------------
    def run_device(self, images_dev, batch: int):
        """images_dev: device pointer to uint8 BGR [batch, H, W, 3]"""
        check(self.ctx.lib.fid_net_run(self.ctx.handle, self.handle, _lib._ptr(images_dev), int(batch)))

    def run(self, images: np.ndarray):
        """images: uint8 [B,H,W,3] host array (B <= max_batch)."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        assert images.ndim == 4 and images.shape[1:3] == self.in_hw and images.shape[3] == 3, images.shape
        if self._in_buf is None or self._in_buf.nbytes < images.nbytes:
            self._in_buf = self.ctx.empty((self.max_batch,) + images.shape[1:], np.uint8)
        check(self.ctx.lib.fid_memcpy_h2d(self.ctx.handle, C.c_void_p(self._in_buf.ptr),
                                          images.ctypes.data_as(C.c_void_p), images.nbytes))
        self.ctx.sync()
        self.run_device(self._in_buf, images.shape[0])
        return images.shape[0]

    def run_profiled(self, images_dev, batch: int) -> np.ndarray:
        ms = np.zeros(len(self.low.op_names), dtype=np.float32)
        check(self.ctx.lib.fid_net_run_profiled(self.ctx.handle, self.handle, _lib._ptr(images_dev), int(batch),
                                                ms.ctypes.data_as(_lib.c_f32_p)))
        return ms

    def set_sub_batch(self, n: int):
        """images per depth-first pass of run / run_device (fid_net_set_sub_batch; 0 = every layer on the whole batch)"""
        check(self.ctx.lib.fid_net_set_sub_batch(self.handle, int(n)))

    # -- tensors ----------------------------------------------------------------------------
    def tensor(self, name: str):
        """(device pointer, (H, W, C, C_stored), dtype) of a tensor of the last run."""
        p = C.c_void_p()
        dims = (C.c_int * 4)()
        dt = C.c_int()
        check(self.ctx.lib.fid_net_tensor(self.handle, self.low.tensor_id[name], C.byref(p), dims, C.byref(dt)))
        return p.value, tuple(dims), (np.float32 if dt.value == 1 else np.float16)

    def read(self, name: str, batch: int) -> np.ndarray:
        """Download tensor `name` as float32 [batch, H, W, C] (channel padding stripped)."""
        ptr, (H, W, Cc, Cp), dt = self.tensor(name)
        buf = self.ctx.borrow(ptr, (batch, H, W, Cp), dt)
        return buf.download()[..., :Cc].astype(np.float32)

    def save_plan(self, path: str):
        """append this net's kernel picks (per conv op and batch size) to a plan file"""
        check(self.ctx.lib.fid_net_plan_save(self.handle, str(path).encode()))

    def load_plan(self, path: str) -> int:
        """install the picks of a plan file that match this device and layer table; returns how many"""
        n = C.c_int()
        check(self.ctx.lib.fid_net_plan_load(self.handle, str(path).encode(), C.byref(n)))
        return n.value

    def plans(self) -> List[dict]:
        """the kernel pick of every conv op that has run so far: [{op, name, batch, gen, bm, bn, bk, ksplit, ns}] (parsed from
        fid_net_plan_save's lines; tests use it to check WHICH kernel family produced a result)"""
        import os
        import tempfile
        fd, path = tempfile.mkstemp(suffix=".plan")
        os.close(fd)
        try:
            self.save_plan(path)
            out = []
            with open(path) as f:
                for line in f:
                    parts = line.rstrip("\n").split("|")
                    if len(parts) != 5:
                        continue
                    v = [int(x) for x in parts[4].split()]
                    oi = int(parts[2])
                    out.append(dict(op=oi, name=self.low.op_names[oi], batch=int(parts[3]), gen=v[0], bm=v[1], bn=v[2], bk=v[3],
                                    ksplit=v[4], ns=v[5]))
            return out
        finally:
            os.unlink(path)

    def macs_per_image(self) -> float:
        v = C.c_double()
        check(self.ctx.lib.fid_net_macs(self.handle, C.byref(v)))
        return v.value

    def close(self):
        if self.handle:
            self.ctx.lib.fid_net_destroy(self.ctx.handle, self.handle)
            self.handle = None


def resolve_model(model_path: str, in_hw=None):
    """model_path -> (Net, params).  Accepted:
      'synthetic:<arch>[?seed=N]'   seeded random-init weights of a known architecture
      '<file>.npz'                  parameters saved by save_params() (+ key '__arch__')
      '<file>.onnx'                 a real ONNX file (weights read by onnx_reader, no onnx/ORT needed)
    Like onnxruntime, a missing file raises (reference models/scrfd.py:66-68 prints and re-raises)."""
    import os
    if model_path is None:
        raise ValueError("model_path is required")
    if model_path.startswith("synthetic:"):
        spec = model_path[len("synthetic:"):]
        arch, _, q = spec.partition("?")
        seed = 0
        for kv in q.split("&"):
            if kv.startswith("seed="):
                seed = int(kv[5:])
        if arch not in ARCHS:
            raise ValueError(f"unknown architecture {arch!r}; known: {sorted(ARCHS)}")
        net = ARCHS[arch](in_hw) if in_hw else ARCHS[arch]()
        return net, synth_params(net, seed)
    if not os.path.exists(model_path):
        raise FileNotFoundError(f"model file not found: {model_path}")
    if model_path.endswith(".npz"):
        z = np.load(model_path, allow_pickle=False)
        arch = str(z["__arch__"])
        net = ARCHS[arch](in_hw) if in_hw else ARCHS[arch]()
        return net, {k: z[k] for k in z.files if k != "__arch__"}
    if model_path.endswith(".onnx"):
        from .onnx_reader import load_onnx_model
        return load_onnx_model(model_path, in_hw)
    raise ValueError(f"unsupported model file {model_path}")


def save_params(path: str, arch: str, params: Dict[str, np.ndarray]):
    np.savez(path, __arch__=np.array(arch), **params)


class HeadViews:
    """The 9 strided views fid_scrfd_postprocess reads (include/faceid.h)."""

    def __init__(self, ptrs: Sequence[int], pix: Sequence[int], anc: Sequence[int], bstride: Sequence[int]):
        self.ptrs = (C.c_void_p * 9)(*[C.c_void_p(int(p)) for p in ptrs])
        self.pix = (C.c_int32 * 9)(*[int(v) for v in pix])
        self.anc = (C.c_int32 * 9)(*[int(v) for v in anc])
        self.bstride = (C.c_int64 * 9)(*[int(v) for v in bstride])

    @staticmethod
    def from_onnx_layout(bufs: Sequence[DeviceBuffer], A: int = 2):
        """bufs: 9 device arrays [B, N_l, 1|4|10] in the ONNX output order (scores, bbox, kps)."""
        ptrs, pix, anc, bs = [], [], [], []
        for k, b in enumerate(bufs):
            c = (1, 4, 10)[k // 3]
            ptrs.append(b.ptr)
            pix.append(A * c)
            anc.append(c)
            bs.append(b.shape[1] * c)
        return HeadViews(ptrs, pix, anc, bs)

    @staticmethod
    def from_fused(cnet: CompiledNet):
        """Views into the executor's fused fp32 head tensors [B, H, W, 32]."""
        ptrs, pix, anc, bs = [None] * 9, [0] * 9, [0] * 9, [0] * 9
        for li, name in enumerate(cnet.low.outputs):
            h = cnet.low.heads[name]
            base, (H, W, _, Cp), dt = cnet.tensor(name)
            assert dt == np.float32
            for part, (off, c) in enumerate((h["score"], h["bbox"], h["kps"])):
                k = part * 3 + li
                ptrs[k] = base + off * 4
                pix[k] = Cp
                anc[k] = c
                bs[k] = H * W * Cp
        return HeadViews(ptrs, pix, anc, bs)


class PostProcessor:
    """fid_scrfd_postprocess with persistent output buffers."""

    def __init__(self, ctx: Context, max_batch: int, cap: int = 256, cand_cap: int = 4096):
        self.ctx, self.cap, self.max_batch = ctx, int(cap), int(max_batch)
        self.det = ctx.empty((max_batch, cap, 5), np.float32)
        self.kps = ctx.empty((max_batch, cap, 10), np.float32)
        self.counts = ctx.empty((max_batch,), np.int32)
        self.cand_cap = int(cand_cap)
        check(ctx.lib.fid_scrfd_set_candidate_capacity(ctx.handle, self.cand_cap))

    def run(self, hv: HeadViews, B, in_hw, img_hw, conf, iou, max_num=0, metric=0, A=2):
        assert B <= self.max_batch
        check(self.ctx.lib.fid_scrfd_postprocess(
            self.ctx.handle, C.cast(hv.ptrs, _lib.c_void_pp), hv.pix, hv.anc, hv.bstride, int(B), int(in_hw[0]),
            int(in_hw[1]), int(A), int(img_hw[0]), int(img_hw[1]), float(conf), float(iou), int(max_num),
            int(metric), C.c_void_p(self.det.ptr), C.c_void_p(self.kps.ptr), C.c_void_p(self.counts.ptr), self.cap))

    def run_ragged(self, hv: HeadViews, B, in_hw, hw, conf, iou, max_num=0, metric=0, A=2):
        """run() for a mixed-size batch: frame b is the letterbox of an hw[b] = (H_b, W_b) image (fid_scrfd_postprocess_ragged)"""
        assert B <= self.max_batch
        hw = np.ascontiguousarray(hw, dtype=np.int32).reshape(-1, 2)
        assert len(hw) == B, (hw.shape, B)
        check(self.ctx.lib.fid_scrfd_postprocess_ragged(
            self.ctx.handle, C.cast(hv.ptrs, _lib.c_void_pp), hv.pix, hv.anc, hv.bstride, int(B), int(in_hw[0]),
            int(in_hw[1]), int(A), hw.ctypes.data_as(_lib.c_i32_p), float(conf), float(iou), int(max_num),
            int(metric), C.c_void_p(self.det.ptr), C.c_void_p(self.kps.ptr), C.c_void_p(self.counts.ptr), self.cap))

    def run_tiled(self, hv: HeadViews, tiles, B, in_hw, img_hw, conf, iou, edge_margin=8, max_num=0, metric=0, A=2):
        """run() for tiled detection (fid_scrfd_postprocess_tiled): the heads hold the T tiles of `tiles` (host int32 [T,6], pipeline.tile_plan),
        det / kps / counts the B frames they were cut from, in frame coordinates; edge_margin < 0 keeps the candidates at a tile's cut edges"""
        assert B <= self.max_batch
        tiles = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 6)
        check(self.ctx.lib.fid_scrfd_postprocess_tiled(
            self.ctx.handle, C.cast(hv.ptrs, _lib.c_void_pp), hv.pix, hv.anc, hv.bstride, tiles.ctypes.data_as(_lib.c_i32_p), len(tiles),
            int(in_hw[0]), int(in_hw[1]), int(A), int(B), int(img_hw[0]), int(img_hw[1]), float(conf), float(iou), int(edge_margin),
            int(max_num), int(metric), C.c_void_p(self.det.ptr), C.c_void_p(self.kps.ptr), C.c_void_p(self.counts.ptr), self.cap))

    def check(self) -> int:
        m = C.c_int()
        check(self.ctx.lib.fid_scrfd_check(self.ctx.handle, C.byref(m)))
        return m.value

    def fetch(self, B) -> List:
        """[(det[K,5], kps[K,5,2])] per frame, host arrays (synchronises)."""
        self.check()
        counts = self.counts.download()[:B]
        det = self.det.download()
        kps = self.kps.download()
        return [(det[b, :counts[b]].copy(), kps[b, :counts[b]].reshape(-1, 5, 2).copy()) for b in range(B)]


class Gallery:
    """fid_gallery: unit-length fp16 rows in HBM (what build_targets collects, reference main.py:78-105)."""

    def __init__(self, ctx: Context, embeddings: np.ndarray, names: Optional[Sequence[str]] = None):
        emb = np.ascontiguousarray(embeddings, dtype=np.float32)
        assert emb.ndim == 2
        self.ctx = ctx
        self.G, self.dim = emb.shape
        self.names = list(names) if names is not None else [str(i) for i in range(self.G)]
        h = C.c_void_p()
        check(ctx.lib.fid_gallery_create(ctx.handle, emb.ctypes.data_as(C.c_void_p), self.G, self.dim, C.byref(h)))
        self.handle = h
        gp = C.c_int()
        check(ctx.lib.fid_gallery_info(h, None, C.byref(gp), None))
        self.Gp = gp.value
        self._quant = None              # True while the int8 copy of the coarse search (fid_gallery_quantize) is current; VectorGallery keeps it

    def match_device(self, q_f16_dev, n, thresh, idx_dev, score_dev):
        check(self.ctx.lib.fid_match(self.ctx.handle, self.handle, _lib._ptr(q_f16_dev), int(n), float(thresh),
                                     _lib._ptr(idx_dev), _lib._ptr(score_dev)))

    def labels(self) -> "LabelTable":
        """the names of this gallery's rows as a device label table (default colours), built once"""
        if getattr(self, "_labels", None) is None:
            self._labels = LabelTable(self.ctx, self.names)
        return self._labels

    def close(self):
        if getattr(self, "_labels", None) is not None:
            self._labels.close()
            self._labels = None
        if self.handle:
            self.ctx.lib.fid_gallery_destroy(self.ctx.handle, self.handle)
            self.handle = None


class LabelTable:
    """fid_labels: per gallery row the name the overlay prints (its first FID_LABEL_MAX bytes; UTF-8 for a str) and a BGR colour, device
    resident -- what fid_draw_faces looks an identity up in.  colors: [G,3] BGR or None (a fixed colour per row index)."""

    def __init__(self, ctx: Context, names: Sequence, colors=None):
        self.ctx, self.G = ctx, len(names)
        raw, offsets, bgr = _lib.label_arrays(names, colors)
        h = C.c_void_p()
        check(ctx.lib.fid_labels_create(ctx.handle, raw, offsets.ctypes.data_as(_lib.c_i32_p),
                                        bgr.ctypes.data_as(C.c_void_p) if bgr is not None else None, self.G, C.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            self.ctx.lib.fid_labels_destroy(self.ctx.handle, self.handle)
            self.handle = None


class VectorGallery:
    """An updatable gallery with top-k search: the role QdrantManager plays in the reference's product layer
    (qdrant_manager.py:91-212: add_embedding / search_similar(limit, score_threshold) / delete_embedding),
    kept in HBM as unit fp16 rows.  Ids are arbitrary hashables; rows freed by delete() are reused."""

    def __init__(self, ctx: Context, dim: int = 512, capacity: int = 1024):
        self.ctx, self.dim = ctx, int(dim)
        self._gal = Gallery(ctx, np.zeros((int(capacity), dim), np.float32))
        self.row_of: Dict[object, int] = {}
        self.id_of: Dict[int, object] = {}
        self._free = list(range(int(capacity) - 1, -1, -1))

    def __len__(self):
        return len(self.row_of)

    def _grow(self):
        old = self._gal
        cap = old.G * 2
        rows = self.ctx.borrow(_gallery_ptr(old), (old.Gp, self.dim), np.float16).download()[:old.G].astype(np.float32)
        new = Gallery(self.ctx, np.concatenate([rows, np.zeros((cap - old.G, self.dim), np.float32)]))
        self._free = list(range(cap - 1, old.G - 1, -1)) + self._free
        old.close()
        self._gal = new
        if old._quant is not None:   # the int8 copy of the coarse search follows the store
            self._quantise()

    def upsert(self, ids, embeddings):
        emb = np.ascontiguousarray(embeddings, dtype=np.float32).reshape(len(ids), self.dim)
        rows = []
        for i in ids:
            if i not in self.row_of:
                if not self._free:
                    self._grow()
                r = self._free.pop()
                self.row_of[i], self.id_of[r] = r, i
            rows.append(self.row_of[i])
        rows = np.asarray(rows, dtype=np.int32)
        check(self.ctx.lib.fid_gallery_set_rows(self.ctx.handle, self._gal.handle, rows.ctypes.data_as(_lib.c_i32_p),
                                                emb.ctypes.data_as(C.c_void_p), len(rows)))

    def delete(self, ids):
        rows = np.asarray([self.row_of.pop(i) for i in ids], dtype=np.int32)
        for r in rows:
            self.id_of.pop(int(r))
            self._free.append(int(r))
        zeros = np.zeros((len(rows), self.dim), np.float32)
        check(self.ctx.lib.fid_gallery_set_rows(self.ctx.handle, self._gal.handle, rows.ctypes.data_as(_lib.c_i32_p),
                                                zeros.ctypes.data_as(C.c_void_p), len(rows)))

    TOPK_MAX = 32                   # FID_TOPK_MAX of include/faceid.h
    MATRIX_KS = (1, 2, 4, 5, 8)     # the k fid_gallery_topk serves

    def _quantise(self):
        """(re)build the gallery's int8 copy (fid_gallery_quantize); upsert / delete keep it current through fid_gallery_set_rows"""
        check(self.ctx.lib.fid_gallery_quantize(self.ctx.handle, self._gal.handle))
        self._gal._quant = True

    def _quant_stale(self):
        """a call wrote gallery rows on the device, which does not refresh the int8 copy: the next coarse search rebuilds it"""
        if self._gal._quant:
            self._gal._quant = False

    def search(self, embeddings, k: int = 5, score_threshold: float = 0.0, via: Optional[str] = None, rerank: int = 32):
        """-> per query a list of (id, score), best first (at most k, only scores > max(0, threshold)).
        via=None: fid_gallery_topk (the score matrix in scratch) for the k it serves, the fused fid_gallery_search for every other k up to 32;
        via="fused" / "matrix" force one of them (equal answers; which is the faster default is tools/bench_topk.py's question).
        via="coarse": fid_gallery_search_coarse -- an int8 scan shortlists `rerank` rows per query (k <= rerank <= 32), which are rescored from the
        fp16 rows.  Every reported score is the exact one; a row whose coarse score is not among the `rerank` best is missed.  The int8 copy is
        built on first use.  Never chosen by via=None."""
        k = int(k)
        if via not in (None, "fused", "matrix", "coarse"):
            raise ValueError("via must be None, 'fused', 'matrix' or 'coarse', not %r" % (via,))
        if k < 1 or k > self.TOPK_MAX:
            raise ValueError("k = %d is outside 1 .. %d: range_search returns every hit at or above a threshold" % (k, self.TOPK_MAX))
        if via == "matrix" and k not in self.MATRIX_KS:
            raise ValueError("via='matrix' serves k in %s only, not %d" % (self.MATRIX_KS, k))
        fn = self.ctx.lib.fid_gallery_topk if via == "matrix" or (via is None and k in self.MATRIX_KS) else self.ctx.lib.fid_gallery_search
        if via == "coarse":
            rerank = int(rerank)
            if rerank < k or rerank > self.TOPK_MAX:
                raise ValueError("rerank = %d is outside k = %d .. %d" % (rerank, k, self.TOPK_MAX))
            if not self._gal._quant:
                self._quantise()
            lib = self.ctx.lib
            fn = lambda c, g, q, n, k, t, i, s: lib.fid_gallery_search_coarse(c, g, q, n, k, rerank, t, i, s)
        emb = np.ascontiguousarray(embeddings, dtype=np.float32).reshape(-1, self.dim)
        n = emb.shape[0]
        e = self.ctx.to_device(emb)
        q = self.ctx.empty((n, self.dim), np.float16)
        check(self.ctx.lib.fid_l2_normalize_f16(self.ctx.handle, C.c_void_p(e.ptr), n, self.dim, C.c_void_p(q.ptr)))
        idx, sc = self.ctx.empty((n, k), np.int32), self.ctx.empty((n, k), np.float32)
        check(fn(self.ctx.handle, self._gal.handle, C.c_void_p(q.ptr), n, k, float(score_threshold), C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)))
        I, S = idx.download(), sc.download()
        return [[(self.id_of[int(j)], float(s)) for j, s in zip(I[r], S[r]) if j >= 0] for r in range(n)]


    # ---- the product layer's duplicate logic on top of search ("duplicate check @0.95, merge @0.8") ---------------------------------
    def is_duplicate(self, embedding, duplicate_threshold: float = 0.95) -> bool:
        """the vector half of the reference's `is_duplicate_image` (smart_face_recognition.py:2632-2641; config.json
        `duplicate_similarity_threshold`): does the nearest stored embedding reach the threshold?"""
        return len(self) > 0 and len(self.search(np.asarray(embedding, np.float32).reshape(1, self.dim), k=1, score_threshold=duplicate_threshold)[0]) > 0

    def similarity_rows(self, ids) -> np.ndarray:
        """cosine similarity of the stored embeddings `ids` against EVERY row of the store, fp32 [len(ids), capacity] (free rows: 0), computed on the
        device in one GEMM per 1 024 ids (fid_cosine_matrix with the store's own unit rows as queries)"""
        gal = self._gal
        base = _gallery_ptr(gal)
        out = np.empty((len(ids), gal.G), np.float32)
        rows = np.asarray([self.row_of[i] for i in ids], dtype=np.int64)
        stage = self.ctx.empty((min(1024, max(1, len(ids))), self.dim), np.float16)
        cm = self.ctx.empty((stage.shape[0], gal.Gp), np.float32)
        unit = self.ctx.borrow(base, (gal.Gp, self.dim), np.float16).download()          # (host copy of the unit rows: the gather of arbitrary ids)
        for c0 in range(0, len(ids), stage.shape[0]):
            blk = rows[c0:c0 + stage.shape[0]]
            q = np.zeros(stage.shape, np.float16)
            q[:len(blk)] = unit[blk]
            stage.upload(q)
            check(self.ctx.lib.fid_cosine_matrix(self.ctx.handle, gal.handle, C.c_void_p(stage.ptr), len(blk), C.c_void_p(cm.ptr)))
            out[c0:c0 + len(blk)] = cm.download()[:len(blk), :gal.G]
        return out

    # ---- range search and self-join (fid_gallery_range): every hit at or above a threshold, only the records cross PCIe ------------------------
    hit_capacity = 1 << 16          # records the first call of a range search has room for; a fuller answer is fetched by a second, larger call

    def _range(self, q_ptr, n: int, threshold: float):
        """fid_gallery_range with the grow-and-repeat contract -> (pairs int32 [total, 2], scores fp32 [total]) on the host"""
        cap = max(1, int(self.hit_capacity))
        total_dev = self.ctx.empty((1,), np.uint64)
        while True:
            pairs, scores = self.ctx.empty((cap, 2), np.int32), self.ctx.empty((cap,), np.float32)
            check(self.ctx.lib.fid_gallery_range(self.ctx.handle, self._gal.handle, C.c_void_p(q_ptr), int(n), float(threshold),
                                                 C.c_void_p(pairs.ptr), C.c_void_p(scores.ptr), cap, C.c_void_p(total_dev.ptr)))
            total = int(total_dev.download()[0])
            if total <= cap:
                break
            cap = total                                   # the counter is not clipped: it names the room the answer needs
        if total == 0:
            return np.empty((0, 2), np.int32), np.empty((0,), np.float32)
        return (self.ctx.borrow(pairs.ptr, (total, 2), np.int32).download(), self.ctx.borrow(scores.ptr, (total,), np.float32).download())

    def range_search(self, embeddings, score_threshold: float):
        """-> per query a list of (id, score): EVERY stored embedding with score >= threshold (and > 0), best first, ascending row among equal
        scores -- the reference's `search_similar(k=len(persons), threshold=...)` (smart_face_recognition.py:2761-2766)"""
        emb = np.ascontiguousarray(embeddings, dtype=np.float32).reshape(-1, self.dim)
        n = emb.shape[0]
        e = self.ctx.to_device(emb)
        q = self.ctx.empty((n, self.dim), np.float16)
        check(self.ctx.lib.fid_l2_normalize_f16(self.ctx.handle, C.c_void_p(e.ptr), n, self.dim, C.c_void_p(q.ptr)))
        pairs, scores = self._range(q.ptr, n, score_threshold)
        out = [[] for _ in range(n)]
        for k in np.lexsort((pairs[:, 1], -scores, pairs[:, 0])):
            out[int(pairs[k, 0])].append((self.id_of[int(pairs[k, 1])], float(scores[k])))
        return out

    def similar_pairs(self, threshold: float):
        """-> [(id_a, id_b, score)]: every pair of stored embeddings with score >= threshold (and > 0), each once with row_of[id_a] < row_of[id_b],
        sorted by (row a, row b); the self-join of fid_gallery_range"""
        pairs, scores = self._range(0, 0, threshold)
        return [(self.id_of[int(pairs[k, 0])], self.id_of[int(pairs[k, 1])], float(scores[k])) for k in np.lexsort((pairs[:, 1], pairs[:, 0]))]

    def find_and_merge_duplicates(self, similarity_threshold: float = 0.8, via: str = "matrix"):
        """The reference's `find_and_merge_duplicates` (smart_face_recognition.py:2726-2797; config.json `merge_duplicate_threshold`) on the vector
        store: ids in ascending order; every id that is still stored absorbs all LARGER ids whose similarity reaches the threshold (their rows are
        deleted, as merge_duplicate_persons does through delete_embedding).  The G x G similarities come from the device in one pass (deletions only
        remove candidates, no embedding changes); the greedy pass over them is the reference's loop.  Returns [(kept id, deleted id, similarity)].
        via="join": the same merges from the self-join's pair list (similar_pairs + merge_from_pairs) instead of the dense matrix.
        via="device": the same merges from fid_gallery_dedup -- the greedy loop itself runs on the device, the absorbed rows are cleared there, and
        ONE download of 8 bytes per person (keeper | score | summary) comes back; the host only sorts the merge list (merges_from_keepers) and does
        delete()'s bookkeeping."""
        if via == "device":
            ids = sorted(self.row_of)
            if not ids:
                return []
            keeper, score, _ = self._dedup_call(ids, similarity_threshold, apply=True)
            merges = merges_from_keepers(ids, keeper, score)
            for _, dead, _ in merges:                                   # delete([m[1] for m in merges]) without its device call
                r = self.row_of.pop(dead)
                self.id_of.pop(r)
                self._free.append(r)
            return merges
        if via == "join":
            merges = merge_from_pairs(list(self.row_of), self.similar_pairs(similarity_threshold), similarity_threshold)
            if merges:
                self.delete([m[1] for m in merges])
            return merges
        if via != "matrix":
            raise ValueError(f"find_and_merge_duplicates: via={via!r}, expected 'matrix', 'join' or 'device'")
        ids = sorted(self.row_of)
        if len(ids) < 2:
            return []
        sims = self.similarity_rows(ids)
        col = np.asarray([self.row_of[i] for i in ids])
        alive = {i: True for i in ids}
        merges = []
        for a, p1 in enumerate(ids):
            if not alive[p1]:
                continue
            s = sims[a, col]
            for b in np.argsort(-s, kind="stable"):
                if s[b] < similarity_threshold:
                    break
                p2 = ids[int(b)]
                if p2 <= p1 or not alive[p2]:
                    continue
                alive[p2] = False
                merges.append((p1, p2, float(s[b])))
        if merges:
            self.delete([m[1] for m in merges])
        return merges

    def _dedup_call(self, ids_sorted, threshold: float, apply: bool):
        """fid_gallery_dedup on the rows of `ids_sorted` -> (keeper int32 [n], score fp32 [n], summary int32 [2]) on the host: one upload (the
        rows), one call, one download (keeper | score | summary travel as ONE buffer)"""
        n = len(ids_sorted)
        if n > DEDUP_MAX_ROWS:
            raise ValueError(f"find_and_merge_duplicates: {n} persons exceed the {DEDUP_MAX_ROWS} of one fid_gallery_dedup call; use via=\"join\"")
        ctx = self.ctx
        rows_dev = ctx.to_device(np.asarray([self.row_of[i] for i in ids_sorted], dtype=np.int32))
        out = ctx.empty((2 * n + 2,), np.int32)
        check(ctx.lib.fid_gallery_dedup(ctx.handle, self._gal.handle, C.c_void_p(rows_dev.ptr), n, C.c_float(threshold), 1 if apply else 0,
                                        C.c_void_p(out.ptr), C.c_void_p(out.ptr + 4 * n), C.c_void_p(out.ptr + 8 * n)))
        if apply:
            self._quant_stale()
        got = out.download()
        return got[:n].copy(), got[n:2 * n].view(np.float32).copy(), got[2 * n:].copy()

    def duplicate_keepers(self, threshold: float = 0.8):
        """A dry run of find_and_merge_duplicates(via="device"): -> {deleted id: (kept id, score)}; neither the store nor the gallery changes."""
        ids = sorted(self.row_of)
        if not ids:
            return {}
        keeper, score, _ = self._dedup_call(ids, threshold, apply=False)
        return {ids[k]: (ids[int(keeper[k])], float(score[k])) for k in np.nonzero(keeper >= 0)[0]}

    # ---- density clusters (fid_gallery_cluster): which stored faces are the same person, independent of the order of the rows --------------------
    def cluster(self, similarity_threshold: float = 0.45, min_samples: int = 2, ids=None) -> "ClusterResult":
        """Density clusters of the stored embeddings `ids` (default: all): two embeddings hit when their cosine is >= the threshold (and > 0); an
        embedding with at least `min_samples` embeddings within the threshold, itself counted, is a core; a cluster is a connected set of cores
        plus the borders that hang on them (include/faceid.h, fid_gallery_cluster, has the rule).  Positions are the ids in ascending order, as
        in find_and_merge_duplicates(via="device"), so a cluster's label is its lowest core id -- but, unlike that greedy walk, the partition
        does not depend on the order.  One upload (the rows), one call, one download (label | degree | via | score | summary as ONE buffer).
        The default threshold is the reference's `grouping_threshold` (config.json); it is UNCALIBRATED for clustering (score_distribution
        measures a labelled store)."""
        order = sorted(self.row_of if ids is None else ids)
        n = len(order)
        if n == 0:
            return cluster_result([], np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(6, np.int32))
        if n > CLUSTER_MAX_ROWS:
            raise ValueError(f"cluster: {n} embeddings exceed the {CLUSTER_MAX_ROWS} of one fid_gallery_cluster call")
        ctx = self.ctx
        rows_dev = ctx.to_device(np.asarray([self.row_of[i] for i in order], dtype=np.int32))
        out = ctx.empty((4 * n + 6,), np.int32)
        check(ctx.lib.fid_gallery_cluster(ctx.handle, self._gal.handle, C.c_void_p(rows_dev.ptr), n, C.c_float(similarity_threshold), int(min_samples),
                                          C.c_void_p(out.ptr), C.c_void_p(out.ptr + 4 * n), C.c_void_p(out.ptr + 8 * n),
                                          C.c_void_p(out.ptr + 12 * n), C.c_void_p(out.ptr + 16 * n)))
        got = out.download()
        return cluster_result(order, got[:n], got[n:2 * n], got[2 * n:3 * n], got[3 * n:4 * n].view(np.float32), got[4 * n:])

    # ---- score distributions (fid_gallery_score_hist): what a threshold is calibrated with -----------------------------------------------------------
    def score_distribution(self, labels, bins: int = 512, ids=None) -> "ScoreDistribution":
        """The genuine / impostor score distributions of the stored embeddings `ids` (default: all) under `labels`, a mapping id -> person (any
        hashable; a missing id or None = unlabelled, in no pair): every pair of labelled embeddings is counted once, under "same person" or
        "different persons", at the bin of its cosine (include/faceid.h, fid_gallery_score_hist, has the rule), and every embedding gets its
        hardest impostor and its weakest genuine partner.  Positions are the ids in ascending order, as in cluster.  One upload (rows | labels),
        one call, one download (hist | summary | imp_via | imp_score | gen_via | gen_score as ONE buffer).  With a power-of-two `bins` the
        count from an edge upward is exactly what `>= threshold` accepts there."""
        order = sorted(self.row_of if ids is None else ids)
        n, bins = len(order), int(bins)
        if bins < 2 or bins > HIST_MAX_BINS or bins % 2:
            raise ValueError(f"score_distribution: bins = {bins} must be even, 2 .. {HIST_MAX_BINS}")
        if n == 0:
            return ScoreDistribution([], np.zeros((2, bins), np.uint64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int32),
                                     np.zeros(0, np.float32), np.zeros(4, np.uint64))
        if n > HIST_MAX_ROWS:
            raise ValueError(f"score_distribution: {n} embeddings exceed the {HIST_MAX_ROWS} of one fid_gallery_score_hist call")
        ctx = self.ctx
        rows = np.asarray([self.row_of[i] for i in order], dtype=np.int32)
        both = ctx.to_device(np.concatenate([rows, label_codes(order, labels)]))
        words = 4 * bins + 8                                                          # hist and summary are uint64: they lead the buffer
        out = ctx.empty((words + 4 * n,), np.int32)
        at = lambda k: C.c_void_p(out.ptr + 4 * (words + k * n))
        check(ctx.lib.fid_gallery_score_hist(ctx.handle, self._gal.handle, C.c_void_p(both.ptr), C.c_void_p(both.ptr + 4 * n), n, bins,
                                             C.c_void_p(out.ptr), at(0), at(1), at(2), at(3), C.c_void_p(out.ptr + 16 * bins)))
        got = out.download()
        tail = got[words:]
        return ScoreDistribution(order, got[:4 * bins].view(np.uint64).reshape(2, bins), tail[:n], tail[n:2 * n].view(np.float32), tail[2 * n:3 * n],
                                 tail[3 * n:].view(np.float32), got[4 * bins:words].view(np.uint64))

    # ---- identity templates (fid_gallery_templates): one row per person from many stored faces --------------------------------------------------------
    def _templates_call(self, labels, weights, min_score, ids):
        """-> (TemplateResult, the device buffer that holds the call's outputs or None, the byte offset of the templates in it)"""
        order = sorted(self.row_of if ids is None else ids)
        codes = label_codes(order, labels)
        persons = persons_of(order, labels, codes)
        n, P = len(order), len(persons)
        if P == 0:
            return TemplateResult(order, [], np.zeros((0, self.dim), np.float16), np.zeros(n, np.float32), np.full(n, -1, np.int32),
                                  np.zeros((0, 4), np.int32), np.zeros(0, np.float32), np.zeros(6, np.int64)), None, 0
        if n > TEMPLATE_MAX_ROWS:
            raise ValueError(f"templates: {n} embeddings exceed the {TEMPLATE_MAX_ROWS} of one fid_gallery_templates call")
        ctx, dim = self.ctx, self.dim
        rows = np.asarray([self.row_of[i] for i in order], dtype=np.int32)
        inp = ctx.to_device(np.concatenate([rows, codes, weight_codes(order, weights)]))
        tw = P * dim // 2                                                             # int32 words of the templates
        out = ctx.empty((12 + tw + 2 * n + 5 * P,), np.int32)                         # summary (int64 [6]) | templates | score | kept | person | cohesion
        at = lambda w: C.c_void_p(out.ptr + 4 * w)
        check(ctx.lib.fid_gallery_templates(ctx.handle, self._gal.handle, C.c_void_p(inp.ptr), C.c_void_p(inp.ptr + 4 * n), C.c_void_p(inp.ptr + 8 * n),
                                            n, P, C.c_float(TEMPLATE_KEEP_ALL if min_score is None else float(min_score)), at(12), at(12 + tw),
                                            at(12 + tw + n), at(12 + tw + 2 * n), at(12 + tw + 2 * n + 4 * P), at(0)))
        got = out.download()
        per = got[12 + tw:]
        res = TemplateResult(order, persons, got[12:12 + tw].view(np.float16).reshape(P, dim), per[:n].view(np.float32), per[n:2 * n],
                             per[2 * n:2 * n + 4 * P].reshape(P, 4), per[2 * n + 4 * P:].view(np.float32), got[:12].view(np.int64))
        return res, out, 48

    def templates(self, labels, weights=None, min_score=None, ids=None) -> "TemplateResult":
        """One template per person from the stored embeddings `ids` (default: all) under `labels`, a mapping id -> person as in
        score_distribution (a missing id or None = unlabelled, in no template): the weighted mean of the person's stored rows, re-normalised,
        taken exactly in integers (include/faceid.h, fid_gallery_templates, has the rule), so the answer does not depend on the order of the
        ids.  weights: a mapping id -> quality in [0, 1] (w = clip(rint(255 q), 1, 255) for q > 0; q <= 0, NaN or a missing id: the face takes
        no part), None = equal weights.  min_score: a face whose score against its person's template is below it is dropped and the template
        taken again from the rest; None (the default) drops nothing -- no value has been measured, score_distribution is the tool to choose one
        with.  Positions are the ids in ascending order, persons are numbered in the order of their first appearance there.  One upload
        (rows | labels | weights), one call, one download."""
        return self._templates_call(labels, weights, min_score, ids)[0]

    def enroll_templates(self, labels, into: "VectorGallery", weights=None, min_score=None, ids=None) -> "TemplateResult":
        """templates(...), and every person with a non-zero template is stored in `into` (another VectorGallery of this context and dim) under
        the person as id -- a new row, or the row the id already has -- through fid_gallery_put_rows_f16: the template rows go from the call's
        output buffer into the gallery on the device, byte for byte.  A person whose template is the zero row is not enrolled (and what
        `into` holds under that id stays).  -> the TemplateResult."""
        if into.ctx is not self.ctx or into.dim != self.dim or into is self:
            raise ValueError("enroll_templates: `into` must be another store of the same context and dim")
        res, out, off = self._templates_call(labels, weights, min_score, ids)
        live = [p for p in range(len(res.persons)) if res.cohesion[p] > 0]
        if not live:
            return res
        for p in live:
            pid = res.persons[p]
            if pid not in into.row_of:
                if not into._free:
                    into._grow()
                r = into._free.pop()
                into.row_of[pid], into.id_of[r] = r, pid
        ctx, lib = self.ctx, self.ctx.lib
        rows_dev = ctx.to_device(np.asarray([into.row_of[res.persons[p]] for p in live], dtype=np.int32))
        a = 0
        while a < len(live):                                                          # one call per run of consecutive persons (one, unless a zero row lies between)
            b = a + 1
            while b < len(live) and live[b] == live[b - 1] + 1:
                b += 1
            check(lib.fid_gallery_put_rows_f16(ctx.handle, into._gal.handle, C.c_void_p(rows_dev.ptr + 4 * a),
                                               C.c_void_p(out.ptr + off + live[a] * self.dim * 2), b - a))
            a = b
        into._quant_stale()
        return res

    # ---- the visit loop (fid_gallery_group): a batch of visits grouped into persons in visit order, one call, one download ------------------------
    def _next_ids(self):
        """fresh integer ids above the largest integer id in the store"""
        k = max((i for i in self.row_of if isinstance(i, (int, np.integer)) and not isinstance(i, bool)), default=-1) + 1
        while True:
            yield int(k)
            k += 1

    def _group_call(self, q_ptr: int, n: int, new_rows, dup: float, group: float, search: float):
        """fid_gallery_group on n unit fp16 rows at device address q_ptr -> (verdict [n], row [n], score [n], summary [2]) on the host"""
        ctx = self.ctx
        rows = np.ascontiguousarray(new_rows, dtype=np.int32)
        rows_dev = ctx.to_device(rows if len(rows) else np.zeros(1, np.int32))
        verdict, row, score = ctx.empty((n,), np.int32), ctx.empty((n,), np.int32), ctx.empty((n,), np.float32)
        summary = ctx.empty((2,), np.int32)
        check(ctx.lib.fid_gallery_group(ctx.handle, self._gal.handle, C.c_void_p(q_ptr), int(n), C.c_float(dup), C.c_float(group), C.c_float(search),
                                        C.c_void_p(rows_dev.ptr), len(rows), C.c_void_p(verdict.ptr), C.c_void_p(row.ptr), C.c_void_p(score.ptr),
                                        C.c_void_p(summary.ptr)))
        self._quant_stale()
        return verdict.download(), row.download(), score.download(), summary.download()

    def group_device(self, q_f16_dev, n: int, ids=None, duplicate_threshold: float = 0.95, grouping_threshold: float = 0.45,
                     similarity_threshold: float = 0.4):
        """group_visits for n unit fp16 rows that are already on the device (a pipeline's `q`, the packed rows of get_batch): no upload, no
        normalisation.  The store grows until n rows are free, the next free rows (in `_free.pop()` order) are handed to fid_gallery_group as
        new_rows, and after ONE download of verdict / row / score / summary per call the consumed rows are bound to their ids and the unused ones
        go back to the free list in their old order.  Calls are chunked at the entry point's limit; a DEFERRED suffix is run again."""
        n = int(n)
        base = int(_lib._ptr(q_f16_dev).value or 0)
        if ids is not None and len(ids) != n:
            raise ValueError(f"group: {len(ids)} ids for {n} visits")
        if ids is not None:                                         # before anything is written: a clash found later would leave rows bound to no id
            if len(set(ids)) != n:
                raise ValueError("group: the ids are not distinct")
            taken = [i for i in ids if i in self.row_of]
            if taken:
                raise ValueError(f"group: id {taken[0]!r} is already stored")
        fresh = self._next_ids()
        first_of_empty_store = len(self) == 0
        records, pos = [], 0
        while pos < n:
            m = min(n - pos, GROUP_MAX_VISITS)
            while len(self._free) < m:
                self._grow()
            rows = [self._free.pop() for _ in range(m)]
            verdict, row, score, summary = self._group_call(base + pos * self.dim * 2, m, rows, duplicate_threshold, grouping_threshold,
                                                            similarity_threshold)
            used, decided = int(summary[0]), int(summary[1])
            self._free.extend(reversed(rows[used:]))
            if decided == 0:
                raise RuntimeError("group: the first visit of a call was deferred although a free row was offered")
            for i in range(decided):
                v = int(verdict[i])
                if v == 0:
                    pid = ids[pos + i] if ids is not None else next(fresh)
                    self.row_of[pid], self.id_of[int(row[i])] = int(row[i]), pid
                    sim = float(score[i])
                    if first_of_empty_store:
                        sim = 1.0                                   # reference smart_face_recognition.py:1825,1839
                    first_of_empty_store = False
                else:
                    pid, sim = (self.id_of[int(row[i])] if row[i] >= 0 else None), float(score[i])
                records.append({"verdict": VISIT_VERDICTS[v], "person_id": pid, "similarity": sim})
            pos += decided
        return records

    def group_visits(self, embeddings, ids=None, duplicate_threshold: float = 0.95, grouping_threshold: float = 0.45,
                     similarity_threshold: float = 0.4, via: str = "device"):
        """The reference's process_visit_data loop (smart_face_recognition.py:1769-1951) for a batch of embeddings in visit order: per visit
        is_duplicate_image (:2618-2652, `duplicate_similarity_threshold`), search_person (:1619-1643, `similarity_threshold`), grouping with
        the best hit at `grouping_threshold_file` (:1859-1861; default 0.45 = reference config.json:22) or add_person (:1531-1602).  A visit
        that becomes a new person is a candidate for every later visit of the call; a recognised one is not stored.
        -> one record per visit: {"verdict": one of VISIT_VERDICTS, "person_id": the id grouped with / duplicate of / newly assigned (None: no
        face), "similarity"}.  ids[i] = the id visit i gets if it is new (default: fresh integers above the largest integer id stored).  An
        all-zero (or non-finite) embedding is a "no face" visit.  If the store was empty, the first new person reports similarity 1.0 (:1825).
        via="device": fid_gallery_group, one call per 65 536 visits.  via="loop": the same answer by the reference's own sequence, one visit at a
        time on what existed before (fid_gallery_topk with k = 1 and k = 5, then upsert) -- the baseline of tools/bench_group.py.  The one
        difference: upsert re-normalises the fp32 embedding, the device path copies the query's fp16 row, so stored bits may differ in the
        last place."""
        emb = np.ascontiguousarray(embeddings, dtype=np.float32).reshape(-1, self.dim)
        n = emb.shape[0]
        if n == 0:
            return []
        e = self.ctx.to_device(emb)
        q = self.ctx.empty((n, self.dim), np.float16)
        check(self.ctx.lib.fid_l2_normalize_f16(self.ctx.handle, C.c_void_p(e.ptr), n, self.dim, C.c_void_p(q.ptr)))
        if via == "device":
            return self.group_device(q, n, ids, duplicate_threshold, grouping_threshold, similarity_threshold)
        if via != "loop":
            raise ValueError(f"group_visits: via={via!r}, expected 'device' or 'loop'")
        if ids is not None and (len(ids) != n or len(set(ids)) != n or any(i in self.row_of for i in ids)):
            raise ValueError(f"group: {n} distinct ids that are not stored yet are needed")
        ctx, lib = self.ctx, self.ctx.lib
        has_face = (q.download().view(np.uint16) & 0x7FFF).any(axis=1)
        fresh = self._next_ids()
        i1, s1, i5, s5 = ctx.empty((1, 1), np.int32), ctx.empty((1, 1), np.float32), ctx.empty((1, 5), np.int32), ctx.empty((1, 5), np.float32)
        records = []
        for i in range(n):
            if not has_face[i]:
                records.append({"verdict": VISIT_VERDICTS[3], "person_id": None, "similarity": 0.0})
                continue
            if len(self) == 0:                                      # :1820-1851: the first person of an empty store, similarity 1.0
                pid = ids[i] if ids is not None else next(fresh)
                self.upsert([pid], emb[i:i + 1])
                records.append({"verdict": VISIT_VERDICTS[0], "person_id": pid, "similarity": 1.0})
                continue
            qi = C.c_void_p(q.ptr + i * self.dim * 2)
            # (the searches run with threshold 0 and `>=` is applied here: Qdrant's score_threshold keeps scores >= it, fid_gallery_topk's is strict)
            check(lib.fid_gallery_topk(ctx.handle, self._gal.handle, qi, 1, 1, C.c_float(0.0), C.c_void_p(i1.ptr), C.c_void_p(s1.ptr)))
            j, s = int(i1.download()[0, 0]), float(s1.download()[0, 0])
            if j >= 0 and s >= np.float32(duplicate_threshold):
                records.append({"verdict": VISIT_VERDICTS[2], "person_id": self.id_of[j], "similarity": s})
                continue
            check(lib.fid_gallery_topk(ctx.handle, self._gal.handle, qi, 1, 5, C.c_float(0.0), C.c_void_p(i5.ptr), C.c_void_p(s5.ptr)))
            I, S = i5.download()[0], s5.download()[0]
            hits = [(int(a), float(b)) for a, b in zip(I, S) if a >= 0 and b >= np.float32(similarity_threshold)]
            sim = hits[0][1] if hits else 0.0
            if hits and sim >= np.float32(grouping_threshold):
                records.append({"verdict": VISIT_VERDICTS[1], "person_id": self.id_of[hits[0][0]], "similarity": sim})
                continue
            pid = ids[i] if ids is not None else next(fresh)
            self.upsert([pid], emb[i:i + 1])
            records.append({"verdict": VISIT_VERDICTS[0], "person_id": pid, "similarity": sim})
        return records


VISIT_VERDICTS = ("new", "recognised", "duplicate", "no face", "deferred")        # FID_VISIT_* (include/faceid.h)
GROUP_MAX_VISITS = 65536                                                          # FID_GROUP_MAX_VISITS


def visit_counters(records):
    """the reference's per-run counter dict (smart_face_recognition.py:1772-1781, summed over the visits :1967-1975) from group_visits' records:
    `processed` counts the visits that passed the duplicate check (:1817), i.e. recognised + new; the keys only the download / SQL layer can
    raise stay 0"""
    out = {"processed": 0, "recognized": 0, "new_persons": 0, "no_faces": 0, "low_quality": 0, "download_failed": 0, "duplicate_faces": 0,
           "low_similarity": 0}
    for r in records:
        v = r["verdict"]
        if v == "no face":
            out["no_faces"] += 1
        elif v == "duplicate":
            out["duplicate_faces"] += 1
        elif v == "recognised":
            out["processed"] += 1
            out["recognized"] += 1
        elif v == "new":
            out["processed"] += 1
            out["new_persons"] += 1
        else:
            raise ValueError(f"visit_counters: verdict {v!r}")
    return out


PAIR_VERDICTS = ("different", "same", "no image", "no face")                     # FID_PAIR_* (include/faceid.h)
PAIR_ERRORS = (None, None, "Could not download one or both images", "Could not detect faces in one or both images")   # :900, :919
PAIR_COUNTER_KEYS = ("processed", "same_person", "different_person", "no_image", "no_face", "labelled", "label_matches")


def pair_counters(counters) -> dict:
    """fid_pair_verify's counter slots as a dict; `errors` = no_image + no_face is the error_count of smart_face_recognition.py:1089-1090"""
    out = {k: int(v) for k, v in zip(PAIR_COUNTER_KEYS, counters)}
    out["errors"] = out["no_image"] + out["no_face"]
    return out


def verify_pairs(ctx: Context, feats1, feats2, threshold: float = 0.4, labels=None):
    """The reference's calculate_face_similarity and verdict (smart_face_recognition.py:965-982, :928-932) for P pairs at once: feats1, feats2
    host [P, D] raw fp32 embeddings (D % 4 == 0), pair p = (feats1[p], feats2[p]); labels: optional [P] of 1 / 0 / -1 (the API's approve, -1 = none).
    One upload (both matrices, the pair table and the labels travel as ONE buffer), one fid_pair_verify, one download.
    -> (score float32 [P], verdict int32 [P] (FID_PAIR_*), counters int32 [8])."""
    a, b = np.ascontiguousarray(feats1, dtype=np.float32), np.ascontiguousarray(feats2, dtype=np.float32)
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError(f"verify_pairs: feats1 {a.shape} and feats2 {b.shape} must be two [P, D] matrices of one shape")
    P, D = a.shape
    if P == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(8, np.int32)
    lab = None
    if labels is not None:
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if lab.shape[0] != P:
            raise ValueError(f"verify_pairs: {lab.shape[0]} labels for {P} pairs")
    emb_bytes = 2 * P * D * 4                                   # a multiple of 16: D % 4 == 0 is checked by the library
    host = np.empty(emb_bytes + P * 8 + (P * 4 if lab is not None else 0), np.uint8)
    host[:emb_bytes // 2] = a.view(np.uint8).reshape(-1)
    host[emb_bytes // 2:emb_bytes] = b.view(np.uint8).reshape(-1)
    pairs = np.stack([np.arange(P, dtype=np.int32), np.arange(P, 2 * P, dtype=np.int32)], axis=1)
    host[emb_bytes:emb_bytes + P * 8] = pairs.view(np.uint8).reshape(-1)
    if lab is not None:
        host[emb_bytes + P * 8:] = lab.view(np.uint8)
    inp = ctx.to_device(host)
    out = ctx.empty((2 * P + 8,), np.int32).zero()              # score [P] | verdict [P] | counters [8]
    check(ctx.lib.fid_pair_verify(ctx.handle, C.c_void_p(inp.ptr), 2 * P, D, C.c_void_p(inp.ptr + emb_bytes), P, None, 0,
                                  C.c_void_p(inp.ptr + emb_bytes + P * 8) if lab is not None else None, C.c_float(threshold),
                                  C.c_void_p(out.ptr), C.c_void_p(out.ptr + 4 * P), C.c_void_p(out.ptr + 8 * P)))
    got = out.download()
    return got[:P].view(np.float32).copy(), got[P:2 * P].copy(), got[2 * P:].copy()


def merge_from_pairs(ids, pairs, threshold: float):
    """The reference's greedy merge loop (smart_face_recognition.py:2755-2792) on a pair list [(id_a, id_b, score)] (each unordered pair at most
    once, either order): ids in ascending order; every id that is still alive absorbs each alive LARGER id it is paired with at score >= threshold,
    its hits taken score-descending, then in ascending id order (what a stable argsort over the ascending ids gives).  Pure host code.
    Returns [(kept id, deleted id, score)] in the order the merges happen."""
    hits = {i: [] for i in ids}
    for a, b, s in pairs:
        if s >= threshold:
            hits[a].append((b, s))
            hits[b].append((a, s))
    alive = set(hits)
    merges = []
    for p1 in sorted(hits):
        if p1 not in alive:
            continue
        for p2, s in sorted(hits[p1], key=lambda h: (-h[1], h[0])):
            if p2 <= p1 or p2 not in alive:
                continue
            alive.discard(p2)
            merges.append((p1, p2, float(s)))
    return merges


DEDUP_MAX_ROWS = 1 << 20                                                          # FID_DEDUP_MAX_ROWS


def merges_from_keepers(ids_sorted, keeper, score):
    """fid_gallery_dedup's answer as the reference's merge list: ids_sorted[k] is the id at position k (ascending), keeper[k] the position that
    absorbed it or -1.  A keeper makes its merges when the loop reaches it, score-descending, then in ascending id order -- so the list is the
    absorbed positions sorted by (keeper, -score, position).  Pure host code.  Returns [(kept id, deleted id, score)], as merge_from_pairs."""
    keeper = np.asarray(keeper)
    dead = [int(k) for k in np.nonzero(keeper >= 0)[0]]
    dead.sort(key=lambda k: (int(keeper[k]), -float(score[k]), k))
    return [(ids_sorted[int(keeper[k])], ids_sorted[k], float(score[k])) for k in dead]


CLUSTER_MAX_ROWS = 1 << 20                                                        # FID_CLUSTER_MAX_ROWS


class ClusterResult:
    """What fid_gallery_cluster / fid_cluster_host answer, keyed by the caller's ids (ids[k] is the id at position k):
    labels   {id: the label id of its cluster, or None}          (a cluster's label is its lowest core id)
    clusters [[ids]], ordered by label and by position inside each list
    noise    [ids] that took part and belong to no cluster;  degree {id: embeddings within the threshold, itself counted; 0 = took no part}
    via      {id: (core id, score)}: the core that reaches the id with the highest score (a border hangs on it)
    counts   {"clusters", "cores", "borders", "noise", "took_part"}
    and the raw per-position arrays label_pos / degree_pos / via_pos / score_pos / summary."""

    def __init__(self, ids, label, degree, via, score, summary):
        self.ids = list(ids)
        self.label_pos, self.degree_pos, self.via_pos = (np.array(a, np.int32) for a in (label, degree, via))
        self.score_pos, self.summary = np.array(score, np.float32), np.array(summary, np.int32)
        self.counts = dict(zip(("clusters", "cores", "borders", "noise", "took_part"), (int(v) for v in self.summary[:5])))

    # (each view is built on first use: a store of 100 000 rows is 100 000 dictionary entries per view, more than the call itself costs)
    @functools.cached_property
    def labels(self):
        ids = self.ids
        return dict(zip(ids, [ids[l] if l >= 0 else None for l in self.label_pos.tolist()]))

    @functools.cached_property
    def clusters(self):
        ids, label = self.ids, self.label_pos.tolist()
        members: Dict[int, list] = {}
        for k in np.nonzero(self.label_pos >= 0)[0].tolist():
            members.setdefault(label[k], []).append(ids[k])
        return [members[l] for l in sorted(members)]

    @functools.cached_property
    def noise(self):
        ids = self.ids
        return [ids[k] for k in np.nonzero((self.label_pos < 0) & (self.degree_pos > 0))[0].tolist()]

    @functools.cached_property
    def degree(self):
        return dict(zip(self.ids, self.degree_pos.tolist()))

    @functools.cached_property
    def via(self):
        ids, via, score = self.ids, self.via_pos.tolist(), self.score_pos.tolist()
        return {ids[k]: (ids[via[k]], score[k]) for k in np.nonzero(self.via_pos >= 0)[0].tolist()}


def cluster_result(ids, label, degree, via, score, summary) -> ClusterResult:
    """the five output arrays of a clustering call as a ClusterResult; summary[5] != 0 (a union-find loop hit its bound) raises"""
    if len(summary) > 5 and int(summary[5]) != 0:
        raise RuntimeError("fid_gallery_cluster: a union-find loop reached its bound; the labels are not to be trusted")
    return ClusterResult(ids, label, degree, via, score, summary)


HIST_MAX_ROWS = 1 << 20                                                           # FID_HIST_MAX_ROWS
HIST_MAX_BINS = 4096                                                              # FID_HIST_MAX_BINS


def label_codes(ids, labels) -> np.ndarray:
    """labels: a mapping id -> person (any hashable; a missing id or None = unlabelled) -> int32 [len(ids)]: the persons numbered in the order of
    their first appearance, -1 = unlabelled"""
    code: Dict[object, int] = {}
    out = np.full(len(ids), -1, np.int32)
    for k, i in enumerate(ids):
        person = labels.get(i)
        if person is not None:
            out[k] = code.setdefault(person, len(code))
    return out


class ScoreDistribution:
    """What fid_gallery_score_hist / fid_score_hist_host answer, keyed by the caller's ids (ids[k] is the id at position k):
    genuine, impostor  uint64 [bins]: the pairs of the same / of different persons per score bin
    edges              float64 [bins + 1]: bin b holds edges[b] <= score < edges[b + 1] (the last bin also holds score = 1; exact for a
                       power-of-two bins, see include/faceid.h)
    genuine_pairs, impostor_pairs, non_finite, took_part
    and the raw per-position arrays imp_via_pos / imp_score_pos / gen_via_pos / gen_score_pos.
    Every rate is taken at an EDGE, from the exact integer cumulative sums, with one division at the end: far(t) = the impostor pairs at or
    above the edge / all impostor pairs, frr(t) = the genuine pairs below the edge / all genuine pairs.  At the last edge (1.0) nothing is
    accepted.  An empty class makes its rates nan."""

    def __init__(self, ids, hist, imp_via, imp_score, gen_via, gen_score, summary):
        self.ids = list(ids)
        hist = np.array(hist, np.uint64).reshape(2, -1)
        self.genuine, self.impostor = hist[0].copy(), hist[1].copy()
        self.bins = int(hist.shape[1])
        self.edges = -1.0 + 2.0 * np.arange(self.bins + 1, dtype=np.float64) / self.bins
        self.imp_via_pos, self.gen_via_pos = np.array(imp_via, np.int32), np.array(gen_via, np.int32)
        self.imp_score_pos, self.gen_score_pos = np.array(imp_score, np.float32), np.array(gen_score, np.float32)
        self.summary = np.array(summary, np.uint64)
        self.took_part, self.genuine_pairs, self.impostor_pairs, self.non_finite = (int(v) for v in self.summary[:4])

    @functools.cached_property
    def _accepted(self):
        """per class, the pairs at or above every edge as Python ints [bins + 1] (the last edge accepts nothing)"""
        out = []
        for h in (self.genuine, self.impostor):
            acc, run = [0], 0
            for v in h[::-1].tolist():
                run += int(v)
                acc.append(run)
            out.append(acc[::-1])
        return out

    def _edge(self, threshold) -> int:
        """the edge at or above the argument (the last one for an argument above it)"""
        return min(int(np.searchsorted(self.edges, float(threshold), side="left")), self.bins)

    def _rates(self, e: int):
        g, i = self.genuine_pairs, self.impostor_pairs
        far = self._accepted[1][e] / i if i else float("nan")
        frr = (g - self._accepted[0][e]) / g if g else float("nan")
        return far, frr

    def far(self, threshold) -> float:
        return self._rates(self._edge(threshold))[0]

    def frr(self, threshold) -> float:
        return self._rates(self._edge(threshold))[1]

    def threshold_at_far(self, target: float):
        """-> (threshold, far, frr) at the LOWEST edge whose FAR <= target; (nan, nan, nan) without impostor pairs or for a target < 0"""
        if self.impostor_pairs:
            for e in range(self.bins + 1):                                            # (far does not rise with the edge)
                far, frr = self._rates(e)
                if far <= target:
                    return float(self.edges[e]), far, frr
        return float("nan"), float("nan"), float("nan")

    def eer(self):
        """-> (threshold, far, frr) at the edge that minimises |far - frr|, the lowest edge among equals (compared as exact integers);
        (nan, nan, nan) when a class is empty"""
        g, i = self.genuine_pairs, self.impostor_pairs
        if not g or not i:
            return float("nan"), float("nan"), float("nan")
        gap = [abs(self._accepted[1][e] * g - (g - self._accepted[0][e]) * i) for e in range(self.bins + 1)]
        e = gap.index(min(gap))
        return (float(self.edges[e]),) + self._rates(e)

    def _ranked(self, via, score, k, sign):
        pos = np.nonzero(via >= 0)[0]
        pos = pos[np.lexsort((pos, sign * score[pos].astype(np.float64)))][:max(int(k), 0)]        # ties: the lower position = the lower id
        return [(self.ids[p], self.ids[int(via[p])], float(score[p])) for p in pos.tolist()]

    def hardest_impostors(self, k: int = 10):
        """the k ids with the highest score against an id of ANOTHER person: [(id, other id, score)], score-descending -- two photographs of one
        person under two labels show up here"""
        return self._ranked(self.imp_via_pos, self.imp_score_pos, k, -1.0)

    def weakest_genuines(self, k: int = 10):
        """the k ids with the lowest score against an id of the SAME person: [(id, other id, score)], score-ascending -- a stranger filed under a
        person's label shows up here"""
        return self._ranked(self.gen_via_pos, self.gen_score_pos, k, 1.0)


TEMPLATE_MAX_ROWS = _lib.TEMPLATE_MAX_ROWS                                        # FID_TEMPLATE_MAX_ROWS
TEMPLATE_KEEP_ALL = -2.0                                                          # a min_score <= -2 keeps every member


def persons_of(ids, labels, codes) -> list:
    """the persons behind label_codes' numbers, in that order"""
    persons = [None] * (int(codes.max()) + 1 if len(codes) else 0)
    for k in np.nonzero(codes >= 0)[0].tolist():
        persons[int(codes[k])] = labels.get(ids[k])
    return persons


def weight_codes(ids, weights) -> np.ndarray:
    """weights: None (every weight 1) or a mapping id -> quality in [0, 1] -> int32 [len(ids)]: clip(rint(255 q), 1, 255) for q > 0; 0 (the
    position takes no part) for q <= 0, NaN or a missing id"""
    if weights is None:
        return np.ones(len(ids), np.int32)
    q = np.array([np.nan if weights.get(i) is None else float(weights.get(i)) for i in ids], np.float64).reshape(len(ids))
    with np.errstate(invalid="ignore"):
        return np.where(q > 0, np.clip(np.rint(255.0 * np.where(q > 0, q, 0)), 1, 255), 0).astype(np.int32)


class TemplateResult:
    """What fid_gallery_templates / fid_templates_host answer, keyed by the caller's ids (ids[k] is the id at position k) and persons:
    persons    the persons, in the order of their numbers;  templates  float16 [P, dim], row p the template of persons[p] (all zero: none)
    count, kept  int32 [P]: the faces that took part / that stayed;  cohesion  float32 [P]: the resultant length of the weighted mean of the
               faces that stayed (1 = all the same vector, 0 = no template)
    lowest, highest  per person the id of its lowest / highest scoring face (None without a face)
    scores     {id: score against its person's first template} for the faces that took part;  dropped  [ids] below min_score
    zero       [persons] without a template;  counts  {"took_part", "persons", "zero", "dropped", "rejected"}
    and the raw per-position arrays score_pos / kept_pos (1 kept, 0 dropped, -1 took no part), person_pos [P, 4], summary."""

    def __init__(self, ids, persons, templates, score, kept, person, cohesion, summary):
        self.ids, self.persons = list(ids), list(persons)
        self.templates = np.array(templates, np.float16)                                # [P, dim]
        self.score_pos, self.kept_pos = np.array(score, np.float32), np.array(kept, np.int32)
        self.person_pos = np.array(person, np.int32).reshape(-1, 4)
        self.count, self.kept = self.person_pos[:, 0].copy(), self.person_pos[:, 1].copy()
        self.cohesion, self.summary = np.array(cohesion, np.float32), np.array(summary, np.int64)
        self.counts = dict(zip(("took_part", "persons", "zero", "dropped", "rejected"), (int(v) for v in self.summary[:5])))

    def template(self, person):
        """the template of one person as float16 [dim]"""
        return self.templates[self.persons.index(person)]

    @functools.cached_property
    def scores(self):
        return {self.ids[k]: float(self.score_pos[k]) for k in np.nonzero(self.kept_pos >= 0)[0].tolist()}

    @functools.cached_property
    def dropped(self):
        return [self.ids[k] for k in np.nonzero(self.kept_pos == 0)[0].tolist()]

    @functools.cached_property
    def zero(self):
        return [self.persons[p] for p in np.nonzero(~(self.cohesion > 0))[0].tolist()]

    @functools.cached_property
    def lowest(self):
        return [self.ids[k] if k >= 0 else None for k in self.person_pos[:, 2].tolist()]

    @functools.cached_property
    def highest(self):
        return [self.ids[k] if k >= 0 else None for k in self.person_pos[:, 3].tolist()]

    def weakest(self, k: int = 10):
        """the k faces with the lowest score against their person's template, over all persons: [(id, score)], score-ascending, the lower
        position among equals -- where to look for label errors"""
        pos = np.nonzero(self.kept_pos >= 0)[0]
        pos = pos[np.lexsort((pos, self.score_pos[pos].astype(np.float64)))][:max(int(k), 0)]
        return [(self.ids[p], float(self.score_pos[p])) for p in pos.tolist()]


def _gallery_ptr(gal: Gallery) -> int:
    p = C.c_void_p()
    check(gal.ctx.lib.fid_gallery_data(gal.handle, C.byref(p)))
    return int(p.value)
