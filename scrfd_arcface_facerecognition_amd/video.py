"""Batched video front end: the step BEFORE the hot path.  The reference reads one frame,
processes it, reads the next (main.py:174-184; main2.py:91-99 for two cameras).  Here frames are collected
into batches in pinned host memory and uploaded on a separate HIP stream while the previous batch is being
processed (double buffering); non-640x640 frames (e.g. 1080p) are letterboxed on the device by the pipeline."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Iterator, List

import numpy as np

from ._lib import Context, Nv12Frames, check
from .engine import Gallery
from .pipeline import FacePipeline, TrackedFacePipeline


class _Pinned:
    def __init__(self, ctx: Context, shape, dtype):
        self.ctx = ctx
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        check(ctx.lib.fid_pinned_alloc(ctx.handle, self.nbytes, C.byref(p)))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr)).view(dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.ctx.lib.fid_pinned_free(self.ctx.handle, C.c_void_p(self.ptr))
            self.ptr = None


class StreamRunner:
    """Runs `pipe` over an iterable of uint8 BGR frames of one size, `pipe.B` frames per step, yielding
    per-frame face lists (FacePipeline.results) in frame order.  Upload of batch i+1 overlaps compute of batch i.
    An item of the iterable may also be a `(stream_id, frame)` pair -- several cameras in one iterable, each camera's frames in time
    order --: a TrackedFacePipeline keeps the cameras' tracks apart by it (a bare frame is camera 0) and is told which frames of a ragged
    last batch are padding, so that they age no track; any other pipeline treats every frame on its own, as before.  With a pipe built
    with best_shot=True, run() ends with `pipe.finish_all()` and `finished()` hands out the ended tracks' best shots.
    annotate=True: every step is followed by `pipe.draw` on the device (boxes, names, scores; `style`: _lib.DrawStyle), the frames are
    downloaded once per batch, and the runner yields `(faces, annotated_frame)` pairs -- the reference's output video (main.py:174-184).
    pixel_format="nv12": the items are a decoder's NV12 frames, uint8 [H*3//2, W] (H rows of Y, then H/2 rows of interleaved U, V; H and W
    even; `standard`: "bt601", "bt709" or "bt601_full"), staged and uploaded as they are -- half the bytes of BGR -- and read by the
    pipeline's *_nv12 stages; no BGR frame is built unless annotate=True, which draws on (and downloads) the pipeline's converted buffer.
    annotate_format="nv12" (with annotate=True): the annotated frames are yielded as NV12, uint8 [H*3//2, W] -- what an encoder takes --, half
    the bytes to download.  NV12 items are drawn in place on the staging buffer's two planes (`pipe.draw(..., out="nv12")`: no BGR frame at
    all; the draw follows the step's last reader, and the download precedes the enqueue of that buffer's next upload, as on the BGR
    path); BGR items are drawn in place and converted once on the device, `standard` then being the output's standard.  H and W even.
    redact (a _lib.RedactStyle, with annotate=True): `pipe.draw(..., redact=redact)`: the faces the style selects -- by default those the
    match did not name -- are hidden behind a mosaic or a solid fill on the frame that is yielded, under the boxes and names, and nowhere
    else: the step's readers (the warp, measure, the best-shot crops) have run on the clean frames before.
    `upload_bytes` is what one step uploads, `download_bytes` what one annotated step downloads (0 without annotate)."""

    def __init__(self, pipe: FacePipeline, gallery: Gallery, frame_hw, similarity_thresh: float = 0.4, annotate: bool = False, style=None,
                 pixel_format: str = "bgr", standard: str = "bt601", annotate_format: str = "bgr", redact=None):
        if pixel_format not in ("bgr", "nv12"):
            raise ValueError(f"pixel_format must be 'bgr' or 'nv12', not {pixel_format!r}")
        if annotate_format not in ("bgr", "nv12"):
            raise ValueError(f"annotate_format must be 'bgr' or 'nv12', not {annotate_format!r}")
        if redact is not None and not annotate:
            raise ValueError("redact needs annotate=True: the redacted frames are the annotated ones the runner yields")
        self.redact = redact
        self.pipe, self.gallery, self.thr = pipe, gallery, float(similarity_thresh)
        self.annotate, self.style = bool(annotate), style
        self.H, self.W = int(frame_hw[0]), int(frame_hw[1])
        self.nv12 = pixel_format == "nv12"
        self.out = "nv12" if annotate_format == "nv12" else None   # what pipe.draw is asked for
        if (self.nv12 or self.out) and (self.H % 2 or self.W % 2):
            raise ValueError(f"NV12 frames have even sizes, not {self.W}x{self.H}")
        ctx = pipe.ctx
        shape = (pipe.B, self.H * 3 // 2, self.W) if self.nv12 else (pipe.B, self.H, self.W, 3)
        self.host = [_Pinned(ctx, shape, np.uint8) for _ in range(2)]
        self.dev = [ctx.empty(shape, np.uint8) for _ in range(2)]
        # what a step hands to the pipeline: the staging buffer itself, or the NV12 view of it (dense layout)
        self.frames = [Nv12Frames(d, self.H, self.W, standard=standard) for d in self.dev] if self.nv12 else self.dev
        self.upload_bytes = self.host[0].nbytes
        self.download_bytes = pipe.B * self.H * self.W * 3 // (2 if self.out else 1) if self.annotate else 0
        if self.out and not self.nv12:
            pipe.nv12_standard = standard
        self.tracked = isinstance(pipe, TrackedFacePipeline)
        self.stream = [np.zeros(pipe.B, np.int32) for _ in range(2)]      # camera of every frame of a staging buffer, -1 = padding

    def _upload(self, k: int):
        """copy pinned buffer k -> device buffer k on the upload stream; waits only for the last step that read dev[k]"""
        ctx = self.pipe.ctx
        check(ctx.lib.fid_upload_async_slot(ctx.handle, k, C.c_void_p(self.dev[k].ptr), C.c_void_p(self.host[k].ptr),
                                            self.host[k].nbytes))

    def run(self, frames: Iterable[np.ndarray]) -> Iterator[List]:
        ctx, B = self.pipe.ctx, self.pipe.B
        it = iter(frames)

        def fill(k):
            n = 0
            for f in it:
                sid = 0
                if isinstance(f, tuple):
                    sid, f = f
                self.host[k].array[n] = f
                self.stream[k][n] = sid
                n += 1
                if n == B:
                    break
            if 0 < n < B:
                self.host[k].array[n:] = 0          # ragged tail: black frames, their results are dropped
                if self.nv12:
                    self.host[k].array[n:, self.H:] = 128           # (black in NV12: Y = 0 with neutral chroma)
                self.stream[k][n:] = -1
            return n

        cur = 0
        n_cur = fill(cur)
        if n_cur:
            self._upload(cur)
        while n_cur:
            check(ctx.lib.fid_upload_wait_slot(ctx.handle, cur))   # compute waits for batch `cur` (no host sync)
            if self.tracked:
                self.pipe.run_step(self.frames[cur], self.H, self.W, self.gallery, self.thr, stream=self.stream[cur].copy())
            else:
                self.pipe.run_step(self.frames[cur], self.H, self.W, self.gallery, self.thr)
            if self.annotate:                                       # the step's last reader of the clean frames has run
                # (BGR out of NV12 items: the pipeline's converted buffer; NV12 out of NV12 items: dev[cur] itself, drawn in place)
                if self.redact is not None:
                    drawn_dev = self.pipe.draw(self.frames[cur], self.H, self.W, self.gallery, self.style, out=self.out, redact=self.redact)
                else:
                    drawn_dev = self.pipe.draw(self.frames[cur], self.H, self.W, self.gallery, self.style, out=self.out)
                if self.out:
                    drawn_dev = drawn_dev.buf
            check(ctx.lib.fid_upload_release(ctx.handle, cur))     # dev[cur] is free again once this step has run
            nxt = cur ^ 1
            n_nxt = fill(nxt)                                       # host fills the other pinned buffer meanwhile
            if n_nxt:
                self._upload(nxt)                                   # dev[nxt]'s last reader was step i-1: starts NOW, beside step i
            res = self.pipe.results(self.gallery)                   # synchronises on batch `cur`
            if self.annotate:
                drawn = drawn_dev.download()                        # (dev[cur]'s next upload is enqueued only after this batch has been yielded)
                for r, frame in zip(res[:n_cur], drawn):
                    yield r, frame
            else:
                for r in res[:n_cur]:
                    yield r
            cur, n_cur = nxt, n_nxt
        if self.tracked and self.pipe.best_shot:
            self.pipe.finish_all()                                  # the video is over: every live track becomes a finished record

    def finished(self, clear: bool = True):
        """TrackedFacePipeline.finished of a pipe built with best_shot=True: the tracks that have ended, run()'s end included"""
        return self.pipe.finished(clear=clear, names=getattr(self.gallery, "names", None))

    def close(self):
        for h in self.host:
            h.free()
