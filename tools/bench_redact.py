#!/usr/bin/env python3
"""Redaction (fid_redact_faces, fid_redact_faces_nv12) against the overlay (fid_draw_faces, fid_draw_faces_nv12) in the same run, on 1080p
frames, for docs/FINDINGS.md ("Redaction").  One process.

 kernels --frames frames of 1080 x 1920 of random bytes (BGR, and dense NV12), the face table of tools/bench_draw.py's scene: 14 seeded faces
         per frame, boxes 40 .. 160 pixels wide anywhere in the frame, every second one known, cap = 256, slots form with id_stride = 14.
         Every face is redacted (who = UNKNOWN | KNOWN), cells = 8, expand = 0.1.  Device events around --inner back-to-back calls:
           mosaic   redact_prepare + redact_means + redact_paint
           fill     redact_prepare + redact_paint
           empty    the same call with counts = 0: redact_prepare + a paint whose every tile ends at the cull
         so that mosaic - fill is what the means cost and fill - empty what the writes cost.  Beside them the overlay with the default style.
         A mosaic over redacted frames costs what one over clean frames costs (the same loads, sums and stores), so the frames are not restored
         between calls.
 runner  host wall time per step of video.StreamRunner(annotate=True) over --steps steps with and without redact=RedactStyle(who = both),
         NV12 in / NV12 out and BGR in / BGR out; the nets and the face load are tools/bench_draw_nv12.py's (SCRFD-2.5G + MobileFaceNet,
         FacePipeline, one face slot per frame).
Inside every repeat the variants take turns; round 0 warms up; median, min and max of --repeats rounds.  Before anything is timed, one mosaic
call of either format is compared byte for byte with its host twin.

One JSON line on stdout, appended to --out.   python tools/bench_redact.py [--frames 32] [--repeats 7] [--inner 20] [--steps 6]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scrfd_arcface_facerecognition_amd import archs  # noqa: E402
from scrfd_arcface_facerecognition_amd._lib import (REDACT_FILL, REDACT_KNOWN, REDACT_MOSAIC, REDACT_UNKNOWN, Context, DrawStyle,  # noqa: E402
                                                    Nv12Frames, RedactStyle, check, nv12_desc)
from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery, LabelTable  # noqa: E402
from scrfd_arcface_facerecognition_amd.pipeline import FacePipeline, calibrate_detector_bias  # noqa: E402
from scrfd_arcface_facerecognition_amd.video import StreamRunner  # noqa: E402

H, W, IN = 1080, 1920, (640, 640)
F, CAP, G = 14, 256, 1000


def note(msg):
    print(f"[bench_redact] {msg}", file=sys.stderr, flush=True)


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32, help="frames per call and per step")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls per device-event window")
    ap.add_argument("--steps", type=int, default=6, help="steps per timed StreamRunner run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redact", "bench_redact.jsonl"))
    args = ap.parse_args()
    assert args.repeats >= 5 and args.frames >= 4 and args.inner >= 1 and args.steps >= 2
    B = args.frames
    ctx = Context(0)
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(2024)
    nv_host = rng.integers(0, 256, (B, H * 3 // 2, W), dtype=np.uint8)
    nv_dev = ctx.to_device(nv_host)
    nv = Nv12Frames(nv_dev, H, W)
    bgr_dev = ctx.empty((B, H, W, 3), np.uint8)
    check(lib.fid_nv12_to_bgr(h, *nv.args(), B, H, W, C.c_void_p(bgr_dev.ptr)))
    bgr_host = bgr_dev.download()
    # tools/bench_draw.py's face table, on 1080p
    det = np.zeros((B, CAP, 5), np.float32)
    w = rng.uniform(40, 160, (B, F))
    x1, y1 = rng.uniform(0, W - 40, (B, F)), rng.uniform(0, H - 40, (B, F))
    det[:, :F, 0], det[:, :F, 1], det[:, :F, 2], det[:, :F, 3], det[:, :F, 4] = x1, y1, x1 + w, y1 + w * rng.uniform(1.0, 1.4, (B, F)), 0.9
    idx = np.where(np.arange(F)[None, :] % 2 == 0, rng.integers(0, G, (B, F)), -1).astype(np.int32)
    score = rng.uniform(0.3, 0.9, (B, F)).astype(np.float32)
    counts = np.full(B, F, np.int32)
    d_det, d_counts, d_zero = ctx.to_device(det), ctx.to_device(counts), ctx.to_device(np.zeros(B, np.int32))
    d_idx, d_score = ctx.to_device(idx), ctx.to_device(score)
    labels = LabelTable(ctx, [f"person_{g:04d}" for g in range(G)])
    both = REDACT_UNKNOWN | REDACT_KNOWN
    mosaic, fill, draw_style = RedactStyle(REDACT_MOSAIC, both), RedactStyle(REDACT_FILL, both, fill_bgr=(40, 40, 40)), DrawStyle()
    line = dict(frames=B, frame_hw=[H, W], faces_per_frame=F, repeats=args.repeats, inner=args.inner, device=ctx.name(),
                style=dict(who=both, cells=mosaic.cells, expand=mosaic.expand))

    def ident(cnt):
        return (B, H, W, C.c_void_p(d_det.ptr), C.c_void_p(cnt.ptr), CAP, C.c_void_p(d_idx.ptr), C.c_void_p(d_score.ptr), F, None, 0)

    # ---- equal to the host twins first
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    host_tail = (B, H, W, p(det), p(counts), CAP, p(idx), p(score), F, None, 0, C.byref(mosaic))
    want_bgr, want_nv = bgr_host.copy(), nv_host.copy()
    check(lib.fid_redact_faces_host(p(want_bgr), *host_tail))
    check(lib.fid_redact_faces_nv12_host(p(want_nv), C.byref(nv12_desc(H, W)), *host_tail))
    check(lib.fid_redact_faces(h, C.c_void_p(bgr_dev.ptr), *ident(d_counts), C.byref(mosaic)))
    check(lib.fid_redact_faces_nv12(h, *nv.args(), *ident(d_counts), C.byref(mosaic)))
    got_bgr, got_nv = bgr_dev.download(), nv_dev.download()
    assert np.array_equal(got_bgr, want_bgr) and np.array_equal(got_nv, want_nv) and (got_bgr != bgr_host).any()
    line["redacted_share_of_pixels"] = round(float((got_bgr != bgr_host).any(axis=-1).mean()), 4)
    bgr_dev.upload(bgr_host)
    nv_dev.upload(nv_host)
    note("both formats equal the host twins; timing")

    def bgr_call(style, cnt=d_counts):
        return lambda: check(lib.fid_redact_faces(h, C.c_void_p(bgr_dev.ptr), *ident(cnt), C.byref(style)))

    def nv_call(style, cnt=d_counts):
        return lambda: check(lib.fid_redact_faces_nv12(h, *nv.args(), *ident(cnt), C.byref(style)))

    kernels = {
        "fid_redact_faces/mosaic": bgr_call(mosaic), "fid_redact_faces/fill": bgr_call(fill), "fid_redact_faces/empty": bgr_call(mosaic, d_zero),
        "fid_redact_faces_nv12/mosaic": nv_call(mosaic), "fid_redact_faces_nv12/fill": nv_call(fill),
        "fid_redact_faces_nv12/empty": nv_call(mosaic, d_zero),
        "fid_draw_faces": lambda: check(lib.fid_draw_faces(h, C.c_void_p(bgr_dev.ptr), *ident(d_counts), None, labels.handle, C.byref(draw_style))),
        "fid_draw_faces_nv12": lambda: check(lib.fid_draw_faces_nv12(h, *nv.args(), *ident(d_counts), None, labels.handle, C.byref(draw_style))),
    }
    k_ms = {k: [] for k in kernels}
    for rep in range(args.repeats + 1):                               # round 0 warms up
        for k, call in kernels.items():
            ctx.event_record(0)
            for _ in range(args.inner):
                call()
            ctx.event_record(1)
            t = ctx.elapsed_ms(0, 1) / args.inner                     # (synchronises)
            if rep:
                k_ms[k].append(t)
    km = {k: spread(v) for k, v in k_ms.items()}
    med = lambda k: km[k]["median"]
    for fam, draw in (("fid_redact_faces", "fid_draw_faces"), ("fid_redact_faces_nv12", "fid_draw_faces_nv12")):
        km[fam + "/mosaic_over_draw"] = round(med(fam + "/mosaic") / med(draw), 3)
        km[fam + "/fill_over_draw"] = round(med(fam + "/fill") / med(draw), 3)
        km[fam + "/means_ms"] = round(med(fam + "/mosaic") - med(fam + "/fill"), 4)
        km[fam + "/paint_ms"] = round(med(fam + "/fill") - med(fam + "/empty"), 4)
    line["kernels_ms"] = km
    note("kernels: " + json.dumps(km))

    # ---- the annotating runner, with and without redaction
    det_net = archs.scrfd_2_5g(IN)
    lbuf, fr4 = ctx.empty((4,) + IN + (3,), np.uint8), ctx.to_device(bgr_host[:4])
    check(lib.fid_letterbox(h, C.c_void_p(fr4.ptr), 4, H, W, C.c_void_p(lbuf.ptr), IN[0], IN[1], None))
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, 0), lbuf.download(), target=48, max_batch=4)
    rec_net = archs.mobilefacenet()
    dnet = CompiledNet(ctx, det_net, det_P, max_batch=B)
    rnet = CompiledNet(ctx, rec_net, archs.synth_params(rec_net, 0), max_batch=B)
    gallery = Gallery(ctx, np.random.default_rng(2).standard_normal((64, 512)).astype(np.float32))
    items = {"nv12": nv_host, "bgr": bgr_host}
    configs = [(fmt, red) for fmt in ("nv12", "bgr") for red in (False, True)]
    runners = {}
    for fmt, red in configs:
        pipe = FacePipeline(ctx, dnet, rnet, batch=B, faces_per_frame=1)
        runners[(fmt, red)] = StreamRunner(pipe, gallery, (H, W), annotate=True, pixel_format=fmt, annotate_format=fmt,
                                           redact=RedactStyle(who=both) if red else None)
    wall = {c: [] for c in configs}
    for rep in range(args.repeats + 1):
        for c, r in runners.items():
            steps = args.steps if rep else 2
            t0 = time.perf_counter()
            n_out = sum(1 for _ in r.run(items[c[0]][i % B] for i in range(steps * B)))
            t = (time.perf_counter() - t0) * 1e3 / steps
            assert n_out == steps * B
            if rep:
                wall[c].append(t)
        note(f"  runner round {rep} done")
    line["steps_per_run"] = args.steps
    line["runner_wall_ms_per_step"] = {}
    for fmt in ("nv12", "bgr"):
        d = {"plain": spread(wall[(fmt, False)]), "redact": spread(wall[(fmt, True)])}
        d["redact_over_plain"] = round(d["redact"]["median"] / d["plain"]["median"], 3)
        line["runner_wall_ms_per_step"][fmt] = d
    for r in runners.values():
        r.close()
    labels.close()
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
