#!/usr/bin/env python3
"""Annotated video out as NV12 against today's BGR way out, on 1080p frames, for docs/FINDINGS.md ("NV12 output").  One process; the nets, the
frames and the face load are tools/bench_nv12.py's (SCRFD-2.5G + MobileFaceNet, FacePipeline at --frames frames per step, one face slot per
frame); the BGR frames are fid_nv12_to_bgr of the NV12 frames.  The yardstick of every ratio is path (a), measured in the same run.

 paths   one step's way out, after run_step has left its results on the device.  `device_ms`: device-event time of the enqueued calls
         (--inner back-to-back per window); `download_ms`: host wall time of the synchronous device-to-host copy of the drawn batch;
         `total_ms`: host wall time of the calls plus the download, from a synchronised device:
           a  fid_nv12_to_bgr + fid_draw_faces + BGR download            (NV12 in, today: pipe.draw(nv12) -> pipe.bgr)
           b  fid_draw_faces_nv12 + NV12 download                         (NV12 in: pipe.draw(nv12, out="nv12"), in place)
           c  fid_draw_faces + fid_bgr_to_nv12 + NV12 download            (BGR in: pipe.draw(bgr, out="nv12"))
         The overlay reads nothing from the frames, so drawing the same frames again costs what drawing clean ones costs.
 kernels fid_draw_faces_nv12 against fid_draw_faces, fid_bgr_to_nv12 against fid_nv12_to_bgr: device events, --inner calls per window.
 runner  host wall time per step of video.StreamRunner(annotate=True) over --steps steps, annotate_format "bgr" against "nv12", for both
         pixel formats; `download_bytes` beside it.
Inside every repeat the variants take turns; round 0 warms up; median, min and max of --repeats rounds.  Before anything is timed, (b) and (c)
are compared byte for byte with the host twins on the step's downloaded results.

One JSON line on stdout, appended to --out.   python tools/bench_draw_nv12.py [--frames 32] [--repeats 7] [--inner 20] [--steps 8]"""
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
from scrfd_arcface_facerecognition_amd._lib import Context, DrawStyle, Nv12Frames, check, label_arrays  # noqa: E402
from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery  # noqa: E402
from scrfd_arcface_facerecognition_amd.pipeline import FacePipeline, calibrate_detector_bias  # noqa: E402
from scrfd_arcface_facerecognition_amd.video import StreamRunner  # noqa: E402

H, W, IN = 1080, 1920, (640, 640)


def note(msg):
    print(f"[bench_draw_nv12] {msg}", file=sys.stderr, flush=True)


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def host_twins(lib, pipe, gallery, nv_host, bgr_host, B):
    """what (b) and (c) must have written, from the step's downloaded results: fid_draw_faces_nv12_host; fid_draw_faces_host + fid_bgr_to_nv12_host"""
    from scrfd_arcface_facerecognition_amd._lib import nv12_desc
    det, counts = pipe.post.det.download(), pipe.post.counts.download()
    idx, score = pipe.idx.download(), pipe.score.download()
    raw, off, cols = label_arrays(gallery.names, None)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    st, desc = DrawStyle(), nv12_desc(H, W)
    tail = (p(det), p(counts), pipe.post.cap, p(idx), p(score), pipe.F, None, 0, None, raw, p(off), p(cols), len(gallery.names), C.byref(st))
    want_b = nv_host.copy()
    check(lib.fid_draw_faces_nv12_host(p(want_b), C.byref(desc), B, H, W, *tail))
    drawn = bgr_host.copy()
    check(lib.fid_draw_faces_host(p(drawn), B, H, W, *tail))
    want_c = np.empty_like(nv_host)
    check(lib.fid_bgr_to_nv12_host(p(drawn), B, H, W, p(want_c), C.byref(desc)))
    return want_b, want_c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32, help="frames per step")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls per device-event window")
    ap.add_argument("--steps", type=int, default=8, help="steps per timed StreamRunner run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nv12out", "bench_draw_nv12.jsonl"))
    args = ap.parse_args()
    assert args.repeats >= 5 and args.frames >= 4 and args.inner >= 1 and args.steps >= 2
    B = args.frames
    ctx = Context(0)
    lib, h = ctx.lib, ctx.handle
    nv_host = np.random.default_rng(0).integers(0, 256, (B, H * 3 // 2, W), dtype=np.uint8)      # random planes, dense layout
    nv_dev = ctx.to_device(nv_host)
    nv = Nv12Frames(nv_dev, H, W)
    bgr_dev = ctx.empty((B, H, W, 3), np.uint8)
    check(lib.fid_nv12_to_bgr(h, *nv.args(), B, H, W, C.c_void_p(bgr_dev.ptr)))
    bgr_host = bgr_dev.download()
    # the nets and the face load of tools/bench_nv12.py
    det_net = archs.scrfd_2_5g(IN)
    lbuf, fr4 = ctx.empty((4,) + IN + (3,), np.uint8), ctx.to_device(bgr_host[:4])
    check(lib.fid_letterbox(h, C.c_void_p(fr4.ptr), 4, H, W, C.c_void_p(lbuf.ptr), IN[0], IN[1], None))
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, 0), lbuf.download(), target=48, max_batch=4)
    rec_net = archs.mobilefacenet()
    det = CompiledNet(ctx, det_net, det_P, max_batch=B)
    rec = CompiledNet(ctx, rec_net, archs.synth_params(rec_net, 0), max_batch=B)
    gallery = Gallery(ctx, np.random.default_rng(2).standard_normal((64, 512)).astype(np.float32))
    pipe = FacePipeline(ctx, det, rec, batch=B, faces_per_frame=1)
    pipe.run_step(nv, H, W, gallery, 0.4)
    faces = sum(len(f) for f in pipe.results(gallery))
    line = dict(frames=B, frame_hw=[H, W], repeats=args.repeats, inner=args.inner, device=ctx.name(), faces_drawn=faces,
                download_bytes=dict(bgr=B * H * W * 3, nv12=B * H * W * 3 // 2))

    # ---- the three paths: equal to the host twins first
    want_b, want_c = host_twins(lib, pipe, gallery, nv_host, bgr_host, B)
    got_b = pipe.draw(nv, H, W, gallery, out="nv12").buf.download()
    nv_dev.upload(nv_host)
    got_c = pipe.draw(bgr_dev, H, W, gallery, out="nv12").buf.download()
    assert np.array_equal(got_b, want_b) and np.array_equal(got_c, want_c) and (got_b != nv_host).any()
    note(f"{faces} faces; (b) and (c) equal the host twins; timing")
    paths = {
        "a": (lambda: pipe.draw(nv, H, W, gallery), lambda: pipe.bgr.download()),
        "b": (lambda: pipe.draw(nv, H, W, gallery, out="nv12"), lambda: nv_dev.download()),
        "c": (lambda: pipe.draw(bgr_dev, H, W, gallery, out="nv12"), lambda: pipe.nv12_out.buf.download()),
    }
    st = DrawStyle()
    tail = (B, H, W, C.c_void_p(pipe.post.det.ptr), C.c_void_p(pipe.post.counts.ptr), pipe.post.cap, C.c_void_p(pipe.idx.ptr),
            C.c_void_p(pipe.score.ptr), pipe.F, None, 0, None, gallery.labels().handle, C.byref(st))
    conv = ctx.empty((B, H * 3 // 2, W), np.uint8)
    conv_nv = Nv12Frames(conv, H, W)
    kernels = {
        "fid_draw_faces": lambda: check(lib.fid_draw_faces(h, C.c_void_p(bgr_dev.ptr), *tail)),
        "fid_draw_faces_nv12": lambda: check(lib.fid_draw_faces_nv12(h, *nv.args(), *tail)),
        "fid_nv12_to_bgr": lambda: check(lib.fid_nv12_to_bgr(h, *nv.args(), B, H, W, C.c_void_p(pipe.bgr.ptr))),
        "fid_bgr_to_nv12": lambda: check(lib.fid_bgr_to_nv12(h, C.c_void_p(bgr_dev.ptr), B, H, W, *conv_nv.args())),
    }
    dev_ms, dl_ms, tot_ms = ({k: [] for k in paths} for _ in range(3))
    k_ms = {k: [] for k in kernels}
    for rep in range(args.repeats + 1):                               # round 0 warms up
        for k, (enqueue, download) in paths.items():
            ctx.event_record(0)
            for _ in range(args.inner):
                enqueue()
            ctx.event_record(1)
            t_dev = ctx.elapsed_ms(0, 1) / args.inner                 # (synchronises)
            t0 = time.perf_counter()
            download()
            t_dl = (time.perf_counter() - t0) * 1e3
            ctx.sync()
            t0 = time.perf_counter()
            enqueue()
            download()
            t_tot = (time.perf_counter() - t0) * 1e3
            if rep:
                dev_ms[k].append(t_dev); dl_ms[k].append(t_dl); tot_ms[k].append(t_tot)
        for k, call in kernels.items():
            ctx.event_record(0)
            for _ in range(args.inner):
                call()
            ctx.event_record(1)
            t = ctx.elapsed_ms(0, 1) / args.inner
            if rep:
                k_ms[k].append(t)
    line["paths"] = {k: dict(device_ms=spread(dev_ms[k]), download_ms=spread(dl_ms[k]), total_ms=spread(tot_ms[k])) for k in paths}
    for k in ("b", "c"):
        line["paths"][k]["total_over_a"] = round(line["paths"][k]["total_ms"]["median"] / line["paths"]["a"]["total_ms"]["median"], 3)
    line["kernels_ms"] = {k: spread(v) for k, v in k_ms.items()}
    line["kernels_ms"]["draw_nv12_over_bgr"] = round(line["kernels_ms"]["fid_draw_faces_nv12"]["median"] / line["kernels_ms"]["fid_draw_faces"]["median"], 3)
    line["kernels_ms"]["bgr_to_nv12_over_nv12_to_bgr"] = round(line["kernels_ms"]["fid_bgr_to_nv12"]["median"] / line["kernels_ms"]["fid_nv12_to_bgr"]["median"], 3)
    note("paths: " + json.dumps(line["paths"]))

    # ---- the annotating runner, four ways
    items = {"nv12": nv_host, "bgr": bgr_host}
    configs = [(fmt, out) for fmt in ("nv12", "bgr") for out in ("bgr", "nv12")]
    runners = {}
    for fmt, out in configs:
        p = FacePipeline(ctx, det, rec, batch=B, faces_per_frame=1)
        runners[(fmt, out)] = StreamRunner(p, gallery, (H, W), annotate=True, pixel_format=fmt, annotate_format=out)
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
        d = {out: dict(spread(wall[(fmt, out)]), download_bytes=runners[(fmt, out)].download_bytes, upload_bytes=runners[(fmt, out)].upload_bytes)
             for out in ("bgr", "nv12")}
        d["nv12_over_bgr"] = round(d["nv12"]["median"] / d["bgr"]["median"], 3)
        line["runner_wall_ms_per_step"][fmt + "_in"] = d
    for r in runners.values():
        r.close()
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
