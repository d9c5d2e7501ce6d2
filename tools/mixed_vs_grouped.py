#!/usr/bin/env python3
"""One mixed-size batch against same-shape groups, one MI355X: SCRFD-10G + IResNet-50 on 64 images in four interleaved sizes, 16 each
(1080x1920, 720x1280, 480x853, 640x640) -- a gallery folder from four kinds of camera.  All images are resident on the device; a step
is letterbox -> detector -> post-process (max_num faces per image) -> fid_face_pack -> alignment -> recogniser -> normalisation.

  (a) grouped   the four same-shape groups of 16, one uniform chain each (what build_targets_from_images' by_shape buckets did)
  (b) mixed     ONE ragged batch of 64 through the *_ragged entry points
  (c) / (e)     64 same-size 1080x1920 images through the uniform letterbox alone, timed twice: the A/A spread is the margin for
  (d)           the same 64 images through the ragged letterbox alone

Device time between two events on the context's stream (fid_event_record), every shape warmed first, the variants alternating inside
every repeat, median over the repeats.  Prints ONE JSON line (and writes it to --out).

    python tools/mixed_vs_grouped.py [--repeats 5] [--steps 20] [--out profiles/r06/mixed_vs_grouped.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1080, 1920), (720, 1280), (480, 853), (640, 640)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-size", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--max-num", type=int, default=2, help="faces per image handed to the recogniser")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5 and args.steps >= 20, "median of >= 5 repeats of >= 20 steps"
    plan = os.path.join(ROOT, "plans", "mi355x.plan")
    if "FID_PLAN" not in os.environ and "FID_PLAN_RO" not in os.environ and os.path.exists(plan):
        os.environ["FID_PLAN_RO"] = plan                  # the picks bench.py runs with, where the plan has them

    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd._lib import Context, check, c_i32_p, c_i64_p
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, HeadViews, PostProcessor
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias

    def log(msg):
        print(f"[mixed_vs_grouped] {msg}", file=sys.stderr, flush=True)

    ctx = Context(0)
    lib, h = ctx.lib, ctx.handle
    G, n_sizes = args.per_size, len(SIZES)
    B = G * n_sizes
    rng = np.random.default_rng(1234)
    calib = rng.integers(0, 256, (8, 640, 640, 3), dtype=np.uint8)
    groups = [rng.integers(0, 256, (G, H, W, 3), dtype=np.uint8) for H, W in SIZES]
    mixed = [groups[i % n_sizes][i // n_sizes] for i in range(B)]          # interleaved: image i has size i % 4
    det_net = archs.scrfd_10g((640, 640))
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, seed=0), calib, target=48)
    rec_net = archs.iresnet50()
    rec_P = archs.synth_params(rec_net, seed=0)
    det = CompiledNet(ctx, det_net, det_P, max_batch=B)
    rows_cap = B * args.max_num
    rec = CompiledNet(ctx, rec_net, rec_P, max_batch=rows_cap)
    post = PostProcessor(ctx, B, cap=256)
    det_in = ctx.empty((B, 640, 640, 3), np.uint8)
    offsets, src = ctx.empty((B + 1,), np.int32), ctx.empty((rows_cap,), np.int32)
    crops, q = ctx.empty((rows_cap, 112, 112, 3), np.uint8), ctx.empty((rows_cap, 512), np.float16)
    groups_dev = [ctx.to_device(g) for g in groups]
    batch = ctx.image_batch(mixed)

    def chain(n_img, n_rows, letterbox, postprocess, align):
        """one detect -> embed chain over n_img images; n_rows recogniser rows (known from the probe pass: no read-back inside a step)"""
        letterbox()
        det.run_device(det_in, n_img)
        postprocess(HeadViews.from_fused(det))             # (per run, as SCRFD._detect_chunk does)
        check(lib.fid_face_pack(h, C.c_void_p(post.counts.ptr), n_img, post.cap, args.max_num, C.c_void_p(offsets.ptr), C.c_void_p(src.ptr), rows_cap))
        if n_rows == 0:
            return
        align(n_rows)
        rec.run_device(crops, n_rows)
        emb_ptr, _, _ = rec.tensor(rec.low.outputs[0])
        check(lib.fid_l2_normalize_f16_packed(h, C.c_void_p(emb_ptr), n_rows, 512, C.c_void_p(src.ptr), C.c_void_p(q.ptr)))

    def group_chain(gi, n_rows):
        H, W = SIZES[gi]
        fr = groups_dev[gi]
        sc = C.c_double()
        chain(G, n_rows,
              lambda: check(lib.fid_letterbox(h, C.c_void_p(fr.ptr), G, H, W, C.c_void_p(det_in.ptr), 640, 640, C.byref(sc))),
              lambda hv: post.run(hv, G, (640, 640), (H, W), 0.5, 0.4, args.max_num, 0),
              lambda n: check(lib.fid_align_crops_packed(h, C.c_void_p(fr.ptr), G, H, W, C.c_void_p(post.kps.ptr), post.cap, C.c_void_p(src.ptr), n,
                                                         C.c_void_p(crops.ptr), None)))

    def mixed_chain(n_rows):
        chain(B, n_rows,
              lambda: check(lib.fid_letterbox_ragged(h, *batch.args(), B, C.c_void_p(det_in.ptr), 640, 640, None)),
              lambda hv: post.run_ragged(hv, B, (640, 640), batch.hw, 0.5, 0.4, args.max_num, 0),
              lambda n: check(lib.fid_align_crops_packed_ragged(h, *batch.args(), B, C.c_void_p(post.kps.ptr), post.cap, C.c_void_p(src.ptr), n,
                                                                C.c_void_p(crops.ptr), None)))

    def total_rows(n_img):
        post.check()
        return int(offsets.download()[n_img])

    # probe pass: the face counts decide every recogniser shape
    rows_g = []
    for gi in range(n_sizes):
        group_chain(gi, 0)
        rows_g.append(total_rows(G))
    mixed_chain(0)
    rows_m = total_rows(B)
    log(f"recogniser rows: groups {rows_g} (sum {sum(rows_g)}), mixed {rows_m}")
    assert rows_m > 0 and sum(rows_g) > 0                  # (a group the detector finds nothing in ends after its pack: chain())

    def grouped():
        for gi in range(n_sizes):
            group_chain(gi, rows_g[gi])

    # letterbox alone on 64 same-size images
    same = ctx.to_device(np.broadcast_to(groups[0][:1], (B,) + groups[0].shape[1:]))
    same_hw = np.tile(np.array([SIZES[0]], np.int32), (B, 1))
    same_off = (np.arange(B, dtype=np.int64) * (SIZES[0][0] * SIZES[0][1] * 3))
    sc = C.c_double()

    def lb_uniform():
        check(lib.fid_letterbox(h, C.c_void_p(same.ptr), B, SIZES[0][0], SIZES[0][1], C.c_void_p(det_in.ptr), 640, 640, C.byref(sc)))

    def lb_ragged():
        check(lib.fid_letterbox_ragged(h, C.c_void_p(same.ptr), same.nbytes, same_hw.ctypes.data_as(c_i32_p),
                                       same_off.ctypes.data_as(c_i64_p), B, C.c_void_p(det_in.ptr), 640, 640, None))

    variants = {"grouped": grouped, "mixed": lambda: mixed_chain(rows_m), "letterbox_uniform": lb_uniform, "letterbox_ragged": lb_ragged,
                "letterbox_uniform_again": lb_uniform}
    for name, fn in variants.items():                      # warm every shape that will be timed (the executor tunes per batch size)
        log(f"warming {name}")
        for _ in range(3):
            fn()
        ctx.sync()

    def timed(fn, k):
        ctx.event_record(0)
        for _ in range(k):
            fn()
        ctx.event_record(1)
        return ctx.elapsed_ms(0, 1) / k                    # synchronises

    ms = {n: [] for n in variants}
    for r in range(args.repeats):
        for name, fn in variants.items():                  # alternating: every repeat visits every variant
            ms[name].append(timed(fn, args.steps))
        log(f"repeat {r}: " + ", ".join(f"{n} {ms[n][-1]:.4f}" for n in variants))
    med = lambda v: float(np.median(v))
    line = {
        "tool": "mixed_vs_grouped", "device": ctx.name(), "images": B, "sizes": SIZES, "per_size": G, "det": "scrfd_10g", "rec": "arcface_r50",
        "max_num": args.max_num, "rows_grouped": rows_g, "rows_mixed": rows_m, "repeats": args.repeats, "steps_per_repeat": args.steps,
        "variants": {n: {"ms_per_step": round(med(ms[n]), 4), "ms_per_step_min_max": [round(min(ms[n]), 4), round(max(ms[n]), 4)]} for n in variants},
    }
    v = line["variants"]
    line["mixed_over_grouped"] = round(v["mixed"]["ms_per_step"] / v["grouped"]["ms_per_step"], 4)
    line["letterbox_ragged_over_uniform"] = round(v["letterbox_ragged"]["ms_per_step"] / v["letterbox_uniform"]["ms_per_step"], 4)
    line["letterbox_uniform_aa"] = round(v["letterbox_uniform_again"]["ms_per_step"] / v["letterbox_uniform"]["ms_per_step"], 4)
    out = json.dumps(line)
    print(out, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
