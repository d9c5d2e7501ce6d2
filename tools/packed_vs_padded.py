#!/usr/bin/env python3
"""Packed face rows against padded face slots on ragged input, one MI355X: SCRFD-10G + IResNet-50, 64 frames of 640 x 640 whose
lower part is zeroed by a different share per frame, so that the face counts differ widely.

  (a) FacePipeline(faces_per_frame = max_b k_b)            B * F recogniser rows
  (b) PackedFacePipeline rows="capacity" (row_cap rows) and rows="count" (the bucket the batch needs, one 4-byte read-back per step)
  (c) PackedFacePipeline rows="capacity" with row_cap = (b)'s count-mode bucket: the two modes at EQUAL rows = the price of the read-back

Device time between two events on the context's stream (fid_event_record), every shape warmed first, the variants alternating inside
every repeat, median over the repeats.  Prints ONE JSON line (and writes it to --out).

    python tools/packed_vs_padded.py [--repeats 5] [--steps 20] [--out profiles/r06/packed_vs_padded.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ragged_frames(B, seed=1234):
    """random frames; every 16th keeps all rows, the others 4 - 30 % of them (the rest is zeroed), two are empty"""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (B, 640, 640, 3), dtype=np.uint8)
    keep = rng.uniform(0.04, 0.30, B)
    keep[::16] = 1.0
    keep[5::32] = 0.0
    for b in range(B):
        frames[b, int(round(keep[b] * 640)):] = 0
    return frames, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--row-cap", type=int, default=0, help="rows of the capacity mode (0: the multiple of 128 at or above 1.5 x the faces found)")
    ap.add_argument("--bucket", type=int, default=64, help="count-mode buckets are the multiples of this up to --row-cap")
    ap.add_argument("--gallery", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 5 and args.steps >= 20, "median of >= 5 repeats of >= 20 steps"
    plan = os.path.join(ROOT, "plans", "mi355x.plan")
    if "FID_PLAN" not in os.environ and "FID_PLAN_RO" not in os.environ and os.path.exists(plan):
        os.environ["FID_PLAN_RO"] = plan                  # the picks bench.py runs with, where the plan has them

    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd._lib import Context
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery
    from scrfd_arcface_facerecognition_amd.pipeline import FacePipeline, PackedFacePipeline, calibrate_detector_bias

    def log(msg):
        print(f"[packed_vs_padded] {msg}", file=sys.stderr, flush=True)

    ctx = Context(0)
    B, thresh = args.batch, 0.4
    calib = np.random.default_rng(1234).integers(0, 256, (8, 640, 640, 3), dtype=np.uint8)
    frames, keep = ragged_frames(B)
    det_net = archs.scrfd_10g((640, 640))
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, seed=0), calib, target=48)
    rec_net = archs.iresnet50()
    rec_P = archs.synth_params(rec_net, seed=0)
    det = CompiledNet(ctx, det_net, det_P, max_batch=B)
    gallery = Gallery(ctx, np.random.default_rng(99).standard_normal((args.gallery, 512)).astype(np.float32))
    fd = ctx.to_device(frames)

    # the counts decide every shape: one detector pass
    probe = PackedFacePipeline(ctx, det, CompiledNet(ctx, archs.mobilefacenet(), archs.synth_params(archs.mobilefacenet(), 0), max_batch=8),
                               batch=B, row_cap=8)
    probe.detect(fd, 640, 640)
    probe.post.check()
    counts = probe.post.counts.download()[:B]
    total, F = int(counts.sum()), int(counts.max())
    probe.rec.close()
    log(f"faces per frame: {counts.tolist()} -> total {total}, max {F}")
    if args.row_cap <= 0:
        args.row_cap = -(-(total * 3 // 2) // 128) * 128
    assert total > 0 and total <= args.row_cap, f"--row-cap {args.row_cap} is below the batch's {total} faces"
    buckets = list(range(args.bucket, args.row_cap, args.bucket)) + [args.row_cap]
    n_count = next(v for v in buckets if v >= total)

    rec = CompiledNet(ctx, rec_net, rec_P, max_batch=max(B * F, args.row_cap))
    variants = {
        "padded": FacePipeline(ctx, det, rec, batch=B, faces_per_frame=F),
        "packed_capacity": PackedFacePipeline(ctx, det, rec, batch=B, row_cap=args.row_cap),
        "packed_count": PackedFacePipeline(ctx, det, rec, batch=B, row_cap=args.row_cap, rows="count", buckets=buckets),
        "packed_capacity_at_count_rows": PackedFacePipeline(ctx, det, rec, batch=B, row_cap=n_count),
    }
    rows = {"padded": B * F, "packed_capacity": args.row_cap, "packed_count": n_count, "packed_capacity_at_count_rows": n_count}
    for name, p in variants.items():                       # warm every shape that will be timed (the executor tunes per batch size)
        log(f"warming {name} ({rows[name]} recogniser rows)")
        for _ in range(3):
            p.run_step(fd, 640, 640, gallery, thresh)
        ctx.sync()
    faces = {name: sum(len(r) for r in p.results(gallery)) for name, p in variants.items()}
    assert variants["packed_count"].n_run == n_count

    def timed(fn, k):
        ctx.event_record(0)
        for _ in range(k):
            fn()
        ctx.event_record(1)
        return ctx.elapsed_ms(0, 1) / k                    # synchronises

    step_ms = {n: [] for n in variants}
    embed_ms = {n: [] for n in variants}
    for r in range(args.repeats):
        for name, p in variants.items():                   # alternating: every repeat visits every variant
            step_ms[name].append(timed(lambda: p.run_step(fd, 640, 640, gallery, thresh), args.steps))
        for name, p in variants.items():                   # align + recogniser + normalisation alone, on the detections of the step before
            embed_ms[name].append(timed(lambda: p.embed(fd, 640, 640), args.steps))
        log(f"repeat {r}: " + ", ".join(f"{n} {step_ms[n][-1]:.3f}" for n in variants))
    med = lambda v: float(np.median(v))
    line = {
        "tool": "packed_vs_padded", "device": ctx.name(), "batch": B, "det": "scrfd_10g", "rec": "arcface_r50", "gallery": args.gallery,
        "faces_total": total, "faces_max_per_frame": F, "frames_without_face": int((counts == 0).sum()),
        "repeats": args.repeats, "steps_per_repeat": args.steps, "count_buckets": buckets,
        "variants": {n: {"rows_run": rows[n], "faces_found": faces[n], "ms_per_step": round(med(step_ms[n]), 4),
                         "ms_per_step_min_max": [round(min(step_ms[n]), 4), round(max(step_ms[n]), 4)],
                         "embed_ms": round(med(embed_ms[n]), 4)} for n in variants},
    }
    v = line["variants"]
    line["embed_ratio_capacity_over_padded"] = round(v["packed_capacity"]["embed_ms"] / v["padded"]["embed_ms"], 4)
    line["rows_ratio_capacity_over_padded"] = round(rows["packed_capacity"] / rows["padded"], 4)
    line["embed_ratio_count_over_padded"] = round(v["packed_count"]["embed_ms"] / v["padded"]["embed_ms"], 4)
    line["rows_ratio_count_over_padded"] = round(rows["packed_count"] / rows["padded"], 4)
    line["count_readback_ms_per_step"] = round(v["packed_count"]["ms_per_step"] - v["packed_capacity_at_count_rows"]["ms_per_step"], 4)
    out = json.dumps(line)
    print(out, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
