#!/usr/bin/env python3
"""Best shots (fid_shot_score / fid_track_keep, pipeline.TrackedFacePipeline(best_shot=True)) measurements for docs/FINDINGS.md: what the
keeper adds to a tracked step.  tools/bench_track.py's video (one smooth random image, 640 x 640 windows sliding 2 pixels per frame, forth
and back; SCRFD-10G + IResNet-50 with seeded weights, the detector's cls bias calibrated on the first frames; B = 64, rows="count", a
gallery of random rows) on a TrackedFacePipeline(refresh 16, retry 1) step in three forms:
  measure        measure=True                      (the form a tree without the keeper has too)
  best_shot_off  measure=True, best_shot=False     (must be the same launches as `measure`)
  best_shot_on   best_shot=True                    (+ fid_shot_score, fid_track_keep: three launches)
each in two regimes: gallery threshold 0 (nearly every face is named: few rows per step) and 0.99 (nobody is named: every face is a row of
every step -- the keeper's heaviest case).  Per configuration: warm(), 8 steps to settle, then 5 repeats of 4 consecutive steps between two
HIP events, the configurations alternating inside every repeat; the median ms per step.
--parent DIR: another checkout of the project, built (its libfaceid.so in place), e.g. the commit before the keeper.  Its `measure` form then
runs in a child process of its own, alternating with this tree's child over --rounds rounds, on the same device; the medians are taken over
all rounds.  A tree that does not know best_shot runs the `measure` form only.
Needs nothing outside the two trees.  bench_shots.py [--parent DIR] [--rounds 2] [--batch 64] [--out FILE]"""
import argparse
import inspect
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, STEPS, SETTLE = 5, 4, 8
HW = 640
REGIMES = {"named": 0.0, "nobody_named": 0.99}


def smooth_image(rng, h, w, cell=40):
    gh, gw = h // cell + 2, w // cell + 2
    grid = rng.integers(0, 256, (gh, gw, 3)).astype(np.float64)
    ys, xs = np.arange(h) / cell, np.arange(w) / cell
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    top = grid[y0][:, x0] * (1 - fx) + grid[y0][:, x0 + 1] * fx
    bot = grid[y0 + 1][:, x0] * (1 - fx) + grid[y0 + 1][:, x0 + 1] * fx
    return np.clip(np.rint(top * (1 - fy) + bot * fy), 0, 255).astype(np.uint8)


def log(msg):
    print(f"[bench_shots] {msg}", file=sys.stderr, flush=True)


def measure_tree(args):
    """this process measures the tree it imports: -> {"forms": {name: [ms per step, one per repeat]}, ...}"""
    sys.path.insert(0, args.tree)
    os.environ.setdefault("FID_AUTOTUNE", "0")
    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd._lib import Context
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline, TrackedFacePipeline, calibrate_detector_bias

    ctx = Context(0)
    B = args.batch
    rng = np.random.default_rng(1234)
    half = 2 * B
    wide = smooth_image(rng, HW, HW + 2 * half)
    tri = [t if t <= half else 2 * half - t for t in range(2 * half)]
    batches = [ctx.to_device(np.stack([wide[:, 2 * tri[(k * B + i) % (2 * half)]:2 * tri[(k * B + i) % (2 * half)] + HW] for i in range(B)]))
               for k in range(4)]
    det_net = archs.scrfd_10g((HW, HW))
    calib = np.stack([wide[:, 2 * t:2 * t + HW] for t in range(0, half, half // 8)][:8])
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, seed=0), calib, target=args.target)
    det = CompiledNet(ctx, det_net, det_P, max_batch=B)
    probe = PackedFacePipeline(ctx, det, CompiledNet(ctx, archs.mobilefacenet(), archs.synth_params(archs.mobilefacenet(), 0), max_batch=8),
                               batch=B, row_cap=8)
    probe.detect(batches[0], HW, HW)
    probe.post.check()
    found = int(np.clip(probe.post.counts.download()[:B], 0, probe.post.cap).sum())
    probe.rec.close()
    row_cap = max(64, -(-(found * 5 // 4) // 64) * 64)
    assert 0 < found <= row_cap <= 1280, f"row_cap {row_cap} against {found} faces per step: lower --target"
    log(f"{args.tree}: {found} faces in the first step, row_cap {row_cap}")
    rec_net = archs.iresnet50()
    rec = CompiledNet(ctx, rec_net, archs.synth_params(rec_net, seed=0), max_batch=row_cap)
    gallery = Gallery(ctx, np.random.default_rng(99).standard_normal((args.gallery, 512)).astype(np.float32))
    kw = dict(batch=B, row_cap=row_cap, rows="count", buckets=list(range(64, row_cap, 64)) + [row_cap], refresh=16, retry=1)
    forms = {"measure": dict(measure=True)}
    if "best_shot" in inspect.signature(TrackedFacePipeline.__init__).parameters:
        forms["best_shot_off"] = dict(measure=True, best_shot=False)
        forms["best_shot_on"] = dict(best_shot=True, finished_cap=4096)
    configs = {f"{f}/{r}": (TrackedFacePipeline(ctx, det, rec, **kw, **fkw), thr) for r, thr in REGIMES.items() for f, fkw in forms.items()}
    step_no = {n: 0 for n in configs}

    def run(name, k):
        pipe, thr = configs[name]
        for _ in range(k):
            pipe.run_step(batches[step_no[name] % 4], HW, HW, gallery, thr)
            step_no[name] += 1

    first = True
    for name, (pipe, thr) in configs.items():
        if first:
            pipe.warm(batches[0], HW, HW, gallery, thr)    # every bucket once: the nets are shared, so once for all configurations
            first = False
        run(name, SETTLE)
        ctx.sync()
    ms = {n: [] for n in configs}
    for r in range(REPS):
        for name in configs:                               # alternating: every repeat visits every configuration
            ctx.sync()
            ctx.event_record(0)
            run(name, STEPS)
            ctx.event_record(1)
            ms[name].append(round(ctx.elapsed_ms(0, 1) / STEPS, 4))
        log(f"repeat {r}: " + ", ".join(f"{n} {ms[n][-1]:.3f}" for n in configs))
    rows, finished = {}, {}
    for name, (pipe, thr) in configs.items():              # rows per step and records per step, in a pass of its own
        got = []
        for _ in range(STEPS):
            run(name, 1)
            got.append(min(int(pipe.offsets.download()[B]), row_cap))
        rows[name] = round(float(np.mean(got)), 1)
        if getattr(pipe, "best_shot", False):
            n, _, _, _ = pipe._finished_store()
            finished[name] = {"records_since_start": n, "dropped": pipe.finished_dropped, "steps": step_no[name]}
    return {"tree": args.tree, "device": ctx.name(), "batch": B, "row_cap": row_cap, "faces_first_step": found, "ms": ms,
            "rows_embedded_per_step_mean": rows, "finished": finished}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE, help="the checkout this process imports and measures")
    ap.add_argument("--parent", default=None, help="a built checkout of another commit: its `measure` form runs alternately with this tree's")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--gallery", type=int, default=1000)
    ap.add_argument("--target", type=int, default=10)
    ap.add_argument("--child", action="store_true", help="(internal) measure --tree and print one JSON line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child or args.parent is None:
        runs = [("this", measure_tree(args))]
        if args.child:
            print(json.dumps(runs[0][1]), flush=True)
            return
    else:
        runs = []
        for r in range(args.rounds):                       # one process per tree and round (a package can be imported once), trees alternating
            for label, tree in (("parent", os.path.abspath(args.parent)), ("this", HERE)):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--batch", str(args.batch), "--gallery", str(args.gallery),
                       "--target", str(args.target)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, cwd=tree)
                runs.append((label, json.loads(p.stdout.strip().splitlines()[-1])))
                log(f"round {r}, {label} done")
    med = statistics.median
    out = {"tool": "bench_shots", "date": time.strftime("%Y-%m-%d"), "device": runs[0][1]["device"], "batch": args.batch,
           "row_cap": runs[0][1]["row_cap"], "repeats": REPS, "steps_per_repeat": STEPS, "rounds": len(runs) if args.parent is None else args.rounds,
           "autotune": os.environ.get("FID_AUTOTUNE", "0"), "configs": {}}
    for label, res in runs:
        for name, v in res["ms"].items():
            c = out["configs"].setdefault(f"{label}:{name}", {"ms": [], "rows_embedded_per_step_mean": res["rows_embedded_per_step_mean"][name]})
            c["ms"] += v
    for c in out["configs"].values():
        v = c.pop("ms")
        c["ms_per_step"], c["ms_per_step_min_max"], c["samples"] = round(med(v), 4), [min(v), max(v)], len(v)
    out["finished"] = runs[-1][1]["finished"]
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
