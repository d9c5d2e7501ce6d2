#!/usr/bin/env python3
"""Score-distribution (fid_gallery_score_hist) measurements for docs/FINDINGS.md, "score distributions".  One process, one store.

  bench_calibrate.py --n 100000 --store realistic [--reps 5] [--bins 64,512,4096] [--out profiles/calibrate/bench_calibrate.jsonl]

Stores at dim 512, every gallery row a position (rows_dev = NULL):
  spread     rows on a fan in a plane (angle uniform in [0, pi]) plus a little noise: the scores cover the whole of [-1, 1], so a wave's 64 counts
             of one step go to many different counters; labels k % 1000
  realistic  persons x 10 noisy copies (centre + 0.7 x noise: genuine scores around 0.67, impostor scores concentrated within +-0.1 of 0, where
             a handful of counters take nearly every count)
Measured, each the median of --reps runs between device events after one warm-up run that sizes the arenas:
  hist[bins/peel]   fid_gallery_score_hist alone, for every bin count and for FID_HIST_PEEL = 0 (the default: every lane adds for itself) and 4 (four
                    rounds of in-wave aggregation before the LDS counters); the two answers must be the same bytes
  cluster           fid_gallery_cluster on the same rows at a threshold no pair reaches (1.5): the same walk and the same tile code with only a
                    counting epilogue, and a second pass that skips every tile pair -- the yardstick
The three calls alternate inside every round, so a drift of the machine hits all of them alike.
One JSON line per run is appended to --out.  There is no pass mark."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--store", choices=("spread", "realistic"), default="realistic")
ap.add_argument("--bins", default="64,512,4096")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrfd_arcface_facerecognition_amd import _lib  # noqa: E402
from scrfd_arcface_facerecognition_amd.engine import Gallery  # noqa: E402

DIM = 512


def make_store(kind, n):
    rng = np.random.default_rng(n)
    if kind == "spread":
        theta = rng.uniform(0.0, np.pi, n).astype(np.float32)
        x = 0.02 * rng.standard_normal((n, DIM), dtype=np.float32)
        x[:, 0] += np.cos(theta)
        x[:, 1] += np.sin(theta)
        return x, (np.arange(n) % 1000).astype(np.int32)
    persons = (n + 9) // 10
    labels = np.repeat(np.arange(persons), 10)[:n].astype(np.int32)
    x = rng.standard_normal((persons, DIM), dtype=np.float32)[labels]
    x += 0.7 * rng.standard_normal((n, DIM), dtype=np.float32)
    return x, labels


def device_ms(ctx, calls, reps):
    """calls: {name: enqueue}; one warm-up round, then `reps` rounds that ALTERNATE the calls, so that a drift of the machine hits all alike
    -> {name: (median ms, min ms)}"""
    times = {name: [] for name in calls}
    for rep in range(reps + 1):
        for name, enqueue in calls.items():
            ctx.sync()
            ctx.event_record(0)
            enqueue()
            ctx.event_record(1)
            ctx.sync()
            if rep:
                times[name].append(ctx.elapsed_ms(0, 1))
    return {name: (statistics.median(t), min(t)) for name, t in times.items()}


ctx = _lib.Context(0)
n = args.n
emb, labels = make_store(args.store, n)
gal = Gallery(ctx, emb)
del emb
labels_dev = ctx.to_device(labels)
ctx.sync()
rec = {"tool": "bench_calibrate", "device": ctx.name(), "date": time.strftime("%Y-%m-%d"), "store": args.store, "n": n, "dim": DIM,
       "pairs": n * (n - 1) // 2, "reps": args.reps, "hist_ms": {}, "hist_min_ms": {}, "ratio_to_cluster": {}}
print(f"device: {ctx.name()}  store: {args.store}  n={n:,d}  pairs={rec['pairs']:,d}", flush=True)

out = ctx.empty((4 * n + 6,), np.int32)
cluster = lambda: _lib.check(ctx.lib.fid_gallery_cluster(ctx.handle, gal.handle, None, n, C.c_float(1.5), 2, C.c_void_p(out.ptr),
                                                         C.c_void_p(out.ptr + 4 * n), C.c_void_p(out.ptr + 8 * n), C.c_void_p(out.ptr + 12 * n),
                                                         C.c_void_p(out.ptr + 16 * n)))
cluster_ms = []


def with_peel(peel, call):
    def enqueue():
        os.environ["FID_HIST_PEEL"] = peel                                            # (read per call)
        call()
    return enqueue


for bins in (int(b) for b in args.bins.split(",")):
    words = 4 * bins + 8
    buf = ctx.empty((words + 4 * n,), np.int32)
    at = lambda k: C.c_void_p(buf.ptr + 4 * (words + k * n))
    call = lambda: _lib.check(ctx.lib.fid_gallery_score_hist(ctx.handle, gal.handle, None, C.c_void_p(labels_dev.ptr), n, bins, C.c_void_p(buf.ptr),
                                                             at(0), at(1), at(2), at(3), C.c_void_p(buf.ptr + 16 * bins)))
    got = device_ms(ctx, {"cluster": cluster, "4": with_peel("4", call), "0": with_peel("0", call)}, args.reps)
    assert int(out.download()[4 * n]) == 0, "a pair reached the threshold of the yardstick"
    cluster_ms.append(got["cluster"][0])
    print(f"bins={bins:<5d} cluster (no hit): {got['cluster'][0]:10.3f} ms (min {got['cluster'][1]:.3f})", flush=True)
    answers = {}
    for peel in ("4", "0"):
        key = f"{bins}/peel{peel}"
        rec["hist_ms"][key], rec["hist_min_ms"][key] = got[peel]
        rec["ratio_to_cluster"][key] = got[peel][0] / got["cluster"][0]
        with_peel(peel, call)()
        answers[peel] = buf.download()
        print(f"bins={bins:<5d} hist peel={peel}      : {got[peel][0]:10.3f} ms (min {got[peel][1]:.3f})  {rec['ratio_to_cluster'][key]:.2f} x cluster", flush=True)
    os.environ.pop("FID_HIST_PEEL", None)
    assert np.array_equal(answers["4"], answers["0"]), "the in-wave aggregation changed the answer"
    summary = answers["4"][4 * bins:words].view(np.uint64)
    hist = answers["4"][:4 * bins].view(np.uint64).reshape(2, bins)
    assert int(summary[1] + summary[2] + summary[3]) == int(summary[0]) * (int(summary[0]) - 1) // 2, "the summary does not add up"
    rec["summary"] = [int(v) for v in summary]
    rec.setdefault("busiest_counter_share", {})[str(bins)] = float(hist.max() / max(1, int(summary[1] + summary[2])))
rec["cluster_ms"] = statistics.median(cluster_ms)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
