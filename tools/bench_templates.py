#!/usr/bin/env python3
"""Identity-template (fid_gallery_templates) measurements for docs/FINDINGS.md, "identity templates".  One process.

  bench_templates.py [--shapes 10000:1000,100000:10000,1000000:100000,1000000:1] [--reps 7] [--chunks 64,256,1024]
                     [--out profiles/templates/bench_templates.jsonl]

Store at dim 512, every gallery row a position (rows_dev = NULL): person centres plus 0.7 x noise, 1 % of the rows replaced by strangers (random
rows under the person's label), weights 1 .. 255, labels in random order.  Per shape n:P, with trimming off (min_score -2) and on (0.5, which drops
the strangers), medians of --reps runs after one warm-up run that sizes the arenas:
  call_ms        fid_gallery_templates between device events
  read_fraction  the bytes the rule must read -- every member row once for the sums and once for the scores, and with trimming the kept rows of
                 the persons that lost a member once more -- over call_ms, as a fraction of copy_GBps
  copy_GBps      a device-to-device copy of the store measured in the same run (bytes read + bytes written over its time)
  torch_ms       what a user would write today on the same device: S.index_add_(0, labels, x.float() * w) and F.normalize(S).half() (no
                 scores, no trimming; between torch events)
  host_ms        fid_templates_host on the same rows (one thread, wall clock)
  chunk_ms       call_ms with FID_TEMPLATE_CHUNK = each of --chunks (trimming off); the answers must be the same bytes
  combine_ms     call_ms with FID_TEMPLATE_COMBINE = atomics and pass (trimming off), alternating; the same bytes
One JSON line per shape is appended to --out.  There is no pass mark."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="10000:1000,100000:10000,1000000:100000,1000000:1")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--chunks", default="64,256,1024")
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrfd_arcface_facerecognition_amd import _lib  # noqa: E402
from scrfd_arcface_facerecognition_amd.engine import Gallery, _gallery_ptr  # noqa: E402

DIM, ROW = 512, 1024
if not args.no_torch:                                                                 # (torch takes the device first, as in bench.py)
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        sys.exit("bench_templates.py needs an MI355X (or --no-torch for the library's numbers alone)")
    torch.zeros(1, device="cuda")
ctx = _lib.Context(0)


def make_rows(n):
    """n rows around n / 10 centres; which person a row is filed under is decided per shape"""
    rng = np.random.default_rng(n)
    centres = rng.standard_normal(((n + 9) // 10, DIM), dtype=np.float32)
    x = centres[np.arange(n) // 10]
    x += 0.7 * rng.standard_normal((n, DIM), dtype=np.float32)
    return x


def device_ms(enqueue, reps):
    t = []
    for rep in range(reps + 1):
        ctx.sync()
        ctx.event_record(0)
        enqueue()
        ctx.event_record(1)
        ctx.sync()
        if rep:
            t.append(ctx.elapsed_ms(0, 1))
    return statistics.median(t), min(t)


stores = {}
for shape in args.shapes.split(","):
    n, P = (int(v) for v in shape.split(":"))
    if n not in stores:
        stores.clear()
        x = make_rows(n)
        gal = Gallery(ctx, x)
        del x
        g16 = ctx.borrow(_gallery_ptr(gal), (gal.Gp, DIM), np.float16).download()[:n]
        stores[n] = (gal, g16)
    gal, g16 = stores[n]
    rng = np.random.default_rng(P)
    # P = n / 10: a person is a centre; otherwise the centres are dealt out to the persons (P = 1: everybody is one person)
    labels = ((np.arange(n) // 10) % P).astype(np.int32)
    strangers = rng.random(n) < 0.01
    labels[strangers] = rng.integers(0, P, int(strangers.sum()))
    weights = rng.integers(1, 256, n).astype(np.int32)
    inp = ctx.to_device(np.concatenate([labels, weights]))
    tw = P * DIM // 2
    out = ctx.empty((12 + tw + 2 * n + 5 * P,), np.int32)
    at = lambda w: C.c_void_p(out.ptr + 4 * w)

    def call(min_score):
        _lib.check(ctx.lib.fid_gallery_templates(ctx.handle, gal.handle, None, C.c_void_p(inp.ptr), C.c_void_p(inp.ptr + 4 * n), n, P,
                                                 C.c_float(min_score), at(12), at(12 + tw), at(12 + tw + n), at(12 + tw + 2 * n),
                                                 at(12 + tw + 2 * n + 4 * P), at(0)))

    rec = {"tool": "bench_templates", "device": ctx.name(), "date": time.strftime("%Y-%m-%d"), "n": n, "P": P, "dim": DIM, "reps": args.reps,
           "chunk": _lib.TEMPLATE_CHUNK, "combine": "int64 atomics"}
    print(f"device: {ctx.name()}  n={n:,d}  P={P:,d}", flush=True)
    answers = {}
    for name, ms in (("keep_all", -2.0), ("trimmed", 0.5)):
        med, low = device_ms(lambda: call(ms), args.reps)
        got = out.download()
        person = got[12 + tw + 2 * n:12 + tw + 2 * n + 4 * P].reshape(P, 4)
        summary = got[:12].view(np.int64)
        again = int(person[person[:, 1] < person[:, 0], 1].sum()) if ms > -2 else 0
        must = (2 * int(summary[0]) + again) * ROW
        rec[name] = {"call_ms": med, "call_min_ms": low, "must_read_bytes": must, "read_GBps": must / med / 1e6, "summary": [int(v) for v in summary]}
        answers[name] = got
        print(f"  {name:9s} call {med:9.3f} ms (min {low:.3f})  reads {must / 1e6:9.1f} MB -> {must / med / 1e6:7.1f} GB/s  summary {[int(v) for v in summary]}", flush=True)
    rec["chunk_ms"] = {}
    for chunk in args.chunks.split(","):
        os.environ["FID_TEMPLATE_CHUNK"] = chunk                                      # (read per call)
        med, low = device_ms(lambda: call(-2.0), args.reps)
        same = np.array_equal(out.download(), answers["keep_all"])
        rec["chunk_ms"][chunk] = med
        print(f"  chunk {chunk:>5s}: {med:9.3f} ms (min {low:.3f})  same bytes: {same}", flush=True)
        assert same, "the chunk size changed the answer"
    os.environ.pop("FID_TEMPLATE_CHUNK", None)
    # how split persons combine: int64 atomics into one row per person, or partial rows and a second pass; alternating, the same bytes
    times = {"atomics": [], "pass": []}
    for rep in range(args.reps + 1):
        for how in times:
            os.environ["FID_TEMPLATE_COMBINE"] = how                                  # (read per call)
            med, _ = device_ms(lambda: call(-2.0), 1)
            if rep:
                times[how].append(med)
            assert np.array_equal(out.download(), answers["keep_all"]), "the combine path changed the answer"
    os.environ.pop("FID_TEMPLATE_COMBINE", None)
    rec["combine_ms"] = {how: statistics.median(t) for how, t in times.items()}
    rec["split_persons"] = int((answers["keep_all"][12 + tw + 2 * n:12 + tw + 2 * n + 4 * P].reshape(P, 4)[:, 0] > _lib.TEMPLATE_CHUNK).sum())
    print(f"  combine: atomics {rec['combine_ms']['atomics']:9.3f} ms   second pass {rec['combine_ms']['pass']:9.3f} ms   ({rec['split_persons']} split persons)", flush=True)
    if not args.no_torch:
        xt = torch.from_numpy(g16).cuda()
        lt, wt = torch.from_numpy(labels.astype(np.int64)).cuda(), torch.from_numpy(weights.astype(np.float32)).cuda()
        t = []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            S = torch.zeros((P, DIM), dtype=torch.float32, device="cuda")
            S.index_add_(0, lt, xt.float() * wt[:, None])
            T = F.normalize(S).half()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                t.append(e0.elapsed_time(e1))
        rec["torch_ms"] = statistics.median(t)
        # the device-to-device copy, through torch as well: read + write of the store
        dst = torch.empty_like(xt)
        c = []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(xt)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                c.append(e0.elapsed_time(e1))
        rec["copy_ms"] = statistics.median(c)
        rec["copy_GBps"] = 2 * n * ROW / rec["copy_ms"] / 1e6
        ours = answers["keep_all"][12:12 + tw].view(np.float16).astype(np.float32)
        cos = (ours.reshape(P, DIM) * T.float().cpu().numpy()).sum(1)
        rec["torch_min_cosine"] = float(cos.min())
        for name in ("keep_all", "trimmed"):
            rec[name]["read_fraction"] = rec[name]["read_GBps"] / rec["copy_GBps"]
        print(f"  torch index_add_ + normalize: {rec['torch_ms']:9.3f} ms   copy {rec['copy_GBps']:.0f} GB/s (read + write)   "
              f"read fraction {rec['keep_all']['read_fraction']:.2f} / {rec['trimmed']['read_fraction']:.2f}   min cosine to ours {cos.min():.6f}", flush=True)
        del xt, dst, S, T
        torch.cuda.empty_cache()
    if not args.no_host:
        tpl, score, kept = np.empty((P, DIM), np.float16), np.empty(n, np.float32), np.empty(n, np.int32)
        person, cohesion, summary = np.empty((P, 4), np.int32), np.empty(P, np.float32), np.empty(6, np.int64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        g = np.ascontiguousarray(g16)
        t0 = time.perf_counter()
        _lib.check(ctx.lib.fid_templates_host(p(g), n, DIM, None, p(labels), p(weights), n, P, C.c_float(-2.0), p(tpl), p(score), p(kept), p(person),
                                              p(cohesion), p(summary)))
        rec["host_ms"] = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(tpl.view(np.uint16).reshape(-1), answers["keep_all"][12:12 + tw].view(np.uint16))
        rec["host_equals_device"] = bool(same)
        print(f"  fid_templates_host: {rec['host_ms']:9.1f} ms   templates equal the device's: {same}", flush=True)
        assert same
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    del inp, out
