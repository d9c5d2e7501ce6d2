#!/usr/bin/env python3
"""Clustering (VectorGallery.cluster on fid_gallery_cluster) measurements for docs/FINDINGS.md, "clustering".  One process, one store.

  bench_cluster.py --G 10000 --cluster 32 [--share 0.1] [--thresh 0.9] [--reps 5] [--tree DIR] [--out profiles/cluster/bench_cluster.jsonl]

The store is bench_dedup.py's planted(): G persons with shuffled integer ids, `share` of them near-copies in clusters of `cluster` rows
(cosine >= 0.9 inside a cluster).  Measured, each the median of --reps runs after one warm-up run that sizes the arenas:
  cluster        VectorGallery.cluster(thresh, 2) and its `clusters` view, wall, end to end: upload of the rows, the call, one download -- with
                 the tile-pair bitmap skip on (the default) and off (FID_CLUSTER_SKIP=0); the two answers must be equal
  cluster_device fid_gallery_cluster alone between device events, skip on and off
  pairs          today's only other route: VectorGallery.similar_pairs(thresh) and a union-find over the pair list on the host, wall; at
                 min_samples = 1 its clusters must be VectorGallery.cluster's
  join_device    fid_gallery_range's self-join kernel alone between device events: the yardstick for ONE triangular pass
--tree imports the package from another checkout (a build of the parent commit): a tree without VectorGallery.cluster runs `pairs` and
`join_device` only, so the two routes can be compared on the same box in the same session.  One JSON line per run is appended to --out."""
import argparse
import ast
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--G", type=int, default=10000)
ap.add_argument("--share", type=float, default=0.1)
ap.add_argument("--cluster", type=int, default=2)
ap.add_argument("--thresh", type=float, default=0.9)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
args = ap.parse_args()

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(args.tree))
from scrfd_arcface_facerecognition_amd import _lib  # noqa: E402
from scrfd_arcface_facerecognition_amd.engine import VectorGallery  # noqa: E402

DIM = 512


def planted_of_bench_dedup():
    """bench_dedup.py's planted() as it stands there (that file is a script: importing it would run it)"""
    path = os.path.join(HERE, "bench_dedup.py")
    tree = ast.parse(open(path).read())
    fn = next(node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "planted")
    ns = {"np": np, "DIM": DIM}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["planted"]


def median_ms(fn, reps):
    out = None
    times = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), out


def device_ms(ctx, enqueue, reps):
    times = []
    for rep in range(reps + 1):
        ctx.sync()
        ctx.event_record(0)
        enqueue()
        ctx.event_record(1)
        ctx.sync()
        if rep:
            times.append(ctx.elapsed_ms(0, 1))
    return statistics.median(times), min(times)


def clustered(res):
    """the part of the answer the pair route also builds: the clusters as lists of ids (the result object builds its views on first use)"""
    res.clusters
    return res


def components(ids, pairs):
    """union-find over a pair list, the lower id as the root -> clusters as VectorGallery.cluster orders them"""
    parent = {i: i for i in ids}

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for a, b, _ in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    groups = {}
    for i in sorted(ids):
        groups.setdefault(find(i), []).append(i)
    return [groups[k] for k in sorted(groups)]


ctx = _lib.Context(0)
emb, ids, n_clusters = planted_of_bench_dedup()(args.G, args.share, args.cluster)
vg = VectorGallery(ctx, DIM, capacity=len(ids))
vg.upsert(ids, emb)
ctx.sync()
has_cluster = hasattr(vg, "cluster")
rec = {"tool": "bench_cluster", "device": ctx.name(), "date": time.strftime("%Y-%m-%d"), "tree": "this" if has_cluster else "parent", "G": args.G,
       "share": args.share, "cluster": args.cluster, "planted_clusters": n_clusters, "thresh": args.thresh, "reps": args.reps}
print(f"device: {ctx.name()}  tree: {os.path.abspath(args.tree)}", flush=True)
print(f"G={args.G:,d}, {n_clusters:,d} clusters of {args.cluster}, threshold {args.thresh}", flush=True)

os.environ.pop("FID_CLUSTER_SKIP", None)
rec["pairs_wall_ms"], rec["pairs_wall_min_ms"], by_pairs = median_ms(lambda: components(ids, vg.similar_pairs(args.thresh)), args.reps)
pairs = vg.similar_pairs(args.thresh)
rec["pairs"] = len(pairs)
rec["pairs_bytes"] = 12 * len(pairs) + 8
print(f"pairs         : {rec['pairs_wall_ms']:9.2f} ms wall (min {rec['pairs_wall_min_ms']:.2f}), {len(pairs):,d} pairs, {rec['pairs_bytes']:,d} bytes", flush=True)

cap = max(1, len(pairs))
pd, sd, td = ctx.empty((cap, 2), np.int32), ctx.empty((cap,), np.float32), ctx.empty((1,), np.uint64)
join = lambda: _lib.check(ctx.lib.fid_gallery_range(ctx.handle, vg._gal.handle, None, 0, C.c_float(args.thresh), C.c_void_p(pd.ptr),
                                                    C.c_void_p(sd.ptr), cap, C.c_void_p(td.ptr)))
rec["join_device_ms"], rec["join_device_min_ms"] = device_ms(ctx, join, args.reps)
print(f"join_device   : {rec['join_device_ms']:9.3f} ms (min {rec['join_device_min_ms']:.3f})", flush=True)

if has_cluster:
    n = len(ids)
    rows_dev = ctx.to_device(np.asarray([vg.row_of[i] for i in sorted(ids)], dtype=np.int32))
    out = ctx.empty((4 * n + 6,), np.int32)
    call = lambda: _lib.check(ctx.lib.fid_gallery_cluster(ctx.handle, vg._gal.handle, C.c_void_p(rows_dev.ptr), n, C.c_float(args.thresh), 2,
                                                          C.c_void_p(out.ptr), C.c_void_p(out.ptr + 4 * n), C.c_void_p(out.ptr + 8 * n),
                                                          C.c_void_p(out.ptr + 12 * n), C.c_void_p(out.ptr + 16 * n)))
    answers = {}
    for skip in ("1", "0"):
        os.environ["FID_CLUSTER_SKIP"] = skip
        tag = "skip" if skip == "1" else "noskip"
        rec[f"cluster_{tag}_wall_ms"], rec[f"cluster_{tag}_wall_min_ms"], res = median_ms(lambda: clustered(vg.cluster(args.thresh, 2)), args.reps)
        rec[f"cluster_{tag}_device_ms"], rec[f"cluster_{tag}_device_min_ms"] = device_ms(ctx, call, args.reps)
        answers[tag] = res
        print(f"cluster {tag:<6s}: {rec[f'cluster_{tag}_wall_ms']:9.2f} ms wall (min {rec[f'cluster_{tag}_wall_min_ms']:.2f}), "
              f"{rec[f'cluster_{tag}_device_ms']:9.3f} ms device (min {rec[f'cluster_{tag}_device_min_ms']:.3f}), counts {res.counts}", flush=True)
    os.environ.pop("FID_CLUSTER_SKIP", None)
    a, b = answers["skip"], answers["noskip"]
    assert a.labels == b.labels and a.degree == b.degree and a.via == b.via, "the bitmap skip changed the answer"
    assert vg.cluster(args.thresh, 1).clusters == by_pairs, "min_samples = 1 and the union-find of similar_pairs disagree"
    rec["counts"] = a.counts
    rec["cluster_bytes"] = 16 * n + 24
    rec["same_as_pairs_at_min_samples_1"] = True
    print(f"pairs / cluster: wall {rec['pairs_wall_ms'] / rec['cluster_skip_wall_ms']:.2f}x, bytes {rec['pairs_bytes'] / rec['cluster_bytes']:.2f}x; "
          f"cluster device / join device: skip {rec['cluster_skip_device_ms'] / rec['join_device_ms']:.2f}x, "
          f"no skip {rec['cluster_noskip_device_ms'] / rec['join_device_ms']:.2f}x", flush=True)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
