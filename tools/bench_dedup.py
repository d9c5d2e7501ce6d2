#!/usr/bin/env python3
"""Duplicate merge (VectorGallery.find_and_merge_duplicates) measurements for docs/FINDINGS.md, "device dedup": the three `via` values on identical
twin stores -- wall time end to end (median of --reps runs after one warm-up run that sizes the arenas), bytes downloaded, merges -- and an
assertion that the merge lists are equal.

  bench_dedup.py --G 10000 --share 0.1 --cluster 32 [--vias device,join,matrix] [--reps 5] [--tree DIR]

The store holds G persons with shuffled integer ids; `share` of them are planted near-copies in clusters of `cluster` rows (cosine >= 0.9 inside a
cluster, so a cluster of m rows is m (m - 1) / 2 pairs for the join and m - 1 merges).  via="matrix" is left out above --matrix-limit persons (its
host matrix is G x G fp32).  --tree imports the package from another checkout (a build of the parent commit, as the tools/ab*.sh helpers compare
builds): a tree without via="device" runs the other two; the printed digest of the merge list compares runs of different processes."""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--G", type=int, default=10000)
ap.add_argument("--share", type=float, default=0.1)
ap.add_argument("--cluster", type=int, default=2)
ap.add_argument("--vias", default="device,join,matrix")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--thresh", type=float, default=0.8)
ap.add_argument("--matrix-limit", type=int, default=20000)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.tree))
from scrfd_arcface_facerecognition_amd import _lib  # noqa: E402
from scrfd_arcface_facerecognition_amd.engine import VectorGallery  # noqa: E402

DIM = 512
ctx = _lib.Context(0)

downloaded = [0]
_download = _lib.DeviceBuffer.download


def counting_download(self, count_bytes=None):
    downloaded[0] += self.nbytes if count_bytes is None else count_bytes
    return _download(self, count_bytes)


_lib.DeviceBuffer.download = counting_download


def planted(G, share, cluster, seed=0):
    """-> emb [G, DIM] fp32, ids (shuffled integers), number of clusters"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((G, DIM), dtype=np.float32)
    n_clusters = int(G * share) // cluster
    members = rng.permutation(G)[:n_clusters * cluster].reshape(n_clusters, cluster)
    centre = rng.standard_normal((n_clusters, 1, DIM), dtype=np.float32)
    centre /= np.linalg.norm(centre, axis=2, keepdims=True)
    noise = x[members] / np.linalg.norm(x[members], axis=2, keepdims=True)
    cos = rng.uniform(0.955, 0.995, (n_clusters, cluster, 1)).astype(np.float32)           # any two members: >= 0.955^2 - noise overlap > 0.9
    x[members] = (cos * centre + np.sqrt(1 - cos * cos) * noise) * rng.uniform(0.5, 2.0, (n_clusters, cluster, 1)).astype(np.float32)
    ids = [int(i) for i in rng.permutation(4 * G)[:G]]
    return x, ids, n_clusters


def store(emb, ids):
    vg = VectorGallery(ctx, DIM, capacity=len(ids))
    vg.upsert(ids, emb)
    ctx.sync()
    return vg


def digest(merges):
    return hashlib.sha1(repr([(a, b) for a, b, _ in merges]).encode()).hexdigest()[:12]


emb, ids, n_clusters = planted(args.G, args.share, args.cluster)
vias = [v for v in args.vias.split(",") if v]
if args.G > args.matrix_limit and "matrix" in vias:
    vias.remove("matrix")
    print(f"via=matrix left out: {args.G:,d} persons > --matrix-limit {args.matrix_limit:,d}", flush=True)
print(f"device: {ctx.name()}  ({time.strftime('%Y-%m-%d')})  tree: {os.path.abspath(args.tree)}", flush=True)
print(f"G={args.G:,d} persons, {n_clusters:,d} clusters of {args.cluster} ({n_clusters * args.cluster:,d} planted rows, "
      f"{n_clusters * args.cluster * (args.cluster - 1) // 2:,d} planted pairs), threshold {args.thresh}", flush=True)

results = {}
for via in vias:
    times, merges, nbytes = [], None, 0
    try:
        for rep in range(args.reps + 1):
            vg = store(emb, ids)
            downloaded[0] = 0
            t0 = time.perf_counter()
            merges = vg.find_and_merge_duplicates(args.thresh, via=via)
            dt = (time.perf_counter() - t0) * 1e3
            nbytes = downloaded[0]
            if rep:
                times.append(dt)
            left = len(vg)
            vg._gal.close()
    except ValueError as e:                                                         # a tree that does not know this `via`
        print(f"via={via:<6s}: not available in this tree ({e})", flush=True)
        continue
    results[via] = (statistics.median(times), nbytes, merges)
    print(f"via={via:<6s}: {statistics.median(times):10.2f} ms wall (median of {args.reps}; min {min(times):.2f}), {nbytes:>14,d} bytes downloaded, "
          f"{len(merges):,d} merges, {left:,d} persons left, merge list {digest(merges)}", flush=True)

ref = None
for via, (_, _, merges) in results.items():
    pairs = [(a, b) for a, b, _ in merges]
    if ref is None:
        ref = (via, pairs, merges)
        continue
    assert pairs == ref[1], f"via={via} and via={ref[0]} disagree"
    assert max((abs(m[2] - r[2]) for m, r in zip(merges, ref[2])), default=0.0) < 1e-3
if len(results) > 1:
    print(f"same merge list from {', '.join(results)}: True", flush=True)
if "device" in results:
    for other in ("join", "matrix"):
        if other in results:
            print(f"{other} / device: wall {results[other][0] / results['device'][0]:.2f}x, bytes {results[other][1] / max(1, results['device'][1]):.1f}x",
                  flush=True)
