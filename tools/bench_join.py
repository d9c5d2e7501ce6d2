#!/usr/bin/env python3
"""Range join (fid_gallery_range) measurements for docs/FINDINGS.md: HIP-event times, median of 5 after one warm-up call.
  a. find_and_merge_duplicates at G = 16 384, via="matrix" (dense G x G through the host) against via="join", end to end
  b. self-join against the general join of the gallery with itself at G = 131 072 (the triangle should cost about half)
  c. self-join at G = 1 M in achieved TFLOP/s, under the default tile-pair order and three others (FID_RANGE_SUPER)
A random unit gallery with ~0.1 % planted near-copies; needs nothing outside the repository.  bench_join.py [a] [b] [c] runs a subset."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrfd_arcface_facerecognition_amd._lib import Context, check  # noqa: E402
from scrfd_arcface_facerecognition_amd.engine import Gallery, VectorGallery, _gallery_ptr  # noqa: E402

DIM, REPS, THRESH = 512, 5, 0.8
ctx = Context(0)
rng = np.random.default_rng(0)
which = set(sys.argv[1:]) or {"a", "b", "c"}


def planted(G):
    """[G, DIM] Gaussian rows, G / 1000 of them near-copies (cosine 0.85 .. 0.99) of another row -> (rows, number of planted pairs)"""
    x = rng.standard_normal((G, DIM), dtype=np.float32)
    k = max(1, G // 1000)
    dst, src = rng.permutation(G)[:2 * k].reshape(2, k)
    cos = rng.uniform(0.85, 0.99, (k, 1)).astype(np.float32)
    x[dst] = cos * x[src] + np.sqrt(1 - cos * cos) * x[dst]          # (rows of equal expected norm: the cosine is `cos` up to ~1 %)
    return x, k


def median_ms(fn, setup=None):
    """median of REPS event-timed calls after one warm-up; setup() runs untimed before each call -> (median ms, last result)"""
    ms, out = [], None
    for rep in range(REPS + 1):
        arg = setup() if setup else None
        ctx.sync()
        ctx.event_record(0)
        out = fn(arg) if setup else fn()
        ctx.event_record(1)
        t = ctx.elapsed_ms(0, 1)
        if rep:
            ms.append(t)
    return statistics.median(ms), out


def range_call(gal, q_ptr, n, cap=1 << 16):
    pairs, scores, total = ctx.empty((cap, 2), np.int32), ctx.empty((cap,), np.float32), ctx.empty((1,), np.uint64)

    def call():
        check(ctx.lib.fid_gallery_range(ctx.handle, gal.handle, C.c_void_p(q_ptr), n, THRESH, C.c_void_p(pairs.ptr), C.c_void_p(scores.ptr),
                                        cap, C.c_void_p(total.ptr)))
    return call, total


print(f"device: {ctx.name()}  ({time.strftime('%Y-%m-%d')})", flush=True)

if "a" in which:
    G = 16384
    emb, k = planted(G)
    ids = list(range(G))

    def store():
        vg = VectorGallery(ctx, DIM, capacity=G)
        vg.upsert(ids, emb)
        return vg
    res = {}
    for via in ("join", "matrix"):
        ms, merges = median_ms(lambda vg: vg.find_and_merge_duplicates(THRESH, via=via), setup=store)
        res[via] = (ms, merges)
        print(f"a. find_and_merge_duplicates G={G:,d} via={via:<6s}: {ms:10.2f} ms end to end, {len(merges)} merges ({k} planted)", flush=True)
    same = [(a, b) for a, b, _ in res["join"][1]] == [(a, b) for a, b, _ in res["matrix"][1]]
    print(f"a. same merges: {same}; matrix / join = {res['matrix'][0] / res['join'][0]:.1f}x", flush=True)

if "b" in which:
    G = 131072
    emb, k = planted(G)
    gal = Gallery(ctx, emb)
    del emb
    self_call, self_total = range_call(gal, 0, 0)
    full_call, full_total = range_call(gal, _gallery_ptr(gal), G, cap=1 << 18)
    ms_self, _ = median_ms(self_call)
    ms_full, _ = median_ms(full_call)
    ts, tf = int(self_total.download()[0]), int(full_total.download()[0])
    print(f"b. G={G:,d}: self-join {ms_self:9.2f} ms ({ts} pairs), general join with itself {ms_full:9.2f} ms ({tf} hits = 2 x {ts} + {G:,d}: {tf == 2 * ts + G}); "
          f"self / general = {ms_self / ms_full:.3f}  ({2.0 * DIM * G * G / ms_full / 1e9:.1f} TFLOP/s general)", flush=True)
    gal.close()

if "c" in which:
    G = 1_000_000
    emb, k = planted(G)
    gal = Gallery(ctx, emb)
    del emb
    self_call, self_total = range_call(gal, 0, 0)
    tiles = (G + 127) // 128
    useful = 2.0 * DIM * G * (G - 1) / 2
    issued = 2.0 * DIM * 128 * 128 * tiles * (tiles + 1) / 2
    for sw in (None, "1", "8", "32"):                     # the order the tile pairs are walked in: default (16 x 16 super-tiles), plain, 8, 32
        if sw:
            os.environ["FID_RANGE_SUPER"] = sw
        ms, _ = median_ms(self_call)
        print(f"c. G={G:,d} super-tile {sw or 'default'}: self-join {ms:9.2f} ms, {int(self_total.download()[0])} pairs ({k} planted): "
              f"{useful / ms / 1e9:.1f} TFLOP/s of pair products ({issued / ms / 1e9:.1f} counting the whole diagonal tiles)", flush=True)
    os.environ.pop("FID_RANGE_SUPER", None)
    gal.close()
