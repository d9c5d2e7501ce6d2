#!/usr/bin/env python3
"""Visit grouping (fid_gallery_group) measurements for docs/FINDINGS.md.
Synthetic identities: unit centres, every embedding at cosine ~0.75 from its centre (two members of one person ~0.56 from each other).  A store of
G existing persons (one member each) receives n visits in one call: about half are members of stored persons, a quarter belong to n / 16 new
persons seen four times each, 3 % are near-copies (0.99) of an earlier visit and the rest are persons seen once.
  device: fid_gallery_group between two HIP events (fid_event_*), median of 5 after one warm-up call, the store restored before every call (the
          rows the call wrote are zeroed again); part A alone = the same arg-max scan through fid_match_keys, parts B + C = the difference
  loop:   VectorGallery.group_visits(via="loop"), the reference's sequence one visit at a time on the entry points that existed before, as wall
          time on 1 024 visits; next to it the wall time of via="device" on the same visits (upload, normalisation and download included)
Needs nothing outside the repository.  bench_group.py [G ...] restricts the store sizes (default 1000 100000)."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrfd_arcface_facerecognition_amd._lib import Context, check  # noqa: E402
from scrfd_arcface_facerecognition_amd.engine import Gallery, VectorGallery, _gallery_ptr  # noqa: E402

DIM, REPS, INTRA = 512, 5, 0.75
THR = (0.95, 0.45, 0.4)                                   # duplicate, grouping, similarity (the reference's config.json defaults, search rounded up)
ctx = Context(0)
rng = np.random.default_rng(0)


def members(centres):
    """one embedding per row of `centres` at cosine ~INTRA from it (Gaussian noise of the centre's expected norm: the cosine holds to ~1 %)"""
    return (INTRA * centres + np.sqrt(1 - INTRA * INTRA) * rng.standard_normal(centres.shape, dtype=np.float32)).astype(np.float32)


def visits_for(stored_centres, n):
    kinds = rng.choice(4, n, p=[0.5, 0.25, 0.03, 0.22])   # stored person, new person seen four times, near-copy, person seen once
    new_centres = rng.standard_normal((max(1, n // 16), DIM), dtype=np.float32)
    out = np.empty((n, DIM), np.float32)
    k = kinds == 0
    out[k] = members(stored_centres[rng.integers(0, len(stored_centres), int(k.sum()))])
    k = kinds == 1
    out[k] = members(new_centres[rng.integers(0, len(new_centres), int(k.sum()))])
    k = kinds == 3
    out[k] = rng.standard_normal((int(k.sum()), DIM), dtype=np.float32)
    for i in np.nonzero(kinds == 2)[0]:
        src = out[int(rng.integers(0, i))] if i else rng.standard_normal(DIM, dtype=np.float32)
        out[i] = 0.99 * src + np.sqrt(1 - 0.99 ** 2) * np.linalg.norm(src) / np.sqrt(DIM) * rng.standard_normal(DIM, dtype=np.float32)
    return out


def median_ms(fn, setup):
    ms = []
    for rep in range(REPS + 1):
        setup()
        ctx.sync()
        ctx.event_record(0)
        fn()
        ctx.event_record(1)
        t = ctx.elapsed_ms(0, 1)
        if rep:
            ms.append(t)
    return statistics.median(ms)


print(f"device: {ctx.name()}  ({time.strftime('%Y-%m-%d')})", flush=True)
for G in [int(a) for a in sys.argv[1:]] or [1000, 100000]:
    centres = rng.standard_normal((G, DIM), dtype=np.float32)
    stored = members(centres)
    for n in (1024, 16384):
        visits = visits_for(centres, n)
        gal = Gallery(ctx, np.concatenate([stored, np.zeros((n, DIM), np.float32)]))        # rows G .. G + n - 1 are free
        base = _gallery_ptr(gal)
        e, q = ctx.to_device(visits), ctx.empty((n, DIM), np.float16)
        check(ctx.lib.fid_l2_normalize_f16(ctx.handle, C.c_void_p(e.ptr), n, DIM, C.c_void_p(q.ptr)))
        new_rows = ctx.to_device(np.arange(G, G + n, dtype=np.int32))
        verdict, row, score = ctx.empty((n,), np.int32), ctx.empty((n,), np.int32), ctx.empty((n,), np.float32)
        summary, keys = ctx.empty((2,), np.int32), ctx.empty((n,), np.uint64)

        def restore():
            check(ctx.lib.fid_memset(ctx.handle, C.c_void_p(base + G * DIM * 2), 0, n * DIM * 2))

        def group():
            check(ctx.lib.fid_gallery_group(ctx.handle, gal.handle, C.c_void_p(q.ptr), n, C.c_float(THR[0]), C.c_float(THR[1]), C.c_float(THR[2]),
                                            C.c_void_p(new_rows.ptr), n, C.c_void_p(verdict.ptr), C.c_void_p(row.ptr), C.c_void_p(score.ptr),
                                            C.c_void_p(summary.ptr)))

        def scan():
            check(ctx.lib.fid_match_keys(ctx.handle, gal.handle, C.c_void_p(q.ptr), n, 0, C.c_void_p(keys.ptr)))

        ms = median_ms(group, restore)
        ms_a = median_ms(scan, restore)
        counts = np.bincount(verdict.download(), minlength=5)
        blocks = (n + 127) // 128
        print(f"G={G:>7,d} n={n:>6,d}: {ms:8.3f} ms per call = {n / ms * 1e3:>11,.0f} visits/s; part A (gallery scan) {ms_a:7.3f} ms, parts B + C "
              f"{ms - ms_a:7.3f} ms; {2 * blocks + 2} launches (memset, prepare, the scan counted as one, {blocks} resolve, {blocks - 1} cross); "
              f"new {counts[0]}, recognised {counts[1]}, duplicate {counts[2]}, no face {counts[3]}, deferred {counts[4]}", flush=True)
        gal.close()
        if n == 1024:
            wall = {}
            for via in ("loop", "device"):
                vg = VectorGallery(ctx, DIM, capacity=G + 2 * n)
                vg.upsert(list(range(G)), stored)
                vg.group_visits(visits[:8], duplicate_threshold=THR[0], grouping_threshold=THR[1], similarity_threshold=THR[2], via=via)   # warm-up
                ctx.sync()
                t0 = time.perf_counter()
                recs = vg.group_visits(visits, duplicate_threshold=THR[0], grouping_threshold=THR[1], similarity_threshold=THR[2], via=via)
                wall[via] = (time.perf_counter() - t0) * 1e3, [r["verdict"] for r in recs]
                vg._gal.close()
            same = sum(a == b for a, b in zip(wall["loop"][1], wall["device"][1]))
            print(f"G={G:>7,d} n={n:>6,d}: via=loop {wall['loop'][0]:9.1f} ms wall ({n / wall['loop'][0] * 1e3:,.0f} visits/s), via=device "
                  f"{wall['device'][0]:8.2f} ms wall end to end; loop / device = {wall['loop'][0] / wall['device'][0]:.0f}x wall, "
                  f"{wall['loop'][0] / ms:.0f}x against the call's event time; same verdict on {same} of {n} visits", flush=True)
