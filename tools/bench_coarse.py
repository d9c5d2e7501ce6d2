#!/usr/bin/env python3
"""Two-stage gallery search against the exact fused search: fid_gallery_search (k = 5) and fid_gallery_search_coarse (k = 5, R in {5, 16, 32}) on
n in {64, 1 024, 10 000} x G in {100 k, 1 M} at dim 512, and the three stages of the coarse path on their own -- fid_coarse_keys (query
quantisation, int8 scan, list merge), fid_rerank_keys, fid_topk_merge.  One process, HIP events around every call, the candidates taken in turn
inside every repeat (so drift hits them alike), one warm-up round, the median of --repeats timed rounds.  recall@k = the share of the exact
search's hits the coarse path reports too, on random-normal rows (every shape) and on clustered rows (persons of eight near-duplicate rows, the
queries near-duplicates of stored persons; n = 1 024 only: it needs a second gallery).  One JSON line per shape.

    python tools/bench_coarse.py [--repeats 7] [--shapes 100000x64,1000000x10000]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrfd_arcface_facerecognition_amd._lib import Context, check  # noqa: E402
from scrfd_arcface_facerecognition_amd.engine import Gallery  # noqa: E402

DIM, K = 512, 5
RS = (5, 16, 32)
GS, NS = (100_000, 1_000_000), (64, 1024, 10_000)
PERSON_ROWS, SPREAD = 8, 0.5                          # clustered rows: centre + SPREAD * noise, both unit-variance normal per element
CLUSTER_N = 1024


def recall(exact_idx, coarse_idx):
    hit = total = 0
    for e, c in zip(exact_idx, coarse_idx):
        e = set(int(j) for j in e if j >= 0)
        hit += len(e & set(int(j) for j in c if j >= 0))
        total += len(e)
    return hit / total if total else 1.0


def unit_queries(ctx, emb):
    e = ctx.to_device(np.ascontiguousarray(emb, np.float32))
    q = ctx.empty(emb.shape, np.float16)
    check(ctx.lib.fid_l2_normalize_f16(ctx.handle, C.c_void_p(e.ptr), emb.shape[0], DIM, C.c_void_p(q.ptr)))
    return q


def quantised_gallery(ctx, rows):
    gal = Gallery(ctx, rows)
    ctx.event_record(0)
    check(ctx.lib.fid_gallery_quantize(ctx.handle, gal.handle))
    ctx.event_record(1)
    return gal, ctx.elapsed_ms(0, 1)


def searches(ctx, gal, q, n):
    """-> {name: (idx, score)} of the exact search and the coarse search at every R, downloaded"""
    lib, h = ctx.lib, ctx.handle
    idx, sc = ctx.empty((n, K), np.int32), ctx.empty((n, K), np.float32)
    out = {}
    check(lib.fid_gallery_search(h, gal.handle, C.c_void_p(q.ptr), n, K, 0.0, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)))
    out["exact"] = (idx.download(), sc.download())
    for R in RS:
        check(lib.fid_gallery_search_coarse(h, gal.handle, C.c_void_p(q.ptr), n, K, R, 0.0, C.c_void_p(idx.ptr), C.c_void_p(sc.ptr)))
        out[R] = (idx.download(), sc.download())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", default="", help="comma-separated GxN; default: every G x n of the module docstring")
    args = ap.parse_args()
    assert args.repeats >= 5
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",") if s] or [(G, n) for G in GS for n in NS]
    ctx = Context(0)
    rng = np.random.default_rng(0)
    gal, gal_G, quant_ms, clustered = None, None, None, None
    for G, n in shapes:
        if G != gal_G:                                    # (shapes of one G share the gallery: 2 GB of host rows at 1 M)
            if gal is not None:
                gal.close()
            persons = max(1, G // PERSON_ROWS)
            centres = rng.standard_normal((persons, DIM), dtype=np.float32)
            rows = rng.standard_normal((G, DIM), dtype=np.float32)
            rows *= np.float32(SPREAD)
            for r0 in range(0, G, 65536):                 # (in pieces: no second 2 GB array at 1 M rows)
                rows[r0:r0 + 65536] += centres[np.arange(r0, min(G, r0 + 65536)) % persons]
            cgal, _ = quantised_gallery(ctx, rows)
            cn = min(CLUSTER_N, persons)
            cq = unit_queries(ctx, centres[rng.permutation(persons)[:cn]] + np.float32(SPREAD) * rng.standard_normal((cn, DIM), dtype=np.float32))
            got = searches(ctx, cgal, cq, cn)
            clustered = dict(n=cn, persons=persons, rows_per_person=PERSON_ROWS, spread=SPREAD,
                             recall={"R%d" % R: round(recall(got["exact"][0], got[R][0]), 5) for R in RS},
                             mean_top1_score=round(float(got["exact"][1][:, 0].mean()), 4))
            cgal.close()
            del rows, centres, cgal
            rows = rng.standard_normal((G, DIM), dtype=np.float32)
            (gal, quant_ms), gal_G = quantised_gallery(ctx, rows), G
            del rows
        q = unit_queries(ctx, rng.standard_normal((n, DIM), dtype=np.float32))
        lib, h, g, qp = ctx.lib, ctx.handle, gal.handle, C.c_void_p(q.ptr)
        idx, sc = ctx.empty((n, K), np.int32), ctx.empty((n, K), np.float32)
        keys_c, keys_e = ctx.empty((n, max(RS)), np.uint64), ctx.empty((n, max(RS)), np.uint64)
        ip, sp, kc, ke = C.c_void_p(idx.ptr), C.c_void_p(sc.ptr), C.c_void_p(keys_c.ptr), C.c_void_p(keys_e.ptr)
        calls = {"search5": lambda: check(lib.fid_gallery_search(h, g, qp, n, K, 0.0, ip, sp))}
        for R in RS:
            calls["coarse5_R%d" % R] = lambda R=R: check(lib.fid_gallery_search_coarse(h, g, qp, n, K, R, 0.0, ip, sp))
        for R in RS:                                      # the stages on their own (each reads what the one before it wrote in this round)
            calls["scan_R%d" % R] = lambda R=R: check(lib.fid_coarse_keys(h, g, qp, n, R, 0, kc))
            calls["rerank_R%d" % R] = lambda R=R: check(lib.fid_rerank_keys(h, g, qp, n, R, 0, kc, ke))
            calls["merge_R%d" % R] = lambda R=R: check(lib.fid_topk_merge(h, ke, 1, n, R, G, 0.0, C.c_void_p(wide[0].ptr), C.c_void_p(wide[1].ptr)))
        wide = (ctx.empty((n, max(RS)), np.int32), ctx.empty((n, max(RS)), np.float32))     # (the public merge takes [n, R] keys at k = R)
        ms = {name: [] for name in calls}
        for rep in range(args.repeats + 1):               # round 0 warms up (scratch arenas, code objects, caches)
            for name, call in calls.items():
                ctx.event_record(0)
                call()
                ctx.event_record(1)
                t = ctx.elapsed_ms(0, 1)
                if rep:
                    ms[name].append(t)
        med = {name: statistics.median(v) for name, v in ms.items()}
        got = searches(ctx, gal, q, n)
        both = [(got[32][1][r, c], got["exact"][1][r, list(got["exact"][0][r]).index(j)]) for r in range(min(n, 1024))
                for c, j in enumerate(got[32][0][r]) if j >= 0 and j in got["exact"][0][r]]
        line = dict(G=G, n=n, dim=DIM, k=K, repeats=args.repeats, ms={k: round(v, 4) for k, v in med.items()},
                    ms_min={k: round(min(v), 4) for k, v in ms.items()}, ms_max={k: round(max(v), 4) for k, v in ms.items()},
                    coarse_over_search={"R%d" % R: round(med["coarse5_R%d" % R] / med["search5"], 3) for R in RS},
                    scan_tops={"R%d" % R: round(2.0 * DIM * G * n / med["scan_R%d" % R] / 1e9, 1) for R in RS},
                    search_tflops=round(2.0 * DIM * G * n / med["search5"] / 1e9, 1),
                    scan_gbytes_per_s={"R%d" % R: round(float(G) * DIM / med["scan_R%d" % R] / 1e6, 1) for R in RS},
                    quantize_gallery_ms=round(quant_ms, 3),
                    recall_random={"R%d" % R: round(recall(got["exact"][0], got[R][0]), 5) for R in RS},
                    recall_clustered=clustered,
                    score_max_diff_R32=float(max((abs(float(a) - float(b)) for a, b in both), default=0.0)),
                    device=ctx.name())
        print(json.dumps(line), flush=True)
    if gal is not None:
        gal.close()
    ctx.close()


if __name__ == "__main__":
    main()
