#!/usr/bin/env python3
"""Top-k gallery search, fused against the score-matrix path: fid_match (the arg-max scan, the floor for any scan of the gallery),
fid_gallery_topk (k = 5, the n x G scores through HBM) and fid_gallery_search (k = 5 and k = 32) on G in {1 k, 100 k, 1 M} x n in {1, 512, 10 000}
at dim 512.  One process, HIP events around every call, the candidates taken in turn inside every repeat (so drift hits them alike), one
warm-up round, the median of --repeats timed rounds.  One JSON line per shape; the two top-5 answers are compared on the way.

    python tools/bench_topk.py [--repeats 7] [--shapes 1000x1,1000000x10000]"""
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

DIM = 512
GS, NS = (1000, 100_000, 1_000_000), (1, 512, 10_000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", default="", help="comma-separated GxN; default: every G x n of the module docstring")
    args = ap.parse_args()
    assert args.repeats >= 5
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",") if s] or [(G, n) for G in GS for n in NS]
    ctx = Context(0)
    rng = np.random.default_rng(0)
    gal, gal_G = None, None
    for G, n in shapes:
        if G != gal_G:                                    # (shapes of one G share the gallery: 2 GB of host rows at 1 M)
            if gal is not None:
                gal.close()
            rows = rng.standard_normal((G, DIM), dtype=np.float32)
            gal, gal_G = Gallery(ctx, rows), G
            del rows
        e = ctx.to_device(rng.standard_normal((n, DIM), dtype=np.float32))
        q = ctx.empty((n, DIM), np.float16)
        check(ctx.lib.fid_l2_normalize_f16(ctx.handle, C.c_void_p(e.ptr), n, DIM, C.c_void_p(q.ptr)))
        out = {k: (ctx.empty((n, k), np.int32), ctx.empty((n, k), np.float32)) for k in (1, 5, 32)}
        old5 = (ctx.empty((n, 5), np.int32), ctx.empty((n, 5), np.float32))
        lib, h, g, qp = ctx.lib, ctx.handle, gal.handle, C.c_void_p(q.ptr)

        def ptrs(pair):
            return C.c_void_p(pair[0].ptr), C.c_void_p(pair[1].ptr)
        calls = {"match": lambda: check(lib.fid_match(h, g, qp, n, 0.0, *ptrs(out[1]))),
                 "topk5": lambda: check(lib.fid_gallery_topk(h, g, qp, n, 5, 0.0, *ptrs(old5))),
                 "search5": lambda: check(lib.fid_gallery_search(h, g, qp, n, 5, 0.0, *ptrs(out[5]))),
                 "search32": lambda: check(lib.fid_gallery_search(h, g, qp, n, 32, 0.0, *ptrs(out[32])))}
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
        i_old, s_old, i_new, s_new = old5[0].download(), old5[1].download(), out[5][0].download(), out[5][1].download()
        line = dict(G=G, n=n, dim=DIM, repeats=args.repeats, ms={k: round(v, 4) for k, v in med.items()},
                    ms_min={k: round(min(v), 4) for k, v in ms.items()}, ms_max={k: round(max(v), 4) for k, v in ms.items()},
                    topk5_over_search5=round(med["topk5"] / med["search5"], 3), search5_over_match=round(med["search5"] / med["match"], 3),
                    search32_over_search5=round(med["search32"] / med["search5"], 3),
                    scan_tflops_search5=round(2.0 * DIM * G * n / med["search5"] / 1e9, 1),
                    top5_rows_equal=float((i_old == i_new).mean()), top5_scores_max_diff=float(np.abs(s_old - s_new).max()),
                    device=ctx.name())
        print(json.dumps(line), flush=True)
    if gal is not None:
        gal.close()
    ctx.close()


if __name__ == "__main__":
    main()
