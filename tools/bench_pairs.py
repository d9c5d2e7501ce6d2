#!/usr/bin/env python3
"""1:1 verification of image pairs, FaceAnalysis.compare_pairs against the route a user had before it: FaceAnalysis.get_batch on all 2 P images
(every face of every image aligned and embedded, two fp32 embedding matrices downloaded) and the reference's formula in numpy on faces[0] of
each image (smart_face_recognition.py:925-932, :978).  SCRFD-10G at 640 x 640 + IResNet-50, synthetic weights, the detector's bias calibrated
on the letterboxed images so that every image is crowded; the images are block noise in four interleaved sizes and start on the host, as a
caller's images do.

Both routes run in one process on the same images, taken in turn inside every repeat; each call ends in a download, so the host clock around it
covers upload, device work and read-back.  One warm-up round, then the median of --repeats rounds.  One JSON line per shape (P pairs); the two
routes' verdicts and scores are compared on the way.

    python tools/bench_pairs.py [--repeats 7] [--pairs 8,64]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1080, 1920), (720, 1280), (480, 853), (640, 640)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", default="8,64", help="comma-separated numbers of pairs")
    ap.add_argument("--threshold", type=float, default=0.4)
    ap.add_argument("--target", type=int, default=48, help="anchors above 0.5 the calibration leaves in the quietest calibration frame")
    args = ap.parse_args()
    assert args.repeats >= 5
    os.environ.setdefault("FID_AUTOTUNE", "0")            # heuristic kernel plans on both routes: get_batch meets many recogniser batch sizes

    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.app import FaceAnalysis
    from scrfd_arcface_facerecognition_amd.models import SCRFD
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    from scrfd_arcface_facerecognition_amd.session import HipSession

    app = FaceAnalysis("synthetic:scrfd_10g", "synthetic:arcface_r50", det_size=(640, 640), max_faces=64)
    ctx = app.ctx
    rng = np.random.default_rng(1234)
    det_net = archs.scrfd_10g((640, 640))

    def noise(i):
        """image i: size i % 4; noise drawn at the size the letterbox reduces it to and repeated up, so that the detector input keeps its contrast"""
        H, W = SIZES[i % len(SIZES)]
        k = max(1, min(H // 360, W // 640))
        lo = rng.integers(0, 256, (-(-H // k), -(-W // k), 3), dtype=np.uint8)
        return np.ascontiguousarray(np.repeat(np.repeat(lo, k, axis=0), k, axis=1)[:H, :W])

    # calibrate on what the detector will see: eight such images through the device letterbox (every size twice)
    sample = ctx.image_batch([noise(i) for i in range(8)])
    calib_dev = ctx.empty((8, 640, 640, 3), np.uint8)
    check(ctx.lib.fid_letterbox_ragged(ctx.handle, *sample.args(), 8, C.c_void_p(calib_dev.ptr), 640, 640, None))
    calib = calib_dev.download()
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, seed=0), calib, target=args.target)
    det = SCRFD("synthetic:scrfd_10g", input_size=(640, 640), conf_thres=0.5, ctx=ctx, max_batch=8)
    det.session = HipSession(None, ctx=ctx, net=det_net, params=det_P, max_batch=8)
    app.det = det

    for P in [int(v) for v in args.pairs.split(",") if v]:
        images = [noise(i) for i in range(2 * P)]
        A, B = images[0::2], images[1::2]
        state = {}

        def pairs_route():
            state["res"], state["counters"] = app.compare_pairs(A, B, args.threshold)

        def batch_route():
            faces = app.get_batch(images)
            state["faces"] = [len(f) for f in faces]
            sims = []
            for p in range(P):
                fa, fb = faces[2 * p], faces[2 * p + 1]
                if not fa or not fb:
                    sims.append(None)
                    continue
                e1, e2 = fa[0].embedding, fb[0].embedding
                sims.append(float(np.dot(e1, e2) / (np.linalg.norm(e1) * np.linalg.norm(e2))))
            state["sims"] = sims

        routes = {"compare_pairs": pairs_route, "get_batch_numpy": batch_route}
        ms = {name: [] for name in routes}
        for rep in range(args.repeats + 1):               # round 0 warms up (kernel plans per batch size, scratch arenas, code objects)
            for name, fn in routes.items():
                ctx.sync()
                t0 = time.perf_counter()
                fn()
                ctx.sync()
                if rep:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        med = {name: statistics.median(v) for name, v in ms.items()}
        both = [(r, s) for r, s in zip(state["res"], state["sims"]) if r["error"] is None and s is not None]
        line = dict(tool="bench_pairs", pairs=P, images=2 * P, sizes=SIZES, det="scrfd_10g", rec="arcface_r50", repeats=args.repeats,
                    autotune=os.environ["FID_AUTOTUNE"], faces_per_image_mean=round(float(np.mean(state["faces"])), 2),
                    faces_embedded={"compare_pairs": int(sum(1 for f in state["faces"] if f)), "get_batch_numpy": int(sum(state["faces"]))},
                    ms={k: round(v, 3) for k, v in med.items()}, ms_min={k: round(min(v), 3) for k, v in ms.items()},
                    ms_max={k: round(max(v), 3) for k, v in ms.items()},
                    get_batch_over_compare_pairs=round(med["get_batch_numpy"] / med["compare_pairs"], 3),
                    counters=state["counters"], pairs_compared=len(both),
                    verdicts_equal=float(np.mean([r["same_person"] == (s > args.threshold) for r, s in both])) if both else None,
                    score_max_diff=float(max(abs(r["confidence"] - s) for r, s in both)) if both else None, device=ctx.name())
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
