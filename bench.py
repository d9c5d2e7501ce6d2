#!/usr/bin/env python3
"""Headline benchmark: faces/s end-to-end (det + align + embed + match) on MI355X; embed cosine delta vs the oracle.

Workload at N = 1 (BASELINE.json configs[1]): SCRFD-10G + ArcFace-R50 (fp16 MFMA, fp32 accumulate), batch = 64
synthetic 640x640 frames per GPU, 1k-entry gallery, F = 1 face kept per frame (the reference's --max-num 1,
main.py:55-60).  At N > 1 (configs[2]): the same 64 frames per GPU (weak scaling: 512 frames at N = 8), frames
shard by rank, ONE RCCL all-gather of the per-rank unit embeddings, then every rank matches all gathered embeddings
against the replicated 100k-entry gallery (so every rank holds the whole batch's result list).

  python bench.py --gpus 1 --steps 20 --warmup 3
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

By default TWO batches are in flight per GPU (--streams 2): steps are issued round-robin to two independent
library contexts on separate HIP streams, so the latency-bound kernels of one batch (IResNet at 64 faces has
only 100-400 tiles per layer) overlap the other batch's.  Every step is still one full pass over one batch and all
K steps complete inside a timed region (barrier + synchronize on both sides, MAX over ranks).

A plain run sets up, warms up, times exactly K steps once, writes the last timed step's outputs when --dump-outputs DIR is
given, and prints ONE JSON line on rank 0 (metric, value, unit, higher_is_better, dtype, ms_per_step, config).
--full adds what the headline figure does not need: the K-step region repeated --repeats times (default 5, the MEDIAN
repeat reported; `ms_per_step_repeats` lists them all), the one-lane and rec_group-1 legs, and rank 0's checker legs:
  roofline:     all MFMA conv launches of one step (the dominant kernel family): algorithmic FLOPs (2 x MACs of the true
                channel counts) and algorithmic HBM bytes (every op's input + residual + output + weights as stored)
                over their summed device time (HIP events on the library's stream); BOTH floors are reported per net
                (hbm_floor_ms at 8 TB/s, mfma_floor_ms at the 2.5 PFLOP/s dense fp16 peak) and `bound` names the larger
  cpu_baseline: the oracle (fp32 torch-CPU restatement of the reference path) on this box's host cores for a bounded
                sample of the same frames (N = 1 only)
  embed_cosine_delta_max / match_score_delta_max: device embeddings / gallery scores vs the oracle's on identical
                landmarks (the second half of BASELINE.json's metric)
  faces_per_s_F8, ms_per_step_h2d_included: side legs (F in {1, 8}; H2D reported separately).

--dump-outputs DIR writes what the last timed step handed its caller as DIR/<name>.npy (float32 / float64): that step's
detections (bboxes, det_scores, landmarks, face_counts: the faces max_num keeps per frame), its raw and unit embeddings and its
gallery matches (match_index, -1 = Unknown; match_score).  Frames, weights and gallery are seeded: the same arguments give the
same inputs on every run, so two builds can be compared output for output.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP16_TFLOPS = 2500.0      # MI355X dense fp16/bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0          # HBM3E peak (spec); ~6.3 TB/s is what a streaming copy achieves
PROFILE_DIRS = ("r05", "r04", "r03", "r02", "r01")
# persisted kernel plan (per conv op and batch size: kernel family / tile / split-K), keyed by device name and layer-table hash: with it
# every box runs the same kernels and fp32 summation orders (bit-identical heads / embeddings) and nothing is timed at start-up.
# The tracked file is loaded READ-ONLY (FID_PLAN_RO): picks missing from it are tuned as before but never written back by a bench
# run (tools/make_plan.sh generates plans through FID_PLAN, which also appends).  FID_PLAN= (empty) switches the default plan off.
DEFAULT_PLAN = os.path.join(ROOT, "plans", "mi355x.plan")
_T0 = time.time()


def log(msg):
    """progress on stderr (the JSON line is the only thing on stdout)"""
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench +{time.time() - _T0:6.1f}s] {msg}", file=sys.stderr, flush=True)


def host_cores():
    """CPU threads this process may actually use (the GPU box grants a share of the host, not all of it)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:        # cgroup v2 quota
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except Exception:
        pass
    return max(1, min(n, int(os.environ.get("FID_CPU_THREADS", "16"))))


_shape_cache = {}


def node_macs(net, node):
    from scrfd_arcface_facerecognition_amd.archs import infer_shapes
    key = id(net)
    if key not in _shape_cache:
        _shape_cache[key] = infer_shapes(net)
    shp = _shape_cache[key]
    if node.kind == "conv":
        _, ho, wo = shp[node.name]
        return ho * wo * node.cout * (node.cin // node.groups) * node.k * node.k
    if node.kind == "fc":
        return node.c * node.h * node.w * node.cout
    if node.kind == "dethead":
        _, h, w = shp[node.name]
        return h * w * node.num_anchors * 15 * node.cin * node.k * node.k
    return 0


def op_bytes(cn, oi, n):
    """Algorithmic HBM bytes of one op on n images with layer-by-layer materialisation: its input (+ residual) read once,
    its output written once, its weights read once -- tensors as stored (fp16 NHWC, channels padded to 32; fp32 heads;
    u8 frames for the ops that read the image)."""
    W_SRC, W_DST, W_RES, W_WBYTES = 1, 2, 3, 14          # word indices of an op record (csrc/net.h)
    T_CP, T_H, T_W, T_DTYPE = 1, 2, 3, 4                 # ... of a tensor record
    op, tens = cn.low.ops[oi], cn.low.tensors

    def tb(tid):
        t = tens[tid]
        return int(t[T_H]) * int(t[T_W]) * int(t[T_CP]) * (4 if int(t[T_DTYPE]) == 1 else 2)
    b = tb(int(op[W_DST])) * n + max(0, int(op[W_WBYTES]))
    cp_src = int(tens[int(op[W_SRC])][T_CP]) if int(op[W_SRC]) >= 0 else 0
    if int(op[0]) == 6:                                    # fused residual block (csrc/conv_bb.hip): two Cp x 9 x Cp fp16 filter banks (Cp = 64, or 32 for conv_bb32); its intermediate map is never stored
        b += 2 * cp_src * 9 * cp_src * 2
    elif int(op[0]) == 8:                                  # fused bottleneck (csrc/mbf_block.hip): W_WBYTES is the second pointwise conv's; + the first one's weights and the depthwise table
        gp = int(op[30])
        b += cp_src * gp * 2 + 9 * gp * 4
    elif int(op[0]) == 7:                                  # depthwise + pointwise (csrc/dwpw.hip): + the depthwise table
        b += 9 * cp_src * 4
    elif int(op[0]) == 10:                                 # fused lateral + fpn (csrc/lat_fpn.hip): W_WBYTES is the 3x3 bank's; + the lateral's weights and, when stored, the lateral itself
        b += 64 * cp_src * 2 + (tb(int(op[22]) - 1) * n if int(op[22]) > 0 else 0)
    elif int(op[0]) == 9:                                  # fused stem block (csrc/stem_block.hip): W_WBYTES is the first conv's; + the second conv's 64 x 9 x 64 bank and the compact even-pixel output
        b += 64 * 9 * 64 * 2 + (tb(int(op[24]) - 1) * n if int(op[24]) > 0 else 0)
    b += tb(int(op[W_SRC])) * n if int(op[W_SRC]) >= 0 else cn.in_hw[0] * cn.in_hw[1] * 3 * n
    if int(op[W_RES]) >= 0:
        b += tb(int(op[W_RES])) * n
    if int(op[0]) == 2 and int(op[20]) > 0:               # conv fused with the block's shortcut: a second output tensor (csrc/net.h W_X_DST2)
        b += tb(int(op[20]) - 1) * n
    return b


def mfma_roofline(pipe, frames_dev, batch, F, group=1, crops=None):
    """HIP-event time of every MFMA conv launch of one step vs its algorithmic FLOPs and bytes (group > 1: the recogniser runs once per
    `group` steps on group * batch * F crops -- a step's share of that run is 1 / group of its time, FLOPs, bytes and launches)."""
    from scrfd_arcface_facerecognition_amd.lower import OP_BBLOCK, OP_CONV, OP_DWPW, OP_LATFPN, OP_MBBLOCK, OP_STEM, OP_STEMBLOCK, OP_STEMFUSED
    tot_ms, tot_flop, tot_bytes, launches, per_net = 0.0, 0.0, 0.0, 0, {}
    for name, cn, imgs, n, share in (("scrfd_10g", pipe.det, frames_dev, batch, 1.0), ("arcface_r50", pipe.rec, crops if crops is not None else pipe.crops, group * batch * F, 1.0 / group)):
        best = None
        for _ in range(3):
            ms = cn.run_profiled(imgs, n)
            best = ms if best is None else np.minimum(best, ms)
        t, fl, by, k = 0.0, 0.0, 0.0, 0
        by_name = {nd.name: nd for nd in cn.net.nodes}
        # a block's shortcut conv that its stride-2 conv absorbed at this batch size (a generation-12 pick: csrc/net.h W_X_W2OFF) is not launched:
        # its FLOPs still count (they are computed, as extra K-steps), its tensor traffic does not exist, its (event-pair) time is not a launch's
        picks = {(p["op"], p["batch"]): p["gen"] for p in cn.plans()}
        absorbed = {oi for oi in range(len(cn.low.ops))
                    if int(cn.low.ops[oi, 0]) == OP_CONV and int(cn.low.ops[oi, 23]) == 0 and int(cn.low.ops[oi, 29]) > 0
                    and picks.get((int(cn.low.ops[oi, 29]) - 1, n)) == 12}
        for oi, names in enumerate(cn.low.op_nodes):
            if int(cn.low.ops[oi, 0]) not in (OP_CONV, OP_STEM, OP_STEMFUSED, OP_BBLOCK, OP_DWPW, OP_MBBLOCK, OP_STEMBLOCK, OP_LATFPN):
                continue
            macs = sum(node_macs(cn.net, by_name[nm]) for nm in names)
            fl += 2.0 * macs * n
            if oi in absorbed:
                continue
            t += float(best[oi]); by += op_bytes(cn, oi, n); k += 1
        t, fl, by, k = t * share, fl * share, by * share, k * share
        hbm_floor, mfma_floor = by / (PEAK_HBM_GBS * 1e9) * 1e3, fl / (PEAK_FP16_TFLOPS * 1e12) * 1e3
        per_net[name] = {"ms": round(t, 4), "tflops": round(fl / t / 1e9, 1), "gbs": round(by / t / 1e6, 1), "launches": round(k, 1), "images_per_run": n,
                         "gflop": round(fl / 1e9, 1), "gbytes": round(by / 1e9, 3),
                         "hbm_floor_ms": round(hbm_floor, 4), "mfma_floor_ms": round(mfma_floor, 4),
                         "bound": "hbm" if hbm_floor > mfma_floor else "mfma",
                         "frac_of_floor": round(max(hbm_floor, mfma_floor) / t, 4),
                         "frac_mfma_peak": round(fl / t / 1e9 / PEAK_FP16_TFLOPS, 4), "frac_hbm_peak": round(by / t / 1e6 / PEAK_HBM_GBS, 4),
                         "net_ms_all_ops": round(float(best.sum()) * share, 4)}
        tot_ms += t; tot_flop += fl; tot_bytes += by; launches += k
    traffic, traffic_src = None, None   # HBM bytes per launch from the committed PMC passes of this same command (profiles/)
    for d in PROFILE_DIRS:
        try:
            pmc = json.load(open(os.path.join(ROOT, "profiles", d, "pmc_traffic.json")))
            traffic = round(pmc["hbm_bytes_per_launch_corrected"])
            traffic_src = f"profiles/{d}/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, collected separately)"
            break
        except Exception:
            pass
    hbm_floor, mfma_floor = tot_bytes / (PEAK_HBM_GBS * 1e9) * 1e3, tot_flop / (PEAK_FP16_TFLOPS * 1e12) * 1e3
    tfl, gbs = tot_flop / tot_ms / 1e9, tot_bytes / tot_ms / 1e6
    # the step's conv work taken as a whole: which floor is higher decides the bound the line quotes; both fractions are given
    hbm_bound = hbm_floor > mfma_floor
    return {"bound": "hbm" if hbm_bound else "mfma",
            "achieved": round(gbs if hbm_bound else tfl, 1), "peak": PEAK_HBM_GBS if hbm_bound else PEAK_FP16_TFLOPS,
            "unit": "GB/s" if hbm_bound else "TFLOP/s",
            "frac": round((gbs / PEAK_HBM_GBS) if hbm_bound else (tfl / PEAK_FP16_TFLOPS), 4),
            "traffic": traffic, "traffic_source": traffic_src,
            "achieved_tflops": round(tfl, 1), "frac_mfma_peak": round(tfl / PEAK_FP16_TFLOPS, 4),
            "achieved_gbs_algorithmic": round(gbs, 1), "frac_hbm_peak": round(gbs / PEAK_HBM_GBS, 4),
            "hbm_floor_ms": round(hbm_floor, 4), "mfma_floor_ms": round(mfma_floor, 4), "conv_ms": round(tot_ms, 4),
            "kernel": "MFMA conv kernels of one step (per layer the autotuner's pick among conv_mfma_kernel / conv_mfma_dma_kernel / "
                      "conv3x3_direct / conv3x3_chunked / conv3x3_pc / conv3x3_pc2 / conv3x3_pcr / conv3x3_wr / conv3x3_ks (both also on STRIP tiles) / "
                      "conv3x3_s2 / conv_gw, and the fused launches conv_bb / conv_bb32 / scrfd_stem_rows / ir_stem_block / lat_fpn / mbf_block / stem_conv_mfma)",
            "launches": round(launches, 1), "avg_us_per_launch": round(tot_ms * 1e3 / launches, 2),
            "gflop_per_step": round(tot_flop / 1e9, 1), "algorithmic_gbytes_per_step": round(tot_bytes / 1e9, 3),
            "algorithmic_bytes_per_launch": round(tot_bytes / launches), "per_net": per_net}


def cpu_baseline(frames, det_net, det_P, rec_net, rec_P, gallery, n_frames):
    """The oracle on the host cores, reference structure (frame by frame, face by face, python gallery loop)."""
    import torch
    from oracle import pipeline as opipe
    cores = host_cores()
    torch.set_num_threads(cores)
    log(f"cpu_baseline: warm-up frame on {cores} threads")
    opipe.process_frame(frames[0], det_net, det_P, rec_net, rec_P, gallery, max_num=1)     # warm-up
    t0 = time.perf_counter()
    faces, done = 0, 0
    while done < n_frames:
        faces += len(opipe.process_frame(frames[done % len(frames)], det_net, det_P, rec_net, rec_P, gallery, max_num=1))
        done += 1
        if done % 32 == 0:
            log(f"cpu_baseline: {done} frames, {time.perf_counter() - t0:.1f} s")
        if time.perf_counter() - t0 > 15:          # bounded sample: ~15 s of CPU work
            break
    dt = time.perf_counter() - t0
    return {"value": round(faces / dt, 3), "unit": "faces/s", "cores": cores, "kind": "port",
            "sample": f"{done} frames of the same synthetic stream, frame by frame like the reference: SCRFD-10G + "
                      f"ArcFace-R50 fp32 torch-CPU oracle + python gallery loop (1k), {dt:.1f} s on {cores} threads"}


def cosine_delta(pipe, frames, rec_net, rec_P, gal_host, thresh, n_check):
    """metric's second half: device embeddings / match scores vs the fp32 oracle on the SAME landmarks (the detector's fp16
    heads may rank another candidate first than fp32 heads would; decisions are compared on identical heads in tests/)."""
    import torch
    from oracle import match as omatch, pipeline as opipe
    torch.set_num_threads(host_cores())
    kps = pipe.post.kps.download()
    emb = pipe.embeddings()
    idx, score = pipe.idx.download(), pipe.score.download()
    worst_e, worst_s, agree = 0.0, 0.0, 0
    g_unit = gal_host / np.linalg.norm(gal_host, axis=1, keepdims=True)
    for b in range(n_check):
        ref, _ = opipe.embed(frames[b], kps[b, 0].reshape(5, 2), rec_net, rec_P)
        e = emb[b * pipe.F]
        worst_e = max(worst_e, 1.0 - float(ref @ e / np.linalg.norm(ref) / np.linalg.norm(e)))
        sims = g_unit @ (ref / np.linalg.norm(ref))
        j = int(idx[b * pipe.F])
        oj, _ = omatch.match_batch(ref[None], gal_host, thresh)      # the reference's strict-'>' scan, vectorised
        agree += int(int(oj[0]) == j)
        worst_s = max(worst_s, abs(float(score[b * pipe.F]) - (float(sims[j]) if j >= 0 else 0.0)))
    return {"embed_cosine_delta_max": round(worst_e, 6), "match_score_delta_max": round(worst_s, 6),
            "match_index_agreement": f"{agree}/{n_check}", "cosine_delta_sample": f"{n_check} faces of the timed batch vs the fp32 oracle on identical landmarks"}


def detector_agreement(pipe, frames, det_net, det_P, rec_net, rec_P, n_frames, n_e2e=16):
    """reference models/scrfd.py:140-177 on the fp32 oracle's heads vs the device's fp16 heads of the timed batch (oracle/agreement.py):
    (1) NMS survivors matched by IoU >= 0.9; a flip is marginal when one quantity within 5e-3 of a decision boundary explains it (score vs
    conf_thres, suppressing IoU vs iou_thres, score order of an overlapping pair), a cascade when it follows from such a flip;
    (2) the face the pipeline EMBEDS (max_num = 1: the survivor of largest area, scrfd.py:159-177 + main.py:130-134): same / marginal (two
    rivals' areas within 1e-2, or the pick is itself an explained flip of (1)) / unexplained, and for frames with the same pick the
    END-TO-END embedding delta: device embedding (device landmarks, device crop, fp16 net) vs the oracle's (oracle landmarks from the fp32
    heads, oracle crop, fp32 net); (3) the head margins: max |device - oracle| per stride over the frames."""
    import torch
    from oracle import agreement as oagree, align as oalign, nets as onets, pipeline as opipe, postprocess as pp
    torch.set_num_threads(host_cores())
    fused = [pipe.det.read(name, pipe.B) for name in det_net.outputs]
    emb = pipe.embeddings()
    per_frame, top1, same_frames = [], {"same": 0, "marginal": 0, "unexplained": 0, "empty": 0}, []
    err = {k: [0.0, 0.0, 0.0] for k in ("score", "bbox", "kps")}
    for fi in range(n_frames):
        blob = oalign.blob_from_images([frames[fi]], det_net.in_scale, det_net.in_mean)
        ref_outs = onets.scrfd_session_outputs(det_net, det_P, blob)
        dev_outs = oagree.fused_to_session_outputs(fused, fi)
        for gi, key in enumerate(("score", "bbox", "kps")):
            for li in range(3):
                err[key][li] = max(err[key][li], float(np.abs(np.asarray(ref_outs[3 * gi + li]) - dev_outs[3 * gi + li]).max()))
        a = oagree.survivor_agreement(ref_outs, dev_outs, (640, 640), pipe.conf, pipe.iou, margin=5e-3)
        per_frame.append(a)
        v, ia, ib = oagree.top1_agreement(a)
        top1[v] += 1
        if v == "same":
            same_frames.append((fi, ref_outs))
    a = oagree.summarize(per_frame)
    worst = 0.0
    for fi, ref_outs in same_frames[:n_e2e]:
        _, okps = pp.detect_from_heads(ref_outs, (640, 640), (640, 640), pipe.conf, pipe.iou, 1)
        ref, _ = opipe.embed(frames[fi], okps[0], rec_net, rec_P)
        e = emb[fi * pipe.F]
        worst = max(worst, 1.0 - float(ref @ e / np.linalg.norm(ref) / np.linalg.norm(e)))
    strides = ("s8", "s16", "s32")
    return {"det_survivor_agreement": {"matched": a["matched"], "marginal_flips": a["marginal_flips"], "cascade_flips": a["cascade_flips"],
                                       "unexplained": a["unexplained"], "survivors_oracle": a["survivors_a"], "survivors_device": a["survivors_b"],
                                       "sample": f"all NMS survivors (max_num = 0) of {n_frames} frames of the timed batch, fp32 oracle heads vs device heads, margin 5e-3"},
            "top1_face_agreement": {"same": top1["same"], "marginal": top1["marginal"], "unexplained": top1["unexplained"], "no_face": top1["empty"],
                                    "sample": f"the face max_num = 1 keeps (largest-area survivor) on {n_frames} frames of the timed batch: fp32 oracle heads vs "
                                              "device heads; marginal = the rivals' areas within 1e-2 or the pick is an explained flip of det_survivor_agreement"},
            "embed_cosine_delta_end_to_end_max": round(worst, 6),
            "embed_cosine_delta_end_to_end_sample": f"{min(n_e2e, len(same_frames))} frames with the same pick: device embedding (device landmarks and crop) vs "
                                                    "the oracle's (fp32 heads -> landmarks -> crop -> fp32 net)",
            "head_score_err_max": dict(zip(strides, (round(x, 6) for x in err["score"]))),
            "head_bbox_err_max": dict(zip(strides, (round(x, 5) for x in err["bbox"]))),
            "head_kps_err_max": dict(zip(strides, (round(x, 5) for x in err["kps"]))),
            "head_err_note": f"max |device - fp32 oracle| over {n_frames} frames; score = sigmoid output (test bound 4e-3 at 640 x 640), bbox / kps in stride units (3e-2)"}


def host_array(buf):
    """a device buffer (torch tensor or the library's DeviceBuffer) as a numpy array"""
    return buf.detach().cpu().numpy() if hasattr(buf, "detach") else buf.download()


def dump_outputs(out_dir, arrays, budget=64 << 20):
    """DIR/<name>.npy per array; above `budget` bytes in all, every array keeps a fixed, seeded sample of its rows"""
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > budget and a.ndim and a.shape[0] > 1:
            k = max(1, a.shape[0] * budget // total)
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], k, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: repeated timed regions, the one-lane / rec_group-1 legs, roofline, "
                         "oracle comparisons, side legs and the CPU baseline (a plain run times the K steps once and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (detections, embeddings, matches) as DIR/<name>.npy")
    ap.add_argument("--repeats", type=int, default=None,
                    help="the K-step timed region is repeated this often; the median is reported (default 1, 5 with --full)")
    ap.add_argument("--batch", type=int, default=64, help="frames per GPU per step")
    ap.add_argument("--faces-per-frame", type=int, default=1)
    ap.add_argument("--gallery", type=int, default=0, help="gallery entries (0 = 1000 at N = 1 [cfg 2], 100000 at N > 1 [cfg 3])")
    ap.add_argument("--cpu-frames", type=int, default=512, help="frames of the CPU baseline sample (0 = skip; also skips the side legs)")
    ap.add_argument("--agree-frames", type=int, default=64, help="frames of the timed batch whose NMS survivors are compared with the fp32 oracle's (~0.1 s each)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-one-lane", action="store_true", help="skip the ms_per_step_1lane leg (profiling runs: the kernel statistics then hold the timed steps only)")
    ap.add_argument("--no-side-legs", action="store_true", help="skip the F = 8 and H2D-included side measurements")
    ap.add_argument("--comm", choices=("torch", "native"), default=os.environ.get("FID_COMM", "torch"),
                    help="who issues the all-gather at N > 1: torch.distributed (RCCL as backend nccl) or the C-ABI's fid_comm (RCCL)")
    ap.add_argument("--match-scope", choices=("all", "own", "sharded"), default="all")
    ap.add_argument("--backend", choices=("nccl", "gloo"), default=os.environ.get("FID_BENCH_BACKEND", "nccl"),
                    help="gloo = REHEARSAL of the N > 1 code path with several ranks on ONE GPU (the gather is staged through host "
                         "memory; RCCL refuses two ranks on one device); its numbers mean nothing")
    ap.add_argument("--schedule", choices=("lanes", "stages"), default=os.environ.get("FID_BENCH_SCHEDULE", "lanes"),
                    help="how two batches are kept in flight per GPU: 'lanes' = two whole pipelines on two streams, steps issued round-robin; "
                         "'stages' (experiment, N = 1) = ONE detector on stream A and ONE recogniser + gallery on stream B, step i+1's detect stage "
                         "beside step i's align / embed / match stages (events between the streams, two sets of post-process buffers)")
    ap.add_argument("--rec-group", type=int, default=int(os.environ.get("FID_BENCH_REC_GROUP", "2")),
                    help="steps whose faces share one recogniser run (pipeline.GroupedFacePipeline: every step detects + aligns its own batch, the "
                         "group's last step embeds and matches all group x batch x F crops; N = 1, schedule 'lanes')")
    ap.add_argument("--streams", type=int, default=int(os.environ.get("FID_BENCH_STREAMS", "2")),
                    help="pipelines in flight per GPU: steps are issued round-robin to this many independent "
                         "contexts/HIP streams so that the small kernels of one batch overlap another batch's")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1

    if "FID_PLAN" not in os.environ and "FID_PLAN_RO" not in os.environ and os.path.exists(DEFAULT_PLAN):
        os.environ["FID_PLAN_RO"] = DEFAULT_PLAN
    elif os.environ.get("FID_PLAN") == "":
        del os.environ["FID_PLAN"]
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("launch with torch.distributed.run --nproc-per-node N for --gpus N")
    log("importing torch")
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X; there is no CPU fallback")
    if args.backend == "gloo":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "gloo":
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    red_dev = "cpu" if args.backend == "gloo" else "cuda"

    class StagedDist:
        """rehearsal only: torch.distributed's surface with device buffers staged through host memory (gloo)"""
        get_rank, get_world_size = staticmethod(dist.get_rank), staticmethod(dist.get_world_size)

        @staticmethod
        def all_gather_into_tensor(out, inp):
            torch.cuda.current_stream().synchronize()
            o = torch.empty(out.shape, dtype=out.dtype)
            dist.all_gather_into_tensor(o, inp.cpu())
            out.copy_(o)

    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd._lib import Context, check
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery
    from scrfd_arcface_facerecognition_amd.pipeline import (Communicator, FacePipeline, GroupedFacePipeline, build_targets_from_images,
                                                            calibrate_detector_bias, run_step_distributed, shard_range)
    # experiment hook (docs/HOOKS.md): FID_BENCH_PRIO="p0,p1" = HIP stream priority per lane (torch: -1 high, 0 default)
    prios = [int(x) for x in os.environ.get("FID_BENCH_PRIO", "").split(",") if x.strip()]
    stream = torch.cuda.Stream(priority=prios[0]) if prios else torch.cuda.Stream()
    ctx = Context(local_rank, stream.cuda_stream)
    B, F = args.batch, args.faces_per_frame
    RG = args.rec_group if args.schedule == "lanes" else 1                        # recogniser runs once per RG steps of a lane
    G = args.gallery or (1000 if world == 1 else 100_000)
    thresh = 0.4
    calib = np.random.default_rng(1234).integers(0, 256, (8, 640, 640, 3), dtype=np.uint8)   # same on every rank
    frames = np.random.default_rng(1234 + rank).integers(0, 256, (B, 640, 640, 3), dtype=np.uint8)
    log("building nets (synthetic weights, detector bias calibration)")
    det_net = archs.scrfd_10g((640, 640))
    det_P, _ = calibrate_detector_bias(ctx, det_net, archs.synth_params(det_net, seed=0), calib, target=48)
    rec_net = archs.iresnet50()
    rec_P = archs.synth_params(rec_net, seed=0)
    det = CompiledNet(ctx, det_net, det_P, max_batch=B)
    rec = CompiledNet(ctx, rec_net, rec_P, max_batch=B * F * RG)

    # gallery (same on every rank): the first 8 entries come from the reference's own gallery construction (build_targets,
    # main.py:78-105) run through the device path on the calibration frames; the rest are random 512-d vectors
    gal_host = np.random.default_rng(99).standard_normal((G, 512)).astype(np.float32)
    names = [str(i) for i in range(G)]

    from models import SCRFD, ArcFace                     # the reference's import path (main.py:11)
    from scrfd_arcface_facerecognition_amd.session import HipSession
    bt_det = SCRFD(None, input_size=(640, 640), conf_thres=0.5, max_batch=8,
                   session=HipSession(None, ctx=ctx, net=det_net, params=det_P, max_batch=8))
    bt_rec = ArcFace(session=HipSession(None, ctx=ctx, net=rec_net, params=rec_P, max_batch=8))
    targets = build_targets_from_images(bt_det, bt_rec, list(calib), [f"calib{i}" for i in range(len(calib))])
    for cn_ in list(bt_det.session._compiled.values()) + list(bt_rec.session._compiled.values()):
        cn_.close()                                       # start-up only: free the gallery-construction nets
    for i, (e, nm) in enumerate(targets):
        gal_host[i], names[i] = e, nm
    log(f"gallery: {G} entries, {len(targets)} of them built by build_targets from the calibration frames")

    sharded = args.match_scope == "sharded" and world > 1
    g_lo, g_hi = shard_range(G, world, rank) if sharded else (0, G)
    gallery = Gallery(ctx, gal_host[g_lo:g_hi], names[g_lo:g_hi])
    log("nets + gallery resident")

    class Lane:
        """one independent pipeline: its own HIP stream / library context, nets, buffers"""
        pass

    lanes = []
    for li in range(max(1, args.streams)):
        ln = Lane()
        if li == 0:
            ln.stream, ln.ctx, ln.det, ln.rec, ln.gallery = stream, ctx, det, rec, gallery
        else:
            ln.stream = torch.cuda.Stream(priority=prios[li]) if li < len(prios) else torch.cuda.Stream()
            ln.ctx = Context(local_rank, ln.stream.cuda_stream)
            ln.det = CompiledNet(ln.ctx, det_net, det_P, max_batch=B)
            ln.rec = CompiledNet(ln.ctx, rec_net, rec_P, max_batch=B * F * RG)
            ln.gallery = Gallery(ln.ctx, gal_host[g_lo:g_hi], names[g_lo:g_hi])
        n = B * F
        with torch.cuda.stream(ln.stream):
            ln.q_local = torch.empty((n * RG, 512), dtype=torch.float16, device="cuda")
            if RG > 1:
                ln.pipe = GroupedFacePipeline(ln.ctx, ln.det, ln.rec, batch=B, faces_per_frame=F, group=RG, q_buffer=ln.q_local)
            else:
                ln.pipe = FacePipeline(ln.ctx, ln.det, ln.rec, batch=B, faces_per_frame=F, q_buffer=ln.q_local)
            ln.frames_dev = ln.ctx.to_device(frames)     # resident in HBM before the timed region
            if world > 1:
                ln.q_all = torch.empty((world * n * RG, 512), dtype=torch.float16, device="cuda")
                ln.idx_all = torch.empty((world * n * RG,), dtype=torch.int32, device="cuda")
                ln.score_all = torch.empty((world * n * RG,), dtype=torch.float32, device="cuda")
                ln.keys_local = torch.empty((world * n * RG,), dtype=torch.int64, device="cuda")
                ln.keys_all = torch.empty((world * world * n * RG,), dtype=torch.int64, device="cuda")
                if args.comm == "native":
                    def exchange(ident):
                        box = [ident]
                        dist.broadcast_object_list(box, src=0)
                        return box[0]
                    ln.dist = Communicator(ln.ctx, world, rank, exchange)
                else:
                    ln.dist = StagedDist if args.backend == "gloo" else dist
        lanes.append(ln)
    pipe, frames_dev = lanes[0].pipe, lanes[0].frames_dev
    if RG > 1 and args.full:                              # the checker legs (cosine delta, survivor agreement, roofline events) look at ONE batch: a plain pipeline on lane 0's nets
        with torch.cuda.stream(lanes[0].stream):
            pipe = FacePipeline(ctx, det, rec, batch=B, faces_per_frame=F)

    def finish():
        """groups a region's last steps left open are embedded + matched inside the region"""
        if RG > 1:
            for li in range(len(lanes)):
                step(li, flush=True)

    def step(i, flush=False):
        ln = lanes[i % len(lanes)]
        with torch.cuda.stream(ln.stream):
            if world > 1:
                run_step_distributed(ln.pipe, ln.frames_dev, 640, 640, ln.gallery, thresh, ln.q_local, ln.q_all, ln.dist,
                                     idx_all=ln.idx_all, score_all=ln.score_all, match_scope=args.match_scope,
                                     keys_local=ln.keys_local, keys_all=ln.keys_all, gallery_first_row=g_lo, gallery_total=G, flush=flush)
            elif flush:
                ln.pipe.flush(ln.gallery, thresh)
            else:
                ln.pipe.run_step(ln.frames_dev, 640, 640, ln.gallery, thresh)

    if args.schedule == "stages" and world == 1:
        # stage-pipelined schedule: the detector (net + post-process) lives on lane 0's context / stream, the recogniser and the gallery on a second
        # context / stream; pipes[k] (k = i & 1) own the post-process buffers, crops and result buffers of the steps in flight
        sA, cA = stream, ctx
        sB = torch.cuda.Stream()
        cB = Context(local_rank, sB.cuda_stream)
        recB = CompiledNet(cB, rec_net, rec_P, max_batch=B * F)
        galB = Gallery(cB, gal_host, names)
        with torch.cuda.stream(sB):
            spipes = [FacePipeline(cB, det, recB, batch=B, faces_per_frame=F) for _ in range(2)]
        ev_det = [torch.cuda.Event() for _ in range(2)]
        ev_free = [None, None]

        def step(i):                                      # noqa: F811  (replaces the lane schedule)
            k = i & 1
            p = spipes[k]
            with torch.cuda.stream(sA):
                if ev_free[k] is not None:
                    sA.wait_event(ev_free[k])             # the align stage of step i - 2 has read this pipe's post-process buffers
                p.detect(frames_dev, 640, 640)
                sA.record_event(ev_det[k])
            with torch.cuda.stream(sB):
                sB.wait_event(ev_det[k])
                p.embed(frames_dev, 640, 640)
                ev_free[k] = sB.record_event()
                p.match(galB, thresh)
        lanes = [lanes[0]]                                # (warm-up loop below: one pass per pipe)
        pipe = spipes[0]

    enqueue_s = []

    def timed_region(fn, k):
        """exactly k steps between (barrier + synchronize) pairs; MAX over ranks"""
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(k):
            fn(i)
        finish()
        enqueue_s.append((time.perf_counter() - t0) / k)      # host time to ENQUEUE a step (diagnostic: must stay well below the step time)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device=red_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el

    def last_step_outputs():
        """What the last timed step (index steps - 1 of the last region) handed its caller, on this rank: its detections, raw and unit
        embeddings and gallery matches (at N > 1 the gathered unit embeddings and, match scope 'all' / 'sharded', the matches of that step
        on every rank).  Face slots past a frame's face count are zeroed in the rank's own arrays: a caller never receives them."""
        i = args.steps - 1
        if args.schedule == "stages" and world == 1:
            ln, p, rec, steps = None, spipes[i & 1], recB, 1
        else:
            ln = lanes[i % len(lanes)]
            p, rec = ln.pipe, ln.rec
            steps = p.last_steps if RG > 1 else 1                         # the lane's last group ends with its last step
        j, n = steps - 1, p.n_slots
        post = p.posts[j] if RG > 1 else p.post
        post.check()
        counts = np.minimum(post.counts.download()[:B], F)
        keep = (np.arange(F)[None, :] < counts[:, None]).astype(np.float32)             # [B, F]
        det = post.det.download()[:B, :F] * keep[..., None]
        kps = post.kps.download()[:B, :F] * keep[..., None]
        emb = rec.read(rec.low.outputs[0], steps * n).reshape(steps * n, -1)[j * n:(j + 1) * n] * keep.reshape(n, 1)
        own = slice(j * n, (j + 1) * n)
        if world == 1:
            q, idx, score = host_array(p.q)[own], host_array(p.idx)[own], host_array(p.score)[own]
        else:
            rows = np.concatenate([np.arange(r * steps * n + j * n, r * steps * n + (j + 1) * n) for r in range(world)])
            q = host_array(ln.q_all)[rows]
            if args.match_scope == "own":
                idx, score = host_array(p.idx)[own], host_array(p.score)[own]
            else:
                idx, score = host_array(ln.idx_all)[rows], host_array(ln.score_all)[rows]
        return {"bboxes": det[..., :4], "det_scores": det[..., 4], "landmarks": kps.reshape(B, F, 5, 2),
                "face_counts": counts.astype(np.float32), "embeddings": emb.reshape(B, F, -1).astype(np.float32),
                "unit_embeddings": q.astype(np.float32), "match_index": idx.astype(np.float64), "match_score": score.astype(np.float32)}

    # what the plan file really installed: its picks are keyed by ISA name + CU count + layer-table hash + candidate-set
    # revision, so a file that does not match this box / library installs NOTHING and every op is tuned at start-up instead -- the line says so
    plan_path = os.environ.get("FID_PLAN") or os.environ.get("FID_PLAN_RO")

    def picks_at(cn, n):
        return {p["op"] for p in cn.plans() if p["batch"] == n}
    pre_picks = {"det": picks_at(det, B), "rec": picks_at(rec, B * F * RG)}
    for i in range(2 if args.schedule == "stages" else len(lanes) * RG):         # every lane tunes its kernels alone on the GPU
        step(i)
        torch.cuda.synchronize()
    if RG > 1:
        for li in range(len(lanes)):                                               # a region whose step count is no multiple of the group flushes a PARTIAL group:
            for k in range(1, RG):                                                 # its recogniser batches (k x B x F crops) are tuned here, not inside a timed region
                for _ in range(k):
                    step(li)
                step(li, flush=True)
                torch.cuda.synchronize()
        if world == 1 and args.full:
            pipe.run_step(frames_dev, 640, 640, gallery, thresh)                   # (the checker pipeline's recogniser batch)
            torch.cuda.synchronize()
    post_picks = {"det": picks_at(det, B), "rec": picks_at(rec, B * F * RG)}
    plan_picks_loaded = {k: len(v) for k, v in pre_picks.items()}
    ops_autotuned = {k: len(post_picks[k] - pre_picks[k]) for k in pre_picks}
    for i in range(args.warmup):
        step(i)
    finish()
    torch.cuda.synchronize()
    log("warm-up done")
    enqueue_s.clear()
    repeats = [timed_region(step, args.steps) for _ in range(max(1, args.repeats))]
    elapsed = float(np.median(repeats))
    host_enqueue_ms = float(np.median(enqueue_s)) * 1e3
    log(f"timed regions done: {[round(r / args.steps * 1e3, 3) for r in repeats]} ms/step, median {elapsed / args.steps * 1e3:.3f}")
    if args.dump_outputs and rank == 0:                  # before any other leg reuses the buffers
        dump_outputs(args.dump_outputs, last_step_outputs())
        log(f"outputs of the last timed step written to {args.dump_outputs}")
    # the same steps on ONE lane (VERDICT r3 item 5 / Weak 9): a kernel change that is slower alone but faster in the two-lane step stays visible
    one_lane_ms = None
    if args.full and len(lanes) > 1 and not args.no_one_lane:
        def step_lane0(i):
            step(0)
        one = [timed_region(step_lane0, args.steps) for _ in range(3)]
        one_lane_ms = float(np.median(one)) / args.steps * 1e3
        log(f"one lane: {[round(r / args.steps * 1e3, 3) for r in one]} ms/step")
    # ... and the same lanes with the recogniser run per step (rec_group 1): what the grouping buys stays on the line
    ungrouped_ms = None
    if args.full and RG > 1 and world == 1 and not args.no_one_lane:
        for ln in lanes:
            with torch.cuda.stream(ln.stream):
                ln.pipe1 = FacePipeline(ln.ctx, ln.det, ln.rec, batch=B, faces_per_frame=F)

        def step_ungrouped(i):
            ln = lanes[i % len(lanes)]
            with torch.cuda.stream(ln.stream):
                ln.pipe1.run_step(ln.frames_dev, 640, 640, ln.gallery, thresh)
        for i in range(len(lanes)):
            step_ungrouped(i)
            torch.cuda.synchronize()
        ung = [timed_region(step_ungrouped, args.steps) for _ in range(3)]
        ungrouped_ms = float(np.median(ung)) / args.steps * 1e3
        log(f"rec_group 1: {[round(r / args.steps * 1e3, 3) for r in ung]} ms/step")

    lanes[0].pipe.post.check()
    counts = lanes[0].pipe.post.counts.download()
    faces_step = int(np.minimum(counts, F).sum())
    if world > 1:
        fc = torch.tensor([faces_step], dtype=torch.int64, device=red_dev)
        dist.all_reduce(fc, op=dist.ReduceOp.SUM)
        faces_total_step = int(fc.item())
        # the gathered result list must cover every rank's faces (scope "all"/"sharded": every rank holds the whole batch)
        if args.match_scope != "own":
            assert lanes[0].idx_all.shape[0] == world * B * F * RG
    else:
        faces_total_step = faces_step

    out = None
    if rank == 0:
        value = faces_total_step * args.steps / elapsed
        par = "1 GPU"
        if world > 1:
            par = (f"frames sharded over {world} GPUs (one process each), 1 RCCL all-gather of the unit embeddings issued by "
                   f"{'the C-ABI communicator (fid_allgather)' if args.comm == 'native' else 'torch.distributed (backend nccl = RCCL)'}, "
                   f"match scope '{args.match_scope}'"
                   + (" (gallery row-sharded, second 8-byte-per-query key all-gather)" if sharded else " (gallery replicated, every rank matches all gathered embeddings)"))
        out = {
            "metric": "faces/sec end-to-end (det+align+embed+match)", "value": round(value, 2), "unit": "faces/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f16", "data": "synthetic" if args.backend == "nccl" else "REHEARSAL (gloo, ranks share one GPU): not a measurement",
            "config": {"workload": ("BASELINE configs[1]: " if world == 1 else "BASELINE configs[2] (weak-scaled: 64 frames per GPU): ")
                                   + f"SCRFD-10G + ArcFace-R50, {B} synthetic 640x640 frames per GPU per step, "
                                   f"F={F} face/frame (max_num), {G}-entry gallery, random-init weights (seed 0)",
                       "frames_per_gpu": B, "faces_per_step": faces_total_step, "gallery": G,
                       "kernel_plan": ("autotuned at start-up" if not plan_path else
                                       os.path.relpath(plan_path, ROOT) if min(plan_picks_loaded.values()) > 0 else
                                       f"autotuned at start-up (plan key mismatch: {os.path.relpath(plan_path, ROOT)} holds no picks for this device / library revision)"),
                       "plan_picks_loaded": plan_picks_loaded, "ops_autotuned_at_startup": ops_autotuned,
                       "parallelism": par + (f", {len(lanes)} batches in flight per GPU on separate HIP streams" if len(lanes) > 1 else "")
                                      + (f"; the recogniser of a lane runs once per {RG} of its steps on their {RG * B * F} crops (every step detects + aligns its "
                                         f"own batch; all {args.steps} steps' faces are embedded and matched inside the timed region)" if RG > 1 else ""),
                       "rec_group": RG},
            "repeats": len(repeats), "ms_per_step_repeats": [round(r / args.steps * 1e3, 4) for r in repeats],
            "ms_per_step_min": round(min(repeats) / args.steps * 1e3, 4),
            "host_enqueue_ms_per_step": round(host_enqueue_ms, 4),
        }
        if one_lane_ms is not None:
            out["ms_per_step_1lane"] = round(one_lane_ms, 4)
        if ungrouped_ms is not None:
            out["ms_per_step_rec_group1"] = round(ungrouped_ms, 4)
        if args.full and not args.no_roofline:
            log("roofline: per-op HIP-event timing")
            out["roofline"] = mfma_roofline(pipe, frames_dev, B, F, RG, crops=lanes[0].pipe.crops)
    side = args.full and rank == 0 and world == 1 and args.cpu_frames > 0
    if side:
        # the batch the roofline leg left in the pipeline is `frames`; re-run one step so idx/score/kps belong to it
        pipe.run_step(frames_dev, 640, 640, gallery, thresh)
        ctx.sync()
        log("cosine delta vs the oracle")
        out.update(cosine_delta(pipe, frames, rec_net, rec_P, gal_host, thresh, n_check=min(16, B)))
        log("detector survivor agreement vs the oracle")
        out.update(detector_agreement(pipe, frames, det_net, det_P, rec_net, rec_P, n_frames=min(args.agree_frames, B)))
    if side and not args.no_side_legs:
        torch.cuda.synchronize()
        # ---- side leg 1: H2D included.  Per lane two device frame buffers and one pinned host batch; the upload of the next
        # batch runs on the lane's copy stream beside the current step (fid_upload_async_slot), no host synchronisation.
        log("side leg: H2D-included steps")
        from scrfd_arcface_facerecognition_amd.video import _Pinned
        for ln in lanes:
            ln.pinned = _Pinned(ln.ctx, frames.shape, np.uint8)
            ln.pinned.array[:] = frames
            ln.dev2 = [ln.frames_dev, ln.ctx.to_device(frames)]
            ln.k = 0

        def step_h2d(i):
            ln = lanes[i % len(lanes)]
            k = ln.k
            ln.k ^= 1
            with torch.cuda.stream(ln.stream):
                check(ln.ctx.lib.fid_upload_async_slot(ln.ctx.handle, k, C.c_void_p(ln.dev2[k].ptr), C.c_void_p(ln.pinned.ptr), ln.pinned.nbytes))
                check(ln.ctx.lib.fid_upload_wait_slot(ln.ctx.handle, k))
                ln.pipe.run_step(ln.dev2[k], 640, 640, ln.gallery, thresh)
                check(ln.ctx.lib.fid_upload_release(ln.ctx.handle, k))
        for i in range(4):
            step_h2d(i)
        h2d = [timed_region(step_h2d, args.steps) for _ in range(3)]
        out["ms_per_step_h2d_included"] = round(float(np.median(h2d)) / args.steps * 1e3, 4)
        out["faces_per_s_h2d_included"] = round(faces_total_step * args.steps / float(np.median(h2d)), 2)
        out["h2d_note"] = (f"{frames.nbytes / 1e6:.1f} MB of frames per step uploaded from pinned host memory on a separate HIP stream, "
                           "double-buffered per lane (fid_upload_async_slot); never part of `value`")
        # ---- side leg 2: F = 8 faces per frame (SURVEY.md 8d reports F in {1, 8}); one lane pair, recogniser at 512 faces
        log("side leg: F = 8")
        F8 = 8
        for ln in lanes:
            ln.rec8 = CompiledNet(ln.ctx, rec_net, rec_P, max_batch=B * F8)
            with torch.cuda.stream(ln.stream):
                ln.pipe8 = FacePipeline(ln.ctx, ln.det, ln.rec8, batch=B, faces_per_frame=F8)

        def step8(i):
            ln = lanes[i % len(lanes)]
            with torch.cuda.stream(ln.stream):
                ln.pipe8.run_step(ln.frames_dev, 640, 640, ln.gallery, thresh)
        for i in range(len(lanes)):
            step8(i)
            torch.cuda.synchronize()
        step8(0); step8(1)
        f8 = [timed_region(step8, 10) for _ in range(3)]
        lanes[0].pipe8.post.check()
        faces8 = int(np.minimum(lanes[0].pipe8.post.counts.download(), F8).sum())
        out["faces_per_s_F8"] = round(faces8 * 10 / float(np.median(f8)), 2)
        out["ms_per_step_F8"] = round(float(np.median(f8)) / 10 * 1e3, 4)
        out["faces_per_step_F8"] = faces8
    if side:
        out["cpu_baseline"] = cpu_baseline(frames, det_net, det_P, rec_net, rec_P, gal_host, args.cpu_frames)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
