"""GPU: measured face quality -- fid_face_measure (csrc/measure.hip) against tests/measure_oracle.py to the bit, fid_face_gates_measured
(csrc/gates.hip) against fid_face_gates and the oracle's formulas, and the opt-in Python surface (FaceAnalysis(measured_quality=True),
PackedFacePipeline / TrackedFacePipeline(measure=True)) against stand-alone measurements."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

import measure_oracle as O
from conftest import load_golden
from oracle import align as oalign
from oracle import gates as ogates

pytestmark = pytest.mark.gpu

CROP = 112 * 112 * 3


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


def measure(ctx, crops, kps=None, src=None, M=None, shift=0):
    """fid_face_measure on host arrays -> (stats, measure) with guard rows behind the outputs; shift: bytes the crop table is moved off its
    dword-aligned allocation (the kernel's byte-load path)"""
    from scrfd_arcface_facerecognition_amd._lib import check
    n = len(crops)
    raw = np.zeros(n * CROP + 8, np.uint8)
    raw[shift:shift + n * CROP] = np.ascontiguousarray(crops, np.uint8).reshape(-1)
    d_crops = ctx.to_device(raw)
    dev = lambda a, dt: None if a is None else ctx.to_device(np.ascontiguousarray(a, dt))
    d_kps, d_src, d_M = dev(kps, np.float32), dev(src, np.int32), dev(M, np.float64)
    stats, meas = ctx.to_device(np.full((n + 1, 8), -7, np.int64)), ctx.to_device(np.full((n + 1, 8), -7.0, np.float32))
    p = lambda b: C.c_void_p(b.ptr) if b is not None else None
    check(ctx.lib.fid_face_measure(ctx.handle, C.c_void_p(d_crops.ptr + shift), n, p(d_kps), p(d_src), p(d_M), p(stats), p(meas)))
    stats, meas = stats.download(), meas.download()
    assert (stats[n] == -7).all() and (meas[n] == -7).all()                # nothing behind the last row is written
    return stats[:n], meas[:n]


def same(got, want, names=None):
    for i in range(len(want[0])):
        assert got[0][i].tolist() == want[0][i].tolist(), (i, names[i] if names else None)
        assert got[1][i].tobytes() == want[1][i].tobytes(), (i, names[i] if names else None, got[1][i], want[1][i])


# ---- 1. fid_face_measure == the oracle -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def table():
    c = O.cases()
    c["want"] = O.measure(c["crops"], kps=c["kps"], src=c["src"], M=c["M"])
    c["want_pixels"] = O.measure(c["crops"], src=c["src"])
    return c


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_every_case_equals_the_oracle(ctx, table, shift):
    c = table
    same(measure(ctx, c["crops"], kps=c["kps"], src=c["src"], M=c["M"], shift=shift), c["want"], c["names"])
    holes = c["src"] < 0
    assert holes.sum() >= 3 and not c["want"][0][holes].any()
    if shift == 0:
        same(measure(ctx, c["crops"], src=c["src"]), c["want_pixels"], c["names"])                        # pixel part only
        names, crops = zip(*O.pixel_cases())                                                               # no table at all
        got = measure(ctx, np.stack(crops))
        same(got, O.measure(np.stack(crops)), names)
        assert got[0][names.index("checkerboard"), 4] == 6400 * 1020 ** 2 and got[1][names.index("checkerboard"), 0] == np.float32(1040400.0)
        ps = O.pose_cases()                                                                                # src == NULL: row i reads landmark row i
        kps, M = np.stack([p[1].reshape(10) for p in ps]), np.stack([p[2] for p in ps])
        got = measure(ctx, np.stack(crops)[:len(ps)], kps=kps, M=M)
        same(got, O.measure(np.stack(crops)[:len(ps)], kps=kps, M=M), [p[0] for p in ps])
        assert got[1][0, 4:].tobytes() == bytes(16) and got[0][0, 7] == 3                                  # template + identity: exactly 0, 0, 0, valid


@pytest.fixture(scope="module")
def random_rows():
    """257 random crops, a [4, 80] landmark table, a src table with holes, plausible matrices; the oracle once"""
    rng = np.random.default_rng(29)
    n = 257
    crops = rng.integers(0, 256, (n, 112, 112, 3), dtype=np.uint8)
    crops[::7] = rng.integers(0, 30, (len(crops[::7]), 112, 112, 3), dtype=np.uint8)
    src = rng.permutation(320)[:n].astype(np.int32)
    src[rng.random(n) < 0.2] = -1
    src[[0, 63, 64, 256]] = [5, -1, 7, 9]
    kps = (O.TEMPLATE.reshape(10)[None] + rng.normal(0, 3.0, (320, 10))).astype(np.float32)
    M = np.tile(O.IDENTITY, (n, 1)) + rng.normal(0, 0.02, (n, 6))
    return dict(crops=crops, src=src, kps=kps, M=M, want=O.measure(crops, kps=kps, src=src, M=M))


@pytest.mark.parametrize("n", [1, 3, 64, 65, 257])
def test_row_counts_and_holes(ctx, random_rows, n):
    r = random_rows
    got = measure(ctx, r["crops"][:n], kps=r["kps"], src=r["src"][:n], M=r["M"][:n])
    same(got, (r["want"][0][:n], r["want"][1][:n]))
    holes = r["src"][:n] < 0
    assert not got[0][holes].any() and got[1][holes].tobytes() == bytes(32 * int(holes.sum()))          # whatever their crop holds
    assert (got[0][~holes, 7] == 3).all()


def test_refusals(ctx):
    lib, h = ctx.lib, ctx.handle
    buf = ctx.empty((CROP + 64,), np.uint8)
    p = C.c_void_p(buf.ptr)
    assert lib.fid_face_measure(h, p, 0, None, None, None, p, p) == 0                                     # nothing to do, nothing enqueued
    assert lib.fid_face_measure(h, p, -1, None, None, None, p, p) == -1
    assert lib.fid_face_measure(h, None, 1, None, None, None, p, p) == -1
    assert lib.fid_face_measure(h, p, 1, None, None, None, None, p) == -1 and lib.fid_face_measure(h, p, 1, None, None, None, p, None) == -1
    assert lib.fid_face_measure(h, p, 1, p, None, None, p, p) == -1 and lib.fid_face_measure(h, p, 1, None, None, p, p, p) == -1
    ctx.sync()


# ---- 2. behind the warp: fid_align_crops_packed with M, then fid_face_measure -------------------------------------------------------------

def box_blur5(frames):
    """5 x 5 box blur on the host, borders replicated, rounded to nearest"""
    f = np.pad(frames.astype(np.int64), ((0, 0), (2, 2), (2, 2), (0, 0)), mode="edge")
    H, W = frames.shape[1:3]
    acc = sum(f[:, dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5))
    return ((2 * acc + 25) // 50).astype(np.uint8)


def synthetic_batch():
    """2 noise frames (texture at all scales), 3 + 2 faces: the template scaled 0.5 .. 2.2, rotated, placed inside the frame"""
    rng = np.random.default_rng(61)
    B, H, W, cap = 2, 320, 320, 4
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    tmpl = O.TEMPLATE.astype(np.float64)
    kps = np.zeros((B, cap, 10), np.float32)
    for b in range(B):
        for f in range(cap):
            s, th = (0.5, 0.9, 1.4, 2.2)[(b + f) % 4], rng.uniform(-0.5, 0.5)
            R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
            t = np.array([rng.uniform(130, W - 130), rng.uniform(130, H - 130)])
            kps[b, f] = ((tmpl - 56) @ R.T * s + t + rng.normal(0, 0.4, (5, 2))).reshape(-1)
    return frames, kps, np.array([3, 2], np.int32), cap


def warp_and_measure(ctx, frames, kps, counts, cap, row_cap=8):
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.app import face_measure
    B, H, W = frames.shape[:3]
    fr, kp, cn = ctx.to_device(frames), ctx.to_device(kps), ctx.to_device(counts)
    off, src = ctx.empty((B + 1,), np.int32), ctx.empty((row_cap,), np.int32)
    check(ctx.lib.fid_face_pack(ctx.handle, C.c_void_p(cn.ptr), B, cap, 0, C.c_void_p(off.ptr), C.c_void_p(src.ptr), row_cap))
    crops, M = ctx.empty((row_cap, 112, 112, 3), np.uint8), ctx.empty((row_cap, 6), np.float64)
    check(ctx.lib.fid_align_crops_packed(ctx.handle, C.c_void_p(fr.ptr), B, H, W, C.c_void_p(kp.ptr), cap, C.c_void_p(src.ptr), row_cap,
                                         C.c_void_p(crops.ptr), C.c_void_p(M.ptr)))
    stats, meas = face_measure(ctx, crops, row_cap, kps=kp, src=src, M=M)
    return crops.download(), M.download(), src.download(), stats.download(), meas.download()


def test_measure_behind_the_warp_and_blur_lowers_sharpness(ctx):
    frames, kps, counts, cap = synthetic_batch()
    crops, M, src, stats, meas = warp_and_measure(ctx, frames, kps, counts, cap)
    # the oracle on the DOWNLOADED crops and M: only the new code is under test
    same((stats, meas), O.measure(crops, kps=kps.reshape(-1, 10), src=src, M=M))
    n = int(counts.sum())
    assert (src[:n] >= 0).all() and (src[n:] < 0).all() and (stats[:n, 7] == 3).all() and not stats[n:].any()
    assert (np.abs(meas[:n, 4:6]) < 0.2).all() and (meas[:n, 6] < 3.0).all()                              # near-frontal by construction
    bcrops, bM, _, bstats, bmeas = warp_and_measure(ctx, box_blur5(frames), kps, counts, cap)
    same((bstats, bmeas), O.measure(bcrops, kps=kps.reshape(-1, 10), src=src, M=bM))
    assert bM.tobytes() == M.tobytes()
    print("\nsharpness, sharp frames:", meas[:n, 0], "\nsharpness, blurred 5x5: ", bmeas[:n, 0])
    assert (bmeas[:n, 0] < meas[:n, 0]).all()


# ---- 3. fid_face_gates_measured -------------------------------------------------------------------------------------------------------

MCFG = dict(sharpness_normalization=120.0, contrast_normalization=45.0, residual_normalization=6.0, yaw_ratio_threshold=0.3,
            pitch_ratio_threshold=0.2)


def gates(ctx, det, kps, counts, F, config=None, measures=None, offsets=None, mcfg=None):
    from scrfd_arcface_facerecognition_amd._lib import MeasureConfig
    from scrfd_arcface_facerecognition_amd.app import face_gates
    B, cap = det.shape[:2]
    dev = None
    if measures is not None:
        dev = (ctx.to_device(np.ascontiguousarray(measures[0], np.int64).reshape(-1, 8)),
               ctx.to_device(np.ascontiguousarray(measures[1], np.float32).reshape(-1, 8)))
    return face_gates(ctx, ctx.to_device(det), ctx.to_device(kps.reshape(B, cap, 10)), ctx.to_device(counts.astype(np.int32)), B, cap, F, config,
                      measures=dev, offsets=ctx.to_device(np.asarray(offsets, np.int32)) if offsets is not None else None,
                      measure_config=MeasureConfig(**(mcfg or MCFG)))


def outputs_equal(a, b):
    return all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(a, b))


def test_invalid_rows_give_fid_face_gates_bit_for_bit(ctx):
    """the 600 golden faces as 40 frames of 15 slots: no row, rows past n_rows, negative rows and rows with clear flags all fall back"""
    from scrfd_arcface_facerecognition_amd._lib import GateConfig, check
    g = load_golden("gates.npz")
    cfg = GateConfig.from_reference_json(json.loads(bytes(g["config"]).decode()))
    B, F = 40, 15
    det = np.concatenate([g["bbox"], g["score"][:, None]], 1).reshape(B, F, 5).astype(np.float32)
    kps = g["kps"].reshape(B, F, 5, 2)
    counts = np.full(B, F)
    base = gates(ctx, det, kps, counts, F, config=cfg)
    assert np.array_equal(base[0].reshape(-1, 5).astype(np.float64), g["quality"])
    rng = np.random.default_rng(2)
    junk = rng.uniform(-5, 500, (B * F, 8)).astype(np.float32)
    clear = np.zeros((B * F, 8), np.int64)
    clear[:, :7] = rng.integers(0, 1 << 40, (B * F, 7))
    clear[:, 7] = rng.choice([0, 4, 8, 1 << 32], B * F)                      # bits 0 and 1 clear, others set: nothing measured
    offs = np.arange(B + 1) * F
    assert outputs_equal(gates(ctx, det, kps, counts, F, config=cfg, measures=(clear, junk)), base)                       # slot form, flags clear
    assert outputs_equal(gates(ctx, det, kps, counts, F, config=cfg, measures=(clear, junk), offsets=offs), base)         # offsets form, flags clear
    valid = clear.copy(); valid[:, 7] = 3
    assert outputs_equal(gates(ctx, det, kps, counts, F, config=cfg, measures=(valid[:1], junk[:1]), offsets=offs + 1), base)     # every row >= n_rows
    assert outputs_equal(gates(ctx, det, kps, counts, F, config=cfg, measures=(valid, junk), offsets=offs - B * F - 20), base)   # every row < 0
    assert not outputs_equal(gates(ctx, det, kps, counts, F, config=cfg, measures=(valid, junk)), base)                   # (valid rows do change it)
    # n_rows = 0 with NULL tables, through the entry point itself
    from scrfd_arcface_facerecognition_amd._lib import MeasureConfig
    q, sd, bt = ctx.empty((B, F, 5), np.float32), ctx.empty((B, F), np.int32), ctx.empty((B, 2), np.int32)
    d_det, d_kps, d_cn = ctx.to_device(det), ctx.to_device(kps.reshape(B, F, 10).astype(np.float32)), ctx.to_device(counts.astype(np.int32))
    check(ctx.lib.fid_face_gates_measured(ctx.handle, C.c_void_p(d_det.ptr), C.c_void_p(d_kps.ptr), C.c_void_p(d_cn.ptr), B, F, F, None, None, None, 0,
                                          C.byref(cfg), C.byref(MeasureConfig(**MCFG)), C.c_void_p(q.ptr), C.c_void_p(sd.ptr), C.c_void_p(bt.ptr)))
    s = sd.download()
    assert outputs_equal((q.download(), s & 0xFFFF, (s >> 16).astype(bool), bt.download()), base)
    assert ctx.lib.fid_face_gates_measured(ctx.handle, C.c_void_p(d_det.ptr), C.c_void_p(d_kps.ptr), C.c_void_p(d_cn.ptr), B, F, F, None, None, None, 5,
                                           C.byref(cfg), C.byref(MeasureConfig(**MCFG)), C.c_void_p(q.ptr), C.c_void_p(sd.ptr), C.c_void_p(bt.ptr)) == -1


def verdict(det_b, n, q_b, flag_b, cfg):
    """the best-face rule and verdict order of fid_face_gates on one frame's (already gated) values"""
    if n == 0:
        return -1, ogates.NO_FACE
    idx = 0
    for f in range(1, n):
        if det_b[f, 4] > det_b[idx, 4]:
            idx = f
    if det_b[idx, 4] < np.float32(cfg["confidence_threshold"]):
        return idx, ogates.LOW_CONFIDENCE
    if flag_b[idx]:
        return idx, ogates.SIDE_FACE
    if q_b[idx, 0] < np.float32(cfg["min_quality_threshold"]):
        return idx, ogates.LOW_QUALITY
    return idx, ogates.ACCEPT


@pytest.mark.parametrize("form", ["offsets", "slots"])
def test_valid_rows_equal_the_oracle_formulas(ctx, form):
    """a ragged batch with more detections than face slots; rows with every flag combination, some faces past n_rows"""
    from scrfd_arcface_facerecognition_amd._lib import GateConfig
    rng = np.random.default_rng(90)
    B, cap, F = 9, 12, 8
    xy = rng.uniform(0, 900, (B, cap, 2)); wh = rng.uniform(40, 500, (B, cap, 2))
    det = np.concatenate([xy, xy + wh, rng.choice([0.3, 0.55, 0.6, 0.75, 0.9], (B, cap, 1))], 2).astype(np.float32)
    kps = (xy[:, :, None, :] + rng.uniform(0, 1, (B, cap, 5, 2)) * wh[:, :, None, :]).astype(np.float32)
    counts = np.array([0, 1, 2, 5, 8, 9, 12, 3, 7])
    kw = dict(confidence_threshold=0.5, decision_threshold=4, min_quality_threshold=0.45)
    cfg = dict(ogates.DEFAULT_CONFIG, **kw)
    base_q, base_score, base_flag, _ = gates(ctx, det, kps, counts, F, config=GateConfig(**kw))
    nb = np.minimum(counts, F)
    if form == "offsets":
        offs = np.concatenate([[0], np.cumsum(nb)])
        row_of = lambda b, f: int(offs[b]) + f
        n_rows = int(offs[B]) - 4                                             # the last four faces have no row
    else:
        offs = None
        row_of = lambda b, f: b * F + f
        n_rows = B * F - 5
    stats = np.zeros((n_rows, 8), np.int64)
    stats[:, 7] = np.arange(n_rows) % 4                                       # every flag combination
    meas = np.zeros((n_rows, 8), np.float32)
    meas[:, 0] = rng.uniform(0, 300, n_rows); meas[:, 2] = rng.uniform(0, 90, n_rows); meas[:, 3] = rng.uniform(0, 0.6, n_rows)
    meas[:, 4] = rng.normal(0, 0.25, n_rows); meas[:, 5] = rng.normal(0, 0.2, n_rows); meas[:, 6] = rng.uniform(0, 9, n_rows)
    q, score, flag, best = gates(ctx, det, kps, counts, F, config=GateConfig(**kw), measures=(stats, meas), offsets=offs)
    assert np.array_equal(score, base_score)
    seen = set()
    for b in range(B):
        wq, wf = np.zeros((F, 5), np.float32), np.zeros(F, bool)
        for f in range(int(nb[b])):
            r = row_of(b, f)
            m, fl = (meas[r], int(stats[r, 7])) if r < n_rows else (None, 0)
            wq[f], wf[f] = O.gated(base_q[b, f], base_flag[b, f], base_score[b, f], det[b, f, 4], m, fl, cfg, MCFG)
            seen.add(fl if m is not None else -1)
            if fl == 0:
                assert wq[f].tobytes() == base_q[b, f].tobytes() and wf[f] == base_flag[b, f]
        assert q[b].tobytes() == wq.tobytes(), b
        assert flag[b].tolist() == wf.tolist(), b
        assert (int(best[b, 0]), int(best[b, 1])) == verdict(det[b], int(nb[b]), wq, wf, cfg), b
    assert seen == {-1, 0, 1, 2, 3}
    assert (flag != base_flag).any() and len(set(best[:, 1].tolist())) >= 2


def one_face(ctx, meas_row, mcfg, gate_kw=None, flags=3):
    """one frontal 0.9 face in one frame, gated with one measure row -> (quality [5], side flag, verdict)"""
    from scrfd_arcface_facerecognition_amd._lib import GateConfig
    det = np.array([[[100, 100, 220, 260, 0.9]]], np.float32)
    kps = np.array([[[[130, 150], [190, 150], [160, 190], [140, 220], [180, 220]]]], np.float32)
    stats = np.zeros((1, 8), np.int64); stats[0, 7] = flags
    q, score, flag, best = gates(ctx, det, kps, np.array([1]), 1, config=GateConfig(**(gate_kw or {})), measures=(stats, np.asarray(meas_row, np.float32)[None]),
                                 mcfg=mcfg)
    return q[0, 0], bool(flag[0, 0]), int(best[0, 1])


@pytest.mark.parametrize("word, key", [(4, "yaw_ratio_threshold"), (5, "pitch_ratio_threshold")])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_ratio_thresholds_are_strict(ctx, word, key, sign):
    v = np.float32(0.2371)
    row = np.zeros(8, np.float32); row[0] = 150; row[2] = 50; row[6] = 1.0; row[word] = sign * v
    loose = dict(MCFG, yaw_ratio_threshold=10.0, pitch_ratio_threshold=10.0)
    assert one_face(ctx, row, dict(loose, **{key: float(v)}))[1:] == (False, ogates.ACCEPT)                      # |ratio| == threshold: not flagged
    below = float(np.nextafter(v, np.float32(0)))
    assert one_face(ctx, row, dict(loose, **{key: below}))[1:] == (True, ogates.SIDE_FACE)                       # the next float below: flagged
    assert one_face(ctx, row, dict(loose, **{key: below}), flags=1)[1:] == (False, ogates.ACCEPT)                # pose part not valid: not looked at


def test_measured_blur_alone_moves_the_verdict(ctx):
    cfg = ogates.DEFAULT_CONFIG
    sharp = np.zeros(8, np.float32); sharp[0] = 400; sharp[2] = 50; sharp[6] = 1.0
    soft = sharp.copy(); soft[0] = 1.5
    q_sharp, _, v0 = one_face(ctx, sharp, MCFG)
    q_soft, _, _ = one_face(ctx, soft, MCFG)
    assert v0 == ogates.ACCEPT and q_sharp[1] == 1.0 and q_soft[1] == np.float32(1.5) / np.float32(120.0)
    assert q_soft[2:].tobytes() == q_sharp[2:].tobytes() and q_soft[0] < q_sharp[0]                             # only blur (and so overall) moved
    mid = float((q_sharp[0] + q_soft[0]) / 2)
    assert one_face(ctx, sharp, MCFG, dict(min_quality_threshold=mid))[2] == ogates.ACCEPT
    assert one_face(ctx, soft, MCFG, dict(min_quality_threshold=mid))[2] == ogates.LOW_QUALITY
    assert cfg["min_quality_threshold"] < mid < 1


# ---- 4. the Python surface, on the synthetic models ------------------------------------------------------------------------------------

def standalone(ctx, image, kpss):
    """every face of one image warped on its own call (fid_align_crops with M) and measured: per face a MEASURE_KEYS dict; the host twin on the
    downloaded crops and matrices must say the same"""
    from scrfd_arcface_facerecognition_amd._lib import check
    from scrfd_arcface_facerecognition_amd.app import face_measure, measured_dicts
    from utils.helpers import measure_crops
    n = len(kpss)
    H, W = image.shape[:2]
    fr, kp, cn = ctx.to_device(image[None]), ctx.to_device(np.asarray(kpss, np.float32).reshape(1, n, 10)), ctx.to_device(np.array([n], np.int32))
    crops, M = ctx.empty((n, 112, 112, 3), np.uint8), ctx.empty((n, 6), np.float64)
    check(ctx.lib.fid_align_crops(ctx.handle, C.c_void_p(fr.ptr), 1, H, W, C.c_void_p(kp.ptr), C.c_void_p(cn.ptr), n, n, C.c_void_p(crops.ptr),
                                  C.c_void_p(M.ptr)))
    stats, meas = face_measure(ctx, crops, n, kps=kp, M=M)
    out = measured_dicts(stats.download(), meas.download())
    host = measure_crops(crops.download(), kps=np.asarray(kpss, np.float32), M=M.download())
    assert [{k: d[k] for k in O.KEYS} for d in host] == out
    return out


def test_face_analysis_measured_quality(monkeypatch):
    monkeypatch.setenv("FID_AUTOTUNE", "0")
    from scrfd_arcface_facerecognition_amd._lib import MEASURE_KEYS, MeasureConfig
    from scrfd_arcface_facerecognition_amd.app import QUALITY_KEYS, FaceAnalysis
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    from scrfd_arcface_facerecognition_amd.session import HipSession
    assert inspect.signature(FaceAnalysis.__init__).parameters["measured_quality"].default is False
    mcfg = MeasureConfig(**MCFG)
    app = FaceAnalysis("synthetic:scrfd_500m?seed=1", "synthetic:arcface_mbf?seed=1", max_faces=4, measured_quality=True, measure_config=mcfg)
    rng = np.random.default_rng(13)
    images = rng.integers(0, 256, (4, 480, 640, 3), dtype=np.uint8)            # (the images of test_face_analysis_get_batch)
    images[1] = 0
    images[3, 200:] = 0
    lb = np.stack([oalign.letterbox(im)[0] for im in images[[0, 2]]])
    P, _ = calibrate_detector_bias(app.ctx, app.det.session.net, app.det.session.params, lb, target=30, max_batch=2)
    app.det.session = HipSession(None, ctx=app.ctx, net=app.det.session.net, params=P, max_batch=8)
    batch = app.get_batch(images, max_num=6)
    single = app.get(images[0], max_num=6)
    print(f"\nfaces per image: {[len(f) for f in batch]}, get(): {len(single)}")
    assert batch[1] == [] and len(single) > 0
    assert max(len(f) for f in batch) > app.max_faces                           # more faces than one run of the crop buffer holds
    for faces, image in ((batch[0], images[0]), (batch[2], images[2]), (batch[3], images[3]), (single, images[0])):
        if not faces:
            continue
        want = standalone(app.ctx, image, [f.kps for f in faces])
        for f, w in zip(faces, want):
            assert list(f.measured) == list(MEASURE_KEYS) and f.measured == w
            # the gates saw the measured scores
            blur = np.float32(w["sharpness"]) / np.float32(MCFG["sharpness_normalization"])
            assert np.float32(f.quality["blur"]) == (blur if blur < 1 else np.float32(1))
    app.measured_quality = False                                                # what the default constructs: no key, the reference's placeholders
    plain = app.get(images[0], max_num=6)
    assert len(plain) == len(single) and all("measured" not in f for f in plain) and all("measured" not in f for fs in app.get_batch(images[:1], 6) for f in fs)
    for f in plain:
        d = np.float32(f.det_score) * np.float32(1.2)
        assert np.float32(f.quality["blur"]) == (d if d < 1 else np.float32(1)) and list(f.quality) == list(QUALITY_KEYS)


H = W = 320
PB = 4


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(ctx):
    """SCRFD-500M at 320x320 and MobileFaceNet with seeded weights on four noise frames"""
    old = os.environ.get("FID_AUTOTUNE")
    os.environ["FID_AUTOTUNE"] = "0"
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery, resolve_model
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    s = Scene()
    rng = np.random.default_rng(43)
    s.frames = rng.integers(0, 256, (PB, H, W, 3), dtype=np.uint8)
    s.frames[2] = 0                                                            # a frame without a face
    det_net, det_P0 = resolve_model("synthetic:scrfd_500m?seed=5", (H, W))
    det_P, _ = calibrate_detector_bias(ctx, det_net, det_P0, s.frames[[0, 1, 3, 0]], target=10, max_batch=4)
    rec_net, rec_P = resolve_model("synthetic:arcface_mbf?seed=5")
    s.det = CompiledNet(ctx, det_net, det_P, max_batch=PB)
    s.rec = CompiledNet(ctx, rec_net, rec_P, max_batch=128)
    s.gallery = Gallery(ctx, np.random.default_rng(77).standard_normal((37, 512)).astype(np.float32))
    s.frames_dev = ctx.to_device(s.frames)
    yield s
    if old is None:
        del os.environ["FID_AUTOTUNE"]
    else:
        os.environ["FID_AUTOTUNE"] = old


def results_equal(a, b):
    assert [len(r) for r in a] == [len(r) for r in b]
    for ra, rb in zip(a, b):
        for (bb, sc, kp, name, sim), (bb2, sc2, kp2, name2, sim2) in zip(ra, rb):
            assert np.array_equal(bb, bb2) and sc == sc2 and np.array_equal(kp, kp2) and name == name2 and sim == sim2


def test_packed_pipeline_measure(ctx, scene):
    from scrfd_arcface_facerecognition_amd._lib import MEASURE_KEYS
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline
    s = scene
    plain = PackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=128)
    plain.run_step(s.frames_dev, H, W, s.gallery, -1.0)                        # (first use of these batch sizes)
    plain.run_step(s.frames_dev, H, W, s.gallery, -1.0)
    want = plain.results(s.gallery)
    assert plain.stats is None and plain.measures is None
    with pytest.raises(RuntimeError):
        plain.results_measured(s.gallery)
    pipe = PackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=128, measure=True)
    pipe.run_step(s.frames_dev, H, W, s.gallery, -1.0)
    assert pipe.stats.shape == (128, 8) and pipe.measures.shape == (128, 8)
    results_equal(pipe.results(s.gallery), want)
    res, measured = pipe.results_measured(s.gallery)
    results_equal(res, want)
    counts = [len(r) for r in res]
    print(f"\nfaces per frame: {counts}")
    assert sum(counts) > 0 and pipe.overflow == 0
    for b in range(PB):
        assert len(measured[b]) == counts[b]
        if counts[b]:
            alone = standalone(ctx, s.frames[b], [face[2] for face in res[b]])
            assert measured[b] == alone and all(list(m) == list(MEASURE_KEYS) for m in measured[b])
    stats = pipe.stats.download()
    assert (stats[:sum(counts), 7] & 1).all() and not stats[sum(counts):].any()          # rows behind the last face: no face, zero words


def test_tracked_pipeline_measure_reports_none_without_a_row(ctx, scene):
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline, TrackedFacePipeline
    s = scene
    probe = PackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=128)
    probe.run_step(s.frames_dev, H, W, s.gallery, -1.0)
    total = sum(len(r) for r in probe.results(s.gallery))
    assert 3 <= total <= 128
    row_cap = total - 2                                                        # the last two due faces find no row in this step
    tracked = TrackedFacePipeline(ctx, s.det, s.rec, batch=PB, row_cap=row_cap, buckets=[row_cap], measure=True, max_tracks=64)
    tracked.run_step(s.frames_dev, H, W, s.gallery, -1.0)
    res, measured = tracked.results_measured(s.gallery)
    assert sum(len(r) for r in res) == total and tracked.overflow == 2
    flat = [(b, f) for b in range(PB) for f in range(len(res[b]))]
    for k, (b, f) in enumerate(flat):
        if k < row_cap:
            assert measured[b][f] == standalone(ctx, s.frames[b], [res[b][f][2]])[0], (b, f)
        else:
            assert measured[b][f] is None, (b, f)
    tracked.close()
