"""The measured face quality (include/faceid.h, fid_face_measure / fid_face_gates_measured) restated in numpy: the integer arrays in int64,
the derived words and the pose part in float64 in the stated operation order, each result rounded once to float32.  Plus `cases()`, the crops
and pose inputs the CPU, sanitizer and GPU tests share.  Test infrastructure only."""
import numpy as np

F = np.float32
N = 6400
LO, HI = 16, 96
KEYS = ("sharpness", "mean", "contrast", "clipped", "yaw", "pitch", "residual")
TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], np.float32)
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])


def luma(crop):
    c = crop.astype(np.int64)
    return (29 * c[..., 0] + 150 * c[..., 1] + 77 * c[..., 2] + 128) >> 8


def pixel_stats(crop):
    """crop uint8 [112,112,3] BGR -> the seven integers N, sum Y, sum Y^2, sum L, sum L^2, n_dark, n_bright (python ints)"""
    Y = luma(crop)
    w = Y[LO:HI, LO:HI]
    L = 4 * w - Y[LO:HI, LO - 1:HI - 1] - Y[LO:HI, LO + 1:HI + 1] - Y[LO - 1:HI - 1, LO:HI] - Y[LO + 1:HI + 1, LO:HI]
    return [N, int(w.sum()), int((w * w).sum()), int(L.sum()), int((L * L).sum()), int((w <= 16).sum()), int((w >= 239).sum())]


def derived(st):
    """the seven integers -> measure[0 .. 3] (float32)"""
    n, sy, syy, sl, sll, nd, nb = st
    nn = np.float64(n * n)
    return [F(np.float64(n * sll - sl * sl) / nn), F(np.float64(sy) / np.float64(n)), F(np.sqrt(np.float64(n * syy - sy * sy) / nn)),
            F(np.float64(nd + nb) / np.float64(n))]


def _ratios(q):
    ex, ey = (q[0, 0] + q[1, 0]) / 2.0, (q[0, 1] + q[1, 1]) / 2.0
    mx, my = (q[3, 0] + q[4, 0]) / 2.0, (q[3, 1] + q[4, 1]) / 2.0
    w, h = q[1, 0] - q[0, 0], my - ey
    return (q[2, 0] - (ex + mx) / 2.0) / w, (q[2, 1] - ey) / h, w, h


def pose(kps, M):
    """kps float32 [5,2] (or [10]), M float64 [6] -> (yaw, pitch, residual) as float32 and the valid flag"""
    zero = (F(0), F(0), F(0), False)
    M = np.asarray(M, np.float64).reshape(6)
    if not np.isfinite(M).all():
        return zero
    k = np.asarray(kps, np.float32).reshape(5, 2).astype(np.float64)
    t = TEMPLATE.astype(np.float64)
    with np.errstate(all="ignore"):
        p = np.empty((5, 2))
        p[:, 0] = (M[0] * k[:, 0] + M[1] * k[:, 1]) + M[2]
        p[:, 1] = (M[3] * k[:, 0] + M[4] * k[:, 1]) + M[5]
        ss = np.float64(0.0)
        for i in range(5):
            dx, dy = p[i, 0] - t[i, 0], p[i, 1] - t[i, 1]
            ss = ss + (dx * dx + dy * dy)
        ryp, rpp, w, h = _ratios(p)
        ryt, rpt, _, _ = _ratios(t)
        if not (w > 0 and h > 0):
            return zero
        out = (F(ryp - ryt), F(rpp - rpt), F(np.sqrt(ss / 5.0)))
    if not all(np.isfinite(v) for v in out):
        return zero
    return out + (True,)


def measure(crops, kps=None, src=None, M=None):
    """fid_face_measure: crops uint8 [n,112,112,3]; kps float32 [*,10] and M float64 [n,6] both or neither; src int32 [n] or None
    -> stats int64 [n,8], measure float32 [n,8]"""
    assert (kps is None) == (M is None)
    n = len(crops)
    stats, meas = np.zeros((n, 8), np.int64), np.zeros((n, 8), np.float32)
    for i in range(n):
        if src is not None and src[i] < 0:
            continue
        st = pixel_stats(crops[i])
        flags = 1
        meas[i, :4] = derived(st)
        if kps is not None:
            face = int(src[i]) if src is not None else i
            yaw, pitch, res, ok = pose(np.asarray(kps, np.float32).reshape(-1, 10)[face], np.asarray(M, np.float64).reshape(-1, 6)[i])
            meas[i, 4:7] = (yaw, pitch, res)
            flags |= 2 if ok else 0
        stats[i] = st + [flags]
    return stats, meas


# ---- fid_face_gates_measured: the measured terms over oracle/gates.py's values ------------------------------------------------------------

def gated(base_q, base_flag, base_score, det_score, meas, flags, cfg, mcfg):
    """One face.  base_q: fid_face_gates' [overall, blur, pose, lighting, size] (float32), base_flag / base_score its side flag and score; meas: the
    face's measure row or None, flags: its stats word 7; cfg: the gate thresholds (dict), mcfg: dict of the five fid_measure_config fields.
    -> (quality [5] float32, side flag)"""
    q = np.asarray(base_q, F)
    blur, ps, light, size = q[1], q[2], q[3], q[4]
    flag = bool(base_flag)
    if meas is not None and flags & 1:
        x = F(meas[0]) / F(mcfg["sharpness_normalization"])
        blur = x if x < F(1) else F(1)
        x = F(meas[2]) / F(mcfg["contrast_normalization"])
        light = (x if x < F(1) else F(1)) * (F(1) - F(meas[3]))
    if meas is not None and flags & 2:
        x = F(1) - F(meas[6]) / F(mcfg["residual_normalization"])
        ps = x if x > F(0) else F(0)
        flag = flag or bool(abs(F(meas[4])) > F(mcfg["yaw_ratio_threshold"])) or bool(abs(F(meas[5])) > F(mcfg["pitch_ratio_threshold"]))
    det = F(det_score)
    o = det * F(cfg["w_detection"]) + size * F(cfg["w_size"])
    o = o + blur * F(cfg["w_blur"])
    o = o + ps * F(cfg["w_pose"])
    o = o + light * F(cfg["w_lighting"])
    return np.array([o, blur, ps, light, size], F), flag


# ---- the shared cases ---------------------------------------------------------------------------------------------------------------------

def _blank(v=0):
    return np.full((112, 112, 3), v, np.uint8)


def _dot(x, y):
    c = _blank()
    c[y, x] = 255
    return c


def pixel_cases():
    """(name, crop uint8 [112,112,3])"""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:112, 0:112]
    out = [("zeros", _blank()), ("ones", _blank(255)),
           ("checkerboard", np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, 2)),
           ("stripes", np.repeat(((xx & 1) * 255).astype(np.uint8)[..., None], 3, 2))]
    for name, ch in (("blue", 0), ("green", 1), ("red", 2)):
        c = _blank()
        c[..., ch] = 255
        out.append((name, c))
    for x, y in ((16, 16), (95, 95), (15, 16), (96, 95), (14, 50), (0, 0)):
        out.append((f"dot_{x}_{y}", _dot(x, y)))
    for i in range(3):
        out.append((f"random_{i}", rng.integers(0, 256, (112, 112, 3), dtype=np.uint8)))
    out.append(("random_dark", rng.integers(0, 40, (112, 112, 3), dtype=np.uint8)))
    out.append(("random_bright", rng.integers(215, 256, (112, 112, 3), dtype=np.uint8)))
    return out


def similarity(scale, theta, tx, ty):
    """M [6] of the map x -> scale * R(theta) x + t"""
    c, s = scale * np.cos(theta), scale * np.sin(theta)
    return np.array([c, -s, tx, s, c, ty], np.float64)


def pose_cases():
    """(name, kps float32 [5,2], M float64 [6])"""
    t = TEMPLATE.copy()
    out = [("template", t, IDENTITY.copy())]
    k = t.copy(); k[2] += (6.5, -3.25)
    out.append(("nose_shifted", k, IDENTITY.copy()))
    # a rotated and scaled copy of the template with the matching M: k = A^-1 (t - b), M = [A | b]
    M = similarity(0.37, 0.4, 11.0, -7.5)
    A, b = M.reshape(2, 3)[:, :2], M.reshape(2, 3)[:, 2]
    out.append(("rotated_scaled", ((t.astype(np.float64) - b) @ np.linalg.inv(A).T).astype(np.float32), M))
    k = t.copy(); k[[0, 1]] = k[[1, 0]]
    out.append(("w_negative", k, IDENTITY.copy()))
    k = t.copy(); k[1, 0] = k[0, 0]
    out.append(("w_zero", k, IDENTITY.copy()))
    k = t.copy(); k[[3, 4], 1] = 40.0
    out.append(("h_negative", k, IDENTITY.copy()))
    k = t.copy(); k[[3, 4], 1] = (k[0, 1] + k[1, 1]) / F(2)
    out.append(("h_zero", k, IDENTITY.copy()))
    M = IDENTITY.copy(); M[4] = np.nan
    out.append(("nan_in_M", t, M))
    M = IDENTITY.copy(); M[2] = np.inf
    out.append(("inf_in_M", t, M))
    out.append(("zero_M", t, np.zeros(6)))
    k = t.copy(); k[2, 0] = np.nan
    out.append(("nan_landmark", k, IDENTITY.copy()))
    rng = np.random.default_rng(8)
    for i in range(4):
        M = similarity(rng.uniform(0.2, 2.0), rng.uniform(-0.6, 0.6), rng.uniform(-30, 30), rng.uniform(-30, 30))
        A, b = M.reshape(2, 3)[:, :2], M.reshape(2, 3)[:, 2]
        k = ((t.astype(np.float64) + rng.normal(0, 2.0, (5, 2)) - b) @ np.linalg.inv(A).T).astype(np.float32)
        out.append((f"random_{i}", k, M))
    return out


def cases():
    """One table holding every case: crops [n,112,112,3], kps float32 [B*cap,10] (a [B,cap] landmark table the rows pick from through src),
    src int32 [n] (holes: rows with src < 0 that hold random bytes), M float64 [n,6], names [n].  Pixel case i is paired with pose case
    i mod len(pose_cases)."""
    px, ps = pixel_cases(), pose_cases()
    rng = np.random.default_rng(17)
    n_face = max(len(px), len(ps)) + 3
    B, cap = 4, -(-n_face // 4) + 2
    slots = rng.permutation(B * cap)[:n_face]                         # the landmark row of every face: scattered over the table
    kps = rng.uniform(0, 112, (B * cap, 10)).astype(np.float32)
    crops, src, M, names = [], [], [], []
    for i in range(n_face):
        pn, crop = px[i % len(px)]
        qn, k, m = ps[i % len(ps)]
        kps[slots[i]] = k.reshape(10)
        crops.append(crop); src.append(int(slots[i])); M.append(m); names.append(f"{pn}+{qn}")
        if i % 5 == 2:                                                # a hole: no face, random bytes and a random M that must not show
            crops.append(rng.integers(0, 256, (112, 112, 3), dtype=np.uint8)); src.append(-1 - (i % 3)); M.append(rng.normal(0, 1, 6))
            names.append("hole")
    return dict(crops=np.stack(crops), kps=kps, src=np.array(src, np.int32), M=np.stack(M).astype(np.float64), names=names)
