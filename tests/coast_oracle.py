"""The rules of fid_track_coast (include/faceid.h) in plain numpy: the executable statement the host twin (csrc/coast_core.h) and the device
kernels of csrc/coast.hip are compared with bit for bit, state included.  Not a test module; tests import it.

Every operation is an np.float32 scalar operation, rounded once (numpy's scalar arithmetic and divide are IEEE, correctly rounded): the
product of a prediction is rounded before its add.  Every float that is stored in the state or emitted for a coasting entry passes
`canon`: a NaN becomes the quiet NaN 0x7FC00000."""
import numpy as np

STARTED, EMBED, COASTED = 1 << 8, 1 << 9, 1 << 10
WORDS = 16               # id, missed, has_vel, ident_idx, bits of ident_score, bits of box[4], bits of vel[4], bits of conf, 0, 0
MISSED_MAX = 1 << 20
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def canon(x):
    x = np.float32(x)
    return QNAN if np.isnan(x) else x


def bits(x):
    return np.array([canon(x)], np.float32).view(np.int32)[0]


class Config:
    def __init__(self, hold=5, predict=True, grow=0.05):
        self.hold, self.predict, self.grow = int(hold), bool(predict), np.float32(grow)


def fresh(S, T):
    e = np.zeros((S, T, WORDS), np.int32)
    e[..., 0] = -1
    return e


def emitted(box, vel, has_vel, missed, cfg):
    """the box an entry emits in a frame in which it coasts (1 <= missed <= hold)"""
    m = np.float32(missed)
    with np.errstate(all="ignore"):
        p = [np.float32(b) for b in box]
        if cfg.predict and has_vel:
            p = [np.float32(np.float32(b) + np.float32(np.float32(v) * m)) for b, v in zip(box, vel)]
        if cfg.grow != 0:
            g = np.float32(cfg.grow * m)
            dx = np.float32(g * np.float32(p[2] - p[0]))
            dy = np.float32(g * np.float32(p[3] - p[1]))
            p = [np.float32(p[0] - dx), np.float32(p[1] - dy), np.float32(p[2] + dx), np.float32(p[3] + dy)]
    return [canon(v) for v in p]


def coast(entries, stream, det, counts, track, ident_idx, ident_score, cfg):
    """entries int32 [S,T,16] is updated in place -> det_out [B,cap2,5], counts_out [B], track_out [B,cap2,2], idx_out, score_out [B,cap2]"""
    S, T = entries.shape[:2]
    det = np.ascontiguousarray(det, np.float32)
    B, cap = det.shape[:2]
    cap2 = cap + T
    f32 = entries.view(np.float32)
    det_out = np.zeros((B, cap2, 5), np.float32)
    counts_out = np.zeros(B, np.int32)
    track_out = np.full((B, cap2, 2), -1, np.int32)
    idx_out = np.full((B, cap2), -1, np.int32)
    score_out = np.zeros((B, cap2), np.float32)
    for b in range(B):
        s = int(stream[b])
        if s < 0:
            continue
        k = min(max(int(counts[b]), 0), cap)
        det_out[b, :k].view(np.int32)[...] = det[b, :k].view(np.int32)
        track_out[b, :k] = track[b, :k]
        if ident_idx is not None:
            idx_out[b, :k] = ident_idx[b, :k]
            score_out[b, :k].view(np.int32)[...] = np.ascontiguousarray(ident_score[b, :k], np.float32).view(np.int32)
        pick = {}
        for f in range(k):
            tid, word = int(track[b, f, 0]), int(track[b, f, 1])
            if word >= 0 and tid >= 0 and (word & 0xFF) < T:
                pick[word & 0xFF] = f                                # the higher f wins
        n = k
        for t in range(T):
            e, ef = entries[s, t], f32[s, t]
            if t in pick:
                f = pick[t]
                tid, word = int(track[b, f, 0]), int(track[b, f, 1])
                if e[0] == tid and not word & STARTED:
                    d = np.float32(int(e[1]) + 1)
                    with np.errstate(all="ignore"):
                        for q in range(4):
                            e[9 + q] = bits(np.float32(np.float32(det[b, f, q] - ef[5 + q]) / d))
                    e[2] = 1
                else:
                    e[0], e[2], e[9:13] = tid, 0, 0
                for q in range(4):
                    e[5 + q] = bits(det[b, f, q])
                e[13] = bits(det[b, f, 4])
                e[1] = 0
                e[3] = ident_idx[b, f] if ident_idx is not None else -1
                e[4] = bits(ident_score[b, f]) if ident_idx is not None else 0
            elif e[0] >= 0:
                e[1] = min(int(e[1]) + 1, MISSED_MAX)
                if 1 <= e[1] <= cfg.hold:
                    box = emitted(ef[5:9], ef[9:13], bool(e[2]), int(e[1]), cfg)
                    det_out[b, n, :4] = box
                    det_out[b, n, 4] = ef[13]
                    track_out[b, n] = (e[0], t | COASTED | (int(e[1]) << 16))
                    idx_out[b, n] = e[3]
                    score_out[b, n] = ef[4]
                    n += 1
        counts_out[b] = n
    return det_out, counts_out, track_out, idx_out, score_out


def coasted(outs, T):
    """per frame the coasted rows of a call's outputs: (row index, track id, slot, missed)"""
    det_out, counts_out, track_out, _, _ = outs
    res = []
    for b in range(len(counts_out)):
        rows = []
        for i in range(int(counts_out[b])):
            w = int(track_out[b, i, 1])
            if w >= 0 and w & COASTED:
                rows.append((i, int(track_out[b, i, 0]), w & 0xFF, w >> 16))
        res.append(rows)
    return res


def thin(seq, seed, p=0.3, blank_every=5):
    """random_walk's batches with detections deleted so that tracks coast: every detection goes with probability p, and every
    `blank_every`-th frame of a batch loses all of them"""
    rng = np.random.default_rng(seed)
    out = []
    for det, counts, stream in seq:
        det, counts = det.copy(), counts.copy()
        for b in range(det.shape[0]):
            k = int(counts[b])
            keep = [f for f in range(k) if rng.random() >= p]
            if blank_every and b % blank_every == blank_every - 1:
                keep = []
            rows = det[b, keep].copy()
            det[b] = 0
            det[b, :len(keep)] = rows
            counts[b] = len(keep)
        out.append((det, counts, stream))
    return out
