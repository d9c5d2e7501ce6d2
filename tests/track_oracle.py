"""The rules of fid_track_step / fid_track_identify (include/faceid.h) in plain numpy: the executable statement the device kernels of
csrc/track.hip are compared with bit for bit, state included.  Not a test module; tests import it.

The overlap uses np.float32 scalars in the order of postproc.hip's nms_select_frame: every operation is rounded once to float32 (numpy's
scalar arithmetic and divide are IEEE, correctly rounded), fmax / fmin ignore a NaN operand like fmaxf / fminf do."""
import numpy as np

STARTED, EMBED = 1 << 8, 1 << 9
SLOT_WORDS = 10          # id, missed, since, ident_idx, bits of ident_score, bits of box x1 y1 x2 y2, 0

_one, _zero = np.float32(1), np.float32(0)


def ovr(a, b):
    """overlap of two boxes (x1, y1, x2, y2), float32 in, float32 out"""
    a = [np.float32(v) for v in a]
    b = [np.float32(v) for v in b]
    with np.errstate(all="ignore"):
        area_a = ((a[2] - a[0]) + _one) * ((a[3] - a[1]) + _one)
        area_b = ((b[2] - b[0]) + _one) * ((b[3] - b[1]) + _one)
        xx1, yy1 = np.fmax(a[0], b[0]), np.fmax(a[1], b[1])
        xx2, yy2 = np.fmin(a[2], b[2]), np.fmin(a[3], b[3])
        w = np.fmax(_zero, (xx2 - xx1) + _one)
        h = np.fmax(_zero, (yy2 - yy1) + _one)
        inter = np.float32(w * h)
        return np.float32(inter / np.float32(np.float32(area_a + area_b) - inter))


class Tracker:
    """S streams x T slots; the arrays are the state of fid_tracker_read"""

    def __init__(self, S, T):
        assert S >= 1 and 1 <= T <= 64
        self.S, self.T = S, T
        self.id = np.full((S, T), -1, np.int32)
        self.box = np.zeros((S, T, 4), np.float32)
        self.missed = np.zeros((S, T), np.int32)
        self.since = np.zeros((S, T), np.int32)
        self.ident_idx = np.zeros((S, T), np.int32)
        self.ident_score = np.zeros((S, T), np.float32)
        self.next_id = np.zeros(S, np.int32)
        self.lost = np.zeros(S, np.int32)

    def reset(self, stream=-1):
        sl = slice(None) if stream < 0 else slice(stream, stream + 1)
        self.id[sl] = -1
        for a in (self.box, self.missed, self.since, self.ident_idx, self.ident_score, self.next_id, self.lost):
            a[sl] = 0

    def state(self):
        """(slots int32 [S,T,10], streams int32 [S,2]) as fid_tracker_read returns them"""
        slots = np.zeros((self.S, self.T, SLOT_WORDS), np.int32)
        slots[..., 0], slots[..., 1], slots[..., 2], slots[..., 3] = self.id, self.missed, self.since, self.ident_idx
        slots[..., 4] = self.ident_score.view(np.int32)
        slots[..., 5:9] = self.box.view(np.int32)
        return slots, np.stack([self.next_id, self.lost], axis=1).astype(np.int32)

    # ---- fid_track_step -------------------------------------------------------------------------
    def step(self, det, counts, stream, iou_thresh, max_age, refresh, retry, row_cap):
        """-> track int32 [B,cap,2], offsets int32 [B+1], src int32 [row_cap]"""
        det = np.asarray(det, np.float32)
        B, cap = det.shape[:2]
        thr = np.float32(iou_thresh)
        track = np.full((B, cap, 2), -1, np.int32)
        flagged = [[] for _ in range(B)]
        fresh = np.zeros((self.S, self.T), bool)                  # started during this call: not `known`
        for s in range(self.S):
            for b in range(B):
                if stream[b] != s:
                    continue
                k = min(max(int(counts[b]), 0), cap)
                matched = np.zeros(self.T, bool)
                for f in range(k):
                    d = det[b, f, :4]
                    best, best_slot = None, -1
                    for t in range(self.T):
                        if self.id[s, t] < 0 or matched[t]:
                            continue
                        o = ovr(self.box[s, t], d)
                        if o > thr and (best is None or o > best):   # strict; the lowest slot wins among equals
                            best, best_slot = o, t
                    if best_slot >= 0:
                        t = best_slot
                        self.box[s, t] = d
                        self.missed[s, t] = 0
                        matched[t] = True
                        self.since[s, t] += 1
                        known = self.ident_idx[s, t] >= 0 and not fresh[s, t]
                        word = t
                        if self.since[s, t] >= (refresh if known else retry):
                            word |= EMBED
                            self.since[s, t] = 0
                        track[b, f] = (self.id[s, t], word)
                    else:
                        free = np.flatnonzero(self.id[s] == -1)
                        if len(free):
                            t = int(free[0])
                            self.id[s, t] = self.next_id[s]
                            self.next_id[s] += 1
                            self.box[s, t] = d
                            self.missed[s, t] = 0
                            self.since[s, t] = 0
                            matched[t] = True
                            fresh[s, t] = True
                            track[b, f] = (self.id[s, t], t | STARTED | EMBED)
                        else:
                            self.lost[s] += 1
                            track[b, f] = (-1, -1)                  # (-1 carries every flag bit)
                    if track[b, f, 1] & EMBED:
                        flagged[b].append(f)
                for t in range(self.T):
                    if self.id[s, t] >= 0 and not matched[t]:
                        self.missed[s, t] += 1
                        if self.missed[s, t] > max_age:
                            self.id[s, t] = -1
                            self.box[s, t] = 0
                            self.missed[s, t] = 0
                            self.since[s, t] = 0
                            fresh[s, t] = False
        offsets = np.zeros(B + 1, np.int32)
        offsets[1:] = np.cumsum([len(v) for v in flagged])
        src = np.full(row_cap, -1, np.int32)
        rows = [b * cap + f for b in range(B) for f in flagged[b]][:row_cap]
        src[:len(rows)] = rows
        self._pending = (np.asarray(stream).copy(), np.asarray(counts).copy(), track.copy(), offsets.copy(), src.copy(), row_cap)
        return track, offsets, src

    # ---- fid_track_identify ---------------------------------------------------------------------
    def identify(self, idx, score, n_rows):
        """-> ident_idx int32 [B,cap], ident_score float32 [B,cap] for the last step's tables"""
        stream, counts, track, offsets, src, row_cap = self._pending
        B, cap = track.shape[:2]
        out_i = np.full((B, cap), -1, np.int32)
        out_s = np.zeros((B, cap), np.float32)
        for s in range(self.S):
            for b in range(B):
                if stream[b] != s:
                    continue
                k = min(max(int(counts[b]), 0), cap)
                row_of = {}
                for i in range(int(offsets[b]), min(int(offsets[b + 1]), n_rows, row_cap)):
                    row_of[int(src[i]) - b * cap] = i
                for f in range(k):                                  # (a slot occurs once per frame: rank order = row order per slot)
                    tid, word = track[b, f]
                    if word < 0:
                        continue
                    t = word & 0xFF
                    if word & STARTED:
                        self.ident_idx[s, t], self.ident_score[s, t] = -1, 0
                    if f in row_of:
                        i = row_of[f]
                        if idx[i] >= 0 and np.float32(score[i]) > self.ident_score[s, t]:
                            self.ident_idx[s, t], self.ident_score[s, t] = idx[i], score[i]
                for f in range(k):
                    word = track[b, f, 1]
                    if word >= 0:
                        out_i[b, f], out_s[b, f] = self.ident_idx[s, word & 0xFF], self.ident_score[s, word & 0xFF]
                    elif f in row_of:
                        out_i[b, f], out_s[b, f] = idx[row_of[f]], score[row_of[f]]
            free = self.id[s] == -1                                  # a slot that is free after the step keeps no identity
            self.ident_idx[s, free] = 0
            self.ident_score[s, free] = 0
        return out_i, out_s


# ---- the sequences of the tests ---------------------------------------------------------------------

def random_walk(seed, calls=3, B=12, cap=8, S=2, n_rect=3):
    """`calls` batches of B frames, the frames dealt to S streams in an irregular interleave.  Per stream a handful of rectangles move on
    integer coordinates; a rectangle drops out for a frame now and then, one leaves for longer than any small max_age and re-enters, clutter
    boxes appear for a single frame, and one rectangle is reported twice in a frame now and then (equal overlaps: ties).
    -> list of (det float32 [B,cap,5], counts int32 [B], stream int32 [B]); deterministic in `seed`."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, 200, (S, n_rect, 2)).astype(np.int64)
    size = rng.integers(20, 60, (S, n_rect, 2)).astype(np.int64)
    vel = rng.integers(-4, 5, (S, n_rect, 2)).astype(np.int64)
    t_stream = np.zeros(S, np.int64)
    away = {(s, n_rect - 1): (4, 9) for s in range(S)}             # frames [4, 9) of the stream: gone
    out = []
    for _ in range(calls):
        det = np.zeros((B, cap, 5), np.float32)
        counts = np.zeros(B, np.int32)
        stream = rng.integers(0, S, B).astype(np.int32)
        for b in range(B):
            s = int(stream[b])
            t = int(t_stream[s])
            t_stream[s] += 1
            pos[s] += vel[s]
            boxes = []
            for r in range(n_rect):
                lo, hi = away.get((s, r), (0, 0))
                if lo <= t < hi or rng.random() < 0.12:
                    continue
                x, y = pos[s, r]
                w, h = size[s, r]
                boxes.append((x, y, x + w, y + h))
                if rng.random() < 0.15:
                    boxes.append(boxes[-1])                         # the same box again: a tie for the later detection
            for _c in range(int(rng.integers(0, 3))):
                x, y = rng.integers(0, 260, 2)
                boxes.append((x, y, x + int(rng.integers(5, 40)), y + int(rng.integers(5, 40))))
            order = rng.permutation(len(boxes))[:cap]
            for f, j in enumerate(order):
                det[b, f, :4] = boxes[j]
                det[b, f, 4] = 1.0 - 0.01 * f
            counts[b] = len(order)
        out.append((det, counts, stream))
    return out


def draw_rows(rng, n, G=5):
    """idx / score as fid_match could write them for n rows: -1 / 0 rows, and scores from a small set so that equal scores occur"""
    idx = rng.integers(-1, G, n).astype(np.int32)
    score = rng.choice(np.array([0.25, 0.5, 0.5, 0.75, 0.9], np.float32), n).astype(np.float32)
    score[idx < 0] = 0
    return idx, score
