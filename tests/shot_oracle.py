"""The rules of fid_shot_score and fid_track_keep / fid_shots_flush (include/faceid.h) in plain numpy / Python: the executable statement the
device kernels of csrc/shots.hip are compared with bit for bit, state and payload included.  Not a test module; tests import it.

The score uses np.float32 scalars, one rounding per operation (numpy's scalar arithmetic and divide are IEEE, correctly rounded); min / max
are Python's `x if x < 1 else 1` / `x if x > 0 else 0`, so a NaN takes the second branch as it does on the device.  The keeper copies a
shot's payload the moment it decides (sequential semantics): the device, which decides first and copies afterwards, must end in the same
bytes."""
import numpy as np

from track_oracle import STARTED, Tracker, draw_rows, random_walk  # noqa: F401  (the tests make their track tables with these)

META_WORDS = 16          # stream, track id, ident_idx, bits of ident_score, bits of shot score, frame, rows, bits of box[4], bits of det score, 0 x 4
CROP = (112, 112, 3)
_one, _zero = np.float32(1), np.float32(0)


# ---- fid_shot_score -----------------------------------------------------------------------------------------

def shot_score(stats, measure, n_s=100.0, n_c=40.0, n_r=8.0):
    """stats int64 [n,8], measure float32 [n,8] -> float32 [n]"""
    stats, measure = np.asarray(stats, np.int64).reshape(-1, 8), np.asarray(measure, np.float32).reshape(-1, 8)
    n_s, n_c, n_r = np.float32(n_s), np.float32(n_c), np.float32(n_r)
    out = np.empty(len(stats), np.float32)
    with np.errstate(all="ignore"):
        for i, (st, m) in enumerate(zip(stats, measure)):
            flags = int(st[7])
            if not flags & 1:
                out[i] = -1.0
                continue
            x = np.float32(m[0] / n_s)
            b = x if x < _one else _one
            x = np.float32(m[2] / n_c)
            l = np.float32((x if x < _one else _one) * np.float32(_one - m[3]))
            p = _zero
            if flags & 2:
                x = np.float32(_one - np.float32(m[6] / n_r))
                p = x if x > _zero else _zero
            out[i] = np.float32(np.float32(b * l) * p)
    out.view(np.uint32)[np.isnan(out)] = 0x7FC00000                # a NaN leaves as the one quiet NaN: its sign and payload are nobody's rule
    return out


def measure_rows(seed, n=64, norms=(100.0, 40.0, 8.0)):
    """random fid_face_measure rows (stats word 7 and the measure words the score reads are what matters), then the pinned ones: each flag bit
    clear, both clear, and values at every min / max seam (sharpness == n_s, contrast == n_c, residual == n_r, clipped == 1) with their
    neighbours, a NaN and an infinity.  norms: the normalisations the seams are placed at (default: the binding's)."""
    rng = np.random.default_rng(seed)
    stats = np.zeros((n, 8), np.int64)
    measure = np.zeros((n, 8), np.float32)
    stats[:, 0] = 6400
    stats[:, 7] = rng.choice([3, 3, 3, 1, 0, 2], n)
    measure[:, 0] = rng.uniform(0, 250, n)
    measure[:, 1] = rng.uniform(0, 255, n)
    measure[:, 2] = rng.uniform(0, 90, n)
    measure[:, 3] = rng.uniform(0, 1, n)
    measure[:, 4:6] = rng.uniform(-0.5, 0.5, (n, 2))
    measure[:, 6] = rng.uniform(0, 12, n)
    f32 = np.float32
    up, down = (lambda v: np.nextafter(f32(v), f32(np.inf))), (lambda v: np.nextafter(f32(v), f32(-np.inf)))
    base = [50.0, 128.0, 20.0, 0.25, 0.0, 0.0, 2.0, 0.0]
    pinned = []
    for flags in (3, 1, 2, 0):
        pinned.append((flags, list(base)))
    for word, seam in ((0, norms[0]), (2, norms[1]), (6, norms[2]), (3, 1.0)):
        for v in (down(seam), f32(seam), up(seam)):
            row = list(base)
            row[word] = v
            pinned.append((3, row))
    for word, v in ((0, np.nan), (2, np.inf), (6, np.nan), (3, np.nan), (0, 0.0), (6, 0.0), (3, 0.0)):
        row = list(base)
        row[word] = v
        pinned.append((3, row))
    ps = np.zeros((len(pinned), 8), np.int64)
    ps[:, 0] = 6400
    ps[:, 7] = [p[0] for p in pinned]
    pm = np.array([p[1] for p in pinned], np.float32)
    return np.concatenate([stats, ps]), np.concatenate([measure, pm])


# ---- fid_track_keep / fid_shots_flush ---------------------------------------------------------------------------

def _bits(v):
    return int(np.float32(v).view(np.int32))


class Keeper:
    """S x T live entries and finished_cap finished records; the arrays are what fid_shots_read / fid_shots_finished return.  `has_shot`
    says which live payloads mean something (the device's other payload bytes are whatever they were)."""

    def __init__(self, S, T, dim, finished_cap, keep_crops=True):
        self.S, self.T, self.dim, self.cap, self.keep_crops = S, T, dim, finished_cap, bool(keep_crops)
        self.live_meta = np.zeros((S, T, META_WORDS), np.int32)
        self.live_meta[..., 1] = -1
        self.live_q = np.zeros((S, T, dim), np.uint16)
        self.live_crop = np.zeros((S, T) + CROP, np.uint8)
        self.fin_meta = np.zeros((finished_cap, META_WORDS), np.int32)
        self.fin_q = np.zeros((finished_cap, dim), np.uint16)
        self.fin_crop = np.zeros((finished_cap,) + CROP, np.uint8)
        self.count, self.dropped = 0, 0
        self.frames = np.zeros(S, np.int64)
        self.log = []                                              # every record that finished, dropped ones included: (meta, q, crop)

    def has_shot(self):
        return (self.live_meta[..., 1] != -1) & (self.live_meta[..., 4].view(np.float32) >= 0)

    def _finish(self, s, t):
        m = self.live_meta[s, t]
        if m[4:5].view(np.float32)[0] >= 0:                        # (rule 6: without a candidate there is no record)
            self.log.append((m.copy(), self.live_q[s, t].copy(), self.live_crop[s, t].copy()))
            if self.count < self.cap:
                self.fin_meta[self.count], self.fin_q[self.count] = m, self.live_q[s, t]
                self.fin_crop[self.count] = self.live_crop[s, t]
                self.count += 1
            else:
                self.dropped += 1
        m[:] = 0
        m[1] = -1

    def keep(self, tracker_ids, stream, cap, track, offsets, src, row_cap, n_rows, score, q, crops, det, ident_idx=None, ident_score=None):
        """tracker_ids int32 [S,T]: the id every tracker slot holds after the step (Tracker.id); the rest as fid_track_keep takes it"""
        stream = np.asarray(stream)
        B = len(stream)
        track = np.asarray(track).reshape(B, cap, 2)
        det = np.asarray(det, np.float32).reshape(B, cap, 5)
        score = np.asarray(score, np.float32)
        n = min(int(offsets[B]), int(n_rows), int(row_cap))
        for s in range(self.S):
            frame_no, c = {}, int(self.frames[s])
            for b in range(B):
                if stream[b] == s:
                    frame_no[b] = c
                    c += 1
            self.frames[s] = c
            for i in range(n):
                b, f = divmod(int(src[i]), cap)
                if stream[b] != s:
                    continue
                tid, word = int(track[b, f, 0]), int(track[b, f, 1])
                if word < 0:
                    continue
                t = word & 0xFF
                m = self.live_meta[s, t]
                if m[1] != -1 and (m[1] != tid or word & STARTED):     # (STARTED under the same id: the tracker was reset)
                    self._finish(s, t)
                if m[1] == -1:
                    m[:] = 0
                    m[0], m[1], m[2], m[4] = s, tid, -1, _bits(-1.0)
                m[6] += 1
                if ident_idx is not None:
                    m[2], m[3] = int(np.asarray(ident_idx).reshape(B, cap)[b, f]), _bits(np.asarray(ident_score, np.float32).reshape(B, cap)[b, f])
                stored = m[4:5].view(np.float32)[0]
                if score[i] >= 0 and (not stored >= 0 or score[i] > stored):
                    m[4], m[5] = _bits(score[i]), frame_no[b]
                    m[7:11] = det[b, f, :4].view(np.int32)
                    m[11] = _bits(det[b, f, 4])
                    self.live_q[s, t] = np.asarray(q).reshape(-1, self.dim)[i]
                    if self.keep_crops:
                        self.live_crop[s, t] = np.asarray(crops).reshape((-1,) + CROP)[i]
            for t in range(self.T):
                if self.live_meta[s, t, 1] != -1 and self.live_meta[s, t, 1] != tracker_ids[s, t]:
                    self._finish(s, t)

    def flush(self, stream=-1):
        for s in (range(self.S) if stream < 0 else [stream]):
            for t in range(self.T):
                if self.live_meta[s, t, 1] != -1:
                    self._finish(s, t)

    def clear_finished(self):
        self.count, self.dropped = 0, 0


# ---- what the tests feed the keeper ---------------------------------------------------------------------------------

def row_payload(rng, n, dim, call=0):
    """q uint16 [n,dim] (any bits: the keeper only moves them) and crops uint8 [n,112,112,3] whose every byte depends on (call, row, position),
    so a record that holds another row's crop, or a crop shifted by a few bytes, shows"""
    q = rng.integers(0, 1 << 16, (n, dim)).astype(np.uint16)
    pos = np.arange(int(np.prod(CROP)), dtype=np.int64)
    crops = np.stack([((pos * 7 + 31 * (i + 1) + 101 * call + (pos >> 8) * (i + 3)) & 255).astype(np.uint8).reshape(CROP) for i in range(n)])
    return q, crops


def draw_scores(rng, n):
    """scores from a small set, so that ties occur, with a negative, a NaN and a zero now and then"""
    return rng.choice(np.array([0.0, 0.125, 0.25, 0.25, 0.5, 0.5, 0.75, -1.0, -0.25, np.nan], np.float32), n).astype(np.float32)
