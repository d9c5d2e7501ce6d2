"""The rules of fid_track_relink (include/faceid.h) in plain numpy: the executable statement the device kernel of csrc/relink.hip, the host
twin and the stand-alone driver are compared with bit for bit, state included.  Not a test module; tests import it.

The score is computed in float64 and rounded to float32 once.  On the exact rows of the tests (unit rows with 4 or 16 non-zeros: every
product and every partial sum is a multiple of 1/64) that is the fp32 sum in any order; on random rows `attempts` keeps the float64 scores,
so that a test can show how far every decision was from its threshold."""
import numpy as np

STARTED, RELINKED = 1 << 8, 1 << 11
WORDS = 8


def slot_of(tid, word, T):
    if word < 0 or tid < 0:
        return -1
    s = int(word) & 63
    return s if s < T else -1


class Relinker:
    """S streams x T live entries, a pool of L per stream; the arrays are the state of fid_relinker_read"""

    def __init__(self, S, T, L, dim):
        assert S >= 1 and 1 <= T <= 64 and 1 <= L <= 64 and dim >= 8 and dim % 8 == 0
        self.S, self.T, self.L, self.dim = S, T, L, dim
        self.live = np.zeros((S, T, WORDS), np.int32)
        self.pool = np.zeros((S, L, WORDS), np.int32)
        self.live_q = np.zeros((S, T, dim), np.float16)
        self.pool_q = np.zeros((S, L, dim), np.float16)
        self.frames = np.zeros(S, np.int32)
        self.live[..., 0] = -1
        self.pool[..., 0] = -1
        self.links = []          # (stream, frame number, new track id, person, linked-from id, score)
        self.overwrites = 0      # retirements into a full pool
        self.attempts = []       # per link attempt: (thresh, [float64 scores of the non-free pool entries])

    def reset(self, stream=-1):
        sl = slice(None) if stream < 0 else slice(stream, stream + 1)
        for a in (self.live, self.pool, self.live_q, self.pool_q, self.frames):
            a[sl] = 0
        self.live[sl, :, 0] = -1
        self.pool[sl, :, 0] = -1

    def state(self):
        return [a.copy() for a in (self.live, self.pool, self.frames, self.live_q, self.pool_q)]

    def chains(self):
        """links whose pooled track was itself linked: the person is neither the new nor the pooled track's id"""
        return [l for l in self.links if l[3] != l[4]]

    def _retire(self, s, slot):
        w = self.live[s, slot]
        if w[2]:
            free = np.flatnonzero(self.pool[s, :, 0] == -1)
            if len(free):
                p = int(free[0])
            else:
                p = int(np.argmin(self.pool[s, :, 2]))       # (the first among equals)
                self.overwrites += 1
            self.pool[s, p] = (w[1], w[0], w[4], 0, 0, 0, 0, 0)
            self.pool_q[s, p] = self.live_q[s, slot]
        self.live[s, slot] = (-1, 0, 0, 0, 0, 0, 0, 0)

    def step(self, stream, counts, track, offsets, src, row_cap, n_rows, q, thresh, window, max_age):
        """-> person int32 [B,cap,2]"""
        B, cap = track.shape[:2]
        T, L = self.T, self.L
        thresh = np.float32(thresh)
        q = np.asarray(q, np.float16)
        person = np.full((B, cap, 2), -1, np.int32)
        for b in range(B):
            s = int(stream[b])
            if s < 0:
                continue
            n = int(self.frames[s])
            k = min(max(int(counts[b]), 0), cap)
            live, pool = self.live[s], self.pool[s]
            for p in range(L):
                if pool[p, 0] != -1 and n - int(pool[p, 2]) > window:
                    pool[p] = (-1, 0, 0, 0, 0, 0, 0, 0)
            seen = np.zeros(T, bool)
            for f in range(k):
                t, word = (int(v) for v in track[b, f])
                slot = slot_of(t, word, T)
                if slot < 0:
                    continue
                if live[slot, 0] != t or word & STARTED:
                    if live[slot, 0] != -1:
                        self._retire(s, slot)
                    live[slot] = (t, t, 0, 0, 0, 0, -1, 0)
                live[slot, 5] = 0
                seen[slot] = True
            for i in range(max(int(offsets[b]), 0), min(int(offsets[b + 1]), n_rows, row_cap)):
                face = int(src[i])
                if not b * cap <= face < b * cap + k:
                    continue
                f = face - b * cap
                slot = slot_of(int(track[b, f, 0]), int(track[b, f, 1]), T)
                if slot < 0:
                    continue
                if not live[slot, 2]:
                    used = np.flatnonzero(pool[:, 0] != -1)
                    with np.errstate(all="ignore"):
                        scores = [float(np.dot(q[i].astype(np.float64), self.pool_q[s, p].astype(np.float64))) for p in used]
                    if len(used):
                        self.attempts.append((float(thresh), scores))
                    best, at = float(thresh), -1
                    for p, sc in zip(used, scores):
                        if sc > best:
                            best, at = sc, int(p)
                    if at >= 0:
                        live[slot, 1], live[slot, 6] = pool[at, 0], pool[at, 1]
                        live[slot, 3] = np.array([best], np.float32).view(np.int32)[0]
                        self.links.append((s, n, int(live[slot, 0]), int(pool[at, 0]), int(pool[at, 1]), best))
                        pool[at] = (-1, 0, 0, 0, 0, 0, 0, 0)
                self.live_q[s, slot] = q[i]
                live[slot, 2], live[slot, 4] = 1, n
            for f in range(k):
                t, word = (int(v) for v in track[b, f])
                slot = slot_of(t, word, T)
                if slot >= 0:
                    person[b, f] = (live[slot, 1], word | (RELINKED if live[slot, 1] != live[slot, 0] else 0))
            for slot in range(T):
                if live[slot, 0] == -1 or seen[slot]:
                    continue
                if live[slot, 5] < 0x7FFFFFFF:
                    live[slot, 5] += 1
                if live[slot, 5] > max_age:
                    self._retire(s, slot)
            self.frames[s] = n + 1
        return person
