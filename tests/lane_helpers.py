"""Shared pieces of tests/test_gpu_two_lanes.py: two library contexts on two HIP streams of one device ("lanes"), built the way bench.py
builds them, each with its OWN frames, weights and gallery; drivers that put one pipeline behind the four calls the in-flight protocol
needs (reset / unit / read, and flush for the grouped one); the protocol itself; and the byte comparison.  Plain module, no fixtures.

The protocol (run_roles).  A lane's work is a fixed list of calls: R rounds as the neighbour (K units enqueued back to back, nothing
read in between), then R rounds as the lane under test (one unit, then every buffer read back).  `solo` runs that list with the other
lane idle at every moment; in flight the same list runs with the neighbour's K units still queued while the lane under test enqueues
its unit and downloads.  A download (fid_memcpy_d2h) synchronises the caller's own stream only.  Every snapshot of the second pass must
equal the first pass's byte for byte: reset() zeroes every buffer a snapshot reads, so both passes start from the same bytes and a row no
kernel writes holds the same stale value in both.

K is sized from a measurement (timings): the device time of the neighbour's K units that is STILL QUEUED when the host has finished
enqueuing them, K x (device ms - host enqueue ms) per unit, must reach MARGIN = 5 times what the lane under test needs for its unit and its
downloads (the larger of its device time and its wall time).  That implies the plain condition K x device ms >= 5 x the tested lane's step
time.  Whether the neighbour really was still running is read off a torch event recorded behind its last unit and queried once the lane
under test has its results on the host."""
import ctypes as C
import math
import time

import numpy as np

H = W = 320
B = 3                      # frames per step
ROUNDS = 4                 # rounds per role
MARGIN = 5.0
K_MAX = 128                # units a neighbour queues at most (keeps a test short where the measurement says the lane is host-bound)
THRESH = 0.02


# ---- comparison: raw bytes, no tolerance ---------------------------------------------------------------------------------------------------

def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(raw(a), raw(b)))


def first_difference(got, want):
    """the first key of two snapshots (dicts of arrays) whose bytes differ, as a message; None when every key is equal"""
    if sorted(got) != sorted(want):
        return f"keys {sorted(got)} != {sorted(want)}"
    for k in want:
        if not same(got[k], want[k]):
            g, w = np.asarray(got[k]), np.asarray(want[k])
            if g.shape != w.shape or g.dtype != w.dtype:
                return f"{k}: {g.dtype}{g.shape} != {w.dtype}{w.shape}"
            bad = np.flatnonzero(raw(g) != raw(w))
            return f"{k}: {bad.size} of {raw(g).size} bytes differ, first at byte {int(bad[0])}"
    return None


def flatten(x):
    """a nested result of the gallery calls (lists / tuples / dicts of ids, scores, names) as (float64 array, structure string): every
    number of such a result is an int or a float32 widened to a Python float, so float64 holds it exactly and equal bytes mean equal results"""
    nums, sig = [], []

    def walk(v):
        if isinstance(v, dict):
            sig.append("{")
            for k in sorted(v):
                sig.append(str(k))
                walk(v[k])
            sig.append("}")
        elif isinstance(v, (list, tuple)):
            sig.append("[")
            for e in v:
                walk(e)
            sig.append("]")
        elif v is None or isinstance(v, (str, bytes)):
            sig.append(repr(v))
        else:
            sig.append("n")
            nums.append(float(v))
    walk(x)
    return np.asarray(nums, np.float64), " ".join(sig)


def same_result(a, b):
    (na, sa), (nb, sb) = flatten(a), flatten(b)
    return sa == sb and same(na, nb)


# ---- lanes -----------------------------------------------------------------------------------------------------------------------------------

class Lane:
    """one HIP stream + one library context on it, as bench.py's Lane; everything else is attached by build_lane"""

    def __init__(self):
        import torch
        from scrfd_arcface_facerecognition_amd._lib import Context
        self.stream = torch.cuda.Stream()
        self.ctx = Context(0, self.stream.cuda_stream)


def build_lane(seed, gallery_rows, rec_batch=32):
    """a lane with SCRFD-500M at 320 x 320 (bias calibrated on its own first batch: the recipe of test_grouped_pipeline_equals_per_step_pipeline),
    IResNet-50, a gallery and three frame batches of its own, the middle one with an all-black frame.  Everything is drawn from `seed`."""
    from scrfd_arcface_facerecognition_amd import archs
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    ln = Lane()
    rng = np.random.default_rng(seed)
    ln.seed = seed
    ln.frames = [rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8) for _ in range(3)]
    ln.frames[1][seed % B] = 0
    ln.det_net = archs.scrfd_500m((H, W))
    ln.det_P, _ = calibrate_detector_bias(ln.ctx, ln.det_net, archs.synth_params(ln.det_net, seed), ln.frames[0], target=30, max_batch=B)
    ln.rec_net = archs.iresnet50()
    ln.rec_P = archs.synth_params(ln.rec_net, seed)
    ln.det = CompiledNet(ln.ctx, ln.det_net, ln.det_P, max_batch=B)
    ln.rec = CompiledNet(ln.ctx, ln.rec_net, ln.rec_P, max_batch=rec_batch)
    ln.gal_host = rng.standard_normal((gallery_rows, 512)).astype(np.float32)
    ln.gallery = Gallery(ln.ctx, ln.gal_host)
    ln.dev = [ln.ctx.to_device(f) for f in ln.frames]
    return ln


def video_frames(seed, n=9, shift=4):
    """n frames of a smooth image that moves `shift` pixels per frame (test_gpu_track.py's scene): detections move with it, so tracks continue
    from frame to frame; where a sequence of them starts over, faces jump, and tracks end and start"""
    from test_gpu_track import smooth_image
    wide = smooth_image(np.random.default_rng(seed), H, W + shift * n)
    return np.stack([wide[:, shift * t:shift * t + W] for t in range(n)])


# ---- drivers: one pipeline behind reset / unit / read ------------------------------------------------------------------------------------------

class Driver:
    """unit() enqueues one unit of work over the lane's next frames and reads nothing back; read() downloads every buffer the pipeline
    writes; reset() puts the driver back to its first frame and zeroes those buffers."""

    def __init__(self, lane, frames_dev, gallery=None):
        self.lane, self.ctx, self.stream = lane, lane.ctx, lane.stream
        self.frames_dev, self.gallery = frames_dev, gallery if gallery is not None else lane.gallery
        self.i = 0

    def buffers(self):
        raise NotImplementedError

    def reset(self):
        self.i = 0
        for buf in self.buffers().values():
            buf.zero()
        self.ctx.sync()

    def step(self):
        self.pipe.run_step(self.frames_dev[self.i % len(self.frames_dev)], H, W, self.gallery, THRESH)
        self.i += 1

    def unit(self):
        self.step()

    def read(self):
        return {k: buf.download() for k, buf in self.buffers().items()}


def _post_buffers(post, tag=""):
    return {f"counts{tag}": post.counts, f"det{tag}": post.det, f"kps{tag}": post.kps}


class GroupedDriver(Driver):
    """bench.py's default lane: GroupedFacePipeline(group=2).  A unit is a whole group (two steps: the second one embeds and matches both)."""

    def __init__(self, lane, faces_per_frame=5):
        from scrfd_arcface_facerecognition_amd.pipeline import GroupedFacePipeline
        super().__init__(lane, lane.dev)
        self.pipe = GroupedFacePipeline(lane.ctx, lane.det, lane.rec, batch=B, faces_per_frame=faces_per_frame, group=2)

    def buffers(self):
        p = self.pipe
        out = {"crops": p.crops, "q": p.q, "idx": p.idx, "score": p.score}
        for j, post in enumerate(p.posts):
            out.update(_post_buffers(post, str(j)))
        return out

    def reset(self):
        assert self.pipe.k == 0
        super().reset()

    def unit(self):
        self.step()
        self.step()

    def flush(self):
        self.pipe.flush(self.gallery, THRESH)


class PackedDriver(Driver):
    """PackedFacePipeline(max_num=0, measure=True) at 32 rows: every step runs the whole row table through the recogniser"""

    def __init__(self, lane, row_cap=32):
        from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline
        super().__init__(lane, lane.dev)
        self.pipe = PackedFacePipeline(lane.ctx, lane.det, lane.rec, batch=B, row_cap=row_cap, max_num=0, measure=True)

    def buffers(self):
        p = self.pipe
        out = {"offsets": p.offsets, "src": p.src, "crops": p.crops, "M": p.M, "stats": p.stats, "measures": p.measures, "q": p.q, "idx": p.idx,
               "score": p.score}
        out.update(_post_buffers(p.post))
        return out


class TrackedDriver(PackedDriver):
    """TrackedFacePipeline over a lane's video (its own detector, calibrated on it).  read() adds the tracker's state and the names and ids
    results_tracked() reports; reset() also forgets every track."""

    def __init__(self, lane, video, det, row_cap=32):
        from scrfd_arcface_facerecognition_amd.pipeline import TrackedFacePipeline
        Driver.__init__(self, lane, [lane.ctx.to_device(video[t:t + B]) for t in range(0, len(video), B)])
        self.pipe = TrackedFacePipeline(lane.ctx, det, lane.rec, batch=B, row_cap=row_cap, max_tracks=32, max_age=1, refresh=3, retry=1, measure=True)

    def buffers(self):
        p = self.pipe
        out = super().buffers()
        out.update(track=p.track, ident_idx=p.ident_idx, ident_score=p.ident_score)
        return out

    def reset(self):
        self.pipe.reset()
        super().reset()

    def read(self):
        out = super().read()
        out["slots"], out["per_stream"] = self.pipe.tracker_state()
        res = self.pipe.results_tracked(self.gallery)
        faces = [f for frame in res for f in frame]
        out["names"] = np.array([f[3] for f in faces], dtype="S16")
        out["ids"] = np.array([f[5] for f in faces], dtype=np.int64)
        out["started"] = np.array([f[6] for f in faces], dtype=np.uint8)
        out["faces_per_frame"] = np.array([len(frame) for frame in res], dtype=np.int64)
        return out


# ---- measurement and the protocol ------------------------------------------------------------------------------------------------------------

def timings(drv, n=3):
    """one unit, alone and synchronised, n times: median device ms between two of the lane's own events (fid_event_record /
    fid_event_elapsed_ms), median host ms to enqueue it, median wall ms until its read() has returned"""
    dev, enq, wall = [], [], []
    for _ in range(n):
        drv.ctx.sync()
        t0 = time.perf_counter()
        drv.ctx.event_record(0)
        drv.unit()
        drv.ctx.event_record(1)
        t1 = time.perf_counter()
        drv.read()
        t2 = time.perf_counter()
        dev.append(drv.ctx.elapsed_ms(0, 1))
        enq.append((t1 - t0) * 1e3)
        wall.append((t2 - t0) * 1e3)
    return dict(dev_ms=float(np.median(dev)), enqueue_ms=float(np.median(enq)), wall_ms=float(np.median(wall)))


def choose_k(neighbour, tested):
    """units the neighbour queues so that MARGIN x the tested lane's time is still queued on the device when the host is done enqueuing"""
    need = MARGIN * max(tested["dev_ms"], tested["wall_ms"])
    still_queued = max(neighbour["dev_ms"] - neighbour["enqueue_ms"], 0.25 * neighbour["dev_ms"])
    return int(min(K_MAX, max(2, math.ceil(need / still_queued))))


def run_roles(a, b, k, in_flight, rounds=ROUNDS):
    """the protocol of the module docstring.  k[x]: units lane x queues as the neighbour.  -> (snapshots per lane in call order,
    rounds per role in which the neighbour's event was not yet complete when the lane under test had its results; None when solo)"""
    import torch
    for d in (a, b):
        d.reset()
    outs, overlap = {a: [], b: []}, []
    for tested, neigh in ((a, b), (b, a)):
        seen = 0
        for _ in range(rounds):
            for _ in range(k[neigh]):
                neigh.unit()
            ev = None
            if in_flight:
                ev = torch.cuda.Event()
                ev.record(neigh.stream)
            else:
                neigh.ctx.sync()
            tested.unit()
            got = tested.read()
            if ev is not None:
                seen += int(not ev.query())
            outs[tested].append(got)
            neigh.ctx.sync()
            outs[neigh].append(neigh.read())
        overlap.append(seen)
    return outs, (overlap if in_flight else None)


def assert_same_snapshots(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        diff = first_difference(g, w)
        assert diff is None, f"{what}, snapshot {i}: in flight differs from the solo run: {diff}"


def assert_overlap(overlap, what, detail=""):
    for role, seen in enumerate(overlap):
        assert seen >= 1, (f"{what}: no overlap happened in role {role}: in none of the rounds was the neighbour's queue still running when the "
                           f"lane under test had its results on the host (this says nothing about the results) {detail}")


def free_later(monkeypatch):
    """DeviceBuffer.free deferred: the returned function frees what has piled up.  hipFree waits for every stream of the device, so a
    helper that frees its temporaries when it returns (VectorGallery's calls) would always find the neighbour's queue drained by the time the
    caller can look at the neighbour's event; the library calls themselves are untouched."""
    from scrfd_arcface_facerecognition_amd._lib import DeviceBuffer
    pile = []

    def later(self):
        if self.owned and self.ptr:
            pile.append((self.ctx, self.ptr))
            self.ptr = 0
    monkeypatch.setattr(DeviceBuffer, "free", later)

    def free_now():
        while pile:
            ctx, ptr = pile.pop()
            if ctx.handle:
                ctx.lib.fid_free(ctx.handle, C.c_void_p(ptr))
    return free_now
