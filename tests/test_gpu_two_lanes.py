"""GPU: two library contexts in flight on one device, each with its own data: every lane's results equal its solo run, byte for byte.

bench.py's headline mode keeps two independent contexts busy on two HIP streams (--streams 2), and its `stages` schedule splits one step over
two contexts; both give every lane the same frames, nets and gallery, so state that leaked from one lane into the other would still look
right there.  Here the lanes carry DIFFERENT frames, weights and galleries (asserted first in every case), every case runs its lanes alone
and synchronised first and then in flight ON THE SAME OBJECTS (the same cached kernel picks), and every buffer a pipeline writes is compared
with the solo run through np.array_equal on its raw bytes.  tests/lane_helpers.py has the lanes, the drivers and the protocol (run_roles):
the neighbour queues K units without reading anything back, only then the lane under test enqueues its unit and downloads; K comes from a
measurement taken on the spot, and a torch event behind the neighbour's last unit says whether it really was still running.

Every assertion in this module is bit equality or one of: the two lanes differ, the probed op ran, overlap happened.  No tolerance, no sleep.
Out of scope: two devices in one process, FID_GRAPH, RCCL."""
import re
import threading

import numpy as np
import pytest

import exact_probe as ep
import lane_helpers as lh
from lane_helpers import B, H, W, THRESH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lanes():
    """lane A (seed 11, 29 gallery rows) and lane B (seed 23, 700 rows); the nets run the heuristic kernel plans (FID_AUTOTUNE=0 is read when a
    net is created), as in test_one_context_from_two_threads"""
    mp = pytest.MonkeyPatch()
    mp.setenv("FID_AUTOTUNE", "0")
    try:
        a, b = lh.build_lane(11, 29), lh.build_lane(23, 700)
    finally:
        mp.undo()
    return a, b


@pytest.fixture(scope="module")
def grouped(lanes):
    return lh.GroupedDriver(lanes[0]), lh.GroupedDriver(lanes[1])


def _assert_lanes_differ(sa, sb, what):
    """Rule 1 on two snapshots of the lanes' solo runs: other detections and other unit embeddings (a lane without a face has an all-zero q)"""
    det = [k for k in sa if k.startswith("det")][0]
    assert not lh.same(sa[det], sb[det]) and not lh.same(sa["q"], sb["q"]), f"{what}: the two lanes' solo results do not differ"
    assert np.any(lh.raw(sa["q"])) and np.any(lh.raw(sb["q"])), f"{what}: a lane embedded no face at all"


def _sizes(a, b, what):
    """solo timings of both drivers and the K each one queues as the neighbour (printed: docs/FINDINGS.md quotes them)"""
    ta, tb = lh.timings(a), lh.timings(b)
    k = {a: lh.choose_k(ta, tb), b: lh.choose_k(tb, ta)}
    for name, t, d in (("A", ta, a), ("B", tb, b)):
        print(f"\n[two lanes] {what}: lane {name} unit {t['dev_ms']:.3f} ms device, {t['enqueue_ms']:.3f} ms to enqueue, {t['wall_ms']:.3f} ms with "
              f"its downloads; queues K = {k[d]} units as the neighbour ({k[d] * t['dev_ms']:.1f} ms of device work)")
    return k


def _roles_case(a, b, what):
    """Rules 1 to 3 for two drivers: sizes, the solo pass, the in-flight pass on the same objects, equality, overlap"""
    k = _sizes(a, b, what)
    solo, _ = lh.run_roles(a, b, k, in_flight=False)
    _assert_lanes_differ(solo[a][-1], solo[b][-1], what)
    both, overlap = lh.run_roles(a, b, k, in_flight=True)
    print(f"[two lanes] {what}: overlap in {overlap[0]} of {lh.ROUNDS} rounds with lane A under test, {overlap[1]} of {lh.ROUNDS} with lane B under test")
    for name, d in (("A", a), ("B", b)):
        lh.assert_same_snapshots(both[d], solo[d], f"{what}, lane {name}")
    lh.assert_overlap(overlap, what, f"(K = {[k[a], k[b]]})")
    return solo


# ---- case 1: exact probes beside a neighbour that never stops ---------------------------------------------------------------------------------

def _kinds(low):
    from scrfd_arcface_facerecognition_amd.lower import W_TYPE
    return [int(r[W_TYPE]) for r in low.ops]


class Side:
    """one probe net of a pair: how it is built (autotuned, or FID_AUTOTUNE=0 for the heuristic plan), the hooks it needs, and the check that
    the op it is about is in the net / ran"""

    def __init__(self, key, untuned=False, env=None, in_low=None, after=None, dethead=False, tunes=False):
        self.key, self.untuned, self.env, self.in_low, self.after, self.dethead = key, untuned, env or {}, in_low, after, dethead
        self.tunes = tunes                                       # as lane A: its first run must leave autotuner picks (CompiledNet.plans())
        self.probe = ep.PROBES[key]()

    def build(self, lane, monkeypatch):
        from scrfd_arcface_facerecognition_amd.engine import CompiledNet
        from family_helpers import own_data_tensors
        if self.untuned:
            monkeypatch.setenv("FID_AUTOTUNE", "0")
        else:
            monkeypatch.delenv("FID_AUTOTUNE", raising=False)
        p = self.probe
        cn = CompiledNet(lane.ctx, p.net, p.P, max_batch=p.batch)
        monkeypatch.delenv("FID_AUTOTUNE", raising=False)
        own = own_data_tensors(cn.low)
        if self.dethead:
            self.names = [p.net.outputs[0], "h"]
        elif self.after is not None:                             # (the shortcut probes: the outputs only, as _shortcut_case reads them)
            self.names = [nm for nm in p.net.outputs if nm in own]
        else:
            self.names = [n.name for n in p.net.nodes if n.name in cn.low.tensor_id and n.name in own]
        assert set(p.net.outputs) <= set(self.names) | {"h"}, (self.names, p.net.outputs)
        return cn

    def read(self, cn):
        return {nm: cn.read(nm, self.probe.batch) for nm in self.names}

    def check(self, got, what):
        """every read-back tensor against the cached exact reference (run_probe's and test_dethead_exact's comparisons)"""
        p = self.probe
        ref, _ = ep.cached_reference(self.key)
        if self.dethead:
            x, n = p.net.outputs[0], p.batch
            _, bb, kp = ref["h"]
            ep.assert_same_bits(got[x], ref[x], f"{what} / {x}")
            ep.assert_same_values(got["h"][..., 2:10].reshape(n, -1, 4), bb.astype(np.float32), f"{what} / bbox")
            ep.assert_same_values(got["h"][..., 10:30].reshape(n, -1, 10), kp.astype(np.float32), f"{what} / kps")
            return
        fp32 = {n.name for n in p.net.nodes if n.kind == "fc"}
        for nm in self.names:
            if nm in fp32:
                ep.assert_same_values(got[nm].reshape(np.shape(ref[nm])), np.asarray(ref[nm], np.float32), f"{what} / {nm}")
            else:
                ep.assert_same_bits(got[nm], ref[nm], f"{what} / {nm}")


def _has_ops(op, count):
    def check(low, cus):
        assert _kinds(low).count(op) == count, low.op_names
    return check


def _split_check(key, names, force, slabs):
    """the mirror's slabs of the probed convs (test_gpu_ops_exact._split_ok): more than one, so the partial sums go through scratch slot 1"""
    def check(low, cus):
        from scrfd_arcface_facerecognition_amd.lower import OP_CONV, W_TYPE
        batch = ep.PROBES[key]().batch
        for name in names:
            assert int(low.ops[low.op_names.index(name)][W_TYPE]) == OP_CONV, low.op_names
            m = ep.split_mirror(*ep.conv_geometry(low, name, batch), cus, tuple(int(v) for v in force.split(",")) if force else None)
            assert m["ksplit"] > 1 and len(m["slabs"]) > 1 and (slabs is None or m["slabs"] == slabs), (name, m)
    return check


def _gen12_ran(cn):
    picks = {p["name"]: p["gen"] for p in cn.plans()}
    assert picks["b.conv2"] == 12, picks


def _pairs():
    from scrfd_arcface_facerecognition_amd import lower
    split_key, split_names, split_force, split_slabs = ep.SPLIT_CASES[0]
    fc_key = ep.FC_KEYS[ep.FC_SHAPES[1]]
    untuned = dict(FID_NO_DIRECT="1")
    return {
        # the fused lateral + fpn levels (the 3x3 convs in front of them tune) beside the fused residual block, whose walk direction alternates per run
        "latfpn+bb": (Side(ep.LATFPN_KEYS[((16, 16), 1)], tunes=True, in_low=_has_ops(lower.OP_LATFPN, 3)),
                      Side(ep.BB_KEYS[((12, 20), 64, 5)], in_low=_has_ops(lower.OP_BBLOCK, 1))),
        # a conv that absorbs its block's shortcut (a generation-12 pick) tunes beside the detector head conv
        "shortcut+dethead": (Side(ep.SHORTCUT_KEYS[((37, 45), 64, 96, 2)], tunes=True, env=dict(FID_FORCE_GEN="12"), after=_gen12_ran),
                             Side(ep.DETHEAD_KEYS[((26, 26), 64, 3)], dethead=True, in_low=lambda low, cus: low.op_names.index("h"))),
        # the detector head conv tunes beside IResNet's form of the fused block
        "dethead+ir": (Side(ep.DETHEAD_KEYS[((26, 26), 64, 3)], tunes=True, dethead=True, in_low=lambda low, cus: low.op_names.index("h")),
                       Side(ep.IR_KEYS[((12, 20), 64, 5)], in_low=_has_ops(lower.OP_BBLOCK, 1))),
        # two 3x3 convs tune over every kernel family beside a forced split-K plan whose slabs meet in scratch slot 1 of the neighbour's context
        "family+splitk": (Side(ep.FAMILY_KEYS[((37, 21), 64, 64, 3)], tunes=True),
                          Side(split_key, untuned=True, env=dict(untuned, FID_CONV_FORCE=split_force),
                               in_low=_split_check(split_key, split_names, split_force, split_slabs))),
        # both lanes split: the forced split-K net is built and run (its slot 1 allocated) beside the FC, whose heuristic plan always splits its K axis
        "splitk+fc": (Side(split_key, untuned=True, env=dict(untuned, FID_CONV_FORCE=split_force),
                           in_low=_split_check(split_key, split_names, split_force, split_slabs)),
                      Side(fc_key, untuned=True, env=untuned, in_low=_split_check(fc_key, ("fc",), split_force, None))),   # (the hook is process-wide)
    }


PAIR_NAMES = ["latfpn+bb", "shortcut+dethead", "dethead+ir", "family+splitk", "splitk+fc"]
A_RUNS = 3                   # lane A's runs per pair: the first tunes (where the net has convs to tune), the others use the picks
FEED_DEPTH = 8               # runs the feeder queues between two of its events; it waits for the event before the last one: 8 to 16 runs stay queued
FEED_BATCHES = 20000         # the feeder's own end, should the main thread never stop it


@pytest.mark.parametrize("pair", PAIR_NAMES)
def test_exact_probes_beside_a_neighbour(monkeypatch, pair):
    """Lane B loops probe P2 (run_device on images uploaded beforehand, FEED_DEPTH to 2 x FEED_DEPTH runs always queued, fed by a second
    Python thread), while lane A BUILDS probe P1 on its own fresh context and runs it A_RUNS times: the first run tunes cold (hipMalloc /
    hipFree of the 320 MB flush buffer, candidates re-run, alternative weight images built and dropped), the others use the picks.  A feeder thread
    rather than K runs queued in advance: hipFree waits for every stream of the device, so a queue built in advance would be gone at the
    tuner's first hipFree; the thread keeps lane B busy through all of it.  After every run of A and every fourth batch of B all read-back
    tensors equal the exact reference of tests/exact_probe.py (bit for bit whatever kernel variant runs).
    Overlap: after A has a run's results on the host, B's newest event was not complete yet, or B finished whole batches during that run."""
    import torch
    sa, sb = _pairs()[pair]
    for k in ("FID_CONV_FORCE", "FID_FORCE_GEN", "FID_FORCE_NS", "FID_PC_RS", "FID_NO_DIRECT", "FID_PLAN", "FID_PLAN_RO", "FID_NO_BB_FUSE", "FID_BB_V",
              "FID_NO_LATFPN_FUSE", "FID_NO_SC_FUSE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in {**sa.probe.env, **sb.probe.env, **sa.env, **sb.env}.items():
        monkeypatch.setenv(k, v)
    la, lb = lh.Lane(), lh.Lane()
    cus = int(re.search(r"\|cus=(\d+)", la.ctx.name()).group(1))
    cb = sb.build(lb, monkeypatch)
    if sb.in_low is not None:
        sb.in_low(cb.low, cus)
    images_b = lb.ctx.to_device(sb.probe.images)

    class Feed:
        batches, last, reads, error = 0, None, [], None
    stop, started = threading.Event(), threading.Event()

    def feeder():
        try:
            prev = None
            while not stop.is_set() and Feed.batches < FEED_BATCHES:
                for _ in range(FEED_DEPTH):
                    cb.run_device(images_b, sb.probe.batch)
                ev = torch.cuda.Event()
                ev.record(lb.stream)
                Feed.last = ev
                if prev is not None:
                    prev.synchronize()
                prev = ev
                Feed.batches += 1
                started.set()
                if Feed.batches % 4 == 0:
                    Feed.reads.append(sb.read(cb))
            lb.ctx.sync()
            Feed.reads.append(sb.read(cb))
        except BaseException as e:                               # noqa: BLE001  (handed to the main thread)
            Feed.error = e
            started.set()

    th = threading.Thread(target=feeder)
    th.start()
    ca, got_a, overlap, tuned = None, [], 0, None
    try:
        assert started.wait(120) and Feed.error is None, Feed.error
        ca = sa.build(la, monkeypatch)                           # fid_net_create: hipMalloc + weight upload beside the neighbour
        if sa.in_low is not None:
            sa.in_low(ca.low, cus)
        for _ in range(A_RUNS):
            before = Feed.batches
            ca.run(sa.probe.images)
            got_a.append(sa.read(ca))
            ev = Feed.last
            overlap += int(th.is_alive() and Feed.error is None and ((ev is not None and not ev.query()) or Feed.batches > before))
            if tuned is None:
                tuned = len(ca.plans())
    finally:
        stop.set()
        th.join()
    try:
        if Feed.error is not None:
            raise Feed.error
        print(f"\n[two lanes] probes {pair}: lane B finished {Feed.batches} batches of {FEED_DEPTH} runs and was read {len(Feed.reads)} times while lane A "
              f"built its net, tuned {tuned} ops and ran; overlap seen after {overlap} of {A_RUNS} runs")
        if sa.after is not None:
            sa.after(ca)
        assert not sa.tunes or tuned > 0, f"probes {pair}: lane A's first run tuned nothing"
        for i, got in enumerate(got_a):
            sa.check(got, f"{sa.key} on lane A, run {i}, beside {sb.key}")
        for i, got in enumerate(Feed.reads):
            sb.check(got, f"{sb.key} on lane B, read {i}, beside {sa.key}")
        if sb.after is not None:
            sb.after(cb)
        assert overlap >= 1, f"probes {pair}: no overlap happened: lane B's feeder neither had work queued nor finished a batch while lane A ran"
    finally:
        for cn in (ca, cb):
            if cn is not None:
                cn.close()
        images_b.free()
        la.ctx.close()
        lb.ctx.close()


# ---- case 2: the benchmark's default, two grouped lanes ----------------------------------------------------------------------------------------

def _grouped_sequence(drivers):
    """six steps per lane over its three frame batches, issued round-robin; every group is read back after its flush (a download waits for
    the caller's own stream only, so the other lane's group is still running); then a seventh step whose partial group flush() finishes"""
    outs = {d: [] for d in drivers}
    for d in drivers:
        d.reset()
    for s in range(6):
        for d in drivers:
            d.step()
        if s & 1:
            for d in drivers:
                assert d.pipe.k == 0 and d.pipe.last_steps == 2
                outs[d].append(d.read())
    for d in drivers:
        d.step()
    for d in drivers:
        d.flush()
    for d in drivers:
        assert d.pipe.k == 0 and d.pipe.last_steps == 1
        outs[d].append(d.read())
    return outs


def test_grouped_lanes_round_robin(grouped):
    """Two GroupedFacePipeline(group=2) lanes as bench.py runs them, but with different frames (one all black per lane), detectors,
    recognisers (IResNet-50 at 30 crops) and galleries (29 and 700 rows): the round-robin sequence, then the two roles of run_roles."""
    a, b = grouped
    solo = {**_grouped_sequence([a]), **_grouped_sequence([b])}
    assert len(solo[a]) == 4
    for s in range(4):
        _assert_lanes_differ(solo[a][s], solo[b][s], f"grouped lanes, group {s}")
    black = a.lane.seed % B                                      # the all-black frame of lane A's second batch: an empty slot in group 0
    assert solo[a][0]["counts1"][black] == 0 and not np.any(lh.raw(solo[a][0]["q"][(B + black) * a.pipe.F:(B + black + 1) * a.pipe.F]) & 0x7F)
    both = _grouped_sequence([a, b])
    for name, d in (("A", a), ("B", b)):
        lh.assert_same_snapshots(both[d], solo[d], f"grouped lanes round-robin, lane {name}")
    _roles_case(a, b, "grouped lanes")


# ---- case 3: a packed lane beside a tracked lane --------------------------------------------------------------------------------------------------

def test_unlike_lanes(lanes):
    """Lane A: PackedFacePipeline(max_num=0, measure=True).  Lane B: TrackedFacePipeline over nine frames that move four pixels per frame, three
    per step; as the neighbour it cycles through them, so tracks continue inside the video and end and start where it begins again.  Compared
    to the bit in both roles: packed offsets and rows, measure rows, the tracker's state, names and ids of results_tracked()."""
    from scrfd_arcface_facerecognition_amd._lib import TRACK_STARTED
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet
    from scrfd_arcface_facerecognition_amd.pipeline import calibrate_detector_bias
    la, lb = lanes
    video = lh.video_frames(lb.seed + 1)
    mp = pytest.MonkeyPatch()
    mp.setenv("FID_AUTOTUNE", "0")
    try:
        det_P, _ = calibrate_detector_bias(lb.ctx, lb.det_net, lb.det_P, video[:B], target=30, max_batch=B)
        det_v = CompiledNet(lb.ctx, lb.det_net, det_P, max_batch=B)
    finally:
        mp.undo()
    a, b = lh.PackedDriver(la), lh.TrackedDriver(lb, video, det_v)
    try:
        solo = _roles_case(a, b, "unlike lanes")
    finally:
        b.pipe.close()
        det_v.close()
    # what lane B's sequence was built for, read off its solo run: tracks that continue, start after the first step, and have ended
    cont = late = 0
    for i, s in enumerate(solo[b]):
        valid = np.arange(s["track"].shape[1])[None, :] < np.clip(s["counts"], 0, s["track"].shape[1])[:, None]
        word = s["track"][..., 1]
        cont += int(np.sum(valid & (word >= 0) & ((word & TRACK_STARTED) == 0)))
        late += int(np.sum(valid & (word >= 0) & ((word & TRACK_STARTED) != 0))) if i > 0 else 0
    last = solo[b][-1]
    ended = int(last["per_stream"][0, 0]) - int(np.sum(last["slots"][0, :, 0] >= 0))
    print(f"[two lanes] unlike lanes: tracked lane continued {cont} detections, started {late} tracks after its first snapshot, {ended} tracks ended")
    assert cont > 0 and late > 0 and ended > 0, (cont, late, ended)
    assert np.any(solo[a][-1]["offsets"]) and np.any(solo[a][-1]["stats"][:, 7] & 1), "the packed lane measured no row"


# ---- case 4: gallery searches beside a pipeline in flight -------------------------------------------------------------------------------------------

def _store_rows(seed=5):
    """300 rows: 50 persons three times each (cosine about 0.92 among a person's rows: duplicates at 0.8) and 150 persons once"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((200, 512)).astype(np.float32)
    owner = np.concatenate([np.repeat(np.arange(50), 3), np.arange(50, 200)])
    rows = centres[owner] + np.float32(0.3) * rng.standard_normal((len(owner), 512)).astype(np.float32)
    queries = centres[rng.integers(0, 200, 192)] + (np.float32(0.2) + np.float32(0.8) * rng.random((192, 1), dtype=np.float32)) * \
        rng.standard_normal((192, 512)).astype(np.float32)
    queries[::7] = rng.standard_normal((len(queries[::7]), 512)).astype(np.float32)      # strangers
    queries[5] = 0                                                                       # a visit without a face
    return rows, queries


def _search_calls(vg, q):
    """the five searches in turn, on query counts that grow from call to call (scratch slots 2 and 3 are sized by the count: they are freed
    and allocated again in mid-sequence), and the fused search once more at the largest count"""
    return [("fused", lambda: vg.search(q[:6], k=5, via="fused")),
            ("coarse", lambda: vg.search(q[:24], k=5, via="coarse", rerank=32)),
            ("range", lambda: vg.range_search(q[:48], 0.5)),
            ("dedup", lambda: vg.find_and_merge_duplicates(0.8, via="device")),
            ("group", lambda: vg.group_visits(q[:96])),
            ("fused again", lambda: vg.search(q, k=7, via="fused"))]


def test_searches_beside_a_neighbour(lanes, grouped, monkeypatch):
    """Lane A holds a VectorGallery on a context of its own on lane A's stream and runs its searches one by one; before each, lane B's
    grouped pipeline queues K units.  Two of the calls change the store, so the solo answers come from a twin store on a twin context (same
    stream, same rows, scratch as fresh as the first one's: both grow their slots at the same calls), not from a second pass over one store.
    Each call's answer equals the twin's; lane B's buffers, read after every call, equal those of the same sequence run alone."""
    import time
    import torch
    from scrfd_arcface_facerecognition_amd._lib import Context
    from scrfd_arcface_facerecognition_amd.engine import VectorGallery, _gallery_ptr
    la, _ = lanes
    _, b = grouped
    rows, queries = _store_rows()

    made = []

    def store():
        ctx = Context(0, la.stream.cuda_stream)
        vg = VectorGallery(ctx, 512, capacity=512)
        vg.upsert(list(range(len(rows))), rows)
        ctx.sync()
        made.append((ctx, vg))
        return vg

    def stored_rows(vg):
        gal = vg._gal
        return gal.ctx.borrow(_gallery_ptr(gal), (gal.Gp, 512), np.float16).download()

    def sequence(vg, k, in_flight, free_now=None):
        b.reset()
        answers, snaps, seen, ms = [], [], [], []
        for name, call in _search_calls(vg, queries):
            for _ in range(k):
                b.unit()
            ev = None
            if in_flight:
                ev = torch.cuda.Event()
                ev.record(b.stream)
            else:
                b.ctx.sync()
            t0 = time.perf_counter()
            answers.append(call())
            ms.append((time.perf_counter() - t0) * 1e3)
            if ev is not None:
                if not ev.query():
                    seen.append(name)
                free_now()
            b.ctx.sync()
            snaps.append(b.read())
        return answers, snaps, seen, ms

    tb = lh.timings(b)
    twin = store()
    _, _, _, ms = sequence(store(), 0, False)                    # a pass that only measures the calls (on a store of its own: it changes it)
    k = lh.choose_k(tb, dict(dev_ms=0.0, wall_ms=max(ms)))
    print(f"\n[two lanes] searches: calls take {', '.join(f'{m:.2f}' for m in ms)} ms alone; lane B unit {tb['dev_ms']:.3f} ms device, "
          f"{tb['enqueue_ms']:.3f} ms to enqueue; queues K = {k} units before every call")
    want, snaps_solo, _, _ = sequence(twin, k, False)
    assert len(want[3]) > 0 and any(len(r) for r in want[0]) and any(len(r) for r in want[2]), "the searches found nothing"
    assert {r["verdict"] for r in want[4]} >= {"new", "recognised", "no face"}, {r["verdict"] for r in want[4]}
    vg = store()
    free_now = lh.free_later(monkeypatch)
    try:
        got, snaps, seen, _ = sequence(vg, k, True, free_now)
    finally:
        free_now()
        monkeypatch.undo()
    print(f"[two lanes] searches: lane B still running after {len(seen)} of {len(got)} calls: {', '.join(seen)}")
    for (name, _), g, w in zip(_search_calls(vg, queries), got, want):
        assert lh.same_result(g, w), f"searches: {name} beside a neighbour differs from the same call made solo"
    assert sorted(vg.row_of.items()) == sorted(twin.row_of.items()) and lh.same(stored_rows(vg), stored_rows(twin)), "searches: the stores differ afterwards"
    lh.assert_same_snapshots(snaps, snaps_solo, "searches, lane B")
    assert len(seen) >= 1, f"searches: no overlap happened: lane B's queue (K = {k}) was never still running when a call returned"
    for ctx, store_ in made:
        store_._gal.close()
        ctx.close()


# ---- case 5: the staged schedule ------------------------------------------------------------------------------------------------------------------------

def test_staged_schedule_equals_one_context(lanes):
    """bench.py --schedule stages at small size: lane A's detector and PostProcessors on context A, a recogniser with lane A's weights and
    lane A's gallery on context B, two FacePipeline(cB, det, recB) objects in turn, ev_det / ev_free between the streams exactly as bench.py
    places them, the host one step ahead of the read-back.  Six steps over six different frame batches (lane A's and lane B's); each
    step's detections, crops, q, idx and score equal FacePipeline.run_step on context A alone with the same detector object."""
    import torch
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet, Gallery
    from scrfd_arcface_facerecognition_amd.pipeline import FacePipeline, GroupedFacePipeline
    la, lb = lanes
    F = 5
    sA, cA, sB, cB = la.stream, la.ctx, lb.stream, lb.ctx
    frames = la.dev + [cA.to_device(f) for f in lb.frames]
    mp = pytest.MonkeyPatch()
    mp.setenv("FID_AUTOTUNE", "0")                               # recB and the reference recogniser share the heuristic plans
    try:
        recB = CompiledNet(cB, la.rec_net, la.rec_P, max_batch=32)
    finally:
        mp.undo()
    galB = Gallery(cB, la.gal_host)

    def snapshot(p):
        return {"counts": p.post.counts.download(), "det": p.post.det.download(), "kps": p.post.kps.download(), "crops": p.crops.download(),
                "q": p.q.download(), "idx": p.idx.download(), "score": p.score.download()}

    def zero(p):
        for buf in (p.post.counts, p.post.det, p.post.kps, p.crops, p.q, p.idx, p.score):
            buf.zero()
    plain = FacePipeline(cA, la.det, la.rec, batch=B, faces_per_frame=F)
    # the reference alternates two pipelines as well, so a row no kernel writes holds what the same step left there two steps earlier
    plains = [plain, FacePipeline(cA, la.det, la.rec, batch=B, faces_per_frame=F)]
    for p in plains:
        zero(p)
    cA.sync()
    want = []
    for i, fr in enumerate(frames):
        plains[i & 1].run_step(fr, H, W, la.gallery, THRESH)
        want.append(snapshot(plains[i & 1]))
    assert not lh.same(want[0]["det"], want[3]["det"]) and not lh.same(want[0]["q"], want[3]["q"]), "the steps' solo results do not differ"
    assert all(np.any(lh.raw(w["q"])) for w in want)

    spipes = [FacePipeline(cB, la.det, recB, batch=B, faces_per_frame=F) for _ in range(2)]
    with pytest.raises(ValueError):
        spipes[0].run_step(frames[0], H, W, galB, THRESH)        # nothing orders the detector's stream and this pipeline's
    with pytest.raises(ValueError):
        GroupedFacePipeline(cB, la.det, recB, batch=B, faces_per_frame=F, group=2).collect(frames[0], H, W)
    for p in spipes:
        zero(p)
    cA.sync()
    cB.sync()
    ev_det = [torch.cuda.Event() for _ in range(2)]
    ev_free = [None, None]
    ev_done = [None, None]

    def step(i):
        k = i & 1
        p = spipes[k]
        with torch.cuda.stream(sA):
            if ev_free[k] is not None:
                sA.wait_event(ev_free[k])
            p.detect(frames[i], H, W)
            sA.record_event(ev_det[k])
        with torch.cuda.stream(sB):
            sB.wait_event(ev_det[k])
            p.embed(frames[i], H, W)
            ev_free[k] = sB.record_event()
            p.match(galB, THRESH)
            ev_done[k] = sB.record_event()

    def read(i, newest):
        """step i's buffers: the post-process buffers first (a download on context A waits for stream A only); whether the newest step's
        match on stream B was still outstanding then is the overlap of this schedule"""
        p = spipes[i & 1]
        out = {"counts": p.post.counts.download(), "det": p.post.det.download(), "kps": p.post.kps.download()}
        busy = newest is not None and not ev_done[newest & 1].query()
        out.update(crops=p.crops.download(), q=p.q.download(), idx=p.idx.download(), score=p.score.download())
        return out, busy
    got, seen = [], 0
    step(0)
    for i in range(1, len(frames)):
        step(i)                                                  # the host runs ahead: step i is queued before step i - 1 is read
        out, busy = read(i - 1, i)
        got.append(out)
        seen += int(busy)
    got.append(read(len(frames) - 1, None)[0])
    print(f"\n[two lanes] staged schedule: the newest step was still running at {seen} of {len(frames) - 1} read-backs")
    recB.close()
    for i, (g, w) in enumerate(zip(got, want)):
        diff = lh.first_difference(g, w)
        assert diff is None, f"staged schedule, step {i}: differs from FacePipeline.run_step on one context: {diff}"
    assert seen >= 1, "staged schedule: no overlap happened: at every read-back the step queued ahead had already finished"


# ---- case 6: one Python thread per lane -------------------------------------------------------------------------------------------------------------------

def test_two_threads_two_lanes(grouped):
    """Case 2's lanes, each driven by its own Python thread with nothing but a barrier at the start between them: the host side of lane
    isolation (the thread-local error string, the ensure_dyn_lds map, the binding's load lock).  Three passes of the sequence per thread."""
    a, b = grouped
    solo = {**_grouped_sequence([a]), **_grouped_sequence([b])}
    _assert_lanes_differ(solo[a][0], solo[b][0], "two threads")
    barrier = threading.Barrier(2)
    got, errors = {a: [], b: []}, []

    def work(d):
        try:
            barrier.wait(120)
            for _ in range(3):
                got[d].append(_grouped_sequence([d])[d])
        except BaseException as e:                               # noqa: BLE001  (handed to the main thread)
            errors.append(e)
            barrier.abort()
    threads = [threading.Thread(target=work, args=(d,)) for d in (a, b)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:
        raise errors[0]
    for name, d in (("A", a), ("B", b)):
        assert len(got[d]) == 3
        for p, seq in enumerate(got[d]):
            lh.assert_same_snapshots(seq, solo[d], f"two threads, lane {name}, pass {p}")
