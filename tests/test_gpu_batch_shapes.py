"""GPU: every conv kernel family on ONE resident net that runs at partial, shrinking and sub-batched batches -- the pattern of
PackedFacePipeline(rows="count"), where a recogniser built for a large max_batch runs at whatever row count a step needs and its activation
slots still hold the previous step's rows.

Two contracts of the executor are pinned here (executor section): rows at or beyond the batch are never READ into a live result
(they are poisoned with 65504 and with NaN before every partial run: a loader that masks a ghost lane by multiplying turns NaN into a live
NaN) and never WRITTEN (the poison is checked byte for byte afterwards: a kernel only knows the batch, so a store into row b is a heap
overrun on a net whose max_batch is b).

  1. forced families (the generation codes of test_gpu_conv_families.py) at partial and shrinking batches against the fp32 oracle
  2. the same picks on a net allocated for exactly b images: bit for bit, every tensor that still holds its own rows
  3. a duplicated image at the first, the middle and the LAST live row (next to the first ghost): bit-identical rows
  4. sub-batches (fid_net_set_sub_batch: run_op with first > 0): oracle, and every pass bit for bit against a small net that ran the slice alone
  5. fid_net_run_profiled computes what fid_net_run computes
  6. IResNet-50 at max_batch 192 under plans/mi355x.plan at the row counts production uses (the batch-128 picks the headline times)
"""
import os

import numpy as np
import pytest

from oracle import align, nets as onets
from scrfd_arcface_facerecognition_amd import archs
from scrfd_arcface_facerecognition_amd.lower import W_X_SCOP

from family_helpers import SlotGuard, force_family, forced_ran, own_data_tensors, slot_table, stack

pytestmark = pytest.mark.gpu

# the generation codes of test_conv_family (those of test_conv_mosaic_7x7 and test_conv_strip are among them)
CODES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 91, 92, 93, 94, 96, 97, 98, 909, 929, 939, 910, 11, 25, 51, 59]

# (map, channels, max_batch M, partial batches in running order, the batch of the bit-for-bit allocation check, sub-batch sizes).
# The image counts break each packing rule: MOSAIC packs four 7x7 images per tile (5 = one tile + one image, 8 = two full tiles, 3 / 2 / 1 =
# ghosts inside the only tile); 14x14 STRIP tiles are 16 strip columns (9 -> 126 columns = 7 tiles + 14 lanes, 16 -> 224 = 14 full tiles,
# 8 -> 112 = 7 full tiles, 1 -> 14 lanes of one tile); pair-of-tiles items and the two-items-per-workgroup loop see odd and even item counts.
MAPS = [((7, 7), (128, 128), 9, (5, 1, 8, 3, 2), 5, (1, 2, 3, 4)),
        ((7, 7), (64, 192), 9, (5, 1, 8, 3, 2), 3, (2, 4)),
        ((14, 14), (128, 128), 17, (9, 1, 16, 8), 9, (1, 2, 3, 4)),
        ((14, 14), (64, 256), 17, (9, 1, 16, 8), 8, (3, 4)),
        ((37, 21), (64, 128), 3, (2, 1), 2, (1, 2)),
        ((20, 20), (64, 96), 5, (3, 1, 4), 3, (1, 2, 3, 4)),
        ((20, 20), (224, 224), 5, (3, 1, 4), 4, (2, 3)),
        ((28, 28), (128, 256), 5, (2, 3), 2, (1, 2, 3, 4))]
MAP_IDS = [f"{hw[0]}x{hw[1]}-{'_'.join(map(str, ch))}" for hw, ch, *_ in MAPS]
# parts 2 and 4 run on four of the eight stacks: (7, 7) / (128, 128), (14, 14) / (128, 128), (37, 21) / (64, 128) and (20, 20) / (64, 96).  Left out
# there for the time budget of this file (docs/FINDINGS.md holds the measured times): (7, 7) / (64, 192), (14, 14) / (64, 256), (20, 20) / (224, 224)
# and (28, 28) / (128, 256).  Parts 1 and 3 keep every stack.
MAPS_2 = [m for i, m in enumerate(MAPS) if i in (0, 2, 4, 5)]
MAP_IDS_2 = [MAP_IDS[MAPS.index(m)] for m in MAPS_2]

# code -> {"partial" / "shrinking" / "alloc" / "sub": [(stack, batch), ...]}: where the forced family really ran and passed (printed and asserted
# by the last test; "alloc" = the bit-for-bit comparison with a net allocated for exactly that batch)
KINDS = ("partial", "shrinking", "alloc", "sub")
RAN = {c: {k: [] for k in KINDS} for c in CODES}
_CASES, _PLANS = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plan_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("plans")


def nhwc(ref):
    return np.transpose(ref, (0, 2, 3, 1))


def stack_case(hw, chans, M):
    """(net, params, image sets X and Y, their oracle outputs): computed once per stack, sliced per run"""
    key = (hw, chans, M)
    if key not in _CASES:
        net = stack(hw, chans)
        P = archs.synth_params(net, seed=9)
        rng = np.random.default_rng(3)
        X, Y = (rng.integers(0, 256, (M,) + hw + (3,), dtype=np.uint8) for _ in range(2))
        ref = [nhwc(onets.run_net(net, P, align.blob_from_images(list(im), net.in_scale, net.in_mean))[net.outputs[0]]) for im in (X, Y)]
        _CASES[key] = (net, P, X, Y, ref[0], ref[1])
    return _CASES[key]


def dup_rows(b):
    """row -> source image of a partial batch: the last live row (and the middle one of four or more) repeats image 0"""
    idx = np.arange(b)
    idx[b - 1] = 0
    if b >= 4:
        idx[b // 2] = 0
    return idx


def run_rows(cn, buf, images):
    """images into the first rows of the test's own input buffer of max_batch images, every other image white; run at len(images)"""
    full = np.full(buf.shape, 255, np.uint8)
    full[:len(images)] = images
    buf.upload(full)
    cn.run_device(buf, len(images))
    return len(images)


def raw(cn, name, first, n):
    """rows [first, first + n) of a tensor as stored (padded channels included), as bit patterns"""
    ptr, (H, W, _, Cp), dt = cn.tensor(name)
    item = np.dtype(dt).itemsize
    buf = cn.ctx.borrow(ptr + first * H * W * Cp * item, (n, H, W, Cp), np.uint32 if item == 4 else np.uint16)
    return buf.download()


def rel_err(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def tuned_net(ctx, plan_dir, key, net, P, max_batch):
    """a net that starts from the picks earlier tests of the same (family, stack) made (the plan key is device | table | op | batch, not the
    allocation): only batch sizes no test has run yet are timed"""
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet
    cn = CompiledNet(ctx, net, P, max_batch=max_batch)
    path = str(plan_dir / ("_".join(map(str, key)).replace(" ", "").replace("(", "").replace(")", "").replace(",", "x") + ".plan"))
    if os.path.exists(path):
        cn.load_plan(path)
    _PLANS[id(cn)] = path
    return cn


def keep_plan(cn):
    path = _PLANS.pop(id(cn))
    if os.path.exists(path):
        os.unlink(path)
    cn.save_plan(path)
    return path


def frozen_net(ctx, monkeypatch, net, P, max_batch, plan):
    """a net of exactly max_batch images that times nothing and runs the picks of a plan file"""
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet
    monkeypatch.setenv("FID_AUTOTUNE", "0")
    cn = CompiledNet(ctx, net, P, max_batch=max_batch)
    monkeypatch.delenv("FID_AUTOTUNE")
    assert cn.load_plan(plan) > 0
    return cn


def test_slot_guard_sees_a_row_written_beyond_the_batch(ctx, monkeypatch):
    """the guard itself: poisoned for b rows, a (legal) run at b + 1 rows writes row b of every slot and the check must name it; a run at b
    rows passes the same check; both patterns read back as what they claim to be"""
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet
    monkeypatch.delenv("FID_AUTOTUNE", raising=False)
    net, P, X, _, _, _ = stack_case((20, 20), (64, 96), 5)
    cn = CompiledNet(ctx, net, P, max_batch=5)
    buf = ctx.to_device(np.full((5, 20, 20, 3), 255, np.uint8))
    try:
        for pattern in ("max", "nan"):
            guard = SlotGuard(ctx, cn, 2, pattern).poison()
            assert len(guard.regions) == len(slot_table(cn.low)[2]) >= 3
            ghost = cn.read(net.outputs[0], 5)[2:]
            assert np.isnan(ghost).all() if pattern == "nan" else (ghost == 65504.0).all()
            run_rows(cn, buf, X[:2])
            guard.check("two rows")
            run_rows(cn, buf, X[:3])
            with pytest.raises(AssertionError, match=r"slot \d+ written beyond batch 2: first changed byte \d+ \(image row 2,"):
                guard.check("three rows")
    finally:
        cn.close()


# ---- 1. + 3. forced families at partial and shrinking batches, against the oracle; duplicated images at the edge of the batch -----------------

@pytest.mark.parametrize("gen", CODES)
@pytest.mark.parametrize("hw,chans,M,seq,b_alloc,subs", MAPS, ids=MAP_IDS)
def test_family_partial_and_shrinking_batches(ctx, monkeypatch, plan_dir, gen, hw, chans, M, seq, b_alloc, subs):
    force_family(monkeypatch, gen)
    monkeypatch.delenv("FID_AUTOTUNE", raising=False)
    net, P, X, Y, refX, refY = stack_case(hw, chans, M)
    out = net.outputs[0]
    mi = MAPS.index((hw, chans, M, seq, b_alloc, subs))
    cn = tuned_net(ctx, plan_dir, (gen, hw, chans), net, P, M)
    buf = ctx.to_device(np.full((M,) + hw + (3,), 255, np.uint8))
    try:
        run_rows(cn, buf, Y)
        ran = forced_ran(cn, gen, M)
        if not ran:
            pytest.skip(f"generation code {gen} takes no layer of this stack")
        got = cn.read(out, M)
        print(f"code {gen} {hw} {chans}: batch {M}: rel err {rel_err(got, refY):.2e} {ran}")
        assert rel_err(got, refY) < 8e-3, (M, ran)
        prev, hits = M, 0
        for i, b in enumerate(seq):
            pattern = ("max", "nan")[(i + mi) % 2]      # both patterns meet every family
            idx = dup_rows(b)
            guard = SlotGuard(ctx, cn, b, pattern).poison()
            run_rows(cn, buf, X[idx])
            ran = forced_ran(cn, gen, b)
            got = cn.read(out, b)
            what = f"code {gen} {hw} {chans}: batch {b} after {prev} of {M}, poison {pattern}, picks {ran}"
            guard.check(what)
            assert np.isfinite(got).all(), what + f": {np.count_nonzero(~np.isfinite(got).all(axis=(1, 2, 3)))} live rows not finite"
            print(f"{what}: rel err {rel_err(got, refX[idx]):.2e}")
            assert rel_err(got, refX[idx]) < 8e-3, what
            bits = raw(cn, out, 0, b)
            assert np.array_equal(bits[b - 1], bits[0]), what + ": the last live row differs from row 0 (same image)"
            assert np.array_equal(bits[b // 2], bits[idx[b // 2]]), what + ": the middle row differs from its copy"
            if ran:                                      # (a family may take no layer at THIS image count: a single item has no pair)
                hits += 1
                RAN[gen]["partial"].append((MAP_IDS[mi], b))
                if b < prev:
                    RAN[gen]["shrinking"].append((MAP_IDS[mi], b))
            prev = b
        keep_plan(cn)
        if not hits:
            pytest.skip(f"generation code {gen} takes no layer of this stack at any of the batches {seq}")
    finally:
        _PLANS.pop(id(cn), None)
        cn.close()


# ---- 2. same picks, different allocation: bit for bit -----------------------------------------------------------------------------------

@pytest.mark.parametrize("gen", CODES)
@pytest.mark.parametrize("hw,chans,M,seq,b,subs", MAPS_2, ids=MAP_IDS_2)
def test_family_partial_batch_equals_exact_allocation(ctx, monkeypatch, plan_dir, gen, hw, chans, M, seq, b, subs):
    """net A (max_batch M) runs M images, is poisoned, runs b; net B (max_batch b) loads A's picks and runs the same b images: every tensor
    that still holds its own rows is bit-identical -- the kernels and the batch are the same, only the allocation behind row b differs"""
    force_family(monkeypatch, gen)
    monkeypatch.delenv("FID_AUTOTUNE", raising=False)
    net, P, X, Y, _, _ = stack_case(hw, chans, M)
    A = tuned_net(ctx, plan_dir, (gen, hw, chans), net, P, M)
    B = None
    buf = ctx.to_device(np.full((M,) + hw + (3,), 255, np.uint8))
    try:
        run_rows(A, buf, Y)
        images = X[dup_rows(b)]
        guard = SlotGuard(ctx, A, b, "nan").poison()
        run_rows(A, buf, images)
        ran = forced_ran(A, gen, b)
        if not ran:
            pytest.skip(f"generation code {gen} takes no layer of this stack at batch {b}")
        guard.check(f"code {gen} {hw} {chans}: batch {b} of {M}")
        plan = keep_plan(A)
        B = frozen_net(ctx, monkeypatch, net, P, b, plan)
        B.run(images)
        assert forced_ran(B, gen, b) == ran
        names = own_data_tensors(A.low)
        assert net.outputs[0] in names and len(names) >= 2
        for name in names:
            assert np.array_equal(raw(A, name, 0, b), raw(B, name, 0, b)), (name, ran)
        RAN[gen]["alloc"].append((MAP_IDS[MAPS.index((hw, chans, M, seq, b, subs))], b))
    finally:
        _PLANS.pop(id(A), None)
        A.close()
        if B is not None:
            B.close()


# ---- 4. sub-batches -----------------------------------------------------------------------------------------------------------------------

def single_tenant_tensors(low):
    """tensors alone in their slot (every output is): the only ones whose rows of EVERY pass survive a sub-batched run -- in a shared slot a
    later pass's rows of a small early tenant land inside an earlier pass's rows of a larger late one, which that pass has consumed by then"""
    t_slot, _, _ = slot_table(low)
    views = {i for n, i in low.tensor_id.items() if n.endswith(".in_view")}
    return sorted(n for n, i in low.tensor_id.items() if i not in views and sum(1 for j, s in enumerate(t_slot) if s == t_slot[i] and j not in views) == 1)


def check_sub_batches(ctx, monkeypatch, A, net, P, images, subs, check_oracle, label):
    """A has run `images` whole once.  For every sub-batch size: run in passes, check_oracle(A), then every pass -- full-size ones and the ragged
    remainder -- bit for bit against a net of exactly that many images that loaded A's picks and ran the slice alone (same kernel, same batch:
    only the `first` offset of every operand differs).  Finally sub-batch 0 restores the whole-batch result bit for bit."""
    M = len(images)
    buf = ctx.to_device(images)
    names = own_data_tensors(A.low)
    whole = {n: raw(A, n, 0, M) for n in names}
    singles = single_tenant_tensors(A.low)
    assert set(net.outputs) <= set(singles)
    import tempfile
    for sb in subs:
        A.set_sub_batch(sb)
        A.run_device(buf, M)
        check_oracle(A, f"{label}: sub-batch {sb} of {M}", sb)
        got = {n: raw(A, n, 0, M) for n in singles}
        fd, plan = tempfile.mkstemp(suffix=".plan")
        os.close(fd)
        os.unlink(plan)
        A.save_plan(plan)
        small = {}
        try:
            for first in range(0, M, sb):
                nb = min(sb, M - first)
                if nb not in small:
                    small[nb] = frozen_net(ctx, monkeypatch, net, P, nb, plan)
                small[nb].run(images[first:first + nb])
                for n in singles:
                    assert np.array_equal(got[n][first:first + nb], raw(small[nb], n, 0, nb)), f"{label}: sub-batch {sb}: rows {first}..{first + nb - 1} of {n} differ from the slice run alone"
        finally:
            for s in small.values():
                s.close()
            os.unlink(plan)
    A.set_sub_batch(0)
    A.run_device(buf, M)
    for n in names:
        assert np.array_equal(raw(A, n, 0, M), whole[n]), f"{label}: {n} after set_sub_batch(0)"


@pytest.mark.parametrize("gen", CODES)
@pytest.mark.parametrize("hw,chans,M,seq,b_alloc,subs", MAPS_2, ids=MAP_IDS_2)
def test_family_sub_batches(ctx, monkeypatch, plan_dir, gen, hw, chans, M, seq, b_alloc, subs):
    force_family(monkeypatch, gen)
    monkeypatch.delenv("FID_AUTOTUNE", raising=False)
    net, P, X, _, refX, _ = stack_case(hw, chans, M)
    out = net.outputs[0]
    A = tuned_net(ctx, plan_dir, (gen, hw, chans), net, P, M)
    try:
        A.run(X)
        if not forced_ran(A, gen, M):
            pytest.skip(f"generation code {gen} takes no layer of this stack")
        hit = []

        def oracle(cn, what, sb):
            got = cn.read(out, M)
            assert np.isfinite(got).all(), what
            assert rel_err(got, refX) < 8e-3, what
            if forced_ran(cn, gen, min(sb, M)) and (M % sb == 0 or forced_ran(cn, gen, M % sb)):
                hit.append(sb)
        check_sub_batches(ctx, monkeypatch, A, net, P, X, subs, oracle, f"code {gen} {hw} {chans}")
        keep_plan(A)
        if not hit:
            pytest.skip(f"generation code {gen} takes no layer of this stack at the sub-batch sizes {subs}")
        RAN[gen]["sub"] += [(MAP_IDS[MAPS.index((hw, chans, M, seq, b_alloc, subs))], sb) for sb in hit]
    finally:
        _PLANS.pop(id(A), None)
        A.close()


def _heads_oracle(net, P, images):
    ref = onets.run_net(net, P, align.blob_from_images(list(images), net.in_scale, net.in_mean))
    n = len(images)

    def check(cn, what, sb=None):
        for name in net.outputs:                                   # the bounds of test_scrfd_heads
            fused = cn.read(name, n)
            sc, bb, kp = ref[name]
            assert np.abs(fused[..., 0:2].reshape(n, -1, 1) - sc).max() < 3e-3, (what, name)
            assert np.abs(fused[..., 2:10].reshape(n, -1, 4) - bb).max() < 3e-2, (what, name)
            assert np.abs(fused[..., 10:30].reshape(n, -1, 10) - kp).max() < 3e-2, (what, name)
    return check


def _embedding_oracle(net, P, images, components):
    ref = onets.run_net(net, P, align.blob_from_images(list(images), net.in_scale, net.in_mean))[net.outputs[0]].reshape(len(images), -1)

    def check(cn, what, sb=None):
        e = cn.read(net.outputs[0], len(images)).reshape(-1, ref.shape[1])
        for i in range(len(images)):                               # the bounds of test_arcface_r50_embeddings / test_arcface_mbf_embeddings
            assert np.isfinite(e[i]).all(), (what, i)
            assert 1.0 - float(e[i] @ ref[i] / np.linalg.norm(e[i]) / np.linalg.norm(ref[i])) < 1e-3, (what, i)
            if components:
                assert np.abs(e[i] / np.linalg.norm(e[i]) - ref[i] / np.linalg.norm(ref[i])).max() < 1e-3, (what, i)
    return check


@pytest.mark.parametrize("arch,n,subs", [("scrfd_10g", 5, (1, 2, 4)), ("scrfd_500m", 5, (1, 2, 4)), ("scrfd_500m+dwpw", 5, (1, 2, 4)),
                                         ("arcface_r50", 6, (2, 4)), ("arcface_mbf", 6, (1, 2, 4))])
def test_architecture_sub_batches(ctx, monkeypatch, arch, n, subs):
    """the fused ops and the split-K workspace the forced stacks do not reach (stem_block, stem_rows, conv_bb, lat_fpn, dethead, mbf_block,
    dwpw with its opt-in hook), in passes of 1 / 2 / 4 images with exact and ragged remainders (IResNet-50, the one net whose every new
    batch size costs seconds of candidate timing: 2 / 4 -- its single-image pass is the 37 -> 1 row step of the plan test below)"""
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet
    from scrfd_arcface_facerecognition_amd import lower
    monkeypatch.delenv("FID_AUTOTUNE", raising=False)
    monkeypatch.delenv("FID_DWPW_FUSE", raising=False)
    if arch.endswith("+dwpw"):
        monkeypatch.setenv("FID_DWPW_FUSE", "1")
    name = arch.split("+")[0]
    det = name.startswith("scrfd")
    net = archs.ARCHS[name]((320, 320)) if det else archs.ARCHS[name]()
    P = archs.synth_params(net, seed=0)
    images = np.random.default_rng(17).integers(0, 256, (n,) + tuple(net.in_hw) + (3,), dtype=np.uint8)
    A = CompiledNet(ctx, net, P, max_batch=n)
    kinds = {int(r[lower.W_TYPE]) for r in A.low.ops}
    want = {"scrfd_10g": {lower.OP_STEMFUSED, lower.OP_BBLOCK, lower.OP_LATFPN}, "scrfd_500m": {lower.OP_STEM, lower.OP_DWCONV, lower.OP_MBBLOCK},
            "scrfd_500m+dwpw": {lower.OP_STEM, lower.OP_DWPW}, "arcface_r50": {lower.OP_STEMBLOCK, lower.OP_BBLOCK},
            "arcface_mbf": {lower.OP_MBBLOCK}}[arch]
    assert want <= kinds, (arch, kinds)
    if det:                                                  # the three fused detector heads (sigmoid on the class scores, fp32 output)
        assert sum(1 for r in A.low.ops if int(r[lower.W_TYPE]) == lower.OP_CONV and r[lower.W_NSIG] > 0) == 3
    try:
        oracle = _heads_oracle(net, P, images) if det else _embedding_oracle(net, P, images, components=(name == "arcface_r50"))
        A.run(images)
        oracle(A, f"{arch}: whole batch {n}")
        check_sub_batches(ctx, monkeypatch, A, net, P, images, subs, oracle, arch)
    finally:
        A.close()


# ---- 5. the profiled run -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arch,n", [("scrfd_500m", 3), ("arcface_r50", 3)])
def test_profiled_run_equals_plain_run(ctx, monkeypatch, arch, n):
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet
    monkeypatch.delenv("FID_AUTOTUNE", raising=False)
    net = archs.ARCHS[arch]((320, 320)) if arch.startswith("scrfd") else archs.ARCHS[arch]()
    P = archs.synth_params(net, seed=0)
    images = np.random.default_rng(19).integers(0, 256, (n,) + tuple(net.in_hw) + (3,), dtype=np.uint8)
    cn = CompiledNet(ctx, net, P, max_batch=n)
    try:
        buf = ctx.to_device(images)
        cn.run_device(buf, n)
        cn.run_device(buf, n)                       # (the first run tunes: a shortcut conv its consumer absorbs from then on ran once more)
        names = own_data_tensors(cn.low)
        assert set(net.outputs) <= set(names)
        plain = {k: raw(cn, k, 0, n) for k in names}
        ms = cn.run_profiled(buf, n)
        for k in names:
            assert np.array_equal(raw(cn, k, 0, n), plain[k]), k
        assert ms.shape == (len(cn.low.op_names),) and np.isfinite(ms).all()
        # an op that launches nothing has no time of its own: a block's shortcut conv absorbed by its consumer's generation-12 pick
        absorbed = {int(cn.low.ops[p["op"]][W_X_SCOP]) - 1 for p in cn.plans() if p["batch"] == n and p["gen"] == 12}
        for oi, t in enumerate(ms):
            assert t >= 0.0 if oi in absorbed else t > 0.0, (oi, cn.low.op_names[oi], float(t))
    finally:
        cn.close()


# ---- 6. one IResNet-50 net under the committed plan, at the batches production uses -----------------------------------------------------------

def test_iresnet50_committed_plan_batch_sequence(ctx, monkeypatch):
    """max_batch 192; row counts 192, 64, 37, 128, 1, 128 on prefixes of one set of crops (crops 36, 63 and 127 repeat crop 0).  Poison and
    guard check around every partial run, duplicates bit-equal within a run, the two 128-row runs bit-equal, every row finite, the batch-128
    picks are the plan file's (the kernels bench.py's headline times), and the fp32 oracle at 1 - cosine < 1e-3, unit components within 1e-3."""
    from conftest import ROOT
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet
    plan = os.path.join(ROOT, "plans", "mi355x.plan")
    monkeypatch.delenv("FID_PLAN", raising=False)
    monkeypatch.delenv("FID_AUTOTUNE", raising=False)
    monkeypatch.setenv("FID_PLAN_RO", plan)
    net = archs.iresnet50()
    P = archs.synth_params(net, 0)
    M = 192
    crops = np.random.default_rng(192).integers(0, 256, (M, 112, 112, 3), dtype=np.uint8)
    for d in (36, 63, 127):
        crops[d] = crops[0]
    cn = CompiledNet(ctx, net, P, max_batch=M)
    try:
        if cn.load_plan(plan) == 0:
            pytest.skip("plans/mi355x.plan holds no picks for this device / library revision")
        file_picks = {}
        for line in open(plan):
            parts = line.rstrip("\n").split("|")
            if len(parts) == 5:
                file_picks[tuple(parts[:4])] = parts[4].split()[:6]           # later lines win, as in plan_load
        out = net.outputs[0]
        oracle_rows = sorted(set(range(37)) | {63, 64, 127})
        uniq = [i for i in oracle_rows if i not in (36, 63, 127)]                  # computed once; the copies of crop 0 share its row
        r = onets.run_net(net, P, align.blob_from_images(list(crops[uniq]), net.in_scale, net.in_mean))[out].reshape(len(uniq), -1)
        ref = {i: r[k] for k, i in enumerate(uniq)}
        for d in (36, 63, 127):
            ref[d] = ref[0]
        buf = ctx.to_device(np.full((M, 112, 112, 3), 255, np.uint8))
        runs = {}
        for k, b in enumerate((192, 64, 37, 128, 1, 128)):
            guard = SlotGuard(ctx, cn, b, ("max", "nan")[k % 2]).poison() if b < M else None
            run_rows(cn, buf, crops[:b])
            if guard:
                guard.check(f"IResNet-50: {b} rows of {M}")
            bits = raw(cn, out, 0, b).reshape(b, -1)
            e = cn.read(out, b).reshape(b, -1)
            assert np.isfinite(e).all(), b
            for d in (36, 63, 127):
                if d < b:
                    assert np.array_equal(bits[d], bits[0]), (b, d)
            if b == 128:
                if 128 in runs:
                    assert np.array_equal(bits, runs[128])
                runs[128] = bits
                mine = [l.rstrip("\n").split("|") for l in _saved_lines(cn)]
                mine = [p for p in mine if len(p) == 5 and p[3] == "128"]
                assert len(mine) >= 40, len(mine)
                for p in mine:
                    assert file_picks.get(tuple(p[:4])) == p[4].split()[:6], p
            for i in {37: range(37), 64: (0, 36, 63), 128: (0, 36, 63, 64, 127)}.get(b, ()):
                assert 1 - float(ref[i] @ e[i] / np.linalg.norm(ref[i]) / np.linalg.norm(e[i])) < 1e-3, (b, i)
                assert np.abs(ref[i] / np.linalg.norm(ref[i]) - e[i] / np.linalg.norm(e[i])).max() < 1e-3, (b, i)
    finally:
        cn.close()


def _saved_lines(cn):
    import tempfile
    fd, path = tempfile.mkstemp(suffix=".plan")
    os.close(fd)
    try:
        cn.save_plan(path)
        return open(path).read().splitlines()
    finally:
        os.unlink(path)


# ---- the table: which family really ran where ----------------------------------------------------------------------------------------------

def test_every_family_ran_at_partial_shrinking_and_sub_batches(capsys):
    if not all(RAN[1][k] for k in KINDS):                    # (generation 1 takes a layer of every stack: its row is empty only where a part was deselected)
        pytest.skip("the family tests of this module did not all run in this session (a -k subset): the table needs parts 1, 2 and 4")
    with capsys.disabled():
        print("\ngeneration code -> (stack, batch) the forced family ran at")
        for c in CODES:
            for kind in KINDS:
                print(f"  {c:>3} {kind:<9} " + (" ".join(f"{s}@{b}" for s, b in RAN[c][kind]) or "-"))
    for c in CODES:
        for kind in KINDS:
            assert RAN[c][kind], f"generation code {c} ran at no {kind} batch of any stack"
