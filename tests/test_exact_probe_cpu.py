"""The exact probes of tests/exact_probe.py, on the reference alone (no GPU): every probe net of test_gpu_conv_exact.py meets the conditions under
which a bit-for-bit comparison is valid and has power; fp32 accumulation of the probed convs does not depend on the summation order; the
comparator sees three planted faults on every probe net; ReLU before and after the fp16 rounding give the same bits.  The probes with
BatchNorm (exact_probe.BN_KEYS): a wrong border class shows at every border pixel, and lowering them yields the constants of the ideal affine
byte for byte, which is what lets the GPU module compare them without a tolerance."""
import dataclasses
import os

import numpy as np
import pytest

import exact_probe as ep

KEYS = sorted(ep.PROBES)


def _held(probe):
    """the conv nodes held to the probed nodes' conditions (an FC or a max pool has its own checks below)"""
    return [n for n in probe.net.nodes if n.name in probe.probed + probe.through and n.kind == "conv"]


CONV_KEYS = [k for k in KEYS if _held(ep.PROBES[k]())]      # (the detector head and FC probes store fp32: no rounding to plant a fault in)


def _probed(key):
    probe = ep.PROBES[key]()
    ref, raw = ep.cached_reference(key)
    return probe, ref, raw, _held(probe)


@pytest.mark.parametrize("key", KEYS)
def test_probe_conditions(key):
    probe, ref, raw, nodes = _probed(key)
    stats = ep.check_exactness(probe.net, probe.P, probe.images, probe.probed + probe.through, probe.onchip, ref, raw)
    assert set(probe.probed) | set(probe.through) | set(probe.onchip) <= set(stats) and len(stats) > 0
    for n in nodes:                                          # the one-node evaluator the checks below plant their faults in IS the reference
        ep.assert_same_bits(ep.eval_node(n, ref, probe.P), ref[n.name], f"{key} / {n.name}")


@pytest.mark.parametrize("key", CONV_KEYS)
def test_fp32_sum_is_order_independent(key):
    probe, ref, raw, nodes = _probed(key)
    for n in nodes:
        fwd, rev = ep.eval_node(n, ref, probe.P, "f32_fwd"), ep.eval_node(n, ref, probe.P, "f32_rev")
        assert fwd.dtype == np.float32 and rev.dtype == np.float32
        assert np.array_equal(fwd.view(np.uint32), rev.view(np.uint32)), (key, n.name)
        assert np.array_equal(fwd.astype(np.float64), raw[n.name]), (key, n.name)


@pytest.mark.parametrize("fault", ["fault_tap", "fault_f16acc", "fault_rtz"])
@pytest.mark.parametrize("key", CONV_KEYS)
def test_comparator_sees_planted_fault(key, fault):
    probe, ref, raw, nodes = _probed(key)
    for n in nodes:
        bad = ep.eval_node(n, ref, probe.P, fault)
        with pytest.raises(AssertionError, match="values differ"):
            ep.assert_same_bits(bad, ref[n.name], f"{key} / {n.name}")
        if fault == "fault_tap":                             # one pixel of one image, and the report names it
            assert {tuple(i[:3]) for i in np.argwhere(bad != ref[n.name])} == {(0, 0, 0)}


@pytest.mark.parametrize("key", CONV_KEYS)
def test_relu_commutes_with_the_rounding(key):
    """epilogue.h applies ReLU after the fp16 rounding in some bodies: the same bits, sign of zero included"""
    probe, ref, raw, nodes = _probed(key)
    seen = False
    for n in nodes:
        if n.act != "relu":
            continue
        v = ep.eval_node(dataclasses.replace(n, act="none"), ref, probe.P, rounded=False)
        assert (v < 0).any() and (v > 0).any()
        before = np.maximum(v, 0.0).astype(np.float16)
        after = np.maximum(v.astype(np.float16), np.float16(0))
        assert np.array_equal(before.view(np.uint16), after.view(np.uint16)), (key, n.name)
        ep.assert_same_bits(before, ref[n.name], f"{key} / {n.name}")
        seen = True
    if not seen:
        assert all(n.act != "relu" for n in nodes)


def _border_nodes(probe):
    return [n for n in probe.net.nodes if n.kind == "conv" and n.pre_bn and n.pad == 1]


@pytest.mark.parametrize("key", ep.BN_KEYS)
def test_border_rows_tell_the_classes_apart(key):
    """the new condition of a border-class node, on every such node of the probe (probed, kept on chip or only read back)"""
    probe, ref, raw, _ = _probed(key)
    stats = ep.check_exactness(probe.net, probe.P, probe.images, probe.probed, probe.onchip, ref, raw)
    nodes = _border_nodes(probe)
    assert nodes and {n.name for n in nodes} & (set(probe.probed) | set(probe.onchip) | set(probe.net.outputs))
    for n in nodes:
        w, rows = ep.fold_node(n, probe.P)
        assert rows.shape == (9, n.cout) and ep._is_f16(w).all()
        assert min((rows[i] != rows[j]).mean() for i in range(9) for j in range(i)) >= 0.25
        if n.name in stats:
            assert stats[n.name]["border"]["row_pairs_differ"] >= 0.25 and stats[n.name]["border"]["border_pixels"] > 0
        ep.assert_same_bits(ep.eval_node(n, ref, probe.P), ref[n.name], f"{key} / {n.name}")     # the fold IS the BatchNorm as it stands
        assert set(ep.border_classes(*ref[n.name].shape[1:3]).flatten()) == set(range(9))


@pytest.mark.parametrize("key", ep.BN_KEYS)
def test_comparator_sees_wrong_border_class(key):
    probe, ref, raw, _ = _probed(key)
    for n in _border_nodes(probe):
        B, H, W, _ = ref[n.name].shape
        bad = ep.eval_node(n, ref, probe.P, "fault_border")                        # the interior row everywhere: border pixels only, and all of them
        with pytest.raises(AssertionError, match="values differ"):
            ep.assert_same_bits(bad, ref[n.name], f"{key} / {n.name}")
        border = {(i, y, x) for i in range(B) for y in range(H) for x in range(W) if y in (0, H - 1) or x in (0, W - 1)}
        assert {tuple(i[:3]) for i in np.argwhere(bad != ref[n.name])} == border
        bad = ep.eval_node(n, ref, probe.P, "fault_class")                         # one pixel of the last image, and the report names it
        assert {tuple(i[:3]) for i in np.argwhere(bad != ref[n.name])} == {(B - 1, 0, 0)}
        with pytest.raises(AssertionError, match=rf"values differ; first \(n={B - 1}, y=0, x=0, c=\d+\)"):
            ep.assert_same_bits(bad, ref[n.name], f"{key} / {n.name}")


def test_border_classes():
    assert ep.border_classes(3, 5).tolist() == [[0, 1, 1, 1, 2], [3, 4, 4, 4, 5], [6, 7, 7, 7, 8]]
    assert ep.border_classes(2, 2).tolist() == [[0, 2], [6, 8]]


@pytest.mark.parametrize("key", ep.BN_KEYS)
def test_bn_probe_lowers_to_ideal_constants(key, monkeypatch):
    """lower() with BatchNorm as it stands (gamma / sqrt(var + eps)) and with the ideal affine (gamma, beta) in its place: the same blob, byte
    for byte -- the fp16 weights and fp32 bias rows the device receives are the ones the exact reference assumes.  And the lowering is the
    one the probe is meant to hit."""
    from scrfd_arcface_facerecognition_amd import lower
    for k in ("FID_NO_BB_FUSE", "FID_NO_STEMBLOCK_FUSE", "FID_NO_SC_FUSE", "FID_NO_STEM_FUSE"):
        monkeypatch.delenv(k, raising=False)
    probe = ep.PROBES[key]()
    a, _ = lower._bn_affine(probe.P, next(k[:-6] for k in probe.P if k.endswith(".gamma")))
    assert (a != np.round(a * 4) / 4).any()                  # (the scale as it stands is NOT a power of two)
    real = lower.lower(probe.net, probe.P)
    monkeypatch.setattr(lower, "_bn_affine", ep.ideal_affine)
    ideal = lower.lower(probe.net, probe.P)
    assert len(real.blob) == len(ideal.blob) > 0
    diff = np.flatnonzero(np.frombuffer(real.blob, np.uint8) != np.frombuffer(ideal.blob, np.uint8))
    assert diff.size == 0, (key, f"{diff.size} bytes differ, first at {diff[:4].tolist()}")
    assert np.array_equal(real.ops, ideal.ops)
    ops = {nm: r for nm, r in zip(real.op_names, real.ops)}
    kinds = [int(r[lower.W_TYPE]) for r in real.ops]
    if key in ep.FAMILY_BN_KEYS.values():
        want = {"c": lower.OP_CONV, "r": lower.OP_CONV}
    elif key in ep.IR_KEYS.values():
        want = {"b.conv2": lower.OP_BBLOCK}
        assert len(real.ops) == 2 and "b.conv1" not in real.tensor_id
    elif key in ep.SHORTCUT_BN_KEYS.values():
        want = {"b.conv1": lower.OP_CONV}
        assert int(ops["b.conv2"][lower.W_X_SRC2]) > 0 and not int(ops["b.conv2"][lower.W_FLAGS]) & lower.CF_BORDER        # (the shortcut's second weight image)
    else:
        want = {"b.conv1": lower.OP_STEMBLOCK}
        assert kinds[0] == lower.OP_STEMBLOCK and "stem.even" in real.tensor_id and "stem" not in real.tensor_id
    for nm, kind in want.items():
        assert int(ops[nm][lower.W_TYPE]) == kind and int(ops[nm][lower.W_FLAGS]) & lower.CF_BORDER, (key, nm, real.op_names)
    assert sum(bool(int(r[lower.W_FLAGS]) & lower.CF_BORDER) for r in real.ops) == len(want)


def test_comparator_details():
    a = np.zeros((1, 2, 2, 4), np.float32)
    b = a.copy()
    b[0, 1, 0, 3] = -0.0
    ep.assert_same_bits(a, b)                               # +0 == -0
    b[0, 1, 0, 3] = np.float32(2.0 ** -14)
    with pytest.raises(AssertionError, match=r"1 of 16 values differ; first \(n=0, y=1, x=0, c=3\): got 0x0000 ref 0x0400; difference in fp16 ulps \{-1024: 1\}"):
        ep.assert_same_bits(a, b)
    b[0, 1, 0, 3] = np.inf
    with pytest.raises(AssertionError, match="not finite"):
        ep.assert_same_bits(a, b)
    with pytest.raises(AssertionError, match="not fp16 values"):
        ep.assert_same_bits(a, a + np.float32(1e-9))


def test_lsb_tracking():
    assert ep.lsb_of([3.0, -6.0, 0.0]) == 1.0 and ep.lsb_of([0.75, 4.0]) == 0.25 and ep.lsb_of([48.0]) == 16.0 and ep.lsb_of([0.0]) == 1.0


# ---- split-K, FC, the fused detector stem, the first conv, max pool and GDC (tests/test_gpu_ops_exact.py) ------------------------------------

from test_conv_variants_cpu import HIPCC, LIB, driver, run      # noqa: E402,F401  (the host-only driver of the library's dispatch functions)

needs_driver = pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(LIB)), reason="needs hipcc and the built libfaceid.so")


@needs_driver
@pytest.mark.parametrize("force", [None, "128,64,2", "64,64,9", "128,128,4", "128,64,7", "128,96,5", "128,32,3"])
def test_split_mirror_is_conv_plan(driver, force):
    """exact_probe.split_mirror against the library's conv_plan (the driver's "h1" / "h0" lines: the heuristic pick with and without split-K at
    256 CUs) on every plain shape of the driver's grid, with and without FID_CONV_FORCE"""
    lines = run(driver, ["grid", "-v"], {"FID_CONV_FORCE": force} if force else {})
    f = tuple(int(v) for v in force.split(",")) if force else None
    seen = split = 0
    for i, line in enumerate(lines):
        if not line.startswith("shape "):
            continue
        w = line.split()
        a = dict(zip(w[1::2], (int(v) for v in w[2::2])))
        if a["out2"] or a["T2"]:                             # (the fused shortcut forms take other branches of conv_plan)
            continue
        j = i + 1
        while not lines[j].startswith("h1 "):
            j += 1
        for tag, allow, row in (("h1", True, lines[j]), ("h0", False, lines[j + 1])):
            v = row.split()
            assert v[0] == tag
            gen, bm, bn, bk, ks = (int(x) for x in v[1:6])
            m = ep.split_mirror(a["M"], a["Cin"], a["Cout"], a["k"] * a["k"], 256, f, allow)
            assert (gen, bm, bn, bk, ks) == (2, m["bm"], m["bn"], m["bk"], m["ksplit"]), (line, row, m)
            assert int(v[7]) == (ks * a["M"] * a["Cout"] * 4 if ks > 1 else 0)
            seen += 1
            split += ks > 1
    assert seen > 10000 and split > 1000


SPLIT_IDS = [f"{k}-{f}" for k, _, f, _ in ep.SPLIT_CASES]


def _split_geometry(key, name, monkeypatch):
    from scrfd_arcface_facerecognition_amd import lower
    probe = ep.PROBES[key]()
    low = lower.lower(probe.net, probe.P)
    assert int(low.ops[low.op_names.index(name)][lower.W_TYPE]) == lower.OP_CONV
    return probe, low, ep.conv_geometry(low, name, probe.batch)


@pytest.mark.parametrize("key,names,force,slabs", ep.SPLIT_CASES, ids=SPLIT_IDS)
def test_split_cases_split_as_they_say(key, names, force, slabs, monkeypatch):
    """the slabs every split-K case is about follow from its FID_CONV_FORCE through the mirror (whatever the CU count), the probed ops carry the
    epilogue features the case names, and a dropped K-step, a K-step of the LAST slab, and a bias added once per slab change the reference"""
    from scrfd_arcface_facerecognition_amd import lower
    ref, _ = ep.cached_reference(key)
    for name in names:
        probe, low, (M, cin_p, cout_p, taps) = _split_geometry(key, name, monkeypatch)
        f = tuple(int(v) for v in force.split(",")) if force else None
        for cus in (64, 256, 304):
            m = ep.split_mirror(M, cin_p, cout_p, taps, cus, f)
            assert len(m["slabs"]) > 1 and sum(m["slabs"]) == m["ksteps"] and (slabs is None or m["slabs"] == slabs), (name, cus, m)
        flags = int(low.ops[low.op_names.index(name)][lower.W_FLAGS])
        assert bool(flags & lower.CF_BORDER) == key.startswith("convbn") and bool(flags & lower.CF_RES_UP2) == key.startswith("up2")
        n = next(x for x in probe.net.nodes if x.name == name)
        first_of_last = sum(m["slabs"][:-1])
        for fault, arg in (("fault_kstep", (m["bk"], cin_p, 0)), ("fault_kstep", (m["bk"], cin_p, first_of_last)),
                           ("fault_kstep", (m["bk"], cin_p, m["ksteps"] - 1)), ("fault_bias_slabs", len(m["slabs"]))):
            bad = ep.eval_node(n, ref, probe.P, fault, arg=arg)
            with pytest.raises(AssertionError, match="values differ"):
                ep.assert_same_bits(bad, ref[name], f"{key} / {name}")
            assert (bad != ref[name]).any(axis=(1, 2, 3)).all(), (name, fault, arg)      # in every image
    if key.startswith("conv-40x24"):                         # three 32-channel chunks per tap: some slab begins inside a tap
        assert cin_p == 96 and any(sum(m["slabs"][:i]) % 3 for i in range(1, len(m["slabs"])))


FC_KEYS = sorted(ep.FC_KEYS.values())


@pytest.mark.parametrize("key", FC_KEYS)
def test_fc_probe_faults_and_order(key):
    """the FC reference does not depend on the order of the K-steps in fp32, and the comparator sees a dropped or doubled K-step of any slab, the
    bias added once per slab and CHW-ordered weight columns"""
    probe, ref, raw, _ = _probed(key)
    n = probe.net.nodes[-1]
    y = ref["fc"]
    fwd, rev = ep.eval_fc(n, ref, probe.P, "f32_fwd"), ep.eval_fc(n, ref, probe.P, "f32_rev")
    assert fwd.dtype == np.float32 and np.array_equal(fwd.view(np.uint32), rev.view(np.uint32)) and np.array_equal(fwd.astype(np.float64), y)
    steps = n.h * n.w * ((n.c + 31) // 32 * 32) // ep.fc_bk(n)
    faults = [("fault_kstep", s) for s in range(steps)] + [("fault_kstep_twice", 0), ("fault_kstep_twice", steps - 1), ("fault_bias_slabs", 3)]
    if n.c % 32 == 0:
        faults.append(("chw", None))
    for fault, arg in faults:
        bad = ep.eval_fc(n, ref, probe.P, fault, arg)
        assert (bad != y).any(axis=1).all(), (key, fault, arg)              # in every image
    with pytest.raises(AssertionError, match=r"values differ; first at \(0, \d+\)"):
        ep.assert_same_values(ep.eval_fc(n, ref, probe.P, "fault_kstep", steps - 1).astype(np.float32), y.astype(np.float32), key)


@pytest.mark.parametrize("key", FC_KEYS)
def test_fc_probe_lowers_to_ideal_constants(key, monkeypatch):
    """lower() with the BatchNorms as they stand and with the ideal affines: the same blob byte for byte; the FC is an OP_CONV with an fp32 result
    on a flattened alias of its input, and the weight rows in the blob are fc_columns' (HWC order, zero columns for the padded channels)"""
    from scrfd_arcface_facerecognition_amd import lower
    probe, ref, raw, _ = _probed(key)
    n = probe.net.nodes[-1]
    real = lower.lower(probe.net, probe.P)
    monkeypatch.setattr(lower, "_bn_affine", ep.ideal_affine)
    ideal = lower.lower(probe.net, probe.P)
    assert real.blob == ideal.blob and np.array_equal(real.ops, ideal.ops)
    op = real.ops[real.op_names.index("fc")]
    src, dst = real.tensors[int(op[lower.W_SRC])], real.tensors[int(op[lower.W_DST])]
    _, W, b = ep.fc_columns(n, ref, probe.P)
    K = W.shape[1]
    assert int(op[lower.W_TYPE]) == lower.OP_CONV and int(dst[lower.T_DTYPE]) == 1 and tuple(int(src[w]) for w in (lower.T_C, lower.T_CP, lower.T_H, lower.T_W)) == (K, K, 1, 1)
    got = np.frombuffer(real.blob, np.float16, count=int(op[lower.W_WROWS]) * K, offset=int(op[lower.W_WOFF])).reshape(int(op[lower.W_WROWS]), K)
    assert np.array_equal(got[:n.cout].astype(np.float64), W) and not got[n.cout:].any()
    assert np.array_equal(np.frombuffer(real.blob, np.float32, count=n.cout, offset=int(op[lower.W_BOFF])).astype(np.float64), b)
    assert (ref["b"] < 0).any() and (ref["b"] > 0).any()


@pytest.mark.parametrize("key", sorted(ep.STEMFUSED_KEYS.values()))
def test_fused_stem_probe(key, monkeypatch):
    """lowers to the one fused op (four ops with FID_NO_STEM_FUSE=1); a pooled row taken one row off at the seam of the 8-row and of the 6-row
    tiles changes the reference, and so does a missing K-step of stem.2 (its power conditions: test_probe_conditions)"""
    from scrfd_arcface_facerecognition_amd import lower
    probe, ref, raw, held = _probed(key)
    monkeypatch.delenv("FID_NO_STEM_FUSE", raising=False)
    assert lower.lower(probe.net, probe.P).op_names == ["stem.fused"] and [n.name for n in held] == ["stem.2"]
    monkeypatch.setenv("FID_NO_STEM_FUSE", "1")
    assert [int(r[lower.W_TYPE]) for r in lower.lower(probe.net, probe.P).ops] == [lower.OP_STEM, lower.OP_CONV, lower.OP_CONV, lower.OP_MAXPOOL]
    pool = probe.net.nodes[-1]
    Hp, Wp = ref["stem.pool"].shape[1:3]
    assert Hp % 8 != 0 or Hp % 6 != 0                        # ragged row tiles in one of the two forms at least
    assert Wp % 6 != 0 or Hp == Wp == 16
    for row in (6, 8):
        bad = ep.eval_pool(pool, ref, "fault_row_off", row)
        assert {int(i[1]) for i in np.argwhere(bad != ref["stem.pool"])} == {row}
        with pytest.raises(AssertionError, match=rf"values differ; first \(n=0, y={row}, "):
            ep.assert_same_bits(bad, ref["stem.pool"], key)


@pytest.mark.parametrize("key", sorted(ep.FIRST_KEYS.values()))
def test_first_conv_probe_lowers_to_the_stem_op(key):
    from scrfd_arcface_facerecognition_amd import lower
    probe = ep.PROBES[key]()
    low = lower.lower(probe.net, probe.P)
    n = probe.net.nodes[0]
    assert [int(r[lower.W_TYPE]) for r in low.ops] == [lower.OP_STEM] and int(low.tensors[0][lower.T_CP]) == (n.cout + 31) // 32 * 32 and int(low.ops[0][lower.W_STRIDE]) == n.stride


@pytest.mark.parametrize("key", sorted(ep.POOL_KEYS.values()))
def test_pool_probe_faults(key):
    """zero padding and a pooled row taken one row off change the reference (the window and padding conditions: test_probe_conditions)"""
    from scrfd_arcface_facerecognition_amd import lower
    probe, ref, raw, _ = _probed(key)
    pool = probe.net.nodes[-1]
    low = lower.lower(probe.net, probe.P)
    assert [int(r[lower.W_TYPE]) for r in low.ops] == [lower.OP_STEM, lower.OP_MAXPOOL]
    H, W = ref["s"].shape[1:3]
    Ho, Wo = ref["pool"].shape[1:3]
    assert (Ho, Wo) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1) and (ref["s"] < 0).mean() > 0.3
    bad = ep.eval_pool(pool, ref, "fault_pad0")
    with pytest.raises(AssertionError, match="values differ"):
        ep.assert_same_bits(bad, ref["pool"], key)
    rows = {int(i[1]) for i in np.argwhere(bad != ref["pool"])}
    assert 0 in rows and (H % 2 == 0 or Ho - 1 in rows)      # the first row, and the last one where its window is clipped (odd maps)
    assert (ep.eval_pool(pool, ref, "fault_row_off", Ho // 2) != ref["pool"]).any()


@pytest.mark.parametrize("key", sorted(ep.GDC_KEYS.values()))
def test_gdc_probe(key):
    """lowers to a depthwise op that meets gdc_rows' dispatch condition; dense weights; every kernel row dropped changes every image"""
    from scrfd_arcface_facerecognition_amd import lower
    probe, ref, raw, held = _probed(key)
    low = lower.lower(probe.net, probe.P)
    assert ep.takes_gdc_rows(low, "g") and [n.name for n in held] == ["g"]
    g = held[0]
    assert (probe.P["g.weight"] != 0).all() and ref["g"].shape[1:3] == (1, 1)
    for row in range(g.k):
        bad = ep.eval_node(g, ref, probe.P, "fault_row", arg=row)
        assert (bad != ref["g"]).any(axis=(1, 2, 3)).all(), (key, row)
    with pytest.raises(AssertionError, match="values differ"):
        ep.assert_same_bits(ep.eval_node(g, ref, probe.P, "fault_row", arg=g.k - 1), ref["g"], key)
