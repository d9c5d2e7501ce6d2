"""The exact probes of tests/exact_probe.py, on the reference alone (no GPU): every probe net of test_gpu_conv_exact.py meets the conditions under
which a bit-for-bit comparison is valid and has power; fp32 accumulation of the probed convs does not depend on the summation order; the
comparator sees three planted faults on every probe net; ReLU before and after the fp16 rounding give the same bits.  The probes with
BatchNorm (exact_probe.BN_KEYS): a wrong border class shows at every border pixel, and lowering them yields the constants of the ideal affine
byte for byte, which is what lets the GPU module compare them without a tolerance."""
import dataclasses

import numpy as np
import pytest

import exact_probe as ep

KEYS = sorted(ep.PROBES)
CONV_KEYS = [k for k in KEYS if ep.PROBES[k]().probed]      # (the detector head probes store fp32: no rounding to plant a fault in)


def _probed(key):
    probe = ep.PROBES[key]()
    ref, raw = ep.cached_reference(key)
    return probe, ref, raw, [n for n in probe.net.nodes if n.name in probe.probed]


@pytest.mark.parametrize("key", KEYS)
def test_probe_conditions(key):
    probe, ref, raw, nodes = _probed(key)
    stats = ep.check_exactness(probe.net, probe.P, probe.images, probe.probed, probe.onchip, ref, raw)
    assert set(probe.probed) | set(probe.onchip) <= set(stats) and len(stats) > 0
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
    kinds = [int(r[0]) for r in real.ops]
    if key in ep.FAMILY_BN_KEYS.values():
        want = {"c": lower.OP_CONV, "r": lower.OP_CONV}
    elif key in ep.IR_KEYS.values():
        want = {"b.conv2": lower.OP_BBLOCK}
        assert len(real.ops) == 2 and "b.conv1" not in real.tensor_id
    elif key in ep.SHORTCUT_BN_KEYS.values():
        want = {"b.conv1": lower.OP_CONV}
        assert int(ops["b.conv2"][23]) > 0 and not int(ops["b.conv2"][11]) & lower.CF_BORDER        # (the shortcut's second weight image)
    else:
        want = {"b.conv1": lower.OP_STEMBLOCK}
        assert kinds[0] == lower.OP_STEMBLOCK and "stem.even" in real.tensor_id and "stem" not in real.tensor_id
    for nm, kind in want.items():
        assert int(ops[nm][0]) == kind and int(ops[nm][11]) & lower.CF_BORDER, (key, nm, real.op_names)
    assert sum(bool(int(r[11]) & lower.CF_BORDER) for r in real.ops) == len(want)


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
