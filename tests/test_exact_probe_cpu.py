"""The exact probes of tests/exact_probe.py, on the reference alone (no GPU): every probe net of test_gpu_conv_exact.py meets the conditions under
which a bit-for-bit comparison is valid and has power; fp32 accumulation of the probed convs does not depend on the summation order; the
comparator sees three planted faults on every probe net; ReLU before and after the fp16 rounding give the same bits."""
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
