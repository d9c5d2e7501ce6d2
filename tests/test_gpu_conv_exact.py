"""GPU: every conv kernel variant and fused op against the exact reference of tests/exact_probe.py, bit for bit.

The probe nets hold small integers times powers of two (exact_probe.int_params), so the fp32 accumulator of every kernel holds the same exact
number whatever its summation order, and the stored fp16 value is the round-to-nearest-even of it: plain equality, no tolerance anywhere in this
module.  tests/test_exact_probe_cpu.py asserts the conditions of that on every probe net.  Every net runs twice and both runs must agree (the
fused block alternates its walking direction).  The op's INPUT tensor is read back and compared first: a mismatch there is a finding about the
layer in front, not about the probed variant.

The lowerings that only exist with a BatchNorm node are covered by the probes of exact_probe.BN_KEYS (BatchNorm with a zero running mean:
power-of-two scales, integer shifts): the nine border-class bias rows of a conv behind a BatchNorm through every kernel family, IResNet's "ir"
form of the fused block, the first block of a stage with its BatchNorms, the fused stem block with a BatchNorm on its second conv.
test_exact_probe_cpu.py::test_bn_probe_lowers_to_ideal_constants shows that the device receives the constants the reference assumes.  Nonzero
running means stay with the tolerance tests."""
import numpy as np
import pytest

import exact_probe as ep
from scrfd_arcface_facerecognition_amd.lower import OP_CONV, W_TYPE, W_X_DST2
from family_helpers import FAMILIES, force_family, forced_ran, own_data_tensors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import Context
    c = Context(0)
    yield c
    c.close()


def run_probe(ctx, key, code=None, check_low=None):
    """build the probe net, run it twice, compare every read-back tensor with the exact reference (inputs of the probed ops first) and the two
    runs with each other.  Returns the names of the ops the forced variant `code` ran."""
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet
    probe = ep.PROBES[key]()
    ref, _ = ep.cached_reference(key)
    fp32 = {n.name for n in probe.net.nodes if n.kind == "fc"}      # an fp32 tensor [B, 1, 1, cout] of exact sums: equal values, no rounding to compare

    def same(got, want, what, nm):
        if nm in fp32:
            ep.assert_same_values(got.reshape(np.shape(want)), np.asarray(want, np.float32), what)
        else:
            ep.assert_same_bits(got, want, what)
    cn = CompiledNet(ctx, probe.net, probe.P, max_batch=probe.batch)
    try:
        if check_low is not None:
            check_low(cn.low)
        names = [n.name for n in probe.net.nodes if n.name in cn.low.tensor_id and n.name in own_data_tensors(cn.low)]
        assert set(probe.probed) <= set(names) and set(probe.net.outputs) <= set(names), (names, probe.net.outputs)
        cn.run(probe.images)
        first = {nm: cn.read(nm, probe.batch) for nm in names}
        cn.run(probe.images)
        second = {nm: cn.read(nm, probe.batch) for nm in names}
        extra = {nm: cn.read(nm, probe.batch) for nm in cn.low.tensor_id if nm.endswith(".even")}
        ran = forced_ran(cn, code) if code is not None else []
    finally:
        cn.close()
    for nm in names:                                         # in graph order: the first mismatch names the layer at fault
        same(first[nm], ref[nm], f"{key} / {nm}" + (" (an INPUT of the probed op: the layer in front)" if nm not in probe.probed else ""), nm)
    for nm, got in extra.items():                            # the fused stem block's compact copy: its first conv's map at the even pixels
        ep.assert_same_bits(got, ref[nm[:-5]][:, ::2, ::2], f"{key} / {nm}")
    for nm in names:
        same(second[nm], first[nm], f"{key} / {nm}: second run against the first", nm)
    return ran


def _shape_id(sh):
    return f"{sh[0][0]}x{sh[0][1]}-{sh[1]}-{sh[2]}x{sh[3]}"


# every row of FAMILIES on the smallest ragged shapes of the family tests, both forms (c: cin -> cout, PReLU; r: cin -> cin, ReLU, + input) in
# one net.  Equality holds whichever variant took a layer, so it is asserted before the case decides whether the forced variant ran at all.
@pytest.mark.parametrize("code", [c for c in sorted(FAMILIES) if c != 10])
@pytest.mark.parametrize("shape", ep.FAMILY_SHAPES, ids=_shape_id)
def test_conv_family_exact(ctx, monkeypatch, code, shape):
    force_family(monkeypatch, code)
    ran = run_probe(ctx, ep.FAMILY_KEYS[shape], code)
    if not set(ran) & {"c", "r"}:
        pytest.skip(f"family code {code} takes neither form of this conv")


# 7x7 maps: conv_ks packs four images into one tile (MOSAIC); nine images = two full tiles and one image
@pytest.mark.parametrize("code", [96, 97, 11])
@pytest.mark.parametrize("shape", ep.MOSAIC_SHAPES, ids=_shape_id)
def test_conv_mosaic_exact(ctx, monkeypatch, code, shape):
    force_family(monkeypatch, code)
    ran = run_probe(ctx, ep.FAMILY_KEYS[shape], code)
    if not set(ran) & {"c", "r"}:
        pytest.skip(f"family code {code} takes neither form of this conv")


# stride 2: c (PReLU) and r (ReLU, + a 1x1 / stride-2 conv of the input)
@pytest.mark.parametrize("code", [10, 1, 2, 11])
@pytest.mark.parametrize("shape", ep.STRIDE2_SHAPES, ids=_shape_id)
def test_conv_stride2_exact(ctx, monkeypatch, code, shape):
    force_family(monkeypatch, code)
    ran = run_probe(ctx, ep.STRIDE2_KEYS[shape], code)
    if not set(ran) & {"c", "r"}:
        pytest.skip(f"family code {code} takes neither form of this stride-2 conv")


# ---- a BatchNorm in front: nine border-class bias rows, the class decoded from each family's own tile coordinates ------------------------
# c: BN - conv - BN - PReLU, r: BN - conv - BN + input.  The family shapes, a 3x5 map (13 of 15 pixels on the border, seven images side by side on
# a STRIP tile) and the 7x7 MOSAIC shape (the edges of four images inside one tile).

BN_RAN = {}               # (family code, shape) -> the border-class convs of the probe the forced variant ran


def _family_bn(ctx, monkeypatch, code, shape):
    from scrfd_arcface_facerecognition_amd import lower
    if (code, shape) not in BN_RAN:
        force_family(monkeypatch, code)

        def low_ok(low):
            flags = {nm: (int(r[lower.W_TYPE]), int(r[lower.W_FLAGS]) & lower.CF_BORDER) for nm, r in zip(low.op_names, low.ops)}
            assert flags["c"] == (lower.OP_CONV, lower.CF_BORDER) and flags["r"] == (lower.OP_CONV, lower.CF_BORDER), low.op_names
        ran = run_probe(ctx, ep.FAMILY_BN_KEYS[shape], code, check_low=low_ok)       # equality first, whichever variant took the layers
        BN_RAN[(code, shape)] = sorted(set(ran) & {"c", "r"})
    return BN_RAN[(code, shape)]


BN_CASES = [(c, sh) for c in sorted(FAMILIES) if c != 10 for sh in ep.FAMILY_BN_SHAPES] + [(c, sh) for c in (96, 97, 11) for sh in ep.MOSAIC_SHAPES]


@pytest.mark.parametrize("code,shape", BN_CASES, ids=lambda v: str(v) if isinstance(v, int) else _shape_id(v))
def test_conv_family_bn_exact(ctx, monkeypatch, code, shape):
    if not _family_bn(ctx, monkeypatch, code, shape):
        pytest.skip(f"family code {code} takes neither form of this conv")


# FAMILIES rows the library never gives a border-class conv, and why.  Every other row must have run one at one shape at least.
NEVER_BORDER = {
    10: "conv_s2.hip takes stride-2 convs only; a BatchNorm in front of a padded conv is folded for stride 1 (lower.py fold_conv), and its DUAL form excludes CF_BORDER",
}


def test_every_family_ran_a_border_class_conv(ctx, monkeypatch):
    ran = {}
    for code, shape in BN_CASES:
        ran.setdefault(code, {})[_shape_id(shape)] = _family_bn(ctx, monkeypatch, code, shape)
    for code in sorted(ran):
        print(f"border-class convs run by family code {code} ({FAMILIES[code]['name']}):", {k: v for k, v in ran[code].items() if v} or "none")
    took = {code for code, by_shape in ran.items() if any(by_shape.values())}
    assert set(FAMILIES) - took == set(NEVER_BORDER), sorted(set(FAMILIES) - took)


# ---- fused ops: fused and unfused lowering, each exact against the reference and hence against each other --------------------------------

def _kinds(low):
    return [int(r[W_TYPE]) for r in low.ops]


def _env(monkeypatch, probe_key, **kv):
    """the hooks of one case: the probe's own, then the case's (None unsets)"""
    for k, v in {**ep.PROBES[probe_key]().env, **kv}.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


# a residual BasicBlock as one launch (csrc/conv_bb.hip; "v2": conv_bb2; 32 stored channels: conv_bb32), ReLU forms
@pytest.mark.parametrize("fuse,shape", [(f, sh) for sh in ep.BB_SHAPES for f in (True, "v2", False) if not (f == "v2" and sh[1] <= 32)],
                         ids=lambda v: v if isinstance(v, str) else (str(v) if isinstance(v, bool) else f"{v[0][0]}x{v[0][1]}-{v[1]}x{v[2]}"))
def test_fused_basic_block_exact(ctx, monkeypatch, fuse, shape):
    from scrfd_arcface_facerecognition_amd import lower
    key = ep.BB_KEYS[shape]
    _env(monkeypatch, key, FID_NO_BB_FUSE=None if fuse else "1", FID_BB_V="2" if fuse == "v2" else None)

    def low_ok(low):
        assert (_kinds(low).count(lower.OP_BBLOCK) == 1) == bool(fuse) and (len(low.ops) == 2) == bool(fuse), low.op_names
    run_probe(ctx, key, check_low=low_ok)


# IResNet's form of the block (BN - conv - BN - PReLU - conv - BN, + input; arcface_r50's stride-1 blocks on 64 channels): conv1's bias row by border class
@pytest.mark.parametrize("fuse,shape", [(f, sh) for sh in ep.IR_SHAPES for f in (True, "v2", False)],
                         ids=lambda v: v if isinstance(v, str) else (str(v) if isinstance(v, bool) else f"{v[0][0]}x{v[0][1]}-{v[1]}x{v[2]}"))
def test_fused_ir_block_exact(ctx, monkeypatch, fuse, shape):
    from scrfd_arcface_facerecognition_amd import lower
    key = ep.IR_KEYS[shape]
    _env(monkeypatch, key, FID_NO_BB_FUSE=None if fuse else "1", FID_BB_V="2" if fuse == "v2" else None)

    def low_ok(low):
        assert (_kinds(low).count(lower.OP_BBLOCK) == 1) == bool(fuse) and (len(low.ops) == 2) == bool(fuse), low.op_names
        op = low.ops[low.op_names.index("b.conv2" if fuse else "b.conv1")]
        assert int(op[lower.W_TYPE]) == (lower.OP_BBLOCK if fuse else lower.OP_CONV) and int(op[lower.W_FLAGS]) & lower.CF_BORDER, low.op_names
    run_probe(ctx, key, check_low=low_ok)


# MobileFaceNet's bottleneck as one launch (csrc/mbf_block.hip): tiled with a residual, stride 2 on a ragged map, whole 14 x 14 maps with 512 expanded channels
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("shape", ep.MBF_SHAPES, ids=lambda v: f"{v[0][0]}x{v[0][1]}-{v[1]}-{v[2]}-{v[3]}s{v[4]}x{v[7]}")
def test_fused_bottleneck_exact(ctx, monkeypatch, fuse, shape):
    from scrfd_arcface_facerecognition_amd import lower
    key = ep.MBF_KEYS[shape]
    _env(monkeypatch, key, FID_NO_MBF_FUSE=None if fuse else "1")

    def low_ok(low):
        assert (_kinds(low).count(lower.OP_MBBLOCK) == 1) == fuse and (_kinds(low).count(lower.OP_DWCONV) == 0) == fuse, low.op_names
    run_probe(ctx, key, check_low=low_ok)


# depthwise 3x3 + pointwise 1x1 as one launch (csrc/dwpw.hip, opt-in)
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("shape", ep.DWPW_SHAPES, ids=lambda v: f"{v[0][0]}x{v[0][1]}-{v[1]}-{v[2]}s{v[3]}x{v[5]}")
def test_fused_depthwise_pointwise_exact(ctx, monkeypatch, fuse, shape):
    from scrfd_arcface_facerecognition_amd import lower
    key = ep.DWPW_KEYS[shape]
    _env(monkeypatch, key, FID_DWPW_FUSE="1" if fuse else None)

    def low_ok(low):
        assert (_kinds(low).count(lower.OP_DWPW) == 1) == fuse and (_kinds(low).count(lower.OP_DWCONV) == 0) == fuse, low.op_names
    run_probe(ctx, key, check_low=low_ok)


# a PAFPN level as one launch (csrc/lat_fpn.hip): three levels, the laterals a finer level adds are stored and compared as well
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("shape", ep.LATFPN_SHAPES, ids=lambda v: f"{v[0][0]}x{v[0][1]}x{v[1]}")
def test_fused_lateral_fpn_exact(ctx, monkeypatch, fuse, shape):
    from scrfd_arcface_facerecognition_amd import lower
    key = ep.LATFPN_KEYS[shape]
    _env(monkeypatch, key, FID_NO_LATFPN_FUSE=None if fuse else "1")

    def low_ok(low):
        assert _kinds(low).count(lower.OP_LATFPN) == (3 if fuse else 0), low.op_names
        if fuse:
            assert "lat0" not in low.tensor_id and "lat1" in low.tensor_id and "lat2" in low.tensor_id
    run_probe(ctx, key, check_low=low_ok)


# IResNet's stem + the 3x3 conv on it as one launch (csrc/stem_block.hip), the forms without a BatchNorm; the shortcut reads the compact even-pixel copy
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("shape", ep.STEM_SHAPES, ids=lambda v: f"{v[0][0]}x{v[0][1]}-{v[1]}x{v[2]}")
def test_fused_stem_block_exact(ctx, monkeypatch, fuse, shape):
    from scrfd_arcface_facerecognition_amd import lower
    key = ep.STEM_KEYS[shape]
    _env(monkeypatch, key, FID_NO_STEMBLOCK_FUSE=None if fuse else "1")

    def low_ok(low):
        assert (int(low.ops[0][lower.W_TYPE]) == lower.OP_STEMBLOCK) == fuse and ("stem.even" in low.tensor_id) == fuse and ("stem" in low.tensor_id) != fuse
    run_probe(ctx, key, check_low=low_ok)


# the same with IResNet's BatchNorms: nine bias rows for the conv on the stem's map, in the fused op or in the conv of its own
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("shape", ep.STEM_SHAPES, ids=lambda v: f"{v[0][0]}x{v[0][1]}-{v[1]}x{v[2]}")
def test_fused_stem_block_bn_exact(ctx, monkeypatch, fuse, shape):
    from scrfd_arcface_facerecognition_amd import lower
    key = ep.STEM_BN_KEYS[shape]
    _env(monkeypatch, key, FID_NO_STEMBLOCK_FUSE=None if fuse else "1")

    def low_ok(low):
        assert (int(low.ops[0][lower.W_TYPE]) == lower.OP_STEMBLOCK) == fuse and ("stem.even" in low.tensor_id) == fuse and ("stem" in low.tensor_id) != fuse
        op = low.ops[low.op_names.index("b.conv1")]
        assert int(op[lower.W_TYPE]) == (lower.OP_STEMBLOCK if fuse else lower.OP_CONV) and int(op[lower.W_FLAGS]) & lower.CF_BORDER, low.op_names
    run_probe(ctx, key, check_low=low_ok)


# the block shortcut (2x2 average pool + 1x1 conv, the weights become quarters) in the stride-2 conv's launch (conv_s2.hip DUAL)
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("shape", ep.DUAL_SHAPES, ids=lambda v: f"{v[0][0]}x{v[0][1]}-{v[1]}x{v[2]}")
def test_fused_shortcut_stride2_exact(ctx, monkeypatch, fuse, shape):
    key = ep.DUAL_KEYS[shape]
    _env(monkeypatch, key, FID_NO_DOWN_FUSE=None if fuse else "1")

    def low_ok(low):
        assert (len(low.ops) == 2) == fuse and any(int(r[W_X_DST2]) > 0 for r in low.ops if int(r[W_TYPE]) == OP_CONV) == fuse, low.op_names
    run_probe(ctx, key, check_low=low_ok)


# the 1x1 / stride-2 shortcut conv as extra K-steps of the conv that adds it (a generation-12 pick; "fused_s2": inside conv_s2.hip, ns = 10): first without the
# BatchNorms of IResNet's block, then with them.  Three runs: the first one tunes with the shortcut as its own op.
SHORTCUT_CASES = dict(argvalues=[("fused", ep.SHORTCUT_SHAPES[0]), ("fused", ep.SHORTCUT_SHAPES[1]), ("fused_s2", ep.SHORTCUT_SHAPES[1]),
                                 ("plain", ep.SHORTCUT_SHAPES[0]), ("plain", ep.SHORTCUT_SHAPES[1])],
                      ids=lambda v: v if isinstance(v, str) else f"{v[0][0]}x{v[0][1]}-{v[1]}-{v[2]}x{v[3]}")


@pytest.mark.parametrize("mode,shape", **SHORTCUT_CASES)
def test_fused_shortcut_conv_exact(ctx, monkeypatch, mode, shape):
    _shortcut_case(ctx, monkeypatch, ep.SHORTCUT_KEYS[shape], mode, border=False)


# the block in its real form: a BatchNorm behind the shortcut and behind both convs, one in front of conv1 (nine bias rows)
@pytest.mark.parametrize("mode,shape", **SHORTCUT_CASES)
def test_fused_shortcut_conv_bn_exact(ctx, monkeypatch, mode, shape):
    _shortcut_case(ctx, monkeypatch, ep.SHORTCUT_BN_KEYS[shape], mode, border=True)


def _shortcut_case(ctx, monkeypatch, key, mode, border):
    from scrfd_arcface_facerecognition_amd import lower
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet
    _env(monkeypatch, key, FID_NO_SC_FUSE="1" if mode == "plain" else None, FID_FORCE_GEN=None if mode == "plain" else "12",
         FID_FORCE_NS="10" if mode == "fused_s2" else None)
    probe = ep.PROBES[key]()
    ref, _ = ep.cached_reference(key)
    cn = CompiledNet(ctx, probe.net, probe.P, max_batch=probe.batch)
    try:
        assert (sum(int(r[lower.W_TYPE]) == lower.OP_CONV and int(r[lower.W_X_SRC2]) > 0 for r in cn.low.ops) == 1) == (mode != "plain")
        assert bool(int(cn.low.ops[cn.low.op_names.index("b.conv1")][lower.W_FLAGS]) & lower.CF_BORDER) == border
        names = [nm for nm in probe.net.outputs if nm in own_data_tensors(cn.low)]
        assert names == probe.net.outputs
        got = []
        for _ in range(3):
            cn.run(probe.images)
            got.append({nm: cn.read(nm, probe.batch) for nm in names})
        picks = {p["name"]: (p["gen"], p["ns"]) for p in cn.plans()}
    finally:
        cn.close()
    assert (picks["b.conv2"][0] == 12) == (mode != "plain"), picks
    assert mode != "fused_s2" or picks["b.conv2"][1] == 10, picks
    for g in got:
        for nm in names:
            ep.assert_same_bits(g[nm], ref[nm], f"{key} / {nm} ({mode}, pick {picks['b.conv2']})")


# a depthwise 3x3 layer of its own: the LDS-tiled kernel (from 50 000 pixels per launch; ragged tiles in both directions) and the plain one
@pytest.mark.parametrize("shape", ep.DW_SHAPES, ids=lambda v: f"{v[0][0]}x{v[0][1]}x{v[1]}")
def test_depthwise_exact(ctx, shape):
    from scrfd_arcface_facerecognition_amd import lower

    def low_ok(low):
        assert _kinds(low).count(lower.OP_DWCONV) == 1, low.op_names
    run_probe(ctx, ep.DW_KEYS[shape], check_low=low_ok)


# the detector head conv through every family that takes it: the fp32 bbox and kps channels (bbox.scale = 1) are exact sums.  The sigmoid scores
# are not compared here: they keep the 2e-3 of test_gpu_conv_families.py::test_dethead_family.
@pytest.mark.parametrize("code", [0, 1, 2, 5])
@pytest.mark.parametrize("shape", ep.DETHEAD_SHAPES, ids=lambda v: f"{v[0][0]}x{v[0][1]}-{v[1]}x{v[2]}")
def test_dethead_exact(ctx, monkeypatch, code, shape):
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet
    force_family(monkeypatch, code)
    key = ep.DETHEAD_KEYS[shape]
    probe = ep.PROBES[key]()
    ref, _ = ep.cached_reference(key)
    x, B = probe.net.outputs[0], probe.batch
    cn = CompiledNet(ctx, probe.net, probe.P, max_batch=B)
    try:
        assert {x, "h"} <= set(own_data_tensors(cn.low))
        runs = []
        for _ in range(2):
            cn.run(probe.images)
            runs.append((cn.read(x, B), cn.read("h", B)))                # h: [B, H, W, 30] = cls (2), bbox (8), kps (20)
        ran = forced_ran(cn, code)
    finally:
        cn.close()
    _, bb, kp = ref["h"]
    for gx, gh in runs:
        ep.assert_same_bits(gx, ref[x], f"{key} / {x} (the INPUT of the head conv)")
        ep.assert_same_values(gh[..., 2:10].reshape(B, -1, 4), bb.astype(np.float32), f"{key} / bbox")
        ep.assert_same_values(gh[..., 10:30].reshape(B, -1, 10), kp.astype(np.float32), f"{key} / kps")
    if "h" not in ran:
        pytest.skip(f"family code {code} does not take the head conv")
