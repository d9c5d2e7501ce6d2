"""GPU: what the exact probes of test_gpu_conv_exact.py left out, bit for bit against the reference of tests/exact_probe.py.

  split-K     the implicit GEMM's K axis in slabs (csrc/conv.hip: ks_begin / ks_end, the `ksplit > 1` branch of tile_epilogue, splitk_epilogue):
              slabs of 9 + 9, of two steps, a ragged last slab, a request the launcher reduces, slabs that begin inside a tap, border-class
              bias rows, a residual, an up-sampled residual, PReLU, the fp32 output
  FC          IResNet's last op: the heuristic plan's own split and slabs of two or three steps, one image to a second M tile, padded channels
              inside K
  stem.fused  the detector stem in its four fused forms and unfused: five lowerings, one reference
  first conv  stem_conv_mfma at every width and stride, stem_conv3x3 where the frame width is no multiple of 4
  max pool, GDC   maxpool_nhwc with clipped windows on negative values; gdc_rows with dead lanes and dead rows

No tolerance anywhere: fp16 tensors through assert_same_bits, fp32 ones through assert_same_values, every net twice (run_probe).
tests/test_exact_probe_cpu.py asserts on the reference alone that these comparisons are valid and would see a dropped K-step, a bias added once
per slab, a pooled row from the wrong tile, a zero-padded pool and a missing kernel row.

Which plan ran.  A split is forced with FID_AUTOTUNE=0 and FID_CONV_FORCE (read per call, by the workspace sizing as well).  A net that does
not autotune keeps no plan table (CompiledNet.plans() lists the autotuner's picks only), so a case asserts what exact_probe.split_mirror says
for its shape and the device's CU count -- tests/test_exact_probe_cpu.py holds the mirror against the library's conv_plan -- and
test_split_cases_launch_the_slabs_the_mirror_names runs every case once more in a child process with FID_KLOG=1, where the launcher prints the
slabs it launches."""
import json
import os
import re
import subprocess
import sys

import pytest

import exact_probe as ep
from scrfd_arcface_facerecognition_amd.lower import OP_CONV, W_TYPE
from test_gpu_conv_exact import _env, _kinds, run_probe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNTUNED = dict(FID_AUTOTUNE="0", FID_NO_DIRECT="1")          # the heuristic plan, and no conv3x3_direct in its place
HOOKS = ("FID_CONV_FORCE", "FID_FORCE_GEN", "FID_FORCE_NS", "FID_PC_RS", "FID_CONV_V1", "FID_PLAN", "FID_PLAN_RO", "FID_STEM_OLD", "FID_STEM_ROLES",
         "FID_STEM_PY", "FID_NO_STEM_FUSE", "FID_STEM_VALU", "FID_GDC_SERIAL")
CLEAN = {k: None for k in HOOKS}                             # (for _env: unset)


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus(ctx):
    return int(re.search(r"\|cus=(\d+)", ctx.name()).group(1))


def _force(force):
    return tuple(int(v) for v in force.split(",")) if force else None


def _fc_force(key):
    """FID_CONV_FORCE asking for slabs of two K-steps of the FC (the launcher allows at most K-steps / 2 slabs: three steps where the count is odd)"""
    n = ep.PROBES[key]().net.nodes[-1]
    return f"64,64,{n.h * n.w * ((n.c + 31) // 32 * 32) // ep.fc_bk(n) // 2}"


FC_CASES = [(ep.FC_KEYS[sh], forced) for sh in ep.FC_SHAPES for forced in (False, True)]
# every net that must run split: (probe key, the probed OP_CONV records, FID_CONV_FORCE or None, the slabs where the force alone decides them)
ALL_SPLIT = list(ep.SPLIT_CASES) + [(key, ("fc",), _fc_force(key) if forced else None, None) for key, forced in FC_CASES]


def _split_ok(low, batch, names, force, slabs, cus):
    """the mirror's slabs of every probed op of a case: more than one, and the ones the case is about"""
    out = {}
    for name in names:
        assert int(low.ops[low.op_names.index(name)][W_TYPE]) == OP_CONV, low.op_names
        m = ep.split_mirror(*ep.conv_geometry(low, name, batch), cus, _force(force))
        assert m["ksplit"] > 1 and len(m["slabs"]) > 1 and (slabs is None or m["slabs"] == slabs), (name, m)
        out[name] = m
    return out


# ---- 1. split-K ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,names,force,slabs", ep.SPLIT_CASES, ids=[f"{k}-{f}" for k, _, f, _ in ep.SPLIT_CASES])
def test_split_k_exact(ctx, cus, monkeypatch, key, names, force, slabs):
    _env(monkeypatch, key, **{**CLEAN, **UNTUNED, "FID_CONV_FORCE": force})
    batch = ep.PROBES[key]().batch
    run_probe(ctx, key, check_low=lambda low: _split_ok(low, batch, names, force, slabs, cus))


# ---- 2. FC -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,forced", FC_CASES, ids=lambda v: v if isinstance(v, str) else ("two-step-slabs" if v else "heuristic"))
def test_fc_exact(ctx, cus, monkeypatch, key, forced):
    """BN - FC - BN on the flattened NHWC map, fp32 result: the heuristic plan always splits its K axis (asserted for this device's CU count).  The row
    with 88 channels fails with "not finite" if the layer in front leaves anything but zeros in its eight padded channels."""
    force = _fc_force(key) if forced else None
    _env(monkeypatch, key, **{**CLEAN, **UNTUNED, "FID_CONV_FORCE": force})
    batch = ep.PROBES[key]().batch

    def low_ok(low):
        m = _split_ok(low, batch, ("fc",), force, None, cus)["fc"]
        assert not forced or (m["per"] <= 3 and len(m["slabs"]) >= m["ksteps"] // 3), m
    run_probe(ctx, key, check_low=low_ok)


# ---- which slabs ran: every split case once more in a child that logs its launches ---------------------------------------------------------------------
CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import exact_probe as ep
from scrfd_arcface_facerecognition_amd._lib import Context
from scrfd_arcface_facerecognition_amd.engine import CompiledNet
ctx = Context(0)
print(ctx.name())
for i, (key, force) in enumerate(json.loads(sys.argv[2])):
    if force:
        os.environ["FID_CONV_FORCE"] = force
    else:
        os.environ.pop("FID_CONV_FORCE", None)
    p = ep.PROBES[key]()
    cn = CompiledNet(ctx, p.net, p.P, max_batch=p.batch)
    ctx.sync()
    sys.stderr.write("[klog] case %d\n" % i)
    sys.stderr.flush()
    cn.run(p.images)
    ctx.sync()
    cn.close()
ctx.close()
"""


def _child(cases, env):
    base = {k: v for k, v in os.environ.items() if k not in HOOKS}
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(cases)], env=dict(base, FID_KLOG="1", **env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    log, case, op = {}, None, None                           # case -> op index -> the "[klog]" lines of its launches
    for line in p.stderr.splitlines():
        m = re.match(r"\[klog\] (case|op|kernel|gemm) (.*)", line)
        if not m:
            continue
        if m.group(1) == "case":
            case, op = int(m.group(2)), None
        elif m.group(1) == "op":
            op = int(m.group(2))
        elif case is not None and op is not None:
            log.setdefault(case, {}).setdefault(op, []).append(m.group(1) + " " + m.group(2))
    return p.stdout, log


def test_split_cases_launch_the_slabs_the_mirror_names(cus, monkeypatch):
    from scrfd_arcface_facerecognition_amd import lower
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    stdout, log = _child([(key, force) for key, _, force, _ in ALL_SPLIT], UNTUNED)
    assert "|cus=%d" % cus in stdout
    for i, (key, names, force, slabs) in enumerate(ALL_SPLIT):
        probe = ep.PROBES[key]()
        low = lower.lower(probe.net, probe.P)
        for name, m in _split_ok(low, probe.batch, names, force, slabs, cus).items():
            lines = log[i][low.op_names.index(name)]
            want = f"gemm gen 2 tile {m['bm']}x{m['bn']}x{m['bk']} ns 4: {m['ksteps']} K-steps in {len(m['slabs'])} slabs of {m['per']}"
            assert want in lines and any("conv_mfma_dma_kernel" in l for l in lines), (key, name, force, want, lines)


# ---- 3. the fused detector stem: four fused forms and the unfused lowering against one reference -------------------------------------------------------
STEM_FORMS = {"rows8": dict(FID_STEM_PY="8"), "rows6": dict(FID_STEM_PY="6"), "roles": dict(FID_STEM_ROLES="1"), "flat": dict(FID_STEM_OLD="1"),
              "unfused": dict(FID_NO_STEM_FUSE="1")}


@pytest.mark.parametrize("form", sorted(STEM_FORMS))
@pytest.mark.parametrize("shape", ep.STEMFUSED_SHAPES, ids=lambda v: f"{v[0][0]}x{v[0][1]}-{v[1]}-{v[2]}x{v[3]}")
def test_fused_stem_exact(ctx, monkeypatch, form, shape):
    """stem.0 and stem.1 are rounded to fp16 on chip exactly as the unfused convs store them and stem.2 is rounded once, before or after the pool
    (exact_probe.stemfused_probe): the reference rounds all three, and the pooled map is compared (the unfused form: all four maps)"""
    from scrfd_arcface_facerecognition_amd import lower
    key = ep.STEMFUSED_KEYS[shape]
    _env(monkeypatch, key, **{**CLEAN, **STEM_FORMS[form]})

    def low_ok(low):
        if form == "unfused":
            assert _kinds(low) == [lower.OP_STEM, lower.OP_CONV, lower.OP_CONV, lower.OP_MAXPOOL], low.op_names
        else:
            assert low.op_names == ["stem.fused"] and _kinds(low) == [lower.OP_STEMFUSED]
    run_probe(ctx, key, check_low=low_ok)


# ---- 4. the first conv of a net on its own ------------------------------------------------------------------------------------------------------------
def _first_id(v):
    return f"{v[0][0]}x{v[0][1]}-{v[1]}s{v[2]}x{v[3]}"


@pytest.mark.parametrize("shape", ep.FIRST_SHAPES, ids=_first_id)
def test_first_conv_exact(ctx, monkeypatch, shape):
    """3 -> 12 / 28 / 64 / 128 channels at stride 1 (ReLU) and 2 (PReLU) on 36 x 52 frames (stem_conv_mfma: 16 x 16 output tiles, ragged both ways)
    and on 36 x 50 ones (a width that is no multiple of 4: stem_conv3x3)"""
    from scrfd_arcface_facerecognition_amd import lower
    key = ep.FIRST_KEYS[shape]
    _env(monkeypatch, key, **CLEAN)
    run_probe(ctx, key, check_low=lambda low: _kinds(low) == [lower.OP_STEM] or pytest.fail(str(low.op_names)))


def test_first_conv_kernels(monkeypatch):
    """frames whose width is a multiple of 4 launch stem_conv_mfma<padded couts / 16, stride>, the others stem_conv3x3"""
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    _, log = _child([(ep.FIRST_KEYS[sh], None) for sh in ep.FIRST_SHAPES], {})
    for i, (hw, cout, stride, _) in enumerate(ep.FIRST_SHAPES):
        cp = (cout + 31) // 32 * 32
        want = f"kernel stem_conv_mfma<{cp // 16}, {stride}>" if hw[1] % 4 == 0 else f"kernel stem_conv3x3 (Cout_p {cp}, stride {stride})"
        assert log[i] == {0: [want]}, (hw, cout, stride, log[i])


# ---- 5. max pool and the global depthwise conv ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ep.POOL_SHAPES, ids=lambda v: f"{v[0][0]}x{v[0][1]}-{v[1]}x{v[2]}")
def test_maxpool_exact(ctx, monkeypatch, shape):
    from scrfd_arcface_facerecognition_amd import lower
    key = ep.POOL_KEYS[shape]
    _env(monkeypatch, key, **CLEAN)
    run_probe(ctx, key, check_low=lambda low: _kinds(low) == [lower.OP_STEM, lower.OP_MAXPOOL] or pytest.fail(str(low.op_names)))


@pytest.mark.parametrize("shape", ep.GDC_SHAPES, ids=lambda v: f"{v[0]}x{v[0]}-{v[1]}-{v[3]}x{v[2]}")
def test_gdc_exact(ctx, monkeypatch, shape):
    """gdc_rows: 512 channels x 1, 3, 5 images; 128 channels x 1 = 128 threads, half of the only block dead; 5 x 5: lanes 5-7 of every group hold no row.
    The op record meets the condition under which csrc/net.hip launches gdc_rows, not dwconv_nhwc (FID_GDC_SERIAL unset)."""
    key = ep.GDC_KEYS[shape]
    _env(monkeypatch, key, **CLEAN)
    run_probe(ctx, key, check_low=lambda low: ep.takes_gdc_rows(low, "g") or pytest.fail(str(low.op_names)))
