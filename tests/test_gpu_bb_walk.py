"""GPU: the walk form of the fused 64-channel block (csrc/conv_bb.hip: conv_bb_walk, column strips walked top-down with the two intermediate
rows above an item carried in LDS) against the exact reference of tests/exact_probe.py, bit for bit, at the shapes of tests/bb_walk_probes.py.

Every shape runs under FID_BB_V=3 (the walk form) and under FID_BB_V=1 (the tile form, conv_bb) through test_gpu_conv_exact.run_probe: two runs
each, so both strip orders are covered, and plain equality with the one reference -- which also pins the two forms to each other.
tests/test_bb_walk_cpu.py asserts that the comparison is valid on these probes.  test_forced_forms_launch_their_kernels runs every case once
more in a child process with FID_KLOG=1: the equality would hold just as well if the hook were ignored and the tile form had run."""
import json
import os
import re
import subprocess
import sys

import pytest

import bb_walk_probes as wp
from test_gpu_conv_exact import _kinds, run_probe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("FID_BB_V", "FID_NO_BB_FUSE", "FID_BB_ABLATE", "FID_BB_STAGGER")


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def keys(cus):
    return wp.register(cus)


@pytest.mark.parametrize("form", ["3", "1"], ids=["walk", "tile"])
@pytest.mark.parametrize("i", range(len(wp.WALK_SHAPES)), ids=wp.IDS)
def test_walk_block_exact(ctx, keys, monkeypatch, i, form):
    from scrfd_arcface_facerecognition_amd import lower
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FID_BB_V", form)

    def low_ok(low):
        assert _kinds(low).count(lower.OP_BBLOCK) == 1 and len(low.ops) == 2, low.op_names
    run_probe(ctx, keys[i], check_low=low_ok)


CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import exact_probe as ep
import bb_walk_probes as wp
from scrfd_arcface_facerecognition_amd._lib import Context
from scrfd_arcface_facerecognition_amd.engine import CompiledNet
ctx = Context(0)
keys = wp.register(int(sys.argv[2]))
for i, (k, form) in enumerate(json.loads(sys.argv[3])):
    os.environ["FID_BB_V"] = form
    p = ep.PROBES[keys[k]]()
    cn = CompiledNet(ctx, p.net, p.P, max_batch=p.batch)
    ctx.sync()
    sys.stderr.write("[klog] case %d\n" % i)
    sys.stderr.flush()
    cn.run(p.images)
    ctx.sync()
    cn.close()
ctx.close()
"""


def test_forced_forms_launch_their_kernels(cus):
    """FID_BB_V=3 launches conv_bb_walk and FID_BB_V=1 conv_bb at every shape of the cases above: each case's log names exactly one of the two"""
    cases = [(k, form) for k in range(len(wp.WALK_SHAPES)) for form in ("3", "1")]
    base = {k: v for k, v in os.environ.items() if k not in HOOKS}
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(cus), json.dumps(cases)], env=dict(base, FID_KLOG="1"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    log, case = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"\[klog\] (case|kernel) (.*)", line)
        if m and m.group(1) == "case":
            case = int(m.group(2))
        elif m and case is not None:
            log.setdefault(case, []).append(m.group(2))
    for i, (k, form) in enumerate(cases):
        walk = [l for l in log.get(i, []) if "conv_bb_walk" in l]
        tile = [l for l in log.get(i, []) if re.search(r"conv_bb(ILb0E|<false>)", l)]       # (mangled or demangled)
        assert (len(walk), len(tile)) == ((1, 0) if form == "3" else (0, 1)), (wp.IDS[k], form, log.get(i))
