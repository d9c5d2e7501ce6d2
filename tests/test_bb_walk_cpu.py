"""CPU: the walk form of the fused 64-channel block (csrc/conv_bb.hip: conv_bb_walk), what can be held without a device.

  * the probes tests/test_gpu_bb_walk.py compares bit for bit (tests/bb_walk_probes.py) meet the exactness conditions that
    tests/test_exact_probe_cpu.py asserts for the committed probes -- the same functions, called on the new keys;
  * the launcher's choice between the tile and the walk form (conv_bb_form_cost: MFMAs per wave of the busiest workgroup) through a
    stand-alone host program: the derived counts at the benchmark shape, the walk form there and the tile form at batch 8."""
import os
import subprocess

import pytest

import bb_walk_probes as wp
import test_exact_probe_cpu as probe_checks
from test_conv_variants_cpu import HERE, HIPCC, LIB, PKG

CUS = 256                 # MI355X: the 33 x 15 probe has CUS / 2 + 2 = 130 images


@pytest.fixture(scope="module")
def keys():
    return wp.register(CUS)


@pytest.mark.parametrize("i", range(len(wp.WALK_SHAPES)), ids=wp.IDS)
def test_walk_probe_meets_the_exactness_conditions(keys, i):
    key = keys[i]
    probe_checks.test_probe_conditions(key)
    probe_checks.test_fp32_sum_is_order_independent(key)
    for fault in ("fault_tap", "fault_f16acc", "fault_rtz"):
        probe_checks.test_comparator_sees_planted_fault(key, fault)
    probe_checks.test_relu_commutes_with_the_rounding(key)


def test_walk_shapes_cover_what_they_say():
    """the item arithmetic of the kernel's header comment on the probe shapes: items per strip, the reduced strip end, strips against workgroups"""
    def geo(hw):
        """(items per strip, real rows of the last item [item s holds output rows 16 s - 1 .. 16 s + 14], bands, columns of the last band)"""
        H, W = hw
        S = (H + 1 + 15) // 16
        return S, H - max(16 * (S - 1) - 1, 0), (W + 13) // 14, W - 14 * ((W - 1) // 14)
    assert geo((37, 45)) == (3, 6, 4, 3)                     # two carries; ragged bottom and right
    assert geo((16, 14)) == (2, 1, 1, 14)                    # the reduced item (one real row: H a multiple of 16); one exact-width strip
    assert geo((17, 16)) == (2, 2, 2, 2)                     # two real rows: the general path; a 2-pixel strip
    assert geo((15, 20)) == (1, 15, 2, 6)                    # one item that ends exactly on its last row (-1 .. 14)
    assert geo((3, 3)) == (1, 3, 1, 3)
    assert geo((33, 15))[:3] == (3, 2, 2) and 2 * wp.batch_of(wp.WALK_SHAPES[5], CUS) > CUS      # more strips than workgroups


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not (os.path.exists(HIPCC) and os.path.exists(LIB)):
        pytest.skip("needs hipcc and the built libfaceid.so")
    exe = str(tmp_path_factory.mktemp("bb_form_cost") / "driver")
    p = subprocess.run([HIPCC, "-std=c++17", "-O1", os.path.join(HERE, "bb_form_cost_driver.cpp"), "-o", exe, "-L" + PKG, "-l:libfaceid.so", "-Wl,-rpath," + PKG],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def _cost(driver, *shapes):
    p = subprocess.run([driver] + [str(v) for sh in shapes for v in sh], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    assert len(rows) == len(shapes)
    return [(int(t), int(w), form) for t, w, form in rows]


def test_launcher_picks_walk_at_the_benchmark_shape_and_tile_at_batch_8(driver):
    bench, small = _cost(driver, (64, 160, 160, 256), (8, 160, 160, 256))
    assert bench == (36 * 270, 3 * (10 * 288 + 18), "walk")             # 9 720 against 8 694: 768 strips are three per CU
    assert small == (5 * 270, 10 * 288 + 18, "tile")                    # 96 strips would leave most CUs idle


def test_form_cost_on_other_shapes(driver):
    got = _cost(driver, (2, 37, 45, 256), (1, 3, 3, 256), (130, 33, 15, 256), (64, 56, 56, 256), (64, 161, 160, 256), (512, 17, 14, 256))
    assert got[0] == (270, 3 * 288, "tile")
    assert got[1] == (270, 288, "tile")
    assert got[2] == (4 * 270, 2 * 3 * 288, "tile")                     # 780 tiles, 260 strips of three items
    assert got[3] == (4 * 270, 4 * 288, "tile")                         # 56 rows are exactly four 14-row tiles: 1 024 tiles against 256 strips of 4 items
    assert got[4] == (36 * 270, 3 * 11 * 288, "walk")                   # 161 rows: eleven full items (two real rows in the last) against twelve tile rows
    assert got[5] == (4 * 270, 2 * 2 * 288, "tile")                     # two-item strips: 1 024 tiles against 512 strips
