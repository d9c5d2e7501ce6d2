"""GPU: seeded random layer shapes through every conv kernel family that takes stride-1 layers (register-staged implicit GEMM,
channel-chunked, producer/consumer, resident-weight, two-tile, weights-in-registers conv3x3_wr in its four variants, weights-in-
registers implicit GEMM conv_gw) against the fp32 CPU oracle on the same weights and frames -- odd maps, partial tiles, odd tile
counts, single images.  A family that takes none of the case's layers is not counted (the plan read-back tells)."""
import numpy as np
import pytest

from family_helpers import force_family, forced_ran
from oracle import align, nets as onets
from scrfd_arcface_facerecognition_amd import archs
from scrfd_arcface_facerecognition_amd.archs import Conv, Net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import Context
    c = Context(0)
    yield c
    c.close()


def random_case(rng):
    h, w = int(rng.integers(12, 45)), int(rng.integers(12, 45))
    w -= w % 4                                            # the first conv reads aligned dwords of the frame rows
    c1 = int(rng.choice([64, 64, 96, 128, 192, 256]))
    c2 = int(rng.choice([64, 64, 128, 80, 256]))
    batch = int(rng.integers(1, 6))
    acts = [str(rng.choice(["relu", "prelu", "none"])) for _ in range(3)]
    return (h, max(w, 12)), c1, c2, batch, acts, bool(rng.integers(0, 2)), bool(rng.integers(0, 2))


def build(hw, c1, c2, acts, res, pre_bn):
    net = Net("t", hw, 127.5, 1.0 / 128.0)
    net.add(Conv("s", "input", 3, 64, act="relu"))
    net.add(Conv("a", "s", 64, c1, act=acts[0], pre_bn=pre_bn))
    net.add(Conv("b", "a", c1, c1, act=acts[1], res="a" if res else None))
    net.add(Conv("c", "b", c1, c2, act=acts[2]))
    net.outputs = ["c"]
    return net


# family codes (family_helpers.FAMILIES) of every variant that takes stride-1 layers
CODES = [1, 3, 5, 7, 8, 91, 92, 93, 94, 96, 97, 98, 909, 929, 939, 910, 11]


@pytest.mark.parametrize("seed", range(24))
def test_families_vs_oracle(ctx, monkeypatch, seed):
    from scrfd_arcface_facerecognition_amd.engine import CompiledNet
    rng = np.random.default_rng(1000 + seed)
    hw, c1, c2, batch, acts, res, pre_bn = random_case(rng)
    net = build(hw, c1, c2, acts, res, pre_bn)
    P = archs.synth_params(net, seed=seed)
    images = rng.integers(0, 256, (batch,) + hw + (3,), dtype=np.uint8)
    ref = onets.run_net(net, P, align.blob_from_images(list(images), net.in_scale, net.in_mean))["c"]
    ref = np.transpose(ref, (0, 2, 3, 1))
    scale = np.abs(ref).max() + 1e-6
    n_checked = 0
    for code in CODES:
        force_family(monkeypatch, code)
        cn = CompiledNet(ctx, net, P, max_batch=batch)
        cn.run(images)
        o = cn.read("c", batch).astype(np.float32)
        ran = forced_ran(cn, code)
        cn.close()
        if not ran:
            continue
        n_checked += 1
        assert np.isfinite(o).all(), (code, hw, c1, c2, batch)
        assert np.abs(o - ref).max() / scale < 8e-3, (code, ran, hw, c1, c2, batch, acts, res, pre_bn)
    assert n_checked >= 2, (hw, c1, c2)
