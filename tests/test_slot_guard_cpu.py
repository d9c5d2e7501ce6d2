"""CPU: the activation-slot arithmetic the GPU batch-shape tests poison and check by (family_helpers.slot_table / guard_regions) against
lower()'s tensor tables -- every tensor's first b images end at or below its slot's guard start, the guard regions are non-empty and
disjoint, a view reports its base's slot -- for the full architectures and the layer stacks tests/test_gpu_batch_shapes.py runs."""
import numpy as np
import pytest

from scrfd_arcface_facerecognition_amd import archs
from scrfd_arcface_facerecognition_amd.lower import T_SLOT, lower

from family_helpers import guard_regions, own_data_tensors, slot_table, stack

# (hw, chans, max_batch): the stacks of tests/test_gpu_batch_shapes.py
STACKS = [((7, 7), (128, 128), 9), ((7, 7), (64, 192), 9), ((14, 14), (128, 128), 17), ((14, 14), (64, 256), 17), ((37, 21), (64, 128), 3),
          ((20, 20), (64, 96), 5), ((20, 20), (224, 224), 5), ((28, 28), (128, 256), 5)]

NETS = {"scrfd_10g": (lambda: archs.scrfd_10g((640, 640)), 4), "scrfd_500m": (lambda: archs.scrfd_500m((320, 320)), 5),
        "iresnet50": (archs.iresnet50, 192), "arcface_mbf": (archs.mobilefacenet, 6), "arcface_mbf_small": (archs.mobilefacenet_small, 6)}
NETS.update({f"stack{hw[0]}x{hw[1]}_{'_'.join(map(str, ch))}": ((lambda hw=hw, ch=ch: stack(hw, ch)), m) for hw, ch, m in STACKS})


@pytest.mark.parametrize("name", sorted(NETS))
def test_slot_guard_layout(name):
    make, max_batch = NETS[name]
    net = make()
    low = lower(net, archs.synth_params(net, 0))
    t_slot, t_bytes, s_bytes = slot_table(low)
    assert len(t_slot) == len(low.tensor_id) == low.tensors.shape[0] and min(t_slot) >= 0
    # the rule of csrc/net.hip (fid_net_create, slot_bytes_per_image) restated on the raw columns: C, Cp, H, W, dtype, slot
    T = np.asarray(low.tensors, dtype=np.int64)
    per_image = T[:, 2] * T[:, 3] * T[:, 1] * np.where(T[:, 4] == 1, 4, 2)
    assert t_bytes == per_image.tolist() and t_slot == T[:, 5].tolist()
    assert s_bytes == {int(s): int(per_image[T[:, 5] == s].max()) for s in np.unique(T[:, 5])}
    assert sorted(s_bytes) == list(range(len(s_bytes)))                   # slots are numbered densely: the library allocates max + 1 of them
    for b in range(1, max_batch):
        regions = guard_regions(low, b, max_batch)
        for t, (slot, nbytes) in enumerate(zip(t_slot, t_bytes)):
            lo, hi = regions[slot]
            assert nbytes > 0 and b * nbytes <= lo, (name, b, t)          # the live rows of every tenant end at or below the guard
            assert max_batch * nbytes <= hi                               # ... and no tenant reaches beyond the slot's allocation
        spans = sorted((slot, lo, hi) for slot, (lo, hi) in regions.items())
        assert all(hi > lo and lo % 2 == 0 and hi % 2 == 0 for _, lo, hi in spans), (name, b)     # non-empty, whole 16-bit pattern words
        assert len({slot for slot, _, _ in spans}) == len(spans)          # one region per slot: disjoint in (slot, byte) terms
        assert all(lo == b * s_bytes[slot] and hi == max_batch * s_bytes[slot] for slot, lo, hi in spans)
    # the largest tenant of a slot fills it exactly: the guard starts where that tensor's row b starts
    for slot, n in s_bytes.items():
        assert n == max(nb for s, nb in zip(t_slot, t_bytes) if s == slot)


@pytest.mark.parametrize("name", ["iresnet50", "arcface_mbf", "arcface_mbf_small"])
def test_view_reports_the_slot_of_its_base(name):
    """the FC layer reads the last activation through a flattened view ([1, 1, H*W*Cp]): same slot, same bytes per image as its base"""
    net = NETS[name][0]()
    low = lower(net, archs.synth_params(net, 0))
    t_slot, t_bytes, _ = slot_table(low)
    views = [n for n in low.tensor_id if n.endswith(".in_view")]
    assert views
    for v in views:
        fc = next(x for x in net.nodes if x.name == v[:-len(".in_view")])
        vi, bi = low.tensor_id[v], low.tensor_id[fc.src]
        assert t_slot[vi] == t_slot[bi] and t_bytes[vi] == t_bytes[bi]
        assert int(low.tensors[vi][T_SLOT]) == int(low.tensors[bi][T_SLOT]) >= 0


@pytest.mark.parametrize("name", sorted(NETS))
def test_own_data_tensors_cover_the_outputs(name):
    """the tensors a bit-for-bit comparison of two nets may read: one per slot at most, every output among them"""
    net = NETS[name][0]()
    low = lower(net, archs.synth_params(net, 0))
    t_slot, _, s_bytes = slot_table(low)
    own = own_data_tensors(low)
    assert set(net.outputs) <= set(own)
    slots = [t_slot[low.tensor_id[n]] for n in own]
    assert len(set(slots)) == len(slots) <= len(s_bytes)
    assert not np.any([n.endswith(".in_view") for n in own])
