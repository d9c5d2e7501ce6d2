"""The exact probes of the walk form of the fused 64-channel block (csrc/conv_bb.hip: conv_bb_walk): exact_probe.bb_probe at the shapes where
the walk can go wrong.  Shared by tests/test_bb_walk_cpu.py and tests/test_gpu_bb_walk.py (and the latter's child process); register() adds
them to exact_probe.PROBES when a test runs, not at import: the parametrised cases of the other probe modules stay the ones they list."""
import functools

import exact_probe as ep

# ((H, W), batch or None = CU count / 2 + 2, what it covers)
WALK_SHAPES = [
    ((37, 45), 2, "three items per strip, two carries, ragged bottom and right"),
    ((16, 14), 3, "the one-row strip end (reduced item), one exact-width strip"),
    ((17, 16), 2, "a two-row last item on the general path, a 2-pixel strip"),
    ((15, 20), 2, "a single item that ends exactly, no carry"),
    ((3, 3), 1, "the launcher's minimum"),
    ((33, 15), None, "more strips than workgroups: some workgroup starts a second strip and must reset its carry"),
]
IDS = [f"{hw[0]}x{hw[1]}x{b or 'cus'}" for hw, b, _ in WALK_SHAPES]
_probe = functools.lru_cache(maxsize=None)(ep.bb_probe)


def batch_of(shape, cus):
    return shape[1] if shape[1] is not None else cus // 2 + 2


def register(cus):
    """probe keys of WALK_SHAPES, in order, on a device with `cus` compute units"""
    keys = []
    for sh in WALK_SHAPES:
        args = (sh[0], 64, batch_of(sh, cus))
        name = f"bb-{args[0][0]}x{args[0][1]}-64x{args[2]}"
        if name not in ep.PROBES:
            assert ep._register(_probe, *args) == name
        keys.append(name)
    return keys
