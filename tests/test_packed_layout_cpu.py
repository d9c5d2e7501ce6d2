"""CPU: the packed face layout (pipeline.packed_layout, the host statement of fid_face_pack), the mapping PackedFacePipeline.results
builds on it, and the build facts of the new kernels (bound, in the library, no scratch)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "scrfd_arcface_facerecognition_amd", "csrc")


def layout_by_loops(counts, cap, max_per_frame, row_cap):
    """the definition, face by face"""
    offsets, src = [0], []
    for b, c in enumerate(counts):
        k = min(max(int(c), 0), cap)
        if max_per_frame > 0:
            k = min(k, max_per_frame)
        src += [b * cap + f for f in range(k)]
        offsets.append(offsets[-1] + k)
    src = (src + [-1] * row_cap)[:row_cap]
    return np.asarray(offsets, np.int32), np.asarray(src, np.int32)


# (counts, cap, max_per_frame, row_cap); tests/test_gpu_packed_faces.py runs the same vectors through fid_face_pack
CASES = [
    ([0, 0, 0, 0], 8, 0, 16),                       # no face at all
    ([3, 0, 11, 2], 8, 0, 32),                      # a count above cap
    ([5, 1, 7, 0, 2], 8, 3, 32),                    # max_per_frame clips
    ([2, -4, 3], 8, 0, 16),                         # a negative count is 0
    ([4, 4, 4, 4], 8, 0, 10),                       # total above row_cap
    ([6], 8, 0, 8),                                 # B = 1
    ([0], 8, 0, 4),
    (list(np.random.default_rng(3).integers(0, 21, 1000)), 32, 0, 12000),      # B = 1000
    (list(np.random.default_rng(4).integers(0, 21, 1000)), 32, 0, 5000),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_packed_layout_properties(case):
    from scrfd_arcface_facerecognition_amd.pipeline import packed_layout
    counts, cap, mpf, row_cap = CASES[case]
    offsets, src = packed_layout(counts, cap, mpf, row_cap)
    eo, es = layout_by_loops(counts, cap, mpf, row_cap)
    assert offsets.dtype == np.int32 and src.dtype == np.int32
    assert offsets.shape == (len(counts) + 1,) and src.shape == (row_cap,)
    assert np.array_equal(offsets, eo) and np.array_equal(src, es)
    k = np.clip(np.asarray(counts), 0, cap)
    if mpf > 0:
        k = np.minimum(k, mpf)
    assert np.array_equal(np.diff(offsets), k) and offsets[0] == 0
    total = int(offsets[-1])
    assert total == int(k.sum())                                   # NOT clipped to row_cap
    n = min(total, row_cap)
    assert (src[:n] >= 0).all() and (src[n:] == -1).all()
    assert (np.diff(src[:n]) > 0).all()                            # strictly increasing over the valid prefix
    for i in range(0, n, max(1, n // 50)):                         # each valid row names a face of the frame that owns the row
        b, f = divmod(int(src[i]), cap)
        assert offsets[b] <= i < offsets[b + 1] and f == i - offsets[b] and f < k[b]


def test_packed_layout_case_list_covers_the_named_situations():
    from scrfd_arcface_facerecognition_amd.pipeline import packed_layout
    assert packed_layout(*CASES[0])[0][-1] == 0
    assert packed_layout(*CASES[1])[0][3] - packed_layout(*CASES[1])[0][2] == 8          # clipped to cap
    assert list(np.diff(packed_layout(*CASES[2])[0])) == [3, 1, 3, 0, 2]
    assert list(np.diff(packed_layout(*CASES[3])[0])) == [2, 0, 3]
    o, s = packed_layout(*CASES[4])
    assert o[-1] == 16 and list(s) == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17]                  # the last faces in order are the dropped ones
    assert packed_layout(*CASES[8])[0][-1] > 5000 > 0


class _Names:
    def __init__(self, n):
        self.names = [f"id{i}" for i in range(n)]


def _fake_pipeline(counts, cap, row_cap, max_num, rng):
    """a PackedFacePipeline without a device: results() only needs _download() and four attributes"""
    from scrfd_arcface_facerecognition_amd.pipeline import PackedFacePipeline, packed_layout

    class Fake(PackedFacePipeline):
        def __init__(self):
            self.B, self.row_cap, self.max_num, self._overflow = len(counts), row_cap, max_num, 0
            B = self.B
            self.h_det = rng.standard_normal((B, cap, 5)).astype(np.float32)
            self.h_kps = rng.standard_normal((B, cap, 10)).astype(np.float32)
            # what the device would have left per ROW: the match result of the face the row holds
            _, src = packed_layout(counts, cap, max_num, row_cap)
            self.h_idx = np.where(src >= 0, src % 7 - 1, -99).astype(np.int32)       # -1 ("Unknown") for some, 0..5 for others
            self.h_score = np.where(src >= 0, src.astype(np.float32) / 1000, np.float32(-5)).astype(np.float32)

        def _download(self):
            return np.asarray(counts, np.int32), self.h_det, self.h_kps, self.h_idx, self.h_score

    return Fake()


@pytest.mark.parametrize("row_cap,max_num", [(32, 0), (9, 0), (32, 2), (4, 2)])
def test_results_mapping_on_host_arrays(row_cap, max_num):
    rng = np.random.default_rng(11)
    counts, cap = [3, 0, 5, 1, 4], 8
    pipe = _fake_pipeline(counts, cap, row_cap, max_num, rng)
    res = pipe.results(_Names(6))
    k = [min(c, max_num) if max_num else c for c in counts]
    total = sum(k)
    assert pipe.overflow == max(0, total - row_cap)
    assert len(res) == len(counts)
    seen = 0
    for b, faces in enumerate(res):
        want = max(0, min(k[b], row_cap - seen))                    # an overflowed batch loses trailing faces only
        assert len(faces) == want
        for f, (bbox, score, kps, name, sim) in enumerate(faces):
            assert np.array_equal(bbox, pipe.h_det[b, f, :4]) and score == float(pipe.h_det[b, f, 4])
            assert np.array_equal(kps, pipe.h_kps[b, f].reshape(5, 2))
            s = b * cap + f
            assert name == ("Unknown" if s % 7 == 0 else f"id{s % 7 - 1}") and sim == float(np.float32(s) / 1000)
        seen += k[b]
    if row_cap >= total:
        assert [len(r) for r in res] == k


def test_new_entry_points_are_declared_bound_and_built():
    from scrfd_arcface_facerecognition_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "faceid.h")).read()
    for name in ("fid_face_pack", "fid_align_crops_packed", "fid_l2_normalize_f16_packed"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        m = re.search(r"/\*(?:(?!\*/).)*\*/\s*int " + name + r"\(", hdr, flags=re.S)
        assert m and "main.py:130-134" in m.group(0) and "models/scrfd.py:159-177" in m.group(0), name     # cites what it serves
    assert lib.fid_abi_version() == 2
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bpack\.hip\b", mk, flags=re.M)
    assert "pack" not in re.search(r"^HANDCOUNTED = (.*)$", mk, flags=re.M).group(1)


_FRAMES, _ROWS = ("BgrBatch", "RaggedBatch", "Nv12Batch"), ("SlotRows", "PackedRows")
# (source, kernel, the template arguments of every instantiation the library launches -- () for a plain kernel)
KERNELS = [
    ("pack.hip", "face_pack", [()]),
    ("align.hip", "align_warp", [(f, r) for f in _FRAMES for r in _ROWS]),
    ("align.hip", "letterbox_kernel", [("BgrBatch", "UniformGeom"), ("Nv12Batch", "UniformGeom"), ("RaggedBatch", "RaggedGeom"),
                                       ("BgrBatch", "TileGeom"), ("Nv12Batch", "TileGeom")]),
    ("postproc.hip", "decode_compact", [("PlaceUniform",), ("PlaceRagged",), ("PlaceTiled",)]),
]


@pytest.mark.parametrize("src,kernel,insts", KERNELS, ids=[k[1] for k in KERNELS])
def test_new_kernels_use_no_scratch(src, kernel, insts, tmp_path):
    """a compile, not a run: the resource remarks of the device pass.  align_warp on the commit before the factoring: occupancy 8
    waves / SIMD, no scratch -- neither the shared __device__ function nor the kernel template over (frame batch, row addresser) may
    cost any of its six instantiations that.  The one-pixel letterbox template and the decode template: no scratch, no spill."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail(f"hipcc not found ({hipcc}): the library cannot have been built either")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    names = sorted({a for inst in insts for a in inst})
    found = {}
    for blk in blocks:
        mangled = blk.split()[0]
        if re.search(r"\d+" + kernel + (r"I" if names else r"E"), mangled):          # (letterbox_kernel4E is not letterbox_kernelI)
            found[tuple(a for a in names if re.search(r"\d+" + a + r"E", mangled))] = blk
    assert sorted(found) == sorted(tuple(sorted(i)) for i in insts), (sorted(found), r.stderr[-500:])
    for k, blk in found.items():
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)) == 0, k
        assert int(re.search(r"VGPRs Spill: (\d+)", blk).group(1)) == 0, k
        # (occupancy is what "not worse than before the factoring" means for a launch; with ROCm 7.2 (AMD clang 22.0.0git, roc-7.2.0)
        # align_warp compiles to 37 VGPRs before and after -- a register count is the compiler's to move, so it is not asserted)
        if kernel == "align_warp":
            assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1)) >= 8, k


def test_new_entry_points_refuse_null_arguments():
    """the NULL check comes first in each: FID_E_INVALID (-1) and a message, on a host without a GPU too.  Every call passes a NULL
    context, so nothing can be dereferenced whatever the order of the checks; the size checks run with a real context in
    tests/test_gpu_packed_faces.py."""
    from scrfd_arcface_facerecognition_amd import _lib
    lib = _lib.load()
    assert lib.fid_face_pack(None, None, 4, 8, 0, None, None, 16) == -1 and lib.fid_last_error()
    assert lib.fid_align_crops_packed(None, None, 4, 64, 64, None, 8, None, 16, None, None) == -1 and lib.fid_last_error()
    assert lib.fid_l2_normalize_f16_packed(None, None, 16, 512, None, None) == -1 and lib.fid_last_error()


def test_distributed_step_refuses_a_packed_pipeline():
    """run_step_distributed reads n_slots / F as a B x F slot grid; a packed pipeline has rows, not slots"""
    from scrfd_arcface_facerecognition_amd.pipeline import run_step_distributed
    pipe = _fake_pipeline([1, 2], 8, 8, 0, np.random.default_rng(0))
    with pytest.raises(TypeError, match="single-device"):
        run_step_distributed(pipe, None, 64, 64, None, 0.4, None, None, None)
