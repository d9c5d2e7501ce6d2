"""CPU: the host half of mixed-size image batches -- `_lib.pack_images` (layout and errors) and the four *_ragged entry points in
header, binding and library."""
import numpy as np
import pytest

from scrfd_arcface_facerecognition_amd import _lib
from test_abi import header_symbols

RAGGED = ("fid_letterbox_ragged", "fid_scrfd_postprocess_ragged", "fid_align_crops_ragged", "fid_align_crops_packed_ragged")
SHAPES = [(5, 7), (1, 1), (33, 97), (64, 64), (97, 33)]


def test_pack_images_layout():
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    images[3] = images[3][:, ::-1]                       # a non-contiguous view packs like its dense copy
    buf, hw, offsets = _lib.pack_images(images)
    assert buf.dtype == np.uint8 and buf.ndim == 1
    assert hw.dtype == np.int32 and hw.shape == (len(SHAPES), 2) and hw.tolist() == [list(s) for s in SHAPES]
    assert offsets.dtype == np.int64 and offsets.shape == (len(SHAPES),)
    sizes = [h * w * 3 for h, w in SHAPES]
    assert offsets.tolist() == [sum(sizes[:i]) for i in range(len(sizes))]          # the running sum: input order, no padding
    assert buf.size == sum(sizes)
    for im, o, n in zip(images, offsets, sizes):
        assert np.array_equal(buf[o:o + n].reshape(im.shape), im)
    one, hw1, off1 = _lib.pack_images([images[0]])
    assert np.array_equal(one, images[0].reshape(-1)) and hw1.tolist() == [[5, 7]] and off1.tolist() == [0]


@pytest.mark.parametrize("bad, index", [
    (np.zeros((4, 4, 3), np.float32), 1),                # a float image
    (np.zeros((4, 4), np.uint8), 2),                     # a 2-D image
    (np.zeros((4, 4, 4), np.uint8), 0),                  # four channels
    (np.zeros((0, 4, 3), np.uint8), 1),                  # H = 0
    (np.zeros((4, 0, 3), np.uint8), 2),                  # W = 0
    ([[1, 2, 3]], 0),                                    # not an array
])
def test_pack_images_names_the_bad_image(bad, index):
    images = [np.zeros((3, 5, 3), np.uint8) for _ in range(3)]
    images[index] = bad
    with pytest.raises(ValueError, match=rf"image {index}\b"):
        _lib.pack_images(images)


def test_pack_images_empty_list():
    with pytest.raises(ValueError):
        _lib.pack_images([])


def test_ragged_entry_points_declared_and_bound():
    syms = header_symbols()
    lib = _lib.load()
    for name in RAGGED:
        assert name in syms and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.fid_abi_version() == 2                    # the change only adds


def test_ragged_calls_reject_null_arguments():
    """argument checks come before any device work: safe without a GPU"""
    lib = _lib.load()
    assert lib.fid_letterbox_ragged(None, None, 0, None, None, 1, None, 64, 64, None) == -1 and lib.fid_last_error()
    assert lib.fid_align_crops_ragged(None, None, 0, None, None, 1, None, None, 1, 1, None, None) == -1
    assert lib.fid_align_crops_packed_ragged(None, None, 0, None, None, 1, None, 1, None, 1, None, None) == -1
    assert lib.fid_scrfd_postprocess_ragged(None, None, None, None, None, 1, 64, 64, 2, None, 0.5, 0.4, 0, 0, None, None, None, 1) == -1


def test_letterbox_geometry_of_the_gpu_test_shapes():
    """the shapes tests/test_gpu_mixed_sizes.py letterboxes give non-zero new_h, new_w at its three output sizes; (2,640) does not at the
    small ones (it is that file's degenerate case)"""
    from oracle.postprocess import letterbox_geometry
    shapes = [(1080, 1920), (640, 640), (1280, 1280), (480, 853), (853, 480), (700, 500), (641, 639), (97, 33), (33, 97), (5, 7)]
    for in_h, in_w in ((640, 640), (64, 96), (63, 95)):
        for H, W in shapes:
            new_w, new_h, _ = letterbox_geometry(H, W, (in_w, in_h))
            assert new_w > 0 and new_h > 0, (H, W, in_h, in_w)
    for in_h, in_w in ((64, 96), (63, 95)):
        assert letterbox_geometry(2, 640, (in_w, in_h))[1] == 0
