"""GPU: the image front end of csrc/align.hip against float64 sampling (tests/sampling_reference.py), at the images, poses and shapes of
tests/test_sampling_envelope_cpu.py.  Every kernel test asserts two things: the bytes lie inside the derived envelope, and the bytes
equal oracle/align.py's -- the second tells "kernel differs from oracle" from "both are outside".  Also here: landmark sets that admit
no transform (zero crop, NaN M row, neighbours untouched) and rank-1 landmark sets (closed form == SVD on the device)."""
import ctypes as C

import numpy as np
import pytest

import sampling_reference as sr
from oracle import align

pytestmark = pytest.mark.gpu

H0, W0 = sr.FRAME_HW
RAGGED_HW = (77, 101)             # the second frame of the mixed-size forms


@pytest.fixture(scope="module")
def ctx():
    from scrfd_arcface_facerecognition_amd._lib import default_context
    return default_context(0)


def _i32(a):
    from scrfd_arcface_facerecognition_amd._lib import c_i32_p
    return a.ctypes.data_as(c_i32_p)


def _i64(a):
    from scrfd_arcface_facerecognition_amd._lib import c_i64_p
    return a.ctypes.data_as(c_i64_p)


def rel_diff(M, ref):
    return np.abs(M - ref).max() / max(1.0, np.abs(ref).max())


class Faces:
    """the frames, the 60 poses, and what each (frame, pose) must give: computed once, shared by the four entry points"""

    def __init__(self):
        self.frames = {"ramp": sr.ramp_image(H0, W0), "noise": sr.noise_image(H0, W0), "small": sr.noise_image(*RAGGED_HW)}
        self.lms = sr.poses()
        self._want = {}
        self.worst = {}

    def want(self, name, i):
        if (name, i) not in self._want:
            M, _ = align.estimate_norm(self.lms[i], f64=True)
            exact, G = sr.exact_warp(self.frames[name], M)
            self._want[name, i] = (M, exact, G, align.norm_crop_image(self.frames[name], self.lms[i]))
        return self._want[name, i]

    def check(self, kernel, name, i, crop, M_dev):
        M, exact, G, ref = self.want(name, i)
        assert rel_diff(M_dev.reshape(2, 3), M) < 1e-9, (kernel, name, i)
        r = sr.warp_ratio(crop, exact, G)
        self.worst[kernel, name] = max(self.worst.get((kernel, name), 0.0), r)
        assert r <= 1.0, (kernel, name, i, r)                                   # inside the envelope
        assert np.array_equal(crop, ref), (kernel, name, i)                     # and the oracle's bytes

    def report(self, kernel):
        for (k, name), r in sorted(self.worst.items()):
            if k == kernel:
                print(f"{kernel}, {name}: max |byte - exact| / bound = {r:.4f}")


@pytest.fixture(scope="module")
def faces():
    return Faces()


F = 8
COUNTS = np.array([8, 5], np.int32)
# frame 0 takes poses 0..6 and the mirrored one, frame 1 poses 8..15
SLOT_POSE = np.array([[0, 1, 2, 3, 4, 5, 6, sr.N_POSES - 1], [8, 9, 10, 11, 12, 13, 14, 15]])


def slot_kps(faces):
    return faces.lms[SLOT_POSE].reshape(2, F, 10).astype(np.float32)


def filled(ctx, shape, dtype=np.uint8):
    """an output buffer of 0xA5 bytes: a zero in it has been written"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return ctx.to_device(np.full(n, 0xA5, np.uint8).view(dtype).reshape(shape))


# ---- the warp: four entry points ---------------------------------------------------------------------------------------------------

def test_align_crops_slots(ctx, faces):
    from scrfd_arcface_facerecognition_amd._lib import check
    names = ["ramp", "noise"]
    fr = ctx.to_device(np.stack([faces.frames[n] for n in names]))
    kp, cn = ctx.to_device(slot_kps(faces)), ctx.to_device(COUNTS)
    crops, M = filled(ctx, (2 * F, 112, 112, 3)), filled(ctx, (2 * F, 6), np.float64)
    check(ctx.lib.fid_align_crops(ctx.handle, C.c_void_p(fr.ptr), 2, H0, W0, C.c_void_p(kp.ptr), C.c_void_p(cn.ptr), F, F, C.c_void_p(crops.ptr),
                                  C.c_void_p(M.ptr)))
    crops, M = crops.download().reshape(2, F, 112, 112, 3), M.download().reshape(2, F, 6)
    for b in range(2):
        for f in range(F):
            if f < COUNTS[b]:
                faces.check("fid_align_crops", names[b], SLOT_POSE[b, f], crops[b, f], M[b, f])
            else:
                assert not crops[b, f].any() and not M[b, f].any(), (b, f)      # the empty slots are zero, as ever
    faces.report("fid_align_crops")


def test_align_crops_packed_all_poses(ctx, faces):
    """the row-table form, every pose on both frames: a shuffled table with -1 rows in it"""
    from scrfd_arcface_facerecognition_amd._lib import check
    names = ["ramp", "noise"]
    n_pose = sr.N_POSES
    fr = ctx.to_device(np.stack([faces.frames[n] for n in names]))
    kp = ctx.to_device(np.broadcast_to(faces.lms.reshape(1, n_pose, 10), (2, n_pose, 10)).astype(np.float32))
    rng = np.random.default_rng(41)
    src = np.concatenate([rng.permutation(2 * n_pose), np.full(7, -1)]).astype(np.int32)
    src = src[rng.permutation(len(src))]
    n = len(src)
    sd = ctx.to_device(src)
    crops, M = filled(ctx, (n, 112, 112, 3)), filled(ctx, (n, 6), np.float64)
    check(ctx.lib.fid_align_crops_packed(ctx.handle, C.c_void_p(fr.ptr), 2, H0, W0, C.c_void_p(kp.ptr), n_pose, C.c_void_p(sd.ptr), n,
                                         C.c_void_p(crops.ptr), C.c_void_p(M.ptr)))
    crops, M = crops.download(), M.download()
    for i, s in enumerate(src):
        if s < 0:
            assert not crops[i].any() and not M[i].any(), i
        else:
            faces.check("fid_align_crops_packed", names[s // n_pose], s % n_pose, crops[i], M[i])
    faces.report("fid_align_crops_packed")


@pytest.fixture(scope="module")
def ragged(ctx, faces):
    """the ramp frame, one byte, then a 77x101 frame: the second image starts at an odd offset"""
    a, b = faces.frames["ramp"], faces.frames["small"]
    host = np.concatenate([a.reshape(-1), np.full(1, 0xEE, np.uint8), b.reshape(-1)])
    hw = np.array([a.shape[:2], b.shape[:2]], np.int32)
    offsets = np.array([0, a.size + 1], np.int64)
    assert offsets[1] % 2 == 1
    return ctx.to_device(host), host.nbytes, hw, offsets


def test_align_crops_ragged(ctx, faces, ragged):
    from scrfd_arcface_facerecognition_amd._lib import check
    names = ["ramp", "small"]
    frames, nbytes, hw, offsets = ragged
    kp, cn = ctx.to_device(slot_kps(faces)), ctx.to_device(COUNTS)
    crops, M = filled(ctx, (2 * F, 112, 112, 3)), filled(ctx, (2 * F, 6), np.float64)
    check(ctx.lib.fid_align_crops_ragged(ctx.handle, C.c_void_p(frames.ptr), C.c_size_t(nbytes), _i32(hw), _i64(offsets), 2, C.c_void_p(kp.ptr),
                                         C.c_void_p(cn.ptr), F, F, C.c_void_p(crops.ptr), C.c_void_p(M.ptr)))
    crops, M = crops.download().reshape(2, F, 112, 112, 3), M.download().reshape(2, F, 6)
    for b in range(2):
        for f in range(F):
            if f < COUNTS[b]:
                faces.check("fid_align_crops_ragged", names[b], SLOT_POSE[b, f], crops[b, f], M[b, f])
            else:
                assert not crops[b, f].any() and not M[b, f].any(), (b, f)
    faces.report("fid_align_crops_ragged")


def test_align_crops_packed_ragged(ctx, faces, ragged):
    from scrfd_arcface_facerecognition_amd._lib import check
    names = ["ramp", "small"]
    frames, nbytes, hw, offsets = ragged
    kp = ctx.to_device(slot_kps(faces))
    rng = np.random.default_rng(42)
    rows = [b * F + f for b in range(2) for f in range(int(COUNTS[b]))]
    src = np.array(rows + [-1, -1, -1], np.int32)[rng.permutation(len(rows) + 3)]
    n = len(src)
    sd = ctx.to_device(src)
    crops, M = filled(ctx, (n, 112, 112, 3)), filled(ctx, (n, 6), np.float64)
    check(ctx.lib.fid_align_crops_packed_ragged(ctx.handle, C.c_void_p(frames.ptr), C.c_size_t(nbytes), _i32(hw), _i64(offsets), 2,
                                                C.c_void_p(kp.ptr), F, C.c_void_p(sd.ptr), n, C.c_void_p(crops.ptr), C.c_void_p(M.ptr)))
    crops, M = crops.download(), M.download()
    for i, s in enumerate(src):
        if s < 0:
            assert not crops[i].any() and not M[i].any(), i
        else:
            faces.check("fid_align_crops_packed_ragged", names[s // F], SLOT_POSE[s // F, s % F], crops[i], M[i])
    faces.report("fid_align_crops_packed_ragged")


# ---- the letterbox ------------------------------------------------------------------------------------------------------------------

_LB = {}


def lb_want(hw, in_hw, name):
    """image, letterbox_expect's dict and the oracle's letterbox, once per (shape, input, image)"""
    key = (hw, in_hw, name)
    if key not in _LB:
        image = sr.ramp_image(*hw) if name == "ramp" else sr.noise_image(*hw)
        _LB[key] = (image, sr.letterbox_expect(image, *in_hw), align.letterbox(image, (in_hw[1], in_hw[0]))[0])
    return _LB[key]


def lb_check(kernel, hw, in_hw, name, got, scale):
    image, e, ref = lb_want(hw, in_hw, name)
    assert scale == e["det_scale"], (kernel, hw, in_hw)
    zero, up, down = sr.letterbox_check(got, e)
    print(f"{kernel} {hw} -> {in_hw} ({e['kind']}), {name}: upper {up:.3f}, lower {down:.3f}")
    assert zero and up <= 1.0 and down <= 1.0, (kernel, hw, in_hw, name, zero, up, down)
    assert np.array_equal(got, ref), (kernel, hw, in_hw, name)


@pytest.mark.parametrize("hw, in_hw", sr.RESIZE_CASES)             # in_w 96, 64, 640, 160: four pixels per thread; 95: the byte kernel
def test_letterbox(ctx, hw, in_hw):
    from scrfd_arcface_facerecognition_amd._lib import check
    names = ["ramp", "noise"]
    fr = ctx.to_device(np.stack([lb_want(hw, in_hw, n)[0] for n in names]))
    out = filled(ctx, (2,) + in_hw + (3,))
    sc = C.c_double()
    check(ctx.lib.fid_letterbox(ctx.handle, C.c_void_p(fr.ptr), 2, hw[0], hw[1], C.c_void_p(out.ptr), in_hw[0], in_hw[1], C.byref(sc)))
    got = out.download()
    for b, n in enumerate(names):
        lb_check("fid_letterbox", hw, in_hw, n, got[b], sc.value)


def test_letterbox_ragged(ctx):
    """every image of test_letterbox as ONE allocation behind a 2-byte pad; one call per detector input over the images that go into it"""
    from scrfd_arcface_facerecognition_amd._lib import check, pack_images
    PAD = 2
    keys = [(hw, in_hw, n) for hw, in_hw in sr.RESIZE_CASES for n in ("ramp", "noise")]
    buf, hw_all, off_all = pack_images([lb_want(*k)[0] for k in keys])
    off_all = off_all + PAD
    host = np.concatenate([np.full(PAD, 0xEE, np.uint8), buf])
    frames = ctx.to_device(host)
    assert len({int(o) % 4 for o in off_all}) >= 3                 # odd image sizes move the residue: most images start unaligned
    for in_hw in sorted({k[1] for k in keys}):
        idx = [i for i, k in enumerate(keys) if k[1] == in_hw]
        hw, off = np.ascontiguousarray(hw_all[idx]), np.ascontiguousarray(off_all[idx])
        B = len(idx)
        out = filled(ctx, (B,) + in_hw + (3,))
        scales = np.zeros(B, np.float64)
        check(ctx.lib.fid_letterbox_ragged(ctx.handle, C.c_void_p(frames.ptr), C.c_size_t(host.nbytes), _i32(hw), _i64(off), B, C.c_void_p(out.ptr),
                                           in_hw[0], in_hw[1], scales.ctypes.data_as(C.POINTER(C.c_double))))
        got = out.download()
        for j, i in enumerate(idx):
            lb_check("fid_letterbox_ragged", keys[i][0], in_hw, keys[i][2], got[j], scales[j])


@pytest.mark.parametrize("in_hw", [(64, 96), (63, 95)])            # four pixels per thread, the byte kernel
def test_tile_cut(ctx, faces, in_hw):
    """a letterboxed (kind 1) rectangle that does not start at the origin -- its rows are W, not w, pixels apart -- and a native (kind 0) one,
    of both frames: the letterbox of the slice as its own image / the slice itself on zeros"""
    from scrfd_arcface_facerecognition_amd._lib import check
    names = ["ramp", "noise"]
    frames = np.stack([faces.frames[n] for n in names])
    tiles = np.array([[b, x0, y0, w, h, kind] for b in range(2) for (x0, y0, w, h, kind) in ((13, 7, 97, 54, 1), (5, 9, 60, 50, 0))], np.int32)
    T = len(tiles)
    fr = ctx.to_device(frames)
    out = filled(ctx, (T,) + in_hw + (3,))
    check(ctx.lib.fid_tile_cut(ctx.handle, C.c_void_p(fr.ptr), 2, H0, W0, _i32(tiles), T, C.c_void_p(out.ptr), in_hw[0], in_hw[1]))
    got = out.download()
    for t, (b, x0, y0, w, h, kind) in enumerate(tiles.tolist()):
        piece = np.ascontiguousarray(frames[b, y0:y0 + h, x0:x0 + w])
        if kind == 0:
            assert np.array_equal(got[t, :h, :w], piece) and not got[t, h:].any() and not got[t, :, w:].any(), t
            continue
        e = sr.letterbox_expect(piece, *in_hw)
        assert e["kind"] == "linear"
        zero, up, down = sr.letterbox_check(got[t], e)
        print(f"fid_tile_cut kind 1 {(h, w)} -> {in_hw}, {names[b]}: upper {up:.3f}, lower {down:.3f}")
        assert zero and up <= 1.0 and down <= 1.0, (t, zero, up, down)
        assert np.array_equal(got[t], align.letterbox(piece, (in_hw[1], in_hw[0]))[0]), t


# ---- landmark sets that admit no transform, and rank-1 sets ------------------------------------------------------------------------

def degenerate_sets():
    good = sr.poses()[3].astype(np.float32)
    nan, pinf, ninf = good.copy(), good.copy(), good.copy()
    nan[2, 1] = np.nan
    pinf[0, 0] = np.inf
    ninf[4, 1] = -np.inf
    return {"five identical points": np.tile(np.float32([[50.0, 40.0]]), (5, 1)), "one NaN coordinate": nan, "+Inf": pinf, "-Inf": ninf,
            "all coordinates 3e38": np.full((5, 2), 3e38, np.float32)}


def test_degenerate_landmarks_get_a_zero_crop_and_leave_their_neighbours_alone(ctx, faces):
    """include/faceid.h at fid_align_crops: a slot whose landmarks admit no transform gets a zero crop and an M row of NaNs"""
    from scrfd_arcface_facerecognition_amd._lib import check
    bad = degenerate_sets()
    ordinary = [0, 1, 2, 4, 5, 6]
    slots = []                                                   # ordinary, bad, ordinary, bad, ... ordinary
    for k, i in enumerate(ordinary):
        slots.append(("ok", i))
        if k < len(bad):
            slots.append(("bad", list(bad)[k]))
    assert [s[0] for s in slots].count("bad") == 5 and slots[0][0] == slots[-1][0] == "ok"
    frame = faces.frames["noise"]
    fr = ctx.to_device(frame[None])

    def run(kps):
        n = len(kps)
        kp, cn = ctx.to_device(np.asarray(kps, np.float32).reshape(1, n, 10)), ctx.to_device(np.array([n], np.int32))
        crops, M = filled(ctx, (n, 112, 112, 3)), filled(ctx, (n, 6), np.float64)
        check(ctx.lib.fid_align_crops(ctx.handle, C.c_void_p(fr.ptr), 1, H0, W0, C.c_void_p(kp.ptr), C.c_void_p(cn.ptr), n, n, C.c_void_p(crops.ptr),
                                      C.c_void_p(M.ptr)))
        return crops.download(), M.download()
    crops, M = run([faces.lms[s[1]] if s[0] == "ok" else bad[s[1]] for s in slots])
    clean_crops, clean_M = run([faces.lms[i] for i in ordinary])
    k = 0
    for j, (kind, what) in enumerate(slots):
        if kind == "bad":
            assert not crops[j].any(), what
            assert np.isnan(M[j]).all(), (what, M[j])
        else:
            assert np.array_equal(crops[j], clean_crops[k]) and np.array_equal(M[j], clean_M[k]), (j, what)
            faces.check("fid_align_crops (between degenerate slots)", "noise", what, crops[j], M[j])
            k += 1


def test_rank1_landmark_sets_on_the_device(ctx, faces):
    """collinear and two-point sets: the closed form must equal the SVD form there too, and the crop is the warp by that M"""
    from scrfd_arcface_facerecognition_amd._lib import check
    sets = sr.rank1_sets()
    n = len(sets)
    frame = faces.frames["ramp"]
    fr = ctx.to_device(frame[None])
    kp, cn = ctx.to_device(sets.reshape(1, n, 10)), ctx.to_device(np.array([n], np.int32))
    crops, M = filled(ctx, (n, 112, 112, 3)), filled(ctx, (n, 6), np.float64)
    check(ctx.lib.fid_align_crops(ctx.handle, C.c_void_p(fr.ptr), 1, H0, W0, C.c_void_p(kp.ptr), C.c_void_p(cn.ptr), n, n, C.c_void_p(crops.ptr),
                                  C.c_void_p(M.ptr)))
    crops, M = crops.download(), M.download().reshape(n, 2, 3)
    for i in range(n):
        ref, _ = align.estimate_norm(sets[i], f64=True)
        assert np.isfinite(M[i]).all() and rel_diff(M[i], ref) < 1e-9, (i, M[i], ref)
        exact, G = sr.exact_warp(frame, M[i])
        r = sr.warp_ratio(crops[i], exact, G)
        print(f"rank-1 set {i}: max |byte - exact| / bound = {r:.4f}")
        assert r <= 1.0 and crops[i].any(), (i, r)
        assert np.array_equal(crops[i], align.warp_affine(frame, M[i])), i
