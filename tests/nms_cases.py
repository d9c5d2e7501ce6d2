"""Candidate lists with planted suppressions for the greedy NMS of csrc/postproc.hip (nms_select), the head tensors that decode to them, and a
Python mirror of how the launcher picks nms_select's path.  tests/test_nms_cases_cpu.py holds the fixtures against the oracle alone;
tests/test_gpu_postprocess_edges.py runs them on the device.  Test infrastructure only.

nms_select takes one of three paths, chosen by the list length K and two values fid::nms_lds_bytes derives from the candidate capacity:
  "mask"        K <= 512, K <= n_box and a mask area exists: every pairwise decision as bit masks (8 words of 64 per row), one wave walks the list
  "loop_lds"    K <= n_box otherwise: the per-survivor loop, every box read from LDS
  "loop_mixed"  K > n_box: the loop, boxes of rank >= n_box read from global memory
A mistake at a seam (a word of 64, rank 512, rank n_box) is off by one word or one box, and a random list shows it only if a suppression happens to
straddle the seam: planted() puts one on every seam."""
import functools

import numpy as np

THR = 0.5                     # the IoU threshold of every planted list: the exact pair below has an overlap of exactly 0.5 in fp32
NMS_MASK_K = 512              # csrc/postproc.hip
LDS_LIMIT = 160 * 1024


def nms_regime(cand_cap, K):
    """(n_box, masks, path): fid::nms_lds_bytes(cand_cap) and the branch nms_select_frame takes for a list of K candidates"""
    cand_cap, K = int(cand_cap), int(K)
    base = (((cand_cap + 15) & ~15) + cand_cap * 8 + 15) & ~15
    masks = NMS_MASK_K * (NMS_MASK_K // 64) * 8
    room = (LDS_LIMIT - base) // 16 if base < LDS_LIMIT else 0
    with_masks = base + NMS_MASK_K * 16 + masks <= LDS_LIMIT
    n_box = min(1024, (LDS_LIMIT - base - masks) // 16) if with_masks else min(1024, room, NMS_MASK_K - 1)
    K = min(K, cand_cap)
    path = "mask" if with_masks and K <= NMS_MASK_K and K <= n_box else "loop_lds" if K <= n_box else "loop_mixed"
    return n_box, with_masks, path


def boundaries_for(cand_cap, K):
    """the ranks at which nms_select's code changes: every multiple of 64 below K, 512 and n_box where they are below K"""
    n_box = nms_regime(cand_cap, K)[0]
    return sorted(set(range(64, K, 64)) | {m for m in (NMS_MASK_K, n_box) if m < K})


# ---- the planted list ---------------------------------------------------------------------------------------------------------------------------
PITCH = 48                    # every structure lives in a cell of its own, PITCH pixels apart: nothing of one cell overlaps anything of another
COLS = 128
SHIFT_B, SHIFT_C = 5, 10      # the greedy triple: 20 x 20 boxes at x = 0, 5, 10 -> IoU(a,b) = IoU(b,c) = 15/25, IoU(a,c) = 10/30
GROUP = 6                     # a background group: one survivor and GROUP - 1 near copies of it at random lower ranks
MIN_PLANTED = 16              # shorter lists (K = 1, 2) are K disjoint boxes: no room for a pair, a triple and a last survivor


def _box(x, y, w, h):
    return [x, y, x + w - 1, y + h - 1]


def planted(K, boundaries=(), seed=0, last_suppressed=False):
    """-> (dets float32 [K,5], plan).  Row r of dets is the candidate of rank plan["rank"][r] (0 = best score).  plan lists, as ranks:
    pairs (s, m): s suppresses m, and s survives;  triples (a, b, c): a survives and suppresses b, IoU(b,c) > THR >= IoU(a,c): c survives only
    because b is gone;  exact (p, q): IoU exactly THR, both survive;  far (0, q): rank 0 suppresses q;  last = K - 1, a survivor.
    last_suppressed (for a list whose last rank IS a seam, K - 1 in boundaries): the seam's pair takes the place of the surviving last rank and of
    the seam's triple, plan["last"] is None -- the one way a wrong read of the single box past the seam can show."""
    K = int(K)
    rng = np.random.default_rng([int(seed), K])
    boxes = np.zeros((K, 4), np.int64)
    free = set(range(K))
    cell = [0]

    def origin():
        c = cell[0]
        cell[0] += 1
        return (c % COLS) * PITCH + int(rng.integers(0, 8)), (c // COLS) * PITCH + int(rng.integers(0, 8))

    def take(r):
        free.remove(r)
        return r

    def below(m):             # the best free rank under m
        return take(max(r for r in free if r < m))

    def from_(m):             # the first free rank at or above m
        return take(min(r for r in free if r >= m))

    plan = dict(pairs=[], triples=[], exact=None, far=None, last=K - 1)
    assert not last_suppressed or (K >= MIN_PLANTED and K - 1 in boundaries)
    if K >= MIN_PLANTED:
        last = None
        if last_suppressed:
            plan["last"] = None
        else:
            x, y = origin()
            last = take(K - 1)
            boxes[last] = _box(x, y, 20, 20)
        x, y = origin()
        first = take(0)
        boxes[first] = _box(x, y, 20, 20)
        seams = sorted(set(int(b) for b in boundaries))
        assert all(8 < m < K for m in seams), (seams, K)
        for m in seams:       # the pair: rank m - 1 (the best free rank under m where two seams touch) suppresses rank m
            if m == last:     # ... unless m is the last rank and survives: it is the c of the seam's triple instead
                continue
            t, s = take(m), below(m)
            x, y = origin()
            boxes[s], boxes[t] = _box(x, y, 20, 20), _box(x + 1, y, 20, 20)
            plan["pairs"].append((s, t))
        for m in seams:       # the triple a < b < m <= c
            if m == K - 1 and last_suppressed:
                continue
            c, b = (last if m == last else from_(m)), below(m)
            a = below(b)
            x, y = origin()
            boxes[a], boxes[b], boxes[c] = _box(x, y, 20, 20), _box(x + SHIFT_B, y, 20, 20), _box(x + SHIFT_C, y, 20, 20)
            plan["triples"].append((a, b, c))
        if not plan["triples"]:                                   # a list without a seam still holds one triple, around its middle
            c, b = from_(K // 2), below(K // 2)
            a = below(b)
            x, y = origin()
            boxes[a], boxes[b], boxes[c] = _box(x, y, 20, 20), _box(x + SHIFT_B, y, 20, 20), _box(x + SHIFT_C, y, 20, 20)
            plan["triples"].append((a, b, c))
        # rank 0 suppresses a candidate at the far end of the list
        q = below(K - 1)
        boxes[q] = boxes[first] + [0, 2, 0, 2]
        plan["far"] = (first, q)
        # the exact pair: inter 100, union 200
        p = from_(K // 3)
        q = from_(p)
        x, y = origin()
        boxes[p], boxes[q] = [x, y, x + 9, y + 9], [x, y, x + 9, y + 19]
        plan["exact"] = (p, q)
    # background: single boxes and groups of one survivor with its near copies, at random ranks
    rest = rng.permutation(sorted(free))
    i = 0
    while i < len(rest):
        n = GROUP if (K >= MIN_PLANTED and rng.integers(0, 8) == 0) else 1
        ranks = np.sort(rest[i:i + n])
        i += n
        x, y = origin()
        w, h = int(rng.integers(16, 25)), int(rng.integers(16, 25))
        boxes[ranks[0]] = _box(x, y, w, h)
        for r in ranks[1:]:
            boxes[r] = _box(x + int(rng.integers(0, 3)), y + int(rng.integers(1, 3)), w, h)
        plan["pairs"].extend((int(ranks[0]), int(r)) for r in ranks[1:])
    rank = rng.permutation(K)                                     # row r holds the candidate of rank rank[r]
    dets = np.zeros((K, 5), np.float32)
    dets[:, :4] = boxes[rank]
    dets[:, 4] = (0.5 + (K - rank) / 32768.0).astype(np.float32)  # multiples of 2^-15 in (0.5, 1): exact and distinct in fp32, K <= 16383
    assert K <= 16383 and len(np.unique(dets[:, 4])) == K
    plan["rank"] = rank
    return dets, plan


def planted_dets(K, boundaries=(), seed=0):
    return planted(K, boundaries, seed)[0]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
# fid_nms: cand_cap = K, so K alone picks the path
NMS_K = [(1, "mask"), (2, "mask"), (63, "mask"), (64, "mask"), (65, "mask"), (511, "mask"), (512, "mask"), (513, "loop_lds"), (1024, "loop_lds"),
         (1025, "loop_mixed"), (13653, "loop_mixed")]
# fid_scrfd_postprocess: (cand_cap, [(K, path)])
POST_CASES = [(4096, [(512, "mask"), (513, "loop_lds"), (1024, "loop_lds"), (1025, "loop_mixed")]),
              (13000, [(512, "mask"), (879, "loop_lds"), (880, "loop_mixed")]),
              (13652, [(512, "mask")]),
              (13653, [(512, "loop_mixed")]),
              (16800, [(40, "loop_lds"), (511, "loop_lds")])]
N_BOX = {4096: 1024, 13000: 879, 13652: 512, 13653: 511, 16800: 511}


def variants(cand_cap, K):
    """variant 0 is the list of the case.  Where the last rank is a seam (K = 65, 513, n_box + 1) it can only survive, and the box-blind slip of
    tests/test_nms_cases_cpu.py passes unseen: variant 1 is the same case with the last rank suppressed across the seam.  A (cand_cap, K) that
    stands alone in its row gets a variant 1 as well (another seed): the other frame of its batch of two."""
    alone = any(cc == cand_cap and len(ks) == 1 for cc, ks in POST_CASES)
    return (0, 1) if alone or (K >= MIN_PLANTED and K - 1 in boundaries_for(cand_cap, K)) else (0,)


def all_cases():
    """(cand_cap, K, path, variant): every list the GPU file runs"""
    out = [(K, K, path, v) for K, path in NMS_K for v in variants(K, K)]
    for cc, ks in POST_CASES:
        out += [(cc, K, path, v) for K, path in ks for v in variants(cc, K)]
    return out


@functools.lru_cache(maxsize=None)
def case(cand_cap, K, variant=0):
    """the planted list of a case, built once: (dets, plan).  Treat both as read-only.  The seed is the variant: tests/test_nms_cases_cpu.py
    holds every list to the share-kept condition (a quarter to three quarters survive), and seeds 0 and 1 meet it for every case."""
    seams = boundaries_for(cand_cap, K)
    dets, plan = planted(K, seams, seed=variant, last_suppressed=variant == 1 and K - 1 in seams)
    dets.setflags(write=False)
    return dets, plan


@functools.lru_cache(maxsize=None)
def oracle_keep(cand_cap, K, variant=0):
    """oracle.postprocess.nms of a case at THR, computed once (the K = 13653 list takes seconds): a tuple of rows of the case's dets"""
    from oracle import postprocess as pp
    return tuple(int(i) for i in pp.nms(case(cand_cap, K, variant)[0], THR))


# ---- heads --------------------------------------------------------------------------------------------------------------------------------------
def empty_heads(in_hw, score=0.125):
    """nine head arrays of a detector input of in_hw = (in_h, in_w) with no candidate: the ONNX output order, 2 anchors per pixel"""
    ns = [(in_hw[0] // s) * (in_hw[1] // s) * 2 for s in (8, 16, 32)]
    return ([np.full((n, 1), score, np.float32) for n in ns] + [np.zeros((n, 4), np.float32) for n in ns]
            + [np.zeros((n, 10), np.float32) for n in ns])


def heads_from_dets(dets, in_hw=(640, 640), seed=0):
    """Nine head arrays that decode, at img_hw == in_hw (det_scale 1), to exactly the boxes and scores of dets: det r sits at a stride-8 anchor of
    its own and its four distances are (anchor centre -+ coordinate) / 8, multiples of 1/8, so distance * 8 and centre -+ that are exact in fp32.
    The landmarks are random multiples of 1/8.  Every other anchor scores 0.125."""
    dets = np.asarray(dets, np.float32)
    K = len(dets)
    fh, fw = in_hw[0] // 8, in_hw[1] // 8
    assert K <= fh * fw * 2 and np.array_equal(dets[:, :4], np.round(dets[:, :4]))
    rng = np.random.default_rng([int(seed), K, 77])
    heads = empty_heads(in_hw)
    anchors = rng.choice(fh * fw * 2, K, replace=False)
    pix = anchors // 2
    cx, cy = ((pix % fw) * 8).astype(np.float64), ((pix // fw) * 8).astype(np.float64)
    d = np.stack([cx - dets[:, 0], cy - dets[:, 1], dets[:, 2] - cx, dets[:, 3] - cy], axis=1) / 8.0
    heads[0][anchors, 0] = dets[:, 4]
    heads[3][anchors] = d.astype(np.float32)
    heads[6][anchors] = (rng.integers(-64, 65, (K, 10)) / 8.0).astype(np.float32)
    assert np.array_equal(heads[3][anchors].astype(np.float64), d)
    return heads
