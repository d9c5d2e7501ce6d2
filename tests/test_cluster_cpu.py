"""CPU: the clustering rule (tests/cluster_oracle.py, what fid_gallery_cluster computes) against sklearn's DBSCAN and scipy's connected
components, its independence of the order of the rows, and the host twin (fid_cluster_host, utils.helpers.cluster_embeddings) against the oracle
bit for bit on the exact probe stores of tests/cluster_cases.py."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as K
import cluster_oracle as O
from dedup_oracle import walk


def random_hits(rng, n, p):
    """a random symmetric 0/1 hit matrix with a unit diagonal, as scores 1.0 / 0.25"""
    h = np.triu(rng.random((n, n)) < p, 1)
    h = h | h.T | np.eye(n, dtype=bool)
    return np.where(h, np.float32(1.0), np.float32(0.25))


def blobs(rng, sizes, bridges=0):
    """dense groups with a few hits between consecutive groups"""
    n = sum(sizes)
    h = np.eye(n, dtype=bool)
    at = 0
    starts = []
    for s in sizes:
        blk = np.triu(rng.random((s, s)) < 0.6, 1)
        h[at:at + s, at:at + s] |= blk | blk.T
        starts.append(at)
        at += s
    for a, b in zip(starts, starts[1:]):
        for _ in range(bridges):
            h[a + int(rng.integers(0, 3)), b + int(rng.integers(0, 3))] = True
    h = h | h.T
    return np.where(h, np.float32(1.0), np.float32(0.25))


# ---- the oracle against independent implementations ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_pts", [1, 2, 3, 5])
def test_oracle_against_sklearn_dbscan(min_pts):
    """D = 1 - hit is a 0 / 1 matrix, so eps = 0.5 has no rounding question.  The noise set and the partition of the cores must be equal; borders
    only where each touches one cluster (DBSCAN hands a contested border to the cluster that reaches it first, the rule to the best score)."""
    DBSCAN = pytest.importorskip("sklearn.cluster").DBSCAN
    rng = np.random.default_rng(min_pts)
    seen_border = 0
    for trial in range(12):
        n = int(rng.integers(5, 90))
        S = random_hits(rng, n, rng.uniform(0.01, 0.12)) if trial % 2 else blobs(rng, [int(s) for s in rng.integers(2, 12, 6)], trial % 3)
        n = len(S)
        part = np.ones(n, bool)
        label, degree, via, score, summary = O.cluster_scores(S, part, 0.5, min_pts)
        hit = S >= 0.5
        db = DBSCAN(eps=0.5, min_samples=min_pts, metric="precomputed").fit(1.0 - hit.astype(np.float64))
        core = np.zeros(n, bool)
        core[db.core_sample_indices_] = True
        assert np.array_equal(core, degree >= min_pts)
        assert np.array_equal(db.labels_ < 0, label < 0)                               # the noise set
        assert {frozenset(np.nonzero((db.labels_ == l) & core)[0].tolist()) for l in set(db.labels_[core])} == \
               {frozenset(np.nonzero((label == l) & core)[0].tolist()) for l in set(label[core])}
        for k in np.nonzero(~core & (label >= 0))[0]:
            touched = {int(label[c]) for c in np.nonzero(hit[k] & core)[0]}
            if len(touched) == 1:                                                       # an uncontested border
                seen_border += 1
                assert db.labels_[via[k]] == db.labels_[k]
        assert summary[0] == len(set(db.labels_[db.labels_ >= 0])) and summary[3] == int((db.labels_ < 0).sum())
    assert min_pts < 3 or seen_border > 5


def test_oracle_with_one_sample_is_connected_components():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(7)
    for trial in range(10):
        n = int(rng.integers(2, 120))
        S = random_hits(rng, n, rng.uniform(0.005, 0.05))
        part = rng.random(n) < 0.9
        label, degree, via, score, summary = O.cluster_scores(S, part, 0.5, 1)
        hit = (S >= 0.5) & part[:, None] & part[None, :]
        ncomp, comp = csgraph.connected_components(hit, directed=False)
        for k in np.nonzero(part)[0]:
            assert label[k] == np.nonzero(part & (comp == comp[k]))[0][0]              # the lowest position of its component
        assert (label[~part] == -1).all() and (degree[~part] == 0).all()
        assert summary == (len(set(comp[part])), int(part.sum()), 0, 0, int(part.sum()), 0)


def test_relabelling_positions_permutes_the_partition_and_nothing_else():
    rng = np.random.default_rng(3)
    for min_pts in (1, 2, 3, 4):
        S = blobs(rng, [9, 4, 1, 12, 7], 1)
        # distinct scores inside the hits, so that no via is decided by the position of its candidates
        n = len(S)
        noise = np.triu(rng.permutation(n * n).reshape(n, n).astype(np.float32) / np.float32(4 * n * n), 1)
        S = np.where(S >= 0.5, np.float32(0.5) + noise + noise.T, S).astype(np.float32)
        part = rng.random(n) < 0.95
        base = O.cluster_scores(S, part, 0.5, min_pts)
        for _ in range(4):
            perm = rng.permutation(n)                                                   # new position k holds old position perm[k]
            got = O.cluster_scores(S[np.ix_(perm, perm)], part[perm], 0.5, min_pts)
            old_of = lambda s: frozenset(int(perm[k]) for k in s)
            assert {old_of(s) for s in O.partition(got[0])} == O.partition(base[0])
            assert np.array_equal(got[1], base[1][perm]) and got[4] == base[4]
            assert np.array_equal(got[3].view(np.uint32), base[3][perm].view(np.uint32))
            assert np.array_equal(np.where(got[2] >= 0, perm[got[2]], -1), base[2][perm])


def test_a_chain_is_one_cluster_whatever_the_ids_while_the_greedy_walk_depends_on_them():
    """A ~ B ~ C with A !~ C: fid_gallery_dedup's walk keeps {A} and {C} apart or together depending on which id is lowest"""
    persons, parts = [], []
    for order in ((1, 2, 3), (2, 1, 3)):                                                # the ids of A, B, C
        x, name_of = K.chain_case(order)
        g16 = K.unit_f16(x)
        keeper, _, _ = walk(g16, np.arange(3), 0.75)
        groups = {}
        for k in range(3):
            groups.setdefault(k if keeper[k] < 0 else int(keeper[k]), set()).add(name_of[k])
        persons.append({frozenset(v) for v in groups.values()})
        label = O.cluster(g16, None, 0.75, 2)[0]
        parts.append({frozenset(name_of[k] for k in s) for s in O.partition(label)})
    assert persons[0] == {frozenset("AB"), frozenset("C")} and persons[1] == {frozenset("ABC")}
    assert parts[0] == parts[1] == {frozenset("ABC")}


# ---- the host twin ---------------------------------------------------------------------------------------------------------------------------------
def host_call(g16, rows, thresh, min_pts, n=None):
    """fid_cluster_host -> (rc, (label, degree, via, score, summary))"""
    from scrfd_arcface_facerecognition_amd import _lib
    g16 = np.ascontiguousarray(g16, np.float16)
    G, dim = g16.shape
    n = (G if rows is None else len(rows)) if n is None else n
    m = max(n, 1)
    outs = (np.full(m, 77, np.int32), np.full(m, 77, np.int32), np.full(m, 77, np.int32), np.full(m, 77, np.float32), np.full(6, 77, np.int32))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    r = None if rows is None else np.ascontiguousarray(rows, np.int32)
    rc = _lib.load().fid_cluster_host(p(g16), G, dim, None if r is None else p(r), n, C.c_float(thresh), min_pts, *[p(o) for o in outs])
    return rc, outs


@pytest.mark.parametrize("n, dim", K.PROBE_SHAPES)
def test_host_twin_equals_the_oracle_on_the_probe_stores(n, dim):
    from utils.helpers import cluster_embeddings
    g, rows, plants = K.probe_case(n, dim)
    g16 = K.unit_f16(g)
    found = 0
    for thresh in (0.75, K.ABOVE):
        for min_pts in (1, 2, 3):
            want = O.cluster(g16, rows, thresh, min_pts)
            rc, got = host_call(g16, rows, thresh, min_pts)
            assert rc == 0 and K.same(got, want) is None, (thresh, min_pts, K.same(got, want))
            found += want[4][0]
            all_rows = O.cluster(g16, None, thresh, min_pts)
            res = cluster_embeddings(g * 3.0, thresh, min_pts)                          # (any scale: the helper normalises)
            assert K.same((res.label_pos, res.degree_pos, res.via_pos, res.score_pos, res.summary), all_rows) is None
            assert res.counts["clusters"] == len(res.clusters) == all_rows[4][0] and len(res.noise) == all_rows[4][3]
    if "far" in plants:
        assert O.cluster(g16, rows, 0.75, 1)[0][290] == O.cluster(g16, rows, 0.75, 1)[0][5]            # exactly at the threshold, two blocks apart
        assert O.cluster(g16, rows, K.ABOVE, 1)[3][290] != 0.75
    assert n == 1 or found > 0


def test_host_twin_on_paths_ties_and_rows_that_take_no_part():
    g, rows, t_of = K.path_case(300, 512)
    g16 = K.unit_f16(g)
    for thresh, min_pts, summary in ((0.75, 3, (1, 298, 2, 0, 300, 0)), (0.75, 2, (1, 300, 0, 0, 300, 0)), (K.ABOVE, 3, (0, 0, 0, 300, 300, 0)),
                                     (K.ABOVE, 1, (300, 300, 0, 0, 300, 0))):
        want = O.cluster(g16, rows, thresh, min_pts)
        assert want[4] == summary
        rc, got = host_call(g16, rows, thresh, min_pts)
        assert rc == 0 and K.same(got, want) is None
    label = O.cluster(g16, rows, 0.75, 3)[0]
    assert t_of[0] == 0 and (label == label[0]).all() and label[0] != 0                 # the lowest CORE position, not the lowest position
    for equal in (True, False):
        for p_low in (True, False):
            g, rows, pos = K.tie_case(equal, p_low)
            g16 = K.unit_f16(g)
            want = O.cluster(g16, rows, 0.625, 4)
            assert want[4] == (2, 2, 5, 0, 7, 0)
            assert want[2][pos["x"]] == (min(pos["P"], pos["Q"]) if equal else pos["P"])
            assert want[3][pos["x"]] == (0.75 if equal else 0.875) and want[0][pos["x"]] == want[2][pos["x"]]
            rc, got = host_call(g16, rows, 0.625, 4)
            assert rc == 0 and K.same(got, want) is None
            assert (got[0][rows < 0] == -1).all() and (got[1][(rows < 0) | (rows >= len(g))] == 0).all()


def test_host_twin_argument_checks_write_nothing():
    g16 = K.unit_f16(K.probe_case(17, 32)[0])
    rows = np.arange(17, dtype=np.int32)
    for thresh, min_pts, n in ((float("nan"), 2, None), (0.0, 2, None), (-0.5, 2, None), (0.75, 0, None), (0.75, 2, 0), (0.75, 2, -3),
                               (0.75, 2, (1 << 20) + 1)):
        rc, outs = host_call(g16, rows, thresh, min_pts, n)
        assert rc == -1, (thresh, min_pts, n)
        assert (outs[0] == 77).all() and (outs[1] == 77).all() and (outs[2] == 77).all() and (outs[3] == 77).all() and (outs[4] == 77).all()


def test_cluster_result_names_clusters_by_ids():
    from scrfd_arcface_facerecognition_amd.engine import ClusterResult, cluster_result
    ids = ["a", "b", "c", "d", "e"]
    res = ClusterResult(ids, [1, 1, -1, 1, -1], [2, 3, 1, 2, 0], [1, 3, -1, 1, -1], [0.5, 0.75, 0, 0.75, 0], [1, 1, 2, 1, 4, 0])
    assert res.labels == {"a": "b", "b": "b", "c": None, "d": "b", "e": None}
    assert res.clusters == [["a", "b", "d"]] and res.noise == ["c"] and res.degree["e"] == 0
    assert res.via == {"a": ("b", 0.5), "b": ("d", 0.75), "d": ("b", 0.75)}
    assert res.counts == {"clusters": 1, "cores": 1, "borders": 2, "noise": 1, "took_part": 4}
    with pytest.raises(RuntimeError):
        cluster_result(ids, [0] * 5, [0] * 5, [0] * 5, [0] * 5, [0, 0, 0, 0, 0, 1])
