"""Oracle for fid_pair_verify / FaceAnalysis.compare_pairs / process_face_comparisons: the reference's verification workflow
(smart_face_recognition.py:878-982, :1023-1143) restated in numpy.  Test infrastructure only; no test in this file.

Probe rows: k entries of +-1 (k = 64, or 4 when dim < 64), the rest 0.  Every product is 0 or +-1, every partial sum a small integer, each
norm exactly sqrt(k) = 8 (or 2) and norm * norm exactly k, a power of two: the cosine is dot / k, a multiple of 1 / k, exact in fp32 under ANY
summation order -- the project's usual probe (tests/exact_probe.py)."""
import numpy as np

DIFFERENT, SAME, NO_IMAGE, NO_FACE = 0, 1, 2, 3                         # FID_PAIR_* (include/faceid.h)
ERR_NO_IMAGE = "Could not download one or both images"                  # :900
ERR_NO_FACE = "Could not detect faces in one or both images"            # :919


# ---- :965-982 calculate_face_similarity ----------------------------------------------------------------------

def similarity(face1, face2):
    """:978 as it stands: the dtype of the inputs decides the arithmetic (fp32 embeddings -> fp32 dot, norms, product and quotient)"""
    return np.dot(face1, face2) / (np.linalg.norm(face1) * np.linalg.norm(face2))


def similarity64(face1, face2):
    """the same formula in float64: the yardstick (0 / 0 -> NaN, silently)"""
    a, b = np.asarray(face1, np.float64), np.asarray(face2, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float64(np.dot(a, b)) / (np.sqrt(np.dot(a, a)) * np.sqrt(np.dot(b, b)))


# ---- :928-943 and the two error returns :896-903, :915-922 -----------------------------------------------------

def compare(img1_present, img2_present, emb1, emb2, thresh):
    """compare_face_images after the downloads and app.get: emb = faces[0].embedding, or None when len(faces) == 0"""
    if not img1_present or not img2_present:                                                   # :896
        return {"same_person": False, "confidence": 0.0, "error": ERR_NO_IMAGE}
    if emb1 is None or emb2 is None:                                                           # :915
        return {"same_person": False, "confidence": 0.0, "error": ERR_NO_FACE}
    sim = similarity64(emb1, emb2)                                                             # :929
    return {"same_person": bool(sim > thresh), "confidence": float(sim), "threshold_used": thresh, "error": None}   # :932, :936-943


# ---- :1088-1122 the counters and the summary of process_face_comparisons -----------------------------------------

def summary(records, comparisons):
    """records: the API's comparison records (only `approve` is read here); comparisons: compare()'s dict per record"""
    results, same, different, errors = [], 0, 0, 0
    for record, c in zip(records, comparisons):
        results.append({"api_approve": record["approve"], "our_result": c["same_person"], "error": c["error"],
                        "match_status": "SAME" if c["same_person"] else "DIFFERENT",           # :1081
                        "api_vs_our_match": record["approve"] == c["same_person"]})            # :1082
        if c["error"]:                                                                         # :1089-1094
            errors += 1
        elif c["same_person"]:
            same += 1
        else:
            different += 1
    api_matches = sum(1 for r in results if r.get("api_vs_our_match") is True)                 # :1108
    total_with_api_data = sum(1 for r in results if "api_vs_our_match" in r and r["api_vs_our_match"] is not None)   # :1109
    accuracy = (api_matches / total_with_api_data * 100) if total_with_api_data > 0 else 0     # :1110
    return {"total_comparisons": len(records), "processed": len(results), "same_person": same, "different_person": different, "errors": errors,
            "accuracy_vs_api": accuracy, "api_matches": api_matches, "total_with_api_data": total_with_api_data, "results": results}


# ---- the entry point's contract (include/faceid.h) on top of the three pieces above ------------------------------

def side_row(e, n_rows, offsets=None, n_img=0):
    """one entry of the pair table -> a row of emb, or -1 (no image) / -2 (no face)"""
    e = int(e)
    if offsets is None:
        return -1 if e == -1 else (e if 0 <= e < n_rows else -2)
    if e < 0 or e >= n_img:
        return -1
    o0, o1 = int(offsets[e]), int(offsets[e + 1])
    return o0 if (o1 > o0 and 0 <= o0 < n_rows) else -2


def verify(emb, n_rows, pairs, thresh, offsets=None, n_img=0, labels=None):
    """-> score float64 [P] (float64 formula; 0 for an error pair), verdict int32 [P], counters int64 [8] as ONE call adds them.  thresh is
    compared as the float32 the entry point receives; rows >= n_rows of `emb` are never touched."""
    t = float(np.float32(thresh))
    P = len(pairs)
    score, verdict, counters = np.zeros(P, np.float64), np.zeros(P, np.int32), np.zeros(8, np.int64)
    for p, (ea, eb) in enumerate(pairs):
        ra, rb = side_row(ea, n_rows, offsets, n_img), side_row(eb, n_rows, offsets, n_img)
        c = compare(ra != -1, rb != -1, emb[ra] if ra >= 0 else None, emb[rb] if rb >= 0 else None, t)
        score[p] = c["confidence"]
        verdict[p] = NO_IMAGE if c["error"] == ERR_NO_IMAGE else NO_FACE if c["error"] == ERR_NO_FACE else SAME if c["same_person"] else DIFFERENT
        counters[0] += 1
        counters[(2, 1, 3, 4)[verdict[p]]] += 1
        if labels is not None and labels[p] in (0, 1):
            counters[5] += 1
            counters[6] += int(bool(labels[p]) == c["same_person"])                            # :1082: an error pair is "not the same person"
    return score, verdict, counters


# ---- probes ------------------------------------------------------------------------------------------------------

def probe_k(dim):
    return 64 if dim >= 64 else 4


def probe_rows(n, dim, rng):
    """n probe rows; the first and the last element are always part of the support (the last float4 of a row takes part in every cosine)"""
    k = probe_k(dim)
    assert dim >= k
    rows = np.zeros((n, dim), np.float32)
    for r in rows:
        sup = np.concatenate([[0, dim - 1], 1 + rng.choice(dim - 2, k - 2, replace=False)]) if dim > k else np.arange(dim)
        r[sup] = rng.choice(np.float32([-1, 1]), k)
    return rows


def probe_partner(row, num, rng):
    """a probe row on the support of `row` whose cosine with it is exactly num / k (num and k of one parity)"""
    sup = np.flatnonzero(row)
    k = len(sup)
    assert -k <= num <= k and (k + num) % 2 == 0
    out = row.copy()
    flip = rng.choice(sup, (k - num) // 2, replace=False)
    out[flip] = -out[flip]
    return out
