"""Oracle for fid_gallery_group: the reference's visit loop (smart_face_recognition.py:1769-1951) restated in float64 on the fp16 rows the device
holds.  Test infrastructure only; no test in this file.

The reference's three searches -- is_duplicate_image's k = 1 (:2632-2641), search_person's k = 5 (:1619-1643) -- all read the same first hit, the
best stored row; `oracle.match.search_similar` / `is_duplicate_embedding` state their semantics (score >= threshold kept, best first, a stable
sort = the lowest row among equal scores) and `best()` below is that first hit.  They are not called as they stand because they re-normalise
their inputs in float64, which moves a cosine of unit fp16 rows in the last places (and divides a free, all-zero row by zero): the device
multiplies the fp16 rows it stores, so the oracle does too, and on the exact probe rows the two agree anyway (test_visit_group_cpu checks that)."""
import numpy as np

NEW, RECOGNISED, DUPLICATE, NO_FACE, DEFERRED = 0, 1, 2, 3, 4          # FID_VISIT_* (include/faceid.h)


def best(store64, q64):
    """(row, score) of the first hit of search_similar(k >= 1, threshold -> 0+): maximum cosine, lowest row among equal scores; a score that is
    not > 0 is no hit (row -1, score 0) -- the rule of fid_match / fid_gallery_topk (a free row is all zero and scores 0)"""
    s = store64 @ q64
    j = int(np.argmax(s))                                    # the first maximum
    return (j, float(s[j])) if s[j] > 0 else (-1, 0.0)


def group_visits(store_rows16, queries16, new_rows, dup, group, search):
    """-> verdict int32 [n], row int32 [n], score float64 [n], summary (number of NEW, first DEFERRED visit or n), the store's fp16 rows after
    the call.  store_rows16 [G, dim] fp16 as stored (free rows zero), queries16 [n, dim] unit fp16 in visit order, new_rows: the free rows
    the k-th new person is written to.  The thresholds are compared as the float32 values the entry point receives."""
    dup, group, search = (float(np.float32(t)) for t in (dup, group, search))
    store16 = np.array(store_rows16, dtype=np.float16, copy=True)
    store = store16.astype(np.float64)                       # the vector store: qdrant_manager.py's collection
    Q = np.asarray(queries16, np.float16).astype(np.float64)
    n, G = len(Q), len(store)
    verdict = np.empty(n, np.int32)
    row = np.full(n, -1, np.int32)
    score = np.zeros(n, np.float64)
    k, first_deferred = 0, n
    for i in range(n):                                       # `for i, visit in enumerate(visits)`, max_workers = 1 (:1769, :1953-1965)
        if not np.any(Q[i] != 0):                            # `if embedding_data is None` -> no_faces (:1796-1801): no face, or a degenerate embedding
            verdict[i] = NO_FACE
            continue
        if first_deferred < n:                               # (no reference analogue: the store's room ran out earlier in this call)
            verdict[i] = DEFERRED
            continue
        r, s = best(store, Q[i])
        if r >= 0 and s >= dup:                              # is_duplicate_image: `len(results) > 0` of a k = 1 search at score_threshold (:2636-2645)
            verdict[i], row[i], score[i] = DUPLICATE, r, s
            continue
        found = r >= 0 and s >= search                       # search_person: search_similar(k = 5, threshold = similarity_threshold) (:1619-1643, :1854)
        similarity = s if found else 0.0                     # `search_results[0]['similarity'] if search_results else 0.0` (:1855)
        if found and similarity >= group:                    # `if search_results and similarity >= grouping_threshold` (:1861)
            verdict[i], row[i], score[i] = RECOGNISED, r, s  # grouped with best_match (:1863-1864); nothing is stored
            continue
        if k >= len(new_rows):                               # add_person has no row left
            verdict[i], first_deferred = DEFERRED, i
            continue
        verdict[i], score[i] = NEW, similarity               # add_person (:1531-1602) -> vector_db.add_embedding (qdrant_manager.py:91-136)
        nr = int(new_rows[k])
        k += 1
        if 0 <= nr < G:                                      # (a row outside the store: nothing is written, the visit is nobody's candidate)
            row[i] = nr
            store16[nr] = np.asarray(queries16, np.float16)[i]
            store[nr] = Q[i]
    return verdict, row, score, (k, first_deferred), store16
