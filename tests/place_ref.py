"""numpy restatement of place recognition (include/radarays_mi355.h, rr_describe_images_device and rr_match_descriptors_device):
the ring-by-sector descriptor of a polar image in exact integers, the circular cross-correlation of descriptors over every sector
shift as one matrix product of the rolled query with the database, and the records the library forms from it in exact Python
integers."""
import numpy as np

import align_ref as A


def ring_edges(cell_begin, cell_end, R):
    L = cell_end - cell_begin
    return [cell_begin + (r * L) // R for r in range(R + 1)]


def sector_edges(n_angles, S):
    return [(j * n_angles) // S for j in range(S + 1)]


def describe(img, cell_begin, cell_end, R, S):
    """d[r][j] = floor(sum of the pixels of ring r x sector j / their number), uint8 [R][S]; from an integral image"""
    x = np.asarray(img)
    assert x.dtype == np.uint8 and x.ndim == 2
    I = np.zeros((x.shape[0] + 1, x.shape[1] + 1), np.int64)
    I[1:, 1:] = x.astype(np.int64).cumsum(axis=0).cumsum(axis=1)
    c, a = np.array(ring_edges(cell_begin, cell_end, R)), np.array(sector_edges(x.shape[1], S))
    total = I[c[1:, None], a[None, 1:]] - I[c[:-1, None], a[None, 1:]] - I[c[1:, None], a[None, :-1]] + I[c[:-1, None], a[None, :-1]]
    count = (c[1:] - c[:-1])[:, None] * (a[1:] - a[:-1])[None, :]
    assert count.min() >= 1
    return (total // count).astype(np.uint8)


def describe_literal(img, cell_begin, cell_end, R, S):
    """the same by a double loop over the rectangles"""
    x = np.asarray(img)
    n_angles, L = x.shape[1], cell_end - cell_begin
    out = np.zeros((R, S), np.uint8)
    for r in range(R):
        for j in range(S):
            rect = x[cell_begin + (r * L) // R:cell_begin + ((r + 1) * L) // R, (j * n_angles) // S:((j + 1) * n_angles) // S]
            out[r, j] = int(rect.astype(np.int64).sum()) // rect.size
    return out


def xcorr_roll(q, c):
    """the literal definition: xcorr[s] = sum(np.roll(q, s, axis=1) * c), int64 [S]"""
    q, c = np.asarray(q).astype(np.int64), np.asarray(c).astype(np.int64)
    return np.array([int((np.roll(q, s, axis=1) * c).sum()) for s in range(q.shape[1])], np.int64)


def xcorr(q, db):
    """xcorr [S][n_db] of one query [R][S] against db [n_db][R][S]: the rolled queries [S][K] times the database [K][n_db].  The
    product runs through BLAS in f64, where it is exact: every partial sum is an integer of at most 255^2 x 8192 < 2^53"""
    q, db = np.asarray(q), np.asarray(db)
    S = q.shape[1]
    rolls = np.stack([np.roll(q, s, axis=1).ravel() for s in range(S)]).astype(np.float64)
    return (rolls @ db.reshape(len(db), -1).astype(np.float64).T).astype(np.int64)


def match(queries, db, top_k):
    """-> (records [n_query][top_k] as dicts of Python integers and floats, sse uint32 [n_query][n_db], shift uint16 [n_query][n_db])"""
    queries, db = np.asarray(queries), np.asarray(db)
    assert queries.dtype == np.uint8 and db.dtype == np.uint8 and queries.ndim == 3 and db.shape[1:] == queries.shape[1:]
    K = queries.shape[1] * queries.shape[2]
    flat = db.reshape(len(db), -1).astype(np.int64)
    sc, scc = flat.sum(axis=1), (flat * flat).sum(axis=1)
    recs, sses, shifts = [], [], []
    for q in queries:
        xc = xcorr(q, db)
        top = xc.max(axis=0)
        shift = xc.argmax(axis=0)                            # the first (smallest) s that attains the maximum
        n_best = (xc == top[None, :]).sum(axis=0)
        qi = q.astype(np.int64)
        sq, sqq = int(qi.sum()), int((qi * qi).sum())
        sse = sqq + scc - 2 * top
        assert sse.min() >= 0 and sse.max() < 2 ** 31
        key = (sse << 32) | np.arange(len(db), dtype=np.int64)
        order = np.sort(key)[:top_k]                          # unique keys: the order is theirs alone
        row = []
        for kk in order:
            i = int(kk) & 0xFFFFFFFF
            row.append({"index": i, "shift": int(shift[i]), "sse": int(sse[i]), "n_best": int(n_best[i]), "xcorr": int(top[i]),
                        "ncc": A.ncc_of(K, int(top[i]), sq, sqq, int(sc[i]), int(scc[i])), "psnr": A.psnr_of(int(sse[i]), K)})
        recs.append(row)
        sses.append(sse.astype(np.uint32))
        shifts.append(shift.astype(np.uint16))
    return recs, np.stack(sses), np.stack(shifts)
