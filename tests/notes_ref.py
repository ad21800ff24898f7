"""numpy restatement of the object annotations (include/radarays_mi355.h, rr_notes.hip).

The definition is the build's own (the reference reduces no label image): these functions state it a second time, independently of
the kernels' structure -- sorting and grouping where the kernels use tables and atomics -- and the GPU tests compare every integer
field bit for bit.  float32 where the header says f32, one rounding per operation, nothing fused."""
import numpy as np

from radarays_ros_amd.native import LABEL_NONE, NOTE_DIRECT, NOTE_DTYPE, NOTE_GHOST, NOTE_MULTIPATH


def pixel_class(info):
    """class of labelled pixels: multipath if kind is 1, otherwise ghost if pass > 0, otherwise direct"""
    i = np.asarray(info, np.uint32)
    kind, pas = (i >> np.uint32(28)) & np.uint32(1), (i >> np.uint32(24)) & np.uint32(15)
    return np.where(kind == 1, NOTE_MULTIPATH, np.where(pas > 0, NOTE_GHOST, NOTE_DIRECT)).astype(np.uint32)


def arc(occupied, n_angles):
    """(az_begin, az_count) of a set of occupied azimuths, walking the circle one azimuth at a time: the longest circular run of
    unoccupied azimuths, among equal ones the run whose first azimuth is lowest; the arc begins behind it"""
    occ = np.zeros(n_angles, bool)
    occ[list(occupied)] = True
    if occ.all():
        return 0, n_angles
    if not occ.any():
        return 0, 0
    best = None
    for start in range(n_angles):                       # a run begins where an unoccupied azimuth follows an occupied one
        if occ[start] or not occ[start - 1]:
            continue
        n = 0
        while not occ[(start + n) % n_angles]:
            n += 1
        if best is None or n > best[0]:                 # starts ascend: an equal run found later does not replace the first
            best = (n, start)
    n, start = best
    return (start + n) % n_angles, n_angles - n


def arcs_by_object(ids, az, n_objects, n_angles):
    """arc() for every object at once: ids / az of the extent pixels -> (az_begin, az_count) uint32 [n_objects]"""
    begin, count = np.zeros(n_objects, np.uint32), np.zeros(n_objects, np.uint32)
    if len(ids) == 0:
        return begin, count
    key = np.unique(ids.astype(np.int64) * n_angles + az.astype(np.int64))          # (object, azimuth) pairs, sorted
    o, a = key // n_angles, key % n_angles
    first = np.r_[True, o[1:] != o[:-1]]
    last = np.r_[o[1:] != o[:-1], True]
    # the run behind every occupied azimuth: up to the object's next occupied azimuth, from its last one round to its first
    nxt = np.r_[a[1:], 0]
    first_of = a[np.maximum.accumulate(np.where(first, np.arange(len(a)), 0))]
    length = np.where(last, first_of + n_angles - a - 1, nxt - a - 1)
    start = (a + 1) % n_angles
    order = np.lexsort((start, -length, o))             # per object: the longest run first, among equal ones the lowest start
    lead = order[np.r_[True, o[order][1:] != o[order][:-1]]]
    obj, ln, st = o[lead], length[lead], start[lead]
    begin[obj] = np.where(ln == 0, 0, (st + ln) % n_angles)
    count[obj] = n_angles - ln
    return begin, count


def annotate_frame(labels, img, n_objects, extent_mask, scroll=0, theta_min=0.0, theta_inc=-2 * np.pi / 400, resolution=0.0438):
    """one label plane [n_cells][n_angles] (image layout) and its image (or None) -> (notes NOTE_DTYPE [n_objects], skipped,
    r_ext float64 [n_objects][4]: the range of the pixel that sets x_min, x_max, y_min, y_max -- what an ulp of cosf / sinf is scaled by)"""
    labels = np.asarray(labels, np.uint32)
    N, A = labels.shape
    notes = np.zeros(n_objects, NOTE_DTYPE)
    notes["bin_min"] = 0xFFFFFFFF
    notes["x_min"] = notes["y_min"] = np.inf
    notes["x_max"] = notes["y_max"] = -np.inf
    r_ext = np.zeros((n_objects, 4))
    b, col = np.nonzero(labels != LABEL_NONE)
    info = labels[b, col]
    ids = (info & np.uint32(0xFFFFFF)).astype(np.int64)
    inside = ids < n_objects
    skipped = int((~inside).sum())
    b, col, info, ids = b[inside], col[inside], info[inside], ids[inside]
    cls = pixel_class(info)
    for name, bit in (("n_direct", NOTE_DIRECT), ("n_ghost", NOTE_GHOST), ("n_multipath", NOTE_MULTIPATH)):
        notes[name] = np.bincount(ids[cls == bit], minlength=n_objects)
    ext = (cls & np.uint32(extent_mask)) != 0
    b, col, ids = b[ext], col[ext], ids[ext]
    if len(ids) == 0:
        return notes, skipped, r_ext
    az = (col - int(scroll)) % A
    z = np.zeros(len(ids), np.int64) if img is None else np.asarray(img)[b, col].astype(np.int64)
    notes["n_extent"] = np.bincount(ids, minlength=n_objects)
    notes["sum_intensity"] = np.bincount(ids, weights=z, minlength=n_objects).astype(np.uint64)          # (exact: below 2^53)
    seen = np.flatnonzero(notes["n_extent"])

    def leaders(*keys):
        """index of every seen object's first pixel in the order (object, keys...)"""
        order = np.lexsort(tuple(reversed(keys)) + (ids,))
        return order[np.r_[True, ids[order][1:] != ids[order][:-1]]]

    notes["bin_min"][seen] = b[leaders(b)]
    notes["bin_max"][seen] = b[leaders(-b)]
    pk = leaders(-z, b, az)                             # the largest value, then the lower bin, then the lower azimuth
    notes["peak"][seen], notes["peak_bin"][seen], notes["peak_az"][seen] = z[pk], b[pk], az[pk]
    notes["az_begin"], notes["az_count"] = arcs_by_object(ids, az, n_objects, A)
    theta = np.float32(theta_min) + az.astype(np.float32) * np.float32(theta_inc)
    r = ((b.astype(np.float64) + 0.5) * float(resolution)).astype(np.float32)
    x, y = r * np.cos(theta), r * np.sin(theta)
    assert x.dtype == np.float32 and y.dtype == np.float32
    for k, (name, v) in enumerate((("x_min", x), ("x_max", -x), ("y_min", y), ("y_max", -y))):
        at = leaders(v)
        notes[name][seen] = v[at] if k % 2 == 0 else -v[at]
        r_ext[seen, k] = r[at]
    return notes, skipped, r_ext


def annotate(labels, imgs, n_objects, extent_mask, **geometry):
    """planes [n][n_cells][n_angles] -> (notes [n][n_objects], skipped uint32 [n], r_ext [n][n_objects][4])"""
    out = [annotate_frame(labels[f], None if imgs is None else imgs[f], n_objects, extent_mask, **geometry) for f in range(len(labels))]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.uint32), np.stack([o[2] for o in out])


INT_FIELDS = ("n_direct", "n_ghost", "n_multipath", "n_extent", "bin_min", "bin_max", "az_begin", "az_count", "peak", "peak_bin", "peak_az",
              "reserved0_", "sum_intensity", "reserved1_")
FLOAT_FIELDS = ("x_min", "x_max", "y_min", "y_max")


def assert_notes(got, want, r_ext):
    """every integer field bit for bit; the floats to the bound tests/test_gpu_detect.py holds a point's x and y to, 1e-6 * r + 1e-6
    with r the range of the pixel that sets the extreme (+-inf, the empty extent, exactly)"""
    assert got.shape == want.shape
    for k in INT_FIELDS:
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:8])
    for i, k in enumerate(FLOAT_FIELDS):
        g, w = got[k].astype(np.float64), want[k].astype(np.float64)
        empty = ~np.isfinite(w)
        assert np.array_equal(g[empty], w[empty]), k
        assert np.all(np.abs(g[~empty] - w[~empty]) <= 1e-6 * r_ext[..., i][~empty] + 1e-6), k
