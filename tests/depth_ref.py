"""numpy restatement of the depth-image ingest (dspmap_preprocess_depth), written from its specification in include/dspmap.h, not from
the kernel: fp32 back-projection with every operation rounded on its own, leaf lattice of the voxel-grid filter over the map box,
per-leaf INTEGER sums of llrint(p * 2^20) (np.add.reduceat on int64), float64 division, axis swap, open-box crop, cap.  It is the
yardstick of tests/test_depth_cpu.py, tests/test_gpu_depth.py and tests/test_gpu_depth_edges.py; the oracle's sequential fp32 filter is
the cross-check.

Also the synthetic test image the checks share, and (at the end) the scenes of tests/test_gpu_depth_edges.py with the two helpers that
say what a scene reaches in k_dp_accumulate: tile_census (the leaves each 64 x 16 tile touches) and forced_fallback (how many of them
cannot sit in the tile's LDS table whatever the order of the waves).  Covered that way: table overflow, probe exhaustion, crowded and
sparse tables, a lattice of 8 leaves, cropped leaves, the tiling's edge shapes, a crop face, the range limits, non-finite values."""
import numpy as np

F = np.float32
U16, F32 = 0, 1
SCALE = 2.0 ** 20


def camera_kw(**over):
    """the test camera: 640 x 480, fx = 320, fy = 326.4, cx = 319.5, cy = 239.5, millimetres, 0 .. 20 m"""
    kw = dict(width=640, height=480, fx=320.0, fy=326.4, cx=319.5, cy=239.5, depth_scale=0.001, min_depth=0.0, max_depth=20.0,
              fmt=U16, row_stride_bytes=0, pixel_step=1)
    kw.update(over)
    return kw


def make_image(width=640, height=480, seed=7, shift=0.0):
    """uint16 millimetres: a wavy wall at 3 m +- 0.5 m with 2 cm noise, a near box at 1.2 m covering 100 x 80 pixels, a patch at 9 m
    (outside the 66 x 66 x 40 @ 0.15 m map box), a lattice of zero pixels (no return), five rows of 65535 (beyond max_depth = 20 m).
    shift moves the wall's wave and the box sideways (a moving-camera sequence)."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    d = 3.0 + 0.5 * np.sin(u / width * 9.0 + 2.0 * shift) * np.cos(v / height * 5.0) + 0.02 * rng.standard_normal(u.shape)
    bx, by = int(width * 0.25 + 40 * shift), int(height * 0.4)
    d[by:by + 80, bx:bx + 100] = 1.2 + 0.005 * rng.standard_normal(d[by:by + 80, bx:bx + 100].shape)
    d[int(height * 0.1):int(height * 0.1) + 50, int(width * 0.7):int(width * 0.7) + 60] = 9.0
    img = np.clip(np.rint(d * 1000.0), 1, 65534).astype(np.uint16)
    img[::17, ::13] = 0
    img[height - 5:, :] = 65535
    return img


def make_image_f32(width=640, height=480, seed=8):
    """float32 metres with every kind of non-return: NaN, +-inf, 0, negative values"""
    img = make_image(width, height, seed).astype(F) * F(0.001)
    img[img > F(60.0)] = np.inf
    img[3::29, 5::31] = np.nan
    img[7::37, 1::23] = -np.inf
    img[11::41, 2::19] = F(-1.5)
    img[13::43, 3::17] = F(0.0)
    return img.astype(F)


def rows_of(img, kw):
    """the image as the camera's layout says: [height, width] of the format's dtype out of a buffer with padded rows"""
    dt = np.uint16 if kw["fmt"] == U16 else np.float32
    h, w = kw["height"], kw["width"]
    if not kw["row_stride_bytes"]:
        return np.asarray(img, dt).reshape(h, w)
    raw = np.frombuffer(np.ascontiguousarray(img).tobytes(), np.uint8)
    stride = kw["row_stride_bytes"]
    rows = [raw[r * stride:r * stride + w * dt().itemsize].view(dt) for r in range(h)]
    return np.stack(rows)


def pad_rows(img, stride_bytes):
    """a buffer whose rows are stride_bytes apart (padding filled with a pattern that would be a valid depth if it were read)"""
    h, w = img.shape
    buf = np.full((h, stride_bytes), 0x5A, np.uint8)
    buf[:, :w * img.itemsize] = np.ascontiguousarray(img).view(np.uint8).reshape(h, w * img.itemsize)
    return buf


def backproject(img, kw):
    """kept pixels in row-major order of the used pixels -> (camera-frame points [n, 3] float32, n_valid)"""
    pts, keep = backproject_grid(img, kw)
    return pts, int(keep.sum())


def backproject_grid(img, kw):
    """-> (camera-frame points [n, 3] float32 of the kept pixels in row-major order, keep [hs, ws] bool over the used pixels)"""
    im = rows_of(img, kw)
    step = kw["pixel_step"]
    sub = im[::step, ::step]
    vv, uu = np.meshgrid(np.arange(0, kw["height"], step), np.arange(0, kw["width"], step), indexing="ij")
    scale = F(kw["depth_scale"])
    with np.errstate(invalid="ignore", over="ignore"):
        if kw["fmt"] == U16:
            ret = sub != 0
            d = (sub.astype(F) * scale).astype(F)
        else:
            ret = np.isfinite(sub) & (sub > 0)
            d = (sub.astype(F) * scale).astype(F)
        keep = ret & (d >= F(kw["min_depth"])) & (d <= F(kw["max_depth"]))
    d = d[keep]
    u = uu[keep].astype(F)
    v = vv[keep].astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (((u - F(kw["cx"])).astype(F) * d).astype(F) / F(kw["fx"])).astype(F)
        y = (((v - F(kw["cy"])).astype(F) * d).astype(F) / F(kw["fy"])).astype(F)
    return np.stack([x, y, d], 1).astype(F), keep


def lattice(leaf, half):
    """the leaf lattice over the map box in the camera frame: -> (lo [3] float (integer values, possibly infinite), div [3] float); floats,
    so that a leaf size far too small for the box is a large or infinite number here and not a failed conversion"""
    hx, hy, hz = (F(h) for h in half)
    hin = (hy, hz, hx)   # the map box in the camera frame: x_map = z_cam, y_map = -x_cam, z_map = -y_cam
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = F(1.0) / F(leaf)
        lo = [float(np.floor(F(-h) * inv)) for h in hin]
        hi = [float(np.floor(h * inv)) for h in hin]
    return lo, [b - a + 1.0 for a, b in zip(lo, hi)]


def lattice_cells(leaf, half):
    """leaves of the lattice over the map box (float: inf for a denormal leaf)"""
    _, div = lattice(leaf, half)
    return div[0] * div[1] * div[2]


def leaf_cells(pts, leaf, half):
    """finite camera-frame points [n, 3] -> (inside [n] bool: the point's leaf touches the map box, cell [inside.sum()] int64 =
    i0 + (i1 + i2 * div1) * div0, div [3] int)"""
    lo, div = lattice(leaf, half)
    div = [int(d) for d in div]
    inv = F(1.0) / F(leaf)
    idx = []
    inside = np.ones(len(pts), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            f = (np.floor((pts[:, a] * inv).astype(F)) - F(int(lo[a]))).astype(F)
            inside &= (f >= 0) & (f < F(div[a]))
            idx.append(f)
    i0, i1, i2 = (f[inside].astype(np.int64) for f in idx)
    return inside, i0 + (i1 + i2 * div[1]) * div[0], div


def filter_points(pts, leaf, half, max_points):
    """camera-frame points -> dict(out [n, 3] float32 map frame, n_leaves, exact [n, 3] float64 centroids of the kept leaves (map frame),
    counts [n] pixels per kept leaf, all_counts: pixels of every occupied leaf touching the map box, absmax: largest |coordinate| summed)"""
    hx, hy, hz = (F(h) for h in half)
    pts = np.asarray(pts, F).reshape(-1, 3)
    pts = pts[np.isfinite(pts).all(1)]
    inside, cell, _ = leaf_cells(pts, leaf, half)
    pts = pts[inside]
    empty = dict(out=np.zeros((0, 3), F), n_leaves=0, exact=np.zeros((0, 3)), counts=np.zeros(0, np.int64), all_counts=np.zeros(0, np.int64),
                 absmax=0.0)
    if len(pts) == 0:
        return empty
    order = np.argsort(cell, kind="stable")
    cell, pts = cell[order], pts[order]
    starts = np.flatnonzero(np.r_[True, cell[1:] != cell[:-1]])
    counts = np.diff(np.r_[starts, len(cell)]).astype(np.int64)
    q = np.rint(pts.astype(np.float64) * SCALE).astype(np.int64)            # llrint: ties to even
    S = np.add.reduceat(q, starts, axis=0)                                    # integer sums: any order gives these
    cen = ((S.astype(np.float64) / counts[:, None].astype(np.float64)) * (1.0 / SCALE)).astype(F)
    exact = np.add.reduceat(pts.astype(np.float64), starts, axis=0) / counts[:, None]
    out = np.stack([cen[:, 2], -cen[:, 0], -cen[:, 1]], 1).astype(F)
    exact = np.stack([exact[:, 2], -exact[:, 0], -exact[:, 1]], 1)
    keep = (out[:, 0] > -hx) & (out[:, 0] < hx) & (out[:, 1] > -hy) & (out[:, 1] < hy) & (out[:, 2] > -hz) & (out[:, 2] < hz)
    n = min(int(keep.sum()), int(max_points))
    return dict(out=out[keep][:n], n_leaves=len(starts), exact=exact[keep][:n], counts=counts[keep][:n], all_counts=counts,
                absmax=float(np.abs(pts).max()))


def preprocess_depth(img, kw, leaf, half, max_points):
    """the whole ingest: -> (filter_points' dict, n_valid)"""
    pts, n_valid = backproject(img, kw)
    r = filter_points(pts, leaf, half, max_points)
    r["cloud"] = pts
    return r, n_valid


def face_distance(out, half):
    """smallest distance of any centroid to any face of the crop box"""
    if len(out) == 0:
        return np.inf
    h = np.asarray(half, np.float64)[None, :]
    return float(np.min(np.abs(np.abs(out.astype(np.float64)) - h)))


def oracle_bound(ref):
    """the worst-case error of a sequential fp32 sum of a leaf's points (the oracle's filter; the float atomics of the cloud path in some
    other order): every one of the n - 1 additions rounds a partial sum of magnitude <= n * max|coordinate| by half an ulp, so the
    mean is off by at most 2^-24 * max|coordinate| * n, n = the largest number of pixels in one leaf; + 2^-21 for the restatement's own
    quantisation and final rounding.  Computed from the input, never from the code under test."""
    return 2.0 ** -24 * ref["absmax"] * float(ref["all_counts"].max()) + 2.0 ** -21


# ---- coverage of k_dp_accumulate's LDS leaf table, computed from the image and the specification (never from the device's output)
TILE_W, TILE_H = 64, 16          # used pixels of a workgroup's tile (DP_TW x DP_TH)
TAB, PROBES = 512, 8             # entries of the tile's leaf table, probes of a run (DP_TAB, DP_PROBES)
HASH_MUL, HASH_SHIFT = 2654435761, 23   # home slot of a leaf: ((cell * HASH_MUL) mod 2^32) >> HASH_SHIFT


def used_shape(kw):
    """-> (ws, hs, tiles): used columns, used rows, tiles of TILE_W x TILE_H used pixels"""
    step = kw["pixel_step"]
    ws, hs = -(-kw["width"] // step), -(-kw["height"] // step)
    return ws, hs, (-(-ws // TILE_W)) * (-(-hs // TILE_H))


def tile_census(img, kw, leaf, half):
    """for every tile of TILE_W x TILE_H USED pixels (row-major over ceil(ws / TILE_W) x ceil(hs / TILE_H)): the set of distinct lattice
    cells its kept in-lattice pixels fall into, as a sorted int64 array (filter_points' cell numbers)"""
    pts, keep = backproject_grid(img, kw)
    finite = np.isfinite(pts).all(1)
    inside, cell, _ = leaf_cells(pts[finite], leaf, half)
    vv, uu = np.nonzero(keep)                      # used row / column of every kept pixel, row-major like pts
    vv, uu = vv[finite][inside], uu[finite][inside]
    ws, hs, tiles = used_shape(kw)
    assert keep.shape == (hs, ws)
    tiles_x = -(-ws // TILE_W)
    tile = (vv // TILE_H) * tiles_x + uu // TILE_W
    return [np.unique(cell[tile == t]) for t in range(tiles)]


def home_slot(cells):
    return ((np.asarray(cells, np.uint64) * np.uint64(HASH_MUL)) % np.uint64(2 ** 32)) >> np.uint64(HASH_SHIFT)


def forced_fallback(cells):
    """a lower bound on the runs of a tile that must add their sums to memory themselves, whatever the order of the waves: a leaf whose
    home slot is h can only sit in slots h .. h + PROBES - 1 (mod TAB), so the leaves whose homes lie in a cyclic interval of L slots
    share min(L + PROBES - 1, TAB) slots; the leaves beyond that number are not in the table, and each of them has at least one run.
    -> the maximum over all intervals of (leaves with home in the interval) - min(L + PROBES - 1, TAB), at least 0"""
    cells = np.unique(np.asarray(cells, np.int64))
    if len(cells) == 0:
        return 0
    per_home = np.bincount(home_slot(cells).astype(np.int64), minlength=TAB)
    pre = np.r_[0, np.cumsum(np.r_[per_home, per_home])]
    s = np.arange(TAB)[:, None]
    L = np.arange(1, TAB + 1)[None, :]
    inside = pre[s + L] - pre[s]
    return int(max(0, (inside - np.minimum(L + PROBES - 1, TAB)).max()))


def noise_image(width=192, height=48, seed=3, lo=500, hi=4500):
    """uint16 millimetres, every pixel an independent uniform depth in [lo, hi): neighbouring pixels fall into unrelated leaves"""
    return np.random.default_rng(seed).integers(lo, hi, (height, width)).astype(np.uint16)


def noise_camera(**over):
    """192 x 48 around the optical axis, the focal lengths of the test camera: 3 x 3 tiles"""
    return camera_kw(**dict(dict(width=192, height=48, cx=95.5, cy=23.5), **over))


# scenes: name -> () -> (image, camera_kw, leaf).  Fixed seeds; what each one must reach is asserted in tests/test_depth_cpu.py.
def scene_overflow():
    """more leaves in a tile than the table has entries: the fallback runs by pigeonhole"""
    return noise_image(), noise_camera(), 0.05


def scene_probe_exhaustion():
    """a tile with fewer leaves than entries whose home slots crowd: the fallback runs although the table has room"""
    return noise_image(), noise_camera(), 0.08


def scene_crowded():
    """every tile between half full and full: the fallback may or may not run, depending on the order of the waves"""
    return noise_image(), noise_camera(), 0.10


def scene_smooth():
    """the synthetic wall the suite has used so far: a few dozen leaves per tile, the table alone"""
    return make_image(), camera_kw(), 0.1


def scene_few_leaves():
    """a leaf larger than the map box: 2 x 2 x 2 leaves take all 307 200 pixels, every run is 64 lanes long, one table key per tile"""
    return noise_image(640, 480, seed=5), camera_kw(), 8.0


def scene_cropped():
    """depths up to 5.4 m in a box of 4.95 m: leaves inside the lattice whose centroid the crop drops (k_dp_emit must clear them too)"""
    return noise_image(seed=13, hi=5400), noise_camera(), 0.1


def _shape_scene(width, height, step, seed):
    return lambda: (noise_image(width, height, seed=seed), camera_kw(width=width, height=height, cx=(width - 1) / 2.0, cy=(height - 1) / 2.0,
                                                                    pixel_step=step), 0.1)


def scene_crop_face(half):
    """one pixel on the optical axis whose depth is half_x as fp32: its centroid lies ON the open box's face"""
    return (np.full((1, 1), F(half[0]), F), camera_kw(width=1, height=1, cx=0.0, cy=0.0, fmt=F32, depth_scale=1.0), 0.1)


def scene_range_limits():
    """min_depth, max_depth and their fp32 neighbours outside"""
    lo, hi = F(1.0), F(2.5)
    img = np.array([[np.nextafter(lo, F(0)), lo, hi, np.nextafter(hi, F(np.inf))]], F)
    return img, camera_kw(width=4, height=1, cx=1.5, cy=0.0, fmt=F32, depth_scale=1.0, min_depth=float(lo), max_depth=float(hi)), 0.1


def scene_nonfinite_x():
    """max_depth = +inf: 3e38 (d finite, X overflows two columns off the axis) and 1e30 (finite everywhere, far outside the lattice)"""
    img = np.array([[3e38, 1e30, 1e30, 1e30, 3e38, 3e38]], F)
    return img, camera_kw(width=6, height=1, cx=2.0, cy=0.0, fmt=F32, depth_scale=1.0, max_depth=float("inf")), 0.1


def scene_nonfinite_d():
    """depth_scale 1e30: d itself overflows to +inf and passes d <= max_depth = +inf"""
    img = np.array([[1e9, 2e9, 1e9, 3e9]], F)
    return img, camera_kw(width=4, height=1, cx=1.0, cy=0.0, fmt=F32, depth_scale=1e30, max_depth=float("inf")), 0.1


TABLE_SCENES = dict(overflow=scene_overflow, probe_exhaustion=scene_probe_exhaustion, crowded=scene_crowded, smooth=scene_smooth,
                    few_leaves=scene_few_leaves, cropped=scene_cropped)
# (width, height, pixel_step) -> (ws, hs, tiles): a second tile column of one lane, a second tile row of one row (three of the four
# waves leave at once), fewer than 64 used columns, one column, a step that leaves 92 x 69 used pixels, a step larger than the image,
# the largest step the entry points accept
SHAPES = {(65, 17, 1): (65, 17, 4), (63, 1, 1): (63, 1, 1), (1, 33, 1): (1, 33, 3), (640, 480, 7): (92, 69, 10), (640, 480, 1000): (1, 1, 1),
          (640, 480, 1 << 24): (1, 1, 1)}
SHAPE_SCENES = {"shape_%dx%d_step%d" % k: _shape_scene(*k, seed=20 + i) for i, k in enumerate(SHAPES)}
VALUE_SCENES = dict(range_limits=scene_range_limits, nonfinite_x=scene_nonfinite_x, nonfinite_d=scene_nonfinite_d)


def scenes(half):
    """every scene: name -> () -> (image, camera_kw, leaf)"""
    out = dict(TABLE_SCENES)
    out.update(SHAPE_SCENES)
    out.update(VALUE_SCENES)
    out["crop_face"] = lambda: scene_crop_face(half)
    return out
