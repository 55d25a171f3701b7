"""numpy restatement of the depth-image ingest (dspmap_preprocess_depth), written from its specification in include/dspmap.h, not from
the kernel: fp32 back-projection with every operation rounded on its own, leaf lattice of the voxel-grid filter over the map box,
per-leaf INTEGER sums of llrint(p * 2^20) (np.add.reduceat on int64), float64 division, axis swap, open-box crop, cap.  It is the
yardstick of tests/test_depth_cpu.py and tests/test_gpu_depth.py; the oracle's sequential fp32 filter is the cross-check.

Also the synthetic test image the checks share."""
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
    return np.stack([x, y, d], 1).astype(F), int(keep.sum())


def filter_points(pts, leaf, half, max_points):
    """camera-frame points -> dict(out [n, 3] float32 map frame, n_leaves, exact [n, 3] float64 centroids of the kept leaves (map frame),
    counts [n] pixels per kept leaf, all_counts: pixels of every occupied leaf touching the map box, absmax: largest |coordinate| summed)"""
    hx, hy, hz = (F(h) for h in half)
    hin = (hy, hz, hx)   # the map box in the camera frame: x_map = z_cam, y_map = -x_cam, z_map = -y_cam
    inv = F(1.0) / F(leaf)
    pts = np.asarray(pts, F).reshape(-1, 3)
    pts = pts[np.isfinite(pts).all(1)]
    div, idx = [], []
    inside = np.ones(len(pts), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            lo = np.floor(F(-hin[a]) * inv)
            hi = np.floor(hin[a] * inv)
            div.append(int(hi) - int(lo) + 1)
            f = (np.floor((pts[:, a] * inv).astype(F)) - F(int(lo))).astype(F)
            inside &= (f >= 0) & (f < F(div[a]))
            idx.append(f)
    pts = pts[inside]
    i0, i1, i2 = (f[inside].astype(np.int64) for f in idx)
    cell = i0 + (i1 + i2 * div[1]) * div[0]
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
