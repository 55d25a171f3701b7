"""numpy restatement of the known-space layer (include/dspmap.h, dspmap_known_integrate and the calls next to it): the window arithmetic
in float64 from the float32 position and resolution, everything a frame decides about a cell in float32 with one numpy operation per
rounding of the definition.

Independent of the kernels' structure: the layer is a dense array in WINDOW order, and moving the window copies the overlap of the old and
the new window into a fresh array of zeros -- no slots, no modulo.  The plane normals and the farthest returns come from the map
(DSPMap.view()); plane_normals() / bin_cloud() build them on the host for the tests that have no device."""
import math

import numpy as np

F = np.float32
NEVER = -1


def dims(cfg):
    return F(cfg.voxel_resolution), (int(cfg.nx), int(cfg.ny), int(cfg.nz))


def pyramid_counts(cfg):
    a = int(cfg.angle_resolution)
    return 2 * int(cfg.half_fov_h) // a, 2 * int(cfg.half_fov_v) // a


# ---- the window
def window_axis(cur, res, n):
    """(k0, o) of one axis: lattice index of map voxel 0, and the centre of that cell relative to the sensor"""
    cur, res = float(F(cur)), float(F(res))
    g = cur / res - n / 2.0
    k0 = int(math.floor(g + 0.5))
    return k0, F((k0 + 0.5) * res - cur)


def window(cfg, cur_pos):
    res, n = dims(cfg)
    ko = [window_axis(cur_pos[a], res, n[a]) for a in range(3)]
    return tuple(k for k, _ in ko), tuple(o for _, o in ko)


def centres(cfg, cur_pos):
    """px [nx], py [ny], pz [nz]: p_a = fl(fl((float)i * res) + o_a)"""
    res, n = dims(cfg)
    _, o = window(cfg, cur_pos)
    return tuple(((np.arange(n[a]).astype(F) * res).astype(F) + o[a]).astype(F) for a in range(3))


# ---- the view
def dot3(x, y, z, nrm):
    """vectorMultiply :1324-1326: fl(fl(fl(x n0) + fl(y n1)) + fl(z n2))"""
    return (((x * nrm[0]).astype(F) + (y * nrm[1]).astype(F)).astype(F) + (z * nrm[2]).astype(F)).astype(F)


def pyramid_of(ph, pv, x, y, z):
    """h * np_v + v of points (float32 arrays of one shape), -1 outside the wedge: the four outer planes, then the first sign change
    found by bisection with the predicates of pyramid_of in dspmap_device.h (<= 0 horizontally, >= 0 vertically)"""
    ph, pv = np.asarray(ph, F), np.asarray(pv, F)
    x, y, z = (np.asarray(a, F) for a in (x, y, z))
    nh, nv = len(ph) - 1, len(pv) - 1
    inside = (dot3(x, y, z, ph[0]) >= 0) & (dot3(x, y, z, ph[nh]) <= 0) & (dot3(x, y, z, pv[0]) <= 0) & (dot3(x, y, z, pv[nv]) >= 0)
    out = []
    for planes, n, below in ((ph, nh, True), (pv, nv, False)):
        lo = np.zeros(x.shape, np.int64)
        hi = np.full(x.shape, n - 1, np.int64)
        while (lo < hi).any():
            act = lo < hi
            mid = (lo + hi) >> 1
            nrm = planes[np.minimum(mid + 1, n)]
            d = (((x * nrm[..., 0]).astype(F) + (y * nrm[..., 1]).astype(F)).astype(F) + (z * nrm[..., 2]).astype(F)).astype(F)
            t = (d <= 0) if below else (d >= 0)
            hi = np.where(act & t, mid, hi)
            lo = np.where(act & ~t, mid + 1, lo)
        out.append(lo)
    return np.where(inside, out[0] * nv + out[1], -1)


def pyramid_of_linear(ph, pv, x, y, z):
    """the reference's own scan (:1329-1367): the first plane at which last_dot * this_dot <= 0; for one point"""
    ph, pv = np.asarray(ph, F), np.asarray(pv, F)
    nh, nv = len(ph) - 1, len(pv) - 1
    x, y, z = (np.asarray(a, F).reshape(1) for a in (x, y, z))
    d = lambda nrm: dot3(x, y, z, nrm)[0]   # noqa: E731
    if not (d(ph[0]) >= 0 and d(ph[nh]) <= 0 and d(pv[0]) <= 0 and d(pv[nv]) >= 0):
        return -1
    idx = []
    for planes, n, last in ((ph, nh, F(1)), (pv, nv, F(-1))):
        found = -1
        for i in range(n):
            this = d(planes[i + 1])
            if F(last * this) <= 0:
                found = i
                break
            last = this
        idx.append(found)
    return idx[0] * nv + idx[1]


def classify(cfg, cur_pos, ph, pv, maxlen, occl_margin=0.3, max_range=np.inf):
    """bool [nz, ny, nx] each: (seen, occluded, beyond max_range, outside the wedge); exactly one is true per cell"""
    px, py, pz = centres(cfg, cur_pos)
    z, y, x = np.meshgrid(pz, py, px, indexing="ij")
    b = pyramid_of(ph, pv, x, y, z)
    dist = np.sqrt((((x * x).astype(F) + (y * y).astype(F)).astype(F) + (z * z).astype(F)).astype(F)).astype(F)
    ml = np.asarray(maxlen, F).reshape(-1)[np.maximum(b, 0)]
    wedge = b >= 0
    occluded = wedge & (ml > 0) & (dist > (ml + F(occl_margin)).astype(F))
    beyond = wedge & ~occluded & ~(dist <= F(max_range))
    seen = wedge & ~occluded & ~beyond
    return seen, occluded, beyond, ~wedge


class Layer:
    """the stamps of the window, [nz, ny, nx] in window order"""

    def __init__(self, cfg):
        self.cfg = cfg
        res, n = dims(cfg)
        self.n = n
        self.stamp = np.zeros((n[2], n[1], n[0]), np.int64)
        self.k0 = None

    def sync(self, cur_pos):
        """move the window: cells that stay keep their stamp, cells that enter read 0"""
        k0, _ = window(self.cfg, cur_pos)
        if self.k0 is not None and k0 != self.k0:
            new = np.zeros_like(self.stamp)
            src, dst = [], []
            for a in range(3):
                lo, hi = max(k0[a], self.k0[a]), min(k0[a], self.k0[a]) + self.n[a]      # lattice cells in both windows
                src.append(slice(lo - self.k0[a], max(hi, lo) - self.k0[a]))
                dst.append(slice(lo - k0[a], max(hi, lo) - k0[a]))
            new[dst[2], dst[1], dst[0]] = self.stamp[src[2], src[1], src[0]]
            self.stamp = new
        self.k0 = k0

    def integrate(self, cur_pos, ph, pv, maxlen, counter, occl_margin=0.3, max_range=np.inf):
        self.sync(cur_pos)
        seen = classify(self.cfg, cur_pos, ph, pv, maxlen, occl_margin, max_range)[0]
        self.stamp[seen] = int(counter)
        return seen

    def reset(self):
        self.stamp[:] = 0

    def ages(self, cur_pos, counter):
        """int32 [nz, ny, nx]"""
        self.sync(cur_pos)
        return np.where(self.stamp == 0, NEVER, int(counter) - self.stamp).astype(np.int32)


def unknown(ages, max_age):
    return (ages < 0) | (ages > int(max_age))


def stats(ages, max_age):
    return int(((ages >= 0) & (ages <= int(max_age))).sum()), int((ages == 0).sum())


def query(cfg, ages, samples, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """ages of samples [n, 4] (t ignored): the cell of dspmap_point_voxel_index's voxel; -1 outside the map or for a NaN coordinate"""
    from tests import query_ref as Q
    q = np.ascontiguousarray(samples, F).reshape(-1, 4)
    p = q[:, :3].copy()
    if world:
        p = (p - np.asarray(cur_pos, F)[None, :]).astype(F)
    nan = np.isnan(q[:, :3]).any(1)
    inside, g = Q.own_voxel(cfg, np.where(nan[:, None], F(0), p))
    return np.where(inside & ~nan, np.asarray(ages, np.int32).reshape(-1)[g], NEVER).astype(np.int32)


# ---- a host-side view for the tests without a device (the GPU tests take the device's planes and returns)
def plane_normals(cfg, quat=(1.0, 0.0, 0.0, 0.0)):
    """(ph [np_h + 1, 3], pv [np_v + 1, 3]): the normals of :563-578 rotated by the attitude (float64 rotation, rounded once)"""
    nh, nv = pyramid_counts(cfg)
    step = F(float(cfg.angle_resolution) * math.pi / 180.0)
    ih, iv = np.arange(-(nh // 2), nh // 2 + 1).astype(F), np.arange(-(nv // 2), nv // 2 + 1).astype(F)
    ph = np.stack([-np.sin(ih * step), np.cos(ih * step), np.zeros_like(ih)], 1).astype(np.float64)
    pv = np.stack([np.sin(iv * step), np.zeros_like(iv), np.cos(iv * step)], 1).astype(np.float64)
    return rotate(ph, quat).astype(F), rotate(pv, quat).astype(F)


def rotate(v, quat):
    w, x, y, z = (float(c) for c in quat)
    n = math.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.asarray(v, np.float64) @ R.T


def bin_cloud(cfg, pts, quat=(1.0, 0.0, 0.0, 0.0)):
    """(ph, pv, maxlen [np]) of a cloud in the sensor frame: the farthest return per pyramid, -1 without one (:266-277)"""
    ph, pv = plane_normals(cfg, quat)
    nh, nv = pyramid_counts(cfg)
    r = rotate(np.asarray(pts, np.float64).reshape(-1, 3), quat).astype(F)
    b = pyramid_of(ph, pv, r[:, 0], r[:, 1], r[:, 2])
    ln = np.sqrt((((r[:, 0] * r[:, 0]).astype(F) + (r[:, 1] * r[:, 1]).astype(F)).astype(F) + (r[:, 2] * r[:, 2]).astype(F)).astype(F)).astype(F)
    ml = np.full(nh * nv, F(-1), F)
    np.maximum.at(ml, b[b >= 0], ln[b >= 0])
    return ph, pv, ml
