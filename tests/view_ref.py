"""numpy restatement of the viewpoint scores (include/dspmap.h, dspmap_score_views), built from what is there: the rays are casts of
tests/cast_ref.cast with ta = tb, the wedge is tests/known_ref.pyramid_of, the distance and the occlusion rule are the expressions of
known_ref.classify, the voxel centres and the view's own voxel are those of tests/query_ref -- one numpy float32 operation per rounding
of the definition.

Independent of the kernel's structure: no chunks, no boxes, no words -- every view classifies every voxel of the map in dense [nz, ny, nx]
arrays, and the rays of all views go through one vectorised cast.  The rotated planes and ray directions are INPUTS (`rays`: a function
quaternion -> (planes_h, planes_v, dirs)): the GPU tests hand in what the device makes of an attitude (DSPMap.view_rays), the tests
without a device use host_rays() below, which rotates in float64."""
import math

import numpy as np

from tests import cast_ref as CR
from tests import known_ref as K
from tests import query_ref as Q

F = np.float32
SCORE_DTYPE = np.dtype([("n_seen", "i4"), ("n_unknown", "i4"), ("n_returns", "i4"), ("status", "i4")])
OK, BLOCKED, OUTSIDE, INVALID = 0, 1, 3, 4
FLT_MAX = np.finfo(F).max


def directions0(cfg):
    """[np_h * np_v, 3] float32: the unrotated central direction of every pyramid b = h * np_v + v, in float64, rounded once"""
    nh, nv = K.pyramid_counts(cfg)
    step = float(cfg.angle_resolution) * math.pi / 180.0
    al = (np.arange(nh) - nh / 2.0 + 0.5) * step
    be = -(np.arange(nv) - nv / 2.0 + 0.5) * step
    y, z = np.meshgrid(np.tan(al), np.tan(be), indexing="ij")
    d = np.stack([np.ones_like(y), y, z], -1).reshape(-1, 3)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def directions(cfg, quat=(1.0, 0.0, 0.0, 0.0)):
    """the central directions rotated by the attitude (float64 rotation of the float32 table, rounded once)"""
    return K.rotate(directions0(cfg).astype(np.float64), quat).astype(F)


def host_rays(cfg):
    """rays(quat) for the tests without a device"""
    return lambda quat: K.plane_normals(cfg, quat) + (directions(cfg, quat),)


def centres(cfg):
    """cx [nx], cy [ny], cz [nz]: dspmap_voxel_center, fl(fl((float)i * res) + corr)"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    return tuple(((np.arange(n[a]).astype(F) * res).astype(F) + corr[a]).astype(F) for a in range(3))


def _length(x, y, z):
    return np.sqrt((((x * x).astype(F) + (y * y).astype(F)).astype(F) + (z * z).astype(F)).astype(F)).astype(F)


def layer_of(cfg, t):
    """the ONE layer a view's t selects: 0 for t < 0 or T == 0, else 1 + k(t)"""
    T, pred = Q._dims(cfg)[:2]
    return int(Q.horizons(pred, np.array([t], F))[0]) + 1


def statuses(cfg, lay, views, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """(status [n], p [n, 3] map-frame positions, cell [n, 3] own cell (x, y, z), layer [n]); step 1 of the definition"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    v = np.ascontiguousarray(views, F).reshape(-1, 9)
    st = np.full(len(v), OK, np.int32)
    with np.errstate(all="ignore"):
        q = v[:, 3:7]
        n2 = (((((q[:, 1] * q[:, 1]).astype(F) + (q[:, 2] * q[:, 2]).astype(F)).astype(F) + (q[:, 3] * q[:, 3]).astype(F)).astype(F)
               + (q[:, 0] * q[:, 0]).astype(F)).astype(F))
        invalid = ~np.isfinite(v[:, 0:7]).all(1) | (n2 == 0) | np.isnan(v[:, 8]) | ~(v[:, 7] > 0)
        p = v[:, 0:3].copy()
        if world:
            p = (p - np.asarray(cur_pos, F)[None, :]).astype(F)
        hv = np.array(half, F)[None, :]
        inside = ~invalid & (np.abs(p) < hv).all(1)
        u = ((p + hv).astype(F) / res).astype(F)
        cell = np.trunc(np.where(inside[:, None], u, F(0))).astype(np.int64)
        inside &= (cell < np.array(n)[None, :]).all(1)
    layer = np.zeros(len(v), np.int64)
    st[invalid] = INVALID
    st[~invalid & ~inside] = OUTSIDE
    for i in np.flatnonzero(inside):
        layer[i] = layer_of(cfg, v[i, 8])
        if lay[layer[i], cell[i, 2], cell[i, 1], cell[i, 0]]:
            st[i] = BLOCKED
    return st, p, cell, layer


def score(cfg, lay, ages, views, max_age, rays, occl_margin=0.3, world=False, cur_pos=(0.0, 0.0, 0.0), details=False):
    """SCORE_DTYPE [n] of views [n, 9] = {x, y, z, qw, qx, qy, qz, max_range, t} through bool layers [L, nz, ny, nx] with ages
    [nz, ny, nx]; rays(quat) -> (planes_h, planes_v, dirs).  details: also a dict per OK view index with the bool grids seen / occluded /
    beyond [nz, ny, nx], ml [NP] and the cast status of every ray"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    lay = np.asarray(lay, bool)
    ages = np.asarray(ages).reshape(n[2], n[1], n[0])
    unknown = K.unknown(ages, max_age)
    v = np.ascontiguousarray(views, F).reshape(-1, 9)
    out = np.zeros(len(v), SCORE_DTYPE)
    st, p, cell, layer = statuses(cfg, lay, v, world, cur_pos)
    out["status"] = st
    ok = np.flatnonzero(st == OK)
    info = {}
    if ok.size == 0:
        return (out, info) if details else out
    cache = {}
    for i in ok:
        key = v[i, 3:7].tobytes()
        if key not in cache:
            cache[key] = tuple(np.asarray(a, F) for a in rays(tuple(float(c) for c in v[i, 3:7])))
    # ---- the rays of every OK view in one cast: a = p, b = fl(p + fl(d * l)), ta = tb = min(t, FLT_MAX)
    NP = len(next(iter(cache.values()))[2])
    reach = F(res * F(n[0] + n[1] + n[2]))
    seg = np.zeros((ok.size, NP, 8), F)
    with np.errstate(all="ignore"):
        for j, i in enumerate(ok):
            dirs = cache[v[i, 3:7].tobytes()][2]
            ell = np.minimum(v[i, 7], reach)
            seg[j, :, 0:3] = p[i][None, :]
            seg[j, :, 4:7] = (p[i][None, :] + (dirs * ell).astype(F)).astype(F)
            seg[j, :, 3] = seg[j, :, 7] = np.minimum(v[i, 8], FLT_MAX)
        hits = CR.cast(cfg, lay, seg.reshape(-1, 8)).reshape(ok.size, NP)
    cx, cy, cz = centres(cfg)
    zc = n[0] * n[1]
    for j, i in enumerate(ok):
        ph, pv, _ = cache[v[i, 3:7].tobytes()]
        h = hits[j]
        hit = h["status"] == CR.HIT
        # a ray walks ONE layer: the one step 1 tested the own cell in
        assert (h["layer"][hit] == layer[i]).all() and not np.isin(h["status"], (CR.START_OUTSIDE,)).any()
        vox = np.where(hit, h["voxel"], 0).astype(np.int64)
        hz, hy, hx = vox // zc, (vox % zc) // n[0], vox % n[0]
        with np.errstate(all="ignore"):
            ml = np.where(hit, _length((cx[hx] - p[i, 0]).astype(F), (cy[hy] - p[i, 1]).astype(F), (cz[hz] - p[i, 2]).astype(F)), F(-1)).astype(F)
            z, y, x = np.meshgrid((cz - p[i, 2]).astype(F), (cy - p[i, 1]).astype(F), (cx - p[i, 0]).astype(F), indexing="ij")
            b = K.pyramid_of(ph, pv, x, y, z)
            dist = _length(x, y, z)
            mlb = ml[np.maximum(b, 0)]
            wedge = b >= 0
            occluded = wedge & (mlb > 0) & (dist > (mlb + F(occl_margin)).astype(F))
            beyond = wedge & ~occluded & ~(dist <= v[i, 7])
        seen = wedge & ~occluded & ~beyond
        out[i] = (int(seen.sum()), int((seen & unknown).sum()), int(hit.sum()), OK)
        if details:
            info[int(i)] = dict(seen=seen, occluded=occluded, beyond=beyond, ml=ml, ray_status=h["status"].copy())
    return (out, info) if details else out
