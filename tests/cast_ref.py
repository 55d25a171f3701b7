"""numpy float32 restatement of the cast grid and the segment casts (include/dspmap.h, dspmap_build_cast_grid and
dspmap_cast_segments), from what the map hands out: results() ([V, 4]), getFutureStatus() ([V, T]) and the configuration.

Independent of the kernels' structure: the occupancy layers are bool grids [L, nz, ny, nx] (tests/distance_ref.occupancy_layers), the
inflation is shifted ORs of a padded bool array (and, as a second route, a maximum over explicit offsets), the cast tests bool cells --
no words, no carried layers -- in a loop over cells that is vectorised over the segments, with one numpy float32 operation per rounding
of the definition.  It asserts the bound of nx + ny + nz steps."""
import numpy as np

from tests import distance_ref as D
from tests import query_ref as Q

F = np.float32
HIT_DTYPE = np.dtype([("s", "f4"), ("voxel", "i4"), ("layer", "i4"), ("status", "i4")])
FREE, HIT, LEFT_MAP, START_OUTSIDE, INVALID = range(5)


def inflate(occ, r):
    """Chebyshev dilation by r of bool grids [..., nz, ny, nx]: one axis after the other, OR of the 2r + 1 shifts of the zero-padded array"""
    out = np.asarray(occ, bool)
    r = int(r)
    if r == 0:
        return out.copy()
    for axis in (-1, -2, -3):
        n = out.shape[axis]
        pad = [(0, 0)] * out.ndim
        pad[axis] = (r, r)
        p = np.pad(out, pad)
        acc = np.zeros_like(out)
        for s in range(2 * r + 1):
            acc |= np.take(p, np.arange(s, s + n), axis=axis)
        out = acc
    return out


def inflate_brute(occ, r):
    """the same for one grid [nz, ny, nx] as a maximum over the (2r + 1)^3 explicit offsets, clipped at the faces"""
    occ = np.asarray(occ, bool)
    nz, ny, nx = occ.shape
    out = np.zeros(occ.shape, np.uint8)
    for dz in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                z0, z1 = max(0, -dz), min(nz, nz - dz)      # cells i with i + d inside the map
                y0, y1 = max(0, -dy), min(ny, ny - dy)
                x0, x1 = max(0, -dx), min(nx, nx - dx)
                if z0 >= z1 or y0 >= y1 or x0 >= x1:
                    continue
                out[z0:z1, y0:y1, x0:x1] = np.maximum(out[z0:z1, y0:y1, x0:x1], occ[z0 + dz:z1 + dz, y0 + dy:y1 + dy, x0 + dx:x1 + dx])
    return out.astype(bool)


def layers(cfg, results, future, threshold, inflate_voxels=0):
    """bool [L, nz, ny, nx]: the raw occupancy of the distance field's rule, inflated"""
    return inflate(D.occupancy_layers(cfg, results, future, threshold), inflate_voxels)


def pack(lay):
    """bool [..., nx] -> uint64 [..., W]: bit (x & 63) of word (x >> 6); bits at x >= nx are 0"""
    lay = np.asarray(lay, bool)
    nx = lay.shape[-1]
    W = (nx + 63) // 64
    pad = [(0, 0)] * (lay.ndim - 1) + [(0, W * 64 - nx)]
    b = np.pad(lay, pad).reshape(lay.shape[:-1] + (W, 64)).astype(np.uint64)
    return np.bitwise_or.reduce(b << np.arange(64, dtype=np.uint64), axis=-1)


def cast(cfg, lay, seg, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """HIT_DTYPE [n] of segments [n, 8] = {ax, ay, az, ta, bx, by, bz, tb} through bool layers [L, nz, ny, nx]"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    lay = np.asarray(lay, bool)
    assert lay.shape == (T + 1, n[2], n[1], n[0])
    seg = np.ascontiguousarray(seg, F).reshape(-1, 8)
    out = np.zeros(len(seg), HIT_DTYPE)
    out["voxel"], out["layer"], out["status"] = -1, -1, INVALID
    valid = np.isfinite(seg[:, 0:3]).all(1) & np.isfinite(seg[:, 4:7]).all(1) & ~np.isnan(seg[:, 3]) & ~np.isnan(seg[:, 7])
    nn = np.array(n, np.int64)
    with np.errstate(all="ignore"):
        a, b = seg[:, 0:3].copy(), seg[:, 4:7].copy()
        if world:
            cur = np.asarray(cur_pos, F)[None, :]
            a, b = (a - cur).astype(F), (b - cur).astype(F)
        hv = np.array(half, F)[None, :]
        inside = valid & (np.abs(a) < hv).all(1)                 # dspmap_point_voxel_index: p >= half or p <= -half is outside
        ua = ((a + hv).astype(F) / res).astype(F)
        ub = ((b + hv).astype(F) / res).astype(F)
        i0 = np.trunc(np.where(inside[:, None], ua, F(0))).astype(np.int64)
        inside &= (i0 < nn[None, :]).all(1)
        out["status"][valid & ~inside] = START_OUTSIDE
        sel = np.flatnonzero(inside)                             # the segments that walk
        ua, ub, cell = ua[sel], ub[sel], i0[sel]
        ta, tb = seg[sel, 3], seg[sel, 7]
        d = (ub - ua).astype(F)
        step = np.sign(d).astype(np.int64)
        moving = d != 0
        bnd = (cell + (step > 0)).astype(F)
        tmax = np.where(moving, ((bnd - ua).astype(F) / np.where(moving, d, F(1))).astype(F), F(np.inf)).astype(F)
        tdelta = np.where(moving, (F(1) / np.abs(np.where(moving, d, F(1)))).astype(F), F(0)).astype(F)
        timed = ~(ta < F(0)) & (T > 0)
        dt = (tb - ta).astype(F)
        s_in = np.zeros(len(sel), F)
        act = np.arange(len(sel))                                # still walking
        bound = n[0] + n[1] + n[2]
        visits = 0
        while act.size:
            visits += 1
            assert visits <= bound + 1, "a cast takes at most nx + ny + nz steps"
            tx, ty, tz = tmax[act, 0], tmax[act, 1], tmax[act, 2]
            first_x = (tx <= ty) & (tx <= tz)
            m = np.where(first_x, 0, np.where(ty <= tz, 1, 2))   # ties to x, then y, then z
            tm = tmax[act, m]
            s_out = np.minimum(tm, F(1))
            t_in = (ta[act] + (s_in[act] * dt[act]).astype(F)).astype(F)
            t_out = (ta[act] + (s_out * dt[act]).astype(F)).astype(F)
            l_a = np.where(timed[act], Q.horizons(pred, t_in) + 1, 0)
            l_b = np.where(timed[act], Q.horizons(pred, t_out) + 1, 0)
            lo, hi = np.minimum(l_a, l_b), np.maximum(l_a, l_b)
            c = cell[act]
            hit_layer = np.full(act.size, -1, np.int64)
            for l in range(T, -1, -1):                           # descending, so that the lowest set layer is the one left standing
                h = (lo <= l) & (l <= hi) & lay[l, c[:, 2], c[:, 1], c[:, 0]]
                hit_layer[h] = l
            gidx = (c[:, 2] * n[1] + c[:, 1]) * n[0] + c[:, 0]
            is_hit = hit_layer >= 0
            k = sel[act[is_hit]]
            out["s"][k], out["voxel"][k], out["layer"][k], out["status"][k] = s_in[act[is_hit]], gidx[is_hit], hit_layer[is_hit], HIT
            free = ~is_hit & ~(tm <= F(1))
            k = sel[act[free]]
            out["s"][k], out["status"][k] = F(1), FREE
            go = ~is_hit & ~free
            g = act[go]
            mg = m[go]
            s_in[g] = tm[go]
            cell[g, mg] += step[g, mg]
            tmax[g, mg] = (tm[go] + tdelta[g, mg]).astype(F)
            left = (cell[g, mg] < 0) | (cell[g, mg] >= nn[mg])
            k = sel[g[left]]
            out["s"][k], out["voxel"][k], out["status"][k] = tm[go][left], gidx[go][left], LEFT_MAP
            act = g[~left]
    return out
