"""numpy restatement of dspmap_build_objects (include/dspmap.h): the connected components of one bool layer of the cast grid occ [nz, ny, nx]
under 6- or 26-connectivity by min-label propagation to a fixed point, then the records, the label grid and the counts, with mass and
momentum from a result grid res [V, 4] (what DSPMap.results() returns).  Everything is integer work: the device has to give the same
integers, bit for bit."""
import numpy as np

from tests import cast_ref as CR

OBJECT_DTYPE = np.dtype([("label", "i4"), ("count", "i4"), ("min_x", "i4"), ("max_x", "i4"), ("min_y", "i4"), ("max_y", "i4"), ("min_z", "i4"), ("max_z", "i4"),
                         ("sum_x", "i8"), ("sum_y", "i8"), ("sum_z", "i8"), ("mass_q", "i8"), ("mom_q", "i8", (3,))])
pack = CR.pack
F = np.float32
Q = F(1048576.0)


def offsets(conn):
    """the lower half of the neighbourhood as (dz, dy, dx): every adjacent pair appears once"""
    assert conn in (6, 26)
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) >= (0, 0, 0):
                    continue
                if conn == 6 and abs(dz) + abs(dy) + abs(dx) != 1:
                    continue
                out.append((dz, dy, dx))
    assert len(out) == (3 if conn == 6 else 13)
    return out


def edges(occ, conn):
    """(a, b): voxel indices of every pair of adjacent set cells, b the neighbour in the lower half"""
    occ = np.asarray(occ, bool)
    nz, ny, nx = occ.shape
    idx = np.arange(occ.size, dtype=np.int64).reshape(occ.shape)
    aa, bb = [], []
    for dz, dy, dx in offsets(conn):
        def sl(d, n):   # (cells that have the neighbour inside the map, the neighbours): the outside does not exist
            return (slice(-d, n), slice(0, n + d)) if d < 0 else (slice(0, n - d), slice(d, n))
        (az, bz), (ay, by), (ax, bx) = sl(dz, nz), sl(dy, ny), sl(dx, nx)
        both = occ[az, ay, ax] & occ[bz, by, bx]
        aa.append(idx[az, ay, ax][both])
        bb.append(idx[bz, by, bx][both])
    return np.concatenate(aa), np.concatenate(bb)


def components(occ, conn):
    """int64 [nz, ny, nx]: per set cell the smallest voxel index of its component, -1 for a clear cell.  Min-label propagation: every
    cell takes the smallest label on either end of its edges, then labels jump (L = L[L]); repeated to the fixed point, where both ends
    of every edge agree.  L[x] <= x throughout, and a label is always a cell of the same component, so the fixed point is the minimum."""
    occ = np.asarray(occ, bool)
    a, b = edges(occ, conn)
    L = np.arange(occ.size, dtype=np.int64)
    for _ in range(occ.size + 1):
        m = np.minimum(L[a], L[b])
        N = L.copy()
        for at in (a, b, L[a], L[b]):
            np.minimum.at(N, at, m)
        while True:
            J = N[N]
            if np.array_equal(J, N):
                break
            N = J
        if np.array_equal(N, L):
            break
        L = N
    else:
        raise AssertionError("no fixed point")
    return np.where(occ.ravel(), L, -1).reshape(occ.shape)


def flood(occ, conn):
    """the same by a plain flood fill, cell by cell (for small shapes)"""
    occ = np.asarray(occ, bool)
    nz, ny, nx = occ.shape
    half = offsets(conn)
    nbr = half + [(-dz, -dy, -dx) for dz, dy, dx in half]
    lab = np.full(occ.shape, -1, np.int64)
    for z0, y0, x0 in zip(*np.nonzero(occ)):          # ascending voxel index: the seed is its component's smallest
        if lab[z0, y0, x0] >= 0:
            continue
        seed = (z0 * ny + y0) * nx + x0
        lab[z0, y0, x0] = seed
        stack = [(z0, y0, x0)]
        while stack:
            z, y, x = stack.pop()
            for dz, dy, dx in nbr:
                zz, yy, xx = z + dz, y + dy, x + dx
                if 0 <= zz < nz and 0 <= yy < ny and 0 <= xx < nx and occ[zz, yy, xx] and lab[zz, yy, xx] < 0:
                    lab[zz, yy, xx] = seed
                    stack.append((zz, yy, xx))
    return lab


def contributions(res):
    """int64 [V, 4]: what every voxel adds to mass_q and mom_q[0..2], each named operation rounded to fp32 on its own"""
    res = np.asarray(res, F).reshape(-1, 4)
    out = np.zeros(res.shape, np.int64)
    with np.errstate(all="ignore"):
        w = res[:, 0]
        ok = np.isfinite(w) & (w > 0) & (w < F(4096))
        out[ok, 0] = (w[ok] * Q).astype(np.int64)            # (astype truncates, as the C cast)
        for k in range(3):
            u = res[:, 1 + k]
            p = (w * u).astype(F)
            okk = ok & np.isfinite(u) & (np.abs(p) < F(4096))
            out[okk, 1 + k] = (p[okk] * Q).astype(np.int64)
    return out


def objects(occ, res, conn, min_cells=1, max_objects=1 << 20, lab=None):
    """(records OBJECT_DTYPE [min(n_objects, max_objects)], label grid int32 [nz, ny, nx], (n_objects, n_components, n_occupied))"""
    occ = np.asarray(occ, bool)
    nz, ny, nx = occ.shape
    if lab is None:
        lab = components(occ, conn)
    z, y, x = np.nonzero(occ)
    cell_lab = lab[z, y, x]
    ids, inv, cnt = np.unique(cell_lab, return_inverse=True, return_counts=True)   # ascending label
    keep = cnt >= min_cells
    ordinal = np.where(keep, np.cumsum(keep) - 1, -1)
    grid = np.full(occ.shape, -1, np.int32)
    grid[z, y, x] = ordinal[inv]
    n_obj = int(keep.sum())
    q = contributions(res)[(z * ny + y) * nx + x]
    rec = np.zeros(ids.size, OBJECT_DTYPE)
    rec["label"], rec["count"] = ids, cnt
    for ax, v in (("x", x), ("y", y), ("z", z)):
        lo, hi = np.full(ids.size, 1 << 30, np.int64), np.full(ids.size, -1, np.int64)
        np.minimum.at(lo, inv, v)
        np.maximum.at(hi, inv, v)
        s = np.zeros(ids.size, np.int64)
        np.add.at(s, inv, v)
        rec["min_" + ax], rec["max_" + ax], rec["sum_" + ax] = lo, hi, s
    acc = np.zeros((ids.size, 4), np.int64)
    np.add.at(acc, inv, q)
    rec["mass_q"], rec["mom_q"] = acc[:, 0], acc[:, 1:]
    return rec[keep][:max_objects], grid, (n_obj, int(ids.size), int(occ.sum()))


def states(rec, shape, res):
    """(centre, box_lo, box_hi, velocity) float32 [k, 3] in the map frame, as DSPMap.object_states"""
    res = float(F(res))
    half = np.array(shape, np.float64) * res / 2.0
    cnt = np.maximum(rec["count"], 1)[:, None].astype(np.float64)
    mean = np.stack([rec["sum_x"], rec["sum_y"], rec["sum_z"]], 1) / cnt
    lo = np.stack([rec["min_x"], rec["min_y"], rec["min_z"]], 1).astype(np.float64)
    hi = np.stack([rec["max_x"], rec["max_y"], rec["max_z"]], 1).astype(np.float64)
    mass = rec["mass_q"].astype(np.float64)[:, None]
    vel = np.where(mass > 0, rec["mom_q"].astype(np.float64) / np.maximum(mass, 1.0), 0.0)
    return (((mean + 0.5) * res - half).astype(F), (lo * res - half).astype(F), ((hi + 1.0) * res - half).astype(F), vel.astype(F))


def scene(shape, seed=11):
    """occ bool [nz, ny, nx].  Plane z = 0 is a serpentine: the even rows are full and joined alternately at the two ends by one cell
    of the odd row between them, so the smallest index has to travel the whole chain.  Plane z = 1 is empty.  Where nz >= 3 the planes
    z >= 2 are filled at random with density 0.18."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    occ = np.zeros((nz, ny, nx), bool)
    occ[0, 0::2, :] = True
    for y in range(1, ny, 2):
        occ[0, y, nx - 1 if (y // 2) % 2 == 0 else 0] = True
    if nz >= 3:
        occ[2:] = rng.random((nz - 2, ny, nx)) < 0.18
    return occ


def summary(lab):
    """(components, largest, singles, with >= 4 cells) of a labelling"""
    cnt = np.unique(lab[lab >= 0], return_counts=True)[1]
    return int(cnt.size), int(cnt.max()), int((cnt == 1).sum()), int((cnt >= 4).sum())
