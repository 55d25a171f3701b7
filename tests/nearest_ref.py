"""numpy restatement of the nearest-obstacle fields (include/dspmap.h, dspmap_build_nearest_field and dspmap_query_nearest), from what
the map hands out: results() ([V, 4]), getFutureStatus() ([V, T]) or a cast grid's bits, and the configuration.

Two independent routes to the pair (D2, nearest target) of every cell of a bool grid: a brute force that compares every cell with every
target under the key d2 * V + index -- the tie rule "smallest global voxel index" as ONE integer --, and a separable one that takes a
lexicographic argmin (total, coordinate) per axis, which is what composes to that rule.  Both truncate at R (None: not at all).  The CPU
tests assert them equal on random grids.  Grids are [nz, ny, nx], the reference's voxel index order (:1081) reshaped."""
import numpy as np

from tests import distance_ref as D
from tests import query_ref as Q

F = np.float32
INF = D.INF
NEAREST_DTYPE = np.dtype([("dist", "f4"), ("voxel", "i4"), ("offset", "f4", (3,)), ("velocity", "f4", (3,))])


def _brute_targets(tgt, R):
    """(D2 int64, near int64) of EVERY cell towards the True cells of tgt; (INF, -1) beyond R or without a target"""
    tgt = np.asarray(tgt, bool)
    V = tgt.size
    u = np.argwhere(tgt)
    if len(u) == 0:
        return np.full(tgt.shape, INF, np.int64), np.full(tgt.shape, -1, np.int64)
    uidx = np.flatnonzero(tgt.ravel())
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in tgt.shape], indexing="ij"), -1).reshape(-1, 3)
    d2 = ((cells[:, None, :] - u[None, :, :]) ** 2).sum(-1).astype(np.int64)
    key = (d2 * V + uidx[None, :]).min(1)
    best, near = key // V, key % V
    if R is not None:
        none = best > R * R
        best, near = np.where(none, INF, best), np.where(none, -1, near)
    return best.reshape(tgt.shape), near.reshape(tgt.shape)


def _argmin_plus(f, carried, axis, R):
    """per cell i along `axis`: the j that minimises (f[j] + (i - j)^2, j) lexicographically -> (that total, j, the carried arrays taken
    at j); totals above R^2 become INF"""
    f = np.moveaxis(f, axis, 0)
    shape = f.shape
    n = shape[0]
    f = f.reshape(n, -1)
    live = np.flatnonzero((f < INF).any(0))      # a column without a target stays without one: only the others are scanned
    N = np.int64(n + 1)
    idx = np.arange(n, dtype=np.int64).reshape(-1, 1)
    key = f[:, live] * N + idx
    out = key.copy()
    for s in range(1, n if R is None else min(n, R + 1)):
        s2 = np.int64(s * s)
        if out.size == 0 or s2 > out.max() // N:       # no candidate s or more cells away can lower or tie any value
            break
        np.minimum(out[s:], key[:-s] + s2 * N, out=out[s:])
        np.minimum(out[:-s], key[s:] + s2 * N, out=out[:-s])
    total = np.full(f.shape, INF, np.int64)
    j = np.zeros(f.shape, np.int64)
    total[:, live], j[:, live] = out // N, out % N
    if R is not None:
        total = np.where(total > R * R, INF, total)
    total = np.minimum(total, INF).reshape(shape)
    j = j.reshape(shape)
    taken = [np.moveaxis(np.take_along_axis(np.moveaxis(c, axis, 0), j, 0), 0, axis) for c in carried]
    return np.moveaxis(total, 0, axis), np.moveaxis(j, 0, axis), taken


def _separable_targets(tgt, R):
    """the same pair, one axis after the other: the row's nearest target (equal: the left), then the lexicographic argmin along y and z"""
    tgt = np.asarray(tgt, bool)
    nz, ny, nx = tgt.shape
    if not tgt.any():
        return np.full(tgt.shape, INF, np.int64), np.full(tgt.shape, -1, np.int64)
    ix = np.arange(nx, dtype=np.int64)
    left = np.maximum.accumulate(np.where(tgt, ix, -INF), axis=2)
    right = np.minimum.accumulate(np.where(tgt, ix, INF)[:, :, ::-1], axis=2)[:, :, ::-1]
    dl, dr = ix - left, right - ix
    g = np.minimum(dl, dr)
    none = g >= INF // 2
    if R is not None:
        none |= g > R
    ux = np.where(none, 0, np.where(dl <= dr, left, right))
    f = np.where(none, INF, np.minimum(g, 1 << 19) ** 2)
    f, uy, (ux,) = _argmin_plus(f, [ux], 1, R)
    f, uz, (ux, uy) = _argmin_plus(f, [ux, uy], 0, R)
    near = np.where(f >= INF, -1, (uz * ny + uy) * nx + ux)
    return f, near


def _combine(route, occ, R, signed):
    occ = np.asarray(occ, bool)
    d2, near = route(occ, R)
    if signed:
        d2c, nearc = route(~occ, R)
        d2, near = np.where(occ, d2c, d2), np.where(occ, nearc, near)
    return d2, near.astype(np.int32)


def nearest_brute(occ, R=None, signed=False):
    """(D2 int64 [nz, ny, nx] with INF for none, near int32 with -1 for none) by brute force: a free cell targets the occupied voxels, an
    occupied one itself, or with signed the free voxels"""
    return _combine(_brute_targets, occ, R, signed)


def nearest_separable(occ, R=None, signed=False):
    return _combine(_separable_targets, occ, R, signed)


def count_minimisers(tgt):
    """per cell the number of targets at the minimal squared distance (brute force; 0 without a target)"""
    tgt = np.asarray(tgt, bool)
    u = np.argwhere(tgt)
    if len(u) == 0:
        return np.zeros(tgt.shape, np.int64)
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in tgt.shape], indexing="ij"), -1).reshape(-1, 3)
    d2 = ((cells[:, None, :] - u[None, :, :]) ** 2).sum(-1)
    return (d2 == d2.min(1, keepdims=True)).sum(1).reshape(tgt.shape)


def value(d2, occ, max_voxels, res, signed=False):
    """dist in metres: fl(fl(sqrt((float)min(D2, R^2))) * res), negated for an occupied cell of a signed field"""
    v = D.value(d2, max_voxels, res)
    return np.where(np.asarray(occ, bool), -v, v).astype(F) if signed else v


def layers(occ_layers, max_voxels, res, signed=False):
    """(near int32 [L, nz, ny, nx], dist float32 [L, nz, ny, nx]) of bool layers"""
    near, dist = [], []
    for o in occ_layers:
        d2, nr = nearest_separable(o, max_voxels, signed)
        near.append(nr)
        dist.append(value(d2, o, max_voxels, res, signed))
    return np.stack(near), np.stack(dist)


def truncate(d2, near, max_voxels):
    """the pair truncated at R from the untruncated one: truncation only takes targets away (a minimiser within R stays the minimiser)"""
    none = d2 > int(max_voxels) ** 2
    return np.where(none, INF, d2), np.where(none, -1, near).astype(np.int32)


def pairs_untruncated(occ_layers, signed=False):
    """(D2 int64, near int32) [L, nz, ny, nx], untruncated: what a caller keeps over several radii (truncate, value)"""
    both = [nearest_separable(o, None, signed) for o in occ_layers]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def field(cfg, results, future, threshold, max_voxels, signed=False):
    """(near, dist, occ) from the masses: the distance field's occupancy rule"""
    occ = D.occupancy_layers(cfg, results, future, threshold)
    return layers(occ, max_voxels, F(cfg.voxel_resolution), signed) + (occ,)


def bits_of(occ_layers):
    """bool [L, nz, ny, nx] -> cast grid words uint64 [L, nz, ny, W], bit (x & 63) of word (x >> 6)"""
    occ = np.asarray(occ_layers, bool)
    L, nz, ny, nx = occ.shape
    W = (nx + 63) // 64
    pad = np.zeros((L, nz, ny, W * 64), np.uint8)
    pad[..., :nx] = occ
    return np.packbits(pad.reshape(L, nz, ny, W, 8, 8), axis=-1, bitorder="little").reshape(L, nz, ny, W, 8).copy().view("<u8").reshape(L, nz, ny, W)


def _put(shape, cells):
    """a bool grid [nz, ny, nx] with the (z, y, x) of cells set; None if one of them does not fit"""
    g = np.zeros(shape, bool)
    for c in cells:
        if any(not 0 <= v < n for v, n in zip(c, shape)):
            return None
        g[tuple(c)] = True
    return g


def tie_scenes(shape, R):
    """hand-made layers [(name, bool grid [nz, ny, nx], (z, y, x) of a cell with several minimisers or None)] for a map of `shape`: what the
    header's tie rule and the truncation decide.  A scene that does not fit the shape is left out."""
    nz, ny, nx = shape
    cz, cy, cx = nz // 2, ny // 2, min(nx // 2, 20)
    out = []

    def add(name, offsets, cell=None):
        cell = (cz, cy, cx) if cell is None else cell
        g = _put(shape, [tuple(c + o for c, o in zip(cell, off)) for off in offsets])
        if g is not None:
            out.append((name, g, cell))
    # equidistant pairs along one axis (offsets are (dz, dy, dx))
    for k in (1, 2, 3):
        add("pair_x_%d" % k, [(0, 0, -k), (0, 0, k)])
        add("pair_y_%d" % k, [(0, -k, 0), (0, k, 0)])
        add("pair_z_%d" % k, [(-k, 0, 0), (k, 0, 0)])
    # equal totals across passes: (dx, dy) = (2, +1) against (1, -2) and the mirrors; the same between x / z and y / z
    for sx in (1, -1):
        for sy in (1, -1):
            add("xy_5_%+d%+d" % (sx, sy), [(0, sy, 2 * sx), (0, -2 * sy, sx)])
            add("xz_5_%+d%+d" % (sx, sy), [(sy, 0, 2 * sx), (-2 * sy, 0, sx)])
            add("yz_5_%+d%+d" % (sx, sy), [(sy, 2 * sx, 0), (-2 * sy, sx, 0)])
    # 3-4-5: (3, 4, 0) against (5, 0, 0) against (0, 0, 5) in (dx, dy, dz), and mirrored so that the far negative side wins after a nearer
    # positive candidate was seen
    if R >= 5:
        for s in (1, -1):
            add("345_xyz_%+d" % s, [(0, 4 * s, 3 * s), (0, 0, 5 * s), (5 * s, 0, 0)])
            add("345_xy_%+d" % s, [(0, 4 * s, 3 * s), (0, 0, 5 * s)])
            add("345_xy_mixed_%+d" % s, [(0, -4 * s, 3 * s), (0, 0, 5 * s)])
            add("345_yz_%+d" % s, [(3 * s, 4 * s, 0), (-5 * s, 0, 0)])
            add("345_zx_%+d" % s, [(-4 * s, 0, 3 * s), (0, 0, -5 * s), (0, 5 * s, 0)])
    # one target: cells exactly R and R + 1 away along x (across word boundaries where the row has them) and along y
    for name, x in (("edge_x63", 63), ("edge_x64", 64), ("edge_x127", 127), ("edge_x0", 0), ("edge_xlast", nx - 1)):
        g = _put(shape, [(0, 0, x)])
        if g is not None:
            out.append((name, g, None))
    for name, y in (("edge_y0", 0), ("edge_ylast", ny - 1), ("edge_ymid", ny // 2)):
        out.append((name, _put(shape, [(nz - 1, y, nx - 1)]), None))
    # the last valid columns occupied: under SIGNED their free targets lie to the left, the padding bits at x >= nx are no targets
    g = np.zeros(shape, bool)
    g[:, :, max(nx - 4, 1):] = True
    out.append(("last_columns", g, None))
    g = np.zeros(shape, bool)
    g[:, :, nx - 1] = True
    g[:, ny - 1, :] = True
    out.append(("last_column_and_row", g, None))
    out.append(("all_set", np.ones(shape, bool), None))
    out.append(("all_clear", np.zeros(shape, bool), None))
    rng = np.random.default_rng(nx * 1000003 + ny * 1009 + nz)
    for dens in (0.001, 0.02, 0.5, 0.98):
        out.append(("random_%g" % dens, rng.random(shape) < dens, None))
    return out


def query(cfg, near, dist, occ, results, samples, world=False, cur_pos=(0.0, 0.0, 0.0), outside=0.0):
    """NEAREST_DTYPE [n] of samples [n, 4] on the fields [L, nz, ny, nx] built over the bool layers occ; results: results() of the map"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    q = np.ascontiguousarray(samples, F).reshape(-1, 4)
    p = q[:, :3].copy()
    if world:
        p = (p - np.asarray(cur_pos, F)[None, :]).astype(F)
    nan = np.isnan(q).any(1)
    layer = Q.horizons(pred, np.where(nan, F(-1), q[:, 3])) + 1
    inside, g = Q.own_voxel(cfg, np.where(nan[:, None], F(0), p))
    inside &= ~nan
    V = n[0] * n[1] * n[2]
    nr = np.asarray(near).reshape(-1, V)[layer, g]
    out = np.zeros(len(q), NEAREST_DTYPE)
    out["dist"] = np.where(inside, np.asarray(dist, F).reshape(-1, V)[layer, g], F(outside))
    out["voxel"] = np.where(inside, nr, -1)
    has = inside & (nr >= 0)
    u = np.where(has, nr, 0)
    for a, ua in enumerate((u % n[0], (u // n[0]) % n[1], u // (n[0] * n[1]))):
        c = ((ua.astype(F) * res).astype(F) + corr[a]).astype(F)      # dspmap_voxel_center
        with np.errstate(invalid="ignore"):
            out["offset"][:, a] = np.where(has, (c - p[:, a]).astype(F), F(0))
    own_occ = np.asarray(occ, bool).reshape(-1, V)[layer, g]
    w = np.where(own_occ, g, nr)
    fill = inside & (layer == 0) & (w >= 0)
    vel = np.asarray(results, F)[np.where(fill, w, 0), 1:4]
    out["velocity"] = np.where(fill[:, None], vel, F(0))
    return out
