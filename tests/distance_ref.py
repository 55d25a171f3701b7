"""numpy restatement of the truncated Euclidean distance fields (include/dspmap.h, dspmap_build_distance_field and
dspmap_query_distance), from what the map hands out: results() ([V, 4]), getFutureStatus() ([V, T]) and the configuration.

Two independent routes to the squared distance D2 in voxel units: a brute force over all (cell, occupied voxel) pairs for small grids
and an exact separable one for real sizes (no truncation inside: full windows, pruned only where dy^2 alone already exceeds every
value of the array).  They are asserted equal on random grids by the CPU tests (and compared with scipy's EDT where scipy exists).
Grids are [nz, ny, nx], the reference's voxel index order (:1081) reshaped."""
import numpy as np

from tests import query_ref as Q

F = np.float32
INF = np.int64(1) << 40   # "no occupied voxel": sums of a few of these stay inside int64


def d2_brute(occ):
    """D2 [nz, ny, nx] int64 of a bool grid by comparing every cell with every occupied voxel; INF everywhere for an empty grid"""
    occ = np.asarray(occ, bool)
    u = np.argwhere(occ)
    if len(u) == 0:
        return np.full(occ.shape, INF, np.int64)
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in occ.shape], indexing="ij"), -1).reshape(-1, 3)
    d = ((cells[:, None, :] - u[None, :, :]) ** 2).sum(-1).min(1)
    return d.reshape(occ.shape).astype(np.int64)


def _min_plus(f, axis):
    """out[i] = min over j of f[j] + (i - j)^2 along `axis`, exact"""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    out = f.copy()
    for s in range(1, n):
        if s * s >= out.max():      # no candidate s or more cells away can lower any value (an all-INF array stops at once too)
            break
        np.minimum(out[s:], f[:-s] + s * s, out=out[s:])
        np.minimum(out[:-s], f[s:] + s * s, out=out[:-s])
    return np.moveaxis(out, 0, axis)


def d2_separable(occ):
    """the same D2, one axis after the other: nearest occupied voxel of each row, then exact min-plus along y and z"""
    occ = np.asarray(occ, bool)
    if not occ.any():
        return np.full(occ.shape, INF, np.int64)
    nx = occ.shape[2]
    ix = np.arange(nx, dtype=np.int64)
    left = np.maximum.accumulate(np.where(occ, ix, -INF), axis=2)                       # nearest occupied index at or below
    right = np.minimum.accumulate(np.where(occ, ix, INF)[:, :, ::-1], axis=2)[:, :, ::-1]   # ... at or above
    g = np.minimum(ix - left, right - ix)
    f = np.where(g >= INF // 2, INF, np.minimum(g, 1 << 19) ** 2)
    f = np.minimum(_min_plus(f, 1), INF)
    return np.minimum(_min_plus(f, 0), INF)


def outside_d2(shape):
    """min over the axes of min(i + 1, n - i)^2: squared steps to the lattice just outside the map"""
    e = None
    for a, n in enumerate(shape):
        i = np.arange(n, dtype=np.int64)
        ea = np.minimum(i + 1, n - i).reshape([-1 if b == a else 1 for b in range(3)])
        e = ea if e is None else np.minimum(e, ea)
    return e * e


def value(d2, max_voxels, res, outside_occupied=False):
    """the field in metres: fl(fl(sqrt((float)min(D2, R^2))) * res), every step float32"""
    d2 = np.asarray(d2, np.int64)
    if outside_occupied:
        d2 = np.minimum(d2, outside_d2(d2.shape))
    d2c = np.minimum(d2, int(max_voxels) ** 2)
    return (np.sqrt(d2c.astype(F)).astype(F) * F(res)).astype(F)


def occupancy_layers(cfg, results, future, threshold):
    """bool [L, nz, ny, nx]: layer 0 = current mass > threshold, layer 1 + k = future status of horizon k > threshold"""
    T = int(cfg.prediction_times)
    shape = (int(cfg.nz), int(cfg.ny), int(cfg.nx))
    thr = F(threshold)
    layers = [np.asarray(results, F)[:, 0] > thr]
    fut = np.asarray(future, F).reshape(len(layers[0]), T) if T else None
    for k in range(T):
        layers.append(fut[:, k] > thr)
    return np.stack([l.reshape(shape) for l in layers])


def d2_layers(occ_layers):
    return np.stack([d2_separable(o) for o in occ_layers])


def field(cfg, results, future, threshold, max_voxels, outside_occupied=False, d2=None):
    """[L, nz, ny, nx] float32; d2 = d2_layers(...) of the same threshold, when the caller keeps it over several (R, flag) pairs"""
    if d2 is None:
        d2 = d2_layers(occupancy_layers(cfg, results, future, threshold))
    return np.stack([value(x, max_voxels, F(cfg.voxel_resolution), outside_occupied) for x in d2])


def query(cfg, fld, samples, world=False, cur_pos=(0.0, 0.0, 0.0), outside=0.0):
    """(dist [n], grad [n, 3]) float32 of samples [n, 4] on a field [L, nz, ny, nx]"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    q = np.ascontiguousarray(samples, F).reshape(-1, 4)
    p = q[:, :3].copy()
    if world:
        p = (p - np.asarray(cur_pos, F)[None, :]).astype(F)
    nan = np.isnan(q).any(1)
    layer = Q.horizons(pred, np.where(nan, F(-1), q[:, 3])) + 1
    inside, g = Q.own_voxel(cfg, np.where(nan[:, None], F(0), p))
    inside &= ~nan
    ix, iy, iz = g % n[0], (g // n[0]) % n[1], g // (n[0] * n[1])
    fld = np.asarray(fld, F)
    dist = np.where(inside, fld[layer, iz, iy, ix], F(outside)).astype(F)
    grad = np.zeros((len(q), 3), F)
    idx = [ix, iy, iz]
    for a in range(3):
        if n[a] == 1:
            continue
        lo, hi = np.maximum(idx[a] - 1, 0), np.minimum(idx[a] + 1, n[a] - 1)
        sel_hi, sel_lo = list(idx), list(idx)
        sel_hi[a], sel_lo[a] = hi, lo
        diff = (fld[layer, sel_hi[2], sel_hi[1], sel_hi[0]] - fld[layer, sel_lo[2], sel_lo[1], sel_lo[0]]).astype(F)
        step = ((hi - lo).astype(F) * res).astype(F)
        grad[:, a] = np.where(inside, (diff / step).astype(F), F(0))
    return dist, grad
