"""numpy float32 restatement of the point / trajectory queries (include/dspmap.h, dspmap_query_occupancy and
dspmap_trajectory_risk), from what the map hands out: results() ([V, 4]), getFutureStatus() ([V, T]) and the configuration.

Independent of the kernel's loop structure: the candidate lattice points of a sample are a wider box (two steps of margin, no
clamping to the map), every fp32 operation of the predicate is an elementwise numpy float32 operation (one rounding each)."""
import numpy as np

F = np.float32


def _dims(cfg):
    T = int(cfg.prediction_times)
    pred = np.array([cfg.prediction_future_time[k] for k in range(T)], F)
    res = F(cfg.voxel_resolution)
    n = (int(cfg.nx), int(cfg.ny), int(cfg.nz))
    half = tuple(F(F(res * F(k)) * F(0.5)) for k in n)     # (res * n) * 0.5 (:528-530)
    corr = tuple(F(-h + F(res * F(0.5))) for h in half)    # dspmap_voxel_center: -half + res / 2
    return T, pred, res, n, half, corr


def horizons(pred, t):
    """-1 = the current mass (t < 0 or T == 0), else the smallest k with pred[k] >= t, clamped to T - 1"""
    t = np.asarray(t, F)
    T = len(pred)
    if T == 0:
        return np.full(t.shape, -1, np.int64)
    ge = pred[None, :] >= t[:, None]
    k = np.where(ge.any(1), ge.argmax(1), T - 1)
    return np.where(t >= F(0), k, -1)


def own_voxel(cfg, p):
    """getPointVoxelsIndexPublic (:1574-1584) on map-frame points [n, 3]: (inside, global index)"""
    T, pred, res, n, half, corr = _dims(cfg)
    inside = np.ones(len(p), bool)
    ijk = []
    for a in range(3):
        x = p[:, a]
        with np.errstate(invalid="ignore"):
            inside &= np.abs(x) < half[a]
            q = np.where(inside, (x + half[a]) / res, F(0)).astype(F)
        ijk.append(np.trunc(q).astype(np.int64))
    g = (ijk[2] * n[1] + ijk[1]) * n[0] + ijk[0]
    inside &= (g >= 0) & (g < n[0] * n[1] * n[2])
    return inside, np.where(inside, g, 0)


def query(cfg, results, future, samples, radius=0.0, world=False, cur_pos=(0.0, 0.0, 0.0), outside=1.0):
    """values [n] float32 and the `outside` flags [n] (point outside the map or a NaN input) of samples [n, 4]"""
    T, pred, res, n, half, corr = _dims(cfg)
    q = np.ascontiguousarray(samples, F).reshape(-1, 4)
    r = F(radius)
    r2 = F(r * r)
    out_v = F(outside)
    table = np.concatenate([np.asarray(results, F)[:, :1], np.asarray(future, F).reshape(len(results), T)], 1)   # col 0: t < 0
    p = q[:, :3].copy()
    if world:
        p = (p - np.asarray(cur_pos, F)[None, :]).astype(F)
    nan = np.isnan(q).any(1)
    k = horizons(pred, np.where(nan, F(-1), q[:, 3])) + 1
    inside, g = own_voxel(cfg, np.where(nan[:, None], F(0), p))
    inside &= ~nan
    val = np.where(inside, table[g, k], out_v).astype(F)
    if r > 0:
        K = int(np.ceil(float(r) / float(res))) + 2
        off = np.arange(-K, K + 1)
        chunk = max(64, 4000000 // len(off) ** 3)   # samples per pass: a few million candidates
        for s0 in range(0, len(q), chunk):
            sl = slice(s0, s0 + chunk)
            ps = p[sl]
            ok = ~nan[sl] & np.isfinite(ps).all(1)
            idx, d2a, ins = [], [], []
            for a in range(3):
                ic = np.where(ok, np.floor((ps[:, a].astype(np.float64) - float(corr[a])) / float(res)), 0).astype(np.int64)
                i = ic[:, None] + off[None, :]                                   # [m, L]
                c = (i.astype(F) * res + corr[a]).astype(F)                      # fl(fl(i * res) + corr)
                d = (c - ps[:, a:a + 1]).astype(F)
                idx.append(i)
                d2a.append((d * d).astype(F))
                ins.append((i >= 0) & (i < n[a]))
            dx2, dy2, dz2 = d2a
            d2 = ((dx2[:, None, None, :] + dy2[:, None, :, None]).astype(F) + dz2[:, :, None, None]).astype(F)   # [m, Lz, Ly, Lx]
            hit = (d2 <= r2) & ok[:, None, None, None]
            inmap = ins[2][:, :, None, None] & ins[1][:, None, :, None] & ins[0][:, None, None, :]
            gl = (idx[2][:, :, None, None] * n[1] + idx[1][:, None, :, None]) * n[0] + idx[0][:, None, None, :]
            kk = np.broadcast_to(k[sl][:, None, None, None], gl.shape)
            cand = np.where(inmap, table[np.where(inmap, gl, 0), kk], out_v).astype(F)
            cand = np.where(hit, cand, F(-np.inf))
            val[sl] = np.maximum(val[sl], cand.reshape(len(ps), -1).max(1))
    val = np.where(nan, out_v, val).astype(F)
    return val, (~inside) | nan


def risk(values, flags, n_samples, threshold=0.5):
    """per trajectory of n_samples consecutive values: sequential fp32 sum, max, first value > threshold (-1), flagged samples"""
    v = np.asarray(values, F).reshape(-1, n_samples)
    f = np.asarray(flags, bool).reshape(-1, n_samples)
    s = np.zeros(len(v), F)
    for j in range(n_samples):          # sequential in sample order: what a float32 loop computes
        s = (s + v[:, j]).astype(F)
    over = v > F(threshold)
    first = np.where(over.any(1), over.argmax(1), -1).astype(np.int32)
    return s, v.max(1), first, f.sum(1).astype(np.int32)
