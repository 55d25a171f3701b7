"""numpy float32 restatement of the occupancy forecast (include/dspmap.h, dspmap_build_forecast and dspmap_query_forecast), from what the
map hands out: export_state() (voxel, slot, rec8 = {flag, vx, vy, vz, px, py, pz, w}) and the configuration.

Independent of the kernel's loop structure: no tiles, no storage order, no per-tile flags.  Every named fp32 operation of the contract
is an elementwise numpy float32 operation (one rounding each); quanta are integers, summed per cell with np.add.at on int64."""
import numpy as np

from tests import query_ref as Q

F = np.float32
MAX_TIMES = 64
LERP = 2
SCALE = F(16777216.0)   # 2^24


def dims(cfg):
    res = F(cfg.voxel_resolution)
    n = (int(cfg.nx), int(cfg.ny), int(cfg.nz))
    half = tuple(F(F(res * F(k)) * F(0.5)) for k in n)   # (res * n) * 0.5 (:528-530)
    return res, n, half


def quanta(w):
    """q = __float2ull_rn(w * 2^24): round to nearest even in float32, NaN and negatives give 0"""
    w = np.asarray(w, F)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.rint((w * SCALE).astype(F))
        x = np.where(np.isnan(x) | (x < 0), F(0), x)
    return x.astype(np.int64)


def value(Q_):
    return (np.asarray(Q_, np.int64).astype(np.float64) * 2.0 ** -24).astype(F)


def layers(cfg, voxel, rec, times):
    """(layers [n, V] float32, quanta sums [n, V] int64, moving destinations dropped by the xi >= nx / yi >= ny rule).  A NaN fx or fy
    (a non-finite position or velocity) is outside the map: not a drop of that rule"""
    res, (nx, ny, nz), (hx, hy, hz) = dims(cfg)
    V = nx * ny * nz
    voxel = np.asarray(voxel, np.int64)
    rec = np.asarray(rec, F).reshape(-1, 8)
    times = np.asarray(times, F).reshape(-1)
    vx, vy, px, py = rec[:, 1], rec[:, 2], rec[:, 4], rec[:, 5]
    q = quanta(rec[:, 7])
    static = (vx == 0) & (vy == 0)
    zi = voxel // (nx * ny)
    acc = np.zeros((len(times), V), np.int64)
    stat = np.zeros(V, np.int64)
    np.add.at(stat, voxel[static], q[static])
    mv = ~static
    dropped = 0
    for j, t in enumerate(times):
        t = F(t)
        with np.errstate(invalid="ignore"):
            fx = (px[mv] + (vx[mv] * t).astype(F)).astype(F)
            fy = (py[mv] + (vy[mv] * t).astype(F)).astype(F)
            inside = (np.abs(fx) < hx) & (np.abs(fy) < hy)      # (false for a NaN)
            xi = np.trunc(np.where(inside, ((fx + hx).astype(F) / res).astype(F), F(0))).astype(np.int64)
            yi = np.trunc(np.where(inside, ((fy + hy).astype(F) / res).astype(F), F(0))).astype(np.int64)
        over = inside & ((xi >= nx) | (yi >= ny))
        dropped += int(over.sum())
        keep = inside & ~over
        np.add.at(acc[j], ((zi[mv] * ny + yi) * nx + xi)[keep], q[mv][keep])
        acc[j] += stat
    return value(acc), acc, dropped


def layers_loop(cfg, voxel, rec, times):
    """the same, one particle and one layer at a time in plain Python (the check of the vectorised restatement)"""
    res, (nx, ny, nz), (hx, hy, hz) = dims(cfg)
    acc = [[0] * (nx * ny * nz) for _ in times]
    dropped = 0
    for v, r in zip(voxel, np.asarray(rec, F).reshape(-1, 8)):
        w = F(r[7]) * SCALE
        q = 0 if (np.isnan(w) or w < 0) else int(np.rint(F(w)))
        vx, vy, px, py = F(r[1]), F(r[2]), F(r[4]), F(r[5])
        for j, t in enumerate(times):
            if vx == 0 and vy == 0:
                acc[j][int(v)] += q
                continue
            with np.errstate(invalid="ignore"):
                fx = F(px + F(vx * F(t)))
                fy = F(py + F(vy * F(t)))
            if not (abs(fx) < hx and abs(fy) < hy):
                continue
            xi, yi = int(F(F(fx + hx) / res)), int(F(F(fy + hy) / res))
            if xi >= nx or yi >= ny:
                dropped += 1
                continue
            acc[j][((int(v) // (nx * ny)) * ny + yi) * nx + xi] += q
    return value(np.array(acc, np.int64)), dropped


def layer_index(times, t):
    """(j, hi): j = the smallest index with times[j] >= t, n where there is none"""
    times = np.asarray(times, F)
    t = np.asarray(t, F)
    with np.errstate(invalid="ignore"):
        ge = times[None, :] >= t[:, None]
    return np.where(ge.any(1), ge.argmax(1), len(times))


def query(cfg, lay, times, samples, world=False, lerp=False, cur_pos=(0.0, 0.0, 0.0), outside=1.0):
    """values [n] float32 of samples [n, 4] over the layers lay [n_times, V]"""
    times = np.asarray(times, F)
    n = len(times)
    q = np.ascontiguousarray(samples, F).reshape(-1, 4)
    p = q[:, :3].copy()
    if world:
        p = (p - np.asarray(cur_pos, F)[None, :]).astype(F)
    nan = np.isnan(q).any(1)
    inside, g = Q.own_voxel(cfg, np.where(nan[:, None], F(0), p))
    inside &= ~nan
    t = np.where(nan, F(0), q[:, 3])
    j = layer_index(times, t)
    jc = np.minimum(j, n - 1)
    val = lay[jc, g]
    if lerp:
        mid = (j > 0) & (j < n)
        jm = np.where(mid, j, 1 if n > 1 else 0)
        a, b = lay[jm - 1, g], lay[jm, g]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            u = ((t - times[jm - 1]).astype(F) / (times[jm] - times[jm - 1]).astype(F)).astype(F)
            li = (a + (u * (b - a).astype(F)).astype(F)).astype(F)
        val = np.where(mid, li, val)
    return np.where(inside, val, F(outside)).astype(F)
