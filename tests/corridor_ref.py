"""numpy restatement of the free boxes grown in the cast grid (include/dspmap.h, dspmap_grow_boxes), on bool cells [L, nz, ny, nx] as
tests/cast_ref.py has them, plus three checkers of a result that know nothing of how it was grown.

Independent of the kernel's structure: no words, no lanes, no votes.  The end-point, frame and horizon rules are those of cast_ref
(tests/query_ref._dims and .horizons, cast_ref's fp32 expressions).  The seeds are grouped by the set of layers they test; per group the
blocked cells are the OR of those layers, and "is a blocked cell in this slab?" is a count from the cells' summed volume (cumulative
sums along the three axes), so that a face test is one vectorised expression over the seeds.  The rounds and the faces
are plain Python loops in the order the definition gives; `order` lets a test grow with another order."""
import numpy as np

from tests import query_ref as Q

F = np.float32
BOX_DTYPE = np.dtype([("lo", "i4", (3,)), ("hi", "i4", (3,)), ("status", "i4"), ("stop", "u4")])
OK, SEED_BLOCKED, SEED_OUTSIDE, INVALID = 0, 1, 3, 4
OBSTACLE, EDGE, LIMIT = 1, 2, 3
MAX_GROW = 64


def unpack(words, nx):
    """uint64 [..., W] (DSPMap.cast_grid) -> bool [..., nx]"""
    words = np.asarray(words, np.uint64)
    b = ((words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    return b.reshape(words.shape[:-1] + (-1,))[..., :nx]


def seed_cells(cfg, seg, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """steps 1 and 2: (valid [n], inside [n], lo [n, 3], hi [n, 3]) -- lo, hi are meaningful where inside"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    seg = np.ascontiguousarray(seg, F).reshape(-1, 8)
    valid = np.isfinite(seg[:, 0:3]).all(1) & np.isfinite(seg[:, 4:7]).all(1) & ~np.isnan(seg[:, 3]) & ~np.isnan(seg[:, 7])
    nn = np.array(n, np.int64)
    hv = np.array(half, F)[None, :]
    inside = valid.copy()
    cells = []
    with np.errstate(all="ignore"):
        for p in (seg[:, 0:3].copy(), seg[:, 4:7].copy()):
            if world:
                p = (p - np.asarray(cur_pos, F)[None, :]).astype(F)
            inside &= (np.abs(p) < hv).all(1)                      # dspmap_point_voxel_index: p >= half or p <= -half is outside
            u = ((p + hv).astype(F) / res).astype(F)
            i = np.trunc(np.where(inside[:, None], u, F(0))).astype(np.int64)
            inside &= (i < nn[None, :]).all(1)
            cells.append(i)
    return valid, inside, np.minimum(cells[0], cells[1]), np.maximum(cells[0], cells[1])


def tested_layers(cfg, seg, with_current=False):
    """step 3: bool [n, L], the layers each seed tests (rows of invalid seeds mean nothing)"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    seg = np.ascontiguousarray(seg, F).reshape(-1, 8)
    ta, tb = seg[:, 3], seg[:, 7]
    with np.errstate(invalid="ignore"):
        timed = ~(ta < F(0)) & (T > 0)
        la = np.where(timed, Q.horizons(pred, ta) + 1, 0)
        lb = np.where(timed, Q.horizons(pred, tb) + 1, 0)         # (a negative tb: horizon -1, layer 0)
    l0, l1 = np.minimum(la, lb), np.maximum(la, lb)
    layer = np.arange(T + 1)[None, :]
    mask = (l0[:, None] <= layer) & (layer <= l1[:, None])
    if with_current:
        mask[:, 0] = True
    return mask


def _summed(blocked):
    """[nz + 1, ny + 1, nx + 1] int32: S[z, y, x] = blocked cells with indices below (z, y, x)"""
    s = np.zeros(tuple(k + 1 for k in blocked.shape), np.int32)
    s[1:, 1:, 1:] = blocked.astype(np.int32).cumsum(0).cumsum(1).cumsum(2)
    return s


def _count(s, g, lo, hi):
    """blocked cells in the inclusive boxes lo .. hi ([m, 3] as x, y, z) of the summed volumes s[g]"""
    x0, y0, z0 = lo[:, 0], lo[:, 1], lo[:, 2]
    x1, y1, z1 = hi[:, 0] + 1, hi[:, 1] + 1, hi[:, 2] + 1
    return (s[g, z1, y1, x1] - s[g, z0, y1, x1] - s[g, z1, y0, x1] - s[g, z1, y1, x0]
            + s[g, z0, y0, x1] + s[g, z0, y1, x0] + s[g, z1, y0, x0] - s[g, z0, y0, x0])


def grow(cfg, lay, seg, max_grow, world=False, with_current=False, cur_pos=(0.0, 0.0, 0.0), order=(0, 1, 2, 3, 4, 5)):
    """BOX_DTYPE [n] of seeds [n, 8] = {ax, ay, az, ta, bx, by, bz, tb} in bool layers [L, nz, ny, nx]"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    lay = np.asarray(lay, bool)
    assert lay.shape == (T + 1, n[2], n[1], n[0])
    g = [int(v) for v in max_grow]
    assert len(g) == 3 and all(0 <= v <= MAX_GROW for v in g) and sorted(order) == list(range(6))
    seg = np.ascontiguousarray(seg, F).reshape(-1, 8)
    out = np.zeros(len(seg), BOX_DTYPE)
    out["lo"], out["hi"], out["status"] = -1, -1, INVALID
    valid, inside, slo_all, shi_all = seed_cells(cfg, seg, world, cur_pos)
    out["status"][valid & ~inside] = SEED_OUTSIDE
    sel = np.flatnonzero(inside)
    if sel.size == 0:
        return out
    mask = tested_layers(cfg, seg, with_current)[sel]
    sets, gid = np.unique(mask, axis=0, return_inverse=True)      # the distinct sets of tested layers and each seed's
    gid = gid.reshape(-1)
    s = np.stack([_summed(lay[np.flatnonzero(m)].any(0)) for m in sets])
    slo, shi = slo_all[sel], shi_all[sel]
    seed_blocked = _count(s, gid, slo, shi) > 0
    lo, hi = slo.copy(), shi.copy()
    stop = np.zeros(len(sel), np.uint32)
    active = np.repeat(~seed_blocked[:, None], 6, 1)
    tests = np.zeros(len(sel), np.int64)
    while active.any():
        for f in order:
            a, up = f >> 1, f & 1
            idx = np.flatnonzero(active[:, f])
            if idx.size == 0:
                continue
            tests[idx] += 1
            c = hi[idx, a] + 1 if up else lo[idx, a] - 1
            edge = (c < 0) | (c >= n[a])
            limit = ~edge & ((c - shi[idx, a] if up else slo[idx, a] - c) > g[a])
            test = ~edge & ~limit
            s0, s1 = lo[idx].copy(), hi[idx].copy()
            s0[:, a] = s1[:, a] = np.where(test, c, 0)
            obstacle = test & (_count(s, gid[idx], s0, s1) > 0)
            cause = np.where(edge, EDGE, np.where(limit, LIMIT, np.where(obstacle, OBSTACLE, 0))).astype(np.uint32)
            stopped = cause > 0
            stop[idx[stopped]] |= cause[stopped] << np.uint32(2 * f)
            active[idx[stopped], f] = False
            (hi if up else lo)[idx[~stopped], a] = c[~stopped]
    assert tests.max() <= 6 * (MAX_GROW + 1), "a box takes at most 6 * (DSPMAP_BOX_MAX_GROW + 1) face tests"
    out["lo"][sel], out["hi"][sel], out["stop"][sel] = lo, hi, stop      # (a blocked seed: its seed box, no causes)
    out["status"][sel] = np.where(seed_blocked, SEED_BLOCKED, OK)
    return out


# ---- three checkers of a result that know nothing of the algorithm: plain loops over the boxes, slices of the bool cells ----
def _blocked_in(lay, layers, lo, hi):
    """brute force: is any cell of the inclusive box lo .. hi (x, y, z; clipped by nothing -- it must lie inside) set in one of `layers`?"""
    return bool(lay[layers, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].any())


def check_contains_seed(cfg, seg, boxes, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """every box with indices contains the voxels of both end points (tests/query_ref.own_voxel: getPointVoxelsIndexPublic); returns how many"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    seg = np.ascontiguousarray(seg, F).reshape(-1, 8)
    has = np.flatnonzero((boxes["status"] == OK) | (boxes["status"] == SEED_BLOCKED))
    for p in (seg[has, 0:3], seg[has, 4:7]):
        if world:
            p = (p - np.asarray(cur_pos, F)[None, :]).astype(F)
        inside, gidx = Q.own_voxel(cfg, p)
        assert inside.all()
        cell = np.stack([gidx % n[0], (gidx // n[0]) % n[1], gidx // (n[0] * n[1])], 1)
        assert ((boxes["lo"][has] <= cell) & (cell <= boxes["hi"][has])).all()
    none = (boxes["status"] == SEED_OUTSIDE) | (boxes["status"] == INVALID)
    assert (boxes["lo"][none] == -1).all() and (boxes["hi"][none] == -1).all() and (boxes["stop"][none] == 0).all()
    assert (none.sum() + has.size) == len(boxes)
    return has.size


def check_free(cfg, lay, seg, boxes, with_current=False):
    """no cell of an OK box is blocked in a tested layer, and a SEED_BLOCKED box holds a blocked cell; returns how many OK boxes"""
    mask = tested_layers(cfg, seg, with_current)
    nn = np.array([cfg.nx, cfg.ny, cfg.nz])
    count = 0
    for i in np.flatnonzero((boxes["status"] == OK) | (boxes["status"] == SEED_BLOCKED)):
        lo, hi = boxes["lo"][i], boxes["hi"][i]
        assert (lo >= 0).all() and (lo <= hi).all() and (hi < nn).all(), i
        blocked = _blocked_in(lay, np.flatnonzero(mask[i]), lo, hi)
        assert blocked == (boxes["status"][i] == SEED_BLOCKED), i
        count += not blocked
    return count


def check_causes(cfg, lay, seg, boxes, max_grow, with_current=False, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """the recorded cause of every face of an OK box is true of the FINAL box: OBSTACLE -- the next slab holds a blocked cell and lies inside
    the map and the limit; EDGE -- c is outside the map; LIMIT -- c is inside the map and beyond max_grow from the seed box.  Returns the
    number of faces seen per cause {1: .., 2: .., 3: ..}"""
    mask = tested_layers(cfg, seg, with_current)
    valid, inside, slo, shi = seed_cells(cfg, seg, world, cur_pos)
    nn = (cfg.nx, cfg.ny, cfg.nz)
    seen = {OBSTACLE: 0, EDGE: 0, LIMIT: 0}
    for i in np.flatnonzero(boxes["status"] == OK):
        lo, hi, stop = boxes["lo"][i].astype(np.int64), boxes["hi"][i].astype(np.int64), int(boxes["stop"][i])
        assert stop >> 12 == 0, i
        for f in range(6):
            a, up = f >> 1, f & 1
            cause = (stop >> (2 * f)) & 3
            c = hi[a] + 1 if up else lo[a] - 1
            dist = c - shi[i, a] if up else slo[i, a] - c
            assert 1 <= dist <= max_grow[a] + 1, (i, f)      # the box grew from the seed box and never past the limit
            if cause == EDGE:
                assert c < 0 or c >= nn[a], (i, f)
            elif cause == LIMIT:
                assert 0 <= c < nn[a] and dist > max_grow[a], (i, f)
            else:
                assert cause == OBSTACLE and 0 <= c < nn[a] and dist <= max_grow[a], (i, f)
                s0, s1 = lo.copy(), hi.copy()
                s0[a] = s1[a] = c
                assert _blocked_in(lay, np.flatnonzero(mask[i]), s0, s1), (i, f)
            seen[cause] += 1
    blocked = boxes["status"] == SEED_BLOCKED
    assert (boxes["stop"][blocked] == 0).all()
    assert (boxes["lo"][blocked] == slo[blocked]).all() and (boxes["hi"][blocked] == shi[blocked]).all()
    return seen
