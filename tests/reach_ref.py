"""numpy restatement of the arrival-time fields grown through the cast grid (include/dspmap.h, dspmap_build_reach_fields and
dspmap_reach_paths), on bool cells [L, nz, ny, nx] as tests/cast_ref.py and tests/corridor_ref.py have them, plus checkers of a result
that know nothing of how it was grown.

Independent of the kernel's structure: no words, no shifts, no carries, no workgroups.  A set is a bool array [n_fields, nz, ny, nx], a
step ORs the six one-cell translations of it (slices, so nothing wraps and nothing leaves the map) and removes the blocked cells of the
step's layers; the steps are a plain Python loop that, like the definition, runs to max_steps (it stops early only when every set is
empty, or nothing changed and the schedule has reached its last layer -- both provably idle).  The point, frame and horizon rules are those
of tests/query_ref (_dims, horizons) and the fp32 expressions of cast_ref."""
import numpy as np

from tests import query_ref as Q

F = np.float32
POINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("field", "i4")])
UNREACHED = 65535
MAX_FIELDS, MAX_STEPS = 64, 4096
NEIGHBOURS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))   # (dx, dy, dz) in the order -x, +x, -y, +y, -z, +z


def unpack(words, nx):
    """uint64 [..., W] (DSPMap.cast_grid) -> bool [..., nx]"""
    words = np.asarray(words, np.uint64)
    b = ((words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    return b.reshape(words.shape[:-1] + (-1,))[..., :nx]


def pack(cells):
    """bool [..., nx] -> uint64 [..., W] (DSPMap.set_cast_grid)"""
    cells = np.asarray(cells, bool)
    nx = cells.shape[-1]
    W = (nx + 63) // 64
    padded = np.zeros(cells.shape[:-1] + (W * 64,), np.uint64)
    padded[..., :nx] = cells
    return (padded.reshape(cells.shape[:-1] + (W, 64)) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def points(rows):
    """POINT_DTYPE [n] from rows (x, y, z, field)"""
    out = np.zeros(len(rows), POINT_DTYPE)
    for i, (x, y, z, f) in enumerate(rows):
        out[i] = (x, y, z, f)
    return out


def point_cells(cfg, pts, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """(finite [n], inside [n], ijk [n, 3] as x, y, z -- meaningful where inside) of POINT_DTYPE points"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    p = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(F)
    finite = np.isfinite(p).all(1)
    hv = np.array(half, F)[None, :]
    with np.errstate(all="ignore"):
        if world:
            p = (p - np.asarray(cur_pos, F)[None, :]).astype(F)
        inside = finite & (np.abs(p) < hv).all(1)                 # dspmap_point_voxel_index: p >= half or p <= -half is outside
        u = ((p + hv).astype(F) / res).astype(F)
        ijk = np.trunc(np.where(inside[:, None], u, F(0))).astype(np.int64)
    inside &= (ijk < np.array(n, np.int64)[None, :]).all(1)       # cast step 2: trunc(u) >= n is outside
    return finite, inside, ijk


def schedule(cfg, t_start, step_seconds, max_steps):
    """int [max_steps + 1]: the layer step n tests (besides layer 0 with WITH_CURRENT)"""
    T, pred = Q._dims(cfg)[:2]
    n = np.arange(max_steps + 1)
    if T == 0 or F(t_start) < F(0):
        return np.zeros(max_steps + 1, np.int64)
    with np.errstate(all="ignore"):
        t = (F(t_start) + (n.astype(F) * F(step_seconds)).astype(F)).astype(F)
    return Q.horizons(pred, t) + 1


def time_invariant(cfg, t_start, step_seconds, max_steps):
    lay = schedule(cfg, t_start, step_seconds, max_steps)
    return bool(lay[0] == lay[-1])


def blocked_at(lay, layers, n, with_current=False):
    """B_n: bool [nz, ny, nx]"""
    b = lay[layers[n]]
    return (b | lay[0]) if with_current else b


def _grown(R):
    """R u N6(R) on the three last axes (z, y, x); nothing wraps, the outside of the map does not exist"""
    g = R.copy()
    g[..., :, :, 1:] |= R[..., :, :, :-1]
    g[..., :, :, :-1] |= R[..., :, :, 1:]
    g[..., :, 1:, :] |= R[..., :, :-1, :]
    g[..., :, :-1, :] |= R[..., :, 1:, :]
    g[..., 1:, :, :] |= R[..., :-1, :, :]
    g[..., :-1, :, :] |= R[..., 1:, :, :]
    return g


def source_sets(cfg, src, n_fields, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """S_f: bool [n_fields, nz, ny, nx]"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    S = np.zeros((n_fields, n[2], n[1], n[0]), bool)
    src = np.asarray(src, POINT_DTYPE).reshape(-1)
    if len(src):
        finite, inside, ijk = point_cells(cfg, src, world, cur_pos)
        ok = inside & (src["field"] >= 0) & (src["field"] < n_fields)
        S[src["field"][ok], ijk[ok, 2], ijk[ok, 1], ijk[ok, 0]] = True
    return S


def fields(cfg, lay, src, n_fields, t_start=-1.0, step_seconds=0.0, max_steps=MAX_STEPS, world=False, with_current=False,
           cur_pos=(0.0, 0.0, 0.0), return_sets=False):
    """uint16 [n_fields, nz, ny, nx]; with return_sets also the list of the sets R_0 .. R_last (bool arrays) it went through"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    lay = np.asarray(lay, bool)
    assert lay.shape == (T + 1, n[2], n[1], n[0]) and 1 <= n_fields <= MAX_FIELDS and 1 <= max_steps <= MAX_STEPS
    layers = schedule(cfg, t_start, step_seconds, max_steps)
    val = np.full((n_fields, n[2], n[1], n[0]), UNREACHED, np.uint16)
    R = source_sets(cfg, src, n_fields, world, cur_pos) & ~blocked_at(lay, layers, 0, with_current)[None]
    val[R] = 0
    sets = [R.copy()]
    for k in range(1, max_steps + 1):
        new = _grown(R) & ~blocked_at(lay, layers, k, with_current)[None]
        val[new & (val == UNREACHED)] = k
        same = np.array_equal(new, R)
        R = new
        if return_sets:
            sets.append(R.copy())
        if not R.any() or (same and (layers[k:] == layers[k]).all()):
            break
    return (val, sets) if return_sets else val


def paths(cfg, val, starts, max_len, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """(steps int32 [n], cells int32 [n, max_len]) of starts (POINT_DTYPE) down the time-invariant fields val [n_fields, nz, ny, nx]"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    nx, ny, nz = n
    starts = np.asarray(starts, POINT_DTYPE).reshape(-1)
    steps = np.full(len(starts), -3, np.int32)
    cells = np.full((len(starts), max_len), -1, np.int32)
    if not len(starts):
        return steps, cells
    finite, inside, ijk = point_cells(cfg, starts, world, cur_pos)
    for i in range(len(starts)):
        f = int(starts["field"][i])
        if not finite[i] or not 0 <= f < val.shape[0]:
            continue                                              # -3
        if not inside[i]:
            steps[i] = -2
            continue
        x, y, z = (int(v) for v in ijk[i])
        v = int(val[f, z, y, x])
        if v == UNREACHED:
            steps[i] = -1
            continue
        steps[i] = v
        for j in range(max_len):
            cells[i, j] = (z * ny + y) * nx + x
            if v == 0:
                break
            for dx, dy, dz in NEIGHBOURS:
                a, b, c = x + dx, y + dy, z + dz
                if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz and int(val[f, c, b, a]) == v - 1:
                    x, y, z, v = a, b, c, v - 1
                    break
            else:
                break                                             # no such neighbour: the path stops, the rest stays -1
    return steps, cells


# ---- checkers: properties of a result, whatever produced it

def check_free(cfg, lay, val, t_start=-1.0, step_seconds=0.0, max_steps=MAX_STEPS, with_current=False):
    """every reached cell is free at the step it was reached, and no value exceeds max_steps; returns the number of reached cells"""
    val = np.asarray(val)
    layers = schedule(cfg, t_start, step_seconds, max_steps)
    reached = val != UNREACHED
    assert (val[reached] <= max_steps).all()
    for v in np.unique(val[reached]):
        b = blocked_at(lay, layers, int(v), with_current)
        hit = (val == v) & b[None]
        assert not hit.any(), ("a cell reached at a step at which it is blocked", int(v), np.argwhere(hit)[:3])
    return int(reached.sum())


def check_predecessors(cfg, lay, val, src, t_start=-1.0, step_seconds=0.0, max_steps=MAX_STEPS, world=False, with_current=False,
                       cur_pos=(0.0, 0.0, 0.0)):
    """a cell of value 0 is a free source cell and every free source cell has value 0; a cell of value v > 0 has a face neighbour that
    arrived by step v - 1 and is free at step v - 1 (what membership of R_{v-1} implies).  In a time-invariant build in addition: that
    neighbour's value is exactly v - 1, values of free neighbours differ by at most 1, and an unreached free cell has no reached
    neighbour below max_steps.  Returns the number of cells of value > 0."""
    val = np.asarray(val)
    nf = val.shape[0]
    layers = schedule(cfg, t_start, step_seconds, max_steps)
    S = source_sets(cfg, src, nf, world, cur_pos) & ~blocked_at(lay, layers, 0, with_current)[None]
    assert np.array_equal(val == 0, S), "the cells of value 0 are not the free source cells"
    big = np.int64(1 << 20)
    v64 = np.where(val == UNREACHED, big, val.astype(np.int64))
    invariant = bool(layers[0] == layers[-1])
    pos = (val != UNREACHED) & (val > 0)
    found = np.zeros(val.shape, bool)
    exact = np.zeros(val.shape, bool)
    pad = np.pad(v64, ((0, 0), (1, 1), (1, 1), (1, 1)), constant_values=big)
    nz, ny, nx = val.shape[1:]
    # free_at[l]: cells free in what a step of layer l tests
    free_of_layer = {int(l): ~blocked_at(lay, np.array([l]), 0, with_current) for l in np.unique(layers)}
    prev_layer = layers[np.clip(v64 - 1, 0, max_steps)]           # the layer of step v - 1, per cell
    for dx, dy, dz in NEIGHBOURS:
        nb = pad[:, 1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
        nb_free = np.zeros(val.shape, bool)
        for l, fr in free_of_layer.items():
            shifted = np.pad(fr, 1, constant_values=False)[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
            nb_free |= (prev_layer == l) & shifted[None]
        found |= pos & (nb <= v64 - 1) & nb_free
        exact |= pos & (nb == v64 - 1)
        if invariant:
            fr = free_of_layer[int(layers[0])]
            both = (v64 < big) & (nb < big)
            assert (np.abs(v64 - nb)[both] <= 1).all(), "neighbouring reached cells differ by more than one step"
            orphan = fr[None] & (v64 == big) & (nb < max_steps)
            assert not orphan.any(), "a free unreached cell next to a cell reached before max_steps"
    assert found[pos].all(), ("a reached cell without a predecessor", np.argwhere(pos & ~found)[:3])
    if invariant:
        assert exact[pos].all(), ("a cell of value v without a neighbour of value v - 1", np.argwhere(pos & ~exact)[:3])
    return int(pos.sum())


def check_paths(cfg, val, starts, steps, cells, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """the paths start in their start's cell with its value, are 6-connected, fall by exactly one per cell, end at value 0 or fill
    max_len, and are -1 behind the end; returns the number of complete paths (those that end at a cell of value 0)"""
    T, pred, res, n, half, corr = Q._dims(cfg)
    nx, ny, nz = n
    starts = np.asarray(starts, POINT_DTYPE).reshape(-1)
    steps, cells = np.asarray(steps), np.asarray(cells)
    finite, inside, ijk = point_cells(cfg, starts, world, cur_pos)
    max_len = cells.shape[1]
    done = 0
    for i in range(len(starts)):
        f = int(starts["field"][i])
        if not finite[i] or not 0 <= f < val.shape[0]:
            assert steps[i] == -3 and (cells[i] == -1).all()
            continue
        if not inside[i]:
            assert steps[i] == -2 and (cells[i] == -1).all()
            continue
        g0 = (int(ijk[i, 2]) * ny + int(ijk[i, 1])) * nx + int(ijk[i, 0])
        v0 = int(val[f].reshape(-1)[g0])
        if v0 == UNREACHED:
            assert steps[i] == -1 and (cells[i] == -1).all()
            continue
        assert steps[i] == v0
        length = min(v0 + 1, max_len)
        row = cells[i]
        assert (row[:length] >= 0).all() and (row[length:] == -1).all(), (i, v0, row[:8])
        if length == 0:
            continue
        assert row[0] == g0
        vals = val[f].reshape(-1)[row[:length]].astype(np.int64)
        assert np.array_equal(vals, v0 - np.arange(length)), (i, vals[:8])
        x, y, z = row[:length] % nx, (row[:length] // nx) % ny, row[:length] // (nx * ny)
        assert (np.abs(np.diff(x)) + np.abs(np.diff(y)) + np.abs(np.diff(z)) == 1).all(), i
        done += int(vals[-1] == 0)
    return done
