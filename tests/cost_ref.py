"""numpy restatement of the clearance-weighted cost-to-go fields (include/dspmap.h, dspmap_build_cost_fields and dspmap_cost_paths), on
bool cells [nz, ny, nx] of ONE layer and a float32 layer of the distance field, plus checkers of a result that know nothing of how it was
computed.

Independent of the kernel's structure: no words, no levels, no buckets, no workgroups.  The weights are a sum of comparisons; the costs come
by repeated relaxation v = min(v, shifted v + w) over the six one-cell translations (slices, so nothing wraps and nothing leaves the map)
until nothing changes -- Bellman-Ford on the whole grid at once.  dijkstra() is a second voice for small cases: a heap, one cell at a time.
The point, frame and horizon rules are those of tests/reach_ref (point_cells, source_sets) and tests/query_ref (horizons)."""
import heapq

import numpy as np

from tests import query_ref as Q
from tests import reach_ref as R

F = np.float32
POINT_DTYPE = R.POINT_DTYPE
UNREACHED = 65535
MAX_BANDS, MAX_WEIGHT, MAX_FIELDS, MAX_COST = 4, 8, 64, 16384
NEIGHBOURS = R.NEIGHBOURS
BIG = np.int64(1 << 40)


def layer_of(cfg, t):
    """the ONE layer a build tests: 0 for t < 0 or a map without horizons, else 1 + k(t)"""
    T, pred = Q._dims(cfg)[:2]
    if T == 0 or not F(t) >= F(0):
        return 0
    return int(Q.horizons(pred, np.array([t], F))[0]) + 1


def weights(blocked, dist, bands):
    """uint8 [nz, ny, nx]: 0 where blocked, else 1 + the penalties of the bands (clearance, penalty) whose clearance the cell's fp32 distance
    lies under; dist may be None without bands"""
    blocked = np.asarray(blocked, bool)
    bands = list(bands)
    assert len(bands) <= MAX_BANDS
    w = np.ones(blocked.shape, np.int64)
    for clearance, penalty in bands:
        assert 0 <= penalty < MAX_WEIGHT and F(clearance) > 0
        w += int(penalty) * (np.asarray(dist, F) < F(clearance))
    assert w.max() <= MAX_WEIGHT
    return np.where(blocked, 0, w).astype(np.uint8)


def _shifted(v, d):
    """v moved by one cell: out[c] = v[c - d] for the neighbour offset d = (dx, dy, dz); BIG where the neighbour is outside the map"""
    dx, dy, dz = d
    pad = np.pad(v, ((0, 0), (1, 1), (1, 1), (1, 1)), constant_values=BIG)
    nz, ny, nx = v.shape[1:]
    return pad[:, 1 - dz:1 - dz + nz, 1 - dy:1 - dy + ny, 1 - dx:1 - dx + nx]


def fields(cfg, w, src, n_fields, max_cost=MAX_COST, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """uint16 [n_fields, nz, ny, nx] from the weights w (uint8, 0 = blocked) by relaxation to the fixed point"""
    w = np.asarray(w)
    assert 1 <= n_fields <= MAX_FIELDS and 1 <= max_cost <= MAX_COST
    free = w > 0
    S = R.source_sets(cfg, src, n_fields, world, cur_pos) & free[None]
    v = np.where(S, np.int64(0), BIG)
    w64 = w.astype(np.int64)[None]
    for _ in range(int(free.sum()) + 2):                          # (a shortest path enters a cell once: at most that many rounds)
        new = v
        for d in NEIGHBOURS:
            new = np.minimum(new, _shifted(v, d) + w64)
        new = np.where(free[None], new, BIG)
        if np.array_equal(new, v):
            break
        v = new
    else:
        raise AssertionError("the relaxation did not settle")
    return np.where(v <= max_cost, v, UNREACHED).astype(np.uint16)


def dijkstra(cfg, w, src, n_fields, max_cost=MAX_COST, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """the same fields from a heap, one cell at a time (small grids)"""
    w = np.asarray(w)
    nz, ny, nx = w.shape
    S = R.source_sets(cfg, src, n_fields, world, cur_pos) & (w > 0)[None]
    out = np.full((n_fields, nz, ny, nx), UNREACHED, np.uint16)
    for f in range(n_fields):
        best = {}
        heap = [(0, int(z), int(y), int(x)) for z, y, x in np.argwhere(S[f])]
        for item in heap:
            best[item[1:]] = 0
        heapq.heapify(heap)
        while heap:
            c, z, y, x = heapq.heappop(heap)
            if best.get((z, y, x), BIG) < c:
                continue
            if c <= max_cost:
                out[f, z, y, x] = c
            for dx, dy, dz in NEIGHBOURS:
                a, b, e = x + dx, y + dy, z + dz
                if 0 <= a < nx and 0 <= b < ny and 0 <= e < nz and w[e, b, a] > 0:
                    nc = c + int(w[e, b, a])
                    if nc < best.get((e, b, a), BIG):
                        best[(e, b, a)] = nc
                        heapq.heappush(heap, (nc, e, b, a))
    return out


def paths(cfg, val, w, starts, max_len, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """(cost int32 [n], cells int32 [n, max_len]) of starts (POINT_DTYPE) down the fields val: from a cell of value v > 0 the FIRST face
    neighbour, in the order -x, +x, -y, +y, -z, +z, whose value is exactly v - w(cell)"""
    nz, ny, nx = val.shape[1:]
    starts = np.asarray(starts, POINT_DTYPE).reshape(-1)
    cost = np.full(len(starts), -3, np.int32)
    cells = np.full((len(starts), max_len), -1, np.int32)
    if not len(starts):
        return cost, cells
    finite, inside, ijk = R.point_cells(cfg, starts, world, cur_pos)
    for i in range(len(starts)):
        f = int(starts["field"][i])
        if not finite[i] or not 0 <= f < val.shape[0]:
            continue                                              # -3
        if not inside[i]:
            cost[i] = -2
            continue
        x, y, z = (int(v) for v in ijk[i])
        v = int(val[f, z, y, x])
        if v == UNREACHED:
            cost[i] = -1
            continue
        cost[i] = v
        for j in range(max_len):
            cells[i, j] = (z * ny + y) * nx + x
            if v == 0:
                break
            want = v - int(w[z, y, x])
            for dx, dy, dz in NEIGHBOURS:
                a, b, c = x + dx, y + dy, z + dz
                if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz and int(val[f, c, b, a]) == want:
                    x, y, z, v = a, b, c, want
                    break
            else:
                break                                             # no such neighbour: the path stops, the rest stays -1
    return cost, cells


# ---- checkers: properties of a result, whatever produced it

def check_fields(cfg, w, val, src, max_cost=MAX_COST, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """a value 0 occurs iff the cell is a free source cell; a cell of value v > 0 has a face neighbour of value exactly v - w(cell); face
    neighbours that are both reached obey v(b) <= v(a) + w(b); a free unreached cell next to a reached one would cost more than max_cost;
    blocked cells are unreached; no value is above max_cost.  Returns the number of cells of value > 0."""
    val, w = np.asarray(val), np.asarray(w)
    nf = val.shape[0]
    free = w > 0
    S = R.source_sets(cfg, src, nf, world, cur_pos) & free[None]
    assert np.array_equal(val == 0, S), "the cells of value 0 are not the free source cells"
    reached = val != UNREACHED
    assert not (reached & ~free[None]).any(), "a blocked cell has a value"
    assert (val[reached] <= max_cost).all(), "a value above max_cost"
    v64 = np.where(reached, val.astype(np.int64), BIG)
    w64 = w.astype(np.int64)[None]
    pos = reached & (val > 0)
    exact = np.zeros(val.shape, bool)
    for d in NEIGHBOURS:
        nb = _shifted(v64, d)                                     # the value of the neighbour a step is taken FROM
        exact |= pos & (nb == v64 - w64)
        both = reached & (nb < BIG)
        assert (v64[both] <= (nb + w64)[both]).all(), "v(b) > v(a) + w(b) for reached face neighbours"
        orphan = free[None] & ~reached & (nb < BIG) & (nb + w64 <= max_cost)
        assert not orphan.any(), ("a free unreached cell that a reached neighbour reaches within max_cost", np.argwhere(orphan)[:3])
    assert exact[pos].all(), ("a cell of value v without a neighbour of value v - w", np.argwhere(pos & ~exact)[:3])
    return int(pos.sum())


def check_paths(cfg, val, w, starts, cost, cells, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """the paths start in their start's cell with its value, are 6-connected, fall by exactly the weight of the cell left, end at value 0 or
    fill max_len, and are -1 behind the end; returns the number of complete paths (those that end at a cell of value 0)"""
    nz, ny, nx = val.shape[1:]
    starts = np.asarray(starts, POINT_DTYPE).reshape(-1)
    cost, cells = np.asarray(cost), np.asarray(cells)
    finite, inside, ijk = R.point_cells(cfg, starts, world, cur_pos)
    max_len = cells.shape[1]
    wflat = np.asarray(w).reshape(-1).astype(np.int64)
    done = 0
    for i in range(len(starts)):
        f = int(starts["field"][i])
        if not finite[i] or not 0 <= f < val.shape[0]:
            assert cost[i] == -3 and (cells[i] == -1).all()
            continue
        if not inside[i]:
            assert cost[i] == -2 and (cells[i] == -1).all()
            continue
        g0 = (int(ijk[i, 2]) * ny + int(ijk[i, 1])) * nx + int(ijk[i, 0])
        vflat = val[f].reshape(-1)
        v0 = int(vflat[g0])
        if v0 == UNREACHED:
            assert cost[i] == -1 and (cells[i] == -1).all()
            continue
        assert cost[i] == v0
        row = cells[i]
        length = int((row >= 0).sum())
        assert (row[:length] >= 0).all() and (row[length:] == -1).all(), (i, v0, row[:8])
        if max_len == 0:
            continue
        assert length >= 1 and row[0] == g0
        vals = vflat[row[:length]].astype(np.int64)
        assert (vals != UNREACHED).all()
        assert np.array_equal(np.diff(vals), -wflat[row[:length - 1]]), (i, vals[:8])     # falls by w of the cell LEFT
        x, y, z = row[:length] % nx, (row[:length] // nx) % ny, row[:length] // (nx * ny)
        assert (np.abs(np.diff(x)) + np.abs(np.diff(y)) + np.abs(np.diff(z)) == 1).all(), i
        assert vals[-1] == 0 or length == max_len, (i, "the path ends before value 0 and before max_len")
        done += int(vals[-1] == 0)
    return done
