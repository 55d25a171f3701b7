"""numpy restatement of dspmap_track_update (include/dspmap.h): the objects of one build associated with those of the previous update by
voxel overlap after a predicted shift, mutual best matches, ids that persist.  Input per update: the label grid int32 [nz, ny, nx] and the
records (OBJECT_DTYPE, already cut at max_objects) of a build of objects, and the current position.  float64 for the predicted shift, each
operation rounded on its own; plain Python / numpy integers for the rest: the device has to give the same integers, bit for bit.

Also the scene the tests run: scene(shape) is a sequence of (occupancy bool [nz, ny, nx], position) made of a few boxes that stand still in
the world or move by integer steps while the window moves under them; scene_events() finds, on the restatement's own output, the events the
sequence has to contain."""
import numpy as np

from tests.objects_ref import OBJECT_DTYPE

TRACK_DTYPE = np.dtype([("id", "i8"), ("parent", "i8"), ("prev_sum_x", "i8"), ("prev_sum_y", "i8"), ("prev_sum_z", "i8"), ("prev_count", "i4"),
                        ("prev_ordinal", "i4"), ("age", "i4"), ("born_seq", "i4"), ("overlap", "i4"), ("shift_x", "i4"), ("shift_y", "i4"), ("shift_z", "i4")])
F = np.float32
MAX_SLOTS = 1 << 24


def window(pos, shape, res):
    """(k0 int [3], g float64 [3]): the world lattice index of map voxel 0 per axis, the known-space layer's expression"""
    n = np.array(shape, np.float64)
    cur = np.asarray(pos, F).astype(np.float64)
    g = cur / np.float64(F(res)) - n / 2.0
    return np.floor(g + 0.5).astype(np.int64), g


def table_slots(max_pairs, capacity):
    """slots of the pair table: max_pairs (0: 8 x the record capacity, at least 1024) rounded up to a power of two, at most 2^24"""
    want = max_pairs if max_pairs > 0 else max(8 * capacity, 1024)
    s = 1
    while s < want and s < MAX_SLOTS:
        s <<= 1
    return s


def predicted(rec, dt, res, max_shift):
    """(p int64 [k, 3] clamped, raw float64 [k, 3] before the clamp): the predicted shift of every record in voxels"""
    k = len(rec)
    raw = np.zeros((k, 3), np.float64)
    mass = rec["mass_q"].astype(np.int64)
    ok = mass > 0
    if ok.any():
        v = rec["mom_q"][ok].astype(np.float64) / mass[ok].astype(np.float64)[:, None]
        d = v * np.float64(F(dt))
        e = d / np.float64(F(res))
        raw[ok] = np.floor(e + 0.5)
    p = np.clip(raw, -float(max_shift), float(max_shift))
    return p.astype(np.int64), raw


class Tracker:
    """the tracker's state through updates: update() returns (tracks TRACK_DTYPE [K_now], counts (6 ints), fault 0 / 1) and leaves what it
    looked at in self.info"""

    def __init__(self, shape, res):
        self.shape, self.res = tuple(shape), res
        self.reset()

    def reset(self):
        self.prev = None          # (labels, records, tracks, k0) of the previous update
        self.next_id, self.seq = 0, 0
        self.info = None

    def update(self, labels, rec, pos, dt, min_overlap=1, max_shift=8, slots=None):
        nx, ny, nz = self.shape
        labels = np.asarray(labels).reshape(nz, ny, nx).astype(np.int64)
        assert rec.dtype == OBJECT_DTYPE
        k0, g = window(pos, self.shape, self.res)
        kn = len(rec)
        stored = len(self.prev[1]) if self.prev is not None else 0
        fresh = self.prev is None
        dk0 = np.zeros(3, np.int64)
        if not fresh:
            dk0 = k0 - self.prev[3]
            if (np.abs(dk0) >= np.array([nx, ny, nz])).any():
                fresh = True
        kp = 0 if fresh else stored
        pairs, shift, p, raw = {}, np.zeros((kp, 3), np.int64), np.zeros((kp, 3), np.int64), np.zeros((kp, 3))
        if kp:
            plab, prec = self.prev[0], self.prev[1]
            p, raw = predicted(prec, dt, self.res, max_shift)
            shift = p - dk0[None, :]
            z, y, x = np.nonzero((plab >= 0) & (plab < kp))
            j = plab[z, y, x]
            xx, yy, zz = x + shift[j, 0], y + shift[j, 1], z + shift[j, 2]
            ins = (xx >= 0) & (xx < nx) & (yy >= 0) & (yy < ny) & (zz >= 0) & (zz < nz)
            j, o = j[ins], labels[zz[ins], yy[ins], xx[ins]]
            ok = (o >= 0) & (o < kn)
            key, cnt = np.unique(j[ok] * (1 << 20) + o[ok], return_counts=True)
            pairs = {(int(k) >> 20, int(k) & 0xfffff): int(c) for k, c in zip(key, cnt)}
        seq = self.seq
        self.seq += 1
        self.info = dict(k0=k0, g=g, dk0=dk0, fresh=fresh, stored=stored, pairs=pairs, p=p, raw=raw, shift=shift, seq=seq)
        if slots is not None and len(pairs) > slots:      # the table is full: the update is void, the stored state emptied
            self.prev = None
            self.info["void"] = True
            return np.zeros(0, TRACK_DTYPE), (0, 0, 0, 0, 0, self.next_id), 1
        bj, bo = {}, {}                                    # o -> (n, j) / j -> (n, o): the largest n, ties to the smaller index
        for (j, o), n in sorted(pairs.items()):
            if o not in bj or n > bj[o][0] or (n == bj[o][0] and j < bj[o][1]):
                bj[o] = (n, j)
            if j not in bo or n > bo[j][0] or (n == bo[j][0] and o < bo[j][1]):
                bo[j] = (n, o)
        tr = np.zeros(kn, TRACK_DTYPE)
        born = 0
        for o in range(kn):
            t = tr[o]
            n, j = bj.get(o, (0, -1))
            if j >= 0 and bo[j][1] == o and n >= min_overlap:
                pt, po = self.prev[2][j], self.prev[1][j]
                t["id"], t["parent"], t["born_seq"], t["age"] = pt["id"], pt["parent"], pt["born_seq"], pt["age"] + 1
                t["prev_ordinal"], t["overlap"] = j, n
                t["shift_x"], t["shift_y"], t["shift_z"] = shift[j]
                t["prev_count"] = po["count"]
                for a, ax in enumerate("xyz"):
                    t["prev_sum_" + ax] = int(po["sum_" + ax]) - int(po["count"]) * int(dk0[a])
            else:
                t["id"] = self.next_id + born
                born += 1
                t["parent"] = self.prev[2][j]["id"] if j >= 0 else -1
                t["born_seq"], t["age"], t["prev_ordinal"], t["overlap"] = seq, 0, -1, n
        self.next_id += born
        matched = kn - born
        self.prev = (labels.copy(), rec.copy(), tr.copy(), k0)
        return tr, (kn, matched, born, stored - matched, len(pairs), self.next_id), 0


def records(labels, mass_q=None, mom_q=None):
    """hand-made records (OBJECT_DTYPE) of a label grid int [nz, ny, nx] whose ordinals are 0 .. k - 1: count, box and index sums from the
    grid, mass_q [k] and mom_q [k, 3] as given (0 by default)"""
    labels = np.asarray(labels)
    k = int(labels.max()) + 1 if labels.size else 0
    rec = np.zeros(max(k, 0), OBJECT_DTYPE)
    for o in range(k):
        z, y, x = np.nonzero(labels == o)
        rec[o]["label"], rec[o]["count"] = (z[0] * labels.shape[1] + y[0]) * labels.shape[2] + x[0], x.size
        for ax, v in (("x", x), ("y", y), ("z", z)):
            rec[o]["min_" + ax], rec[o]["max_" + ax], rec[o]["sum_" + ax] = v.min(), v.max(), v.sum()
    if mass_q is not None:
        rec["mass_q"] = mass_q
    if mom_q is not None:
        rec["mom_q"] = mom_q
    return rec


def states(tracks, rec, res, dt):
    """(displacement, velocity) float32 [k, 3], as DSPMap.track_states"""
    res = float(F(res))
    cnt = np.maximum(rec["count"], 1)[:, None].astype(np.float64)
    pcnt = np.maximum(tracks["prev_count"], 1)[:, None].astype(np.float64)
    mean = np.stack([rec["sum_x"], rec["sum_y"], rec["sum_z"]], 1) / cnt
    prev = np.stack([tracks["prev_sum_x"], tracks["prev_sum_y"], tracks["prev_sum_z"]], 1) / pcnt
    disp = np.where((tracks["prev_ordinal"] >= 0)[:, None], (mean - prev) * res, 0.0)
    vel = disp / float(dt) if float(dt) > 0.0 else np.zeros_like(disp)
    return disp.astype(F), vel.astype(F)


# ---- the scene
BASE = (5, -7, 2)                 # k0 of step 0: off zero on every axis, one of them negative
FRAC = (0.3, -0.3)                # g = k0 + frac: a fractional part of 0.3 rounds down, one of 0.7 up
BLOCK_STEPS = 2                   # the last steps of a scene: one thick block that stays where it is -- it overlaps itself under any shift
                                  # of up to two cells per axis, so a predicted shift can be seen on a MATCHED track


def position(k0, shape, res, frac):
    """a float32 position whose window is k0 and whose g has the fractional part frac (mod 1)"""
    return tuple(F((k + n / 2.0 + frac) * float(F(res))) for k, n in zip(k0, shape))


def _box(x0, x1, y0, y1, z0, z1):
    return [(x, y, z) for z in range(z0, z1 + 1) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1)]


def _steps_small():
    """3 x 3 x 3: single cells and one row.  (cells in the coordinates of step 0's window, offset of the window against step 0)"""
    p, row = [(1, 1, 1)], _box(0, 2, 0, 0, 0, 0)
    ends = [(0, 0, 0), (2, 0, 0)]
    return [(p, (0, 0, 0)), (p, (1, 0, 0)), (p, (1, 1, 0)), (p, (1, 1, 1)), (p, (0, 1, 1)), (p, (0, 0, 1)), (p, (0, 0, 0)),
            (row, (0, 0, 0)),                         # the cell vanishes, a row appears
            (ends, (0, 0, 0)),                        # the row splits into its two ends: equal counts, the smaller ordinal keeps the id
            (row, (0, 0, 0)),                         # they merge again: equal counts, the smaller previous ordinal gives the id
            (row, "jump"), (row, "jump")] + [(_box(0, 2, 0, 2, 0, 2), "jump")] * (1 + BLOCK_STEPS)


def _steps_general(nx, ny, nz):
    """maps of at least 16 x 12 x 6: boxes two cells thick in y and z, in three bands of y that never touch"""
    a, a_l, a_r = _box(1, 6, 1, 2, 1, 2), _box(1, 2, 1, 2, 1, 2), _box(4, 6, 1, 2, 1, 2)      # splits 8 : 12
    b, c, bc = _box(9, 10, 1, 2, 1, 2), _box(12, 14, 1, 2, 1, 2), _box(9, 14, 1, 2, 1, 2)    # merge 8 : 12
    d, e, de = _box(1, 2, 5, 6, 3, 4), _box(4, 5, 5, 6, 3, 4), _box(1, 5, 5, 6, 3, 4)        # merge 8 : 8, a tie
    f, f_l, f_r = _box(8, 12, 5, 6, 3, 4), _box(8, 9, 5, 6, 3, 4), _box(11, 12, 5, 6, 3, 4)  # splits 8 : 8, a tie
    g, h = _box(1, 2, 9, 10, 1, 2), _box(5, 6, 9, 10, 1, 2)                                  # vanishes / appears
    mv = [(_box(60 + s, 62 + s, 9, 10, 3, 4) if nx > 64 else _box(9 + s, 11 + s, 9, 10, 3, 4)) for s in range(3)]   # walks over x = 63 | 64
    return [(a + b + c + d + e + f + g + mv[0], (0, 0, 0)),
            (a + b + c + d + e + f + g + mv[1], (1, 0, 0)),
            (a_l + a_r + b + c + d + e + f + g + mv[2], (1, 1, 0)),
            (a_l + a_r + bc + d + e + f + g + mv[2], (1, 1, 1)),
            (a_l + a_r + bc + de + f + g + mv[2], (0, 1, 1)),
            (a_l + a_r + bc + de + f_l + f_r + mv[2], (0, 0, 1)),
            (a_l + a_r + bc + de + f_l + f_r + h + mv[2], (0, 0, 0)),
            (a_l + a_r + bc + de + f_l + f_r + h + mv[2], "jump"),
            (a_l + a_r + bc + de + f_l + f_r + h + mv[2], "jump")] + [(_box(1, 14, 1, ny - 2, 1, nz - 2), "jump")] * (1 + BLOCK_STEPS)


def scene(shape, res=0.15):
    """[(occ bool [nz, ny, nx], position (3 float32))] per step.  The boxes stand in the world (one walks along x); the window moves by one
    cell up and down every axis, then by the map's own length along x ("jump": the boxes go with it, nothing can be associated).  At the
    end everything merges into one thick block, which then stays for BLOCK_STEPS steps."""
    nx, ny, nz = shape
    steps = _steps_small() if min(shape) < 6 else _steps_general(nx, ny, nz)
    out = []
    for s, (cells, off) in enumerate(steps):
        jump = off == "jump"
        off = (0, 0, 0) if jump else off
        occ = np.zeros((nz, ny, nx), bool)
        for x, y, z in cells:
            x, y, z = x - off[0], y - off[1], z - off[2]
            assert 0 <= x < nx and 0 <= y < ny and 0 <= z < nz, (shape, s)
            occ[z, y, x] = True
        k0 = (BASE[0] + off[0] + (nx if jump else 0), BASE[1] + off[1], BASE[2] + off[2])
        pos = position(k0, shape, res, FRAC[s % 2])
        assert tuple(window(pos, shape, res)[0]) == k0
        out.append((occ, pos))
    return out


def scene_events(shape, runs):
    """what happened in a run of the restatement over a scene: runs = [(tracks, counts, info, records)] per step -> dict of booleans"""
    ev = dict(split=False, merge=False, vanish=False, appear=False, tie=False, crossing=False, fresh_jump=False, match=False)
    plus, minus, down, up = set(), set(), False, False
    for s, (tr, counts, info, rec) in enumerate(runs):
        fr = info["g"] - np.floor(info["g"])
        down |= bool((fr < 0.5).all())
        up |= bool((fr > 0.5).all())
        if s == 0:
            continue
        if info["fresh"]:
            ev["fresh_jump"] |= info["stored"] > 0 and counts[3] == info["stored"] and counts[2] == counts[0]
            continue
        for a in range(3):
            if info["dk0"][a] > 0 and counts[1] > 0:
                plus.add(a)
            if info["dk0"][a] < 0 and counts[1] > 0:
                minus.add(a)
        pairs = info["pairs"]
        matched = tr[tr["prev_ordinal"] >= 0]
        ev["match"] |= len(matched) > 0
        kept = set(int(j) for j in matched["prev_ordinal"])
        for t in tr[tr["prev_ordinal"] < 0]:
            if t["parent"] < 0:
                ev["appear"] = True
        for (j, o), n in pairs.items():
            if tr[o]["prev_ordinal"] < 0 and j in kept:          # a born object overlapped by a track that lives on
                ev["split"] = True
        for o in range(len(tr)):
            ns = sorted(n for (j, oo), n in pairs.items() if oo == o)
            if len(ns) >= 2:
                ev["merge"] |= tr[o]["prev_ordinal"] >= 0
                if ns[-1] == ns[-2]:
                    ev["tie"] |= tr[o]["prev_ordinal"] == min(j for (j, oo), n in pairs.items() if oo == o and n == ns[-1])
        ev["vanish"] |= any(all(j != jj for (jj, o) in pairs) for j in range(info["stored"]))
        on = (tr["prev_ordinal"] >= 0) & (rec["min_x"] <= 63) & (rec["max_x"] >= 64)
        ev["crossing"] |= bool(on.any())
    ev["dk0_plus"], ev["dk0_minus"] = plus == {0, 1, 2}, minus == {0, 1, 2}
    ev["rounds_down"], ev["rounds_up"] = down, up
    if shape[0] <= 64:
        ev["crossing"] = True          # (only maps of more than one word have the edge)
    return ev
