"""Scenes with DENSE observations for the pair kernels (k_pyr_prepare's work items, k_ck_partial, k_weight), with their coverage
conditions and a float64 restatement of mapUpdate's pass 1 (helpers; no tests here).

Why: the wall clouds of the other stage tests leave at most 10 observations in a pyramid, so a 3x3 neighbourhood holds O <= 90 of them and
the pair kernels only ever take their first one or two shape-dependent paths.  The fan cloud below puts a CHOSEN number of points into
every pyramid: O runs from 0 to 891, crosses every switch point of the kernels exactly (O = 64 | 65, 128 | 129, 256 | 257), and 48 bins
are filled past the reference's cap of 99.

Every condition is computed from the ORACLE's state (obs_count, pyramid_lists, pyramid_candidates) -- never from the HIP side -- and is
asserted by tests/test_pair_scenes_cpu.py (oracle alone) and again by tests/test_gpu_pair_kernels.py around what it compares.

The constants that mirror the kernels (dsp-map_amd/csrc/dspmap_kernels.hip):
  * WU_SPLIT_AT   wu_split(O): 1, 2, 4 or 8 lanes share a particle in k_weight; an item is 256 / split particles
  * (the same three values are k_ck_partial's opad = 64, 128, 256 -> G = 4, 2, 1 particle groups)
  * STAGE_ROUND   k_weight<true> and k_ck_partial stage a neighbourhood's observations in rounds of 256
  * CK_SMALL_FOV  particles in the field of view up to which k_ck_partial's items are 32 particles, above 64
"""
import ctypes as C
import functools
import types

import numpy as np

from tests import common

KAPPA = 0.01            # dsp_dynamic.h's kappa: what Ck holds besides the pair sum once lambda is 0
P_DET = 0.95
OBS_CAP = 99            # observations a pyramid counts (:282-284); the 100th slot is written and never counted
WU_SPLIT_AT = (64, 128, 256)
WU_TPB = 256
STAGE_ROUND = 256
CK_SMALL_FOV = 60000
EXACT_O = (64, 65, 128, 129, 256, 257)
# classes of O: one per lane split, the last split once more per staging round (2, 3, 4 rounds)
O_CLASSES = ((1, 64), (65, 128), (129, 256), (257, 512), (513, 768), (769, 1 << 30))

# points per pyramid, per column h = 0 .. 27, equal on all 16 rows ...
COLUMNS = (0, 0, 1, 3, 5, 7, 7, 7, 7, 7, 7, 7, 14, 14, 14, 14, 14, 14, 28, 28, 28, 28, 28, 28, 60, 120, 120, 120)
# ... then the centre bin (row 8) of these columns is raised until the 3x3 sum around it is exactly this
EXACT_AT = {7: 64, 10: 65, 14: 128, 16: 129, 20: 256, 22: 257}
# 5x5 neighbourhoods: six full columns, 25-bin sums of 25 x 99 = 2475 > 2048 (10 staging rounds, 50 kB of dynamic LDS)
COLUMNS_5X5 = COLUMNS[:22] + (120,) * 6
TABLES = {"fan": (COLUMNS, EXACT_AT), "fan5x5": (COLUMNS_5X5, {})}

BIG = dict(nx=50, ny=50, nz=24, res=0.15, ppv=20)
# name -> configuration, observation stddev (both sides), particles, and what the scene is stated to select:
#   chunk   particles per k_ck_partial item (n_fov on that side of CK_SMALL_FOV)
#   variant the k_weight instantiation (DSPMap.weight_variant): 12 cull radii = 12 x 9 sigma against the map's corner (5.6 m for BIG)
SCENES = {
    "short_lists": dict(cfg=dict(nx=40, ny=40, nz=20, res=0.15, ppv=12), sigma=0.1, uniform=120000, near=0, table="fan", chunk=32,
                        variant="mask", emptied=((12, 8), (26, 3))),
    "long_lists": dict(cfg=BIG, sigma=0.1, uniform=600000, near=0, table="fan", chunk=64, variant="mask", emptied=()),
    "culled": dict(cfg=BIG, sigma=0.03, uniform=200000, near=3, table="fan", chunk=32, variant="skip", emptied=()),
    # the 5x5 neighbourhood (PYRAMID_NEIGHBOR_N = 2) at the default 3 degree pyramids, which dspmap_create accepts: the same fan, same map
    "wide5x5": dict(cfg=dict(BIG, neighbor_n=2), sigma=0.03, uniform=200000, near=3, table="fan5x5", chunk=32, variant="skip", emptied=()),
}


def wu_split(O):
    """lanes per particle in k_weight (wu_split)"""
    return 1 << sum(O > t for t in WU_SPLIT_AT)


def item_particles(O):
    return WU_TPB // wu_split(O)


def count_table(table):
    columns, exact = TABLES[table]
    cnt = np.repeat(np.asarray(columns, np.int64)[:, None], 16, axis=1)
    for h, target in exact.items():
        cnt[h, 8] += target - cnt[h - 1:h + 2, 7:10].sum()
    return cnt


def _pyramid_of(o, pts):
    """pyramid index of every point (-1: outside the field of view) by the oracle's own three functions; the planes are those of the
    oracle's last bin_points"""
    L, h = o.L, o.h
    out = np.full(len(pts), -1, np.int64)
    npv = o.cfg.half_fov_v * 2 // o.cfg.angle_resolution
    for i, (x, y, z) in enumerate(pts.tolist()):
        if L.dspo_in_pyramids_area(h, x, y, z):
            out[i] = L.dspo_pyramid_h(h, x, y, z) * npv + L.dspo_pyramid_v(h, x, y, z)
    return out


@functools.lru_cache(maxsize=None)
def dense_fan(table, seed=3, pool=150000):
    """the fan cloud of a count table (sensor frame = world frame, identity attitude): a pool of random directions inside the field of
    view (+-41.9 x +-23.9 degrees, ranges 1.0 .. 2.6 m) is binned by the oracle, the first cnt[h, v] points of every bin are taken and
    shuffled.  Returns (points (n, 3) float32, cnt (28, 16))"""
    from oracle import oracle_py as orc
    o = orc.Oracle(orc.make_config(nx=4, ny=4, nz=4, ppv=1))      # (the planes depend on the field of view alone)
    o.bin_points(np.zeros((0, 3), np.float32))
    rng = np.random.default_rng(seed)
    az = np.radians(rng.uniform(-41.9, 41.9, pool))
    el = np.radians(rng.uniform(-23.9, 23.9, pool))
    d = np.stack([np.ones(pool), np.tan(az), np.tan(el)], 1)
    pts = (rng.uniform(1.0, 2.6, pool)[:, None] * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    b = _pyramid_of(o, pts)
    o.close()
    cnt = count_table(table)
    have = np.bincount(b[b >= 0], minlength=cnt.size)
    assert have.min() >= cnt.max(), (have.min(), cnt.max())
    order = np.argsort(b, kind="stable")
    order = order[b[order] >= 0]
    rank = np.arange(len(order)) - np.concatenate([[0], np.cumsum(have)])[b[order]]
    take = order[rank < cnt.ravel()[b[order]]]
    out = pts[rng.permutation(take)]
    out.setflags(write=False)
    return out, cnt


def scene_particles(name, o, cloud):
    """px, py, pz, vx, vy, w of the named scene: all static (nothing moves under predict(0, 0, 0, dt), nothing is drawn)"""
    sc = SCENES[name]
    px, py, pz, vx, vy, w = common.random_particles(7, sc["uniform"], common.half_extent(o.cfg), static_frac=1.0)
    if sc["near"]:
        rng = np.random.default_rng(11)
        near = (np.repeat(cloud, sc["near"], axis=0) + rng.normal(0, sc["sigma"], (len(cloud) * sc["near"], 3))).astype(np.float32)
        wn = rng.uniform(0.2, 1.0, len(near)).astype(np.float32)
        z = np.zeros(len(near), np.float32)
        px, py, pz = (np.concatenate([a, near[:, k]]) for k, a in enumerate((px, py, pz)))
        vx, vy, w = np.concatenate([vx, z]), np.concatenate([vy, z]), np.concatenate([w, wn])
    if sc["emptied"]:
        npv = o.cfg.half_fov_v * 2 // o.cfg.angle_resolution
        o.bin_points(np.zeros((0, 3), np.float32))
        keep = ~np.isin(_pyramid_of(o, np.stack([px, py, pz], 1)), [h * npv + v for h, v in sc["emptied"]])
        px, py, pz, vx, vy, w = (a[keep] for a in (px, py, pz, vx, vy, w))
    return px, py, pz, vx, vy, w


@functools.lru_cache(maxsize=None)
def reference(name, own_lambda=False):
    """The oracle's run of a scene, once per process: inject, bin_points, predict(0, 0, 0, 1/30), lambda = 0 (own_lambda: the frame's
    own expected_new_born_objects stays), mapUpdate.  Everything a test needs is COPIED out (read-only) and the oracle is closed."""
    from oracle import oracle_py as orc
    sc = SCENES[name]
    o = orc.Oracle(orc.make_config(**sc["cfg"]))
    o.set_tables(*common.tables(1))
    o.L.dspo_set_observation_stddev(o.h, sc["sigma"])
    cloud, cnt_table = dense_fan(sc["table"])
    px, py, pz, vx, vy, w = scene_particles(name, o, cloud)
    o.inject(px, py, pz, vx, vy, np.zeros_like(px), w, 1.0)
    r = types.SimpleNamespace(name=name, scene=sc, cloud=cloud, cnt_table=cnt_table, capp=o.capp, slots=o.slots, NP=o.NP)
    r.voxel0, r.slot0, r.rec0 = o.export_sparse()                  # what both sides start from
    r.n_valid = o.bin_points(cloud)
    o.predict(0.0, 0.0, 0.0, 1 / 30.0)
    r.lam = float(o.L.dspo_expected_newborn(o.h))
    if not own_lambda:
        o.L.dspo_set_expected_newborn(o.h, 0.0)
    r.add = np.float32(0.0 if not own_lambda else np.float32(r.lam)) + np.float32(KAPPA)
    r.obs_count, r.obs_maxlen = o.obs_count.copy(), o.obs_max_length.copy()
    r.obs_xyz = o.obs[:, :, :3].copy()
    nbs = (2 * max(1, sc["cfg"].get("neighbor_n", 0)) + 1) ** 2 + 1          # the neighbour table's stride (:126-127): count + bins
    r.lists, r.cand = o.pyramid_lists.copy(), o.pyramid_candidates.copy()
    r.nb = o._view(o.L.dspo_neighbor_table(o.h), (o.NP, nbs), np.int32).copy()
    r.P = (r.lists[:, :, 0] & 1).sum(1)
    r.O = np.array([r.obs_count[r.nb[b, 1:1 + r.nb[b, 0]]].sum() for b in range(o.NP)])
    r.voxel1, r.slot1, r.rec1 = o.export_sparse()                  # after the prediction: the weights pass 1 reads
    r.pdf = o.pdf_lut.copy()
    o.L.dspo_map_update_ck(o.h)                                    # pass 1 alone: the pair sums
    r.raw = o.obs[:, :, 3].copy()
    o.L.dspo_map_update_weights(o.h)                               # += lambda + kappa (:737), pass 2
    r.ck = o.obs[:, :, 3].copy()
    r.voxel2, r.slot2, r.rec2 = o.export_sparse()
    o.close()
    for a in vars(r).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def counted(r, a):
    """the counted observations' entries of a per-slot array (NP, 100), pyramid-major"""
    return np.concatenate([a[b, :r.obs_count[b]] for b in np.nonzero(r.obs_count)[0]])


# ------------------------------------------------------------------------------------------------------ coverage conditions
def check_scene(r):
    """what one scene must reach (oracle state only)"""
    sc = r.scene
    assert r.n_valid == len(r.cloud) == r.cnt_table.sum()                                    # every point of the fan is valid
    assert np.array_equal(r.obs_count.reshape(r.cnt_table.shape), np.minimum(r.cnt_table, OBS_CAP))
    assert (r.obs_count == OBS_CAP).sum() >= 40 and (r.cnt_table > OBS_CAP).sum() >= 40      # bins cut to the reference's cap
    assert r.cand.max() <= r.capp, (r.cand.max(), r.capp)                                    # no list is cut
    assert np.array_equal(r.cand, r.P)
    assert len(r.voxel1) == len(r.voxel0) and np.array_equal(r.rec1[:, 4:8], r.rec0[:, 4:8])   # nothing moved, nothing left
    n_fov = int(r.P.sum())
    assert (n_fov <= CK_SMALL_FOV) == (sc["chunk"] == 32), n_fov
    for b in (h * r.cnt_table.shape[1] + v for h, v in sc["emptied"]):
        assert r.obs_count[b] > 0 and r.P[b] == 0, b                                         # observed, no particle: chunk 0 alone
    raw = counted(r, r.raw)
    assert np.median(raw) >= 5 * KAPPA, np.median(raw)                                       # the Ck bar bears on the pair sum
    if sc["table"] == "fan":
        assert r.O.max() == 891
        assert ((r.O == 0) & (r.P > 0)).sum() >= 8                                           # pyramids nobody observes, with particles
        for x in EXACT_O:
            assert ((r.O == x) & (r.P > 0)).sum() >= 3, x
    else:
        assert r.O.max() > 8 * STAGE_ROUND                                                   # nine staging rounds or more
    return n_fov


def check_classes(refs):
    """over the union of the given scenes: every class of O has a pyramid whose list fits ONE k_weight item and one whose list does not"""
    for lo, hi in O_CLASSES:
        fits = more = 0
        for r in refs:
            item = np.array([item_particles(x) for x in r.O])
            cls = (r.O >= lo) & (r.O <= hi) & (r.P > 0)
            fits += int((cls & (r.P <= item)).sum())
            more += int((cls & (r.P > item)).sum())
        assert fits and more, (lo, hi, fits, more)


def expected_items(r):
    """(k_ck_partial items, k_weight items, particles per k_ck_partial item) from the oracle's P and O: pyr_items_block's rule"""
    chunk = 32 if r.P.sum() <= CK_SMALL_FOV else 64
    ck = int(((r.P[r.O > 0] + chunk - 1) // chunk).sum())
    wu = int(sum(max(1, -(-int(p) * wu_split(int(x)) // WU_TPB)) for p, x in zip(r.P, r.O)))
    return ck, wu, chunk


# ------------------------------------------------------------------------------------------------------ float64 restatement
def lut_pdf(pdf, x, mu, sigma):
    """queryNormalPDF (:1294-1301) in fp32: the reference's index arithmetic, value for value"""
    c = (x - mu) / np.float32(sigma)
    c = np.minimum(np.maximum(c, np.float32(-9.9)), np.float32(9.9))
    return pdf[(c * np.float32(1000) + np.float32(10000)).astype(np.int32)]


def restate_pass1(r, samples):
    """mapUpdate's pass 1 (:709-735) for the observations (b, j) of `samples`: the terms (P_d w) ((a b) c) in fp32 as the reference forms
    them, their sum in float64.  Returns (sums, number of terms)"""
    index = np.full(int(r.voxel1.max()) * r.slots + r.slots, -1, np.int64)
    index[r.voxel1.astype(np.int64) * r.slots + r.slot1] = np.arange(len(r.voxel1))
    sums, terms = [], []
    for b, j in samples:
        ob = r.obs_xyz[b, j]
        ent = np.concatenate([r.lists[q][(r.lists[q, :, 0] & 1) == 1, 1:3] for q in r.nb[b, 1:1 + r.nb[b, 0]]])
        rec = r.rec1[index[ent[:, 0].astype(np.int64) * r.slots + ent[:, 1]]]
        g = (lut_pdf(r.pdf, rec[:, 4], ob[0], r.scene["sigma"]) * lut_pdf(r.pdf, rec[:, 5], ob[1], r.scene["sigma"])) \
            * lut_pdf(r.pdf, rec[:, 6], ob[2], r.scene["sigma"])
        t = (np.float32(P_DET) * rec[:, 7]) * g
        assert t.dtype == np.float32
        sums.append(float(t.astype(np.float64).sum()))
        terms.append(len(t))
    return np.array(sums), np.array(terms)


def sample_observations(r, n, seed=0):
    """n counted observations (b, j), at random over the scene, plus the first observation of every emptied pyramid"""
    b = np.repeat(np.arange(r.NP), r.obs_count)
    j = np.concatenate([np.arange(c) for c in r.obs_count])
    pick = np.random.default_rng(seed).choice(len(b), n, replace=False)
    extra = [(h * r.cnt_table.shape[1] + v, 0) for h, v in r.scene["emptied"]]
    return [(int(b[k]), int(j[k])) for k in pick] + extra
