"""Edge configurations of what dspmap_create accepts, with one scene builder per kind of edge (helpers; no tests here).

Every scene states its COVERAGE CONDITIONS on the oracle's state (the check_* functions): a case cannot pass without touching the
edge it is named for.  tests/test_config_edges_cpu.py asserts them on every entry (oracle only), tests/test_gpu_config_edges.py
asserts them again around the stage it compares with the HIP map.

What the systematic resampler (:992-1048) can and cannot reach -- the conditions below follow from it:
  * a voxel with n >= 5 live particles leaves min(n, M) weight units; one particle that holds (nearly) all the weight survives
    once and is copied M - 1 times.  M copies -- the capacity of the kernels' per-voxel copy notes -- is never made, so the
    condition is "some voxel makes M - 1 copies, the most there is".
  * after resampling a voxel holds at most M < slots particles: "a completely full voxel" is a condition BEFORE the stage; after
    it the conditions are a live particle in slot 63 / 64 / slots - 1 and a folded-back (fat) particle.
  * M = 1 has two slots per voxel: n < 5 always, the stage only sums and clears flags (no copies, nothing folded).
"""
import numpy as np

from tests import common

T6 = (0.05, 0.2, 0.5, 1.0, 1.5, 2.0)
T10 = (0.05, 0.1, 0.2, 0.3, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0)
T16 = tuple(float(np.float32(0.05 + 0.13 * k)) for k in range(16))
SMALL = dict(nx=16, ny=16, nz=6)

# name -> configuration keywords (make_config of both sides), kind of coverage, storage order forced on the HIP handle (None: its own
# choice) and the storage order of the bit-identical partner handle (None: no partner)
EDGES = {
    "slots64": dict(cfg=dict(SMALL, ppv=32), kind="slots"),                       # first word exactly full; one-wave resampler at 64
    "slots66": dict(cfg=dict(SMALL, ppv=33), kind="slots"),                       # two bits in word two; k_resample_wg<2>, k_resample<2,*>
    "slots125": dict(cfg=dict(SMALL, ppv=25, safe_factor=5), kind="slots"),                 # the static-model header's factor, two words
    "slots128": dict(cfg=dict(SMALL, ppv=64), kind="slots"),                      # both words full, M = 64
    "m1": dict(cfg=dict(nx=3, ny=3, nz=3, ppv=1), kind="tiny"),                   # M = 1, 27 voxels in one partial tile
    "one_voxel": dict(cfg=dict(nx=1, ny=1, nz=1, ppv=9), kind="tiny"),            # V = 1
    "ragged_cubes": dict(cfg=dict(nx=18, ny=14, nz=10, ppv=12), kind="plain", tiling=1, partner=0),   # padding in x, y and z
    "planes_max": dict(cfg=dict(SMALL, ppv=12, angle=1, half_fov_h=64, half_fov_v=48), kind="planes"),  # 129 / 97 planes, CAPP = 2
    "angle5": dict(cfg=dict(SMALL, ppv=12, angle=5), kind="planes"),              # truncated pyramid counts
    "angle7": dict(cfg=dict(SMALL, ppv=12, angle=7), kind="planes"),
    "t0": dict(cfg=dict(SMALL, ppv=12, pred_times=()), kind="plain"),             # no rollout
    "t16": dict(cfg=dict(SMALL, ppv=12, pred_times=T16), kind="plain"),           # fullest window plan
    "wide": dict(cfg=dict(nx=2048, ny=8, nz=4, ppv=6, pred_times=T10), kind="wide", tiling=0, partner=1),   # collapsed window plan
}
# one map past 2^24 voxels (17.8 M; 71 M cells < 2^31; the oracle's arrays near 2.6 GB): what the packed (voxel << 7 | slot) of the
# constructor pre-fill could not address.  512 x 512 x 64 is exactly 2^24 voxels -- its highest packed value still fits 31 bits -- so
# the map is four layers taller.
BIG = dict(nx=512, ny=512, nz=68, ppv=2, pred_times=(0.5,))

SLOT_EDGES = [n for n, e in EDGES.items() if e["kind"] == "slots"]
TWO_WORD = [n for n in EDGES if (EDGES[n]["cfg"].get("safe_factor", 0) or 2) * EDGES[n]["cfg"]["ppv"] > 64]

# the immediate neighbours OUTSIDE the space: dspmap_create refuses each
OUTSIDE = {
    "ppv65": dict(SMALL, ppv=65),
    "slots129": dict(SMALL, ppv=43, safe_factor=3),
    "t17": dict(SMALL, ppv=12, pred_times=tuple(0.1 * (k + 1) for k in range(16)) + (9.9,)),   # (see outside_config: 17 horizons)
    "fov_h65": dict(SMALL, ppv=12, angle=1, half_fov_h=65, half_fov_v=48),
    "fov_v49": dict(SMALL, ppv=12, angle=1, half_fov_h=64, half_fov_v=49),
    "cells_2p31": dict(nx=1024, ny=1024, nz=1024, ppv=1),                           # 2^30 voxels x 2 slots
}


def outside_config(make_config, name):
    """a configuration structure for OUTSIDE[name]; 17 horizons do not fit the structure's table: the count alone says 17"""
    kw = dict(OUTSIDE[name])
    if name == "t17":
        kw["pred_times"] = kw["pred_times"][:16]
        c = make_config(**kw)
        c.prediction_times = 17
        return c
    return make_config(**kw)


def slots_of(name):
    c = EDGES[name]["cfg"]
    return (c.get("safe_factor", 0) or 2) * c["ppv"]


def make_pair(dsp, orc, name, seed=1, tiling="own"):
    """oracle + HIP handle of the named edge on the same tables; tiling: 'own' = the entry's storage order, else 0 / 1 / None"""
    e = EDGES[name]
    o = orc.Oracle(orc.make_config(**e["cfg"]))
    m = dsp.DSPMap(dsp.make_config(**e["cfg"]))
    til = e.get("tiling") if tiling == "own" else tiling
    if til is not None:
        m.set_param(dsp.capi.P_TILING, til)
    p, v, r = common.tables(seed)
    o.set_tables(p, v, r)
    m.set_tables(p, v, r)
    return o, m


# ------------------------------------------------------------------------------------------------------------------ scenes
def _grid(cfg):
    ix, iy, iz = np.meshgrid(np.arange(cfg.nx), np.arange(cfg.ny), np.arange(cfg.nz), indexing="ij")
    return ix.ravel(), iy.ravel(), iz.ravel()


def fill_plan(cfg, slots, seed):
    """particles per voxel, in common.uniform_per_voxel's voxel order: an OVER-FILLED box (slots + 2 each: the oracle turns the last two
    away and the voxel is completely full), an EMPTY box, in between 0 .. 1.5 M at random.  A one-voxel map has neither box."""
    rng = np.random.default_rng(seed)
    ix, iy, iz = _grid(cfg)
    M = cfg.max_particle_num_voxel
    cnt = rng.integers(0, M + M // 2 + 2, len(ix))
    full = (ix < max(1, cfg.nx // 4)) & (iy < max(1, cfg.ny // 2))
    empty = (ix >= cfg.nx - max(1, cfg.nx // 4)) & (iy >= cfg.ny // 2)
    if len(ix) == 1:
        full[:] = False; empty[:] = False
        cnt[:] = slots - 2
    cnt[full] = slots + 2
    cnt[empty] = 0
    return cnt, full, empty


def state_scene(o, seed=11, vmax=1.0, over_fill=True, newborn_frac=0.3):
    """px, py, pz, vx, vy, w, flag for inject_both: fill_plan's counts per voxel (over_fill=False: the uniform 1.2 M per voxel that does
    NOT reach the edges -- kept to show that the coverage conditions notice), heavy-tailed weights; the particles of the over-filled box
    do not move (their voxels stay full under a prediction step); the first particle of every fourth voxel holds nearly all of the
    voxel's weight and stands still: in a voxel with n >= M it is copied M - 1 times, in a full voxel its copies are folded back (:1037-1041)."""
    cfg = o.cfg
    M, slots = cfg.max_particle_num_voxel, o.slots
    rng = np.random.default_rng(seed)
    cnt, full, empty = fill_plan(cfg, slots, seed + 1)
    if not over_fill:
        cnt = np.full(len(cnt), int(1.2 * M))
        full = np.zeros(len(cnt), bool)
    kmax = int(cnt.max())
    px, py, pz, vx, vy, w = common.uniform_per_voxel(cfg, kmax, seed + 2, vmax=vmax, wlo=0.002, whi=0.05)
    vox = np.repeat(np.arange(len(cnt)), kmax)           # uniform_per_voxel: ix-major voxel order, kmax consecutive particles each
    j = np.tile(np.arange(kmax), len(cnt))
    w = (w * np.exp(rng.normal(0, 1.0, w.shape))).astype(np.float32)
    still = rng.random(len(w)) < 0.5
    vx[still | full[vox]] = 0.0
    vy[still | full[vox]] = 0.0
    heavy_voxel = vox % 4 == 0
    heavy = (j == 0) & heavy_voxel
    w[heavy_voxel] = rng.uniform(0.0011, 0.002, int(heavy_voxel.sum())).astype(np.float32)   # all of them together: below half a unit
    w[heavy] = np.float32(100.0)
    vx[heavy] = 0.0; vy[heavy] = 0.0      # (it stays out of k_rollout, whose windows take groups below 256 units of moving weight)
    flag = np.where(rng.random(len(w)) < newborn_frac, 15.0, 1.0).astype(np.float32)
    flag[heavy] = 1.0
    keep = j < cnt[vox]
    return tuple(a[keep] for a in (px, py, pz, vx, vy, w, flag))


def inject_state(o, m, seed=11, vmax=1.0, over_fill=True, newborn_frac=0.3):
    px, py, pz, vx, vy, w, flag = state_scene(o, seed, vmax, over_fill, newborn_frac)
    if m is None:
        o.inject(px, py, pz, vx, vy, np.zeros_like(px), w, flag)
        return len(o.export_sparse()[0])
    return common.inject_both(o, m, px, py, pz, vx, vy, w, flag)


def fan_cloud(cfg, rng_m=0.4, max_points=3000):
    """one point at the centre of every pyramid of the field of view (sensor frame, x forward), at a range inside the map box; a field
    of view with more than max_points pyramids: every pyramid of the first and the last row and column, every third one in between.
    (Why not all 12 288 of planes_max: the reference sums the birth normaliser 1 / Ck over all observations sequentially in fp32
    (:799-805); over 13 088 observations that sum is 1.06e-4 from the exact sum of its own terms -- the HIP map's fixed-point sum was
    1e-7 from it -- so the oracle is no yardstick for a 1e-4 bar there.  reference_normaliser_error() is asserted for every scene.)"""
    A = cfg.angle_resolution
    nh, nv = cfg.half_fov_h * 2 // A, cfg.half_fov_v * 2 // A
    az = np.radians(-cfg.half_fov_h + (np.arange(nh) + 0.5) * A)
    el = np.radians(-cfg.half_fov_v + (np.arange(nv) + 0.5) * A)
    AZ, EL = np.meshgrid(az, el, indexing="ij")       # the angles of the boundary planes: atan(y / x) and atan(z / x)
    r = min(rng_m, 0.8 * min(common.half_extent(cfg)))
    d = np.stack([np.ones_like(AZ), np.tan(AZ), np.tan(EL)], -1)
    if nh * nv > max_points:
        keep = np.zeros((nh, nv), bool)
        keep[::3, ::3] = True
        keep[0] = keep[-1] = True
        keep[:, 0] = keep[:, -1] = True
        d = d[keep]
    d = d.reshape(-1, 3)
    return (r * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def observation_cloud(cfg, seed=5):
    """a wall inside the map box + the fan: observations in the first and the last pyramid row and column"""
    half = common.half_extent(cfg)
    if half[0] * 0.7 <= 0.8:               # (a map too small for the wall's ground strip: the fan alone)
        return fan_cloud(cfg)
    wall = common.wall_cloud(seed, n_side=40, dist=min(3.0, half[0] * 0.7), half_w=min(2.6, half[1] * 0.8), half_h=min(1.3, half[2] * 0.8))
    wall = wall[(np.abs(wall[:, 0]) < half[0]) & (np.abs(wall[:, 1]) < half[1]) & (np.abs(wall[:, 2]) < half[2])]
    return np.concatenate([fan_cloud(cfg), wall]).astype(np.float32)


def wide_scene(o, seed=21):
    """the wide grid: a thin uniform fill (one particle in two voxels out of three, so that no pyramid list is cut), every other particle
    moving at up to 1.5 m/s, and M particles per voxel in the first and in the last 512 voxel indices (k_rollout takes its windows from 384
    moving particles per group of tiles on)"""
    cfg = o.cfg
    rng = np.random.default_rng(seed)
    px, py, pz, vx, vy, w = common.uniform_per_voxel(cfg, 1, seed, vmax=1.5, wlo=0.01, whi=0.05)
    keep = rng.random(len(px)) < 0.66
    still = rng.random(len(px)) < 0.5
    vx[still] = 0.0; vy[still] = 0.0
    ix, iy, iz = _grid(cfg)
    g = (iz * cfg.ny + iy) * cfg.nx + ix                 # the reference's voxel index (:1081): a group of 8 tiles is 512 of them
    ends = (g < 512) | (g >= o.V - 512)
    ex = common.uniform_per_voxel(cfg, cfg.max_particle_num_voxel, seed + 1, vmax=1.5, wlo=0.01, whi=0.05)
    sel = np.repeat(ends, cfg.max_particle_num_voxel)
    parts = [np.concatenate([a[keep], b[sel]]) for a, b in zip((px, py, pz, vx, vy, w), ex)]
    return tuple(parts) + (np.ones(len(parts[0]), np.float32),)


def inject_wide(o, m, seed=21):
    px, py, pz, vx, vy, w, flag = wide_scene(o, seed)
    if m is None:
        o.inject(px, py, pz, vx, vy, np.zeros_like(px), w, flag)
        return len(o.export_sparse()[0])
    return common.inject_both(o, m, px, py, pz, vx, vy, w, flag)


def inject_edge(name, o, m, seed=11, vmax=1.0, newborn_frac=0.3):
    """the named entry's state scene on both sides (m = None: the oracle alone)"""
    if EDGES[name]["kind"] == "wide":
        return inject_wide(o, m, seed + 10)
    return inject_state(o, m, seed, vmax=vmax, newborn_frac=newborn_frac)


# ------------------------------------------------------------------------------------------------------ coverage conditions
def slot_census(o):
    voxel, slot, rec = o.export_sparse()
    per_voxel = np.bincount(voxel, minlength=o.V)
    return voxel, slot, rec, per_voxel


def check_slot_coverage(o, need_full=True, need_empty=True):
    """live particles in slot 63 (when there is one), in slot 64 (two-word maps) and in the last slot; a completely full and a completely
    empty voxel; nothing beyond the last slot (export_sparse cannot show one: the particle array has exactly `slots` columns)"""
    voxel, slot, rec, per_voxel = slot_census(o)
    assert len(slot) and slot.max() == o.slots - 1, (slot.max() if len(slot) else None, o.slots)
    if o.slots > 63:
        assert (slot == 63).any(), "no live particle in slot 63"
    if o.slots > 64:
        assert (slot == 64).any(), "no live particle in slot 64"
    if need_full:
        assert (per_voxel == o.slots).any(), "no completely full voxel (fullest: %d of %d)" % (per_voxel.max(), o.slots)
    if need_empty:
        assert (per_voxel == 0).any(), "no completely empty voxel"
    assert per_voxel.max() <= o.slots
    return per_voxel


def check_resample_coverage(o, per_voxel_before):
    """after occupancy_resample: some voxel made M - 1 copies (flag 0.6 marks a copy, :1030), and a voxel that was full folded copies
    back into a fat particle (:1037-1041)"""
    M = o.cfg.max_particle_num_voxel
    voxel, slot, rec, per_voxel = slot_census(o)
    copies = np.bincount(voxel[np.abs(rec[:, 0] - 0.6) < 1e-3], minlength=o.V)
    assert copies.max() == M - 1, (copies.max(), M)
    assert per_voxel.max() <= M
    was_full = np.nonzero(per_voxel_before == o.slots)[0]
    fat = 0
    for v in was_full:
        wv = rec[voxel == v][:, 7]
        fat += len(wv) > 0 and wv.max() > 1.9 * float(o.results[v, 0]) / M      # (a survivor carries one unit, mass / M, unless folded)
    assert fat > 0, "no folded-back particle in a voxel that was full"


def check_plane_coverage(o):
    """observations in the first and the last pyramid row and column after bin_points"""
    A = o.cfg.angle_resolution
    nh, nv = o.cfg.half_fov_h * 2 // A, o.cfg.half_fov_v * 2 // A
    assert nh * nv == o.NP
    cnt = o.obs_count.reshape(nh, nv)
    assert cnt[0].any() and cnt[-1].any() and cnt[:, 0].any() and cnt[:, -1].any()
    assert cnt[0, 0] and cnt[-1, -1] and cnt[0, -1] and cnt[-1, 0]          # the four corner pyramids
    return nh, nv


def reference_normaliser_error(o):
    """after map_update: how far the reference's sequential fp32 sum of 1 / Ck (:799-805) is from the exact sum of the same terms"""
    cnt = o.obs_count
    inv = np.concatenate([np.float32(1) / o.obs[b, :cnt[b], 3] for b in np.nonzero(cnt)[0]]).astype(np.float32)
    exact = float(inv.astype(np.float64).sum())
    return abs(float(np.cumsum(inv, dtype=np.float32)[-1]) - exact) / exact


def check_wide_coverage(o, m=None):
    """moving particles in the first and in the last group of 8 tiles (512 voxel indices); after a prediction: no pyramid list of the
    oracle was offered more than the HIP map's lists accept before their cut"""
    voxel, slot, rec, per_voxel = slot_census(o)
    moving = voxel[(rec[:, 1] != 0) | (rec[:, 2] != 0)]
    assert (moving < 512).sum() >= 384 and (moving >= o.V - 512).sum() >= 384      # (384: from there on k_rollout uses its windows)
    return moving


# the wide grid is looked at ACROSS (yaw 90 degrees): along x every voxel beyond a few metres falls into the four pyramids around the
# axis and their lists would be cut, whatever the fill
WIDE_QUAT = (0.70710678, 0.0, 0.0, 0.70710678)


def quat_of(name):
    return WIDE_QUAT if EDGES[name]["kind"] == "wide" else (1.0, 0.0, 0.0, 0.0)


def check_lists_uncut(o):
    assert o.pyramid_candidates.max() <= common.capa(o.capp), (o.pyramid_candidates.max(), common.capa(o.capp))


def oracle_invariants_of_resample(o, orc_mod=None):
    """occupancy_resample on the present state: per-voxel mass conserved to fp32 rounding, counts <= M where a resampling ran, every
    flag 1 or 0.6 afterwards; returns the occupancy column"""
    M = o.cfg.max_particle_num_voxel
    voxel, slot, rec, per_voxel = slot_census(o)
    alive = rec[:, 7] >= np.float32(1e-3)
    mass_in = np.bincount(voxel[alive], weights=rec[alive, 7].astype(np.float64), minlength=o.V)
    n_in = np.bincount(voxel[alive], minlength=o.V)
    o.occupancy_resample()
    voxel2, slot2, rec2, per_voxel2 = slot_census(o)
    mass_out = np.bincount(voxel2, weights=rec2[:, 7].astype(np.float64), minlength=o.V)
    occ = o.results[:, 0].astype(np.float64)
    assert np.allclose(occ, mass_in, rtol=2e-5, atol=1e-7)
    assert np.allclose(mass_out, mass_in, rtol=2e-4, atol=1e-6)
    ran = n_in >= 5
    assert (per_voxel2[ran] <= np.minimum(n_in[ran], M)).all() and (per_voxel2[ran] >= 1).all()
    assert np.array_equal(per_voxel2[~ran], n_in[~ran])
    assert slot2.max() <= o.slots - 1
    assert set(np.unique(rec2[:, 0]).tolist()) <= {1.0, float(np.float32(0.6))}
    return occ
