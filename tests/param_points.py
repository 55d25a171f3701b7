"""Parameter points off the defaults and the schedule of mid-run changes (helpers; no tests here), shared by
tests/test_runtime_params_cpu.py -- which asserts on the ORACLE ALONE that every point and every scheduled change is in effect -- and
tests/test_gpu_runtime_params.py, which holds the HIP map to the oracle at the points and its frame paths to each other under the schedule.

Two maps:
  * STAGE_CFG  40 x 40 x 20 at 0.15 m, 12 particles per voxel: the stage tests and the single frames against the oracle.  Its corner lies
    4.5 m from the sensor; weight_culls() (dspmap_kernels.hip) is true iff that is more than 12 * DSPMAP_P_PAIR_CULL_SIGMAS * sigma_ob, at
    the default 9 sigmas iff sigma_ob < 0.0417: SIGMA_CULLS = 0.03 selects k_weight<true> and the prepared pair path, SIGMA_MASKS = 0.2
    k_weight<false>.
  * the 16 x 16 x 6 map of tests/test_gpu_frame_params_by_value.py (corner at 1.756 m) for the frame paths.  At 9 sigmas no sigma_ob of
    0.03 .. 0.4 crosses the switch there (it lies at 0.0163), so every handle of those tests is created with BASE_CULL_SIGMAS = 4: the
    switch lies at 1.756 / 48 = 0.0366, between the schedule's 0.03 and 0.1.  That setting only ever meets other HIP handles with the same
    setting: a cull at 4 sigmas is no statement about the oracle.
"""
import functools

import numpy as np

from tests import common

STAGE_CFG = dict(nx=40, ny=40, nz=20, res=0.15, ppv=12)
STAGE_PARTICLES = 20000
SIGMA_CULLS, SIGMA_MASKS = 0.03, 0.2
BASE_CULL_SIGMAS = 4.0
IN_EFFECT_FRACTION, IN_EFFECT_REL = 0.05, 1e-3      # the bar of test_variant_multiple_neighbors_weight_update

# the example node's values (src/map_sim_example.cpp:522-526) and the constructor's for what the example leaves alone (:156-158, :70)
DEFAULT = dict(kappa=0.01, p_det=0.95, nb_weight=1e-4, occl_margin=0.3, sigma_ob=0.1)
KAPPA_PDET = ((0.01, 0.95), (0.0, 0.95), (1.0, 0.95), (0.01, 0.5), (0.01, 1.0))
NB_WEIGHTS = (1e-6, 1e-4, 0.04)
OCCL_MARGINS = (0.0, 0.15, 0.3)


def _points():
    pts = [("kappa%g_pdet%g" % kp, dict(kappa=kp[0], p_det=kp[1])) for kp in KAPPA_PDET]
    pts += [("nb_weight%g" % w, dict(nb_weight=w)) for w in NB_WEIGHTS]
    pts += [("occl_margin%g" % g, dict(occl_margin=g)) for g in OCCL_MARGINS]
    pts += [("sigma%g" % s, dict(sigma_ob=s)) for s in (SIGMA_CULLS, SIGMA_MASKS)]
    return pts


STAGE_POINTS = _points()                             # (name, what differs from DEFAULT); three of them ARE the default point


def point_values(point):
    return dict(DEFAULT, **point)


def is_default(point):
    return point_values(point) == DEFAULT


def apply_point_oracle(o, point):
    v = point_values(point)
    o.L.dspo_set_kappa(o.h, v["kappa"])
    o.L.dspo_set_detection_probability(o.h, v["p_det"])
    o.L.dspo_set_newborn_weight(o.h, v["nb_weight"])
    o.L.dspo_set_occlusion_margin(o.h, v["occl_margin"])
    o.L.dspo_set_observation_stddev(o.h, v["sigma_ob"])


def apply_point_map(m, capi, point):
    v = point_values(point)
    m.set_param(capi.P_KAPPA, v["kappa"])
    m.set_param(capi.P_DETECTION, v["p_det"])
    m.setNewBornParticleWeight(v["nb_weight"])
    m.set_param(capi.P_OCCLUSION_MARGIN, v["occl_margin"])
    m.setObservationStdDev(v["sigma_ob"])


# ------------------------------------------------------------------------------------------------------ the stage scene
STAGE_SEED = 71
STAGE_CUR = (0.2, -0.1, 0.05)
STAGE_MOVE = (-0.01, 0.0, 0.002, 1 / 30.0)


@functools.lru_cache(maxsize=None)
def stage_inputs():
    """the scene of tests/test_gpu_parity.py's _setup_update_scene at the identity attitude, with every eighth point of its wall cloud: three
    tenths of the particles clustered around the observed surface, four tenths up to 0.45 m BEHIND an observation on its ray (the band
    the occlusion margins 0, 0.15 and 0.3 cut differently, :761), the rest spread over the map.  Why every eighth point: lambda, the expected
    number of newborns in Ck (:292, :737), is 0.002 per valid point at the example's values; with the full cloud's 2100 points it is 4.2
    and kappa = 0 against 0.01 moves no weight by 1e-3.  -> (points, (px, py, pz, vx, vy, vz, w)), read-only"""
    from oracle import oracle_py as orc
    half = common.half_extent(orc.make_config(**STAGE_CFG))
    rng = np.random.default_rng(STAGE_SEED)
    pts = common.wall_cloud(STAGE_SEED, n_side=60, dist=min(3.0, half[0] * 0.7), half_w=min(2.6, half[1] * 0.8), half_h=min(1.3, half[2] * 0.8))[::8].copy()
    k, kb = (STAGE_PARTICLES * 3) // 10, (STAGE_PARTICLES * 4) // 10
    near = (pts[rng.integers(0, len(pts), k)] + rng.normal(0, 0.12, (k, 3))).astype(np.float32)
    src = pts[rng.integers(0, len(pts), kb)].astype(np.float64)
    behind = (src * (1.0 + rng.uniform(0.0, 0.45, (kb, 1)) / np.linalg.norm(src, axis=1, keepdims=True)) + rng.normal(0, 0.01, (kb, 3))).astype(np.float32)
    near = np.concatenate([near, behind])
    k += kb
    bx, by, bz, bvx, bvy, bw = common.random_particles(STAGE_SEED + 1, STAGE_PARTICLES - k, half)
    z = np.zeros(k, np.float32)
    parts = [np.concatenate(ab).astype(np.float32) for ab in ((near[:, 0], bx), (near[:, 1], by), (near[:, 2], bz), (z, bvx), (z, bvy))]
    parts += [np.zeros(STAGE_PARTICLES, np.float32), np.concatenate([rng.uniform(0.005, 0.08, k).astype(np.float32), bw])]
    # no voxel near its 24 slots: which arrival an overfull voxel turns away depends on the order, and is no part of these tests.  The
    # clustered particles past the 16th of a voxel are put somewhere else in the map.
    res = np.float32(STAGE_CFG["res"])
    cell = [np.floor((parts[a] + np.float32(half[a])) / res).astype(np.int64) for a in range(3)]
    vox = (cell[2] * STAGE_CFG["ny"] + cell[1]) * STAGE_CFG["nx"] + cell[0]
    order = np.argsort(vox, kind="stable")
    rank = np.empty(len(vox), np.int64)
    rank[order] = np.arange(len(vox)) - np.searchsorted(vox[order], vox[order], side="left")
    over = np.nonzero(rank >= 16)[0]
    for a in range(3):
        parts[a][over] = rng.uniform(-0.95 * half[a], 0.95 * half[a], len(over)).astype(np.float32)
    for a in parts + [pts]:
        a.setflags(write=False)
    return pts, tuple(parts)


def stage_oracle(orc):
    o = orc.Oracle(orc.make_config(**STAGE_CFG))
    o.set_tables(*common.tables(STAGE_SEED))
    return o


def stage_birth_sources(orc, pts):
    """static and dynamic sources (matched and unmatched clusters) among the first 400 points, as test_config_update_and_birth tags them"""
    from tests.test_gpu_parity import _birth_sources
    return _birth_sources(orc, np.random.default_rng(7), pts[:min(400, len(pts))], STAGE_CUR, n_dyn=60)


def oracle_stage(orc, o, upto_update=False):
    """bin_points -> predict -> map_update [-> add_newborn] on an oracle that holds the scene's particles and the point's parameters"""
    pts, _ = stage_inputs()
    o.L.dspo_set_current_position(o.h, *STAGE_CUR)
    o.bin_points(pts)
    o.predict(*STAGE_MOVE)
    o.map_update()
    if not upto_update:
        o.L.dspo_use_velocity_estimator(o.h, 0)
        o.set_birth_cloud(stage_birth_sources(orc, pts))
        o.add_newborn()


@functools.lru_cache(maxsize=None)
def oracle_stage_run(name):
    """the oracle alone at one point, once per process: (particles after mapUpdate, newborns after the births, slots per voxel), copies"""
    from oracle import oracle_py as orc
    o = stage_oracle(orc)
    o.inject(*stage_inputs()[1])
    apply_point_oracle(o, dict(STAGE_POINTS)[name])
    oracle_stage(orc, o, upto_update=True)
    after_update = tuple(x.copy() for x in o.export_sparse())
    o.L.dspo_use_velocity_estimator(o.h, 0)
    o.set_birth_cloud(stage_birth_sources(orc, stage_inputs()[0]))
    o.add_newborn()
    v, s, r = o.export_sparse()
    nb = r[:, 0] > 10
    out = after_update, (v[nb].copy(), s[nb].copy(), r[nb].copy()), o.slots
    o.close()
    return out


DEFAULT_POINT = [n for n, p in STAGE_POINTS if is_default(p)][0]


# ------------------------------------------------------------------------------------------------------ the schedule
def swap_tables():
    """the tables a scheduled swap brings: other lengths than common.tables' 200003 / 50021, a position table three times as wide"""
    return common.tables(9, n=150001, sigma_p=0.15, sigma_v=0.05, nrand=40009)


class Change:
    """one scheduled change: applied BEFORE frame `frame` is fed.  kind: 'weights' (the weight update), 'birth' (number / weight of the
    newborns), 'draws' (which table entries the frame draws) -- what the oracle-only condition looks at.  on_oracle is None where the
    oracle has no such parameter (the pair cull is the HIP map's own approximation)."""

    def __init__(self, frame, name, kind, on_map, on_oracle, estimator_only=False):
        self.frame, self.name, self.kind, self.on_map, self.on_oracle, self.estimator_only = frame, name, kind, on_map, on_oracle, estimator_only

    def __repr__(self):
        return "%s@%d" % (self.name, self.frame)


def _swap_map(m, capi):
    m.set_tables(*swap_tables())


def _swap_oracle(o):
    o.set_tables(*swap_tables())


CURSORS = (70001, 50021, 333)            # inside the swapped tables (150001, 150001, 40009)

# frames 7, 10, 19, 28, 30 and 37 have a clearOccupancyMapPrediction pending (f % 3 == 1 or f % 10 == 0), the others do not
SCHEDULE = (
    Change(3, "sigma_to_culls", "weights", lambda m, c: m.setObservationStdDev(SIGMA_CULLS), lambda o: o.L.dspo_set_observation_stddev(o.h, SIGMA_CULLS)),
    Change(7, "sigma_back", "weights", lambda m, c: m.setObservationStdDev(0.1), lambda o: o.L.dspo_set_observation_stddev(o.h, 0.1)),
    Change(10, "pair_cull_sigmas", "weights", lambda m, c: m.set_param(c.P_PAIR_CULL_SIGMAS, 2.0), None),
    Change(12, "kappa", "weights", lambda m, c: m.set_param(c.P_KAPPA, 0.3), lambda o: o.L.dspo_set_kappa(o.h, 0.3)),
    Change(15, "p_det", "weights", lambda m, c: m.set_param(c.P_DETECTION, 0.6), lambda o: o.L.dspo_set_detection_probability(o.h, 0.6)),
    Change(19, "occl_margin", "weights", lambda m, c: m.set_param(c.P_OCCLUSION_MARGIN, 0.0), lambda o: o.L.dspo_set_occlusion_margin(o.h, 0.0)),
    Change(21, "nb_weight", "birth", lambda m, c: m.setNewBornParticleWeight(0.002), lambda o: o.L.dspo_set_newborn_weight(o.h, 0.002)),
    Change(24, "nb_number_8", "birth", lambda m, c: m.setNewBornParticleNumberofEachPoint(8), lambda o: o.L.dspo_set_newborn_number(o.h, 8)),
    Change(28, "nb_number_32", "birth", lambda m, c: m.setNewBornParticleNumberofEachPoint(32), lambda o: o.L.dspo_set_newborn_number(o.h, 32)),
    Change(30, "tables", "draws", _swap_map, _swap_oracle),
    Change(33, "cursors", "draws", lambda m, c: m.set_cursors(*CURSORS), lambda o: o.L.dspo_set_cursors(o.h, *CURSORS)),
    Change(37, "filter_resolution", "birth", lambda m, c: m.setOriginalVoxelFilterResolution(0.3),
           lambda o: o.L.dspo_set_voxel_filter_resolution(o.h, 0.3), estimator_only=True),
)
N_FRAMES = 40
# the frames of tests/test_gpu_frame_params_by_value.py's _frames carry 0, 1, 255, 256, 257 or 600 points in an order its seed picks; with this
# seed every frame behind a change has 255 points or more (asserted by tests/test_runtime_params_cpu.py): a change in front of an empty frame
# could not show.  The empty and the one-point frames fall between the changes.
FRAMES_SEED = 13
FROZEN_SPLIT = (3, 16)                  # (int)(20 * 0.15f), (int)(20 * 0.8f): what the late newborn-number changes must leave (:808-811)


def schedule(estimator):
    return [c for c in SCHEDULE if estimator or not c.estimator_only]


def at_frame(changes, f, skip=None):
    return [c for c in changes if c.frame == f and c.name != skip]


def clears(f):
    """clearOccupancyMapPrediction before some frames, not before others (the rule of tests/test_gpu_frame_params_by_value.py)"""
    return f % 3 == 1 or f % 10 == 0


# ------------------------------------------------------------------------------------------------------ "in effect"
def changed_fraction(a, b, slots):
    """a, b: (voxel, slot, records (n, 8)) of two runs.  The share of the particles of either run that the other does not hold in the same
    slot, or holds with a weight more than IN_EFFECT_REL apart (relative), or at another position."""
    ka, kb = a[0].astype(np.int64) * slots + a[1], b[0].astype(np.int64) * slots + b[1]
    both, ia, ib = np.intersect1d(ka, kb, return_indices=True)
    ra, rb = a[2][ia], b[2][ib]
    diff = (np.abs(ra[:, 7] - rb[:, 7]) > IN_EFFECT_REL * np.abs(rb[:, 7])) | (ra[:, 4:7] != rb[:, 4:7]).any(1)
    union = len(ka) + len(kb) - len(both)
    return (int(diff.sum()) + union - len(both)) / max(union, 1)


def in_effect(kind, a, b, slots):
    """the bar of the issue: more than 5 % of the live weights differ by more than 1e-3 relative; for the birth parameters a different
    number of particles (n_born) will do as well"""
    if kind == "birth" and len(a[0]) != len(b[0]):
        return True
    return changed_fraction(a, b, slots) > IN_EFFECT_FRACTION


def run_oracle(orc, cfg, frames, changes, upto, skip=None, estimator=2, tables_seed=5):
    """the oracle alone through frames 0 .. upto with the changes of the schedule (all but `skip`): -> (voxel, slot, records) after frame
    `upto`, and the frozen static / model split.  estimator: dspo_use_velocity_estimator's numbering (2: every point in view a static
    source -- the HIP map without an estimator; 1: the restated estimator)."""
    import ctypes as C
    o = orc.Oracle(orc.make_config(**cfg))
    o.set_tables(*common.tables(tables_seed))
    o.L.dspo_use_velocity_estimator(o.h, estimator)
    for f in range(upto + 1):
        for c in at_frame(changes, f, skip):
            if c.on_oracle:
                c.on_oracle(o)
        pts, pos, quat, t = frames[f]
        assert o.update(pts, pos, t, quat) == 1
    a, b = C.c_int(), C.c_int()
    assert o.L.dspo_birth_statics(o.h, C.byref(a), C.byref(b)) == 1
    out = tuple(x.copy() for x in o.export_sparse()), (a.value, b.value)
    o.close()
    return out
