"""The oracle's side of the run-time filter parameters (no GPU): the two setters the reference has no counterpart for, pinned by the closed
form of mapUpdate for one particle and one observation; the frozen static / model split of the birth stage; and the conditions under which
tests/test_gpu_runtime_params.py means anything -- every parameter point and every scheduled change of tests/param_points.py is IN EFFECT on
the oracle (more than 5 % of the live weights move by more than 1e-3, or the number of newborns changes), so that no GPU test can pass on
a point or a schedule that does nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import common
from tests import param_points as PP
from tests.test_gpu_frame_params_by_value import CFG, _frames       # (helpers of a GPU test file; nothing here touches a device)


# ------------------------------------------------------------------------------------------------------ closed form
LAMBDA = 0.04


@pytest.mark.parametrize("kappa,p_det", PP.KAPPA_PDET)
def test_kappa_and_detection_probability_closed_form(orc, kappa, p_det):
    """One particle, one observation in its pyramid, nothing in the eight neighbours, lambda set by the caller:
         Ck = p_det w g + lambda + kappa (:732, :737),   w' = w ((1 - p_det) + p_det g / Ck) (:779, :786)
    with g the oracle's own product of three dspo_query_normal_pdf values: the algebra of the two new setters alone is under test.  The
    expression has fewer than eight fp32 roundings: 8 ulps."""
    o = orc.Oracle(orc.make_config(nx=40, ny=40, nz=20, ppv=12))
    o.set_tables(*common.tables(1))
    w = np.float32(0.5)
    z = np.zeros(1, np.float32)
    o.inject(np.array([2.0], np.float32), np.array([0.01], np.float32), np.array([0.01], np.float32), z, z, z, np.array([w]))
    assert o.bin_points(np.array([[2.05, 0.02, 0.0]], np.float32)) == 1
    o.predict(0.0, 0.0, 0.0, 0.0)
    b = int(np.nonzero(o.obs_count)[0][0])
    assert o.obs_count.sum() == 1 and (o.pyramid_lists[:, :, 0] & 1).sum() == 1 and (o.pyramid_lists[b, :, 0] & 1).sum() == 1
    o.L.dspo_set_expected_newborn(o.h, LAMBDA)          # (after binning, which sets the frame's own)
    o.L.dspo_set_kappa(o.h, kappa)
    o.L.dspo_set_detection_probability(o.h, p_det)
    _, _, rec = o.export_sparse()
    ob = o.obs[b, 0, :3]
    pdf = [o.L.dspo_query_normal_pdf(o.h, float(rec[0, 4 + k]), float(ob[k]), 0.1) for k in range(3)]
    g = float(np.float32(np.float32(pdf[0] * pdf[1]) * pdf[2]))
    assert g > 0.01
    o.map_update()
    ck = o.obs[b, 0, 3]
    w1 = o.export_sparse()[2][0, 7]
    pd, ka, la = float(np.float32(p_det)), float(np.float32(kappa)), float(np.float32(LAMBDA))
    ck_ref = pd * float(w) * g + la + ka
    w_ref = float(w) * ((1.0 - pd) + pd * g / ck_ref)
    assert abs(float(ck) - ck_ref) <= 8 * np.spacing(np.float32(ck_ref)), (ck, ck_ref)
    assert abs(float(w1) - w_ref) <= 8 * np.spacing(np.float32(w_ref)), (w1, w_ref)
    assert w1 != w                                       # (the update did touch the particle)
    o.close()


# ------------------------------------------------------------------------------------------------------ frozen statics
def _statics(o):
    a, b = C.c_int(), C.c_int()
    frozen = o.L.dspo_birth_statics(o.h, C.byref(a), C.byref(b))
    return frozen, (a.value, b.value)


def test_birth_statics_freeze_at_the_first_frame(orc):
    """(int)(n * 0.15f), (int)(n * 0.8f) of the newborn number AT THE FIRST BIRTH CALL (:808-811): 20 -> (3, 16) stays when 8 arrives
    later; a fresh map set to 8 first gets (1, 6).  The loop over a source's children runs to the current number all the same (:868)."""
    frames = [fr for fr in _frames(orc, 12, seed=11) if len(fr[0]) > 0][:3]
    late = orc.Oracle(orc.make_config(**CFG)); late.set_tables(*common.tables(5)); late.L.dspo_use_velocity_estimator(late.h, 2)
    assert _statics(late)[0] == 0
    pts, pos, quat, t = frames[0]
    assert late.update(pts, pos, t, quat) == 1
    assert _statics(late) == (1, (3, 16))
    n0 = late.L.dspo_count_live(late.h)
    late.L.dspo_set_newborn_number(late.h, 8)
    pts, pos, quat, t = frames[1]
    assert late.update(pts, pos, t, quat) == 1
    assert _statics(late) == (1, PP.FROZEN_SPLIT)
    early = orc.Oracle(orc.make_config(**CFG)); early.set_tables(*common.tables(5)); early.L.dspo_use_velocity_estimator(early.h, 2)
    early.L.dspo_set_newborn_number(early.h, 8)
    pts, pos, quat, t = frames[0]
    assert early.update(pts, pos, t, quat) == 1
    assert _statics(early) == (1, (1, 6))
    assert 0 < early.L.dspo_count_live(early.h) < n0      # 8 children per source instead of 20
    late.close(); early.close()


# ------------------------------------------------------------------------------------------------------ the stage points
@pytest.mark.parametrize("name", [n for n, p in PP.STAGE_POINTS if not PP.is_default(p)])
def test_stage_points_are_in_effect(name):
    """every parameter point of the stage parity test differs from the default point on the oracle by the bar of
    test_variant_multiple_neighbors_weight_update: weights after mapUpdate, or -- for the newborn weight -- the weights of the newborns"""
    upd0, born0, slots = PP.oracle_stage_run(PP.DEFAULT_POINT)
    upd, born, _ = PP.oracle_stage_run(name)
    frac_w, frac_b = PP.changed_fraction(upd, upd0, slots), PP.changed_fraction(born, born0, slots)
    print(name, "weights changed %.3f, newborn weights changed %.3f" % (frac_w, frac_b))
    assert len(born[0]) > 3000 and len(upd[0]) > 10000
    if name.startswith("nb_weight"):
        assert frac_b > PP.IN_EFFECT_FRACTION, frac_b
    else:
        assert frac_w > PP.IN_EFFECT_FRACTION, frac_w


def test_stage_points_cover_what_the_issue_names():
    names = dict(PP.STAGE_POINTS)
    assert len(names) == 13 and sum(PP.is_default(p) for p in names.values()) == 3
    assert {(p["kappa"], p["p_det"]) for p in map(PP.point_values, names.values())} >= set(PP.KAPPA_PDET)
    # one sigma on each side of weight_culls() at the stage map: the corner against 12 cull radii of 9 sigmas
    corner = float(np.linalg.norm(common.half_extent(_cfg_of(PP.STAGE_CFG))))
    assert 12 * 9 * PP.SIGMA_CULLS < corner < 12 * 9 * PP.SIGMA_MASKS
    assert 0.03 <= PP.SIGMA_CULLS and PP.SIGMA_MASKS <= 0.4


def _cfg_of(kw):
    from oracle import oracle_py as orc
    return orc.make_config(**kw)


# ------------------------------------------------------------------------------------------------------ the schedule
def test_schedule_crosses_the_weight_switch_on_the_small_map():
    """the frame-path tests' map with BASE_CULL_SIGMAS: 0.03 culls, 0.1 does not; every sigma inside pair_scenes' range; change frames with
    and without a pending clear; cursors inside the swapped tables, which have other lengths and a position table three times as wide"""
    corner = float(np.linalg.norm(common.half_extent(_cfg_of(CFG))))
    assert 12 * PP.BASE_CULL_SIGMAS * PP.SIGMA_CULLS < corner < 12 * PP.BASE_CULL_SIGMAS * 0.1
    assert corner < 12 * 2.0 * 0.1                         # (the scheduled cull setting at sigma 0.1: still every pair evaluated)
    pend = [PP.clears(c.frame) for c in PP.SCHEDULE]
    assert any(pend) and not all(pend)
    assert [c.frame for c in PP.SCHEDULE] == sorted({c.frame for c in PP.SCHEDULE}) and PP.SCHEDULE[-1].frame < PP.N_FRAMES - 1
    counts = [len(fr[0]) for fr in _schedule_frames()]
    assert min(counts[c.frame] for c in PP.SCHEDULE) >= 255 and counts.count(0) >= 3 and counts.count(1) >= 3, counts
    p0, v0, r0 = common.tables(5)
    p1, v1, r1 = PP.swap_tables()
    assert len(p1) != len(p0) and len(r1) != len(r0)
    assert 2.5 < p1.std() / p0.std() < 3.5 and np.abs(p1).max() > 2.5 * np.abs(p0).max()
    assert PP.CURSORS[0] < len(p1) and PP.CURSORS[1] < len(v1) and PP.CURSORS[2] < len(r1)


@functools.lru_cache(maxsize=None)
def _schedule_frames():
    from oracle import oracle_py as orc
    return _frames(orc, PP.N_FRAMES, seed=PP.FRAMES_SEED)


@pytest.mark.parametrize("change", [c for c in PP.SCHEDULE if c.on_oracle], ids=lambda c: c.name)
def test_scheduled_change_is_in_effect_on_the_oracle(orc, change):
    """the oracle fed the frames of the frame-path tests with the whole schedule, against a control oracle that was not given this one
    change: the frame behind the change differs by the bar.  The late newborn-number changes leave the frozen split where it was."""
    est = 1 if change.estimator_only else 2
    changes = PP.schedule(change.estimator_only)
    frames = _schedule_frames()
    got, split = PP.run_oracle(orc, CFG, frames, changes, change.frame, estimator=est)
    ctl, split_ctl = PP.run_oracle(orc, CFG, frames, changes, change.frame, skip=change.name, estimator=est)
    slots = 2 * CFG["ppv"]
    print(change, "particles %d / %d, changed %.3f" % (len(got[0]), len(ctl[0]), PP.changed_fraction(got, ctl, slots)))
    assert len(ctl[0]) > 1000
    assert PP.in_effect(change.kind, got, ctl, slots), (change, len(got[0]), len(ctl[0]))
    assert split == split_ctl == PP.FROZEN_SPLIT
