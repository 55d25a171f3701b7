"""GPU tests of the pair kernels (k_pyr_prepare's work items, k_ck_partial, k_weight) where observations are DENSE: the scenes of
tests/pair_scenes.py -- up to 891 observations in a 3x3 neighbourhood (2475 in a 5x5 one), every lane split and lane layout of the
kernels on both sides of its switch point, both chunk sizes, bins at the reference's cap -- against the CPU oracle through the stage API.

What the Ck bar means here: lambda (expected_new_born_objects, :292) is switched off on both sides after binning, so Ck = pair sum +
kappa and RTOL bears on what k_ck_partial computes (the coverage conditions assert median pair sum >= 5 kappa).  With the frame's own
lambda = 23 the same bar would let through about 1 % of the sum; one run keeps the constant so that path stays compared too.

Which path ran is read back, not assumed: the k_weight instantiation (DSPMap.weight_variant), the chunk size and both item counts
(DSPMap.pair_items) against the numbers that follow from the oracle's list lengths and observation counts.
"""
import numpy as np
import pytest

from tests import common
from tests import pair_scenes as S

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def hip_run(dsp, r, own_lambda=False, cull_sigmas=None):
    """the scene's stages on a fresh HIP handle, from the oracle's exported state"""
    sc = r.scene
    m = dsp.DSPMap(dsp.make_config(**sc["cfg"]))
    m.set_tables(*common.tables(1))
    m.setObservationStdDev(sc["sigma"])
    if cull_sigmas is not None:
        m.set_param(dsp.capi.P_PAIR_CULL_SIGMAS, cull_sigmas)
    m.clear_state()
    m.import_state(r.voxel0, r.rec0, r.slot0)
    m.bin_points(r.cloud)
    m.predict(0.0, 0.0, 0.0, 1 / 30.0)
    if not own_lambda:
        m._chk(m.L.dspmap_set_expected_newborn(m.h, 0.0))      # (after binning: the frame's reset clears the override)
    m.map_update()
    return m


def compare_with_oracle(m, r, own_lambda=False):
    obs, cnt, ml, lam = m.observations()
    assert np.array_equal(cnt, r.obs_count) and np.array_equal(ml, r.obs_maxlen)
    assert np.array_equal(m.pyramid_counts(), r.P)
    assert lam == (pytest.approx(r.lam, rel=1e-6) if own_lambda else 0.0)
    ck_o, ck_g = S.counted(r, r.ck).astype(np.float64), S.counted(r, obs[:, :, 3]).astype(np.float64)
    rel = np.abs(ck_g - ck_o) / ck_o
    vg, sg, rg = m.export_state()                                                 # (both exports are in (voxel, slot) order)
    assert np.array_equal(r.voxel2, vg) and np.array_equal(r.slot2, sg)           # slot-exact records
    assert np.array_equal(r.rec2[:, 1:7], rg[:, 1:7])
    wo, wg = r.rec2[:, 7].astype(np.float64), rg[:, 7].astype(np.float64)
    relw = np.abs(wg - wo) / np.maximum(np.abs(wo), 1e-12)
    assert np.array_equal(r.voxel1, r.voxel2) and np.array_equal(r.slot1, r.slot2)
    changed = r.rec2[:, 7] != r.rec1[:, 7]
    print("%s%s: Ck rel max %.3g median %.3g over %d observations; weights rel max %.3g median %.3g over %d changed"
          % (r.name, " (own lambda)" if own_lambda else "", rel.max(), np.median(rel), len(rel), relw.max(),
             np.median(relw[changed]), changed.sum()))
    assert changed.sum() > 5000
    assert rel.max() < RTOL, (rel.max(), int(np.argmax(rel)))
    assert relw.max() < RTOL, (relw.max(), int(np.argmax(relw)))
    norm_o = float(np.sum(1.0 / ck_o))                                            # newborn normaliser (:799-805)
    assert m.counters()["newborn_weight"] == pytest.approx(1e-4 * norm_o, rel=1e-5)


def check_paths(m, r):
    assert m.weight_variant() == r.scene["variant"]
    ck, wu, chunk = S.expected_items(r)
    assert chunk == r.scene["chunk"]
    assert m.pair_items() == (ck, wu, chunk)


@pytest.mark.parametrize("name", ["short_lists", "long_lists", "culled", "wide5x5"])
def test_pair_kernels_against_oracle_dense(dsp, orc, name):
    r = S.reference(name)
    S.check_scene(r)
    m = hip_run(dsp, r)
    check_paths(m, r)
    compare_with_oracle(m, r)
    m.close()


def test_scenes_cover_every_class_of_observation_count(orc):
    S.check_classes([S.reference("short_lists"), S.reference("long_lists")])


def test_pair_kernels_against_oracle_with_the_frames_own_lambda(dsp, orc):
    r = S.reference("short_lists", own_lambda=True)
    assert r.lam > 20
    m = hip_run(dsp, r, own_lambda=True)
    check_paths(m, r)
    compare_with_oracle(m, r, own_lambda=True)
    m.close()


@pytest.mark.parametrize("name", ["culled", "long_lists"])
def test_range_culling_of_pairs_changes_nothing_dense(dsp, orc, name):
    """the shape of test_range_culling_of_pairs_changes_nothing on dense neighbourhoods: a second handle evaluates every pair
    (DSPMAP_P_PAIR_CULL_SIGMAS = 1e6) from the same imported state.  On `culled` the two handles run DIFFERENT k_weight instantiations."""
    r = S.reference(name)
    a, b = hip_run(dsp, r), hip_run(dsp, r, cull_sigmas=1e6)
    assert a.weight_variant() == r.scene["variant"] and b.weight_variant() == "mask"
    assert a.pair_items() == b.pair_items() == S.expected_items(r)
    oa, ca, _, _ = a.observations(); ob, cb, _, _ = b.observations()
    assert np.array_equal(ca, cb) and ca.sum() > 10000
    assert np.array_equal(oa[:, :, 3], ob[:, :, 3])                               # Ck, bit for bit
    (va, sa, ra), (vb, sb, rb) = a.export_state(), b.export_state()
    assert np.array_equal(va, vb) and np.array_equal(sa, sb)
    wa, wb = ra[:, 7].astype(np.float64), rb[:, 7].astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(wa), np.abs(wb)).astype(np.float32)).astype(np.float64)
    print("%s: weights that differ between culled and all pairs: %.3g of %d" % (name, (wa != wb).mean(), len(wa)))
    assert (np.abs(wa - wb) <= ulp).all()
    assert (wa != wb).mean() < 1e-3
    a.close(); b.close()
