"""CPU tests of the dense-observation scenes of the pair kernels (tests/pair_scenes.py), oracle alone: every scene reaches what it is
named for, and the oracle's pass 1 agrees with a float64 restatement of it within the bound of its own sequential fp32 sum -- the
yardstick tests/test_gpu_pair_kernels.py holds the HIP kernels against."""
import numpy as np
import pytest

from tests import pair_scenes as S


def test_count_table_hits_every_switch_point_exactly():
    cnt = S.count_table("fan")
    assert cnt.shape == (28, 16) and cnt.sum() == 11697
    assert (cnt > S.OBS_CAP).sum() == 48
    for h, target in S.EXACT_AT.items():
        assert cnt[h - 1:h + 2, 7:10].sum() == target
    assert [S.wu_split(x) for x in (0, 1, 64, 65, 128, 129, 256, 257, 891)] == [1, 1, 1, 2, 2, 4, 4, 8, 8]
    assert sorted(S.EXACT_O) == sorted(S.EXACT_AT.values()) == sorted([t for t in S.WU_SPLIT_AT] + [t + 1 for t in S.WU_SPLIT_AT])
    assert np.minimum(S.count_table("fan5x5"), S.OBS_CAP)[-5:, :5].sum() > 8 * S.STAGE_ROUND


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_scene_reaches_what_it_is_named_for(orc, name):
    r = S.reference(name)
    n_fov = S.check_scene(r)
    ck, wu, chunk = S.expected_items(r)
    assert chunk == r.scene["chunk"]
    raw = S.counted(r, r.raw)
    print("%s: %d observations, n_fov %d, P max %d (capp %d), O max %d, raw sums median %.3g (min %.3g, max %.3g), lambda %.3g, items %d / %d"
          % (name, r.obs_count.sum(), n_fov, r.P.max(), r.capp, r.O.max(), np.median(raw), raw.min(), raw.max(), r.lam, ck, wu))


def test_lists_on_both_sides_of_one_item_in_every_class_of_observation_count(orc):
    S.check_classes([S.reference("short_lists"), S.reference("long_lists")])
    r = S.reference("long_lists")
    assert ((r.O <= 64) & (r.O > 0) & (r.P > 256)).sum() >= 1      # more than one item at one lane per particle


def test_the_frames_own_constant_dominates_ck(orc):
    """why the scenes switch lambda off: with the frame's own constant the pair sum is a small part of Ck"""
    r, rl = S.reference("short_lists"), S.reference("short_lists", own_lambda=True)
    assert rl.lam == pytest.approx(1e-4 * 20 * len(r.cloud), rel=1e-6) and rl.lam > 1.0
    assert np.array_equal(r.raw, rl.raw)
    assert np.median(S.counted(r, r.raw)) < 0.1 * rl.lam


@pytest.mark.parametrize("name", ["short_lists", "long_lists", "culled"])
def test_pass1_of_the_oracle_against_its_float64_restatement(orc, name):
    """|fp32 sequential sum - exact sum| <= n 2^-24 x sum for n positive terms (each of the n - 1 additions rounds by at most 2^-24 of a
    partial sum that is at most the total)"""
    r = S.reference(name)
    samples = S.sample_observations(r, 40)
    sums, terms = S.restate_pass1(r, samples)
    got = np.array([r.raw[b, j] for b, j in samples], np.float64)
    assert terms.max() > 300 and (sums > 0).all()
    rel = np.abs(got - sums) / sums
    print("%s: restatement vs oracle, max rel %.3g over %d observations of up to %d terms" % (name, rel.max(), len(samples), terms.max()))
    assert (rel <= terms * 2.0 ** -24).all(), (rel.max(), terms[np.argmax(rel)])
