"""CPU tests of the joint gain of views (dspmap_score_view_sets*, dspmap_select_views*): the numpy restatement the GPU tests hold the
kernels to (tests/view_select_ref.py) has the properties the definition implies on a hand-made 16 x 16 x 6 grid; the scenes of the GPU
tests are not degenerate -- the greedy pick is mostly NOT the best stand-alone view, gains tie, sets overlap --; the entry points are
exported and bound, every argument error is DSPMAP_E_ARG with its text before any device is touched and in the documented order, the byte
cap fires, a slab handle is a state error, a valid call needs a grid and so a device, and the drop-in class offers the new members."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import view_ref as V
from tests import view_select_ref as R

OK, E_ARG, E_DEVICE, E_STATE = 1, -1, -2, -3
NAMES = ("dspmap_score_view_sets", "dspmap_score_view_sets_device", "dspmap_select_views", "dspmap_select_views_device")
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S2 = float(np.sqrt(0.5))
INF = float("inf")
RES = 0.15
WIDE, CUBE, NARROW, TINY = (66, 12, 8), (16, 16, 6), (65, 5, 4), (3, 3, 3)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _view(pos, quat=(1.0, 0.0, 0.0, 0.0), max_range=INF, t=-1.0):
    return np.array(tuple(pos) + tuple(quat) + (max_range, t), F)


def _cfg(dsp, shape):
    return dsp.make_config(nx=shape[0], ny=shape[1], nz=shape[2], res=RES, ppv=12, seed=7)


# ---- the restatement on a hand-made grid
def test_restatement_properties_on_a_small_grid(dsp):
    cfg = _cfg(dsp, CUBE)
    lay = np.zeros((cfg.prediction_times + 1, 6, 16, 16), bool)
    lay[:, :, :, 12] = True
    lay[:, 2:4, 6:10, 12] = False                                         # a window in the wall
    ages = np.full((6, 16, 16), -1, np.int32)
    ages[:, :, :5] = 0                                                    # the near third is known
    ages[:, :8, 5:9] = 3                                                  # ... and a block seen too long ago
    rays = V.host_rays(cfg)
    views = np.stack([_view((-0.5, 0.02, 0.01)), _view((-0.5, 0.02, 0.01), max_range=0.9), _view((-0.9, -0.6, 0.2)),
                      _view((-0.9, 0.6, -0.2), quat=(0.9914449, 0.0, 0.0, -0.1305262)), _view((0.2, 0.3, 0.1), quat=(S2, 0.0, 0.0, S2)),
                      _view((-0.5, 0.02, 0.01), max_range=0.0), _view((9.0, 0.0, 0.0)), _view((0.9, 0.0, 0.0), quat=(0.0, 0.0, 0.0, 1.0))])
    scores, S, unknown = R.seen_sets(cfg, lay, ages, views, 2, rays)
    assert scores["status"].tolist() == [V.OK] * 5 + [V.INVALID, V.OUTSIDE, V.OK]
    assert not S[5].any() and not S[6].any() and S[0].sum() == scores["n_seen"][0]
    picks = R.greedy_from(S, unknown, 0, 8, 1)
    real = picks[picks["view"] >= 0]
    assert 3 <= len(real) < 8 and (np.diff(real["gain"]) <= 0).all()    # gains do not increase
    assert len(set(real["view"].tolist())) == len(real) and 1 not in real["view"]   # view 1 sees a subset of view 0
    union_unknown = int((S.any(0) & unknown).sum())
    assert picks["covered"][-1] == union_unknown == real["gain"].sum()    # the greedy cover ends at the union
    assert (picks["view"][len(real):] == -1).all() and (picks["gain"][len(real):] == 0).all() and (picks["covered"][len(real):] == union_unknown).all()
    # a set of one view is that view's score; a view and its duplicate are the single view
    one = R.sets_from(scores, S, unknown, len(views), 1)
    assert np.array_equal(one["n_seen"], scores["n_seen"]) and np.array_equal(one["n_unknown"], scores["n_unknown"])
    assert one["n_ok"].tolist() == [1] * 5 + [0, 0, 1] and not one["reserved"].any()
    twice = np.stack([views, views], 1)                                   # [8, 2, 9]
    two, sc2 = R.score_sets(cfg, lay, ages, twice, 2, rays)
    assert np.array_equal(two["n_seen"], one["n_seen"]) and np.array_equal(two["n_unknown"], one["n_unknown"]) and (two["n_ok"] == 2 * one["n_ok"]).all()
    assert np.array_equal(sc2[:, 0], scores) and np.array_equal(sc2[:, 1], scores)
    # fixed views: what they cover is gone from the gains, and they are no candidates
    fixed = R.greedy_from(S, unknown, 1, 8, 1)
    assert 0 not in fixed["view"] and fixed["covered"][-1] == union_unknown
    assert fixed["gain"].sum() == union_unknown - scores["n_unknown"][0]
    # min_gain ends the rounds early; n == n_fixed has no candidate
    big = R.greedy_from(S, unknown, 0, 8, int(real["gain"][1]) + 1)
    assert big["view"].tolist() == [int(real["view"][0])] + [-1] * 7 and (big["covered"] == real["covered"][0]).all()
    none = R.greedy_from(S, unknown, len(views), 3, 1)
    assert none["view"].tolist() == [-1] * 3 and (none["covered"] == union_unknown).all()


# ---- the scenes of the GPU tests
def _scene(dsp, shape):
    from tests import test_gpu_view as G
    cfg = _cfg(dsp, shape)
    lay = G._layers(shape, cfg.prediction_times + 1)
    views = R.scene_views(cfg, shape)
    ages = R.scene_ages(shape)
    return cfg, lay, ages, views


@pytest.mark.parametrize("shape", [WIDE, CUBE, NARROW, TINY], ids=["66x12x8", "16x16x6", "65x5x4", "3x3x3"])
def test_scenes_of_the_gpu_tests_are_not_degenerate(dsp, shape):
    cfg, lay, ages, views = _scene(dsp, shape)
    scores, S, unknown = R.seen_sets(cfg, lay, ages, views, R.SCENE_MAX_AGE, V.host_rays(cfg))
    picks = R.greedy_from(S, unknown, 0, R.SCENE_K, 1)
    rounds = int((picks["view"] >= 0).sum())
    U = S & unknown[None]
    C = np.zeros_like(unknown)
    not_best = ties = 0
    picked = []
    for r in range(rounds):
        gains = (U & ~C[None]).sum((1, 2, 3))
        assert gains.max() == picks["gain"][r] and int(np.argmax(gains)) == picks["view"][r]
        ties += int((gains == gains.max()).sum() > 1)
        alone = scores["n_unknown"].copy()
        alone[np.array(picked, int)] = -1
        not_best += int(alone[picks["view"][r]] < alone.max())
        picked.append(int(picks["view"][r]))
        C |= U[picks["view"][r]]
    print(shape, "rounds", rounds, "pick is not the best stand-alone view", not_best, "ties", ties, "sum of stand-alone",
          int(scores["n_unknown"][picked].sum()), "covered", int(picks["covered"][-1]))
    assert not (set(picked) & set(range(90, 100)))                        # a duplicate never comes before its original, and after it gains 0
    if shape in (WIDE, CUBE):
        assert rounds >= 8 and not_best >= 3 and ties >= 1
        assert scores["n_unknown"][picked].sum() > 2 * picks["covered"][-1]       # the stand-alone scores, summed, overstate the gain
        fixed = R.greedy_from(S, unknown, 5, R.SCENE_K, 1)
        assert fixed["view"].tolist() != picks["view"].tolist() and (fixed["view"][fixed["view"] >= 0] >= 5).all()
        sets, idx = R.scene_sets(views, 4, 48)
        got = R.sets_from(scores[idx.ravel()], S[idx.ravel()], unknown, 48, 4)
        member = scores["n_unknown"][idx]
        partial = (member.max(1) < got["n_unknown"]) & (got["n_unknown"] < member.sum(1))
        print(shape, "sets whose union lies strictly between the best member and the sum", int(partial.sum()))
        assert partial.sum() >= 20 and got["n_ok"][-1] == 0 and got["n_seen"][-1] == 0
        assert (got["n_ok"] < 4).any() and (got["n_ok"] == 4).any()
    if shape == NARROW:
        assert 1 <= rounds < R.SCENE_K and picks["view"][rounds] == -1     # ends by min_gain before k


# ---- the library without a device
def test_view_select_symbols_exported_and_bound(dsp):
    lib = dsp.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dsp.capi.LIB_PATH]).decode()
    hdr = open(os.path.join(ROOT, "include", "dspmap.h")).read()
    for n in NAMES:
        assert " T %s\n" % n in out, n
        assert n in dsp.capi.SIGNATURES and getattr(lib, n) is not None
        assert "int %s(dspmap_t* m" % n in hdr, n
    for meth in ("score_view_sets", "select_views"):
        assert callable(getattr(dsp.DSPMap, meth))
    assert "#define DSPMAP_VIEW_MASK_MAX_BYTES (1ull << 30)" in hdr and "#define DSPMAP_VIEW_MAX_PICKS 64" in hdr
    assert dsp.capi.VIEW_MASK_MAX_BYTES == 1 << 30 and dsp.capi.VIEW_MAX_PICKS == 64
    assert dsp.capi.VIEW_SET_SCORE_DTYPE == R.SET_SCORE_DTYPE and dsp.capi.VIEW_PICK_DTYPE == R.PICK_DTYPE
    assert "typedef struct dspmap_view_set_score { int n_seen, n_unknown, n_ok, reserved; } dspmap_view_set_score;" in hdr
    assert "typedef struct dspmap_view_pick { int view, gain, covered, reserved; } dspmap_view_pick;" in hdr
    assert '"dspmap_viewsel.hip"' in open(os.path.join(ROOT, "dsp-map_amd", "build_ext.py")).read()
    blob = open(dsp.capi.LIB_PATH, "rb").read()
    for k in (b"k_vs_unknown", b"k_vs_sets", b"k_vs_gain", b"k_vs_pick", b"k_vs_cover"):
        assert k in blob, k


def test_view_select_argument_errors_without_a_device(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    h = m.h
    err = lambda: L.dspmap_last_error(h).decode()   # noqa: E731
    views, sets, picks, scores = np.zeros((8, 9), F), np.zeros(4, R.SET_SCORE_DTYPE), np.zeros(64, R.PICK_DTYPE), np.zeros(8, V.SCORE_DTYPE)
    for fn in (L.dspmap_score_view_sets, L.dspmap_score_view_sets_device):
        assert fn(None, 2, 4, _p(views), 0, 0, _p(sets), None) == E_ARG
        # (arguments, text); every later line also breaks an argument that is checked AFTER the one its text names
        for args, text in (
                ((-1, 4, _p(views), 0, 0, _p(sets), None), "dspmap_score_view_sets: negative set count -1"),
                ((-1, 0, None, -1, 2, None, None), "dspmap_score_view_sets: negative set count -1"),
                ((2, 4, None, 0, 0, _p(sets), None), "dspmap_score_view_sets: NULL view or output array"),
                ((2, 4, _p(views), 0, 0, None, None), "dspmap_score_view_sets: NULL view or output array"),
                ((2, 0, None, 0, 0, _p(sets), None), "dspmap_score_view_sets: NULL view or output array"),
                ((2, 0, _p(views), 0, 0, _p(sets), None), "dspmap_score_view_sets: 0 views per set"),
                ((2, -3, _p(views), -1, 0, _p(sets), None), "dspmap_score_view_sets: -3 views per set"),
                ((65536, 32768, _p(views), -1, 0, _p(sets), None), "dspmap_score_view_sets: 65536 x 32768 views exceed INT_MAX"),
                ((2, 4, _p(views), -1, 0, _p(sets), None), "dspmap_score_view_sets: negative max_age -1"),
                ((2, 4, _p(views), -5, 2, _p(sets), None), "dspmap_score_view_sets: negative max_age -5"),
                ((2, 4, _p(views), 0, 2, _p(sets), None), "dspmap_score_view_sets: unknown flags 0x2"),
                ((2, 4, _p(views), 0, 3, _p(sets), None), "dspmap_score_view_sets: unknown flags 0x3"),
                ((65536, 16384, _p(views), 0, 4, _p(sets), None), "dspmap_score_view_sets: unknown flags 0x4")):   # ... before the cap
            assert fn(h, *args) == E_ARG and err() == text, (args, err())
        for args in ((2, 4, _p(views), 3, 0, _p(sets), None), (2, 4, _p(views), 3, 1, _p(sets), _p(scores)), (0, 0, None, 0, 0, None, None),
                     (0, -1, None, 0, 0, None, None)):                    # valid arguments: the missing grid decides, also for no sets
            assert fn(h, *args) == E_STATE and "dspmap_build_cast_grid" in err() and err().startswith("dspmap_score_view_sets: ")
    for fn in (L.dspmap_select_views, L.dspmap_select_views_device):
        assert fn(None, 8, _p(views), 0, 0, 0, 4, 1, _p(picks), None) == E_ARG
        for args, text in (
                ((-1, _p(views), 0, 0, 0, 4, 1, _p(picks), None), "dspmap_select_views: negative view count -1"),
                ((-2, None, 5, -1, 2, 65, 0, None, None), "dspmap_select_views: negative view count -2"),
                ((8, None, 0, 0, 0, 4, 1, _p(picks), None), "dspmap_select_views: NULL view or pick array"),
                ((8, _p(views), 9, 0, 0, 4, 1, None, None), "dspmap_select_views: NULL view or pick array"),
                ((8, _p(views), -1, 0, 0, 4, 1, _p(picks), None), "dspmap_select_views: n_fixed -1 outside [0, 8]"),
                ((8, _p(views), 9, 0, 0, 65, 1, _p(picks), None), "dspmap_select_views: n_fixed 9 outside [0, 8]"),
                ((0, None, 1, 0, 0, 0, 1, None, None), "dspmap_select_views: n_fixed 1 outside [0, 0]"),
                ((8, _p(views), 8, 0, 0, -1, 0, None, None), "dspmap_select_views: k -1 outside [0, 64]"),
                ((8, _p(views), 0, 0, 0, 65, 0, _p(picks), None), "dspmap_select_views: k 65 outside [0, 64]"),
                ((8, _p(views), 0, -1, 0, 64, 0, _p(picks), None), "dspmap_select_views: min_gain 0 below 1"),
                ((8, _p(views), 0, -1, 0, 4, -7, _p(picks), None), "dspmap_select_views: min_gain -7 below 1"),
                ((8, _p(views), 0, -1, 2, 4, 1, _p(picks), None), "dspmap_select_views: negative max_age -1"),
                ((8, _p(views), 0, 0, 2, 4, 1, _p(picks), None), "dspmap_select_views: unknown flags 0x2"),
                ((8, _p(views), 0, 0, -1, 0, 1, None, None), "dspmap_select_views: unknown flags 0xffffffff")):
            assert fn(h, *args) == E_ARG and err() == text, (args, err())
        for args in ((8, _p(views), 0, 3, 0, 4, 1, _p(picks), None), (8, _p(views), 8, 3, 1, 64, 1000, _p(picks), _p(scores)),
                     (8, _p(views), 3, 0, 0, 0, 1, None, None), (0, None, 0, 0, 0, 0, 1, None, None), (0, None, 0, 0, 0, 3, 1, _p(picks), None)):
            assert fn(h, *args) == E_STATE and "dspmap_build_cast_grid" in err() and err().startswith("dspmap_select_views: ")
    assert not sets.view(np.int32).any() and not picks.view(np.int32).any() and not scores.view(np.int32).any()   # nothing was written
    for bad in (np.zeros((3, 8), F), np.zeros((2, 3, 8), F), np.zeros((2, 3, 9), F), np.zeros(9, F)):   # [n, 9] and nothing else
        with pytest.raises(ValueError):
            m.select_views(bad, 4, 0)
    for bad in (np.zeros((3, 9), F), np.zeros((2, 3, 8), F)):
        with pytest.raises(ValueError):
            m.score_view_sets(bad, 0)
    for call in (lambda: m.select_views(views, 4, -1), lambda: m.select_views(views, 65, 0), lambda: m.select_views(views, 4, 0, min_gain=0),
                 lambda: m.select_views(views, 4, 0), lambda: m.score_view_sets(views.reshape(2, 4, 9), 0, scores=True)):
        with pytest.raises(dsp.capi.DSPMapError):
            call()
    m.close()


def test_view_mask_byte_cap(dsp):
    """130 x 64 x 40: a mask is 40 * 64 * 3 words = 61440 bytes, so 17476 views lie under 2^30 bytes and 17477 do not; the cap is an
    argument check -- it fires without a grid --, under it the missing grid decides"""
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=130, ny=64, nz=40, res=0.15))
    err = lambda: L.dspmap_last_error(m.h).decode()   # noqa: E731
    mask = 40 * 64 * 3 * 8
    under = (1 << 30) // mask
    assert under == 17476
    views = np.zeros((under + 1 + 3, 9), F)
    sets, picks = np.zeros(under + 4, R.SET_SCORE_DTYPE), np.zeros(4, R.PICK_DTYPE)
    text = "the masks of %d views take %d bytes, more than DSPMAP_VIEW_MASK_MAX_BYTES = 1073741824"
    for fn in (L.dspmap_select_views, L.dspmap_select_views_device):
        assert fn(m.h, under + 1, _p(views), 0, 0, 0, 4, 1, _p(picks), None) == E_ARG
        assert err() == "dspmap_select_views: " + text % (under + 1, (under + 1) * mask)
        assert fn(m.h, under, _p(views), 0, 0, 0, 4, 1, _p(picks), None) == E_STATE and "dspmap_build_cast_grid" in err()
    for fn in (L.dspmap_score_view_sets, L.dspmap_score_view_sets_device):
        for ns, sz in ((under + 1, 1), (4370, 4), (1, under + 1)):
            assert fn(m.h, ns, sz, _p(views), 0, 0, _p(sets), None) == E_ARG, (ns, sz)
            assert err() == "dspmap_score_view_sets: " + text % (ns * sz, ns * sz * mask)
        assert fn(m.h, 4369, 4, _p(views), 0, 0, _p(sets), None) == E_STATE and "dspmap_build_cast_grid" in err()
    with pytest.raises(dsp.capi.DSPMapError, match="DSPMAP_VIEW_MASK_MAX_BYTES"):
        m.select_views(views, 4, 0)
    m.close()


def test_view_select_on_slab_is_state_error(dsp):
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=16, ny=16, nz=6, res=0.15, ppv=12, z_lo=0, z_hi=3))
    err = lambda: L.dspmap_last_error(m.h)   # noqa: E731
    views, sets, picks = np.zeros((4, 9), F), np.zeros(2, R.SET_SCORE_DTYPE), np.zeros(2, R.PICK_DTYPE)
    for fn in (L.dspmap_score_view_sets, L.dspmap_score_view_sets_device):
        assert fn(m.h, 2, 2, _p(views), 0, 0, _p(sets), None) == E_STATE and b"slab" in err()
        assert fn(m.h, 2, 2, _p(views), -1, 0, _p(sets), None) == E_ARG       # the argument checks come first
    for fn in (L.dspmap_select_views, L.dspmap_select_views_device):
        assert fn(m.h, 4, _p(views), 0, 0, 0, 2, 1, _p(picks), None) == E_STATE and b"slab" in err()
        assert fn(m.h, 4, _p(views), 0, 0, 0, 2, 0, _p(picks), None) == E_ARG
    m.close()


def test_view_select_valid_calls_need_a_device(dsp):
    """no CPU fallback: a valid call needs a cast grid (the state check that comes first), and the grid it names is DSPMAP_E_DEVICE with
    "no HIP device" on a machine without one"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = dsp.load_library()
    m = dsp.DSPMap(dsp.make_config(nx=20, ny=20, nz=10, res=0.15))
    err = lambda: L.dspmap_last_error(m.h)   # noqa: E731
    views, sets, picks = np.zeros((4, 9), F), np.zeros(2, R.SET_SCORE_DTYPE), np.zeros(2, R.PICK_DTYPE)
    assert L.dspmap_score_view_sets(m.h, 2, 2, _p(views), 0, 0, _p(sets), None) == E_STATE and b"dspmap_build_cast_grid" in err()
    assert L.dspmap_select_views(m.h, 4, _p(views), 0, 0, 0, 2, 1, _p(picks), None) == E_STATE and b"dspmap_build_cast_grid" in err()
    assert L.dspmap_build_cast_grid(m.h, 0.1, 0, 0) == E_DEVICE and b"no HIP device" in err()
    with pytest.raises(dsp.capi.DSPMapError, match="no HIP device"):
        m.build_cast_grid(0.1, 0)
    m.close()


def test_dropin_class_offers_view_select_members(tmp_path):
    """include/dsp_dynamic.h: scoreViewSets and selectViews type-check and forward to the C ABI"""
    src = tmp_path / "viewsel.cpp"
    src.write_text('#include "dsp_dynamic.h"\nDSPMap my_map;\nint main() {\n'
                   "    dspmap_view v[4] = {{0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 3.f, -1.f}, {1.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, INFINITY, 0.5f}};\n"
                   "    dspmap_view_set_score ss[2];\n    dspmap_view_score s[4];\n    dspmap_view_pick p[DSPMAP_VIEW_MAX_PICKS];\n"
                   "    int a = my_map.scoreViewSets(2, 2, v, 30, ss) + my_map.scoreViewSets(2, 2, v, 0, ss, s, true);\n"
                   "    int b = my_map.selectViews(4, v, 2, 30, p) + my_map.selectViews(4, v, DSPMAP_VIEW_MAX_PICKS, 0, p, 1, 5, s, true);\n"
                   "    static_assert(sizeof(dspmap_view_set_score) == 16 && sizeof(dspmap_view_pick) == 16, \"layout\");\n"
                   "    static_assert(DSPMAP_VIEW_MASK_MAX_BYTES == 1073741824ull, \"cap\");\n"
                   "    return a + b + ss[0].n_seen + ss[0].n_unknown + ss[1].n_ok + ss[1].reserved + p[0].view + p[0].gain + p[1].covered + p[1].reserved;\n}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    hdr = open(os.path.join(ROOT, "include", "dsp_dynamic.h")).read()
    for call in ("dspmap_score_view_sets(h_", "dspmap_select_views(h_"):
        assert call in hdr, call
