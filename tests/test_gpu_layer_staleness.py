"""GPU test of what makes the planning layers' snapshots stale (dspmap_layers_stale, dspmap_internal.h): one 16 x 16 x 6 map with the scene of
test_gpu_frontier.py, all snapshots built, then every call that changes something a snapshot was taken of, one after the other.  After each
call the device accessors say which snapshots are gone -- a stale one hands out NULL -- and that is compared with the table below, which
is the rule written out: the map carries the distance field, the forecast and the cast grid; the cast grid carries the arrival fields and
the frontiers; the arrival fields carry their timeline; the known-space layer and the position carry the frontiers.  What went stale is
rebuilt before the next call, and every rebuild is checked too: a build takes away nothing that does not depend on what it builds."""
import numpy as np
import pytest

from tests import frontier_ref as R
from tests.test_gpu_frontier import CUBE, WALL_DIST, _cloud, _scene

pytestmark = pytest.mark.gpu
DF, CG, RF, TL, FC, FR = range(6)
ACCESSORS = ["dspmap_distance_field_device", "dspmap_cast_grid_device", "dspmap_reach_fields_device", "dspmap_reach_timeline_device",
             "dspmap_forecast_device", "dspmap_frontier_grid_device"]
SRC = np.array([[0.0, 0.0, 0.0, 0]], np.float64)
#                             df cg rf tl fc fr     1: NULL after the call
MATRIX = [("update",                1, 1, 1, 1, 1, 1),
          ("seed_uniform",          1, 1, 1, 1, 1, 1),
          ("clear_state",           1, 1, 1, 1, 1, 1),
          ("build_cast_grid",       0, 0, 1, 1, 0, 1),   # (the grid itself is valid again when the call returns)
          ("mask_cast_grid",        0, 0, 1, 1, 0, 1),
          ("set_cast_grid",         0, 0, 1, 1, 0, 1),
          ("build_reach_fields",    0, 0, 0, 1, 0, 0),   # a plain build replaces the fields the timeline belonged to
          ("build_reach_timeline",  0, 0, 0, 0, 0, 0),
          ("build_distance_field",  0, 0, 0, 0, 0, 0),
          ("build_forecast",        0, 0, 0, 0, 0, 0),
          ("integrate_known",       0, 0, 0, 0, 0, 1),
          ("reset_known",           0, 0, 0, 0, 0, 1),
          ("set_known",             0, 0, 0, 0, 0, 1),
          ("set_current_position",  0, 0, 0, 0, 0, 1)]


def _stale(m):
    return tuple(int(not getattr(m.L, fn)(m.h)) for fn in ACCESSORS)


def _rebuild(m, words, age):
    """builds what is stale, in the order of the dependencies; after each build exactly the rest is still stale"""
    s = list(_stale(m))
    if s[CG]:
        assert s[RF] and s[TL] and s[FR]
    if s[RF]:
        assert s[TL]

    def built(*which):
        for k in which:
            s[k] = 0
        assert _stale(m) == tuple(s), (which, _stale(m), s)
    if s[DF]:
        m.build_distance_field(0.5, 8)
        built(DF)
    if s[CG]:
        m.build_cast_grid(0.5, 0)
        m.set_cast_grid(words)
        built(CG)
    if s[RF] or s[TL]:
        m.build_reach_timeline(SRC, max_steps=16)
        built(RF, TL)
    if s[FC]:
        m.build_forecast([0.1, 0.4])
        built(FC)
    if s[FR]:
        m.set_known(age)
        m.build_frontiers(max_age=2)
        built(FR)
    assert _stale(m) == (0,) * 6


def test_every_trigger_clears_what_depends_on_it_and_nothing_else(dsp):
    m, lay = _scene(dsp, CUBE)
    words, age = R.pack(lay), R.scene(CUBE)[1]
    pts = _cloud(WALL_DIST[CUBE])
    assert _stale(m) == (1, 0, 1, 1, 1, 1)               # the scene: a cast grid and a known-space layer, nothing else yet
    _rebuild(m, words, age)
    frame = [4]

    def update():
        assert m.update(pts, (0.0, 0.0, 0.0), frame[0] / 30.0, (1.0, 0.0, 0.0, 0.0)) == 1
        frame[0] += 1
    fire = {"update": update,
            "seed_uniform": lambda: m.seed_uniform(2),
            "clear_state": m.clear_state,
            "build_cast_grid": lambda: m.build_cast_grid(0.5, 0),
            "mask_cast_grid": lambda: m.mask_cast_grid(2),
            "set_cast_grid": lambda: m.set_cast_grid(words),
            "build_reach_fields": lambda: m.build_reach_fields(SRC, max_steps=16),
            "build_reach_timeline": lambda: m.build_reach_timeline(SRC, max_steps=16),
            "build_distance_field": lambda: m.build_distance_field(0.5, 8),
            "build_forecast": lambda: m.build_forecast([0.1, 0.4]),
            "integrate_known": m.integrate_known,
            "reset_known": m.reset_known,
            "set_known": lambda: m.set_known(age),
            "set_current_position": lambda: m.set_current_position(0.3, -0.15, 0.0)}
    assert list(fire) == [row[0] for row in MATRIX]
    for name, *want in MATRIX:
        fire[name]()
        assert _stale(m) == tuple(want), (name, _stale(m))
        _rebuild(m, words, age)
    m.close()
    # a second handle: plain fields, no timeline -- and the timeline of a later build goes with the next plain one
    m2, _ = _scene(dsp, CUBE)
    m2.build_reach_fields(SRC, max_steps=16)
    assert _stale(m2) == (1, 0, 0, 1, 1, 1)
    m2.build_reach_timeline(SRC, max_steps=16)
    assert _stale(m2) == (1, 0, 0, 0, 1, 1)
    m2.build_reach_fields(SRC, max_steps=16)
    assert _stale(m2) == (1, 0, 0, 1, 1, 1)
    m2.build_cast_grid(0.5, 0)
    assert _stale(m2) == (1, 0, 1, 1, 1, 1)
    m2.close()
