"""numpy restatement of the joint gain of views (include/dspmap.h, dspmap_score_view_sets and dspmap_select_views), on top of what is
there: the seen set of a view is tests/view_ref.score(..., details=True)["seen"], unknown is tests/known_ref.unknown.  Dense bool grids
[nz, ny, nx] throughout: no words, no chunks, no launches -- a union is np.logical_or, a gain is a sum."""
import numpy as np

from tests import known_ref as K
from tests import view_ref as V

SET_SCORE_DTYPE = np.dtype([("n_seen", "i4"), ("n_unknown", "i4"), ("n_ok", "i4"), ("reserved", "i4")])
PICK_DTYPE = np.dtype([("view", "i4"), ("gain", "i4"), ("covered", "i4"), ("reserved", "i4")])


# ---- the scene the CPU guards and the GPU tests share (the layers and candidates of tests/test_gpu_view.py)
SCENE_MAX_AGE, SCENE_K = 2, 16


def scene_ages(shape, seed=2):
    """int32 [nz, ny, nx]: ages -1 .. 5, 40 % of the cells forced to -1"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    ages = rng.integers(-1, 6, (nz, ny, nx)).astype(np.int32)
    ages[rng.random((nz, ny, nx)) < 0.4] = -1
    return ages


def scene_views(cfg, shape):
    """[100, 9]: test_gpu_view._views(n_ok=60) -- 60 inside, 12 outside, 10 invalid, 8 blocked --, then the first 10 once more"""
    from tests import test_gpu_view as G
    v = G._views(cfg, shape, n_ok=60)
    return np.concatenate([v, v[:10]])


def scene_sets(views, set_size, n_sets):
    """[n_sets, set_size, 9]: member j of set s is view (s + 7 j) mod n -- attitudes, ranges and layers mix --; the last set is views
    60 .. 60 + set_size, none of which is OK, and the one before it starts with an OK, an OUTSIDE, an INVALID and a BLOCKED view"""
    n = len(views)
    idx = (np.arange(n_sets)[:, None] + 7 * np.arange(set_size)[None, :]) % n
    idx[-1] = 60 + np.arange(set_size)
    idx[-2, :4] = (1, 65, 75, 85)
    return views[idx], idx


def seen_sets(cfg, lay, ages, views, max_age, rays, occl_margin=0.3, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """(scores SCORE_DTYPE [n], S bool [n, nz, ny, nx], unknown bool [nz, ny, nx]): S_i of every view, all False for one that is not OK"""
    v = np.ascontiguousarray(views, np.float32).reshape(-1, 9)
    shape = (cfg.nz, cfg.ny, cfg.nx)
    scores, info = V.score(cfg, lay, ages, v, max_age, rays, occl_margin, world=world, cur_pos=cur_pos, details=True)
    S = np.zeros((len(v),) + shape, bool)
    for i, d in info.items():
        S[i] = d["seen"]
    return scores, S, K.unknown(np.asarray(ages).reshape(shape), max_age)


def sets_from(scores, S, unknown, n_sets, set_size):
    """SET_SCORE_DTYPE [n_sets] of views laid out [n_sets][set_size]"""
    out = np.zeros(n_sets, SET_SCORE_DTYPE)
    for s in range(n_sets):
        member = slice(s * set_size, (s + 1) * set_size)
        union = S[member].any(0) if set_size else np.zeros_like(unknown)
        out[s] = (int(union.sum()), int((union & unknown).sum()), int((scores["status"][member] == V.OK).sum()), 0)
    return out


def greedy_from(S, unknown, n_fixed, k, min_gain):
    """PICK_DTYPE [k]: the rounds exactly as defined -- C_0 the union of the fixed views' U_i, then per round the candidate with the
    largest |U_i \\ C|, the smallest index among equals, until the best gain is below min_gain"""
    U = S & unknown[None]
    C = U[:n_fixed].any(0) if n_fixed else np.zeros_like(unknown)
    out = np.zeros(k, PICK_DTYPE)
    stopped = False
    for r in range(k):
        best, gain = -1, 0
        if not stopped:
            for i in range(n_fixed, len(U)):
                g = int((U[i] & ~C).sum())
                if g > gain:                                      # strictly: the first index keeps a tie
                    best, gain = i, g
        if best >= 0 and gain >= min_gain:
            C = C | U[best]
            out[r] = (best, gain, int(C.sum()), 0)
        else:
            stopped = True
            out[r] = (-1, 0, int(C.sum()), 0)
    return out


def score_sets(cfg, lay, ages, views, max_age, rays, occl_margin=0.3, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """(SET_SCORE_DTYPE [n_sets], SCORE_DTYPE [n_sets, set_size]) of views [n_sets, set_size, 9]"""
    v = np.ascontiguousarray(views, np.float32)
    n_sets, set_size = v.shape[:2]
    scores, S, unknown = seen_sets(cfg, lay, ages, v, max_age, rays, occl_margin, world, cur_pos)
    return sets_from(scores, S, unknown, n_sets, set_size), scores.reshape(n_sets, set_size)


def select(cfg, lay, ages, views, max_age, rays, k, n_fixed=0, min_gain=1, occl_margin=0.3, world=False, cur_pos=(0.0, 0.0, 0.0)):
    """(PICK_DTYPE [k], SCORE_DTYPE [n]) of views [n, 9]"""
    scores, S, unknown = seen_sets(cfg, lay, ages, views, max_age, rays, occl_margin, world, cur_pos)
    return greedy_from(S, unknown, n_fixed, k, min_gain), scores
