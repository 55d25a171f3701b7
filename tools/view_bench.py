"""Timing of the viewpoint scores (dspmap_score_views_device) against the route a user has without them: dspmap_get_cast_grid and
dspmap_get_known -- the grid and the ages copied to the host -- and, per candidate, NP ray walks and a classification of every voxel on
the CPU (the numpy restatement of the tests, tests/view_ref.score: whole-array operations, no per-cell Python loop).  Workloads: config B
(66 x 66 x 40 @ 0.15 m, 24 particles / voxel) and 132 x 132 x 60 (9 particles / voxel), each after 20 frames of the synthetic depth
stream (scene.py) with dspmap_known_integrate after every frame, on an unmasked grid (threshold 0.2, inflated by one voxel).

Arms, interleaved call by call: 1 / 16 / 256 / 4096 candidate views (random positions inside the map, random yaw, t = -1) at max_range 3 m
and +inf, and -- at 16 views -- the handle's own chunking against one workgroup per view (DSPMAP_P_VIEW_CHUNKS = 1).  Device times are HIP
events on the handle's stream (a torch stream) around EVERY one of `--reps` calls after `--warmup` untimed ones; the median is reported
(and the minimum).  The host route is wall time on the FIRST 16 views of each range, the median of `--host-reps` runs; its time for more
views is that figure scaled, and the output says so.  The tool asserts that both routes give the same scores.  Prints one JSON line per
workload.  bench.py is not involved.

    python tools/view_bench.py [--reps 200] [--warmup 3] [--host-reps 1] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

COUNTS = (1, 16, 256, 4096)
RANGES = (3.0, float("inf"))
MAX_AGE = 5
N_HOST = 16


def candidates(w, n, max_range, seed):
    rng = np.random.default_rng(seed)
    half = np.array([w["nx"], w["ny"], w["nz"]]) * w["res"] * 0.5
    v = np.zeros((n, 9), np.float32)
    v[:, 0:3] = rng.uniform(-0.9, 0.9, (n, 3)) * half
    yaw = rng.uniform(-np.pi, np.pi, n)
    v[:, 3], v[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    v[:, 7], v[:, 8] = max_range, -1.0
    return v


def run(D, scene, name, args):
    from tests import reach_ref, view_ref
    w = WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames, after_frame=lambda m: m.integrate_known())
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"]),
           "state": "%d frames of scene.py, integrated one by one; unmasked grid" % args.frames, "pyramids": m.NP, "voxels": m.V}
    with torch.cuda.stream(st):
        m.build_cast_grid(0.2, 1)
        st.synchronize()
    margin = float(m.get_param(D.capi.P_OCCLUSION_MARGIN))
    views = {r: candidates(w, max(COUNTS), r, 7) for r in RANGES}
    dviews = {r: torch.from_numpy(v).cuda() for r, v in views.items()}
    torch.cuda.synchronize()

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

    # the route without the feature: grid and ages over the bus, every ray walked and every voxel classified on the CPU
    cache = {}

    def rays(quat):
        if quat not in cache:
            cache[quat] = m.view_rays(quat)
        return cache[quat]

    with torch.cuda.stream(st):
        for r in RANGES:
            for i in range(N_HOST):
                rays(tuple(float(c) for c in views[r][i, 3:7]))                       # (the attitudes' planes: not part of the timed route)
        host = {}
        for r in RANGES:
            tc, tg = [], []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                grid = m.cast_grid()
                ages = m.known_age()
                t1 = time.perf_counter()
                want = view_ref.score(m.cfg, reach_ref.unpack(grid, m.cfg.nx), ages, views[r][:N_HOST], MAX_AGE, rays, margin)
                t2 = time.perf_counter()
                tc.append((t1 - t0) * 1e3)
                tg.append((t2 - t1) * 1e3)
            got = m.score_views(dviews[r][:N_HOST], MAX_AGE)
            st.synchronize()
            got = got.cpu().numpy()
            for j, f in enumerate(("n_seen", "n_unknown", "n_returns", "status")):
                assert np.array_equal(got[:, j], want[f]), "the device and the host route disagree on %s" % f
            host[r] = (float(np.median(tc)), float(np.median(tg)), want)
    for r in RANGES:
        tag = "inf" if r == float("inf") else "%gm" % r
        copies, walk, want = host[r]
        out["host_ms_copies_and_%d_views_range_%s" % (N_HOST, tag)] = [round(copies, 2), round(walk, 1)]
        out["host_ms_scaled_to_256_views_range_%s" % tag] = round(copies + walk * 256 / N_HOST, 0)
        ok = want["status"] == 0
        out["first_%d_views_range_%s_ok_seen_unknown_returns" % (N_HOST, tag)] = [int(ok.sum()), int(want["n_seen"].sum()), int(want["n_unknown"].sum()),
                                                                                 int(want["n_returns"].sum())]
    arms, keys = [], []
    for r in RANGES:
        tag = "inf" if r == float("inf") else "%gm" % r
        for n in COUNTS:
            arms.append(lambda r=r, n=n: m.score_views(dviews[r][:n], MAX_AGE))
            keys.append("score_%d_views_range_%s_us_median_min" % (n, tag))
    for k, v in zip(keys, timed(arms, args.reps)):
        out[k] = v
    # the chosen chunking against one workgroup per view, at 16 views
    def forced(r, chunks):
        def fn():
            m.set_param(D.capi.P_VIEW_CHUNKS, chunks)
            m.score_views(dviews[r][:16], MAX_AGE)
        return fn
    arms = [forced(r, c) for r in RANGES for c in (0, 1)]
    keys = ["score_16_views_range_%s_%s_us_median_min" % ("inf" if r == float("inf") else "%gm" % r, c) for r in RANGES
            for c in ("chunked", "one_workgroup_per_view")]
    for k, v in zip(keys, timed(arms, args.reps)):
        out[k] = v
    m.set_param(D.capi.P_VIEW_CHUNKS, 0)
    out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d on %d views, scaled" % (args.reps, args.warmup, args.host_reps, N_HOST)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=3, frames=20, host_reps=1)
    harness.main(run, ap)


if __name__ == "__main__":
    main()
