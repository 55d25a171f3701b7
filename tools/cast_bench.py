"""Timing of the segment casts (dspmap_build_cast_grid, dspmap_cast_segments_device) against the two routes a user has without them:
(c) dspmap_trajectory_risk at r = 0 over the same segments sampled every half voxel -- NOT equivalent, it can miss voxels a segment only
clips -- and (d) the host route: results() + getFutureStatus() copies and a walk of the grid on the CPU (the numpy restatement of the
tests on a subsample, scaled to the whole batch and labelled as such).  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24 particles /
voxel) and 132 x 132 x 60 (9 particles / voxel), each after 20 frames of the synthetic depth stream (scene.py); L = 7 layers.

131 072 segments of mean length ~3 m with both ends inside the map, static (ta < 0) and space-time (ta = 0, tb = |ab| / 1.5 m/s).
Device times are HIP events on the handle's stream (a torch stream) around EVERY one of `--reps` calls after `--warmup` untimed ones,
the arms interleaved call by call; the median is reported (and the minimum).  Prints one JSON line per workload.  bench.py is not
involved.

    python tools/cast_bench.py [--reps 200] [--warmup 20] [--host-sub 4096] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

THRESHOLD = 0.2
N_SEG = 131072
SPEED = 1.5      # m/s along a space-time segment


def segments(w, n, seed=0):
    """[n, 8] float32, both ends inside the map, lengths around 3 m (a random direction, 1 .. 5 m, redrawn until b is inside)"""
    rng = np.random.default_rng(seed)
    half = np.array([w["nx"], w["ny"], w["nz"]], np.float64) * w["res"] * 0.5
    a = rng.uniform(-0.98, 0.98, (n, 3)) * half
    b = np.empty_like(a)
    todo = np.arange(n)
    for _ in range(200):
        if not todo.size:
            break
        d = rng.standard_normal((todo.size, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        cand = a[todo] + d * rng.uniform(1.0, 5.0, (todo.size, 1))
        ok = (np.abs(cand) < 0.98 * half).all(1)
        b[todo[ok]] = cand[ok]
        todo = todo[~ok]
    b[todo] = a[todo]
    seg = np.zeros((n, 8), np.float32)
    seg[:, 0:3], seg[:, 4:7] = a, b
    length = np.linalg.norm(b - a, axis=1)
    return seg, length


def run(D, scene, name, args):
    from tests import cast_ref, distance_ref
    w = WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames)

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

    seg, length = segments(w, N_SEG)
    seg_static, seg_time = seg.copy(), seg.copy()
    seg_static[:, 3] = seg_static[:, 7] = -1.0
    seg_time[:, 7] = (length / SPEED).astype(np.float32)
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel, %d frames of scene.py" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"], args.frames),
           "layers": m.T + 1, "threshold": THRESHOLD, "segments": N_SEG, "mean_length_m": round(float(length.mean()), 2)}
    # (a) the build
    b0, b2 = timed([lambda: m.build_cast_grid(THRESHOLD, 0), lambda: m.build_cast_grid(THRESHOLD, 2)], args.reps)
    out["a_build_inflate0_us_median_min"], out["a_build_inflate2_us_median_min"] = b0, b2
    m.build_cast_grid(THRESHOLD, 0)
    grid = m.cast_grid()
    out["occupied_per_layer"] = [int(np.unpackbits(grid[l].view(np.uint8)).sum()) for l in range(m.T + 1)]
    # (b) the casts and (c) trajectory_risk at r = 0 on the same segments, one sample per half voxel
    ds, dt = torch.from_numpy(seg_static).cuda(), torch.from_numpy(seg_time).cuda()
    n_samp = int(np.ceil(length.max() / (0.5 * w["res"]))) + 1
    u = np.linspace(0.0, 1.0, n_samp, dtype=np.float32)[None, :, None]

    def samples(s):
        q = np.empty((N_SEG, n_samp, 4), np.float32)
        q[:, :, :3] = s[:, None, 0:3] + (s[:, None, 4:7] - s[:, None, 0:3]) * u
        q[:, :, 3] = np.where(s[:, None, 3] < 0, -1.0, s[:, None, 3] + (s[:, None, 7] - s[:, None, 3]) * u[:, :, 0])
        return torch.from_numpy(q).cuda()

    qs, qt = samples(seg_static), samples(seg_time)
    torch.cuda.synchronize()
    arms = [lambda: m.cast_segments(ds), lambda: m.cast_segments(dt),
            lambda: m.trajectory_risk(qs, radius=0.0, threshold=THRESHOLD), lambda: m.trajectory_risk(qt, radius=0.0, threshold=THRESHOLD)]
    r = timed(arms, args.reps)
    out["b_cast_static_us_median_min"], out["b_cast_spacetime_us_median_min"] = r[0], r[1]
    out["c_trajectory_risk_r0_static_us_median_min"], out["c_trajectory_risk_r0_spacetime_us_median_min"] = r[2], r[3]
    out["c_samples_per_segment"] = n_samp
    with torch.cuda.stream(st):
        hs, ht = m.cast_segments(ds), m.cast_segments(dt)
        rs = m.trajectory_risk(qs, radius=0.0, threshold=THRESHOLD)
        st.synchronize()
    out["hit_fraction_static_spacetime"] = [round(float((hs["status"] == 1).float().mean()), 4), round(float((ht["status"] == 1).float().mean()), 4)]
    missed = ((hs["status"] == 1) & (rs["first_over"] < 0)).sum().item()
    out["c_not_equivalent"] = "samples every half voxel miss voxels a segment only clips: %d of %d static hits are not seen by (c)" % (
        missed, int((hs["status"] == 1).sum().item()))
    # (d) the host route: the two whole-grid copies, then a walk on the CPU (the numpy restatement on a subsample, scaled)
    t0 = time.perf_counter()
    res = m.results()
    fut = m.getFutureStatus()
    t1 = time.perf_counter()
    lay = distance_ref.occupancy_layers(m.cfg, res, fut, THRESHOLD)
    sub = seg_time[:args.host_sub]
    t2 = time.perf_counter()
    cast_ref.cast(m.cfg, lay, sub)
    t3 = time.perf_counter()
    out["d_host_copies_results_future_ms"] = round((t1 - t0) * 1e3, 3)
    out["d_host_walk_ms_scaled"] = round((t3 - t2) * 1e3 * N_SEG / len(sub), 1)
    out["d_host_walk"] = "numpy restatement (tests/cast_ref.py) on %d segments, scaled to %d" % (len(sub), N_SEG)
    out["timed_calls"] = "%d after %d untimed, arms interleaved" % (args.reps, args.warmup)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=20, frames=20)
    ap.add_argument("--host-sub", type=int, default=4096)
    harness.main(run, ap)


if __name__ == "__main__":
    main()
