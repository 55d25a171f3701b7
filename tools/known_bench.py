"""Timing of the known-space layer (dspmap_known_integrate, dspmap_mask_cast_grid, dspmap_query_known_device) against the route a user has
without it: dspmap_get_observations plus dspmap_get_view -- the frame's observations, rotated planes and farthest returns copied to the
host -- and the classification of every cell on the CPU (the numpy restatement of the tests, tests/known_ref.classify: whole-array
operations, no per-cell Python loop).  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24 particles / voxel) and 132 x 132 x 60 (9 particles /
voxel), each after 20 frames of the synthetic depth stream (scene.py).

Arms, interleaved call by call: (m) dspmap_known_reset, which is one hipMemsetAsync of the stamp buffer -- the yardstick for a kernel that
writes at most 4 B per cell; (a) dspmap_known_integrate; (b) dspmap_mask_cast_grid on a grid built once; (c) 131 072 samples through
dspmap_query_known_device.  Device times are HIP events on the handle's stream (a torch stream) around EVERY one of `--reps` calls after
`--warmup` untimed ones; the median is reported (and the minimum).  The host route is wall time, the median of `--host-reps` runs, and
the tool asserts that both routes stamp the same cells.  Prints one JSON line per workload.  bench.py is not involved.

    python tools/known_bench.py [--reps 200] [--warmup 3] [--host-reps 3] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

N_QUERY = 131072


def run(D, scene, name, args):
    from tests import known_ref
    w = WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames)
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"]),
           "state": "%d frames of scene.py" % args.frames, "stamp_bytes": 4 * m.V}
    cur = np.array(m.scene_frames[-1][1], np.float32)
    counter = int(m.get_param(D.capi.P_UPDATE_COUNTER))
    margin = float(m.get_param(D.capi.P_OCCLUSION_MARGIN))

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

    # the route without the feature: the frame's observations and view over the bus, every cell classified on the CPU
    tc, tg = [], []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        m.observations()
        ph, pv, ml = m.view()
        t1 = time.perf_counter()
        seen = known_ref.classify(m.cfg, cur, ph, pv, ml, margin)[0]
        t2 = time.perf_counter()
        tc.append((t1 - t0) * 1e3)
        tg.append((t2 - t1) * 1e3)
    with torch.cuda.stream(st):
        m.reset_known()
        m.integrate_known()
        ages = m.known_age()
        m.build_cast_grid(0.2, 1)
    assert np.array_equal(ages == 0, seen) and np.array_equal(ages == -1, ~seen), "the device and the host route disagree"
    out["cells_seen_of"] = [int(seen.sum()), int(seen.size)]
    out["host_ms_copies_classification"] = [round(float(np.median(tc)), 2), round(float(np.median(tg)), 1)]
    out["frame_counter"] = counter
    rng = np.random.default_rng(0)
    half = np.array([w["nx"], w["ny"], w["nz"]]) * w["res"] * 0.5
    q = np.concatenate([rng.uniform(-1.0, 1.0, (N_QUERY, 3)) * half, np.zeros((N_QUERY, 1))], 1).astype(np.float32)
    dq = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    arms = [m.reset_known, m.integrate_known, lambda: m.mask_cast_grid(0), lambda: m.query_known(dq)]
    keys = ["memset_stamps_us_median_min", "integrate_us_median_min", "mask_%d_layers_us_median_min" % (m.T + 1), "query_us_median_min_%d_samples" % N_QUERY]
    for k, v in zip(keys, timed(arms, args.reps)):
        out[k] = v
    out["integrate_GBs_of_stamp_bytes"] = round(4 * m.V / (out[keys[1]][0] * 1e-6) / 1e9, 1)
    with torch.cuda.stream(st):
        again = m.known_age()
    assert np.array_equal(again, ages), "the timed calls changed the layer"
    out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d" % (args.reps, args.warmup, args.host_reps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=3, frames=20, host_reps=3)
    harness.main(run, ap)


if __name__ == "__main__":
    main()
