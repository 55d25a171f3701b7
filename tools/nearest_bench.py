"""Timing of the nearest-obstacle fields (dspmap_build_nearest_field, dspmap_query_nearest_device) next to the distance fields they
extend, and against the route a user has without them: results() + getFutureStatus() host copies and a CPU distance transform WITH
indices of the T + 1 layers (scipy's distance_transform_edt(return_indices=True) where scipy is installed; without scipy that arm is
left out and said so).  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24 particles / voxel) and 132 x 132 x 60 (9 particles / voxel), each
after 20 frames of the synthetic depth stream (scene.py); L = 7 layers, threshold 0.2, R = 20 and R = 64.

Device times are HIP events on the handle's stream around EVERY one of `--reps` calls after `--warmup` untimed ones, the arms of a
radius interleaved call by call (the four flag combinations and dspmap_build_distance_field of the same R in the same run); medians
(and minima) are reported, and the ratio of each nearest build to the distance build.  The nearest build writes 8 bytes per cell instead
of 4 and carries 32-bit intermediates where the distance build carries 16; SIGNED runs the passes over twice the layers.  The host route
is timed on the wall clock, interleaved with event-timed builds as in tools/distance_bench.py, and its distances are asserted equal to
the device's (scipy's tie rule is another: indices are compared through the distance they give).  Prints one JSON line per workload.
bench.py is not involved.

    python tools/nearest_bench.py [--reps 200] [--warmup 3] [--host-reps 5] [--builds-only] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

THRESHOLD = 0.2
ARMS = [("nearest", False, False), ("nearest_signed", True, False), ("nearest_grid", False, True), ("nearest_signed_grid", True, True)]


def run(D, scene, name, args):
    w = WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames, spare=args.host_reps)
    T = m.T
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel, %d frames of scene.py" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"], args.frames),
           "layers": T + 1, "threshold": THRESHOLD}
    with torch.cuda.stream(st):
        m.build_cast_grid(THRESHOLD, 0)
    for R in (20, 64):
        fns = [lambda: m.build_distance_field(THRESHOLD, R)]
        fns += [lambda s=s, g=g: m.build_nearest_field(THRESHOLD, R, signed=s, from_cast_grid=g) for _, s, g in ARMS]
        t = harness.timed(st, fns, args.reps, args.warmup)
        out["build_R%d_us_median_min" % R] = dict(zip(["distance"] + [a[0] for a in ARMS], t))
        out["build_R%d_ratio_to_distance" % R] = {a[0]: round(t[i + 1][0] / t[0][0], 2) for i, a in enumerate(ARMS)}
    with torch.cuda.stream(st):
        m.build_distance_field(THRESHOLD, 20)
        m.build_nearest_field(THRESHOLD, 20)
        assert np.array_equal(m.nearest_distance().view(np.uint32), m.distance_field().view(np.uint32))
        out["occupied_per_layer"] = [int(v) for v in (m.nearest_distance() == 0).reshape(T + 1, -1).sum(1)]
    if args.builds_only:
        print(json.dumps(out))
        m.close()
        return
    rng = np.random.default_rng(0)
    half = np.array([w["nx"], w["ny"], w["nz"]], np.float32) * np.float32(w["res"]) * np.float32(0.5)
    q = np.empty((131072, 4), np.float32)
    q[:, :3] = rng.uniform(-1, 1, (len(q), 3)) * half
    q[:, 3] = np.concatenate([[-1.0], [0.05, 0.2, 0.5, 1.0, 1.5, 2.0]])[rng.integers(0, 7, len(q))]
    qd = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    t = harness.timed(st, [lambda: m.query_distance(qd), lambda: m.query_distance(qd, grad=False), lambda: m.query_nearest(qd)], args.reps, args.warmup)
    out["query_131072_us_median_min"] = dict(zip(["distance_grad", "distance_nograd", "nearest"], t))
    # the route without the feature, interleaved with the build: frame, build (events), host copies + CPU transform with indices (wall clock)
    try:
        from scipy import ndimage
    except Exception:  # noqa: BLE001
        ndimage = None
    shape = (w["nz"], w["ny"], w["nx"])
    build_us, copy_ms, cpu_ms = [], [], []
    for i in range(args.host_reps):
        with torch.cuda.stream(st):
            pts, pos, quat, ts = m.scene_frames[args.frames + i]
            m.clearOccupancyMapPrediction()
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, ts, quat) == 1
            st.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            m.build_nearest_field(THRESHOLD, 64)
            e1.record(st)
            st.synchronize()
            near = m.nearest_field()
        build_us.append(e0.elapsed_time(e1) * 1000.0)
        t0 = time.perf_counter()
        res = m.results()
        fut = m.getFutureStatus()
        t1 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        if ndimage is None:
            continue
        layers = [res[:, 0] > THRESHOLD] + [fut[:, k] > THRESHOLD for k in range(T)]
        found = []
        for occ in layers:
            found.append(ndimage.distance_transform_edt(~np.ascontiguousarray(occ).reshape(shape), return_indices=True))
        t2 = time.perf_counter()
        cpu_ms.append((t2 - t1) * 1e3)
        cells = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"))
        for l, (occ, (dist, idx)) in enumerate(zip(layers, found)):      # equal distances wherever a target lies within R
            if not occ.any():
                assert (near[l] == -1).all()
                continue
            d2 = ((cells - idx) ** 2).sum(0)
            mine = ((cells - np.stack(np.unravel_index(np.maximum(near[l], 0), shape))) ** 2).sum(0)
            within = d2 <= 64 * 64
            assert ((near[l] >= 0) == within).all() and np.array_equal(mine[within], d2[within]), l
    out["interleaved_build_R64_us_median"] = round(float(np.median(build_us)), 2)
    out["host_copies_results_future_ms_median"] = round(float(np.median(copy_ms)), 3)
    if ndimage is None:
        out["cpu_transform"] = "scipy is not installed: the CPU arm was not run"
    else:
        out["cpu_transform_%d_layers_ms_median" % (T + 1)] = round(float(np.median(cpu_ms)), 2)
        out["cpu_transform"] = "scipy.ndimage.distance_transform_edt(return_indices=True) (untruncated); distances asserted equal"
    out["timed_calls"] = "%d after %d untimed, arms interleaved; host route %d rounds" % (args.reps, args.warmup, args.host_reps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=3, frames=20, host_reps=5)
    ap.add_argument("--builds-only", action="store_true")
    harness.main(run, ap)


if __name__ == "__main__":
    main()
