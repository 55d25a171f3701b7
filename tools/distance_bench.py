"""Timing of the distance fields (dspmap_build_distance_field, dspmap_query_distance_device) against the route a user has without
them: getFutureStatus + results() host copies and a CPU distance transform of the T + 1 layers (scipy's EDT where scipy is installed,
else the numpy restatement of the tests, labelled as such).  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24 particles / voxel) and
132 x 132 x 60 (9 particles / voxel), each after 20 frames of the synthetic depth stream (scene.py); L = 7 layers, R = 20 and R = 64.

Device times are HIP events on the handle's stream (a torch stream) around EVERY one of `--reps` calls after `--warmup` untimed ones;
the median is reported (and the minimum).  The host route is timed on the wall clock, interleaved with event-timed builds: a fresh frame,
one build, one host route, `--host-reps` times (the host route consumes the future status, so every round needs its own frame).
Also printed: the bytes each pass moves (to set against the per-kernel times of a `rocprofv3 --kernel-trace --stats` run of this
script with --builds-only).  Prints one JSON line per workload.  bench.py is not involved.

    python tools/distance_bench.py [--reps 200] [--warmup 20] [--host-reps 5] [--builds-only] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

THRESHOLD = 0.2


def cpu_transform():
    try:
        from scipy import ndimage
        return "scipy.ndimage.distance_transform_edt", lambda occ: ndimage.distance_transform_edt(~occ)
    except Exception:  # noqa: BLE001
        from tests import distance_ref
        return "numpy restatement (tests/distance_ref.py; scipy is not installed)", distance_ref.d2_separable


def pass_bytes(V, T, R, ts=32):
    """bytes each pass reads / writes (the halo rows of passes 2 and 3 counted as read again; caches will serve most of them)"""
    L = T + 1
    halo = (ts + 2 * R) / ts
    return {"k_dist_x": [V * 16 + T * V * 12, L * V], "k_dist_axis<false>": [int(L * V * halo), 2 * L * V],
            "k_dist_axis<true>": [int(2 * L * V * halo), 4 * L * V]}


def run(D, scene, name, args):
    w = WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames, spare=args.host_reps)

    def frame(f):
        """one of the frames behind the fill, for the host route"""
        pts, pos, quat, t = m.scene_frames[f]
        if f:
            m.clearOccupancyMapPrediction()
        assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1

    def timed(fn, reps):
        """device time (us) of each of reps calls: events on the handle's stream around every call -> (median, min)"""
        return harness.timed(st, [fn], reps, args.warmup)[0]

    V, T = m.V, m.T
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel, %d frames of scene.py" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"], args.frames),
           "layers": T + 1, "threshold": THRESHOLD}
    for R in (20, 64):
        out["build_R%d_us_median_min" % R] = timed(lambda: m.build_distance_field(THRESHOLD, R), args.reps)
        out["pass_bytes_read_written_R%d" % R] = pass_bytes(V, T, R)
    fld = m.distance_field()
    out["occupied_per_layer"] = [int((fld[l] == 0).sum()) for l in range(T + 1)]
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
    out["query_131072_grad_us_median_min"] = timed(lambda: m.query_distance(qd), args.reps)
    out["query_131072_nograd_us_median_min"] = timed(lambda: m.query_distance(qd, grad=False), args.reps)
    # the route without the feature, interleaved with the build: frame, build (events), host copies + CPU transform (wall clock)
    label, edt = cpu_transform()
    shape = (w["nz"], w["ny"], w["nx"])
    build_us, copy_ms, cpu_ms = [], [], []
    for i in range(args.host_reps):
        with torch.cuda.stream(st):
            frame(args.frames + i)
            st.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            m.build_distance_field(THRESHOLD, 20)
            e1.record(st)
            st.synchronize()
        build_us.append(e0.elapsed_time(e1) * 1000.0)
        t0 = time.perf_counter()
        res = m.results()
        fut = m.getFutureStatus()
        t1 = time.perf_counter()
        layers = [res[:, 0] > THRESHOLD] + [fut[:, k] > THRESHOLD for k in range(T)]
        for occ in layers:
            edt(np.ascontiguousarray(occ).reshape(shape))
        t2 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        cpu_ms.append((t2 - t1) * 1e3)
    out["interleaved_build_R20_us_median"] = round(float(np.median(build_us)), 2)
    out["host_copies_results_future_ms_median"] = round(float(np.median(copy_ms)), 3)
    out["cpu_transform_%d_layers_ms_median" % (T + 1)] = round(float(np.median(cpu_ms)), 2)
    out["cpu_transform"] = label + " (untruncated)"
    out["timed_calls"] = "%d after %d untimed; host route %d rounds" % (args.reps, args.warmup, args.host_reps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=20, frames=20, host_reps=5)
    ap.add_argument("--builds-only", action="store_true")
    harness.main(run, ap)


if __name__ == "__main__":
    main()
