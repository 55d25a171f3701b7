"""Timing of the tracking extension (dspmap_track_update) against the route a user has without it: the label grid (4 B per voxel) and the
records copied to the host after every build (DSPMap.object_labels, DSPMap.objects), then the association in numpy (the restatement of the
tests, tests/track_ref.Tracker).  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24 particles / voxel) and 132 x 132 x 60 (9 particles /
voxel), each after 20 frames of the synthetic depth stream (scene.py), a cast grid built from the last one with threshold 0.2, inflated by
0 and by 2 voxels, and its objects at connectivity 26 with min_cells 4.

The stream's scene is STATIC: every timed update associates the build with itself, so every track matches in place.  Moving, splitting
and merging objects are covered by the tests, not by this tool.

Arms, interleaved call by call: dspmap_track_update as it is (one table insert per run of equal pairs) and with DSPMAP_TRACK_PER_CELL (one
per cell).  Device times are HIP events on the handle's stream (a torch stream) around EVERY one of `--reps` calls after `--warmup`
untimed ones; the median is reported (and the minimum).  The host route is wall time, the median of `--host-reps` runs, and the tool
asserts that both routes give the same tracks and counts.  Prints one JSON line per workload and inflation.  bench.py is not involved.

    python tools/track_bench.py [--reps 200] [--warmup 3] [--host-reps 3] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

THRESHOLD, INFLATE = 0.2, (0, 2)
MIN_CELLS, MAX_OBJECTS, DT, MAX_SHIFT = 4, 4096, 1.0 / 30.0, 8


def run(D, scene, name, args):
    from tests import track_ref as R
    w = WORKLOADS[name]
    shape = (w["nx"], w["ny"], w["nz"])
    m, st = harness.open_map(D, scene, name, args.frames)
    pos = m.scene_frames[-1][1]

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

    for inflate in INFLATE:
        out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"]),
               "state": "%d frames of scene.py (a static scene: every track matches in place), build_cast_grid(%g, %d), build_objects(26, %d, %d)"
                        % (args.frames, THRESHOLD, inflate, MIN_CELLS, MAX_OBJECTS)}
        with torch.cuda.stream(st):
            m.build_cast_grid(THRESHOLD, inflate)
            m.build_objects(t=-1.0, connectivity=26, min_cells=MIN_CELLS, max_objects=MAX_OBJECTS)
            m.reset_tracks()
            st.synchronize()
        # the route without the feature: label grid and records over the bus after every build, the association on the CPU
        T = R.Tracker(shape, w["res"])
        tc, ta, host = [], [], None
        for _ in range(max(args.host_reps, 2)):
            t0 = time.perf_counter()
            with torch.cuda.stream(st):
                grid, rec = m.object_labels(), m.objects()
            t1 = time.perf_counter()
            host = T.update(grid, rec.astype(R.OBJECT_DTYPE), pos, DT, 1, MAX_SHIFT)
            t2 = time.perf_counter()
            tc.append((t1 - t0) * 1e3)
            ta.append((t2 - t1) * 1e3)
        out["host_ms_copies_association"] = [round(float(np.median(tc)), 2), round(float(np.median(ta)), 1)]
        out["host_copy_bytes"] = int(grid.nbytes + rec.nbytes)
        with torch.cuda.stream(st):
            for per_cell in [False] * (max(args.host_reps, 2) - 1) + [True]:
                m.update_tracks(DT, 1, MAX_SHIFT, 0, per_cell)
            tr, counts = m.tracks(), m.track_counts()
        assert counts == host[1] and host[2] == 0, "the device and the host route disagree about the counts: %s %s" % (counts, host[1])
        assert tr.tobytes() == host[0].astype(D.capi.TRACK_DTYPE).tobytes(), "... about the tracks"
        out["tracks_matched_born_ended_pairs_next_id"] = list(counts)
        keys = [("update_us_median_min", lambda: m.update_tracks(DT, 1, MAX_SHIFT, 0, False)),
                ("update_per_cell_us_median_min", lambda: m.update_tracks(DT, 1, MAX_SHIFT, 0, True))]
        torch.cuda.synchronize()
        for (k, _), v in zip(keys, timed([fn for _, fn in keys], args.reps)):
            out[k] = v
        with torch.cuda.stream(st):
            again = m.tracks()
        assert np.array_equal(again["id"], tr["id"]) and (again["age"] > tr["age"]).all(), "the timed updates lost a track"
        out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d" % (args.reps, args.warmup, max(args.host_reps, 2))
        out["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(out), flush=True)
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=3, frames=20, host_reps=3)
    harness.main(run, ap)


if __name__ == "__main__":
    main()
