"""Timing of the objects extension (dspmap_build_objects, dspmap_query_objects) against the route a user has without it: dspmap_get_results
(16 B per voxel) and dspmap_get_cast_grid copied to the host, then the labelling and the per-label reductions on the CPU --
scipy.ndimage.label where scipy imports, else the numpy restatement of the tests (tests/objects_ref.components) --, each followed by the
restatement's reductions (tests/objects_ref.objects).  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24 particles / voxel) and
132 x 132 x 60 (9 particles / voxel), each after 20 frames of the synthetic depth stream (scene.py) and a cast grid built from the last one
with threshold 0.2, inflated by 0 and by 2 voxels.

Arms, interleaved call by call: dspmap_build_objects with connectivity 6 and 26 (two memsets and eight launches each; min_cells 4,
max_objects 4096) and dspmap_query_objects_device on 131 072 samples.  Device times are HIP events on the handle's stream (a torch stream)
around EVERY one of `--reps` calls after `--warmup` untimed ones; the median is reported (and the minimum).  The host route is wall time,
the median of `--host-reps` runs, and the tool asserts that both routes give the same records, label grid and counts at both
connectivities.  Prints one JSON line per workload and inflation.  bench.py is not involved.

    python tools/objects_bench.py [--reps 200] [--warmup 3] [--host-reps 3] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

THRESHOLD, INFLATE = 0.2, (0, 2)
MIN_CELLS, MAX_OBJECTS, N_SAMPLES = 4, 4096, 131072


def unpack(words, nx):
    """uint64 [nz, ny, W] -> bool [nz, ny, nx]"""
    bits = (words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(words.shape[:-1] + (-1,))[..., :nx].astype(bool)


def host_labels(R, occ, conn):
    """per set cell the smallest voxel index of its component, -1 elsewhere: scipy's labelling renamed, or the restatement's own"""
    try:
        from scipy import ndimage
    except ImportError:
        return R.components(occ, conn), "numpy"
    lab, n = ndimage.label(occ, ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
    idx = np.arange(occ.size, dtype=np.int64).reshape(occ.shape)
    first = np.full(n + 1, occ.size, np.int64)
    np.minimum.at(first, lab.ravel(), idx.ravel())
    return np.where(occ, first[lab], -1), "scipy"


def run(D, scene, name, args):
    from tests import objects_ref as R
    w = WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames)
    half = np.array([w["nx"], w["ny"], w["nz"]], np.float64) * w["res"] / 2.0
    rng = np.random.default_rng(7)
    q = np.zeros((N_SAMPLES, 4), np.float32)
    q[:, :3] = rng.uniform(-half * 1.05, half * 1.05, (N_SAMPLES, 3))

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

    for inflate in INFLATE:
        out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"]),
               "state": "%d frames of scene.py, build_cast_grid(%g, %d)" % (args.frames, THRESHOLD, inflate),
               "min_cells_max_objects": [MIN_CELLS, MAX_OBJECTS]}
        with torch.cuda.stream(st):
            m.build_cast_grid(THRESHOLD, inflate)
            st.synchronize()
        # the route without the feature: results and grid over the bus, labelling and reductions on the CPU
        for conn in (6, 26):
            tc, tl, tr, host, how = [], [], [], None, None
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                with torch.cuda.stream(st):
                    res = m.results()
                    words = m.cast_grid(0)
                t1 = time.perf_counter()
                occ = unpack(words, w["nx"])
                lab, how = host_labels(R, occ, conn)
                t2 = time.perf_counter()
                host = R.objects(occ, res, conn, MIN_CELLS, MAX_OBJECTS, lab=lab)
                t3 = time.perf_counter()
                tc.append((t1 - t0) * 1e3)
                tl.append((t2 - t1) * 1e3)
                tr.append((t3 - t2) * 1e3)
            out["host_c%d_ms_copies_labelling_reductions" % conn] = [round(float(np.median(tc)), 2), round(float(np.median(tl)), 1), round(float(np.median(tr)), 1)]
            out["host_labelling"] = how
            out["host_copy_bytes"] = int(res.nbytes + words.nbytes)
            with torch.cuda.stream(st):
                m.build_objects(t=-1.0, connectivity=conn, min_cells=MIN_CELLS, max_objects=MAX_OBJECTS)
                rec, grid, counts = m.objects(), m.object_labels(), m.object_counts()
            assert counts == host[2], "the device and the host route disagree about the counts (connectivity %d): %s %s" % (conn, counts, host[2])
            assert rec.tobytes() == host[0].astype(D.capi.OBJECT_DTYPE).tobytes(), "... about the records (connectivity %d)" % conn
            assert np.array_equal(grid, host[1]), "... about the label grid (connectivity %d)" % conn
            out["c%d_objects_components_occupied" % conn] = list(counts)
            if len(rec):
                big = rec[np.argmax(rec["count"]):][:1]
                out["c%d_largest_cells_speed" % conn] = [int(big["count"][0]), round(float(np.linalg.norm(m.object_states(big)[3][0])), 3)]
        qd = torch.as_tensor(q, device="cuda")
        od = torch.empty(N_SAMPLES, dtype=torch.int32, device="cuda")

        def build(conn):
            return lambda: m.build_objects(t=-1.0, connectivity=conn, min_cells=MIN_CELLS, max_objects=MAX_OBJECTS)

        def query():
            m._chk(m.L.dspmap_query_objects_device(m.h, N_SAMPLES, qd.data_ptr(), 0, od.data_ptr()))
        torch.cuda.synchronize()
        keys = [("build_c6_us_median_min", build(6)), ("build_c26_us_median_min", build(26)), ("query_%d_us_median_min" % N_SAMPLES, query)]
        for (k, _), v in zip(keys, timed([fn for _, fn in keys], args.reps)):
            out[k] = v
        with torch.cuda.stream(st):
            assert np.array_equal(m.query_objects(q), od.cpu().numpy()) and np.array_equal(m.results(), res), "the timed calls changed something"
        out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d" % (args.reps, args.warmup, args.host_reps)
        out["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(out), flush=True)
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=3, frames=20, host_reps=3)
    harness.main(run, ap)


if __name__ == "__main__":
    main()
