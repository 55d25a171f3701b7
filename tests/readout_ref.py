"""numpy float32 restatement of the occupied-voxel readout (include/dspmap.h, dspmap_get_occupancy and
dspmap_get_occupancy_with_future; getOccupancyMap* :385-426 of the reference): the voxels whose mass exceeds the threshold, in
ascending voxel index, as the centres dspmap_voxel_center gives (getVoxelPositionFromIndex :1090-1107).

Independent of the kernels' structure (count, scan, emit): one comparison over the whole mass column, one index split, and the
centre as two elementwise float32 operations (one rounding each, no fused multiply-add)."""
import numpy as np

F = np.float32


def centres(cfg, index):
    """float32 [n, 3] centres of the GLOBAL voxel indices: (float)xi * res + (-half + res * 0.5f) per axis, half = (res * n) * 0.5"""
    g = np.asarray(index, np.int64).ravel()
    nx, ny, nz = int(cfg.nx), int(cfg.ny), int(cfg.nz)
    res = F(cfg.voxel_resolution)
    zc = ny * nx
    zi = g // zc
    rest = g - zi * zc
    yi = rest // nx
    xi = rest - yi * nx
    out = np.empty((len(g), 3), F)
    for a, (i, n) in enumerate(((xi, nx), (yi, ny), (zi, nz))):
        half = F(F(res * F(n)) * F(0.5))            # (res * n) * 0.5 (:528-530)
        corr = F(F(-half) + F(res * F(0.5)))        # -half + res / 2
        prod = (i.astype(F) * res).astype(F)        # fl((float)i * res)
        out[:, a] = (prod + corr).astype(F)         # fl(prod + corr)
    return out


def occupied_list(cfg, mass, thr, v_base=0):
    """(n, xyz [n, 3] float32) of the voxels i with mass[i] > thr, ascending; mass is the (slab's) mass column, index i is the
    voxel v_base + i of the whole map.  The comparison is made in float32; a NaN threshold selects nothing."""
    mass = np.ascontiguousarray(mass, F).ravel()
    with np.errstate(invalid="ignore"):
        idx = np.flatnonzero(mass > F(thr))
    return int(idx.size), centres(cfg, idx.astype(np.int64) + int(v_base))
