"""numpy restatement of dspmap_build_frontiers (include/dspmap.h): the frontier between known-free and unknown space as a predicate over
one bool layer of the cast grid occ [nz, ny, nx] and the ages of the known-space layer age [nz, ny, nx] (what DSPMap.known_age() returns).
Everything is integer work: the device has to give the same integers, bit for bit."""
import numpy as np

from tests import cast_ref as CR

BLOCK_DTYPE = np.dtype([("block", "i4"), ("count", "i4"), ("sum_x", "i4"), ("sum_y", "i4"), ("sum_z", "i4"), ("unknown_faces", "i4")])
pack = CR.pack


def frontier(occ, age, max_age, min_unknown):
    """(frontier bool, u int32, free bool), each [nz, ny, nx]"""
    occ = np.asarray(occ, bool)
    age = np.asarray(age, np.int64)
    assert occ.shape == age.shape and occ.ndim == 3
    known = (age >= 0) & (age <= max_age)
    unknown = ~known
    free = known & ~occ
    u = np.zeros(occ.shape, np.int32)
    for ax in range(3):                                  # the six face neighbours INSIDE the map: the outside does not exist
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        u[tuple(lo)] += unknown[tuple(hi)]               # the neighbour at +1
        u[tuple(hi)] += unknown[tuple(lo)]               # the neighbour at -1
    return free & (u >= min_unknown), u, free


def cells(fr):
    """ascending voxel indices (z * ny + y) * nx + x of the frontier cells, int32"""
    return np.flatnonzero(np.asarray(fr, bool).ravel()).astype(np.int32)


def blocks(fr, u, block):
    """BLOCK_DTYPE records of the non-empty blocks in ascending block index"""
    fr = np.asarray(fr, bool)
    nz, ny, nx = fr.shape
    nbx, nby = -(-nx // block), -(-ny // block)
    z, y, x = np.nonzero(fr)
    idx = ((z // block) * nby + y // block) * nbx + x // block
    ids, inv = np.unique(idx, return_inverse=True)
    out = np.zeros(ids.size, BLOCK_DTYPE)
    out["block"] = ids
    for name, val in (("count", np.ones(idx.size, np.int64)), ("sum_x", x), ("sum_y", y), ("sum_z", z), ("unknown_faces", u[z, y, x])):
        out[name] = np.bincount(inv, weights=val, minlength=ids.size).astype(np.int64) if idx.size else 0
    return out


def centers(blk, shape, res, min_count=1):
    """float32 [k, 3] centroids in the map frame: ((sum / count) + 0.5) * res - half"""
    blk = blk[blk["count"] >= min_count]
    res = float(np.float32(res))
    half = np.array(shape, np.float64) * res / 2.0
    mean = np.stack([blk["sum_x"], blk["sum_y"], blk["sum_z"]], 1) / np.maximum(blk["count"], 1)[:, None]
    return ((mean + 0.5) * res - half).astype(np.float32)


def scene(shape, seed=5):
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    split = 64 if nx > 64 else nx // 2
    known = x < split + (y & 1)                 # the known/unknown border alternates between x = 63|64 and 64|65: it crosses a word
    known &= rng.random(known.shape) >= 0.06    # unknown holes
    age = np.where(known, rng.integers(0, 4, known.shape), -1).astype(np.int32)   # max_age = 2 makes age 3 unknown too
    occ = rng.random(known.shape) < 0.1
    return occ, age
