// dspmap_known_slots.h -- the slot arithmetic of the known-space layer's toroidal store, for every kernel that reads or writes a stamp
// (dspmap_known.hip, dspmap_view.hip, dspmap_frontier.hip): ONE copy, so that the three can never disagree about where a cell lives.
#pragma once
#include "dspmap_device.h"
#include "dspmap_kernels.h"

// the slot of map voxel i of an axis whose voxel 0 lives in slot b (0 <= b < n, 0 <= i < n)
__device__ __forceinline__ int kn_slot(int i, int b, int n) { const int s = i + b; return s >= n ? s - n : s; }
__device__ __forceinline__ size_t kn_cell(const MapDims& d, const KnownArgs& a, int x, int y, int z) {
    return ((size_t)kn_slot(z, a.bz, d.nz) * d.ny + kn_slot(y, a.by, d.ny)) * d.nx + kn_slot(x, a.bx, d.nx);
}
__device__ __forceinline__ int kn_age(unsigned stamp, unsigned now) { return stamp ? (int)(now - stamp) : -1; }
