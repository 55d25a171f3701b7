// dspmap_block_scan.h -- the workgroup scan of the ordered compactions (dspmap_frontier.hip, dspmap_objects.hip)
#pragma once
#include "dspmap_device.h"

// inclusive scan of one int per thread over a workgroup of WAVES waves; s_w: WAVES ints; total: the workgroup's sum, in every thread
template <int WAVES> __device__ __forceinline__ int block_incl_scan_i(int v, int* s_w, int& total) {
    const int inc = wave_incl_scan_i(v);
    const int wv = (int)threadIdx.x >> 6;
    __syncthreads();   // (s_w may still be read from an earlier scan)
    if (lane_id() == 63) s_w[wv] = inc;
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int j = 0; j < WAVES; ++j) {
        if (j < wv) off += s_w[j];
        total += s_w[j];
    }
    return inc + off;
}
