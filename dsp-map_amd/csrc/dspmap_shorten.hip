// dspmap_shorten.hip -- cell paths shortened to line-of-sight waypoints in the cast grid (dspmap_shorten_paths*; semantics next to them in
// include/dspmap.h).  The reference has no counterpart: a planner that wants the few straight pieces behind a wavefront's one-voxel
// staircase copies the paths and the grid out (getOccupancyMapWithFutureStatus :405-426) and string-pulls them in a host loop, one DDA
// per candidate shortcut.
//
// The work: the greedy rule is strictly sequential along a path (the next anchor is the farthest candidate the last one sees), so the
// parallelism inside a path is the candidates of ONE round, and the parallelism of a batch is its paths.
//
// Chosen: ONE WAVE PER PATH, lane l owns candidate k = p + 1 + l of the round's anchor p -- which is why a window holds at most 64 cells.
// A round: every lane reads its cell (consecutive ints: one or two lines), runs cast_walk (dspmap_cast_walk.h: the instructions of k_cast,
// so a segment this kernel calls FREE is FREE under dspmap_cast_segments bit for bit) from the shared anchor, the wave ballots "FREE",
// q is the highest set lane or the fallback p + 1, lane 0 writes the segment record (two 16-byte stores) and its end index, and p moves
// on.  p, q, the segment count and the path's length are wave-uniform (ballots and readfirstlane) and live in scalar registers; the loop
// over rounds branches on scalars, never per lane.  No LDS, no atomics.  A path of m cells takes at most min(max_seg, m - 1) rounds of
// at most nx + ny + nz cast steps; the casts of a round diverge in their trip counts (the far candidates walk longest), which is the
// cost that remains.  The grids are 0.3 MB to a few MB and sit in L2, and the candidates of a round walk away from ONE cell: their
// first words are the same lines.
//
// Rejected:
//  - one lane per path, as k_cast has one per segment: up to 64 casts per round one after the other in a lane, and the lanes of a wave
//    at different anchors of different paths -- every load diverges.
//  - a binary search for the farthest visible candidate: visibility along a path is not monotone (a cell behind a corner can be seen
//    again further on), so the rule would be another one; the ballot costs one round of parallel casts whatever the mask looks like.
//  - a workgroup per path with windows above 64: four waves would vote through LDS with two barriers per round for a window no planner
//    asked for; a caller who wants longer pieces shortens the output once more (its vertices are cells again).
#include "dspmap_cast_walk.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"

#define SHORTEN_TPB 256
#define SHORTEN_WAVES (SHORTEN_TPB / 64)

// vertex of cell c at position j of a path whose first cell is occupied at step v: {voxel centre, time} (include/dspmap.h, "vertex", "time")
__device__ __forceinline__ float4 sh_vertex(const MapDims& d, const ShortenArgs& a, int c, int v, int j) {
    const int plane = d.nx * d.ny;
    const int z = c / plane, r = c - z * plane, y = r / d.nx, x = r - y * d.nx;
    float t = -1.0f;
    if (a.timed) t = __fadd_rn(a.t_start, __fmul_rn((float)max(v - j, 0), a.step_seconds));   // the schedule expression of dspmap_build_reach_fields
    return make_float4(__fadd_rn(__fmul_rn((float)x, d.res), a.cx), __fadd_rn(__fmul_rn((float)y, d.res), a.cy),
                       __fadd_rn(__fmul_rn((float)z, d.res), a.cz), t);
}

__global__ void __launch_bounds__(SHORTEN_TPB) k_shorten(MapDims d, ShortenArgs a, int n, const int* __restrict__ steps, const int* __restrict__ cells,
                                                         int4* __restrict__ info, float4* __restrict__ seg, int* __restrict__ end) {
    const int lane = threadIdx.x & 63;
    const unsigned i = blockIdx.x * SHORTEN_WAVES + (threadIdx.x >> 6);   // the wave's path
    if (i >= (unsigned)n) return;                                         // (wave-uniform: the ballots below see whole waves)
    const int* path = cells + (size_t)i * a.max_len;
    const int v = grid_uniform(steps[i]);
    // n_cells: the leading entries in [0, V), found 64 at a time
    int m = 0;
    if (v >= 0) {
        for (int base = 0; base < a.max_len; base += 64) {
            const int j = base + lane;
            const bool ok = j < a.max_len && (unsigned)path[j] < (unsigned)d.v_glob;
            const u64 bad = ~__ballot(ok);
            if (bad) { m = base + __builtin_ctzll(bad); break; }
            m = base + 64;
        }
    }
    m = grid_uniform(m);
    float4* seg_i = seg + 2 * (size_t)i * a.max_seg;
    int* end_i = end + (size_t)i * a.max_seg;
    int p = 0, s = 0, n_blocked = 0, truncated = 0;
    while (p < m - 1) {
        if (s == a.max_seg) { truncated = 1; break; }
        const float4 A = sh_vertex(d, a, path[p], v, p);   // (every lane reads the same address: one request)
        const int k = p + 1 + lane;
        bool free_ = false;
        if (lane < a.window && k < m) {
            const float4 B = sh_vertex(d, a, path[k], v, k);
            float cs; int voxel, layer, status;
            cast_walk(d, a.bits, A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w, cs, voxel, layer, status);
            free_ = status == DSPMAP_CAST_FREE;
        }
        const u64 mask = __ballot(free_);
        int q = p + 1;
        if (mask) q += 63 - __builtin_clzll(mask);
        else ++n_blocked;
        q = grid_uniform(q);
        if (lane == 0) {
            seg_i[2 * (size_t)s] = A;
            seg_i[2 * (size_t)s + 1] = sh_vertex(d, a, path[q], v, q);
            end_i[s] = q;
        }
        p = q;
        ++s;
    }
    for (int u = s + lane; u < a.max_seg; u += 64) {   // every entry behind n_segments is written
        seg_i[2 * (size_t)u] = make_float4(0.f, 0.f, 0.f, 0.f);
        seg_i[2 * (size_t)u + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
        end_i[u] = -1;
    }
    if (lane == 0) info[i] = make_int4(m, s, n_blocked, truncated);
}

void launch_shorten(const LaunchCtx& c, const ShortenArgs& a, int n, const int* steps, const int* cells, dspmap_path_info* info, dspmap_segment* seg,
                    int* end) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_shorten, dim3((unsigned)(((long long)n + SHORTEN_WAVES - 1) / SHORTEN_WAVES)), dim3(SHORTEN_TPB), 0, c.stream, c.d, a, n,
                       steps, cells, (int4*)info, (float4*)seg, end);
}
