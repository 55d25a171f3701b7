// dspmap_view.hip -- scores of candidate viewpoints (dspmap_score_views*, dspmap_view_rays, dspmap_debug_view_cells; semantics next to
// them in include/dspmap.h): how many voxels a frame taken from a candidate pose would stamp in the known-space layer, and how many of
// them are unknown now.  The reference has no counterpart; the pieces are its own -- the rotated pyramid planes (:226-232), the pyramid of
// a point (:1329-1367), the occlusion rule of mapUpdate (:761) -- with one synthetic farthest return per pyramid: the cast of the
// pyramid's central ray through the cast grid (cast_walk, the code k_cast runs).
//
//   k_view_score   one workgroup per (view, chunk of the view's rows).
//                  Head: every thread decides the view's status from the 36 bytes of the view (wave-uniform, before any walk); a view that
//                  is not OK costs one store and ends there.
//                  Phase 1: the planes rotated into LDS (rotate_by_quat over planes_h0 / planes_v0, what k_reset does for a frame), then one
//                  lane per ray: rotate the pyramid's central direction, walk the bit grid, ml[b] -> LDS.  EVERY chunk repeats this phase:
//                  NP rays of at most nx + ny + nz steps through a grid that sits in L2 are a few microseconds, less than a second
//                  launch and a round trip of ml[n][NP] through memory would cost, and no kernel has to wait for another.
//                  Phase 2: the waves walk rows of 64 consecutive x (wave-uniform y, z) of the axis-aligned box of max_range around the view,
//                  clipped to the map and grown by a cell; pyramid_of opens with the four outer-plane tests, so a wave wholly outside the
//                  wedge leaves after four dot products.  Seen cells are counted with ballots; the age is read only by seen lanes.
//                  Tail: one LDS reduction, then one integer atomic per workgroup and non-zero counter into the zero-initialised score.
//                  All counts are integers of exactly defined predicates: the result does not depend on the chunking.
//                  MASK instantiation (dspmap_score_view_sets / dspmap_select_views, dspmap_viewsel.hip): the same kernel, and lane 0 of
//                  every wave stores the ballot of `seen` -- which IS the word of the view's seen set in the cast grid's layout -- into
//                  the view's mask [nz][ny][W].  Only non-zero words are stored: the caller CLEARS all masks first (one hipMemsetAsync).
//                  Storing zeros in the loop instead would not do: the loop walks the box of max_range only, a view that is not OK never
//                  reaches it, and a wave that leaves at the wedge test would need a store of its own -- all words outside the box
//                  would want a second loop over the whole layer per view, with its index arithmetic, where the memset writes the same
//                  bytes at the full rate of the memory and knows nothing of views.
//   k_view_rays    the same rotation for one attitude, written out (dspmap_view_rays).
// Nothing of the map, the grid or the layer is written.
#include "dspmap_cast_walk.h"
#include "dspmap_internal.h"
#include "dspmap_known_slots.h"   // kn_cell, kn_age

#define VW_TPB 256
#define VW_WAVES (VW_TPB / 64)

// the age of map voxel (x, y, z)
__device__ __forceinline__ int vw_age(const MapDims& d, const KnownArgs& a, int x, int y, int z) {
    return kn_age(a.stamp[kn_cell(d, a, x, y, z)], a.now);
}

// the planes of attitude q into ph [(np_h + 1) * 3], pv [(np_v + 1) * 3]: k_reset's expression on k_reset's tables
__device__ __forceinline__ void vw_rotate_planes(const MapDims& d, const DevState& s, const float q[4], float* ph, float* pv) {
    for (int i = threadIdx.x; i <= d.np_h; i += VW_TPB) {
        float o[3];
        rotate_by_quat(s.planes_h0[3 * i], s.planes_h0[3 * i + 1], s.planes_h0[3 * i + 2], q, o);
        ph[3 * i] = o[0]; ph[3 * i + 1] = o[1]; ph[3 * i + 2] = o[2];
    }
    for (int j = threadIdx.x; j <= d.np_v; j += VW_TPB) {
        float o[3];
        rotate_by_quat(s.planes_v0[3 * j], s.planes_v0[3 * j + 1], s.planes_v0[3 * j + 2], q, o);
        pv[3 * j] = o[0]; pv[3 * j + 1] = o[1]; pv[3 * j + 2] = o[2];
    }
}

// first / last index of an axis whose voxel centre can lie within R of p: [(p - R + half) / res - 1, (p + R + half) / res + 1] clipped to the
// map.  Centre i lies at -half + (i + 0.5) res, so the exact bounds are half a cell inside these; the cell of slack on either side is far more
// than the roundings of this expression and of the classified distance can move.  (p finite, R > 0 or +inf.)
__device__ __forceinline__ void vw_axis_box(float p, float R, float half, float res, int n, int& lo, int& hi) {
    const float a = floorf((p - R + half) / res) - 1.f, b = floorf((p + R + half) / res) + 1.f;
    lo = (int)fminf(fmaxf(a, 0.f), (float)n);          // (n: an empty range, the box lies beyond the map)
    hi = (int)fminf(fmaxf(b, -1.f), (float)(n - 1));
}

template <bool DEBUG, bool MASK = false>
__global__ void __launch_bounds__(VW_TPB) k_view_score(MapDims d, DevState s, ViewArgs a, int n, int chunks, const float* __restrict__ views,
                                                        int4* __restrict__ out, u64* __restrict__ dbg_words, float* __restrict__ dbg_ml) {
    __shared__ float s_ph[DSP_MAX_PLANES_H * 3];
    __shared__ float s_pv[DSP_MAX_PLANES_V * 3];
    __shared__ int s_cnt[3];
    extern __shared__ float s_ml[];   // [np]
    const int view = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    if (view >= n) return;
    const float* v = views + 9 * (size_t)view;
    float px = v[0], py = v[1], pz = v[2];
    const float q[4] = {v[3], v[4], v[5], v[6]};
    const float R = v[7], t = v[8];
    // ---- head: the status (wave-uniform; nothing is walked for a view that is not OK)
    int status = DSPMAP_VIEW_OK, layer = 0, ix = 0, iy = 0, iz = 0;
    const float n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3] + q[0] * q[0];   // rotate_by_quat's divisor
    if (!(grid_finite(px) && grid_finite(py) && grid_finite(pz) && grid_finite(q[0]) && grid_finite(q[1]) && grid_finite(q[2]) &&
          grid_finite(q[3])) || n2 == 0.f || t != t || !(R > 0.f)) {
        status = DSPMAP_VIEW_INVALID;
    } else {
        origin_apply(a.org, px, py, pz);
        bool inside = !grid_beyond(d, px, py, pz);
        if (inside) {
            ix = grid_axis_cell(px, d.half_x, d.res);   // cast step 2
            iy = grid_axis_cell(py, d.half_y, d.res);
            iz = grid_axis_cell(pz, d.half_z, d.res);
            inside = ix < d.nx && iy < d.ny && iz < d.nz;
        }
        if (!inside) {
            status = DSPMAP_VIEW_OUTSIDE;
        } else {
            layer = q_horizon(d, t) + 1;   // 0 for t < 0 or T == 0
            const size_t nw = (size_t)(d.nx + 63) >> 6;   // (the parent form of W in 64 bits, as cast_walk keeps it)
            const u64 word = a.bits[(((size_t)layer * d.nz + iz) * d.ny + iy) * nw + ((unsigned)ix >> 6)];
            if ((word >> (ix & 63)) & 1ull) status = DSPMAP_VIEW_BLOCKED;
        }
    }
    if (status != DSPMAP_VIEW_OK) {
        if (chunk == 0 && threadIdx.x == 0) out[view].w = status;   // (counts stay 0)
        if (DEBUG) for (int b = threadIdx.x; b < d.np; b += VW_TPB) dbg_ml[b] = -1.f;
        return;
    }
    // ---- phase 1: planes and farthest returns
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    vw_rotate_planes(d, s, q, s_ph, s_pv);
    const float ell = fminf(R, a.reach);
    const float tc = fminf(t, 3.402823466e+38f);   // ta = tb: dt = 0 also for t = +inf, and k(tc) = k(t)
    int hits = 0;
    for (int b = threadIdx.x; b < d.np; b += VW_TPB) {
        float dir[3];
        rotate_by_quat(a.dirs0[3 * b], a.dirs0[3 * b + 1], a.dirs0[3 * b + 2], q, dir);
        const float ex = __fadd_rn(px, __fmul_rn(dir[0], ell)), ey = __fadd_rn(py, __fmul_rn(dir[1], ell)), ez = __fadd_rn(pz, __fmul_rn(dir[2], ell));
        float ml = -1.f;
        if (grid_finite(ex) && grid_finite(ey) && grid_finite(ez)) {   // (cast step 1: a segment with a non-finite end is no cast)
            float sp;
            int voxel, lay, st;
            cast_walk(d, a.bits, px, py, pz, tc, ex, ey, ez, tc, sp, voxel, lay, st);
            if (st == DSPMAP_CAST_HIT) {
                const int zc = d.ny * d.nx;
                const int hz = voxel / zc, rest = voxel - hz * zc, hy = rest / d.nx, hx = rest - hy * d.nx;
                const float rx = __fsub_rn(__fadd_rn(__fmul_rn((float)hx, d.res), a.cx), px);
                const float ry = __fsub_rn(__fadd_rn(__fmul_rn((float)hy, d.res), a.cy), py);
                const float rz = __fsub_rn(__fadd_rn(__fmul_rn((float)hz, d.res), a.cz), pz);
                ml = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(rx, rx), __fmul_rn(ry, ry)), __fmul_rn(rz, rz)));
                ++hits;
            }
        }
        s_ml[b] = ml;
        if (DEBUG) dbg_ml[b] = ml;
    }
    __syncthreads();
    // ---- phase 2: the cells
    int x0, x1, y0, y1, z0, z1;
    vw_axis_box(px, R, d.half_x, d.res, d.nx, x0, x1);
    vw_axis_box(py, R, d.half_y, d.res, d.ny, y0, y1);
    vw_axis_box(pz, R, d.half_z, d.res, d.nz, z0, z1);
    int seen_n = 0, unk_n = 0;
    if (x0 <= x1 && y0 <= y1 && z0 <= z1) {
        const int l = lane_id();
        const int W = (d.nx + 63) >> 6;
        const int w0 = x0 >> 6, nwb = (x1 >> 6) - w0 + 1, nyb = y1 - y0 + 1;
        const int n_items = nwb * nyb * (z1 - z0 + 1);   // (<= words of a layer < 2^31)
        for (int item = chunk * VW_WAVES + ((int)threadIdx.x >> 6); item < n_items; item += chunks * VW_WAVES) {
            const int w = w0 + item % nwb, row = item / nwb, y = y0 + row % nyb, z = z0 + row / nyb;   // (wave-uniform)
            const int x = w * 64 + l;
            const bool in = x < d.nx;
            const float rx = __fsub_rn(__fadd_rn(__fmul_rn((float)x, d.res), a.cx), px);   // dspmap_voxel_center's centre, minus the view
            const float ry = __fsub_rn(__fadd_rn(__fmul_rn((float)y, d.res), a.cy), py);
            const float rz = __fsub_rn(__fadd_rn(__fmul_rn((float)z, d.res), a.cz), pz);
            const int b = in ? pyramid_of(d, s_ph, s_pv, rx, ry, rz) : -1;
            if (!__ballot(b >= 0)) continue;   // the whole wave lies outside the wedge
            bool seen = false, unknown = false;
            if (b >= 0) {
                const float dist = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(rx, rx), __fmul_rn(ry, ry)), __fmul_rn(rz, rz)));
                const float ml = s_ml[b];
                const bool occluded = ml > 0.f && dist > __fadd_rn(ml, a.kn.occl_margin);   // :761
                seen = !occluded && dist <= R;
                if (seen) {
                    const int age = vw_age(d, a.kn, x, y, z);
                    unknown = age < 0 || age > a.max_age;
                }
            }
            const u64 sb = __ballot(seen), ub = __ballot(unknown);
            seen_n += (int)__popcll(sb);   // (every lane carries the wave's count)
            unk_n += (int)__popcll(ub);
            if (DEBUG && l == 0 && sb) dbg_words[((size_t)z * d.ny + y) * W + w] = sb;
            if (MASK && l == 0 && sb) dbg_words[((size_t)view * d.nz * d.ny + (size_t)z * d.ny + y) * W + w] = sb;   // (dbg_words: the masks [n][nz][ny][W])
        }
    }
    // ---- tail: wave -> workgroup -> score
    hits = wave_sum_i(hits);
    if (lane_id() == 0) {
        if (seen_n) atomicAdd(&s_cnt[0], seen_n);
        if (unk_n) atomicAdd(&s_cnt[1], unk_n);
        if (hits && chunk == 0) atomicAdd(&s_cnt[2], hits);   // (every chunk walked the same rays: one of them reports)
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&((int*)(out + view))[threadIdx.x], s_cnt[threadIdx.x]);
}

// planes_h [(np_h + 1) * 3], planes_v [(np_v + 1) * 3], dirs [np * 3] of attitude q, consecutively in `out`
__global__ void __launch_bounds__(VW_TPB) k_view_rays(MapDims d, DevState s, ViewArgs a, float q0, float q1, float q2, float q3, float* __restrict__ out) {
    const float q[4] = {q0, q1, q2, q3};
    float* ph = out;
    float* pv = ph + 3 * (d.np_h + 1);
    float* dirs = pv + 3 * (d.np_v + 1);
    if (blockIdx.x == 0) vw_rotate_planes(d, s, q, ph, pv);
    for (int b = blockIdx.x * VW_TPB + threadIdx.x; b < d.np; b += gridDim.x * VW_TPB) {
        float dir[3];
        rotate_by_quat(a.dirs0[3 * b], a.dirs0[3 * b + 1], a.dirs0[3 * b + 2], q, dir);
        dirs[3 * b] = dir[0]; dirs[3 * b + 1] = dir[1]; dirs[3 * b + 2] = dir[2];
    }
}

// workgroups per view: enough of them to give every CU a few, no more than the map has row items for (a chunk of fewer than VW_WAVES
// items idles waves), and at most 64 -- every chunk repeats the rays
int view_chunks(const MapDims& d, int n, int n_cu, int forced) {
    const long long items = (long long)grid_layer_words(d);
    long long most = (items + VW_WAVES - 1) / VW_WAVES;
    if (most > 64) most = 64;
    if (most < 1) most = 1;
    long long c = forced > 0 ? forced : ((long long)(n_cu > 0 ? n_cu : 256) * 4 + n - 1) / (n > 0 ? n : 1);
    if (c > most) c = most;
    if (c < 1) c = 1;
    while (c > 1 && (long long)n * c > 0x7fffffffll) --c;
    return (int)c;
}

void launch_view_score(const MapDims& d, const DevState& s, hipStream_t stream, const ViewArgs& a, int n, int chunks, const dspmap_view* views,
                       dspmap_view_score* out, u64* dbg_words, float* dbg_ml) {
    if (n <= 0) return;
    const dim3 grid((unsigned)((long long)n * chunks));
    const size_t lds = sizeof(float) * (size_t)d.np;
    if (dbg_words)
        hipLaunchKernelGGL(k_view_score<true>, grid, dim3(VW_TPB), lds, stream, d, s, a, n, chunks, (const float*)views, (int4*)out, dbg_words, dbg_ml);
    else
        hipLaunchKernelGGL(k_view_score<false>, grid, dim3(VW_TPB), lds, stream, d, s, a, n, chunks, (const float*)views, (int4*)out, (u64*)nullptr,
                           (float*)nullptr);
}

void launch_view_masks(const MapDims& d, const DevState& s, hipStream_t stream, const ViewArgs& a, int n, int chunks, const dspmap_view* views,
                       dspmap_view_score* out, u64* masks) {
    if (n <= 0) return;
    hipLaunchKernelGGL((k_view_score<false, true>), dim3((unsigned)((long long)n * chunks)), dim3(VW_TPB), sizeof(float) * (size_t)d.np, stream, d, s, a, n,
                       chunks, (const float*)views, (int4*)out, masks, (float*)nullptr);
}

void launch_view_rays(const MapDims& d, const DevState& s, hipStream_t stream, const ViewArgs& a, const float q[4], float* out) {
    hipLaunchKernelGGL(k_view_rays, dim3((unsigned)((d.np + VW_TPB - 1) / VW_TPB)), dim3(VW_TPB), 0, stream, d, s, a, q[0], q[1], q[2], q[3], out);
}
