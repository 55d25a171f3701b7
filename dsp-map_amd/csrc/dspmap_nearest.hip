// dspmap_nearest.hip -- nearest-obstacle fields of the current and the predicted occupancy: WHICH voxel is the closest occupied one, and
// the signed distance to it (dspmap_build_nearest_field, dspmap_query_nearest*; semantics next to them in include/dspmap.h).  The reference
// has no counterpart.
//
// The separable transform of dspmap_distance.hip with the argmin carried through its three passes.  The tie rule -- the minimiser with the
// smallest global voxel index: smallest uz, then uy, then ux -- composes over the passes when each pass picks, among its candidates of
// minimal total, the one with the smaller coordinate along its own axis: pass z then fixes the smallest uz of all minimisers, and what it
// carries for that plane is pass y's choice, the smallest uy among the plane's minimisers, with pass x's smallest ux of that row.
// Truncation commutes as in the distance field: a partial result above R^2 only leads to totals above R^2, so it is stored as "none".
//
//   pass 1  k_near_x     one wave per row (y, z, virtual layer): the occupancy word is balloted from the masses (df_row_word) or loaded from
//                        the cast grid; nearest set bit left and right by clz / ctz over the own word and its two neighbours; the signed
//                        offset ux - x of the nearer one (equal: the left) in 8 bits, NEAR_NONE8 where it is more than R cells away.
//   pass 2  k_near_axis<false>  along y: DF_TS + 2R rows x 64 lanes staged in LDS as one 32-bit key per cell, the partial D2 in bits 16..30 and
//                        the carried offsets below; scanned outwards from dy = 0, the minimum of (total, scanned coordinate) kept as ONE
//                        integer; the winner's carried offsets are read back from LDS.  Output: the key pass 3 stages, 32 bits per cell.
//   pass 3  k_near_axis<true>   the same along z, then near = own index + the three offsets (int32) and the distance (float).
// With DSPMAP_NEAREST_SIGNED the complement sets run as L further virtual layers of the same launches (pass 1 inverts the word, masked to
// x < nx): the final pass of a plain layer writes the free cells, that of a complement layer the occupied ones, negated -- every cell is
// written by exactly one thread.  Lanes run along x in every pass; nothing of the map is written.
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"

#define NR_TPB 256
#define NR_WAVES (NR_TPB / 64)
#define NR_TS 32            // output rows of the scanned axis per workgroup (passes 2 and 3)
#define NR_RMAX 64          // largest truncation radius (dspmap_build_nearest_field refuses more)
#define NEAR_NONE8 (-128)   // pass 1: no set bit within R cells of the row
#define NEAR_NONE_D2 0x7fffu   // a key's partial D2 for "none": above every R^2, and its sum with 64^2 stays inside 16 bits
#define NEAR_NONE_KEY (NEAR_NONE_D2 << 16)

__global__ void __launch_bounds__(NR_TPB) k_near_x(MapDims d, DevState s, NearArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * NR_WAVES + (threadIdx.x >> 6);   // y + ny * z
    const int vl = blockIdx.y;                                    // virtual layer: [0, L) plain, [L, 2L) the complements
    if (row >= d.ny * d.nz) return;   // (wave-uniform: the ballots below see whole waves)
    const int layer = vl >= a.L ? vl - a.L : vl;
    const bool comp = vl >= a.L;
    const int z = row / d.ny, y = row - z * d.ny;
    const int nw = (int)grid_row_words(d);
    const u64* grid_row = a.grid ? a.grid + ((size_t)layer * grid_layer_words(d) + (size_t)row * nw) : nullptr;
    signed char* out = a.x8 + ((size_t)vl * d.v_glob + (size_t)row * d.nx);
    // the word w of the row's target set: bits at x >= nx are 0 in either polarity
    auto word = [&](int w) -> u64 {
        u64 v = grid_row ? grid_row[w] : df_row_word(d, s, a.thr, a.fut_zero, layer, w * 64 + lane, y, z);
        const int left = d.nx - w * 64;
        const u64 valid = left >= 64 ? ~0ull : ((1ull << left) - 1);
        if (comp) v = ~v;
        return v & valid;
    };
    u64 prev = 0, cur = word(0);
    for (int w = 0; w < nw; ++w) {
        const u64 next = w + 1 < nw ? word(w + 1) : 0;
        // nearest set bit at or below the lane: in its own word, else the top one of the word before (anything further is > 64 cells away)
        const u64 ml = cur & (~0ull >> (63 - lane));
        const int dl = ml ? lane - (63 - __builtin_clzll(ml)) : (prev ? lane + 1 + __builtin_clzll(prev) : 1024);
        const u64 mr = cur >> lane;
        const int dr = mr ? __builtin_ctzll(mr) : (next ? 64 - lane + __builtin_ctzll(next) : 1024);
        const int x = w * 64 + lane;
        if (x < d.nx) out[x] = (signed char)(min(dl, dr) > a.R ? NEAR_NONE8 : (dl <= dr ? -dl : dr));   // equal: the left, the smaller ux
        prev = cur;
        cur = next;
    }
}

// FINAL = false: scan y (input x8, output key32); FINAL = true: scan z (input key32, output near and dist).
// grid: x = 64-lane chunks of a row * tiles of NR_TS rows of the scanned axis, y = the other axis, z = virtual layer
template <bool FINAL>
__global__ void __launch_bounds__(NR_TPB) k_near_axis(MapDims d, NearArgs a) {
    __shared__ unsigned keys[(NR_TS + 2 * NR_RMAX) * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_scan = FINAL ? d.nz : d.ny;
    const int nxc = (int)grid_row_words(d);
    const int xc = blockIdx.x % nxc, tile = blockIdx.x / nxc;
    const int oth = blockIdx.y, vl = blockIdx.z;
    const int x = xc * 64 + lane;
    const int s0 = tile * NR_TS;
    const size_t plane = (size_t)d.nx * d.ny;
    const size_t stride = FINAL ? plane : (size_t)d.nx;
    const size_t cell0 = (FINAL ? (size_t)oth * d.nx : (size_t)oth * plane) + x;   // index of (x, row 0 of the scanned axis) inside a layer
    const size_t base = (size_t)vl * d.v_glob + cell0;
    const int R = a.R, R2 = R * R;
    const int rows = NR_TS + 2 * R;
    for (int r = wave; r < rows; r += NR_WAVES) {
        const int si = s0 - R + r;
        unsigned v = NEAR_NONE_KEY;   // beyond the map / the row: never a target
        if (x < d.nx && (unsigned)si < (unsigned)n_scan) {
            if (FINAL) v = a.key32[base + (size_t)si * stride];
            else {
                const int o = a.x8[base + (size_t)si * stride];
                if (o != NEAR_NONE8) v = ((unsigned)(o * o) << 16) | (unsigned)(o & 0xff);
            }
        }
        keys[r * 64 + lane] = v;
    }
    __syncthreads();
    for (int j = wave; j < NR_TS; j += NR_WAVES) {
        const int si = s0 + j;
        if (si >= n_scan) break;   // (wave-uniform)
        const unsigned* col = keys + (j + R) * 64 + lane;
        // best = (total << 8) | (scanned coordinate + 64): the smaller total wins, among equal totals the smaller coordinate.  A start without
        // a target is (R^2 + 1, 255): it loses to every total <= R^2 and ends as "none".  (A lane beyond the row never asks for another step.)
        const unsigned t0 = col[0] >> 16;
        unsigned best = x < d.nx ? (t0 <= (unsigned)R2 ? (t0 << 8) | 64u : ((unsigned)(R2 + 1) << 8) | 255u) : 0u;
        for (int dd = 1; dd <= R; ++dd) {
            const unsigned dd2 = (unsigned)(dd * dd);
            // <=, not <: a candidate at -dd with an equal total has the smaller coordinate and must still win
            if (!__builtin_amdgcn_ballot_w64(dd2 <= (best >> 8))) break;
            const unsigned cm = (((col[-dd * 64] >> 16) + dd2) << 8) | (unsigned)(64 - dd);
            const unsigned cp = (((col[dd * 64] >> 16) + dd2) << 8) | (unsigned)(64 + dd);
            best = min(best, min(cm, cp));   // ("none" entries total > 0x7fff: they never win or tie)
        }
        if (x >= d.nx) continue;
        const unsigned total = best >> 8;
        const bool none = total > (unsigned)R2;
        const int bd = none ? 0 : (int)(best & 0xffu) - 64;
        const unsigned carried = col[bd * 64] & 0xffffu;
        if (!FINAL) {
            a.key32[base + (size_t)si * stride] = none ? NEAR_NONE_KEY : (total << 16) | ((unsigned)(bd & 0xff) << 8) | carried;
        } else {
            const bool comp = vl >= a.L;
            // unsigned: every cell.  Signed: the plain layer writes the free cells (D2 > 0 or none), the complement layer the occupied ones
            if (a.sgn && !none && total == 0) continue;
            const size_t cell = cell0 + (size_t)si * stride;
            const size_t o = (size_t)(comp ? vl - a.L : vl) * d.v_glob + cell;
            const int ox = (int)(signed char)(carried & 0xffu), oy = (int)(signed char)(carried >> 8);
            a.near[o] = none ? -1 : (int)cell + ox + oy * d.nx + bd * (int)plane;
            const float v = __fmul_rn(sqrtf((float)(none ? R2 : (int)total)), d.res);   // (IEEE sqrt: correctly rounded)
            a.dist[o] = comp ? -v : v;
        }
    }
}

// One thread per sample, as k_dist_query: the pair of the point's own voxel, the offset to the nearest voxel's centre and the velocity of
// the occupied voxel of the pair.
__global__ void __launch_bounds__(NR_TPB) k_near_query(MapDims d, DevState s, NearQueryArgs a, int n, const float4* __restrict__ q,
                                                        dspmap_nearest* __restrict__ out) {
    const unsigned i = blockIdx.x * NR_TPB + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 smp = q[i];
    dspmap_nearest r = {a.outside, -1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (!(smp.x != smp.x || smp.y != smp.y || smp.z != smp.z || smp.w != smp.w)) {
        float px = smp.x, py = smp.y, pz = smp.z;
        origin_apply(a.org, px, py, pz);
        int g;
        if (voxel_of(d, px, py, pz, g)) {
            const int layer = q_horizon(d, smp.w) + 1;
            const size_t o = (size_t)layer * d.v_glob + g;
            r.dist = a.dist[o];
            r.voxel = a.near[o];
            if (r.voxel >= 0) {
                const int plane = d.nx * d.ny;
                const int uz = r.voxel / plane, rest = r.voxel - uz * plane, uy = rest / d.nx, ux = rest - uy * d.nx;
                r.ox = __fsub_rn(__fadd_rn(__fmul_rn((float)ux, d.res), a.cx), px);   // dspmap_voxel_center's expression - p
                r.oy = __fsub_rn(__fadd_rn(__fmul_rn((float)uy, d.res), a.cy), py);
                r.oz = __fsub_rn(__fadd_rn(__fmul_rn((float)uz, d.res), a.cz), pz);
            }
            // the occupied voxel of the pair: the own cell if it is occupied (it targets itself, or its distance is negative), else the target
            const int w = (r.voxel == g || r.dist < 0.f) ? g : r.voxel;
            if (layer == 0 && w >= 0) {
                const float4 res = s.res4[lv_of_g(d, w)];   // (unsharded: every voxel is in the slab)
                r.vx = res.y; r.vy = res.z; r.vz = res.w;
            }
        }
    }
    out[i] = r;
}

void launch_nearest_field(const LaunchCtx& c, const NearArgs& a) {
    const MapDims& d = c.d;
    const int rows = d.ny * d.nz;
    const int nxc = (int)grid_row_words(d);
    const int VL = a.sgn ? 2 * a.L : a.L;
    hipLaunchKernelGGL(k_near_x, dim3((rows + NR_WAVES - 1) / NR_WAVES, VL), dim3(NR_TPB), 0, c.stream, d, c.s, a);
    hipLaunchKernelGGL((k_near_axis<false>), dim3(nxc * ((d.ny + NR_TS - 1) / NR_TS), d.nz, VL), dim3(NR_TPB), 0, c.stream, d, a);
    hipLaunchKernelGGL((k_near_axis<true>), dim3(nxc * ((d.nz + NR_TS - 1) / NR_TS), d.ny, VL), dim3(NR_TPB), 0, c.stream, d, a);
}

void launch_nearest_query(const LaunchCtx& c, const NearQueryArgs& a, int n, const float4* q, dspmap_nearest* out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_near_query, dim3((unsigned)(((long long)n + NR_TPB - 1) / NR_TPB)), dim3(NR_TPB), 0, c.stream, c.d, c.s, a, n, q, out);
}
