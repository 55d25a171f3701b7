// dspmap_distance.hip -- truncated Euclidean distance fields of the current and the predicted occupancy (dspmap_build_distance_field,
// dspmap_query_distance*; semantics next to them in include/dspmap.h).  The reference has no counterpart: a planner that needs clearance
// copies the whole grid out (getOccupancyMapWithFutureStatus :405-426) and runs a distance transform on the CPU, once per horizon.
//
// The squared Euclidean distance to the nearest occupied voxel separates by axis (min over x', y', z' of dx^2 + dy^2 + dz^2 =
// min over z' of (dz^2 + min over y' of (dy^2 + min over x' of dx^2))), and truncation commutes with it: a partial result above R^2 can
// only lead to totals above R^2, so every pass may clamp what it stores and look no further than R cells.  Everything up to the final
// square root is integer arithmetic on values <= 65^2: the field is defined bit for bit.
//
//   pass 1  k_dist_x     one wave per row (y, z, layer): the masses are read in place and in storage order (res4[lv].x / fut_status_at, as
//                        dspmap_query.hip reads them), compared with the threshold and balloted into 64-bit words; a lane's distance to
//                        the nearest set bit comes from clz / ctz over its own word and the two next to it (R + 1 <= 65 cells never
//                        reach further).  The three words are wave-uniform: they live in SGPRs, no LDS.  8 bits per cell.
//   pass 2  k_dist_axis<false>  along y: columns of 64 x-lanes staged in LDS as squares, DF_TS output rows + R halo rows either side;
//                        min over |dy| <= R of g^2 + dy^2, scanned outwards from dy = 0 and left as soon as dy^2 can no longer improve
//                        any lane of the wave (dense layers stop after a few steps).  16 bits per cell.
//   pass 3  k_dist_axis<true>   the same along z on pass 2's output, then the outside-occupied term, the clamp to R^2, sqrt, scale.
// Lanes run along x in every pass: every global access is a run of consecutive cells, no transposes.  All L layers go in one launch per
// pass (the layer is a grid dimension).  Nothing of the map is written.
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"

#define DF_TPB 256
#define DF_WAVES (DF_TPB / 64)
#define DF_TS 32      // output rows of the scanned axis per workgroup (passes 2 and 3)
#define DF_RMAX 64    // largest truncation radius (dspmap_build_distance_field refuses more)

// (df_row_word, the occupancy word of 64 cells of a row, lives in dspmap_device.h: dspmap_cast.hip packs its grid with it too)
__global__ void __launch_bounds__(DF_TPB) k_dist_x(MapDims d, DevState s, DistArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * DF_WAVES + (threadIdx.x >> 6);   // y + ny * z
    const int layer = blockIdx.y;
    if (row >= d.ny * d.nz) return;   // (wave-uniform: the ballots below see whole waves)
    const int z = row / d.ny, y = row - z * d.ny;
    const int nw = (int)grid_row_words(d);
    const int cap = a.R + 1;
    unsigned char* out = a.g8 + ((size_t)layer * d.v_glob + (size_t)row * d.nx);
    u64 prev = 0, cur = df_row_word(d, s, a.thr, a.fut_zero, layer, lane, y, z);
    for (int w = 0; w < nw; ++w) {
        const u64 next = w + 1 < nw ? df_row_word(d, s, a.thr, a.fut_zero, layer, (w + 1) * 64 + lane, y, z) : 0;
        // nearest set bit at or below the lane: in its own word, else the top one of the word before (anything further is > 64 cells away)
        const u64 ml = cur & (~0ull >> (63 - lane));
        const int dl = ml ? lane - (63 - __builtin_clzll(ml)) : (prev ? lane + 1 + __builtin_clzll(prev) : cap);
        const u64 mr = cur >> lane;
        const int dr = mr ? __builtin_ctzll(mr) : (next ? 64 - lane + __builtin_ctzll(next) : cap);
        const int x = w * 64 + lane;
        if (x < d.nx) out[x] = (unsigned char)min(min(dl, dr), cap);
        prev = cur;
        cur = next;
    }
}

// FINAL = false: scan y (input g8, output h16); FINAL = true: scan z (input h16, output the field).
// grid: x = 64-lane chunks of a row * tiles of DF_TS rows of the scanned axis, y = the other axis, z = layer
template <bool FINAL>
__global__ void __launch_bounds__(DF_TPB) k_dist_axis(MapDims d, DistArgs a) {
    __shared__ unsigned short sq[(DF_TS + 2 * DF_RMAX) * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_scan = FINAL ? d.nz : d.ny;
    const int nxc = (int)grid_row_words(d);
    const int xc = blockIdx.x % nxc, tile = blockIdx.x / nxc;
    const int oth = blockIdx.y, layer = blockIdx.z;
    const int x = xc * 64 + lane;
    const int s0 = tile * DF_TS;
    const size_t plane = (size_t)d.nx * d.ny;
    const size_t stride = FINAL ? plane : (size_t)d.nx;
    const size_t base = (size_t)layer * d.v_glob + (FINAL ? (size_t)oth * d.nx : (size_t)oth * plane) + x;
    const int R = a.R, R2 = R * R;
    const int rows = DF_TS + 2 * R;
    for (int r = wave; r < rows; r += DF_WAVES) {
        const int si = s0 - R + r;
        unsigned v = 0xffffu;   // beyond the map / the row: never the minimum (its sum with dy^2 stays far inside an int)
        if (x < d.nx && (unsigned)si < (unsigned)n_scan) {
            if (FINAL) v = a.h16[base + (size_t)si * stride];
            else { const unsigned g = a.g8[base + (size_t)si * stride]; v = g * g; }
        }
        sq[r * 64 + lane] = (unsigned short)v;
    }
    __syncthreads();
    for (int j = wave; j < DF_TS; j += DF_WAVES) {
        const int si = s0 + j;
        if (si >= n_scan) break;   // (wave-uniform)
        const unsigned short* col = sq + (j + R) * 64 + lane;
        int best = x < d.nx ? min((int)col[0], R2) : 0;   // (a lane beyond the row never asks for another step)
        for (int dd = 1; dd <= R; ++dd) {
            const int dd2 = dd * dd;
            if (!__builtin_amdgcn_ballot_w64(dd2 < best)) break;   // no lane can improve any more: candidates further out cost >= dd^2
            best = min(best, min((int)col[dd * 64], (int)col[-dd * 64]) + dd2);
        }
        if (x >= d.nx) continue;
        if (!FINAL) {
            a.h16[base + (size_t)si * stride] = (unsigned short)best;
        } else {
            if (a.outside_occ) {   // the lattice point just outside each face: min(i + 1, n - i) steps away along that axis
                const int e = min(min(min(x + 1, d.nx - x), min(oth + 1, d.ny - oth)), min(si + 1, d.nz - si));
                best = min(best, e * e);
            }
            a.field[base + (size_t)si * stride] = __fmul_rn(sqrtf((float)best), d.res);   // (IEEE sqrt: correctly rounded)
        }
    }
}

// One thread per sample, as k_query<false, ...>: the field at the point's own voxel and up to six neighbours of the same layer.
__global__ void __launch_bounds__(DF_TPB) k_dist_query(MapDims d, DistQueryArgs a, int n, const float4* __restrict__ q,
                                                        float* __restrict__ dist, float* __restrict__ grad) {
    const unsigned i = blockIdx.x * DF_TPB + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 s = q[i];
    float v = a.outside, gx = 0.f, gy = 0.f, gz = 0.f;
    if (!(s.x != s.x || s.y != s.y || s.z != s.z || s.w != s.w)) {
        float px = s.x, py = s.y, pz = s.z;
        origin_apply(a.org, px, py, pz);
        int g;
        if (voxel_of(d, px, py, pz, g)) {
            const float* F = a.field + (size_t)(q_horizon(d, s.w) + 1) * d.v_glob;
            const int plane = d.nx * d.ny;
            const int iz = g / plane, rest = g - iz * plane, iy = rest / d.nx, ix = rest - iy * d.nx;
            v = F[g];
            if (grad) {
                if (d.nx > 1) {
                    const int lo = max(ix - 1, 0), hi = min(ix + 1, d.nx - 1);
                    gx = __fdiv_rn(__fsub_rn(F[g + (hi - ix)], F[g - (ix - lo)]), __fmul_rn((float)(hi - lo), d.res));
                }
                if (d.ny > 1) {
                    const int lo = max(iy - 1, 0), hi = min(iy + 1, d.ny - 1);
                    gy = __fdiv_rn(__fsub_rn(F[g + (hi - iy) * d.nx], F[g - (iy - lo) * d.nx]), __fmul_rn((float)(hi - lo), d.res));
                }
                if (d.nz > 1) {
                    const int lo = max(iz - 1, 0), hi = min(iz + 1, d.nz - 1);
                    gz = __fdiv_rn(__fsub_rn(F[g + (hi - iz) * plane], F[g - (iz - lo) * plane]), __fmul_rn((float)(hi - lo), d.res));
                }
            }
        }
    }
    dist[i] = v;
    if (grad) {
        grad[3 * (size_t)i] = gx;
        grad[3 * (size_t)i + 1] = gy;
        grad[3 * (size_t)i + 2] = gz;
    }
}

void launch_distance_field(const LaunchCtx& c, const DistArgs& a) {
    const MapDims& d = c.d;
    const int rows = d.ny * d.nz;
    const int nxc = (int)grid_row_words(d);
    hipLaunchKernelGGL(k_dist_x, dim3((rows + DF_WAVES - 1) / DF_WAVES, a.L), dim3(DF_TPB), 0, c.stream, d, c.s, a);
    hipLaunchKernelGGL((k_dist_axis<false>), dim3(nxc * ((d.ny + DF_TS - 1) / DF_TS), d.nz, a.L), dim3(DF_TPB), 0, c.stream, d, a);
    hipLaunchKernelGGL((k_dist_axis<true>), dim3(nxc * ((d.nz + DF_TS - 1) / DF_TS), d.ny, a.L), dim3(DF_TPB), 0, c.stream, d, a);
}

void launch_distance_query(const LaunchCtx& c, const DistQueryArgs& a, int n, const float4* q, float* dist, float* grad) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_dist_query, dim3((unsigned)(((long long)n + DF_TPB - 1) / DF_TPB)), dim3(DF_TPB), 0, c.stream, c.d, a, n, q,
                       dist, grad);
}
