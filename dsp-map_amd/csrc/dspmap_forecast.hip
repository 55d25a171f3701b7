// dspmap_forecast.hip -- occupancy forecast at caller-chosen times from the live particle set (dspmap_build_forecast, dspmap_query_forecast*;
// semantics next to them in include/dspmap.h).  The reference predicts at the PREDICTION_TIMES it was compiled with, inside its resampling
// loop (:950-964), from the weights before resampling and without the frame's newborns; a planner with its own knots has to take the next
// configured horizon.  The particles are in HBM after every frame: rolling them out to any list of times is one sweep.
//
//   k_forecast_sweep    one wave per 64-voxel tile, one lane per voxel, the access pattern of the frame's sweeps: the tile's flags through the
//                       scalar unit (an empty tile ends there), the occupancy words, then the live slot rows -- weights always, velocities only
//                       where the tile holds a moving particle (DevState::tile_moving), positions only for the rows that do.  A static
//                       particle's quantum stays in the lane's 64-bit sum (one plain store per voxel); a moving one adds it to its destination
//                       of every layer with one 64-bit integer atomic (fut_add).  Integer sums do not depend on the order of the adds: a layer
//                       is defined bit for bit.
//   k_forecast_combine  storage order -> the reference's voxel order: out[j][g] = fut_value(dyn[j][lv] + stat[lv]), coalesced float stores.
//   k_forecast_query    one thread per sample: the own voxel's value in the layer its t selects, or the fp32 interpolation of two layers.
// Nothing of the map is written: no accumulator, no per-tile flag.
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"

#define FC_TPB 256
#define FC_WAVES (FC_TPB / 64)
#define FC_RB 4   // slot rows requested together

// the layer (z index; the handle is unsharded) of storage voxel lv: a particle never leaves it (vz == 0)
__device__ __forceinline__ int fc_layer_of_lv(const MapDims& d, int lv) {
    return d.tiling ? ((lv >> 6) / (d.ncx * d.ncy)) * 4 + ((lv >> 4) & 3) : lv / (d.ny * d.nx);
}

// a particle's quantum: fut_quantum's integer for every weight the frame can produce; a negative weight (an import can hold one) would
// wrap in the conversion, so it is 0 here like a NaN
__device__ __forceinline__ u64 fc_quantum(float w) { return w > 0.f ? fut_quantum(w) : 0ull; }

template <int MW>
__global__ void __launch_bounds__(FC_TPB) k_forecast_sweep(MapDims d, DevState s, ForecastArgs a) {
    const int l = lane_id();
    const int BX = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * FC_WAVES + (threadIdx.x >> 6)));
    if (BX * 64 >= d.v_loc) return;   // (wave-uniform, as every exit below: the wave reductions see whole waves)
    int t_live, t_mov;
    sload_i2(s.tile_live + BX, s.tile_moving + BX, t_live, t_mov);   // one scalar round trip
    if (!t_live) return;              // no particle since the tile's last visit: its sums stay at the zero they were preset to
    if (!d.tile_skip) t_mov = 1;
    const int lv = BX * 64 + l;
    const bool inr = lv < d.v_loc;
    u64 m[MW];
    bool nonempty = false;
#pragma unroll
    for (int e = 0; e < MW; ++e) {
        m[e] = inr ? (s.mask[(size_t)lv * MW + e] | s.nbmask[(size_t)lv * MW + e]) : 0ull;   // every live particle, born this frame or not
        nonempty |= m[e] != 0ull;
    }
    if (!__ballot(nonempty)) return;
    const size_t tcell = (size_t)BX * d.slots * 64;
    const size_t V = (size_t)d.v_loc;
    const int zl = fc_layer_of_lv(d, inr ? lv : 0);
    u64 stat = 0ull;
#pragma unroll
    for (int e = 0; e < MW; ++e) {
        u64 tor = wave_or_u64(m[e]);   // rows of this word that are live in some voxel of the tile
        while (tor) {
            int row[FC_RB];
            float w[FC_RB];
            V2 vv[FC_RB];
#pragma unroll
            for (int r = 0; r < FC_RB; ++r) {
                row[r] = tor ? __ffsll((long long)tor) - 1 : -1;
                if (tor) tor &= tor - 1ull;
                const bool mine = row[r] >= 0 && ((m[e] >> row[r]) & 1ull);
                const size_t idx = tcell + (size_t)(e * 64 + (row[r] < 0 ? 0 : row[r])) * 64 + l;
                w[r] = 0.f; vv[r].x = 0.f; vv[r].y = 0.f;
                if (mine) {
                    w[r] = s.w[idx];
                    if (t_mov) vv[r] = ld_vel(s, idx);   // (a tile of static particles: its velocity rows are not fetched)
                } else {
                    row[r] = -1;
                }
            }
#pragma unroll
            for (int r = 0; r < FC_RB; ++r) {
                if (row[r] < 0) continue;
                const u64 q = fc_quantum(w[r]);
                if (vv[r].x == 0.f && vv[r].y == 0.f) { stat += q; continue; }   // p + 0 * t: this voxel, in every layer
                if (!q) continue;
                const P3 p = ld_pos(s, tcell + (size_t)(e * 64 + row[r]) * 64 + l);
                for (int j = 0; j < a.n; ++j) {
                    const float t = a.t[j];
                    const float fx = p.x + vv[r].x * t;   // (-ffp-contract=off: two roundings, as rollout_direct)
                    const float fy = p.y + vv[r].y * t;
                    if (!(fabsf(fx) < d.half_x && fabsf(fy) < d.half_y)) continue;   // (outside the map, or a NaN an import left in p or v)
                    const int xi = (int)div_res(d, fx + d.half_x);
                    const int yi = (int)div_res(d, fy + d.half_y);
                    if (xi >= d.nx || yi >= d.ny) continue;   // (the one float below half whose quotient rounds up to n)
                    const int dl = lv_of_xyz(d, xi, yi, zl);
                    if ((unsigned)dl < (unsigned)d.v_loc) fut_add(&a.dyn[(size_t)j * V + dl], q);
                }
            }
        }
    }
    if (inr) a.stat[lv] = stat;
}

// grid: x = 256 voxels of a layer in index order, y = layer
__global__ void __launch_bounds__(FC_TPB) k_forecast_combine(MapDims d, ForecastArgs a) {
    const int g = blockIdx.x * FC_TPB + threadIdx.x;
    const int j = blockIdx.y;
    if (g >= d.v_glob) return;
    const int lv = lv_of_true(d, g);   // (unsharded: v_base == 0)
    a.out[(size_t)j * d.v_glob + g] = fut_value(a.dyn[(size_t)j * d.v_loc + lv] + a.stat[lv]);
}

// One thread per sample, as k_dist_query: the point's own voxel, no footprint.
__global__ void __launch_bounds__(FC_TPB) k_forecast_query(MapDims d, ForecastQueryArgs a, int n, const float4* __restrict__ q,
                                                            float* __restrict__ out) {
    const unsigned i = blockIdx.x * FC_TPB + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 s = q[i];
    float v = a.outside;
    if (!(s.x != s.x || s.y != s.y || s.z != s.z || s.w != s.w)) {
        float px = s.x, py = s.y, pz = s.z;
        origin_apply(a.org, px, py, pz);
        int g;
        if (voxel_of(d, px, py, pz, g)) {
            int j = a.n;   // the smallest index with times[j] >= t
            for (int k = a.n - 1; k >= 0; --k)
                if (a.t[k] >= s.w) j = k;
            if (j >= a.n) {
                v = a.field[(size_t)(a.n - 1) * d.v_glob + g];
            } else if (j == 0 || !a.lerp) {
                v = a.field[(size_t)j * d.v_glob + g];
            } else {
                const float va = a.field[(size_t)(j - 1) * d.v_glob + g], vb = a.field[(size_t)j * d.v_glob + g];
                const float u = __fdiv_rn(__fsub_rn(s.w, a.t[j - 1]), __fsub_rn(a.t[j], a.t[j - 1]));
                v = __fadd_rn(va, __fmul_rn(u, __fsub_rn(vb, va)));
            }
        }
    }
    out[i] = v;
}

// (the caller has zeroed a.dyn and a.stat on the stream: the moving particles' accumulators and the static sums of the tiles the sweep leaves early)
void launch_forecast(const LaunchCtx& c, const ForecastArgs& a) {
    const MapDims& d = c.d;
    const int ntiles = (d.v_loc + 63) / 64;
    const dim3 grid((ntiles + FC_WAVES - 1) / FC_WAVES);
    if (d.mw == 1) hipLaunchKernelGGL((k_forecast_sweep<1>), grid, dim3(FC_TPB), 0, c.stream, d, c.s, a);
    else hipLaunchKernelGGL((k_forecast_sweep<2>), grid, dim3(FC_TPB), 0, c.stream, d, c.s, a);
    hipLaunchKernelGGL(k_forecast_combine, dim3((d.v_glob + FC_TPB - 1) / FC_TPB, a.n), dim3(FC_TPB), 0, c.stream, d, a);
}

void launch_forecast_query(const LaunchCtx& c, const ForecastQueryArgs& a, int n, const float4* q, float* out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_forecast_query, dim3((unsigned)(((long long)n + FC_TPB - 1) / FC_TPB)), dim3(FC_TPB), 0, c.stream, c.d, a, n, q, out);
}
