// dspmap_cast_walk.h -- the Amanatides-Woo walk of a segment through the cast grid (include/dspmap.h, dspmap_cast_segments, steps 2 - 4) as ONE
// device function: k_cast (dspmap_cast.hip) runs it per segment, k_view_score (dspmap_view.hip) per ray of a candidate view.  Both get the
// same instructions, so a view's rays are casts bit for bit.
#pragma once
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "../../include/dspmap.h"

// one axis of the DDA set-up (include/dspmap.h, steps 2 and 3); pa is inside the map along this axis.  (grid_axis_cell's quotient, which
// the walk needs unrounded as well)
__device__ __forceinline__ void cast_axis(float pa, float pb, float half, float res, int& i, int& st, float& tmax, float& tdelta) {
    const float ua = __fdiv_rn(__fadd_rn(pa, half), res), ub = __fdiv_rn(__fadd_rn(pb, half), res);
    i = (int)ua;
    const float dd = __fsub_rn(ub, ua);
    st = dd > 0.f ? 1 : (dd < 0.f ? -1 : 0);
    tmax = INFINITY;
    tdelta = 0.f;
    if (st != 0) {
        const float bnd = (float)(i + (st > 0 ? 1 : 0));
        tmax = __fdiv_rn(__fsub_rn(bnd, ua), dd);
        tdelta = __fdiv_rn(1.0f, fabsf(dd));
    }
}

// The cast of the map-frame segment a -> b with times ta, tb (all finite / not NaN: step 1 is the caller's) through bits [L][nz][ny][W]:
// s, voxel, layer, status as dspmap_cast_hit names them.  At most nx + ny + nz steps.
__device__ __forceinline__ void cast_walk(const MapDims& d, const u64* __restrict__ bits, float ax, float ay, float az, float ta, float bx, float by,
                                          float bz, float tb, float& s, int& voxel, int& layer, int& status) {
    s = 0.f; voxel = -1; layer = -1;
    int ix = 0, iy = 0, iz = 0, sx = 0, sy = 0, sz = 0;
    float tmx = INFINITY, tmy = INFINITY, tmz = INFINITY, tdx = 0.f, tdy = 0.f, tdz = 0.f;
    bool inside = !grid_beyond(d, ax, ay, az);
    if (inside) {
        cast_axis(ax, bx, d.half_x, d.res, ix, sx, tmx, tdx);
        cast_axis(ay, by, d.half_y, d.res, iy, sy, tmy, tdy);
        cast_axis(az, bz, d.half_z, d.res, iz, sz, tmz, tdz);
        inside = ix < d.nx && iy < d.ny && iz < d.nz;   // (all >= 0: p > -half)
    }
    status = DSPMAP_CAST_START_OUTSIDE;
    if (inside) {
        const bool timed = !(ta < 0.f) && d.T > 0;
        const float dt = __fsub_rn(tb, ta);
        const size_t nw = (size_t)(d.nx + 63) >> 6, rows = (size_t)d.ny * d.nz;   // (the walk keeps its own 64-bit form of the word layout)
        int l_in = timed ? q_horizon(d, __fadd_rn(ta, __fmul_rn(0.f, dt))) + 1 : 0;
        size_t key = ~(size_t)0;
        u64 word = 0;
        float s_in = 0.f;
        status = DSPMAP_CAST_INVALID;   // (never left standing: the loop below ends within nx + ny + nz steps)
        const int max_steps = d.nx + d.ny + d.nz;
        for (int it = 0; it <= max_steps; ++it) {
            const bool mx = tmx <= tmy && tmx <= tmz;
            const bool my = !mx && tmy <= tmz;
            const float tm = mx ? tmx : (my ? tmy : tmz);
            int l_out = 0;
            if (timed) l_out = q_horizon(d, __fadd_rn(ta, __fmul_rn(fminf(tm, 1.f), dt))) + 1;
            const int l0 = min(l_in, l_out), l1 = max(l_in, l_out);
            const size_t cell = ((size_t)iz * d.ny + iy) * nw + ((unsigned)ix >> 6);
            int l = l0;
            for (; l <= l1; ++l) {
                const size_t k = (size_t)l * rows * nw + cell;
                if (k != key) { word = bits[k]; key = k; }
                if ((word >> (ix & 63)) & 1ull) break;
            }
            const int here = (iz * d.ny + iy) * d.nx + ix;
            if (l <= l1) { s = s_in; voxel = here; layer = l; status = DSPMAP_CAST_HIT; break; }
            if (!(tm <= 1.f)) { s = 1.f; status = DSPMAP_CAST_FREE; break; }
            s_in = tm;
            l_in = l_out;   // t_in of the next cell is t_out of this one: the same expression of the same parameter (tm <= 1)
            bool left;
            if (mx) { ix += sx; tmx = __fadd_rn(tm, tdx); left = (unsigned)ix >= (unsigned)d.nx; }
            else if (my) { iy += sy; tmy = __fadd_rn(tm, tdy); left = (unsigned)iy >= (unsigned)d.ny; }
            else { iz += sz; tmz = __fadd_rn(tm, tdz); left = (unsigned)iz >= (unsigned)d.nz; }
            if (left) { s = s_in; voxel = here; status = DSPMAP_CAST_LEFT_MAP; break; }
        }
    }
}
