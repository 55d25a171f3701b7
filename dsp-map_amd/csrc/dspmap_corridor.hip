// dspmap_corridor.hip -- axis-aligned free boxes (safe corridors) grown in the cast grid (dspmap_grow_boxes*; semantics next to them in
// include/dspmap.h).  The reference has no counterpart: a planner that wants the largest free box around a piece of its path copies the
// grid out (getOccupancyMapWithFutureStatus :405-426) and grows the box in a host loop.
//
// The work: a box is grown face by face, and a face test asks "is any bit set in this slab, in any tested layer?".  The slab of a y or z
// face is rows of words, the slab of an x face is one bit of one word per (y, z).  The face tests of one box are strictly sequential (the
// slab of a face depends on every extension made before it), so the parallelism inside a box is the width of ONE slab, and the
// parallelism of a batch is its seeds.
//
// Chosen: ONE WAVE PER SEED.  Every slab -- the seed box itself, an x, a y or a z face -- is the same thing: a box [x0, x1] x [y0, y1] x
// [z0, z1] of cells times nl tested layers, and box_blocked() answers it for all of them.  The 64 lanes spread over (word of the x range,
// y, z, layer), the word index fastest, so that neighbouring lanes read neighbouring words of a row and then neighbouring rows.  A lane
// loads its word, masks it to the x range (the first and the last word of the range; an x face has a one-bit range in one word) and
// the verdict is one wave-wide vote (__any).  A lane takes BOX_ILP items 64 apart per vote, so that several loads are in flight before
// the wave waits, and the wave leaves the slab at the first vote that finds a bit: an obstacle in the first 256 items costs one round
// trip.  The box state (lo, hi, the active faces, the causes) is made wave-uniform with readfirstlane and lives in scalar registers; the
// loop over rounds and faces branches on scalars, never per lane.  Per seed: two 16-byte loads in (every lane reads the same address:
// one request), two 16-byte stores out by lane 0.  The grids are 0.3 MB to a few MB and sit in L2; the slabs of consecutive rounds
// overlap in all but one row, so most words come from the CU's vector cache.
//
// Rejected:
//  - one lane per seed, as k_cast does it: a face test of a 17 x 9 slab in two layers is 300 dependent-free loads that a lane would issue
//    one after the other, a box of 40 face tests thousands, and the lanes of a wave diverge in all of it.  k_cast's lanes keep one word
//    in registers and step inside it; a growing box has no such locality per lane.
//  - a workgroup (4 waves) per seed: a typical slab at max_grow (8, 8, 4) holds 50 - 600 items, one to three votes of one wave; four waves
//    would share 1 - 2 items per lane and pay an LDS round and two barriers per face test for the joint verdict, ~40 times per box.  The
//    batch supplies the occupancy instead: 32 768 seeds are 32 768 waves.
//  - per-column ORs of the tested layers cached in LDS: the columns a box reads are those of its final extent, up to 129 x 129 words
//    per seed at the largest max_grow -- 130 KB, and the same words would be read once from L2 to fill it as are read from the vector
//    cache without it.  It removes the layer factor (nl <= T + 1) from later rounds only.
//  - pre-ORing the layers per distinct (l0, l1) of the batch into a grid of its own: up to (T + 1)(T + 2) / 2 = 28 extra grids (56 with
//    DSPMAP_BOX_WITH_CURRENT), each the size of a layer, built per call for a batch that may use two of them, plus a pass over the seeds
//    to find the distinct pairs and a sort or an indirection per seed.  It would pay for batches of one time window; the entry point
//    does not know that, and a caller who does can build its grid for that window and pass ta = tb.
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"

#define BOX_TPB 256
#define BOX_WAVES (BOX_TPB / 64)
#define BOX_ILP 4   // items per lane between two votes

// the tested layers of a seed: [l0, l0 + nl - extra) and, if extra, layer 0 in front of them
struct BoxLayers {
    int l0, nl, extra;
};

// is a bit set in the cells [x0, x1] x [y0, y1] x [z0, z1] (inside the map) of any tested layer?  Called by whole waves with wave-uniform
// arguments; the answer is wave-uniform.
__device__ __forceinline__ bool box_blocked(const MapDims& d, const u64* __restrict__ bits, int lane, int x0, int x1, int y0, int y1, int z0, int z1,
                                            const BoxLayers& ly) {
    const unsigned w0 = (unsigned)x0 >> 6, nwd = ((unsigned)x1 >> 6) - w0 + 1, nyr = (unsigned)(y1 - y0 + 1), nzr = (unsigned)(z1 - z0 + 1);
    const unsigned nw = grid_row_words(d);
    const size_t layer_words = grid_layer_words(d);
    const unsigned items = nwd * nyr * nzr * (unsigned)ly.nl;   // (<= W * ny * nz * L < 2^31: dspmap_build_cast_grid refuses more)
    const u64 first = ~0ull << (x0 & 63), last = ~0ull >> (63 - (x1 & 63));
    for (unsigned base = 0; base < items; base += 64 * BOX_ILP) {
        bool hit = false;
#pragma unroll
        for (int u = 0; u < BOX_ILP; ++u) {
            unsigned t = base + u * 64 + lane;
            if (t < items) {
                const unsigned wi = t % nwd; t /= nwd;
                const unsigned yi = t % nyr; t /= nyr;
                const unsigned zi = t % nzr; t /= nzr;                       // t: index into the tested layers
                const int layer = (int)t < ly.extra ? 0 : ly.l0 + (int)t - ly.extra;
                u64 word = bits[(size_t)layer * layer_words + ((size_t)(z0 + zi) * d.ny + (y0 + yi)) * nw + (w0 + wi)];
                if (wi == 0) word &= first;
                if (wi + 1 == nwd) word &= last;
                hit |= word != 0;
            }
        }
        if (__any(hit)) return true;
    }
    return false;
}

// one axis of the seed box (include/dspmap.h, step 2): both end points inside the map along it, the cells they lie in
__device__ __forceinline__ bool box_axis(float pa, float pb, float half, float res, int n, int& lo, int& hi) {
    if (fabsf(pa) >= half || fabsf(pb) >= half) return false;   // dspmap_point_voxel_index's test (NaN-free here)
    const int ia = grid_axis_cell(pa, half, res), ib = grid_axis_cell(pb, half, res);
    lo = min(ia, ib);
    hi = max(ia, ib);
    return hi < n;
}

__global__ void __launch_bounds__(BOX_TPB) k_grow_boxes(MapDims d, BoxArgs a, int n, const float4* __restrict__ seg, int4* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const unsigned i = blockIdx.x * BOX_WAVES + (threadIdx.x >> 6);   // the wave's seed (unsigned: n may come within a block of INT_MAX)
    if (i >= (unsigned)n) return;                                     // (wave-uniform)
    const float4 A = seg[2 * (size_t)i], B = seg[2 * (size_t)i + 1];  // {ax, ay, az, ta}, {bx, by, bz, tb}
    int lo[3] = {-1, -1, -1}, hi[3] = {-1, -1, -1};
    int status = DSPMAP_BOX_INVALID;
    unsigned stop = 0;
    const bool valid = grid_finite(A.x) && grid_finite(A.y) && grid_finite(A.z) && grid_finite(B.x) && grid_finite(B.y) && grid_finite(B.z) &&
                       A.w == A.w && B.w == B.w;
    if (valid) {
        float ax = A.x, ay = A.y, az = A.z, bx = B.x, by = B.y, bz = B.z;
        origin_apply(a.org, ax, ay, az, bx, by, bz);
        int l[3], h[3];
        bool inside = box_axis(ax, bx, d.half_x, d.res, d.nx, l[0], h[0]);
        inside = box_axis(ay, by, d.half_y, d.res, d.ny, l[1], h[1]) && inside;
        inside = box_axis(az, bz, d.half_z, d.res, d.nz, l[2], h[2]) && inside;
        status = DSPMAP_BOX_SEED_OUTSIDE;
        if (grid_uniform(inside ? 1 : 0)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = grid_uniform(l[k]); hi[k] = grid_uniform(h[k]); }
            // the layers of cast step 4 with t_in = ta, t_out = tb: layer 0 only if ta < 0 (or T == 0, where q_horizon gives -1 for every t)
            int la = 0, lb = 0;
            if (!(A.w < 0.f)) { la = q_horizon(d, A.w) + 1; lb = q_horizon(d, B.w) + 1; }
            BoxLayers ly;
            ly.l0 = grid_uniform(min(la, lb));
            ly.extra = (a.with_current && ly.l0 > 0) ? 1 : 0;
            ly.nl = grid_uniform(max(la, lb)) - ly.l0 + 1 + ly.extra;
            if (box_blocked(d, a.bits, lane, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], ly)) {
                status = DSPMAP_BOX_SEED_BLOCKED;
            } else {
                status = DSPMAP_BOX_OK;
                const int nn[3] = {d.nx, d.ny, d.nz};
                const int slo[3] = {lo[0], lo[1], lo[2]}, shi[3] = {hi[0], hi[1], hi[2]};   // the seed box: what max_grow is measured from
                unsigned active = 0x3f;
                while (active) {   // a face is tested at most max_grow + 1 <= 65 times
#pragma unroll
                    for (int f = 0; f < 6; ++f) {
                        if (!((active >> f) & 1u)) continue;
                        const int ax_ = f >> 1, up = f & 1;
                        const int c = up ? hi[ax_] + 1 : lo[ax_] - 1;
                        unsigned cause = 0;
                        if (c < 0 || c >= nn[ax_]) {
                            cause = DSPMAP_BOX_STOP_EDGE;
                        } else if ((up ? c - shi[ax_] : slo[ax_] - c) > a.grow[ax_]) {
                            cause = DSPMAP_BOX_STOP_LIMIT;
                        } else {
                            int s0[3] = {lo[0], lo[1], lo[2]}, s1[3] = {hi[0], hi[1], hi[2]};
                            s0[ax_] = s1[ax_] = c;
                            if (box_blocked(d, a.bits, lane, s0[0], s1[0], s0[1], s1[1], s0[2], s1[2], ly)) cause = DSPMAP_BOX_STOP_OBSTACLE;
                        }
                        if (cause) {
                            active &= ~(1u << f);
                            stop |= cause << (2 * f);
                        } else if (up) {
                            hi[ax_] = c;
                        } else {
                            lo[ax_] = c;
                        }
                    }
                }
            }
        }
    }
    if (lane == 0) {
        out[2 * (size_t)i] = make_int4(lo[0], lo[1], lo[2], hi[0]);
        out[2 * (size_t)i + 1] = make_int4(hi[1], hi[2], status, (int)stop);
    }
}

void launch_grow_boxes(const LaunchCtx& c, const BoxArgs& a, int n, const dspmap_segment* seed, dspmap_box* out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_grow_boxes, dim3((unsigned)(((long long)n + BOX_WAVES - 1) / BOX_WAVES)), dim3(BOX_TPB), 0, c.stream, c.d, a, n,
                       (const float4*)seed, (int4*)out);
}
