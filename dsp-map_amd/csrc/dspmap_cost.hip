// dspmap_cost.hip -- clearance-weighted cost-to-go fields: a bucketed (Dial) wavefront through one layer of the cast grid, the step into a
// cell weighted by the clearance band the distance field puts it in (dspmap_build_cost_fields*, dspmap_cost_paths*; semantics next to them
// in include/dspmap.h).  The reference has no counterpart: a planner that wants "short, but rather through the middle of the corridor"
// copies the grid, the distance layer and the paths out and runs Dijkstra on the host.
//
// The work: with integer weights 1 .. 8 the cells of cost exactly c are
//     N_c = ( union over k = 1 .. 8 of  N6(N_{c-k}) & W_k )  &  ~settled,          W_k = the free cells of weight k,
// one bit per voxel in the cast grid's word layout.  The levels of a field are strictly sequential (up to DSPMAP_COST_MAX_COST of them), the
// fields of a batch are independent, W_k and the weight bytes are the same for all fields of a build.
//
// Chosen: k_cost_weights, a launch of its own ahead of the wavefront, one wave per word: a lane reads its cell's float of the distance
// layer, the eight ballots of (w == k) ARE the words of W_1 .. W_8, and the weight byte goes out coalesced.  The weight values that occur
// are ORed into one device word.  Then k_cost_wave, ONE WORKGROUP OF 1024 THREADS PER FIELD for every level in ONE launch, the owner-of-a-word
// scheme of k_reach (dspmap_reach.hip) on the helpers both share (dspmap_grid.h: grid_cell, GridWords, grid_grow6, grid_store_bits)
// and with its three rotating verdict flags.  The paths are launch_field_paths of dspmap_reach.hip, WEIGHTED.  Per field the
// device scratch holds eleven sets: a ring of the last eight GROWN level sets G_j = N6(N_j), two level sets N in ping-pong, and the
// settled set.  A level is
//     phase A: own word only -- OR of G_{c-k}[t] & W_k[t] over the k that occur and whose ring slot is not known to be empty, and-not settled;
//              the new bits go to N[i & 1] (i counts the levels executed), into settled, and their cells get the value c (a bit is new
//              once, so no test of the field);
//     barrier + verdict;
//     phase B: only if the level is not empty: G_c[t] = the grown N[i & 1], seven reads, into ring slot c & 7.
// Phase A of the next level reads own words of G only, so ONE barrier per level orders everything: N[i & 1] is next written in phase A of
// executed level i + 2, behind the barrier of level i + 1 that every reader of phase B_i has passed.  Holding the grown set in the ring (against
// N_j itself) takes the neighbour reads out of the loop over k and, with the ping-pong, costs no second barrier.  Which ring slots are
// empty is the same in every thread (it comes from the verdicts), so a level that no live slot can feed -- the gaps in front of a heavy
// cell -- is skipped without a barrier or a memory access.  The loop ends when all eight slots are empty or c > max_cost.  The scratch is
// re-read every level by one workgroup on one CU and so stays in L2, as k_reach<LDS = false>'s does; workgroup-scope ordering of
// __syncthreads() is all it needs.  Every loop is bounded by max_cost, the word count, the source count or max_len; nothing waits on
// another workgroup.
//
// Rejected:
//  - an LDS home for the sets: eleven (or, with N_j in the ring, ten) sets of 42 KB do not fit the CU's 160 KiB on 66 x 66 x 40, the map
//    the project measures, and a second home for small maps only is a second set of ways to go wrong.
//  - more than one workgroup per field: a spin on memory another workgroup writes deadlocks as soon as the workgroups are not all
//    resident (dspmap_reach.hip, top), and a hung kernel takes the device from everyone.
//  - the ring holding N_j, grown inside the loop over k: seven reads per occurring weight and level instead of one.
//  - uint16 values relaxed in place (Bellman-Ford): 16 times the memory traffic of a bit per cell, and an unbounded number of sweeps.
//  - a heap or a per-cell bucket queue: serial per field, and the bit sets already are the buckets.
//  - one launch per level: up to 16 384 launches, and the exit rule would need a read-back per level.
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"

#define COST_TPB 1024
#define COST_W_TPB 256

// one wave per word of the layer: lane = bit = x & 63.  weight[V] bytes, wk[8][nwords] the sets W_1 .. W_8, *occ |= 1 << k for every k that occurs
__global__ void __launch_bounds__(COST_W_TPB) k_cost_weights(MapDims d, CostWeightArgs a) {
    const unsigned lane = threadIdx.x & 63;
    const GridWords gw(d);
    const unsigned W = gw.W, nwords = gw.nwords;
    const unsigned t = blockIdx.x * (COST_W_TPB / 64) + (threadIdx.x >> 6);   // (the same for the whole wave)
    if (t >= nwords) return;
    const unsigned yz = t / W, w = t - yz * W, x = w * 64 + lane;
    const bool inside = x < (unsigned)d.nx;
    const size_t cell = (size_t)yz * d.nx + x;
    const u64 blocked = a.bits[t];
    int wt = 0;
    if (inside && !((blocked >> lane) & 1)) {
        wt = 1;
        if (a.n_bands > 0) {
            const float F = a.dist[cell];
#pragma unroll
            for (int i = 0; i < COST_MAX_BANDS; ++i)
                if (i < a.n_bands && F < a.clearance[i]) wt += a.penalty[i];
        }
    }
    if (inside) a.weight[cell] = (unsigned char)wt;
    u64 mine = 0;
    int occ = 0;
#pragma unroll
    for (int k = 1; k <= COST_MAX_WEIGHT; ++k) {
        const u64 b = __ballot(wt == k);
        if (lane == (unsigned)(k - 1)) mine = b;
        if (b) occ |= 1 << k;
    }
    if (lane < COST_MAX_WEIGHT) a.wk[(size_t)lane * nwords + t] = mine;
    if (lane == 0 && occ) atomicOr(a.occ, occ);
}

// the sets of field f (COST_SET_COUNT): [0, 8) the ring of grown level sets, [8, 10) the level sets in ping-pong, [10] settled
__global__ void __launch_bounds__(COST_TPB) k_cost_wave(MapDims d, CostArgs a, const float4* __restrict__ src) {
    __shared__ int s_flag[3];   // bit 0: the level is not empty
    const unsigned tid = threadIdx.x, f = blockIdx.x;
    const GridWords gw(d);
    const unsigned W = gw.W, plane = gw.plane, nwords = gw.nwords;
    u64* ring = a.sets + (size_t)f * COST_SET_COUNT * nwords;
    u64* lvl = ring + (size_t)8 * nwords;
    u64* settled = ring + (size_t)10 * nwords;
    unsigned short* fld = a.field + (size_t)f * d.v_glob;
    const u64* __restrict__ wk = a.wk;
    const int occ = *a.occ;       // bit k: weight k occurs in this build (written by k_cost_weights, a launch earlier)

    for (unsigned t = tid; t < nwords; t += COST_TPB) lvl[t] = 0;
    if (tid < 3) s_flag[tid] = 0;
    __syncthreads();
    for (unsigned i = tid; i < (unsigned)a.n_src; i += COST_TPB) {
        const float4 p = src[i];
        if ((unsigned)__float_as_int(p.w) != f) continue;   // (a field outside [0, n_fields) matches no workgroup)
        int x, y, z;
        if (grid_cell(d, a.org, p.x, p.y, p.z, x, y, z) != 0) continue;
        atomicOr((unsigned long long*)&lvl[gw.word_of(d, x, y, z)], GridWords::bit_of(x));
    }
    __syncthreads();
    unsigned live = 0;            // bit j: ring slot j holds a non-empty grown set (the same in every thread)
    unsigned it = 0;              // levels that took the barrier: the index of the verdict flag
    for (int c = 0; c <= a.max_cost; ++c) {
        unsigned use = 0;         // the k whose slot is live and whose weight occurs
        if (c > 0) {
            for (int k = 1; k <= COST_MAX_WEIGHT; ++k)
                if (((occ >> k) & 1) && c >= k && ((live >> ((c - k) & 7)) & 1)) use |= 1u << k;
            if (!use) {           // nothing can feed this level: it is empty, and so is its slot
                live &= ~(1u << (c & 7));
                if (!live) break;
                continue;
            }
        }
        u64* N = lvl + (size_t)(it & 1) * nwords;       // (by executed level, not by c: a skipped level takes no barrier)
        int verdict = 0;
        for (unsigned t = tid; t < nwords; t += COST_TPB) {   // phase A: own words only
            u64 fresh;
            if (c == 0) {
                fresh = N[t];
                if (fresh) {      // a source in a blocked cell is ignored: the free cells are the union of the W_k
                    u64 free_w = 0;
                    for (int k = 1; k <= COST_MAX_WEIGHT; ++k)
                        if ((occ >> k) & 1) free_w |= wk[(size_t)(k - 1) * nwords + t];
                    fresh &= free_w;
                }
                settled[t] = fresh;
            } else {
                u64 cand = 0;
                for (unsigned u = use; u; u &= u - 1) {
                    const int k = __builtin_ctz(u);
                    const u64 g = ring[(size_t)((c - k) & 7) * nwords + t];
                    if (g) cand |= g & wk[(size_t)(k - 1) * nwords + t];
                }
                fresh = cand;
                if (cand) {
                    const u64 s = settled[t];
                    fresh = cand & ~s;
                    if (fresh) settled[t] = s | fresh;
                }
            }
            N[t] = fresh;
            if (fresh) {
                verdict = 1;
                const unsigned yz = t / W, w = t - yz * W;
                grid_store_bits(fld + (size_t)yz * d.nx + w * 64, fresh, (unsigned short)c);
            }
        }
        if (verdict) atomicOr(&s_flag[it % 3], 1);
        if (tid == 0) s_flag[(it + 1) % 3] = 0;        // (its last readers, those of barrier it - 2, are past barrier it - 1)
        __syncthreads();
        const int v = s_flag[it % 3];
        ++it;
        if (!v) {
            live &= ~(1u << (c & 7));
            if (!live) break;                          // eight empty levels in a row: every later one is empty
            continue;
        }
        live |= 1u << (c & 7);
        u64* G = ring + (size_t)(c & 7) * nwords;
        for (unsigned t = tid; t < nwords; t += COST_TPB) {   // phase B: the grown set of this level into its slot
            const unsigned z = t / plane, r = t - z * plane, y = r / W, w = r - y * W;
            G[t] = grid_grow6<false>(N + t, N[t], w, y, z, gw, d);  // (bits at x >= nx may be set here; no W_k holds them)
        }
    }
}

void launch_cost_weights(const LaunchCtx& c, const CostWeightArgs& a) {
    const MapDims& d = c.d;
    const size_t nwords = grid_layer_words(d);
    const unsigned per = COST_W_TPB / 64;
    hipLaunchKernelGGL(k_cost_weights, dim3((unsigned)((nwords + per - 1) / per)), dim3(COST_W_TPB), 0, c.stream, d, a);
}

void launch_cost_wave(const LaunchCtx& c, const CostArgs& a, const dspmap_reach_point* src) {
    if (a.n_fields <= 0) return;
    hipLaunchKernelGGL(k_cost_wave, dim3(a.n_fields), dim3(COST_TPB), 0, c.stream, c.d, a, (const float4*)src);
}
