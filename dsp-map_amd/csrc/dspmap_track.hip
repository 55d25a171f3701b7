// dspmap_track.hip -- the objects of consecutive builds associated by voxel overlap: persistent ids, age, parent (dspmap_track_update and
// its accessors; semantics next to them in include/dspmap.h).  The reference has no counterpart.  Inputs: label grid, records and counts of
// the valid dspmap_build_objects, the tracker's own copies of the same three from the previous update and the previous tracks.  Integers
// throughout but the predicted shift, whose double operations are each rounded on their own, so the update is defined bit for bit.
//
// Separate launches, all on the handle's stream, no host read between them:
//   k_track_shift    one thread per previous track: its predicted shift in voxels from momentum / mass, dt and the window move.
//   k_track_pairs    one wave per word item (z, y, w) of the PREVIOUS label grid (the decomposition of k_objects_accumulate), lane = x.
//                    A lane whose cell holds ordinal j < K_prev looks at the current label grid at its shifted cell; a current ordinal
//                    o < K_now there makes the pair (j, o).  Lanes whose pair equals that of the lane before them form a run; the run's
//                    first lane inserts the run's length into the open-addressing table n(j, o) -- a 64-bit compare-and-swap on the key,
//                    then an integer add on the count.  (DSPMAP_TRACK_PER_CELL: every lane inserts 1.)  Integer sums do not depend on
//                    the order of arrival; the SLOT a pair lands in does, and nothing behind this kernel depends on the slot.
//   k_track_best     one thread per table slot: (n << 32 | 0x7fffffff - index) by atomicMax into best_prev[j] and best_now[o] -- the
//                    largest n wins, ties go to the smaller index --, and the number of pairs.
//   k_track_sums / _scan / _emit   ordered compaction (the pattern of dspmap_objects.hip) of the unmatched current objects into ranks; _emit
//                    writes one record per current object.
//   k_track_keep     one thread: the counts, next_id and the number of records the stored previous state holds; a full pair table makes
//                    the update void here.
// Every probe loop is bounded by the table size.  Nothing of the map, the grid or the objects is written.
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"
#include "dspmap_block_scan.h"

#define TK_TPB 256
#define TK_WAVES (TK_TPB / 64)
static_assert(FR_TILE == TK_TPB, "a tile is one record per thread");
static_assert(sizeof(dspmap_track) == 72, "dspmap_track is 72 bytes");
static_assert(2 * TRK_ORD_BITS < 64, "a pair's key holds two ordinals");

// the records the current build kept / the stored previous state holds (0 where nothing is associated)
__device__ __forceinline__ int tk_k_now(const TrackArgs& a) {
    long long n = a.obj_counts[0];
    if (n > a.max_objects) n = a.max_objects;
    if (n > a.cap) n = a.cap;
    return n < 0 ? 0 : (int)n;
}
__device__ __forceinline__ int tk_k_prev(const TrackArgs& a) {
    if (a.fresh) return 0;
    long long n = a.counts[TRK_KEPT];
    if (n > a.cap) n = a.cap;
    return n < 0 ? 0 : (int)n;
}

__global__ void __launch_bounds__(TK_TPB) k_track_shift(MapDims d, TrackArgs a) {
    const int j = (int)(blockIdx.x * TK_TPB + threadIdx.x);
    if (j >= tk_k_prev(a)) return;
    const dspmap_object r = a.p_objects[j];
    int4 s = make_int4(-a.dk0[0], -a.dk0[1], -a.dk0[2], 0);
    if (r.mass_q > 0) {
        const double lim = (double)a.max_shift;
        int p3[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = (double)r.mom_q[k] / (double)r.mass_q;
            const double dd = v * (double)a.dt;
            const double e = dd / (double)d.res;
            double p = floor(e + 0.5);
            p = p < -lim ? -lim : (p > lim ? lim : p);
            p3[k] = (int)p;
        }
        s.x += p3[0]; s.y += p3[1]; s.z += p3[2];
    }
    a.shift[j] = s;
}

// n(j, o) += n: linear probing from the key's hash, at most `slots` probes; a table without a slot for the key sets the fault word
__device__ __forceinline__ void tk_insert(const TrackArgs& a, u64 key, int n) {
    const unsigned mask = (unsigned)a.slots - 1u;
    unsigned slot = (unsigned)((key * 0x9e3779b97f4a7c15ull) >> 32) & mask;
    for (int probe = 0; probe < a.slots; ++probe, slot = (slot + 1u) & mask) {
        u64 cur = __hip_atomic_load(a.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) {
            cur = atomicCAS((unsigned long long*)(a.keys + slot), 0ull, (unsigned long long)key);
            if (cur == 0ull) cur = key;
        }
        if (cur == key) { atomicAdd(a.vals + slot, n); return; }
        // (a full table: the update is void already, do not walk the rest of it)
        if ((probe & 63) == 63 && __hip_atomic_load(a.counts + TRK_FAULT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    }
    atomicOr((unsigned long long*)&a.counts[TRK_FAULT], 1ull);
}

template <bool PER_CELL>
__global__ void __launch_bounds__(TK_TPB) k_track_pairs(MapDims d, TrackArgs a, int n_items) {
    const int item = (int)blockIdx.x * TK_WAVES + ((int)threadIdx.x >> 6);
    if (item >= n_items) return;   // (wave-uniform)
    const int l = lane_id();
    const int W = (int)grid_row_words(d);
    const int w = item % W, row = item / W, y = row % d.ny, z = row / d.ny;
    const int x = w * 64 + l;
    const int kp = tk_k_prev(a), kn = tk_k_now(a);
    u64 key = 0ull;
    if (x < d.nx) {
        const int j = a.p_labels[row * d.nx + x];
        if (j >= 0 && j < kp) {
            const int4 s = a.shift[j];
            const int xx = x + s.x, yy = y + s.y, zz = z + s.z;
            if (xx >= 0 && xx < d.nx && yy >= 0 && yy < d.ny && zz >= 0 && zz < d.nz) {
                const int o = a.labels[(zz * d.ny + yy) * d.nx + xx];
                if (o >= 0 && o < kn) key = (((u64)j << TRK_ORD_BITS) | (u64)o) + 1ull;
            }
        }
    }
    if (!__ballot(key != 0ull)) return;   // (wave-uniform)
    if (PER_CELL) {
        if (key) tk_insert(a, key, 1);
        return;
    }
    // runs of equal pairs: bit l of cont = lane l continues the run of lane l - 1; a run's first lane adds its length
    const u64 before = __shfl_up(key, 1, WAVE);
    const bool cont = key != 0ull && l > 0 && key == before;
    const u64 contm = __ballot(cont);
    if (key == 0ull || cont) return;
    const u64 rest = l < 63 ? contm >> (l + 1) : 0ull;                    // (its top bit is clear)
    const int more = (int)__ffsll((long long)~rest) - 1;                  // lanes that continue this run
    const u64 run = (more >= 63 ? ~0ull : (1ull << (more + 1)) - 1ull) << l;
    tk_insert(a, key, (int)__popcll(run));
}

__global__ void __launch_bounds__(TK_TPB) k_track_best(TrackArgs a) {
    const int slot = (int)(blockIdx.x * TK_TPB + threadIdx.x);
    const u64 key = slot < a.slots ? a.keys[slot] : 0ull;
    const u64 used = __ballot(key != 0ull);
    if (!used) return;   // (wave-uniform)
    if (lane_id() == (int)__ffsll((long long)used) - 1) atomicAdd((unsigned long long*)&a.counts[4], (unsigned long long)__popcll(used));
    if (!key) return;
    const u64 k = key - 1ull;
    const int j = (int)(k >> TRK_ORD_BITS), o = (int)(k & ((1u << TRK_ORD_BITS) - 1u));
    const u64 n = (u64)(unsigned)a.vals[slot] << 32;
    if (j >= a.cap || o >= a.cap) return;   // (cannot be: both were below K_prev and K_now)
    atomicMax((unsigned long long*)(a.best_prev + j), (unsigned long long)(n | (u64)(0x7fffffff - o)));
    atomicMax((unsigned long long*)(a.best_now + o), (unsigned long long)(n | (u64)(0x7fffffff - j)));
}

// current object o: bj(o) (-1: none), n(bj(o), o), and whether o is matched to it
struct TkMatch { int bj, n; bool matched; };
__device__ __forceinline__ TkMatch tk_match(const TrackArgs& a, int o, int kp) {
    TkMatch r{-1, 0, false};
    if (kp <= 0) return r;   // (nothing is associated: the best arrays are not even cleared on a fresh start)
    const u64 b = a.best_now[o];
    if (!b) return r;
    r.bj = 0x7fffffff - (int)(b & 0xffffffffull);
    r.n = (int)(b >> 32);
    const u64 p = a.best_prev[r.bj];
    r.matched = (0x7fffffff - (int)(p & 0xffffffffull)) == o && r.n >= a.min_overlap;
    return r;
}

__global__ void __launch_bounds__(TK_TPB) k_track_sums(TrackArgs a) {
    __shared__ int s_w[TK_WAVES];
    const int tile = (int)blockIdx.x, o = tile * FR_TILE + (int)threadIdx.x;
    const int sel = o < tk_k_now(a) && !tk_match(a, o, tk_k_prev(a)).matched ? 1 : 0;
    int total;
    (void)block_incl_scan_i<TK_WAVES>(sel, s_w, total);
    if (threadIdx.x == 0) a.tile_sum[tile] = total;
}

// ONE workgroup: the tile sums -> exclusive bases, chunk by chunk with a carry; counts[2] = the born
__global__ void __launch_bounds__(TK_TPB) k_track_scan(TrackArgs a, int n_tiles) {
    __shared__ int s_w[TK_WAVES];
    long long carry = 0;
    for (int base = 0; base < n_tiles; base += TK_TPB) {   // (uniform trip count)
        const int i = base + (int)threadIdx.x;
        const int v = i < n_tiles ? a.tile_sum[i] : 0;
        int total;
        const int inc = block_incl_scan_i<TK_WAVES>(v, s_w, total);
        if (i < n_tiles) a.tile_sum[i] = (int)carry + inc - v;
        carry += total;
    }
    if (threadIdx.x == 0) a.counts[2] = carry;
}

__global__ void __launch_bounds__(TK_TPB) k_track_emit(TrackArgs a) {
    __shared__ int s_w[TK_WAVES];
    const int tile = (int)blockIdx.x, o = tile * FR_TILE + (int)threadIdx.x;
    const int kp = tk_k_prev(a);
    const bool in = o < tk_k_now(a);
    TkMatch mt{-1, 0, false};
    if (in) mt = tk_match(a, o, kp);
    const int sel = in && !mt.matched ? 1 : 0;
    int total;
    const int rank = a.tile_sum[tile] + block_incl_scan_i<TK_WAVES>(sel, s_w, total) - sel;
    if (!in || a.counts[TRK_FAULT] != 0) return;   // (a void update writes no record)
    dspmap_track t;
    if (mt.matched) {
        const dspmap_track pt = a.p_tracks[mt.bj];
        const dspmap_object po = a.p_objects[mt.bj];
        const int4 s = a.shift[mt.bj];
        t.id = pt.id; t.parent = pt.parent; t.born_seq = pt.born_seq; t.age = pt.age + 1;
        t.prev_ordinal = mt.bj; t.overlap = mt.n;
        t.shift_x = s.x; t.shift_y = s.y; t.shift_z = s.z;
        t.prev_count = po.count;
        t.prev_sum_x = po.sum_x - (long long)po.count * a.dk0[0];
        t.prev_sum_y = po.sum_y - (long long)po.count * a.dk0[1];
        t.prev_sum_z = po.sum_z - (long long)po.count * a.dk0[2];
    } else {
        t.id = a.counts[TRK_NEXT] + rank;
        t.parent = mt.bj >= 0 ? a.p_tracks[mt.bj].id : -1;
        t.born_seq = a.seq; t.age = 0;
        t.prev_ordinal = -1; t.overlap = mt.n;
        t.shift_x = t.shift_y = t.shift_z = 0;
        t.prev_count = 0;
        t.prev_sum_x = t.prev_sum_y = t.prev_sum_z = 0;
    }
    a.tracks[o] = t;
}

// one thread, behind everything that reads the stored state: the counts, and what the NEXT update finds
__global__ void k_track_keep(TrackArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long* c = a.counts;
    if (c[TRK_FAULT] != 0) {   // the pair table was full: no tracks, the stored state emptied, next_id as it was
        c[0] = c[1] = c[2] = c[3] = c[4] = 0;
        c[5] = c[TRK_NEXT];
        c[TRK_KEPT] = 0;
        return;
    }
    const long long kn = tk_k_now(a), born = c[2], matched = kn - born;
    c[0] = kn; c[1] = matched;
    c[3] = c[TRK_KEPT] - matched;   // (on a fresh start nothing matched: every stored track ends)
    c[5] = c[TRK_NEXT] + born;
    c[TRK_NEXT] = c[5];
    c[TRK_KEPT] = kn;
}

void launch_track(const LaunchCtx& c, const TrackArgs& a) {
    const MapDims& d = c.d;
    const int n_items = (int)grid_layer_words(d);
    const int n_tiles = frontier_tiles(a.cap);
    const dim3 tpb(TK_TPB), words((unsigned)((n_items + TK_WAVES - 1) / TK_WAVES)), recs((unsigned)n_tiles);
    if (!a.fresh) {
        hipLaunchKernelGGL(k_track_shift, recs, tpb, 0, c.stream, d, a);
        if (a.per_cell) hipLaunchKernelGGL(k_track_pairs<true>, words, tpb, 0, c.stream, d, a, n_items);
        else hipLaunchKernelGGL(k_track_pairs<false>, words, tpb, 0, c.stream, d, a, n_items);
        hipLaunchKernelGGL(k_track_best, dim3((unsigned)((a.slots + TK_TPB - 1) / TK_TPB)), tpb, 0, c.stream, a);
    }
    hipLaunchKernelGGL(k_track_sums, recs, tpb, 0, c.stream, a);
    hipLaunchKernelGGL(k_track_scan, dim3(1), tpb, 0, c.stream, a, n_tiles);
    hipLaunchKernelGGL(k_track_emit, recs, tpb, 0, c.stream, a);
    hipLaunchKernelGGL(k_track_keep, dim3(1), dim3(64), 0, c.stream, a);
}
