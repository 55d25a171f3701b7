// dspmap_reach.hip -- arrival-time fields: a space-time wavefront through the cast grid (dspmap_build_reach_fields*, dspmap_reach_paths*;
// semantics next to them in include/dspmap.h).  The reference has no counterpart: a planner that asks "which cells can I reach through
// the predicted occupancy, and how early?" copies the grid out (getOccupancyMapWithFutureStatus :405-426) and runs a BFS on the host.
//
// The work: step n of a field is R_n = (R_{n-1} u N6(R_{n-1})) \ B_n on one bit per voxel -- per 64-bit word of a row a shift left, a shift
// right, two carry bits out of the row's neighbouring words, four ORs with the words at y +- 1 and z +- 1, one and-not with the blocked
// word of the step's layer.  The steps of a field are strictly sequential (up to 4096 of them), a step touches nz * ny * W words (960 on a
// 40 x 40 x 24 map, 5 280 on 66 x 66 x 40, 23 760 on 132 x 132 x 60), and the fields of a batch are independent.
//
// Chosen: ONE WORKGROUP OF 1024 THREADS PER FIELD runs every step of its field in ONE launch; the batch of fields supplies the CUs.  A
// thread owns the words t = tid, tid + 1024, ... of the set for the whole run.  The two sets (R_{n-1}, R_n) ping-pong in LDS whenever
// 2 * nz * ny * W * 8 bytes fit REACH_LDS_BYTES (dynamic shared memory, raised to the CU's 160 KiB by hipFuncSetAttribute as
// dspmap_sweep.hip does for k_rollout): 84 KB on 66 x 66 x 40.  Larger maps keep them in per-field device scratch instead, which one
// workgroup re-reads every step and which therefore stays in L2; the code is the same template, and because a workgroup runs on one CU
// the workgroup-scope ordering of __syncthreads() is all the two storages need.  Per step and word: seven reads of the old set, and ONLY
// IF the grown word is non-zero one or two loads of the blocked words through L2 (the layer changes with n, so they are not cached in
// LDS); the front is a thin shell, so most words of most steps stop at the seven reads.  The cells that are new in R_n (grown & ~old: the
// front, not the volume) are walked bit by bit and the value n is stored where the field still reads 65535 -- a cell that was removed
// and comes back keeps its first arrival.  The owner of a word is the only thread that ever reads or writes its 64 values, so that test
// needs no atomic.  ONE barrier per step: the step's verdict {changed, non-empty} is ORed into one of three rotating LDS flags before
// the barrier and read behind it; the flag of step n + 1 is cleared by thread 0 before the barrier of step n, when its last readers
// (step n - 2) are provably past.  The loop leaves early when the set is empty (it stays empty) or when a step changed nothing and the
// schedule has reached its last layer (n >= n_fix, walked once on the host): every later step would repeat it.  That is invisible in
// the result.  Sources are ORed into R with atomics before step 0, every thread scanning a stride of the batch's sources for its field.
// Every loop is bounded by max_steps, the word count or the source count; nothing waits on another workgroup.
//
// The timeline build (dspmap_build_reach_timeline*) is the same launch with KEEP: every step's set also goes to a dense row of device
// memory, one more word store per word and step, and k_reach_timeline_paths walks backwards through the rows in a launch of its own.
// Dense rows against compacting the non-zero words (a count across the workgroup per step, a search per load of the walk) and against
// re-running the wavefront per path: DESIGN.md, "Space-time paths".
//
// Rejected:
//  - one launch per step over all fields (the textbook level-synchronous BFS): up to 4096 launches of a few microseconds of work each, and
//    the early exit would need a read-back per step.  A serpentine maze of 700 steps would cost 700 launch gaps.
//  - several workgroups per field with a grid-wide barrier or flags in memory between them: a spin on memory another workgroup writes
//    deadlocks as soon as the workgroups are not all resident, and a hung kernel takes the device from everyone.  Very large maps pay
//    with one CU per field instead (out of scope: more than one workgroup per field).
//  - a third set "ever reached" in LDS to avoid the uint16 re-read: 126 KB instead of 84 KB on 66 x 66 x 40 and it would push
//    maps between 107 and 160 KB out of LDS; the re-read is per FRONT bit, each of which is written at most a few times in a run.
//  - a lane per cell and uint16 distances relaxed in place (Bellman-Ford style): 64 times the LDS of a bit set, so only toy maps would
//    fit, and the blocked test becomes a bit extract per cell and step instead of one and-not per 64 cells.
//  - keeping the blocked words of the tested layer in LDS: the layer changes with n in the scheduled case, and in the static case the
//    and-not is already skipped for every word the front does not touch.
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"

#define REACH_TPB 1024
#define REACH_PATH_TPB 256

// the layer step n tests besides (with_current) layer 0
__device__ __forceinline__ int reach_layer(const MapDims& d, const ReachArgs& a, int n) {
    if (!a.timed) return 0;
    return q_horizon(d, __fadd_rn(a.t_start, __fmul_rn((float)n, a.step_seconds))) + 1;
}

// KEEP (dspmap_build_reach_timeline): the owner of word t also stores R_n's word to row n of its field's history, hist[(f * (max_steps + 1)
// + n) * nwords + t] -- in step 0 and in every later step, zero words too, because nothing clears the rows -- and thread 0 leaves the last
// step executed in last[f].  The history is write-only inside the launch (k_reach_timeline_paths reads it behind the kernel boundary), so
// the one barrier per step and its flag rotation are those of the plain build.  hist and last follow src in the argument list so that the
// KEEP = false instantiations read their arguments where they always did.
template <bool LDS, bool KEEP>
__global__ void __launch_bounds__(REACH_TPB) k_reach(MapDims d, ReachArgs a, const float4* __restrict__ src, u64* __restrict__ hist,
                                                     int* __restrict__ last) {
    extern __shared__ u64 s_reach[];
    __shared__ int s_flag[3];   // bit 0: the step changed the set, bit 1: the set is not empty
    const unsigned tid = threadIdx.x, f = blockIdx.x;
    const GridWords gw(d);
    const unsigned W = gw.W, plane = gw.plane, nwords = gw.nwords;
    u64* set = LDS ? s_reach : a.sets + (size_t)f * 2 * nwords;
    unsigned short* fld = a.field + (size_t)f * d.v_glob;
    const u64* __restrict__ bits = a.bits;
    const u64 row_mask = grid_row_mask(d);                                    // bits at x >= nx are never reached
    unsigned co = 0, no = nwords;                                             // R_{n-1} at set[co ..], R_n at set[no ..]
    u64* row = KEEP ? hist + (size_t)f * ((size_t)a.max_steps + 1) * nwords : nullptr;   // row n of this field's history, from row 0 on
    int done = a.max_steps;                                                   // (KEEP) the last step executed

    for (unsigned t = tid; t < nwords; t += REACH_TPB) set[co + t] = 0;
    if (tid < 3) s_flag[tid] = 0;
    __syncthreads();
    for (unsigned i = tid; i < (unsigned)a.n_src; i += REACH_TPB) {
        const float4 p = src[i];
        if ((unsigned)__float_as_int(p.w) != f) continue;   // (a field outside [0, n_fields) matches no workgroup)
        int x, y, z;
        if (grid_cell(d, a.org, p.x, p.y, p.z, x, y, z) != 0) continue;
        atomicOr((unsigned long long*)&set[co + gw.word_of(d, x, y, z)], GridWords::bit_of(x));
    }
    __syncthreads();
    {   // step 0: R_0 = S \ B_0, in place (a thread touches its own words only)
        const int l = reach_layer(d, a, 0);
        for (unsigned t = tid; t < nwords; t += REACH_TPB) {
            u64 v = set[co + t];
            if (KEEP && !v) row[t] = 0;
            if (!v) continue;
            u64 b = bits[(size_t)l * nwords + t];
            if (a.with_current && l > 0) b |= bits[t];
            v &= ~b;
            set[co + t] = v;
            if (KEEP) row[t] = v;
            const unsigned yz = t / W, w = t - yz * W;
            grid_store_bits(fld + (size_t)yz * d.nx + w * 64, v, 0);
        }
    }
    __syncthreads();
    for (int n = 1; n <= a.max_steps; ++n) {
        const int l = reach_layer(d, a, n);
        int verdict = 0;
        if (KEEP) row += nwords;
        for (unsigned t = tid; t < nwords; t += REACH_TPB) {
            const unsigned z = t / plane, r = t - z * plane, y = r / W, w = r - y * W;
            const u64* cur = set + co + t;
            const u64 c = cur[0];
            u64 g = grid_grow6<true>(cur, c, w, y, z, gw, d);
            if (w + 1 == W) g &= row_mask;
            if (g) {
                u64 b = bits[(size_t)l * nwords + t];
                if (a.with_current && l > 0) b |= bits[t];
                g &= ~b;
            }
            set[no + t] = g;
            if (KEEP) row[t] = g;
            verdict |= (g != c ? 1 : 0) | (g ? 2 : 0);
            const u64 fresh = g & ~c;                  // the front: cells of R_n that R_{n-1} did not hold
            if (fresh)                                 // (a cell that comes back keeps its first arrival)
                grid_store_bits<true>(fld + (size_t)(t / W) * d.nx + w * 64, fresh, (unsigned short)n, DSPMAP_REACH_UNREACHED);
        }
        if (verdict) atomicOr(&s_flag[n % 3], verdict);
        if (tid == 0) s_flag[(n + 1) % 3] = 0;         // (its last readers, those of step n - 2, are past the barrier of step n - 1)
        __syncthreads();
        const int v = s_flag[n % 3];
        const unsigned tmp = co; co = no; no = tmp;
        if (KEEP) done = n;
        if (!(v & 2)) break;                           // an empty set stays empty
        if (!(v & 1) && n >= a.n_fix) break;           // nothing changed and the layer never changes again: every later step repeats this one
    }
    if (KEEP && tid == 0) last[f] = done;              // rows (done, max_steps] are never written: R_n = R_done there, for both exits
}

static_assert(DSPMAP_COST_UNREACHED == DSPMAP_REACH_UNREACHED, "the paths of both kinds of field read one marker");
// the head of every path: the start's field f and cell (x, y, z), the value v it reads there, and the path's status word -- v, -1 for an
// unreached cell, -2 outside the map, -3 for a non-finite coordinate or a field outside [0, n_fields) (either wins over "outside")
__device__ __forceinline__ int path_head(const MapDims& d, const SampleOrigin& org, int n_fields, const unsigned short* __restrict__ field, float4 p,
                                         int& f, int& x, int& y, int& z, int& v) {
    f = __float_as_int(p.w);
    x = y = z = v = 0;
    int st = grid_cell(d, org, p.x, p.y, p.z, x, y, z);
    if ((unsigned)f >= (unsigned)n_fields) st = -3;
    if (st == 0) {
        v = field[(size_t)f * d.v_glob + ((size_t)z * d.ny + y) * d.nx + x];
        st = v == DSPMAP_REACH_UNREACHED ? -1 : v;
    }
    return st;
}
// ... and its tail: the cells behind the path's last one read -1
__device__ __forceinline__ void path_tail(int* out, int j, int max_len) {
    for (; j < max_len; ++j) out[j] = -1;
}

// one lane per start: the steepest descent through a time-invariant field, first neighbour of the wanted value in the order -x, +x, -y, +y,
// -z, +z.  The wanted value is v - 1 in an arrival field and, WEIGHTED, v - weight[g] in a cost field: the weight of the cell left
template <bool WEIGHTED>
__global__ void __launch_bounds__(REACH_PATH_TPB) k_field_paths(MapDims d, FieldPathArgs a, int n, const float4* __restrict__ start,
                                                                int* __restrict__ steps_out, int* __restrict__ cells_out) {
    const unsigned i = blockIdx.x * REACH_PATH_TPB + threadIdx.x;
    if (i >= (unsigned)n) return;
    int f, x, y, z, v;
    const int st = path_head(d, a.org, a.n_fields, a.field, start[i], f, x, y, z, v);
    steps_out[i] = st;
    int* out = cells_out + (size_t)i * a.max_len;
    int j = 0;
    if (st >= 0) {
        const unsigned short* __restrict__ fld = a.field + (size_t)f * d.v_glob;
        const int sy = d.nx, sz = d.nx * d.ny;
        int g = (z * d.ny + y) * d.nx + x;
        for (; j < a.max_len;) {                       // (bounded by max_len; v falls by at least one per cell)
            out[j++] = g;
            if (v == 0) break;
            const int want = v - (WEIGHTED ? (int)a.weight[g] : 1);
            // the six neighbour loads of a step are issued together: independent addresses, one wait
            const bool ok[6] = {x > 0, x + 1 < d.nx, y > 0, y + 1 < d.ny, z > 0, z + 1 < d.nz};
            const int off[6] = {-1, 1, -sy, sy, -sz, sz};
            int nv[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) nv[k] = fld[g + (ok[k] ? off[k] : 0)];
            int pick = -1;
#pragma unroll
            for (int k = 5; k >= 0; --k)
                if (ok[k] && nv[k] == want) pick = k;
            if (pick < 0) break;                       // no such neighbour (never in a field the build made, time-invariant for arrivals): stop
            g += off[pick];
            x += pick == 1 ? 1 : (pick == 0 ? -1 : 0);
            y += pick == 3 ? 1 : (pick == 2 ? -1 : 0);
            z += pick == 5 ? 1 : (pick == 4 ? -1 : 0);
            v = want;
        }
    }
    path_tail(out, j, a.max_len);
}

// one lane per start: backwards through the sets a timeline build kept.  The cell at step s > 0 came from R_{s-1}: it waits where it is if
// it is in that set, else it moves to the first face neighbour in the order -x, +x, -y, +y, -z, +z that is (one exists, because
// R_s is a subset of R_{s-1} u N6(R_{s-1})).  Every loop is bounded by max_len and by the value, which falls by one per cell.
__global__ void __launch_bounds__(REACH_PATH_TPB) k_reach_timeline_paths(MapDims d, ReachTimelinePathArgs a, int n, const float4* __restrict__ start,
                                                                         int* __restrict__ steps_out, int* __restrict__ cells_out) {
    const unsigned i = blockIdx.x * REACH_PATH_TPB + threadIdx.x;
    if (i >= (unsigned)n) return;
    int f, x, y, z, v;
    const int st = path_head(d, a.org, a.n_fields, a.field, start[i], f, x, y, z, v);
    steps_out[i] = st;
    int* out = cells_out + (size_t)i * a.max_len;
    int j = 0;
    if (st >= 0) {
        const unsigned W = grid_row_words(d);
        const size_t nwords = grid_layer_words(d);
        const u64* __restrict__ rows = a.hist + (size_t)f * ((size_t)a.max_steps + 1) * nwords;
        const int lastf = a.last[f];
        for (; j < a.max_len;) {                       // (bounded by max_len; v falls by one per cell)
            out[j++] = (z * d.ny + y) * d.nx + x;
            if (v == 0) break;
            const u64* __restrict__ P = rows + (size_t)min(v - 1, lastf) * nwords;   // R_{v-1} (a step behind the last one executed repeats it)
            // the seven bit loads of a step are issued together: the own cell, then the six neighbours; independent addresses, one wait
            const bool ok[7] = {true, x > 0, x + 1 < d.nx, y > 0, y + 1 < d.ny, z > 0, z + 1 < d.nz};
            const int dx[7] = {0, -1, 1, 0, 0, 0, 0}, dy[7] = {0, 0, 0, -1, 1, 0, 0}, dz[7] = {0, 0, 0, 0, 0, -1, 1};
            u64 wv[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const int cx = ok[k] ? x + dx[k] : x, cy = ok[k] ? y + dy[k] : y, cz = ok[k] ? z + dz[k] : z;
                wv[k] = P[((size_t)cz * d.ny + cy) * W + ((unsigned)cx >> 6)];
            }
            int pick = -1;
#pragma unroll
            for (int k = 6; k >= 0; --k)
                if (ok[k] && ((wv[k] >> ((x + dx[k]) & 63)) & 1)) pick = k;
            if (pick < 0) break;                       // neither the cell nor a neighbour (never, see above): stop, the rest is -1
            x += dx[pick]; y += dy[pick]; z += dz[pick];
            --v;
        }
    }
    path_tail(out, j, a.max_len);
}

void reach_init_device() {   // per device, once (dspmap_init_device)
    (void)hipFuncSetAttribute((const void*)k_reach<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, REACH_LDS_BYTES);
    (void)hipFuncSetAttribute((const void*)k_reach<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, REACH_LDS_BYTES);
}

// hist != nullptr: the timeline build -- every step's set goes to hist, the last step executed per field to last
void launch_reach(const LaunchCtx& c, const ReachArgs& a, const dspmap_reach_point* src, u64* hist, int* last) {
    if (a.n_fields <= 0) return;
    const MapDims& d = c.d;
    const size_t set_bytes = 2 * sizeof(u64) * grid_layer_words(d);
    const dim3 grid(a.n_fields), block(REACH_TPB);
    if (a.sets && hist)
        hipLaunchKernelGGL((k_reach<false, true>), grid, block, 0, c.stream, d, a, (const float4*)src, hist, last);
    else if (a.sets)
        hipLaunchKernelGGL((k_reach<false, false>), grid, block, 0, c.stream, d, a, (const float4*)src, hist, last);
    else if (hist)
        hipLaunchKernelGGL((k_reach<true, true>), grid, block, set_bytes, c.stream, d, a, (const float4*)src, hist, last);
    else
        hipLaunchKernelGGL((k_reach<true, false>), grid, block, set_bytes, c.stream, d, a, (const float4*)src, hist, last);
}

void launch_field_paths(const LaunchCtx& c, const FieldPathArgs& a, bool weighted, int n, const dspmap_reach_point* start, int* steps_out, int* cells_out) {
    if (n <= 0) return;
    const dim3 grid((unsigned)(((long long)n + REACH_PATH_TPB - 1) / REACH_PATH_TPB)), block(REACH_PATH_TPB);
    if (weighted) hipLaunchKernelGGL(k_field_paths<true>, grid, block, 0, c.stream, c.d, a, n, (const float4*)start, steps_out, cells_out);
    else hipLaunchKernelGGL(k_field_paths<false>, grid, block, 0, c.stream, c.d, a, n, (const float4*)start, steps_out, cells_out);
}

void launch_reach_timeline_paths(const LaunchCtx& c, const ReachTimelinePathArgs& a, int n, const dspmap_reach_point* start, int* steps_out,
                                 int* cells_out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_reach_timeline_paths, dim3((unsigned)(((long long)n + REACH_PATH_TPB - 1) / REACH_PATH_TPB)), dim3(REACH_PATH_TPB), 0,
                       c.stream, c.d, a, n, (const float4*)start, steps_out, cells_out);
}
