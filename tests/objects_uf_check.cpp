// objects_uf_check.cpp -- the labelling core of dspmap_build_objects (dsp-map_amd/csrc/dspmap_unionfind.h) on the host: the same uf_find /
// uf_unite the kernels call, with a compare-exchange loop behind atomic_min.  Every scene file given on the command line is labelled
//   - sequentially, visiting the set cells in several shuffled orders, and
//   - from 8 std::threads that share the cells of one shuffled order,
// and each labelling is compared cell for cell with the expected labels in the file.  Built with -fsanitize=address,undefined and with
// -fsanitize=thread (tests/test_objects_cpu.py).
// File: int32 {nx, ny, nz, connectivity}, nx * ny * nz bytes of occupancy in voxel order, nx * ny * nz int32 expected labels (-1 = clear).
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <random>
#include <thread>
#include <vector>

#include "../dsp-map_amd/csrc/dspmap_unionfind.h"

struct HostLabels {
    std::atomic<int>* L;
    int load(int i) const { return L[i].load(std::memory_order_relaxed); }
    int atomic_min(int i, int v) const {   // returns the old value; the stored value only ever goes down, so the loop ends
        int cur = L[i].load(std::memory_order_relaxed);
        while (cur > v && !L[i].compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
        return cur;
    }
};

struct Scene {
    int nx = 0, ny = 0, nz = 0, conn = 0;
    std::vector<uint8_t> occ;
    std::vector<int32_t> want;
    int V() const { return nx * ny * nz; }
};

static bool read_scene(const char* path, Scene* s) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    int32_t h[4];
    bool ok = fread(h, sizeof(int32_t), 4, f) == 4;
    if (ok) {
        s->nx = h[0]; s->ny = h[1]; s->nz = h[2]; s->conn = h[3];
        ok = s->nx > 0 && s->ny > 0 && s->nz > 0 && (s->conn == 6 || s->conn == 26) && (long long)s->nx * s->ny * s->nz < (1 << 24);
    }
    if (ok) {
        s->occ.resize((size_t)s->V());
        s->want.resize((size_t)s->V());
        ok = fread(s->occ.data(), 1, s->occ.size(), f) == s->occ.size() && fread(s->want.data(), sizeof(int32_t), s->want.size(), f) == s->want.size();
    }
    fclose(f);
    return ok;
}

// k_objects_init: a set cell starts at the first cell of its run of set cells along x (here over the whole row), a clear cell at -1
static void init_labels(const Scene& s, std::atomic<int>* L) {
    for (int row = 0; row < s.ny * s.nz; ++row) {
        int start = -1;
        for (int x = 0; x < s.nx; ++x) {
            const int g = row * s.nx + x;
            if (!s.occ[(size_t)g]) { start = -1; L[g].store(-1, std::memory_order_relaxed); continue; }
            if (start < 0) start = g;
            L[g].store(start, std::memory_order_relaxed);
        }
    }
}

// k_objects_merge for one cell: unite with the set cells of the lower half of its neighbourhood; ORs the fault codes
static int merge_cell(const Scene& s, HostLabels& m, int g) {
    const int x = g % s.nx, y = (g / s.nx) % s.ny, z = g / (s.nx * s.ny);
    int fault = UF_OK;
    for (int dz = -1; dz <= 0; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (dz == 0 && (dy > 0 || (dy == 0 && dx >= 0))) continue;                    // the lower half only
                if (s.conn == 6 && (dz != 0) + (dy != 0) + (dx != 0) != 1) continue;
                const int xx = x + dx, yy = y + dy, zz = z + dz;
                if (xx < 0 || xx >= s.nx || yy < 0 || yy >= s.ny || zz < 0) continue;         // outside the map: does not exist
                const int ng = (zz * s.ny + yy) * s.nx + xx;
                if (s.occ[(size_t)ng]) fault |= uf_unite(m, g, ng, s.V());
            }
    return fault;
}

// k_objects_flatten, then the comparison; returns the number of differing cells (or -1 after a fault)
static long long flatten_and_compare(const Scene& s, HostLabels& m, int fault, const char* what) {
    if (fault) { printf("FAULT %d in %s\n", fault, what); return -1; }
    long long bad = 0;
    for (int g = 0; g < s.V(); ++g) {
        int got = -1;
        if (s.occ[(size_t)g]) got = uf_find(m, g, s.V(), &fault);
        if (got != s.want[(size_t)g] && bad++ < 5) printf("%s: cell %d labelled %d, expected %d\n", what, g, got, s.want[(size_t)g]);
    }
    if (fault) { printf("FAULT %d flattening %s\n", fault, what); return -1; }
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: %s scene.bin ...\n", argv[0]); return 2; }
    const int n_threads = 8, n_orders = 4;
    for (int a = 1; a < argc; ++a) {
        Scene s;
        if (!read_scene(argv[a], &s)) { printf("cannot read %s\n", argv[a]); return 2; }
        std::vector<int> cells;
        for (int g = 0; g < s.V(); ++g) if (s.occ[(size_t)g]) cells.push_back(g);
        std::vector<std::atomic<int>> L((size_t)s.V());
        HostLabels m{L.data()};
        std::mt19937 rng(12345u + (unsigned)a);
        for (int o = 0; o < n_orders; ++o) {   // order 0: ascending; then shuffled
            if (o) std::shuffle(cells.begin(), cells.end(), rng);
            init_labels(s, L.data());
            int fault = UF_OK;
            for (int g : cells) fault |= merge_cell(s, m, g);
            if (flatten_and_compare(s, m, fault, "sequential") != 0) return 1;
            init_labels(s, L.data());
            std::vector<int> faults((size_t)n_threads, UF_OK);
            std::vector<std::thread> pool;
            for (int t = 0; t < n_threads; ++t)
                pool.emplace_back([&, t] {
                    for (size_t i = (size_t)t; i < cells.size(); i += (size_t)n_threads) faults[(size_t)t] |= merge_cell(s, m, cells[i]);
                });
            for (auto& th : pool) th.join();
            fault = UF_OK;
            for (int f : faults) fault |= f;
            if (flatten_and_compare(s, m, fault, "threads") != 0) return 1;
        }
        printf("OK %s: %d x %d x %d, connectivity %d, %zu cells, %d orders sequential and from %d threads\n", argv[a], s.nx, s.ny, s.nz, s.conn,
               cells.size(), n_orders, n_threads);
    }
    return 0;
}
