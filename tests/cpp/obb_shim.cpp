// Oriented-box queries from C++: hagrid::overlap_obbs of include/hagrid/traverse.h over a grid built through the headers, compiled as plain C++ (-DHOST=
// -DDEVICE=) and linked with libhagrid_amd.so.  Verifies ids and counts against obb_brute_force of include/hagrid/obb.h on the host: sheared boxes around
// triangles of the scene, with body labels and without.  usage: obb_shim [triangles] [queries]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hagrid/build.h"
#include "hagrid/mem_manager.h"
#include "hagrid/obb.h"
#include "hagrid/traverse.h"

using namespace hagrid;
namespace ho = hagrid::overlap;
namespace hb = hagrid::obb;

static uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
static float rnd(uint64_t seed, uint64_t i) { return float(mix(seed + (i + 1) * 0x9E3779B97F4A7C15ull) >> 40) * (1.0f / 16777216.0f); }

typedef ho::IdList<ho::kMaxIds> List;

struct Query {
    const hb::ObbRecord* rec;
    const int* label_;
    const int* tri_labels_;
    hb::Obb box() const { return hb::from_record(*rec); }
    bool labelled() const { return label_ != nullptr; }
    int label() const { return *label_; }
    int tri_label(int id, int i) const { return tri_labels_[3 * size_t(id) + i]; }
};

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 20000, nq = argc > 2 ? atoi(argv[2]) : 1000;
    if (nq > n) { fprintf(stderr, "at most as many queries as triangles\n"); return 2; }
    std::vector<Tri> host_tris(n);
    const float s = 2.0f / cbrtf(float(n));
    for (int i = 0; i < n; i++) {
        vec3 c(rnd(1, 9 * i), rnd(1, 9 * i + 1), rnd(1, 9 * i + 2));
        vec3 a = (2.0f * vec3(rnd(1, 9 * i + 3), rnd(1, 9 * i + 4), rnd(1, 9 * i + 5)) - vec3(1.0f)) * s;
        vec3 b = (2.0f * vec3(rnd(1, 9 * i + 6), rnd(1, 9 * i + 7), rnd(1, 9 * i + 8)) - vec3(1.0f)) * s;
        vec3 v0 = c, v1 = c + a, v2 = c + b, e1 = v0 - v1, e2 = v2 - v0, nn = cross(e1, e2);
        host_tris[i] = Tri(v0, nn.x, e1, nn.y, e2, nn.z);
    }
    // labels: a body of four consecutive triangles each.  Box i: centred on a vertex of triangle i, two axes along the triangle's edges (doubled), the
    // third a random lean -- a sheared frame; its label is the body of triangle i
    std::vector<int> host_labels(size_t(n) * 3, -1), host_qlabels(nq);
    for (int i = 0; i < n; i++) host_labels[size_t(i) * 3 + (i % 3)] = i / 4;
    std::vector<hb::ObbRecord> host_obbs(nq);
    for (int i = 0; i < nq; i++) {
        const Tri& t = host_tris[i];
        hb::ObbRecord r = {};
        r.c[0] = t.v0.x; r.c[1] = t.v0.y; r.c[2] = t.v0.z;
        r.u[0] = 2.0f * t.e1.x; r.u[1] = 2.0f * t.e1.y; r.u[2] = 2.0f * t.e1.z;
        r.v[0] = 2.0f * t.e2.x; r.v[1] = 2.0f * t.e2.y; r.v[2] = 2.0f * t.e2.z;
        r.w[0] = (2.0f * rnd(2, 3 * i) - 1.0f) * s; r.w[1] = (2.0f * rnd(2, 3 * i + 1) - 1.0f) * s; r.w[2] = (2.0f * rnd(2, 3 * i + 2) - 1.0f) * s;
        r.first = i % 5 == 4 ? i : 0;
        host_obbs[i] = r;
        host_qlabels[i] = i / 4;
    }
    MemManager mem(true);
    auto tris = mem.alloc<Tri>(host_tris.size());
    mem.copy<Copy::HST_TO_DEV>(tris, host_tris.data(), host_tris.size());
    hb::ObbRecord* obbs = mem.alloc<hb::ObbRecord>(nq);
    mem.copy<Copy::HST_TO_DEV>(obbs, host_obbs.data(), host_obbs.size());
    int* labels = mem.alloc<int>(host_labels.size());
    mem.copy<Copy::HST_TO_DEV>(labels, host_labels.data(), host_labels.size());
    int* qlabels = mem.alloc<int>(nq);
    mem.copy<Copy::HST_TO_DEV>(qlabels, host_qlabels.data(), host_qlabels.size());
    Grid grid;
    grid.entries = nullptr; grid.cells = nullptr; grid.ref_ids = nullptr; grid.small_cells = nullptr;
    build_grid(mem, tris, n, grid, 0.12f, 2.4f);
    merge_grid(mem, grid, 0.995f);
    flatten_grid(mem, grid);
    expand_grid(mem, grid, tris, 3);
    ho::Clip clip;
    clip.set(grid.bbox.min, grid.bbox.max);
    const float eps = ho::GridConsts::abs_margin(grid.bbox.min, grid.bbox.max);

    int* ids = mem.alloc<int>(size_t(nq) * ho::kMaxIds);
    int* counts = mem.alloc<int>(nq);
    std::vector<int> h_ids(size_t(nq) * ho::kMaxIds), h_counts(nq);
    int bad = 0, found = 0;
    const Tri* t = host_tris.data();
    for (int pass = 0; pass < 4; pass++) {
        const bool lab = pass < 2;
        const int k = pass % 2 == 0 ? 8 : 3;
        if (lab) overlap_obbs(grid, tris, obbs, nq, k, ids, counts, nullptr, false, qlabels, labels);
        else     overlap_obbs(grid, tris, obbs, nq, k, ids, counts);
        mem.copy<Copy::DEV_TO_HST>(h_ids.data(), ids, size_t(nq) * k);
        mem.copy<Copy::DEV_TO_HST>(h_counts.data(), counts, nq);
        for (int i = 0; i < nq; i++) {
            List l;
            l.init(k, host_obbs[i].first);
            Query q;
            q.rec = &host_obbs[i]; q.label_ = lab ? &host_qlabels[i] : nullptr; q.tri_labels_ = host_labels.data();
            hb::obb_brute_force([t](int j) { return t[j]; }, n, clip, eps, q, false, l);
            int wrong = h_counts[i] != l.count() ? 1 : 0;
            for (int j = 0; j < k; j++) wrong += h_ids[size_t(i) * k + j] != l.id[j] ? 1 : 0;
            bad += wrong ? 1 : 0;
            found += l.found() ? 1 : 0;
        }
    }
    printf("%d queries, %d answers with a triangle, %d mismatches vs host brute force\n", nq, found, bad);
    mem.free(ids); mem.free(counts); mem.free(qlabels); mem.free(labels); mem.free(obbs);
    mem.free(grid.entries); mem.free(grid.cells); mem.free(grid.ref_ids); mem.free(grid.small_cells); mem.free(tris);
    fflush(stdout);
    return bad == 0 && found > 0 ? 0 : 1;
}
