// obb_host -- the oriented-box queries of include/hagrid/obb.h on the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: the box / triangle
// test, the brute-force definition and the walk over the construction format that hagrid_amd/csrc/overlap.hip (obb_tris_kernel) runs on the device, with a
// switch that turns the float prune off.  tests/test_obb_cpu.py compares what this writes with hagrid_amd/scene.py and the fixture tests/golden/obb.npz,
// tests/test_obb_gpu.py with what the device wrote.
//
//   obb_host pairs PARAMS OBBS TRIS OUT               PARAMS: i32 n;  box OBBS[i] against triangle TRIS[i];  OUT: n i32 (1: they meet)
//   obb_host brute PARAMS TRIS OBBS QLABELS TLABELS IDS COUNTS
//                                                     PARAMS: i32 n, i32 k, i32 any, 3 f32 grid box min, 3 f32 grid box max;  every box against all triangles;
//                                                     IDS: n x k i32, COUNTS: n i32
//   obb_host walk  PARAMS ENTRIES CELLS REFS TRIS OBBS QLABELS TLABELS IDS COUNTS TOTALS
//                                                     PARAMS: the grid header (host_support.h), i32 n, i32 k, i32 any, i32 float_prune (0: the integer range
//                                                     prunes alone);  TOTALS: n x 3 i32 (cells visited, pairs offered to obb_meets, blocks pruned)
// OBBS: n records of 64 bytes.  QLABELS: n i32 and TLABELS: 3 i32 per triangle, or both empty (no labels).
#include <string>
#include <vector>

#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/grid.h"
#include "hagrid/obb.h"
#include "host_support.h"

using namespace hagrid;
using namespace host_support;
namespace ho = hagrid::overlap;
namespace hb = hagrid::obb;

namespace {

typedef ho::IdList<ho::kMaxIds> List;

static_assert(sizeof(hb::ObbRecord) == 64, "the record is 64 bytes");

// the accessor of overlap.h: the grid and the clip box
struct OverlapGrid : HostGrid<kEndUnbounded> { ho::Clip clip; };

// the query of obb.h's ObbFilter
struct HostQuery {
    const hb::ObbRecord* rec;
    const int32_t* label_;                  // of this query, or null
    const std::vector<int32_t>* tri_labels_;
    hb::Obb box() const { return hb::from_record(*rec); }
    bool labelled() const { return label_ != nullptr; }
    int label() const { return *label_; }
    int tri_label(int id, int i) const {
        const size_t at = 3 * size_t(id) + size_t(i);
        if (id < 0 || at >= tri_labels_->size()) { fprintf(stderr, "triangle id beyond the labels\n"); exit(2); }
        return (*tri_labels_)[at];
    }
};

// the batch as the files give it
struct Batch {
    std::vector<hb::ObbRecord> obbs;
    std::vector<int32_t> qlabels, tlabels;
    void load(int n, size_t num_tris, const char* q, const char* ql, const char* tl) {
        obbs = read_file<hb::ObbRecord>(q); qlabels = read_file<int32_t>(ql); tlabels = read_file<int32_t>(tl);
        if (int(obbs.size()) != n) { fprintf(stderr, "the box file does not hold n records\n"); exit(2); }
        if (qlabels.empty() != tlabels.empty()) { fprintf(stderr, "one label file without the other\n"); exit(2); }
        if (!qlabels.empty() && (qlabels.size() != size_t(n) || tlabels.size() != 3 * num_tris)) { fprintf(stderr, "the label files do not hold one label per box and three per triangle\n"); exit(2); }
    }
    HostQuery query(int i) const {
        HostQuery q;
        q.rec = &obbs[i]; q.label_ = qlabels.empty() ? nullptr : qlabels.data() + i; q.tri_labels_ = &tlabels;
        return q;
    }
};

void to_record(const List& l, int k, int32_t* ids, int32_t& count) {
    for (int j = 0; j < k; j++) ids[j] = l.id[j];
    count = l.count();
}

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: obb_host pairs|brute|walk PARAMS ... OUT\n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    if (op == "pairs" && argc == 6) {
        const int n = p.get<int32_t>();
        const std::vector<hb::ObbRecord> a = read_file<hb::ObbRecord>(argv[3]);
        const std::vector<Tri> b = read_file<Tri>(argv[4]);
        if (int(a.size()) != n || int(b.size()) != n) { fprintf(stderr, "pairs: the files do not hold n records\n"); return 2; }
        std::vector<int32_t> out(size_t(n), 0);
        for (int i = 0; i < n; i++) out[i] = hb::obb_meets(hb::from_record(a[i]), b[i]) ? 1 : 0;
        write_file(argv[5], out);
    } else if (op == "brute" && argc == 9) {
        const int n = p.get<int32_t>(), k = p.get<int32_t>(), any = p.get<int32_t>();
        const vec3 glo = p.get3(), ghi = p.get3();
        if (k < 1 || k > ho::kMaxIds || (any && k != 1)) { fprintf(stderr, "brute: bad k\n"); return 2; }
        ho::Clip clip;
        clip.set(glo, ghi);
        const float eps = ho::GridConsts::abs_margin(glo, ghi);
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        Batch batch;
        batch.load(n, tris.size(), argv[4], argv[5], argv[6]);
        std::vector<int32_t> ids(size_t(n) * k), counts((size_t(n)));
        const Tri* t = tris.data();
        for (int i = 0; i < n; i++) {
            List l;
            l.init(k, batch.obbs[i].first);
            hb::obb_brute_force([t](int j) { return t[j]; }, int(tris.size()), clip, eps, batch.query(i), any != 0, l);
            to_record(l, k, ids.data() + size_t(i) * k, counts[i]);
        }
        write_file(argv[7], ids);
        write_file(argv[8], counts);
    } else if (op == "walk" && argc == 13) {
        const GridHeader h = p.get_grid_header();
        const int n = p.get<int32_t>(), k = p.get<int32_t>(), any = p.get<int32_t>(), float_prune = p.get<int32_t>();
        if (k < 1 || k > ho::kMaxIds || (any && k != 1)) { fprintf(stderr, "walk: bad k\n"); return 2; }
        OverlapGrid g;
        g.load(h, argv[3], argv[4], argv[5]);
        g.clip.set(h.lo, h.hi);
        g.tris = read_file<Tri>(argv[6]);
        Batch batch;
        batch.load(n, g.tris.size(), argv[7], argv[8], argv[9]);
        std::vector<int32_t> ids(size_t(n) * k), counts((size_t(n))), totals(size_t(n) * 3);
        ho::ArrayStack<ho::kMaxLevels> st;
        for (int i = 0; i < n; i++) {
            List l;
            l.init(k, batch.obbs[i].first);
            ho::Counts c;
            hb::obb_query(g, st, batch.query(i), any != 0, l, c, float_prune != 0);
            to_record(l, k, ids.data() + size_t(i) * k, counts[i]);
            totals[size_t(i) * 3] = c.cells; totals[size_t(i) * 3 + 1] = c.sats; totals[size_t(i) * 3 + 2] = c.pruned;
        }
        write_file(argv[10], ids);
        write_file(argv[11], counts);
        write_file(argv[12], totals);
    } else {
        fprintf(stderr, "obb_host: unknown operation or wrong number of files: %s\n", op.c_str());
        return 2;
    }
    return 0;
}
