// nearest_k_host -- the k-list of include/hagrid/closest.h (NearList: hagrid_amd.h, hagrid_nearest_tris) on the HOST (g++ -ffp-contract=off -DHOST=
// -DDEVICE=), driven from files: the brute-force definition and the walk over the construction format that nearest_tris_kernel of
// hagrid_amd/csrc/closest.hip runs on the device.  tests/test_nearest_k_cpu.py compares what this writes with hagrid_amd/scene.py (nearest_tris) and the
// fixture tests/golden/nearest_k.npz, tests/test_nearest_k_gpu.py with what the device wrote.
//
//   nearest_k_host brute PARAMS TRIS POINTS CURSORS QLABELS TLABELS ENTRIES RECORDS
//   nearest_k_host walk  PARAMS GRID_ENTRIES CELLS REFS TRIS POINTS CURSORS QLABELS TLABELS ENTRIES RECORDS COUNTS
// PARAMS: (walk: the grid header of host_support.h,) i32 n, i32 k, i32 cursors given, i32 labels given.  A point is 4 f32: x, y, z, r; a cursor and an
// entry {f32 d2, i32 id}; QLABELS n i32, TLABELS 3 i32 per triangle (files that are not given are not read).  ENTRIES: n * k entries; RECORDS: n * k
// result records of closest_host; COUNTS: n x 4 i32 (cells visited, triangles tested, pruned, 1 = the list came back full).
#include <string>
#include <vector>

#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/grid.h"
#include "hagrid/closest.h"
#include "host_support.h"

using namespace hagrid;
using namespace host_support;
namespace hc = hagrid::closest;

namespace {

constexpr int KMAX = 8;
struct Point { float x, y, z, r; };
struct Entry { float d2; int32_t id; };
struct Result { float qx, qy, qz, d2; int32_t id, feature; float side; int32_t zero; };
static_assert(sizeof(Point) == 16 && sizeof(Entry) == 8 && sizeof(Result) == 32, "record layout");

struct Batch {
    int n, k;
    std::vector<Point> pts;
    std::vector<Entry> cursors;
    std::vector<int32_t> qlabels, tlabels;
    std::vector<Entry> entries;
    std::vector<Result> records;

    void load(Params& p, size_t num_tris, const char* points, const char* cursor_file, const char* ql_file, const char* tl_file) {
        n = p.get<int32_t>(); k = p.get<int32_t>();
        const bool has_cursors = p.get<int32_t>() != 0, has_labels = p.get<int32_t>() != 0;
        if (k < 1 || k > KMAX) { fprintf(stderr, "k must be 1 .. %d\n", KMAX); exit(2); }
        pts = read_file<Point>(points);
        if (has_cursors) cursors = read_file<Entry>(cursor_file);
        if (has_labels) { qlabels = read_file<int32_t>(ql_file); tlabels = read_file<int32_t>(tl_file); }
        if (int(pts.size()) != n || (has_cursors && int(cursors.size()) != n) || (has_labels && (int(qlabels.size()) != n || tlabels.size() != 3 * num_tris))) {
            fprintf(stderr, "the files do not hold n points, n cursors, n query labels or 3 labels per triangle\n"); exit(2);
        }
        entries.resize(size_t(n) * k); records.resize(size_t(n) * k);
    }
    vec3 point(int i) const { return vec3(pts[i].x, pts[i].y, pts[i].z); }
    void setup(int i, hc::NearList<KMAX>& list) const {
        list.setup(k, cursors.empty() ? -1.0f : cursors[i].d2, cursors.empty() ? -1 : cursors[i].id, qlabels.empty() ? -1 : qlabels[i],
                   tlabels.empty() ? nullptr : tlabels.data());
    }
    template <typename F>
    void store(int i, const hc::NearList<KMAX>& list, F tri_at) {
        for (int j = 0; j < k; j++) {
            int id; float d2;
            list.get(j, id, d2);
            Entry& e = entries[size_t(i) * k + j];
            e.d2 = d2; e.id = id;
            hc::Best b;
            hc::slot_record(tri_at, id, d2, point(i), b);
            Result& r = records[size_t(i) * k + j];
            r.qx = b.q.x; r.qy = b.q.y; r.qz = b.q.z; r.d2 = b.d2; r.id = b.id; r.feature = b.feature; r.side = float(b.side); r.zero = 0;
        }
    }
};

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: nearest_k_host brute|walk PARAMS ... \n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    Batch b;
    if (op == "brute" && argc == 10) {
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        b.load(p, tris.size(), argv[4], argv[5], argv[6], argv[7]);
        const Tri* t = tris.data();
        for (int i = 0; i < b.n; i++) {
            hc::NearList<KMAX> list;
            b.setup(i, list);
            hc::brute_force([t](int j) { return t[j]; }, int(tris.size()), b.point(i), b.pts[i].r, list);
            b.store(i, list, [t](int j) { return t[j]; });
        }
        write_file(argv[8], b.entries);
        write_file(argv[9], b.records);
    } else if (op == "walk" && argc == 14) {
        const GridHeader h = p.get_grid_header();
        HostGrid<kEndUnbounded> g;
        g.load(h, argv[3], argv[4], argv[5]);
        g.tris = read_file<Tri>(argv[6]);
        b.load(p, g.tris.size(), argv[7], argv[8], argv[9], argv[10]);
        std::vector<int32_t> counts(size_t(b.n) * 4);
        hc::ArrayStack<hc::kMaxLevels> st;
        for (int i = 0; i < b.n; i++) {
            hc::NearList<KMAX> list;
            hc::Counts c;
            b.setup(i, list);
            hc::closest_query(g, st, b.point(i), b.pts[i].r, list, c);
            b.store(i, list, [&g](int j) { return g.tri(j); });
            counts[size_t(i) * 4] = c.cells; counts[size_t(i) * 4 + 1] = c.tris; counts[size_t(i) * 4 + 2] = c.pruned; counts[size_t(i) * 4 + 3] = list.full() ? 1 : 0;
        }
        write_file(argv[11], b.entries);
        write_file(argv[12], b.records);
        write_file(argv[13], counts);
    } else {
        fprintf(stderr, "nearest_k_host: unknown operation or wrong number of files: %s\n", op.c_str());
        return 2;
    }
    return 0;
}
