// segments_host -- the capsule query of include/hagrid/capsule.h (hagrid_amd.h: hagrid_segment_tris) on the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=),
// driven from files: seg_tri pair by pair, the brute-force definition, and the walk over the construction format that segment_tris_kernel
// (hagrid_amd/csrc/capsule.hip) runs on the device.  tests/test_segments_cpu.py compares what this writes with hagrid_amd/scene.py (segment_pairs,
// segment_tris) and the fixture tests/golden/segments.npz, tests/test_segments_gpu.py with what the device wrote.
//
//   segments_host pairs PARAMS TRIS SEGMENTS OUT
//   segments_host brute PARAMS TRIS SEGMENTS CURSORS QLABELS TLABELS ENTRIES RECORDS
//   segments_host walk  PARAMS GRID_ENTRIES CELLS REFS TRIS SEGMENTS CURSORS QLABELS TLABELS ENTRIES RECORDS COUNTS
// PARAMS: (walk: the grid header of host_support.h,) i32 n, i32 k, i32 cursors given, i32 labels given, i32 box_only (walk: 1 leaves the separating axes
// out of the lower bound, to measure what they prune); pairs: i32 n alone.  A segment is 8 f32: ax, ay, az, r, bx, by, bz, 0; a cursor and an entry
// {f32 d2, i32 id}; QLABELS 2 n i32, TLABELS 3 i32 per triangle (files that are not given are not read).  ENTRIES: n * k entries; RECORDS: n * k records
// {qx, qy, qz, d2, id, feature, side, s}; COUNTS: n x 4 i32 (cells visited, triangles tested, pruned, 1 = the list came back full).  pairs: triangle i
// against segment i, 8 words each: valid, d2, qx, qy, qz, feature, side, s.
#include <string>
#include <vector>

#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/grid.h"
#include "hagrid/capsule.h"
#include "host_support.h"

using namespace hagrid;
using namespace host_support;
namespace hc = hagrid::closest;
namespace cap = hagrid::capsule;

namespace {

constexpr int KMAX = 8;
struct Segment { float ax, ay, az, r, bx, by, bz, zero; };
struct Entry { float d2; int32_t id; };
struct Result { float qx, qy, qz, d2; int32_t id, feature; float side, s; };
static_assert(sizeof(Segment) == 32 && sizeof(Entry) == 8 && sizeof(Result) == 32, "record layout");

struct Batch {
    int n, k, box_only;
    std::vector<Segment> segs;
    std::vector<Entry> cursors;
    std::vector<int32_t> qlabels, tlabels;
    std::vector<Entry> entries;
    std::vector<Result> records;

    void load(Params& p, size_t num_tris, const char* seg_file, const char* cursor_file, const char* ql_file, const char* tl_file) {
        n = p.get<int32_t>(); k = p.get<int32_t>();
        const bool has_cursors = p.get<int32_t>() != 0, has_labels = p.get<int32_t>() != 0;
        box_only = p.get<int32_t>();
        if (k < 1 || k > KMAX) { fprintf(stderr, "k must be 1 .. %d\n", KMAX); exit(2); }
        segs = read_file<Segment>(seg_file);
        if (has_cursors) cursors = read_file<Entry>(cursor_file);
        if (has_labels) { qlabels = read_file<int32_t>(ql_file); tlabels = read_file<int32_t>(tl_file); }
        if (int(segs.size()) != n || (has_cursors && int(cursors.size()) != n) || (has_labels && (int(qlabels.size()) != 2 * n || tlabels.size() != 3 * num_tris))) {
            fprintf(stderr, "the files do not hold n segments, n cursors, 2 n query labels or 3 labels per triangle\n"); exit(2);
        }
        entries.resize(size_t(n) * k); records.resize(size_t(n) * k);
    }
    vec3 a(int i) const { return vec3(segs[i].ax, segs[i].ay, segs[i].az); }
    vec3 b(int i) const { return vec3(segs[i].bx, segs[i].by, segs[i].bz); }
    void setup(int i, cap::SegList<KMAX>& list) const {
        list.setup(k, cursors.empty() ? -1.0f : cursors[i].d2, cursors.empty() ? -1 : cursors[i].id, qlabels.empty() ? -1 : qlabels[2 * size_t(i)],
                   qlabels.empty() ? -1 : qlabels[2 * size_t(i) + 1], tlabels.empty() ? nullptr : tlabels.data());
    }
    template <typename F>
    void store(int i, const cap::SegList<KMAX>& list, F tri_at) {
        for (int j = 0; j < k; j++) {
            int id; float d2;
            list.get(j, id, d2);
            Entry& e = entries[size_t(i) * k + j];
            e.d2 = d2; e.id = id;
            cap::SegRecord o;
            cap::slot_record(tri_at, id, d2, a(i), b(i), o);
            Result& r = records[size_t(i) * k + j];
            r.qx = o.q.x; r.qy = o.q.y; r.qz = o.q.z; r.d2 = o.d2; r.id = o.id; r.feature = o.feature; r.side = float(o.side); r.s = o.s;
        }
    }
};

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: segments_host pairs|brute|walk PARAMS ... \n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    Batch b;
    if (op == "pairs" && argc == 6) {
        const int n = p.get<int32_t>();
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        const std::vector<Segment> segs = read_file<Segment>(argv[4]);
        if (int(tris.size()) != n || int(segs.size()) != n) { fprintf(stderr, "pairs: the files do not hold n triangles and n segments\n"); return 2; }
        std::vector<uint32_t> out(size_t(n) * 8);
        for (int i = 0; i < n; i++) {
            const vec3 a(segs[i].ax, segs[i].ay, segs[i].az), bb(segs[i].bx, segs[i].by, segs[i].bz);
            cap::SegPair r;
            r.d2 = 0.0f; r.q = vec3(0.0f, 0.0f, 0.0f); r.s = 0.0f; r.feature = 0;
            const bool valid = cap::seg_tri(tris[i], a, bb, r);
            const int32_t side = valid ? hc::tri_side(tris[i], a + (bb - a) * r.s, r.q) : 0;
            const float f[4] = {r.d2, r.q.x, r.q.y, r.q.z};
            uint32_t* o = &out[size_t(i) * 8];
            o[0] = valid ? 1u : 0u;
            memcpy(o + 1, f, 16);
            o[5] = uint32_t(r.feature); o[6] = uint32_t(side);
            memcpy(o + 7, &r.s, 4);
        }
        write_file(argv[5], out);
    } else if (op == "brute" && argc == 10) {
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        b.load(p, tris.size(), argv[4], argv[5], argv[6], argv[7]);
        const Tri* t = tris.data();
        for (int i = 0; i < b.n; i++) {
            cap::SegList<KMAX> list;
            b.setup(i, list);
            cap::brute_force([t](int j) { return t[j]; }, int(tris.size()), b.a(i), b.b(i), b.segs[i].r, list);
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
            cap::SegList<KMAX> list;
            hc::Counts c;
            b.setup(i, list);
            cap::segment_query(g, st, b.a(i), b.b(i), b.segs[i].r, list, c, b.box_only == 0);
            b.store(i, list, [&g](int j) { return g.tri(j); });
            counts[size_t(i) * 4] = c.cells; counts[size_t(i) * 4 + 1] = c.tris; counts[size_t(i) * 4 + 2] = c.pruned; counts[size_t(i) * 4 + 3] = list.full() ? 1 : 0;
        }
        write_file(argv[11], b.entries);
        write_file(argv[12], b.records);
        write_file(argv[13], counts);
    } else {
        fprintf(stderr, "segments_host: unknown operation or wrong number of files: %s\n", op.c_str());
        return 2;
    }
    return 0;
}
