// segments_host -- the capsule query of include/hagrid/capsule.h (hagrid_amd.h: hagrid_segment_tris) on the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=),
// driven from files: seg_tri pair by pair, the brute-force definition, and the walk over the construction format that segment_tris_kernel
// (hagrid_amd/csrc/capsule.hip) runs on the device.  tests/test_segments_cpu.py compares what this writes with hagrid_amd/scene.py (segment_pairs,
// segment_tris) and the fixture tests/golden/segments.npz, tests/test_segments_gpu.py with what the device wrote.
//
//   segments_host pairs PARAMS TRIS SEGMENTS OUT
//   segments_host brute PARAMS TRIS SEGMENTS CURSORS QLABELS TLABELS ENTRIES RECORDS
//   segments_host walk  PARAMS GRID_ENTRIES CELLS REFS TRIS SEGMENTS CURSORS QLABELS TLABELS ENTRIES RECORDS COUNTS
// brute and walk, their PARAMS and files: list_host.h; box_only = 1 leaves the separating axes out of the walk's lower bound, to measure what they prune.
// A segment is 8 f32: ax, ay, az, r, bx, by, bz, 0; two labels per segment; RECORDS: {qx, qy, qz, d2, id, feature, side, s}.  pairs: PARAMS is i32 n alone;
// triangle i against segment i, 8 words each: valid, d2, qx, qy, qz, feature, side, s.
#include "hagrid/capsule.h"
#include "list_host.h"

using namespace list_host;
namespace cap = hagrid::capsule;

namespace {

struct Segments {
    struct Query { float ax, ay, az, r, bx, by, bz, zero; };
    typedef cap::SegList<KMAX> List;
    enum { kLabels = 2, kBoxOnly = 1 };
    static vec3 a(const Query& q) { return vec3(q.ax, q.ay, q.az); }
    static vec3 b(const Query& q) { return vec3(q.bx, q.by, q.bz); }
    static void setup(List& l, int k, float cursor_d2, int cursor_id, const int32_t* labels, const int32_t* tri_labels) {
        l.setup(k, cursor_d2, cursor_id, labels ? labels[0] : -1, labels ? labels[1] : -1, tri_labels);
    }
    template <typename F>
    static void brute(F tri_at, int num_tris, const Query& q, List& l) { cap::brute_force(tri_at, num_tris, a(q), b(q), q.r, l); }
    template <typename G, typename S>
    static void walk(const G& g, S& st, const Query& q, List& l, hc::Counts& c, bool box_only) { cap::segment_query(g, st, a(q), b(q), q.r, l, c, !box_only); }
    template <typename F>
    static void record(F tri_at, int id, float d2, const Query& q, Result& r) {
        cap::SegRecord o;
        cap::slot_record(tri_at, id, d2, a(q), b(q), o);
        r.qx = o.q.x; r.qy = o.q.y; r.qz = o.q.z; r.d2 = o.d2; r.id = o.id; r.feature = o.feature; r.side = float(o.side); r.last = o.s;
    }
};
typedef Segments::Query Segment;
static_assert(sizeof(Segment) == 32, "record layout");

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: segments_host pairs|brute|walk PARAMS ... \n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
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
    } else if (run<Segments>(op, p, argc, argv) != 0) {
        fprintf(stderr, "segments_host: unknown operation or wrong number of files: %s\n", op.c_str());
        return 2;
    }
    return 0;
}
