// closest_host -- include/hagrid/closest.h on the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: the per-pair
// arithmetic, the brute-force definition and the walk over the construction format that hagrid_amd/csrc/closest.hip runs on the device.
// tests/test_closest_cpu.py compares what this writes with hagrid_amd/scene.py and the fixture tests/golden/closest.npz,
// tests/test_closest_gpu.py with what the device wrote.
//
//   closest_host pairs PARAMS TRIS POINTS OUT        PARAMS: i32 n;  triangle i against point i;  OUT: n x 8 words: i32 valid, f32 d2, 3 f32 q,
//                                                    i32 feature, i32 side, 0
//   closest_host brute PARAMS TRIS POINTS OUT        PARAMS: i32 n;  every point against all triangles;  OUT: n result records (32 bytes)
//   closest_host walk  PARAMS ENTRIES CELLS REFS TRIS POINTS OUT COUNTS
//                                                    PARAMS: the grid header (host_support.h), i32 n;
//                                                    OUT: n result records;  COUNTS: n x 3 i32 (cells visited, triangles tested, pruned)
// A point is 4 f32: x, y, z, r.  A result record: {f32 qx, qy, qz, d2}, {i32 id, i32 feature, f32 side, 0}.
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

struct Point { float x, y, z, r; };
struct Result { float qx, qy, qz, d2; int32_t id, feature; float side; int32_t zero; };
static_assert(sizeof(Point) == 16 && sizeof(Result) == 32, "record layout");

Result to_record(const hc::Best& b) {
    Result r;
    r.qx = b.q.x; r.qy = b.q.y; r.qz = b.q.z; r.d2 = b.d2;
    r.id = b.id; r.feature = b.feature; r.side = float(b.side); r.zero = 0;
    return r;
}

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: closest_host pairs|brute|walk PARAMS ... OUT\n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    if (op == "pairs" && argc == 6) {
        const int n = p.get<int32_t>();
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        const std::vector<Point> pts = read_file<Point>(argv[4]);
        if (int(tris.size()) != n || int(pts.size()) != n) { fprintf(stderr, "pairs: the files do not hold n records\n"); return 2; }
        std::vector<uint32_t> out(size_t(n) * 8, 0u);
        for (int i = 0; i < n; i++) {
            const vec3 pt(pts[i].x, pts[i].y, pts[i].z);
            hc::Pair r;
            uint32_t* o = out.data() + size_t(i) * 8;
            if (!hc::point_tri(tris[i], pt, r)) continue;
            o[0] = 1u; o[1] = as<uint32_t>(r.d2); o[2] = as<uint32_t>(r.q.x); o[3] = as<uint32_t>(r.q.y); o[4] = as<uint32_t>(r.q.z);
            o[5] = uint32_t(r.feature); o[6] = uint32_t(hc::tri_side(tris[i], pt, r.q));
        }
        write_file(argv[5], out);
    } else if (op == "brute" && argc == 6) {
        const int n = p.get<int32_t>();
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        const std::vector<Point> pts = read_file<Point>(argv[4]);
        if (int(pts.size()) != n) { fprintf(stderr, "brute: the point file does not hold n records\n"); return 2; }
        std::vector<Result> out((size_t(n)));
        const Tri* t = tris.data();
        for (int i = 0; i < n; i++) {
            hc::Best b;
            hc::brute_force([t](int j) { return t[j]; }, int(tris.size()), vec3(pts[i].x, pts[i].y, pts[i].z), pts[i].r, b);
            out[i] = to_record(b);
        }
        write_file(argv[5], out);
    } else if (op == "walk" && argc == 10) {
        const GridHeader h = p.get_grid_header();
        const int n = p.get<int32_t>();
        HostGrid<kEndUnbounded> g;
        g.load(h, argv[3], argv[4], argv[5]);
        g.tris = read_file<Tri>(argv[6]);
        const std::vector<Point> pts = read_file<Point>(argv[7]);
        if (int(pts.size()) != n) { fprintf(stderr, "walk: the point file does not hold n records\n"); return 2; }
        std::vector<Result> out((size_t(n)));
        std::vector<int32_t> counts(size_t(n) * 3);
        hc::ArrayStack<hc::kMaxLevels> st;
        for (int i = 0; i < n; i++) {
            hc::Best b;
            hc::Counts c;
            hc::closest_query(g, st, vec3(pts[i].x, pts[i].y, pts[i].z), pts[i].r, b, c);
            out[i] = to_record(b);
            counts[size_t(i) * 3] = c.cells; counts[size_t(i) * 3 + 1] = c.tris; counts[size_t(i) * 3 + 2] = c.pruned;
        }
        write_file(argv[8], out);
        write_file(argv[9], counts);
    } else {
        fprintf(stderr, "closest_host: unknown operation or wrong number of files: %s\n", op.c_str());
        return 2;
    }
    return 0;
}
