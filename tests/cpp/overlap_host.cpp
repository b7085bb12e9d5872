// overlap_host -- include/hagrid/overlap.h on the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: the triangle / box test,
// the brute-force definition and the walk over the construction format that hagrid_amd/csrc/overlap.hip runs on the device.
// tests/test_overlap_cpu.py compares what this writes with hagrid_amd/scene.py and the fixture tests/golden/overlap.npz,
// tests/test_overlap_gpu.py with what the device wrote.
//
//   overlap_host pairs PARAMS TRIS BOXES OUT         PARAMS: i32 n;  triangle i against box i;  OUT: n i32 (1: the triangle meets the box)
//   overlap_host brute PARAMS TRIS BOXES IDS COUNTS  PARAMS: i32 n, i32 k, i32 any, 3 f32 grid box min, 3 f32 grid box max;  every box, clipped, against all triangles;  IDS: n x k i32, COUNTS: n i32
//   overlap_host walk  PARAMS ENTRIES CELLS REFS TRIS BOXES IDS COUNTS TOTALS
//                                                    PARAMS: the grid header (host_support.h), i32 n, i32 k, i32 any;
//                                                    TOTALS: n x 3 i32 (cells visited, tests evaluated, sub-blocks pruned)
// A box is 32 bytes: 3 f32 min, i32 first, 3 f32 max, i32 pad.
#include <string>
#include <vector>

#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/grid.h"
#include "hagrid/overlap.h"
#include "host_support.h"

using namespace hagrid;
using namespace host_support;
namespace ho = hagrid::overlap;

namespace {

struct BoxRec { float lo[3]; int32_t first; float hi[3]; int32_t pad; };
static_assert(sizeof(BoxRec) == 32, "record layout");

typedef ho::IdList<ho::kMaxIds> List;

void to_record(const List& l, int k, int32_t* ids, int32_t& count) {
    for (int j = 0; j < k; j++) ids[j] = l.id[j];
    count = l.count();
}

// the accessor of overlap.h: the grid and the clip box
struct OverlapGrid : HostGrid<kEndUnbounded> { ho::Clip clip; };

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: overlap_host pairs|brute|walk PARAMS ... OUT\n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    if (op == "pairs" && argc == 6) {
        const int n = p.get<int32_t>();
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        const std::vector<BoxRec> boxes = read_file<BoxRec>(argv[4]);
        if (int(tris.size()) != n || int(boxes.size()) != n) { fprintf(stderr, "pairs: the files do not hold n records\n"); return 2; }
        std::vector<int32_t> out(size_t(n), 0);
        for (int i = 0; i < n; i++) {
            const vec3 lo(boxes[i].lo[0], boxes[i].lo[1], boxes[i].lo[2]), hi(boxes[i].hi[0], boxes[i].hi[1], boxes[i].hi[2]);
            out[i] = (!ho::inactive(lo, hi) && ho::meets(tris[i], lo, hi)) ? 1 : 0;
        }
        write_file(argv[5], out);
    } else if (op == "brute" && argc == 7) {
        const int n = p.get<int32_t>(), k = p.get<int32_t>(), any = p.get<int32_t>();
        const vec3 glo = p.get3(), ghi = p.get3();
        ho::Clip clip;
        clip.set(glo, ghi);
        if (k < 1 || k > ho::kMaxIds || (any && k != 1)) { fprintf(stderr, "brute: bad k\n"); return 2; }
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        const std::vector<BoxRec> boxes = read_file<BoxRec>(argv[4]);
        if (int(boxes.size()) != n) { fprintf(stderr, "brute: the box file does not hold n records\n"); return 2; }
        std::vector<int32_t> ids(size_t(n) * k), counts((size_t(n)));
        const Tri* t = tris.data();
        for (int i = 0; i < n; i++) {
            const vec3 lo(boxes[i].lo[0], boxes[i].lo[1], boxes[i].lo[2]), hi(boxes[i].hi[0], boxes[i].hi[1], boxes[i].hi[2]);
            List l;
            l.init(k, boxes[i].first);
            ho::brute_force([t](int j) { return t[j]; }, int(tris.size()), clip, lo, hi, any != 0, l);
            to_record(l, k, ids.data() + size_t(i) * k, counts[i]);
        }
        write_file(argv[5], ids);
        write_file(argv[6], counts);
    } else if (op == "walk" && argc == 11) {
        const GridHeader h = p.get_grid_header();
        const int n = p.get<int32_t>(), k = p.get<int32_t>(), any = p.get<int32_t>();
        if (k < 1 || k > ho::kMaxIds || (any && k != 1)) { fprintf(stderr, "walk: bad k\n"); return 2; }
        OverlapGrid g;
        g.load(h, argv[3], argv[4], argv[5]);
        g.clip.set(h.lo, h.hi);
        g.tris = read_file<Tri>(argv[6]);
        const std::vector<BoxRec> boxes = read_file<BoxRec>(argv[7]);
        if (int(boxes.size()) != n) { fprintf(stderr, "walk: the box file does not hold n records\n"); return 2; }
        std::vector<int32_t> ids(size_t(n) * k), counts((size_t(n))), totals(size_t(n) * 3);
        ho::ArrayStack<ho::kMaxLevels> st;
        for (int i = 0; i < n; i++) {
            const vec3 lo(boxes[i].lo[0], boxes[i].lo[1], boxes[i].lo[2]), hi(boxes[i].hi[0], boxes[i].hi[1], boxes[i].hi[2]);
            List l;
            l.init(k, boxes[i].first);
            ho::Counts c;
            ho::overlap_query(g, st, lo, hi, any != 0, l, c);
            to_record(l, k, ids.data() + size_t(i) * k, counts[i]);
            totals[size_t(i) * 3] = c.cells; totals[size_t(i) * 3 + 1] = c.sats; totals[size_t(i) * 3 + 2] = c.pruned;
        }
        write_file(argv[8], ids);
        write_file(argv[9], counts);
        write_file(argv[10], totals);
    } else {
        fprintf(stderr, "overlap_host: unknown operation or wrong number of files: %s\n", op.c_str());
        return 2;
    }
    return 0;
}
