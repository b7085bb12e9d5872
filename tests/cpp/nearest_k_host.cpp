// nearest_k_host -- the k-list of include/hagrid/closest.h (NearList: hagrid_amd.h, hagrid_nearest_tris) on the HOST (g++ -ffp-contract=off -DHOST=
// -DDEVICE=), driven from files: the brute-force definition and the walk over the construction format that nearest_tris_kernel of
// hagrid_amd/csrc/closest.hip runs on the device.  tests/test_nearest_k_cpu.py compares what this writes with hagrid_amd/scene.py (nearest_tris) and the
// fixture tests/golden/nearest_k.npz, tests/test_nearest_k_gpu.py with what the device wrote.
//
//   nearest_k_host brute PARAMS TRIS POINTS CURSORS QLABELS TLABELS ENTRIES RECORDS
//   nearest_k_host walk  PARAMS GRID_ENTRIES CELLS REFS TRIS POINTS CURSORS QLABELS TLABELS ENTRIES RECORDS COUNTS
// The operations, PARAMS and the files: list_host.h.  A point is 4 f32: x, y, z, r; one label per point; RECORDS: the result records of closest_host.
#include "list_host.h"

using namespace list_host;

namespace {

struct Points {
    struct Query { float x, y, z, r; };
    typedef hc::NearList<KMAX> List;
    enum { kLabels = 1, kBoxOnly = 0 };
    static vec3 p(const Query& q) { return vec3(q.x, q.y, q.z); }
    static void setup(List& l, int k, float cursor_d2, int cursor_id, const int32_t* labels, const int32_t* tri_labels) {
        l.setup(k, cursor_d2, cursor_id, labels ? labels[0] : -1, tri_labels);
    }
    template <typename F>
    static void brute(F tri_at, int num_tris, const Query& q, List& l) { hc::brute_force(tri_at, num_tris, p(q), q.r, l); }
    template <typename G, typename S>
    static void walk(const G& g, S& st, const Query& q, List& l, hc::Counts& c, bool) { hc::closest_query(g, st, p(q), q.r, l, c); }
    template <typename F>
    static void record(F tri_at, int id, float d2, const Query& q, Result& r) {
        hc::Best b;
        hc::slot_record(tri_at, id, d2, p(q), b);
        r.qx = b.q.x; r.qy = b.q.y; r.qz = b.q.z; r.d2 = b.d2; r.id = b.id; r.feature = b.feature; r.side = float(b.side); r.last = 0.0f;
    }
};
static_assert(sizeof(Points::Query) == 16, "record layout");

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: nearest_k_host brute|walk PARAMS ... \n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    if (run<Points>(op, p, argc, argv) == 0) return 0;
    fprintf(stderr, "nearest_k_host: unknown operation or wrong number of files: %s\n", op.c_str());
    return 2;
}
