// distance_host -- include/hagrid/distance.h on the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven from files: the definition (closest.h's brute force
// over the voxel centres with r = band) and the scatter that hagrid_amd/csrc/distance.hip runs on the device, sequentially: sizes -> exclusive sums -> tasks ->
// splat -> finish.  tests/test_distance_lattice_cpu.py compares what this writes with hagrid_amd/scene.py and the fixture tests/golden/distance_lattice.npz.
//
//   distance_host brute   PARAMS TRIS OUT
//   distance_host scatter PARAMS TRIS OUT
// PARAMS: 3 f32 origin, 3 f32 size, 3 i32 n, f32 band, 3 f32 grid box min, 3 f32 grid box max, i32 T (voxels per task), i32 reverse (tasks taken last first).
// OUT: one result record per voxel (32 bytes: {f32 qx, qy, qz, d2}, {i32 id, i32 feature, f32 side, 0}), then 4 i64: triangles with a voxel box, tasks,
// pairs within the band, voxels with an answer (brute: 0, 0, pairs, voxels).
#include <string>
#include <vector>

#include "hagrid/common.h"
#include "hagrid/prims.h"
#include "hagrid/closest.h"
#include "hagrid/distance.h"
#include "host_support.h"

using namespace hagrid;
using namespace host_support;
namespace hc = hagrid::closest;
namespace hd = hagrid::distance;

namespace {

struct Result { float qx, qy, qz, d2; int32_t id, feature; float side; int32_t zero; };
static_assert(sizeof(Result) == 32, "record layout");

Result to_record(const hc::Best& b) {
    Result r;
    r.qx = b.q.x; r.qy = b.q.y; r.qz = b.q.z; r.d2 = b.d2;
    r.id = b.id; r.feature = b.feature; r.side = float(b.side); r.zero = 0;
    return r;
}

struct HostSlots {
    std::vector<unsigned long long>& v;
    unsigned long long load(int e) const { return v.at(size_t(e)); }
    void take_min(int e, unsigned long long key) { if (key < v.at(size_t(e))) v[size_t(e)] = key; }
};

void write_out(const char* name, const std::vector<Result>& out, const int64_t counts[4]) {
    std::vector<char> bytes(out.size() * sizeof(Result) + 4 * sizeof(int64_t));
    if (!out.empty()) memcpy(bytes.data(), out.data(), out.size() * sizeof(Result));
    memcpy(bytes.data() + out.size() * sizeof(Result), counts, 4 * sizeof(int64_t));
    write_file(name, bytes);
}

} // namespace

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: distance_host brute|scatter PARAMS TRIS OUT\n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    float origin[3], size[3], lo[3], hi[3];
    int n[3];
    for (int a = 0; a < 3; a++) origin[a] = p.get<float>();
    for (int a = 0; a < 3; a++) size[a] = p.get<float>();
    for (int a = 0; a < 3; a++) n[a] = p.get<int32_t>();
    const float band = p.get<float>();
    for (int a = 0; a < 3; a++) lo[a] = p.get<float>();
    for (int a = 0; a < 3; a++) hi[a] = p.get<float>();
    const int T = p.get<int32_t>();
    const int reverse = p.get<int32_t>();
    const std::vector<Tri> tris = read_file<Tri>(argv[3]);
    const int num_tris = int(tris.size());
    const long long voxels = (long long)n[0] * n[1] * n[2];
    if (n[0] <= 0 || n[1] <= 0 || n[2] <= 0 || voxels > (1ll << 28) || T < 1 || !(band >= 0.0f)) { fprintf(stderr, "distance_host: bad parameters\n"); return 2; }
    const hd::Consts c = hd::make_consts(lo, hi, origin, size, n, band);
    const Tri* t = tris.data();
    auto tri_at = [t](int j) { return t[j]; };
    std::vector<Result> out((size_t(voxels)));
    int64_t counts[4] = {0, 0, 0, 0};

    if (op == "brute") {
        for (int e = 0; e < int(voxels); e++) {
            const vec3 pt = hd::element_centre(c, e);
            hc::Best b;
            hc::brute_force(tri_at, num_tris, pt, band, b);
            out[size_t(e)] = to_record(b);
            counts[3] += b.id >= 0 ? 1 : 0;
            for (int j = 0; j < num_tris; j++) {
                hc::Pair r;
                if (hc::point_tri(tris[size_t(j)], pt, r) && r.d2 <= c.r2) counts[2]++;
            }
        }
    } else if (op == "scatter") {
        // sizes
        std::vector<int> sizes((size_t(num_tris)));
        for (int j = 0; j < num_tris; j++) {
            const int v = hd::tri_box(tris[size_t(j)], c).voxels();
            sizes[size_t(j)] = hd::num_tasks(v, T);
            counts[0] += v > 0 ? 1 : 0; counts[1] += sizes[size_t(j)];
        }
        // exclusive sums
        std::vector<int> offsets(size_t(num_tris) + 1, 0);
        long long sum = 0;
        for (int j = 0; j < num_tris; j++) { offsets[size_t(j)] = int(sum); sum += sizes[size_t(j)]; }
        offsets[size_t(num_tris)] = int(sum);
        if (sum > 0x3fffffff) { fprintf(stderr, "distance_host: too many tasks\n"); return 2; }
        const int total = int(sum);
        const int* off = offsets.data();
        // splat, task by task
        std::vector<unsigned long long> keys(size_t(voxels), hd::kEmpty);
        HostSlots slots{keys};
        for (int i = 0; i < total; i++) {
            const int task = reverse ? total - 1 - i : i;
            const int j = hd::find_task([off](int k) { return off[k]; }, num_tris, task);
            if (!(off[j] <= task && task < off[j + 1])) { fprintf(stderr, "distance_host: find_task returned a triangle that does not own the task\n"); return 2; }
            const hd::Box box = hd::tri_box(tris[size_t(j)], c);
            const int v = box.voxels(), run = task - off[j];
            const long long first = (long long)run * T, last = first + T < v ? first + T : v;
            for (long long k = first; k < last; k++) {
                vec3 pt;
                const int e = hd::box_voxel(box, c, int(k), pt);
                if (e < 0 || e >= voxels) { fprintf(stderr, "distance_host: a box voxel outside the lattice\n"); return 2; }
                counts[2] += hd::splat_voxel(tris[size_t(j)], j, pt, c.r2, e, slots) ? 1 : 0;
            }
        }
        // finish
        for (int e = 0; e < int(voxels); e++) {
            hc::Best b;
            hd::finish_voxel(tri_at, keys[size_t(e)], hd::element_centre(c, e), c.r2, b);
            out[size_t(e)] = to_record(b);
            counts[3] += b.id >= 0 ? 1 : 0;
        }
    } else {
        fprintf(stderr, "distance_host: unknown operation %s\n", op.c_str());
        return 2;
    }
    write_out(argv[4], out, counts);
    return 0;
}
