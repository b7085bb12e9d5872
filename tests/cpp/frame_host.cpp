// frame_host -- the per-ray functions of include/hagrid/frame.h compiled for the HOST (g++ -ffp-contract=off -DHOST= -DDEVICE=), driven
// from files: tests/test_frame_cpu.py compares what this writes with hagrid_amd/scene.py bit for bit.  The gfx950 kernels call the same
// functions (hagrid_amd/csrc/frame.hip), so this is the kernels' arithmetic without a GPU.
//
//   frame_host primary PARAMS OUT                    PARAMS: 12 f32 camera (eye dir right up), f32 clip, i32 w, i32 h, i64 first, i32 count
//   frame_host bounce  PARAMS TRIS RAYS HITS OUT     PARAMS: u64 seed, u64 first, 3 f32 lo, 3 f32 hi, f32 tmax, u32 flags, i32 num_rays
//   frame_host shade   PARAMS HITS OUT               PARAMS: i32 mode, f32 clip, i32 n
//   frame_host ao      PARAMS HITS COUNTS OUT        PARAMS: i32 samples, i32 n
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hagrid/frame.h"

using namespace hagrid;

namespace {

template <typename T>
std::vector<T> read_file(const char* name) {
    std::vector<T> v;
    FILE* f = fopen(name, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", name); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize(size_t(bytes) / sizeof(T));
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short read of %s\n", name); exit(2); }
    fclose(f);
    return v;
}

template <typename T>
void write_file(const char* name, const std::vector<T>& v) {
    FILE* f = fopen(name, "wb");
    if (!f || (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size())) { fprintf(stderr, "cannot write %s\n", name); exit(2); }
    fclose(f);
}

struct Params {
    std::vector<char> bytes;
    size_t pos = 0;
    template <typename T> T get() {
        T t;
        if (pos + sizeof(T) > bytes.size()) { fprintf(stderr, "parameter file too short\n"); exit(2); }
        memcpy(&t, bytes.data() + pos, sizeof(T));
        pos += sizeof(T);
        return t;
    }
    vec3 get3() { const float x = get<float>(), y = get<float>(), z = get<float>(); return vec3(x, y, z); }
};

} // namespace

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: frame_host primary|bounce|shade|ao PARAMS ... OUT\n"); return 2; }
    const std::string op = argv[1];
    Params p;
    p.bytes = read_file<char>(argv[2]);
    if (op == "primary" && argc == 4) {
        frame::Camera cam;
        cam.eye = p.get3(); cam.dir = p.get3(); cam.right = p.get3(); cam.up = p.get3();
        const float clip = p.get<float>();
        const int w = p.get<int32_t>(), h = p.get<int32_t>();
        const int64_t first = p.get<int64_t>();
        const int count = p.get<int32_t>();
        std::vector<Ray> out((size_t(count)));
        for (int i = 0; i < count; i++) out[i] = frame::primary_ray(cam, clip, w, h, first + i);
        write_file(argv[3], out);
    } else if (op == "bounce" && argc == 7) {
        const uint64_t seed = p.get<uint64_t>(), first = p.get<uint64_t>();
        const vec3 lo = p.get3(), hi = p.get3();
        const float tmax = p.get<float>();
        const uint32_t flags = p.get<uint32_t>();
        const int n = p.get<int32_t>();
        const std::vector<Tri> tris = read_file<Tri>(argv[3]);
        const std::vector<Ray> rays = read_file<Ray>(argv[4]);
        const std::vector<Hit> hits = read_file<Hit>(argv[5]);
        if (int(rays.size()) != n || int(hits.size()) != n) { fprintf(stderr, "bounce: ray / hit files do not hold num_rays records\n"); return 2; }
        std::vector<Ray> out((size_t(n)));
        for (int i = 0; i < n; i++) {                 // the rule of frame_bounce_rays_kernel
            if (hits[i].id >= 0) {
                if (size_t(hits[i].id) >= tris.size()) { fprintf(stderr, "bounce: hit id beyond the triangles\n"); return 2; }
                out[i] = frame::bounce_ray(rays[i], hits[i].t, frame::tri_normal(tris[hits[i].id]), seed, first + uint64_t(i), tmax);
            } else if (flags & HAGRID_BOUNCE_REDRAW_MISSES) {
                out[i] = frame::incoherent_ray(lo, hi, seed ^ 0x6D69737300000000ull, first + uint64_t(i), 0.0f, FLT_MAX);
            } else {
                out[i] = frame::inactive_ray();
            }
        }
        write_file(argv[6], out);
    } else if (op == "shade" && argc == 5) {
        const int mode = p.get<int32_t>();
        const float clip = p.get<float>();
        const int n = p.get<int32_t>();
        const std::vector<Hit> hits = read_file<Hit>(argv[3]);
        if (int(hits.size()) != n) { fprintf(stderr, "shade: the hit file does not hold n records\n"); return 2; }
        std::vector<uint32_t> out((size_t(n)));
        for (int i = 0; i < n; i++) out[i] = frame::shade_hit(hits[i], mode, clip);
        write_file(argv[4], out);
    } else if (op == "ao" && argc == 6) {
        const int samples = p.get<int32_t>(), n = p.get<int32_t>();
        const std::vector<Hit> hits = read_file<Hit>(argv[3]);
        const std::vector<int32_t> counts = read_file<int32_t>(argv[4]);
        if (int(hits.size()) != n || int(counts.size()) != n) { fprintf(stderr, "ao: hit / count files do not hold n records\n"); return 2; }
        std::vector<uint32_t> out((size_t(n)));
        for (int i = 0; i < n; i++) out[i] = frame::shade_occlusion(hits[i].id, counts[i], samples);
        write_file(argv[5], out);
    } else {
        fprintf(stderr, "frame_host: unknown operation or wrong number of files: %s\n", op.c_str());
        return 2;
    }
    return 0;
}
