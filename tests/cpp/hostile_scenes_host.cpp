// hostile_scenes_host.cpp -- the CPU oracle's construction over a list of scenes, as a stand-alone program for the sanitizers
// (tests/test_hostile_scenes_cpu.py builds it with -fsanitize=address,undefined,float-cast-overflow together with oracle/hagrid_oracle.c).
//
//   hostile_scenes_host LIST      LIST: one scene per line, "<file of float32 triangles> <number of triangles> <expected return code>"
//
// Before the scenes: the total functions of include/hagrid/grid.h and prims.h (what the device compiles) against the oracle's restatements, on the
// documented values and on 20000 seeded boxes and triangles with zero, denormal, huge, infinite and NaN components.
// A scene that is expected to build goes through merge, flatten, expand, the grid check and compress as well; a scene that is expected to be
// refused must leave the grid untouched.  Prints "ok" per scene; exit status 1 on the first scene that does something else.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <cstdint>
#include <cstring>
#include <limits>

#include "hagrid/grid.h"
#include "hagrid/prims.h"
#include "hagrid_oracle.h"

namespace {

uint64_t rng_state = 0x686F7374696C65ull;
uint32_t rnd() {          // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return uint32_t((z ^ (z >> 31)) >> 32);
}
float special() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float v[] = { 0.0f, -0.0f, 1e-45f, 1e-38f, 1e-30f, 1e-20f, 1e-6f, 0.25f, 1.0f, 3.0f, 1e6f, 1e20f, 3e38f, inf, -inf, nan, -1.0f, -3e38f };
    return v[rnd() % (sizeof(v) / sizeof(v[0]))];
}
float uniform() { return float(rnd() >> 8) * (1.0f / 16777216.0f) * 4.0f - 2.0f; }

hagrid::BBox hbox(const OBBox& b) { return hagrid::BBox(hagrid::vec3(b.min.x, b.min.y, b.min.z), hagrid::vec3(b.max.x, b.max.y, b.max.z)); }
bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

bool dims_are(const float* lo, const float* hi, int n, float density, int x, int y, int z) {
    OBBox b; b.min = { lo[0], lo[1], lo[2] }; b.max = { hi[0], hi[1], hi[2] }; b.pad0 = b.pad1 = 0;
    oivec3 o; orc_compute_grid_dims(&b, n, density, &o);
    const hagrid::ivec3 h = hagrid::compute_grid_dims(hbox(b), n, density);
    return o.x == x && o.y == y && o.z == z && h.x == x && h.y == y && h.z == z;
}

int total_functions() {
    const int big = 0x7fffffff;
    const float zero[3] = { 0, 0, 0 }, flat[3] = { 1, 1, 0 }, thin[3] = { 1, 1, 1e-30f }, one[3] = { 1, 1, 1 }, brick[3] = { 1, 2, 4 };
    if (!dims_are(zero, flat, 200, 0.12f, big, big, 1) || !dims_are(zero, thin, 200, 0.12f, big, big, 1) || !dims_are(zero, zero, 37, 0.12f, 1, 1, 1) ||
        !dims_are(zero, one, 0, 2.4f, 1, 1, 1) || !dims_are(zero, brick, 1000, 0.12f, 2, 4, 9) || !dims_are(zero, one, 500, 1e30f, big, big, big)) {
        printf("total functions: a documented value differs\n"); return 1;
    }
    const int counts[] = { 0, 1, 37, 200, 100000, 0x7fffffff }, sizes[] = { 1, 2, 30, 994, 1 << 20 };
    const float densities[] = { 0.12f, 2.4f, 1e-30f, 1e30f };
    int compared = 0;
    for (int i = 0; i < 20000; i++) {
        OBBox b, o; b.pad0 = b.pad1 = o.pad0 = o.pad1 = 0;
        float lo[3], ext[3];
        for (int a = 0; a < 3; a++) { lo[a] = (i & 1) ? special() : uniform(); ext[a] = special(); }
        b.min = { lo[0], lo[1], lo[2] }; b.max = { lo[0] + ext[0], lo[1] + ext[1], lo[2] + ext[2] };
        o.min = { special(), special(), special() }; o.max = { special(), special(), special() };
        const int n = counts[rnd() % 6]; const float density = densities[rnd() % 4];
        oivec3 od; orc_compute_grid_dims(&b, n, density, &od);
        const hagrid::ivec3 hd = hagrid::compute_grid_dims(hbox(b), n, density);
        if (od.x != hd.x || od.y != hd.y || od.z != hd.z) { printf("total functions: compute_grid_dims differs at input %d\n", i); return 1; }
        if ((orc_grid_dims_defined(&b, n, density) != 0) != hagrid::grid_dims_defined(hbox(b), n, density)) { printf("total functions: grid_dims_defined differs at input %d\n", i); return 1; }
        OBBox ow; orc_widen_scene_box(&b, &ow);
        const hagrid::BBox hw = hagrid::widen_scene_box(hbox(b));
        if (!same_bits(ow.min.x, hw.min.x) || !same_bits(ow.min.y, hw.min.y) || !same_bits(ow.min.z, hw.min.z) ||
            !same_bits(ow.max.x, hw.max.x) || !same_bits(ow.max.y, hw.max.y) || !same_bits(ow.max.z, hw.max.z)) { printf("total functions: widen_scene_box differs at input %d\n", i); return 1; }
        const oivec3 dd = { sizes[rnd() % 5], sizes[rnd() % 5], sizes[rnd() % 5] };
        ORange r; orc_compute_range(&dd, &b, &o, &r);
        const hagrid::Range hr = hagrid::compute_range(hagrid::ivec3(dd.x, dd.y, dd.z), hbox(b), hbox(o));
        if (r.lx != hr.lx || r.ly != hr.ly || r.lz != hr.lz || r.hx != hr.hx || r.hy != hr.hy || r.hz != hr.hz) { printf("total functions: compute_range differs at input %d\n", i); return 1; }
        float t[12];
        for (int a = 0; a < 12; a++) t[a] = uniform();
        t[rnd() % 12] = special();
        if (i % 5 == 0) { t[0] = 3e38f; t[4] = -3e38f; }
        OTri ot; std::memcpy(&ot, t, sizeof(ot));
        hagrid::Tri ht; std::memcpy(&ht, t, sizeof(ht));
        if ((orc_tri_admissible(&ot) != 0) != hagrid::tri_admissible(ht)) { printf("total functions: tri_admissible differs at input %d\n", i); return 1; }
        compared++;
    }
    printf("total functions: %d inputs compared\n", compared);
    return 0;
}

} // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s LIST\n", argv[0]); return 2; }
    if (total_functions() != 0) return 1;
    FILE* list = fopen(argv[1], "r");
    if (!list) { perror(argv[1]); return 2; }
    char path[1024];
    int n = 0, want = 0;
    while (fscanf(list, "%1023s %d %d", path, &n, &want) == 3) {
        std::vector<OTri> tris(n > 0 ? n : 1);
        FILE* f = fopen(path, "rb");
        if (!f || fread(tris.data(), sizeof(OTri), size_t(n), f) != size_t(n)) { fprintf(stderr, "%s: cannot read %d triangles\n", path, n); return 2; }
        fclose(f);
        OGrid g;
        orc_grid_init(&g);
        const int rc = orc_build_grid(tris.data(), n, &g, 0.12f, 2.4f);
        if (rc != want) { printf("%s: orc_build_grid returned %d, expected %d\n", path, rc, want); return 1; }
        if (rc != 0) {
            if (g.entries || g.cells || g.ref_ids || g.num_cells) { printf("%s: a refusal touched the grid\n", path); return 1; }
        } else {
            orc_merge_grid(&g, 0.995f);
            orc_flatten_grid(&g);
            orc_expand_grid(&g, tris.data(), 3);
            char msg[256];
            if (orc_check_grid(&g, tris.data(), n, 1, msg, sizeof(msg)) != 0) { printf("%s: %s\n", path, msg); return 1; }
            orc_compress_grid(&g);
            orc_grid_free(&g);
        }
        printf("ok %s\n", path);
    }
    fclose(list);
    return 0;
}
