// assemble_host -- the per-triangle function of include/hagrid/assemble.h on the host (tests/test_assemble_cpu.py).
//
//   assemble_host obj FILE          FILE through load_obj_indexed (include/hagrid/load_obj.h: vertices + index triples), every triple
//                                   through assemble::mesh_tri; writes "<count or -1>\n" and the raw Tri records to stdout -- the
//                                   output format of obj_dump, which goes through load_obj_triangles
//   assemble_host scene IN OUT      a scene of meshes, instances and matrices from IN, assembled like hagrid_scene_assemble does it:
//                                   OUT = int64 bad-index count | Tri records | (instance, triangle) int32 pairs
//
// IN (little-endian): int32 num_meshes, num_instances, has_transforms; per mesh int32 num_vertices, num_tris, stride (bytes),
// has_indices; per mesh its vertex bytes (num_vertices * stride) and, with has_indices, 3 * num_tris int32; int32 instance_mesh[];
// with has_transforms 12 floats per instance.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hagrid/assemble.h"
#include "hagrid/load_obj.h"

using namespace hagrid;

struct HostMesh {
    int32_t num_vertices, num_tris, stride, has_indices;
    std::vector<float> vertices;
    std::vector<int32_t> indices;
};

template <typename T>
static bool get(FILE* f, T* dst, size_t n) { return n == 0 || std::fread(dst, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "obj")) {
        std::vector<vec3> vertices;
        std::vector<int> indices;
        const bool ok = load_obj_indexed(argv[2], vertices, indices);
        const int n = int(indices.size() / 3);
        std::printf("%d\n", ok ? n : -1);
        if (!ok) return 0;
        std::vector<Tri> tris;
        bool bad = false;
        for (int p = 0; p < n; p++)
            tris.push_back(assemble::mesh_tri(&vertices[0].x, 3, int(vertices.size()), static_cast<const int*>(indices.data()), p, nullptr, &bad));
        if (bad) return 3;                                  // (the loader refuses indices beyond the vertex list)
        if (n) std::fwrite(tris.data(), sizeof(Tri), tris.size(), stdout);
        return 0;
    }
    if (argc != 4 || std::strcmp(argv[1], "scene")) return 2;
    FILE* in = std::fopen(argv[2], "rb");
    if (!in) return 2;
    int32_t head[3];
    if (!get(in, head, 3)) return 2;
    const int num_meshes = head[0], num_instances = head[1];
    std::vector<HostMesh> meshes((size_t(num_meshes)));
    for (auto& m : meshes) if (!get(in, &m.num_vertices, 4)) return 2;
    for (auto& m : meshes) {
        m.vertices.resize(size_t(m.num_vertices) * size_t(m.stride / 4));
        if (!get(in, m.vertices.data(), m.vertices.size())) return 2;
        if (m.has_indices) { m.indices.resize(3 * size_t(m.num_tris)); if (!get(in, m.indices.data(), m.indices.size())) return 2; }
    }
    std::vector<int32_t> instance_mesh((size_t(num_instances)));
    if (!get(in, instance_mesh.data(), instance_mesh.size())) return 2;
    std::vector<float> transforms;
    if (head[2]) { transforms.resize(12 * size_t(num_instances)); if (!get(in, transforms.data(), transforms.size())) return 2; }
    std::fclose(in);

    std::vector<Tri> tris;
    std::vector<int32_t> origins;
    int64_t bad_count = 0;
    for (int i = 0; i < num_instances; i++) {
        const HostMesh& m = meshes[size_t(instance_mesh[size_t(i)])];
        for (int p = 0; p < m.num_tris; p++) {
            bool bad = false;
            tris.push_back(assemble::mesh_tri(static_cast<const float*>(m.vertices.data()), m.stride / 4, m.num_vertices,
                                              m.has_indices ? static_cast<const int*>(m.indices.data()) : static_cast<const int*>(nullptr), p,
                                              head[2] ? transforms.data() + 12 * size_t(i) : nullptr, &bad));
            bad_count += bad;
            origins.push_back(i); origins.push_back(p);
        }
    }
    FILE* out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    std::fwrite(&bad_count, sizeof(bad_count), 1, out);
    if (!tris.empty()) { std::fwrite(tris.data(), sizeof(Tri), tris.size(), out); std::fwrite(origins.data(), 4, origins.size(), out); }
    std::fclose(out);
    return 0;
}
