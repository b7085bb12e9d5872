// hagrid/assemble.h -- the Tri array of a scene of indexed meshes and instances (hagrid_amd.h: "scenes on the device").
//
// The reference makes its 48-byte Tri records on the host, in its front-end (src/main.cpp:246-275: v0, e1 = v0 - v1,
// e2 = v2 - v0, the normal in the three w slots), and so did this project until build_grid's input could be assembled
// on the device.  Here the same packing is a HOST DEVICE inline function of three vertices and an optional 3 x 4
// matrix.  The gfx950 kernel of hagrid_amd/csrc/assemble.hip calls it, and so can a host program
// (tests/cpp/assemble_host.cpp, tools/hagrid_cli.cpp): both give the bits of hagrid_amd/scene.py (transform_points,
// tris_from_vertices, assemble_tris) -- float32, no contraction (-ffp-contract=off), every sum in the order written.
// Below it, a shim over the C ABI on device pointers, in the style of the other headers of this directory.
#ifndef HAGRID_ASSEMBLE_H
#define HAGRID_ASSEMBLE_H

#include <vector>

#include "mem_manager.h"
#include "prims.h"
#include "vec.h"

namespace hagrid {
namespace assemble {

// ---- one vertex / one triangle ---------------------------------------------------------------------------------------------

/// A point under the 3 x 4 matrix m (row-major, last column = translation): x' = ((m[0]*x + m[1]*y) + m[2]*z) + m[3],
/// rows 1 and 2 likewise with m[4..7], m[8..11]
HOST DEVICE inline vec3 transform_point(const float* m, const vec3& v) {
    return vec3(((m[0] * v.x + m[1] * v.y) + m[2] * v.z) + m[3],
                ((m[4] * v.x + m[5] * v.y) + m[6] * v.z) + m[7],
                ((m[8] * v.x + m[9] * v.y) + m[10] * v.z) + m[11]);
}

/// The packing of main.cpp:259-267: e1 = v0 - v1, e2 = v2 - v0, n = cross(e1, e2), record = v0, n.x, e1, n.y, e2, n.z
HOST DEVICE inline Tri make_tri(const vec3& v0, const vec3& v1, const vec3& v2) {
    const vec3 e1 = v0 - v1, e2 = v2 - v0, n = cross(e1, e2);
    return Tri(v0, n.x, e1, n.y, e2, n.z);
}

/// The Tri of three vertices placed by the matrix m; m == nullptr uses the vertices as they are (NOT a multiplication by
/// the identity, which would turn -0 into +0)
HOST DEVICE inline Tri assemble_tri(const vec3& v0, const vec3& v1, const vec3& v2, const float* m) {
    if (!m) return make_tri(v0, v1, v2);
    return make_tri(transform_point(m, v0), transform_point(m, v1), transform_point(m, v2));
}

/// Vertex i of a buffer of float32 x, y, z records stride_words floats apart.  (The pointer types of this and the next function are template
/// parameters so that the kernel can pass pointers it knows to be device memory; a host program passes const float* and const int*.)
template <typename FloatPtr>
HOST DEVICE inline vec3 load_vertex(FloatPtr vertices, int stride_words, int i) {
    const FloatPtr p = vertices + size_t(i) * size_t(stride_words);
    return vec3(p[0], p[1], p[2]);
}

/// Triangle p of a mesh (indices null: vertices 3p, 3p+1, 3p+2) under the matrix m or nullptr; the vertex stride is given in floats
/// (hagrid_mesh.vertex_stride / 4).  A triangle that names a vertex outside 0 .. num_vertices-1 reads nothing out of bounds: it becomes
/// the degenerate triangle on vertex 0 and *bad is set (it is left alone otherwise).  num_vertices must be positive.
template <typename FloatPtr, typename IntPtr>
HOST DEVICE inline Tri mesh_tri(FloatPtr vertices, int stride_words, int num_vertices, IntPtr indices, int p, const float* m, bool* bad) {
    int i0, i1, i2;
    if (indices) { i0 = indices[3 * size_t(p)]; i1 = indices[3 * size_t(p) + 1]; i2 = indices[3 * size_t(p) + 2]; }
    else { i0 = 3 * p; i1 = i0 + 1; i2 = i0 + 2; }                      // (3p + 2 fits an int: checked where the scene is described)
    const unsigned nv = unsigned(num_vertices);
    if (unsigned(i0) >= nv || unsigned(i1) >= nv || unsigned(i2) >= nv) { i0 = i1 = i2 = 0; *bad = true; }
    return assemble_tri(load_vertex(vertices, stride_words, i0), load_vertex(vertices, stride_words, i1), load_vertex(vertices, stride_words, i2), m);
}

// ---- shim over the C ABI: device pointers, a MemManager's context and stream, asynchronous ---------------------------------

/// A scene of meshes and instances (hagrid_scene).  The vertex and index buffers stay the caller's and are read at every
/// assemble(): rewrite the vertices, assemble again, build the grid again.
class MeshScene {
public:
    /// instance_mesh empty: one instance per mesh, in order
    MeshScene(MemManager& mem, const std::vector<hagrid_mesh>& meshes, const std::vector<int32_t>& instance_mesh = std::vector<int32_t>())
        : ctx_(mem.context()), scene_(nullptr), num_instances_(int(instance_mesh.empty() ? meshes.size() : instance_mesh.size())) {
        hagrid::detail::check(ctx_, hagrid_scene_create(ctx_, meshes.data(), int(meshes.size()), instance_mesh.empty() ? nullptr : instance_mesh.data(), num_instances_, &scene_));
    }
    ~MeshScene() { hagrid_scene_destroy(ctx_, scene_); }
    MeshScene(const MeshScene&) = delete;
    MeshScene& operator=(const MeshScene&) = delete;

    int num_instances() const { return num_instances_; }
    /// first output triangle of instance i; i = num_instances() gives the total
    int first_tri(int i) const { return hagrid_scene_first_tri(scene_, i); }
    int num_tris() const { return first_tri(num_instances_); }
    /// transforms: 12 floats per instance on the device, or nullptr; tris: num_tris() records; origins: (instance, triangle) pairs or nullptr
    void assemble(const float* transforms, Tri* tris, int32_t* origins = nullptr) {
        hagrid::detail::check(ctx_, hagrid_scene_assemble(ctx_, scene_, transforms, tris, origins));
    }
    /// triangles with an index out of range since the last call (waits for the stream)
    int64_t bad_indices() {
        int64_t n = 0;
        hagrid::detail::check(ctx_, hagrid_scene_bad_indices(ctx_, scene_, &n));
        return n;
    }

private:
    hagrid_ctx* ctx_;
    hagrid_scene* scene_;
    int num_instances_;
};

} // namespace assemble
} // namespace hagrid

#endif // HAGRID_ASSEMBLE_H
