// assemble.hip -- a scene of indexed meshes and instances becomes the Tri array on the device (include/hagrid_amd.h "scenes on the device").
//
// One kernel, one output triangle per lane, 256 lanes per block.  The arithmetic is include/hagrid/assemble.h (the same function a host
// program calls); the kernel finds the lane's instance, gathers three vertices and stores the record as three float4.  Which instance a
// triangle belongs to is a binary search over the first-triangle table.  Most wavefronts lie inside ONE instance: the search runs once for
// the wavefront's first triangle (a wave-uniform value: scalar registers, scalar loads), and when the wavefront's last triangle is still
// below that instance's end, the mesh record and the twelve matrix words are wave-uniform too -- the compiler keeps them in scalar
// registers.  Only wavefronts that straddle an instance boundary search per lane.  Everything the kernel writes -- records, origins, the
// bad-index count -- leaves through vector stores and a vector atomic.
#include "ctx.h"

#include <climits>

#include "hagrid/assemble.h"

using namespace hagrid_impl;
namespace ha = hagrid::assemble;
using hagrid::Tri;

// The scene behind the C handle: the host's copy of the first-triangle table, and one pool buffer with the device tables.
struct hagrid_scene {
    hagrid_ctx* ctx = nullptr;                    // the context whose pool holds the tables: the only one the scene may be used with
    int num_meshes = 0, num_instances = 0;
    std::vector<int> first;                       // first[i] = first output triangle of instance i; first[num_instances] = total
    void* table = nullptr;                        // pool buffer: bad-index count (16 bytes) | mesh records | instance -> mesh | first
    unsigned long long* d_bad = nullptr;
    const hagrid_mesh* d_meshes = nullptr;
    const int* d_inst_mesh = nullptr;
    const int* d_first = nullptr;
};

namespace {

constexpr int kBlock = 256;

struct alignas(4) Origin { int instance, tri; };

// (Plain 16-byte stores: build_grid reads the records next.  Streaming stores were measured on assemble + build_grid and bought nothing: profiles/NOTES.md.)
__device__ __forceinline__ void store4(float4* p, float x, float y, float z, float w) { *p = make_float4(x, y, z, w); }

// The vertex and index addresses come out of a table, so the compiler takes them for generic pointers (flat loads); they are device memory.
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* as_global(const void* p) {
    return (const __attribute__((address_space(1))) T*)p;
}

// largest i with first[i] <= t, for 0 <= t < first[n]: the instance of output triangle t (instances without triangles are never found)
__device__ __forceinline__ int find_instance(const int* __restrict__ first, int n, int t) {
    int lo = 0, hi = n;                           // first[lo] <= t < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool emit(const hagrid_mesh* __restrict__ meshes, const int* __restrict__ inst_mesh, const int* __restrict__ first,
                                     const float* __restrict__ transforms, int inst, int t, float4* __restrict__ tris, Origin* __restrict__ origins) {
    const hagrid_mesh m = meshes[inst_mesh[inst]];
    const int p = t - first[inst];
    bool bad = false;
    const Tri tri = ha::mesh_tri(as_global<float>(m.vertices), m.vertex_stride >> 2, m.num_vertices, as_global<int>(m.indices), p,
                                 transforms ? transforms + 12 * size_t(inst) : nullptr, &bad);
    float4* out = tris + 3 * size_t(t);
    store4(out, tri.v0.x, tri.v0.y, tri.v0.z, tri.nx);
    store4(out + 1, tri.e1.x, tri.e1.y, tri.e1.z, tri.ny);
    store4(out + 2, tri.e2.x, tri.e2.y, tri.e2.z, tri.nz);
    if (origins) { Origin o; o.instance = inst; o.tri = p; origins[t] = o; }
    return bad;
}

__global__ void __launch_bounds__(kBlock) assemble_tris_kernel(const hagrid_mesh* __restrict__ meshes, const int* __restrict__ inst_mesh, const int* __restrict__ first,
                                                               int num_instances, int total, const float* __restrict__ transforms,
                                                               float4* __restrict__ tris, Origin* __restrict__ origins, unsigned long long* __restrict__ bad_count) {
    const unsigned tu = blockIdx.x * unsigned(kBlock) + threadIdx.x;
    const unsigned w0 = __builtin_amdgcn_readfirstlane(tu);          // the wavefront's first triangle
    if (w0 >= unsigned(total)) return;
    const unsigned wl = min(w0 + 63u, unsigned(total) - 1u);          // ... and its last
    const int i0 = find_instance(first, num_instances, int(w0));      // wave-uniform
    const bool live = tu < unsigned(total);
    const int t = int(tu);
    bool bad = false;
    if (wl < unsigned(first[i0 + 1])) {                               // the whole wavefront inside instance i0: mesh record and matrix are scalars
        if (live) bad = emit(meshes, inst_mesh, first, transforms, i0, t, tris, origins);
    } else {
        if (live) bad = emit(meshes, inst_mesh, first, transforms, find_instance(first, num_instances, t), t, tris, origins);
    }
    const unsigned long long b = __ballot(bad);
    if (b && int(threadIdx.x & 63u) == __ffsll(b) - 1) atomicAdd(bad_count, (unsigned long long)__popcll(b));
}

inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }

int check_mesh(hagrid_ctx* ctx, const hagrid_mesh& m) {
    if (m.reserved != 0) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: hagrid_mesh.reserved must be 0");
    if (m.num_vertices < 0 || m.num_tris < 0) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: a mesh has a negative vertex or triangle count");
    if (m.vertex_stride < 12 || m.vertex_stride % 4 != 0) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: the vertex stride must be at least 12 and a multiple of 4");
    if (m.num_vertices == 0 && m.num_tris > 0) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: a mesh without vertices must have no triangles");
    if (m.num_tris > 0 && !m.vertices) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: a mesh with triangles has a null vertex buffer");
    if (!aligned(m.vertices, 4) || !aligned(m.indices, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: vertex and index buffers must be 4-byte aligned");
    if (!m.indices && m.num_tris > INT_MAX / 3) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: a mesh without indices names vertices beyond 2^31 - 1");
    return HAGRID_OK;
}

} // namespace

extern "C" int hagrid_scene_create(hagrid_ctx* ctx, const hagrid_mesh* meshes, int num_meshes, const int32_t* instance_mesh, int num_instances, hagrid_scene** out) {
    if (!ctx) return HAGRID_EINVAL;
    if (!out) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: null output handle");
    *out = nullptr;
    if (num_meshes < 0 || num_instances < 0) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: negative mesh or instance count");
    if (!meshes && num_meshes > 0) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: null mesh array");
    if (!instance_mesh && num_instances != num_meshes) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: without an instance list there is one instance per mesh (num_instances must be num_meshes)");
    for (int k = 0; k < num_meshes; k++) HG_TRY(check_mesh(ctx, meshes[k]));
    std::vector<int> inst(size_t(num_instances), 0), first(size_t(num_instances) + 1, 0);
    int64_t total = 0;
    for (int i = 0; i < num_instances; i++) {
        const int k = instance_mesh ? instance_mesh[i] : i;
        if (k < 0 || k >= num_meshes) HG_FAIL(ctx, HAGRID_EINVAL, "scene_create: an instance names a mesh outside the mesh array");
        inst[size_t(i)] = k;
        first[size_t(i)] = int(total);
        total += meshes[k].num_tris;
        if (total > int64_t(INT32_MAX)) HG_FAIL(ctx, HAGRID_ERANGE, "scene_create: more than 2^31 - 1 output triangles");
    }
    first[size_t(num_instances)] = int(total);

    HG_HIP(ctx, hipSetDevice(ctx->device));
    const size_t off_meshes = 16, off_inst = off_meshes + up16(sizeof(hagrid_mesh) * size_t(num_meshes)), off_first = off_inst + up16(4 * size_t(num_instances));
    const size_t bytes = off_first + up16(4 * (size_t(num_instances) + 1));
    std::vector<char> host(bytes, 0);
    if (num_meshes) memcpy(host.data() + off_meshes, meshes, sizeof(hagrid_mesh) * size_t(num_meshes));
    if (num_instances) memcpy(host.data() + off_inst, inst.data(), 4 * size_t(num_instances));
    memcpy(host.data() + off_first, first.data(), 4 * (size_t(num_instances) + 1));
    char* table = static_cast<char*>(hagrid_mem_alloc(ctx, bytes));
    if (!table) return HAGRID_ENOMEM;                                  // (hagrid_mem_alloc left the message)
    const int rc = hagrid_mem_copy_h2d(ctx, table, host.data(), bytes);
    if (rc < 0) { const std::string msg = ctx->err; hagrid_mem_free(ctx, table); ctx->err = msg; return rc; }

    hagrid_scene* s = new hagrid_scene();
    s->ctx = ctx; s->num_meshes = num_meshes; s->num_instances = num_instances;
    s->first.swap(first);
    s->table = table;
    s->d_bad = reinterpret_cast<unsigned long long*>(table);
    s->d_meshes = reinterpret_cast<const hagrid_mesh*>(table + off_meshes);
    s->d_inst_mesh = reinterpret_cast<const int*>(table + off_inst);
    s->d_first = reinterpret_cast<const int*>(table + off_first);
    *out = s;
    return HAGRID_OK;
}

extern "C" void hagrid_scene_destroy(hagrid_ctx* ctx, hagrid_scene* scene) {
    if (!scene) return;
    if (ctx && ctx == scene->ctx && scene->table) hagrid_mem_free(ctx, scene->table);       // (another context's pool does not know the buffer)
    delete scene;
}

extern "C" int hagrid_scene_first_tri(const hagrid_scene* scene, int instance) {
    if (!scene || instance < 0 || instance > scene->num_instances) return HAGRID_EINVAL;
    return scene->first[size_t(instance)];
}

extern "C" int hagrid_scene_assemble(hagrid_ctx* ctx, hagrid_scene* scene, const void* transforms, void* tris, void* origins) {
    if (!ctx) return HAGRID_EINVAL;
    if (!scene) HG_FAIL(ctx, HAGRID_EINVAL, "scene_assemble: null scene");
    if (scene->ctx != ctx) HG_FAIL(ctx, HAGRID_EINVAL, "scene_assemble: the scene belongs to another context");
    const int total = scene->first[size_t(scene->num_instances)];
    if (total == 0) return HAGRID_OK;
    if (!tris) HG_FAIL(ctx, HAGRID_EINVAL, "scene_assemble: null triangle buffer");
    if (!aligned(tris, 16)) HG_FAIL(ctx, HAGRID_EINVAL, "scene_assemble: the triangle buffer is not 16-byte aligned");
    if (!aligned(transforms, 4) || !aligned(origins, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "scene_assemble: transforms and origins must be 4-byte aligned");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    trav_image_source_touched(ctx, tris, size_t(total) * 48);
    assemble_tris_kernel<<<grid_blocks(total, kBlock), kBlock, 0, ctx->stream>>>(scene->d_meshes, scene->d_inst_mesh, scene->d_first, scene->num_instances, total,
                                                                                static_cast<const float*>(transforms), static_cast<float4*>(tris),
                                                                                static_cast<Origin*>(origins), scene->d_bad);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

extern "C" int hagrid_scene_bad_indices(hagrid_ctx* ctx, hagrid_scene* scene, int64_t* count) {
    if (!ctx) return HAGRID_EINVAL;
    if (!scene || !count) HG_FAIL(ctx, HAGRID_EINVAL, "scene_bad_indices: null scene or count");
    if (scene->ctx != ctx) HG_FAIL(ctx, HAGRID_EINVAL, "scene_bad_indices: the scene belongs to another context");
    unsigned long long n = 0;
    HG_TRY(hagrid_mem_copy_d2h(ctx, &n, scene->d_bad, sizeof(n)));      // drains the stream
    if (n) HG_HIP(ctx, hipMemsetAsync(scene->d_bad, 0, sizeof(n), ctx->stream));
    *count = int64_t(n);
    return HAGRID_OK;
}
