// hagrid/traverse.h -- ray traversal with the reference's signatures (src/traverse.h:11-14), as
// header-only shims over the C ABI.  Work goes to the current MemManager's context (the reference keeps
// the equivalent state in per-process __constant__ symbols, traverse.cu:7-12).
#ifndef HAGRID_TRAVERSE_H
#define HAGRID_TRAVERSE_H

#include "build.h"
#include "grid.h"
#include "vec.h"
#include "prims.h"

namespace hagrid {

/// Prepares the traversal of `grid` (traverse.cu:97-109): validates it and builds the context's traversal image
/// (hagrid_amd.h: hagrid_setup_traversal).  Call it again whenever the grid was rebuilt, as the reference's front-end does.
inline void setup_traversal(const Grid& grid) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_setup_traversal(detail::current_ctx(), &p));
}

/// Nearest hit per ray: hits[i].id = primitive id or -1, hits[i].t = distance.  Asynchronous on the
/// context's stream, like a kernel launch.
inline void traverse_grid(const Grid& grid, const Tri* tris, const Ray* rays, Hit* hits, int num_rays) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_traverse_grid(detail::current_ctx(), &p, tris, rays, hits, num_rays));
}

/// Extensions over the same walk (no counterpart in src/traverse.h): occlusion rays stop at their first accepted
/// intersection (hits[i].id >= 0 <=> occluded); `with_uvs` stores the barycentrics like a COMPUTE_UVS build (prims.h:285-288).
inline void traverse_grid_any_hit(const Grid& grid, const Tri* tris, const Ray* rays, Hit* hits, int num_rays) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_traverse_grid_ex(detail::current_ctx(), &p, tris, rays, hits, num_rays, HAGRID_TRAVERSE_ANY_HIT));
}
inline void traverse_grid_with_uvs(const Grid& grid, const Tri* tris, const Ray* rays, Hit* hits, int num_rays) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_traverse_grid_ex(detail::current_ctx(), &p, tris, rays, hits, num_rays, HAGRID_TRAVERSE_UVS));
}

/// Extension: the k nearest intersections of every ray, sorted by (t, id), in hits[i * k .. i * k + k - 1]; unused slots are misses
/// (id -1, t = tmax).  1 <= k <= HAGRID_MAX_HITS; the semantics are in multi_hit.h and hagrid_amd.h (hagrid_traverse_grid_multi).
inline void traverse_grid_multi(const Grid& grid, const Tri* tris, const Ray* rays, Hit* hits, int num_rays, int k, bool with_uvs = false) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_traverse_grid_multi(detail::current_ctx(), &p, tris, rays, hits, num_rays, k, with_uvs ? HAGRID_TRAVERSE_UVS : 0u));
}

/// Extension: traverse_grid_multi over the triangles that TAKE PART for each ray (hagrid_amd.h: hagrid_traverse_grid_filtered; the rule: ray_filter.h).
/// filters: nullptr or one 8-byte record per ray (uint32 mask, int32 skip -- RayFilter of ray_filter.h); tri_masks: nullptr or one uint32 per triangle;
/// both DEVICE pointers.  any_hit needs k = 1: the ray stops at the first candidate the walk meets (occlusion rays with self-exclusion).
inline void traverse_grid_filtered(const Grid& grid, const Tri* tris, const Ray* rays, const void* filters, const uint32_t* tri_masks, Hit* hits,
                                   int num_rays, int k, bool with_uvs = false, bool any_hit = false) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_traverse_grid_filtered(detail::current_ctx(), &p, tris, rays, filters, tri_masks, hits, num_rays, k,
                                                                       (with_uvs ? HAGRID_TRAVERSE_UVS : 0u) | (any_hit ? HAGRID_TRAVERSE_ANY_HIT : 0u)));
}

/// Extension: nearest-surface queries (hagrid_amd.h: hagrid_closest_points; the arithmetic and the walk: closest.h).  points: num_points records of
/// 16 bytes (x, y, z, r), results: 32 bytes each ({qx, qy, qz, d2}, {int id, int feature, float side, 0}), counters: nullptr or int64[4] -- all DEVICE
/// pointers, 16-byte aligned.  Asynchronous on the context's stream.
inline void closest_points(const Grid& grid, const Tri* tris, const void* points, void* results, int num_points, void* counters = nullptr) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_closest_points(detail::current_ctx(), &p, tris, points, results, num_points, counters, 0u));
}

/// Extension: neighbour queries (hagrid_amd.h: hagrid_nearest_tris; the list and the walk: closest.h).  The k <= HAGRID_MAX_NEAREST nearest triangles within r
/// of every point, nearest first: entries (num_points * k records of 8 bytes {float d2, int id}) and / or records (num_points * k records of closest_points);
/// cursors: nullptr or one entry per point (only what sorts after it is listed), the labels: both or neither, counters: nullptr or int64[5] -- all DEVICE
/// pointers.  Asynchronous on the context's stream.
inline void nearest_tris(const Grid& grid, const Tri* tris, const void* points, int num_points, int k, void* entries, void* records = nullptr, const void* cursors = nullptr,
                         const int* query_labels = nullptr, const int* tri_labels = nullptr, void* counters = nullptr) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_nearest_tris(detail::current_ctx(), &p, tris, points, num_points, k, cursors, query_labels, tri_labels, entries, records, counters, 0u));
}

/// Extension: box-overlap queries (hagrid_amd.h: hagrid_overlap_boxes, hagrid_overlap_lattice; the test, the list and the walk: overlap.h).  boxes:
/// num_boxes records of 32 bytes (BBox with `first` in the pad slot after min), ids: num_boxes * k int32, counts: nullptr or num_boxes int32, counters:
/// nullptr or int64[4] -- all DEVICE pointers.  any: stop at the first triangle that meets the box (k must be 1).  Asynchronous on the context's stream.
inline void overlap_boxes(const Grid& grid, const Tri* tris, const BBox* boxes, int num_boxes, int k, int* ids, int* counts = nullptr, void* counters = nullptr, bool any = false) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_overlap_boxes(detail::current_ctx(), &p, tris, boxes, num_boxes, k, ids, counts, counters, any ? HAGRID_OVERLAP_ANY : 0u));
}
/// The voxels of an n.x * n.y * n.z lattice (x fastest; voxel c of an axis is [origin + float(c) * size, origin + float(c + 1) * size]) as the boxes.
inline void overlap_lattice(const Grid& grid, const Tri* tris, const vec3& origin, const vec3& size, const ivec3& n, int k, int* ids, int* counts = nullptr, void* counters = nullptr,
                            bool any = false) {
    hagrid_grid p = detail::to_pod(grid);
    const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {size.x, size.y, size.z};
    const int m[3] = {n.x, n.y, n.z};
    detail::check(detail::current_ctx(), hagrid_overlap_lattice(detail::current_ctx(), &p, tris, o, s, m, k, ids, counts, counters, any ? HAGRID_OVERLAP_ANY : 0u));
}
/// Extension: contact queries (hagrid_amd.h: hagrid_overlap_tris; the pair: tri_tri.h, the query: overlap.h).  queries: num_queries Tri records (may be
/// `tris`), first: nullptr or num_queries int32, query_labels (3 per query) and tri_labels (3 per scene triangle): both or neither; ids, counts, counters and
/// any as for overlap_boxes -- all DEVICE pointers.  Asynchronous on the context's stream.
inline void overlap_tris(const Grid& grid, const Tri* tris, const Tri* queries, int num_queries, int k, int* ids, int* counts = nullptr, void* counters = nullptr, bool any = false,
                         const int* first = nullptr, const int* query_labels = nullptr, const int* tri_labels = nullptr) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_overlap_tris(detail::current_ctx(), &p, tris, queries, num_queries, first, query_labels, tri_labels, k, ids, counts, counters,
                                                             any ? HAGRID_OVERLAP_ANY : 0u));
}
/// Extension: oriented-box queries (hagrid_amd.h: hagrid_overlap_obbs; the pair, the query and the prune: obb.h).  obbs: num_obbs records of 64 bytes
/// (c.xyz, first, u.xyz, 0, v.xyz, 0, w.xyz, 0), query_labels (1 per box) and tri_labels (3 per scene triangle): both or neither; ids, counts, counters and
/// any as for overlap_boxes -- all DEVICE pointers.  Asynchronous on the context's stream.
inline void overlap_obbs(const Grid& grid, const Tri* tris, const void* obbs, int num_obbs, int k, int* ids, int* counts = nullptr, void* counters = nullptr, bool any = false,
                         const int* query_labels = nullptr, const int* tri_labels = nullptr) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_overlap_obbs(detail::current_ctx(), &p, tris, obbs, num_obbs, query_labels, tri_labels, k, ids, counts, counters,
                                                             any ? HAGRID_OVERLAP_ANY : 0u));
}
/// Extension: overlap lists, stage 1 (hagrid_amd.h: hagrid_box_refs, hagrid_tri_refs, hagrid_obb_refs; the list type and the duplicate model: overlap.h).  Records
/// and labels as for overlap_boxes, overlap_tris and overlap_obbs.  offsets nullptr: count mode, counts[i] = the references of query i; else fill mode: the
/// references as entries {+0.0f, id} into [offsets[i], offsets[i + 1]) of `entries` (capacity slots of 8 bytes).  counters: nullptr or int64[6] -- all DEVICE
/// pointers.  hagrid_unique_lists and hagrid_compact_lists make the sorted lists of them.  Asynchronous on the context's stream.
inline void box_refs(const Grid& grid, const Tri* tris, const BBox* boxes, int num_boxes, int* counts, const long long* offsets = nullptr, void* entries = nullptr, int64_t capacity = 0,
                     void* counters = nullptr) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_box_refs(detail::current_ctx(), &p, tris, boxes, num_boxes, offsets, counts, entries, capacity, counters, 0u));
}
inline void tri_refs(const Grid& grid, const Tri* tris, const Tri* queries, int num_queries, int* counts, const long long* offsets = nullptr, void* entries = nullptr, int64_t capacity = 0,
                     void* counters = nullptr, const int* first = nullptr, const int* query_labels = nullptr, const int* tri_labels = nullptr) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_tri_refs(detail::current_ctx(), &p, tris, queries, num_queries, first, query_labels, tri_labels, offsets, counts, entries, capacity,
                                                         counters, 0u));
}
inline void obb_refs(const Grid& grid, const Tri* tris, const void* obbs, int num_obbs, int* counts, const long long* offsets = nullptr, void* entries = nullptr, int64_t capacity = 0,
                     void* counters = nullptr, const int* query_labels = nullptr, const int* tri_labels = nullptr) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_obb_refs(detail::current_ctx(), &p, tris, obbs, num_obbs, query_labels, tri_labels, offsets, counts, entries, capacity, counters, 0u));
}

/// Extension: crossing queries (hagrid_amd.h: hagrid_count_crossings, hagrid_list_crossings, hagrid_points_inside, hagrid_inside_lattice, hagrid_fill_lattice; the record, the paging and the walk:
/// crossings.h).  records: num_rays Hit-shaped records (count, t_first, length, winding bits); counters: nullptr or int64[4] -- DEVICE pointers.  Asynchronous.
inline void count_crossings(const Grid& grid, const Tri* tris, const Ray* rays, Hit* records, int num_rays, void* counters = nullptr) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_count_crossings(detail::current_ctx(), &p, tris, rays, records, num_rays, counters, 0u));
}
/// The crossings themselves, sorted by (t, id), 8 bytes each (float t; int32 key = id * 2 + entering): offsets = DEVICE int64[num_rays + 1] (CSR form, stride 0) or
/// nullptr with stride >= 1 (ray i owns stride slots); entries: `capacity` entries; records: nullptr or the records of count_crossings; counters: nullptr or
/// int64[6] -- DEVICE pointers.  Slots a list leaves over get (tmax, -1).  The semantics are in crossings.h and hagrid_amd.h (hagrid_list_crossings).  Asynchronous.
inline void list_crossings(const Grid& grid, const Tri* tris, const Ray* rays, int num_rays, const int64_t* offsets, int stride, void* entries, int64_t capacity,
                           Hit* records = nullptr, void* counters = nullptr) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_list_crossings(detail::current_ctx(), &p, tris, rays, num_rays, offsets, stride, entries, capacity, records, counters, 0u));
}
/// points: num_points records x, y, z, reach; dirs: nullptr (the three defaults) or num_dirs * 3 HOST floats; inside: num_points int32; records: nullptr or
/// num_points * m Hit-shaped records, direction fastest.
inline void points_inside(const Grid& grid, const Tri* tris, const void* points, int num_points, int* inside, const float* dirs = nullptr, int num_dirs = 0,
                          Hit* records = nullptr, void* counters = nullptr, bool winding = false) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(detail::current_ctx(), hagrid_points_inside(detail::current_ctx(), &p, tris, points, num_points, dirs, num_dirs, inside, records, counters,
                                                              winding ? HAGRID_INSIDE_WINDING : 0u));
}
/// the centres of the voxels of an n.x * n.y * n.z lattice (x fastest) as the points, reach +inf
inline void inside_lattice(const Grid& grid, const Tri* tris, const vec3& origin, const vec3& size, const ivec3& n, int* inside, const float* dirs = nullptr,
                           int num_dirs = 0, Hit* records = nullptr, void* counters = nullptr, bool winding = false) {
    hagrid_grid p = detail::to_pod(grid);
    const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {size.x, size.y, size.z};
    const int m[3] = {n.x, n.y, n.z};
    detail::check(detail::current_ctx(), hagrid_inside_lattice(detail::current_ctx(), &p, tris, o, s, m, dirs, num_dirs, inside, records, counters,
                                                               winding ? HAGRID_INSIDE_WINDING : 0u));
}
/// The inside of a closed surface on the lattice by scan lines, one ray per voxel row of every axis in `axes` (1 = x, 2 = y, 4 = z): hagrid_fill_lattice.  inside: one
/// int32 per voxel (1, 0, or -1 where no row was usable); workspace: one byte per voxel, needed with more than one axis; records: nullptr or the records of the row
/// rays; counters: nullptr or int64[5] -- DEVICE pointers.  winding (the recommended rule) counts leaving minus entering instead of the parity.
inline void fill_lattice(const Grid& grid, const Tri* tris, const vec3& origin, const vec3& size, const ivec3& n, int* inside, void* workspace, unsigned axes = 7u,
                         bool winding = true, Hit* records = nullptr, void* counters = nullptr) {
    hagrid_grid p = detail::to_pod(grid);
    const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {size.x, size.y, size.z};
    const int m[3] = {n.x, n.y, n.z};
    detail::check(detail::current_ctx(), hagrid_fill_lattice(detail::current_ctx(), &p, tris, o, s, m, axes, inside, workspace, records, counters,
                                                             winding ? HAGRID_INSIDE_WINDING : 0u));
}
/// Extension: the distance lattice by scatter (hagrid_amd.h: hagrid_distance_lattice; the key, the voxel box and its margin, tasks: distance.h): for every voxel
/// centre the answer of closest_points with r = band.  workspace: 8 bytes per voxel; ids (int32), d2 (float32), records (32 bytes, those of closest_points): one
/// per voxel, each may be nullptr but not all; counters: nullptr or int64[4] -- DEVICE pointers.
inline void distance_lattice(const Grid& grid, const Tri* tris, const vec3& origin, const vec3& size, const ivec3& n, float band, void* workspace, int* ids, float* d2,
                             void* records = nullptr, void* counters = nullptr) {
    hagrid_grid p = detail::to_pod(grid);
    const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {size.x, size.y, size.z};
    const int m[3] = {n.x, n.y, n.z};
    detail::check(detail::current_ctx(), hagrid_distance_lattice(detail::current_ctx(), &p, tris, o, s, m, band, workspace, ids, d2, records, counters, 0u));
}

/// Extension: independent batches in flight.  Every MemManager is a context with a stream of its own (hagrid_ctx_set_stream on
/// mem.context()); `share_traversal(dst, src)` lets `dst` traverse with the traversal image setup_traversal built in `src`, and the
/// overload below traverses on a named manager instead of the current one.  Two 1M-ray batches in flight take 0.118 ms each
/// instead of 0.177 ms (hagrid_amd.h: hagrid_share_traversal).
inline void share_traversal(MemManager& dst, MemManager& src) {
    detail::check(dst.context(), hagrid_share_traversal(dst.context(), src.context()));
}
inline void traverse_grid(MemManager& on, const Grid& grid, const Tri* tris, const Ray* rays, Hit* hits, int num_rays) {
    hagrid_grid p = detail::to_pod(grid);
    detail::check(on.context(), hagrid_traverse_grid(on.context(), &p, tris, rays, hits, num_rays));
}

} // namespace hagrid

#endif // HAGRID_TRAVERSE_H
