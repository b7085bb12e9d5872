/*
 * hagrid_amd.h -- C ABI of libhagrid_amd.so, the MI355X (gfx950) implementation of Hagrid's
 * irregular-grid construction and ray-traversal hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ types, no torch types.  Every entry
 * point names the reference interface it stands behind (paths relative to the reference's src/).  The
 * C++ API of the reference (build.h / traverse.h / mem_manager.h / profile) is provided on top of this
 * file as header-only shims in include/hagrid/ -- see INTEGRATION.md.
 *
 * Conventions
 *   - Every function returning int returns HAGRID_OK (0) or a negative HAGRID_E* code;
 *     hagrid_last_error(ctx) then holds "file(line): message" (the text the reference prints before
 *     abort(), common.h:103-108).  Nothing aborts behind the ABI; the C++ shims abort like the reference.
 *   - All Tri / Ray / Hit / grid array pointers are DEVICE pointers.  Grid arrays produced by the build
 *     passes come from the context's buffer pool and are released with hagrid_mem_free (main.cpp:496-498).
 *   - All work is enqueued on the context's HIP stream (default: the null stream, like the reference's
 *     <<<...>>> launches).  Build passes synchronise with the host where they need sizes; traversal is
 *     asynchronous.
 *   - HAGRID_ENOMEM (a device allocation failed; the library shares the device with whoever else fills it, so this is an ordinary event
 *     in a frame loop).  For EVERY entry point that can answer it: the context stays usable; hagrid_last_error names this failure;
 *     nothing the call allocated stays in use (the pool's books are what they were, minus what the call is documented to release);
 *     every pointer left in a descriptor is a live pool pointer that hagrid_mem_free accepts exactly once; no HIP error state is
 *     left behind for the next call.  What the descriptor and the caller's buffers ARE afterwards is one of two states, named at
 *     each entry point: "unchanged" (byte for byte what they were before the call, and still valid) or "released" (given back to
 *     the pool and NULL in the descriptor).  Some allocations are OPTIONAL (a pass runs without the buffer, only slower): their
 *     failure is not an error, the call answers HAGRID_OK with the same results.
 *   - One host thread per context.  Contexts are independent (the reference keeps per-TU __constant__
 *     state and therefore allows one grid per process: traverse.cu:7-12; here the traversal constants
 *     live in the context / the grid descriptor).
 */
#ifndef HAGRID_AMD_H
#define HAGRID_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HAGRID_ABI_VERSION 3   /* 3 (still): hagrid_nearest_tris was ADDED, nothing else moved; 3 (still): hagrid_distance_lattice was ADDED, nothing else moved; 3 (still): hagrid_list_crossings was ADDED, nothing else moved; 3 (still): hagrid_count_crossings, hagrid_points_inside and hagrid_inside_lattice were ADDED, nothing else moved; 3 (still): hagrid_mesh and the scene entry points (hagrid_scene_create ... hagrid_scene_bad_indices) were ADDED, nothing else moved; 3 (still): hagrid_traverse_grid_multi and hagrid_shade_layers were ADDED, nothing else moved; 3 (still): the frame entry points (hagrid_gen_primary_rays ... hagrid_render_frame) were ADDED, nothing else moved; 3: code-path selectors left hagrid_set_option (test library); 2: hagrid_traversal_stats grew by long_list_refs (64 bytes), hagrid_grid_broadcast checks the communicator */
#define HAGRID_MAX_LEVELS 32

enum {
    HAGRID_OK = 0,
    HAGRID_EINVAL = -1,   /* bad argument */
    HAGRID_EHIP = -2,     /* a HIP runtime call failed */
    HAGRID_ENOMEM = -3,   /* device allocation failed */
    HAGRID_ERANGE = -4,   /* a count does not fit the 30-bit entry / 31-bit index space */
    HAGRID_ENODEV = -5    /* no usable gfx950 device */
};

typedef struct hagrid_ctx hagrid_ctx;

/* Grid descriptor: the reference's `struct Grid` (grid.h:48-62) as a POD.  std::vector<int> offsets
 * becomes a fixed array + count. */
typedef struct hagrid_grid {
    void* entries;        /* uint32 words, log_dim | begin << 2     (grid.h:12-20) */
    void* ref_ids;        /* int32                                  (grid.h:50)    */
    void* cells;          /* 32-byte Cell records, NULL if compressed (grid.h:23-33) */
    void* small_cells;    /* 16-byte SmallCell records or NULL      (grid.h:36-45) */
    float bbox_min[3];
    float bbox_max[3];
    int32_t dims[3];      /* top-level resolution */
    int32_t num_cells;
    int32_t num_entries;
    int32_t num_refs;
    int32_t shift;
    int32_t num_offsets;
    int32_t offsets[HAGRID_MAX_LEVELS];
} hagrid_grid;

/* Per-batch traversal counters (exact integers; the algorithmic-bytes formula of DESIGN.md). */
typedef struct hagrid_traversal_stats {
    int64_t rays, rays_hit_grid, cells, entry_words, refs, sentinels, hits;
    int64_t long_list_refs;   /* of `refs`: tested in lists of more than four ids (shorter lists are inline in the traversal image) */
} hagrid_traversal_stats;

/* Sizes the construction passes of a context went through since its last hagrid_build_grid (diagnostics: the inputs of the
 * compulsory-traffic formula of SURVEY.md 8(d) "algorithmic bytes -- build"; bench.py: roofline_build). */
#define HAGRID_MAX_MERGE_PASSES 96
typedef struct hagrid_build_counts {
    int64_t num_tris, top_cells, top_refs;                 /* N, T, R0 (references emitted at the top level, before the SAT filter) */
    int32_t num_levels, merge_passes, expand_passes, compressed;
    int64_t level_refs[HAGRID_MAX_LEVELS];                 /* R_l: references entering level l */
    int64_t level_cells[HAGRID_MAX_LEVELS];                /* C_l: cells of level l */
    int64_t level_kept[HAGRID_MAX_LEVELS];                 /* references of level l that stay in a leaf (R_l - kept = split_l) */
    int64_t build_cells, build_refs, build_entries;        /* C, R, E after build_grid */
    int64_t merge_cells[HAGRID_MAX_MERGE_PASSES];          /* cells / references entering each merge axis pass */
    int64_t merge_refs[HAGRID_MAX_MERGE_PASSES];
    int64_t merged_cells, merged_refs;                     /* after merge_grid */
    int64_t flatten_entries_in, flatten_entries_out;       /* E, E' */
    int64_t expand_cells;                                  /* C of every expand axis pass */
    int64_t compress_cells, compress_refs_out;             /* compress_grid: C and R + sentinels */
} hagrid_build_counts;

/* ---- context ----------------------------------------------------------------------------------- */

int hagrid_abi_version(void);
/* 1 when the library was built with HAGRID_DEBUG_SYNC (every kernel launch of a pass is followed by a stream synchronisation and an
 * error check that aborts with "file(line): message", the reference's DEBUG_SYNC of common.h:95-108), else 0. */
int hagrid_debug_sync_enabled(void);

/* Creates a context on HIP device `device`.  keep != 0 is MemManager's keep mode (mem_manager.h:40-42):
 * freed buffers stay allocated for reuse by later builds. */
int hagrid_ctx_create(hagrid_ctx** out, int device, int keep);
void hagrid_ctx_destroy(hagrid_ctx* ctx);
/* Launch all further work on `stream` (a hipStream_t; NULL = null stream). */
int hagrid_ctx_set_stream(hagrid_ctx* ctx, void* stream);
/* Waits until all work queued on the context's stream is done (hipStreamSynchronize): for callers that keep several contexts in
 * flight and have no HIP of their own to wait with.  The reference synchronises with cudaDeviceSynchronize / event waits in
 * its front-end (main.cpp:414-425, profile.cu:5-18). */
int hagrid_ctx_synchronize(hagrid_ctx* ctx);
const char* hagrid_last_error(const hagrid_ctx* ctx);
/* Name / compute-unit count / memory of the context's device (diagnostics, bench records). */
int hagrid_device_info(const hagrid_ctx* ctx, char* name, int name_len, int* compute_units, int64_t* total_mem);

/* ---- MemManager backend (mem_manager.h:34-119, mem_manager.cu:6-75) -------------------------------- */
/* alloc<T>(n) -> hagrid_mem_alloc(n * sizeof(T)): best-fit reuse of a free slot, else hipMalloc. */
void* hagrid_mem_alloc(hagrid_ctx* ctx, size_t bytes);
/* free(ptr): NULL is a no-op; an untracked pointer is an error (the reference asserts). */
int hagrid_mem_free(hagrid_ctx* ctx, void* ptr);
/* copy<HST_TO_DEV | DEV_TO_HST | DEV_TO_DEV>; blocking like cudaMemcpy. */
int hagrid_mem_copy_h2d(hagrid_ctx* ctx, void* dst, const void* src, size_t bytes);
int hagrid_mem_copy_d2h(hagrid_ctx* ctx, void* dst, const void* src, size_t bytes);
int hagrid_mem_copy_d2d(hagrid_ctx* ctx, void* dst, const void* src, size_t bytes);
/* zero() / one() (memset 0x00 / 0xFF). */
int hagrid_mem_zero(hagrid_ctx* ctx, void* ptr, size_t bytes);
int hagrid_mem_one(hagrid_ctx* ctx, void* ptr, size_t bytes);
size_t hagrid_mem_usage(const hagrid_ctx* ctx);
size_t hagrid_mem_max_usage(const hagrid_ctx* ctx);
/* debug_slots(): prints the slot table to stdout. */
void hagrid_mem_debug_slots(const hagrid_ctx* ctx);

/* Diagnostics for the bench record (SURVEY.md 8(d) "BW_peak": a measured device copy / triad figure from the same run):
 * streams `bytes` per array through a float4 copy (c = a) and a triad (c = a + 3 b) kernel `iters` times and returns the best
 * rate of each in GB/s (copy: 2 * bytes, triad: 3 * bytes per pass). */
int hagrid_bandwidth_probe(hagrid_ctx* ctx, size_t bytes, int iters, float* copy_gbps, float* triad_gbps);
/* The sizes recorded by the construction passes of this context (see hagrid_build_counts). */
int hagrid_get_build_counts(const hagrid_ctx* ctx, hagrid_build_counts* out);

/* ---- profile (common.h:15, profile.cu:5-18) ------------------------------------------------------- */
/* Event pair on the context's stream around arbitrary host code; end returns the elapsed ms. */
int hagrid_profile_begin(hagrid_ctx* ctx);
float hagrid_profile_end(hagrid_ctx* ctx);

/* ---- construction (build.h:17-31) ------------------------------------------------------------------ */
/* build_grid (build.cu:718-760).  tris: 48-byte Tri records on the device.  grid is overwritten.
 * Admissible scenes: HAGRID_EINVAL for a triangle with a float that is not finite, or whose v0 - e1 or v0 + e2 is not finite
 * (hagrid_last_error names the smallest such index); nothing but the bounding-box pass has run by then.  HAGRID_ERANGE for finite triangles whose
 * scene-box extent is not finite, for a top-level grid, a level's references or cells, or the totals beyond 2^30 - 1 (true totals: a sum of 2^32 or
 * more is seen), and for 24 levels or more.  A scene whose box has no volume (a quad, a ground plane, coincident points) is built in a box widened
 * to 2^-10 of the scene's scale on its thin axes; that box is grid->bbox.  After a refusal *grid is as it was, the context stays usable and the pool's
 * usage is unchanged.  HAGRID_ENOMEM, in whichever level of the construction: the same -- *grid is UNCHANGED byte for byte (it is written when the last
 * kernel has run), every temporary and every output array already taken is back in the pool.  Optional: the one buffer the temporaries of a context's
 * later constructions are carved from.  Grids of 16 to 23 levels (grid->shift > 15) are built, and hagrid_merge_grid, hagrid_flatten_grid and hagrid_expand_grid accept
 * them; hagrid_compress_grid returns 0, and every traversal, query and blob call -- hagrid_setup_traversal, hagrid_grid_release_for_traversal,
 * hagrid_grid_pack and hagrid_grid_save included -- answers HAGRID_EINVAL ("bad shift") before it launches or writes anything. */
int hagrid_build_grid(hagrid_ctx* ctx, const void* tris, int num_tris, hagrid_grid* grid,
                      float top_density, float snd_density);
/* merge_grid (merge.cu:331-377).  On HAGRID_ENOMEM and HAGRID_EHIP the grid is gone: cells and ref_ids are RELEASED and NULL in the
 * descriptor, num_cells = num_refs = 0 (the voxel map may already name the new cells); entries stay the caller's to free.  That holds for
 * every allocation of the pass -- the nine working buffers in front of the first kernel as well as the status words of a scan in a late
 * iteration: one state, whenever it happens.  A refused argument (HAGRID_EINVAL) leaves the grid alone. */
int hagrid_merge_grid(hagrid_ctx* ctx, hagrid_grid* grid, float alpha);
/* flatten_grid (flatten.cu:109-175).  HAGRID_ENOMEM: the grid is UNCHANGED -- the pass collapses the voxel map in a working copy and
 * swaps grid->entries (releasing the old map) only when everything has run. */
int hagrid_flatten_grid(hagrid_ctx* ctx, hagrid_grid* grid);
/* expand_grid (expand.cu:199-225).  HAGRID_ENOMEM (the second cell buffer, the flags): the grid is UNCHANGED; nothing was launched.
 * Optional: the list of cells of the later iterations, the voxel map resolved into one word per voxel. */
int hagrid_expand_grid(hagrid_ctx* ctx, hagrid_grid* grid, const void* tris, int iters);
/* compress_grid (compress.cu:38-63): returns 1 when compressed, 0 when the virtual resolution does not
 * fit 16 bits (grid untouched), negative on error.  HAGRID_ENOMEM: the grid is UNCHANGED (cells and ref_ids are released only when
 * the small cells and their references stand). */
int hagrid_compress_grid(hagrid_ctx* ctx, hagrid_grid* grid);

/* ---- the grid as one buffer: multi-GPU broadcast and save / load (no reference counterpart) -------------- */
/* Blob = header (256 bytes) + entries + cells | small_cells + ref_ids + triangles, every section 128-byte aligned.  The same bytes
 * are the file form.  Little-endian, offsets in bytes from the start of the blob. */
typedef struct hagrid_blob_header {
    uint32_t magic, version;                       /* "HGRB", 1 */
    int32_t dims[3], shift;
    int32_t num_cells, num_entries, num_refs, num_tris;
    int32_t compressed, num_offsets;
    int32_t offsets[HAGRID_MAX_LEVELS];
    float bbox_min[3], bbox_max[3];
    uint64_t off_entries, off_cells, off_refs, off_tris, total_bytes;
    uint8_t reserved[16];
} hagrid_blob_header;
/* Size of the blob of `grid` with `num_tris` triangles (0 for an incomplete grid). */
size_t hagrid_grid_blob_bytes(const hagrid_grid* grid, int num_tris);
/* Copies grid + triangles into one new pool buffer (device-to-device); release it with hagrid_mem_free.  HAGRID_ENOMEM: *blob is NULL,
 * *bytes is not written, grid and triangles are UNCHANGED (they are only read). */
int hagrid_grid_pack(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, int num_tris, void** blob, size_t* bytes);
/* Turns a blob held in a pool buffer of this context into a grid IN PLACE: the buffer is split into the four arrays, which from then
 * on are ordinary pool buffers (grid->entries, grid->cells | small_cells, grid->ref_ids, *tris: each released with hagrid_mem_free, in
 * any order, like the arrays of a built grid); `blob` itself must not be freed afterwards.  Nothing is copied and nothing is allocated: the
 * call cannot answer HAGRID_ENOMEM. */
int hagrid_grid_unpack(hagrid_ctx* ctx, void* blob, size_t bytes, hagrid_grid* grid, void** tris, int* num_tris);
/* The blob as a file.  HAGRID_ENOMEM (save: the blob, or host memory for it; load: host memory, or the pool buffer the file goes into): save has
 * written no file and leaves grid and triangles UNCHANGED; load leaves *grid, *tris and *num_tris UNCHANGED (they are written by the
 * unpacking, last) and keeps no buffer. */
int hagrid_grid_save(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, int num_tris, const char* path);
int hagrid_grid_load(hagrid_ctx* ctx, const char* path, hagrid_grid* grid, void** tris, int* num_tris);
/* One process per GPU: rank `root` passes its grid and triangles (they stay untouched), every other rank receives them (grid, *tris,
 * *num_tris are outputs there, arrays owned as after hagrid_grid_unpack).  `comm` is an ncclComm_t of RCCL spanning the ranks; two
 * ncclBroadcast calls on the context's stream: the 256-byte header, then the blob, straight from / into pool memory.  RCCL is
 * looked up in the running process (the copy PyTorch or the host program loaded, else /opt/rocm/lib/librccl.so).  Blocking.
 * HAGRID_ENOMEM for the blob (the root's pack, a receiver's buffer) is agreed among the ranks before the blob travels: every rank answers an
 * error and keeps no buffer; the receivers' *grid, *tris and *num_tris are UNCHANGED.  The call's own 260 bytes are taken in front of the first
 * collective: a rank that cannot get them answers HAGRID_ENOMEM at once, and the other ranks wait for it in the collective. */
int hagrid_grid_broadcast(hagrid_ctx* ctx, void* comm, int rank, int root, hagrid_grid* grid, void** tris, int* num_tris);

/* ---- traversal (traverse.h:11-14) ------------------------------------------------------------------- */
/* setup_traversal (traverse.cu:97-109): prepares the traversal state of `grid`.  The reference uploads constants; here
 * the constants travel with every launch and this call builds the TRAVERSAL IMAGE of the grid in the context (one per
 * context: the grid of the last call): ONE 16-byte record per cell step -- the cell's bounds as byte offsets, the reference ids of
 * lists of up to four (20-bit ids) or three (26-bit ids) inline -- so that a cell step is one dependent gather instead of
 * entry -> entry -> cell, and the reference-id gather disappears for short lists.  Three layouts (hagrid_amd/csrc/trav_image.hip):
 * grids of at most three levels get a block of records per top-level cell, indexed by the voxel -- found by arithmetic where
 * (nearly) every top-level cell has the full depth (uniform layout), through a table otherwise (table layout); every other grid
 * gets a record per voxel-map entry at the entry's index (general layout: inner entries are links to their child blocks, and the
 * kernel keeps the innermost block a ray is in -- one gather per step at any depth).  Cells whose bounds a byte cannot hold (the
 * large cells of empty space) get a wide record in the table and general layouts.  "traverse.image" = 0 builds nothing (traversal
 * reads the construction format); 1 and 2 build the image (1 was round 1-4's compact form and is kept as a value).  An image that
 * would exceed max(1 GB, 8x the entries + cells it replaces) ("traverse.image_max_mb") is not built, nor is one for a grid no layout
 * describes (a virtual resolution of 65536 per axis, reference ids beyond 26 bits, a list of 2^20 ids).
 * hagrid_traverse_grid uses the image when it is called with the same grid (same arrays, same counts); the image is
 * dropped when a construction pass runs in this context or when one of the grid's arrays is freed or overwritten through
 * this API; without an image traversal reads the construction format.  Hits are identical either way.  Synchronous (size / fit
 * read-backs); 0.3 ms and 129 MB for the 1M-triangle scene of BASELINE.md.
 * HAGRID_ENOMEM: the grid is UNCHANGED (it is only read) and the context holds NO traversal image -- the image of an earlier call is dropped
 * first, every buffer of the unfinished one is back in the pool -- so hagrid_traverse_grid still works and reads the construction format.  The
 * call does not end "OK without an image" for lack of memory: that answer is kept for grids no layout describes.  Optional: the compact layout
 * that is built next to a much bigger uniform one. */
int hagrid_setup_traversal(hagrid_ctx* ctx, const hagrid_grid* grid);
/* Extension: after hagrid_setup_traversal built the image of `grid` (no layout refers to the voxel map), the
 * caller may give the construction format up: entries and cells | small_cells are released to the pool and set to NULL in the
 * descriptor, the image answers for them (1M-triangle scene: 166 MB of 365 MB).  hagrid_traverse_grid[_ex] keep working with that
 * descriptor; what reads the construction format (construction passes, hagrid_traverse_grid_stats, hagrid_grid_pack, forced kernel
 * variants) is refused.  ref_ids and the triangles stay with the caller as before. */
int hagrid_grid_release_for_traversal(hagrid_ctx* ctx, hagrid_grid* grid);
/* Extension: independent batches in flight.  A launch over a SMALL batch (1M rays) keeps the machine full for the first half of its
 * time only; the second half is the drain of its last wavefronts.  A caller with independent batches (tiles of a frame, samples,
 * frames) fills that drain by giving every batch in flight its own context = its own stream (hagrid_ctx_set_stream): contexts are
 * independent.  This call lets `dst` traverse with the traversal image hagrid_setup_traversal built in `src` (same device) instead
 * of building a copy of its own -- one image in the caches, however many streams.  The image stays the property of `src`: it
 * must outlive its use in `dst`, and after the next hagrid_setup_traversal / construction pass / free of the grid in `src` the
 * share must be renewed (hagrid_setup_traversal(dst, ...) or a construction pass in `dst` ends it too).  Waits for `src`'s stream.
 * Measured, 1M-triangle scene, 1024 x 1024 primary rays: 0.177 ms per batch with one in flight, 0.118 ms with two
 * (profiles/dev_r2_inflight.txt). */
int hagrid_share_traversal(hagrid_ctx* dst, hagrid_ctx* src);
/* traverse_grid (traverse.cu:111-117): rays 32-byte Ray records, hits 16-byte Hit records.
 * hits[i].id = primitive id or -1, hits[i].t = distance (tmax on a miss), u = v = 0.  Asynchronous.
 * Rays are taken as they are.  A ray with a NaN or infinite org / dir component, a NaN tmin / tmax, or a dir with no component whose float32 reciprocal is finite
 * ((+-0, +-0, +-0), or every component below about 2.94e-39) is a MISS that takes no
 * cell step: id -1, t = the bits of its tmax, u = v = 0 (multi-hit: k such records), whatever else the batch holds; +-inf are valid tmin / tmax; the
 * sign of a zero dir component changes no result (include/hagrid/ray.h admit_ray).
 * HAGRID_ENOMEM (only with hagrid_set_ray_binning: the permutation, the keys, the bin table, its partial sums, the words of the automatic mode,
 * the status words of the scan): the traversal kernel was not launched, so `hits` is UNCHANGED -- not one byte written -- and so are grid, tris and
 * rays; the binning buffers are back in the pool.  Optional (the launch keeps its default order): the row scores and the tile-order buffer of a ray buffer. */
int hagrid_traverse_grid(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris,
                         const void* rays, void* hits, int num_rays);
/* Variants of the same walk (no separate entry point in the reference).  flags:
 *   HAGRID_TRAVERSE_ANY_HIT  a ray is finished at its FIRST accepted intersection in traversal order (cells along the ray,
 *                            references in list order): shadow / occlusion rays.  hits[i].id >= 0 exactly when the nearest-hit
 *                            traversal finds a hit; id and t are those of that first intersection.
 *   HAGRID_TRAVERSE_UVS      hits[i].u, hits[i].v = barycentrics of the hit, as the reference stores them when it is compiled
 *                            with COMPUTE_UVS (prims.h:285-288).
 * flags = 0 is hagrid_traverse_grid. */
#define HAGRID_TRAVERSE_ANY_HIT 1u
#define HAGRID_TRAVERSE_UVS 2u
int hagrid_traverse_grid_ex(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris,
                            const void* rays, void* hits, int num_rays, uint32_t flags);
/* Same traversal, additionally: steps[i] (device int32, may be NULL) = the reference's per-ray step
 * count (traverse.cu:80,93), and *stats (host, may be NULL) = batch totals.  Synchronous.
 * HAGRID_ENOMEM (the eight counters, taken only when stats is given): nothing was launched; hits and steps are UNCHANGED, *stats is all zeroes. */
int hagrid_traverse_grid_stats(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris,
                               const void* rays, void* hits, int num_rays,
                               void* steps, hagrid_traversal_stats* stats);

/* Extension (no reference counterpart): MULTI-HIT traversal -- the first k surfaces along every ray, sorted (transparency, x-ray
 * pictures, thickness and inside / outside queries).  An INTERSECTION of ray i with triangle j exists exactly when
 * intersect_prim_ray(tri[j], Ray(org, tmin, dir, tmax), j, h) of include/hagrid/prims.h accepts it with the ray's own, unshrunk tmin
 * and tmax; its value is h.t (with HAGRID_TRAVERSE_UVS also h.u, h.v).  hits holds num_rays * k 16-byte Hit records: hits[i*k ..
 * i*k + k-1] are the min(k, number of intersections) intersections of ray i that are smallest in the order (t ascending, then id
 * ascending), in that order; unused slots hold id = -1, t = tmax, u = v = 0 (a miss of hagrid_traverse_grid); an inactive ray
 * (tmax = -1) gets k such slots.  So:
 *   - the list for k is a prefix of the list for k + 1;
 *   - k = 1 is NOT promised to equal hagrid_traverse_grid bit for bit: the nearest-hit walk shrinks tmax in its scaled comparison and
 *     breaks ties in t by list order (the two differ in a ray or two of ten thousand on a mesh);
 *   - calling hagrid_traverse_grid k times with tmin = nextafter(t) is NOT this query: intersect_prim_ray compares t with
 *     abs_det * tmin in the scaled domain, so the triangle just found is accepted again.  (hagrid_traverse_grid_filtered below continues a
 *     ray past a hit: tmin = t and skip = the triangle just found.)
 * flags: 0 or HAGRID_TRAVERSE_UVS.  Asynchronous on the context's stream.  One launch walks the CONSTRUCTION format in buffer order
 * with the list in registers (hagrid_amd/csrc/trav_multi.hip): the traversal image, hagrid_set_ray_binning, tile packets and the
 * learned tile order are not applied, and the hints kept for the nearest-hit path stay untouched.  HAGRID_EINVAL: k < 1 or
 * k > HAGRID_MAX_HITS; any flag other than HAGRID_TRAVERSE_UVS (HAGRID_TRAVERSE_ANY_HIT contradicts k hits); a grid released by
 * hagrid_grid_release_for_traversal; a context with "traverse.id_is_steps" = 1.  HAGRID_ERANGE: num_rays * k beyond 2^31 - 1.
 * num_rays = 0 is HAGRID_OK. */
#define HAGRID_MAX_HITS 8
int hagrid_traverse_grid_multi(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris,
                               const void* rays, void* hits, int num_rays, int k, uint32_t flags);

/* Extension (no reference counterpart): FILTERED traversal -- hagrid_traverse_grid_multi in which every ray says which triangles it sees
 * (Embree's ray mask, the visibility masks of OptiX / DXR, "ignore the primitive I start on"): shadow rays that leave from a surface with
 * tmin = 0 and no epsilon, a ray continued past the hit it just reported, a sensor that does not see its own body.
 *   filters    DEVICE, 8 bytes per ray, 8-byte aligned: uint32 mask, int32 skip.  NULL: mask = HAGRID_RAY_MASK_ALL and no skip for every
 *              ray.  skip < 0 (any negative value) skips nothing, and so does a skip that names no triangle.
 *   tri_masks  DEVICE, uint32 per triangle of the array the grid was built over, 4-byte aligned.  NULL: all ones.  Its length is the
 *              caller's business, as with tris.
 * Triangle j TAKES PART for ray i exactly when (mask_i & tri_masks[j]) != 0 and j != skip_i (include/hagrid/ray_filter.h).  The CANDIDATES of
 * ray i are the intersections of hagrid_traverse_grid_multi -- the same acceptance, the ray's own, unshrunk window -- with the triangles that
 * take part.  hits has exactly that entry point's layout: ray i gets k records, the min(k, m) smallest of its m candidates in the order
 * (t ascending, then id ascending), unused slots id = -1, t = tmax, u = v = 0.  So:
 *   - the list for k is a prefix of the list for k + 1;
 *   - the answer equals the unfiltered answer over the scene with the triangles that take no part deleted, ids unchanged;
 *   - a ray with mask == 0 takes no cell step and gets k empty slots; inactive and inadmissible rays are treated as in multi-hit;
 *   - with filters == NULL, tri_masks == NULL and no HAGRID_TRAVERSE_ANY_HIT the output is that of hagrid_traverse_grid_multi, bit for bit.
 * flags: HAGRID_TRAVERSE_UVS and HAGRID_TRAVERSE_ANY_HIT.  Any-hit needs k = 1: the ray stops behind the first cell in which the walk met a
 * candidate; hits[i].id >= 0 exactly when the candidate set is not empty, and id and t are those of SOME candidate, t that pair's own t bit for
 * bit (the contract of HAGRID_OVERLAP_ANY: which candidate is not promised).  It is the occlusion ray with self-exclusion: skip = the triangle the ray starts on, tmin = 0.
 * A mode of the multi-hit kernel (hagrid_amd/csrc/trav_multi.hip), asynchronous on the context's stream: the traversal image, ray binning,
 * tile packets, the learned tile order and the hints kept for the nearest-hit path are neither used nor touched.  Errors: everything
 * hagrid_traverse_grid_multi refuses, with the same codes (k < 1 or k > HAGRID_MAX_HITS, a released grid, "traverse.id_is_steps" = 1,
 * HAGRID_ERANGE for num_rays * k beyond 2^31 - 1, the level limit of the grid); HAGRID_EINVAL in addition for HAGRID_TRAVERSE_ANY_HIT with
 * k != 1, an unknown flag, misaligned filters or tri_masks.  num_rays = 0 is HAGRID_OK. */
#define HAGRID_RAY_MASK_ALL 0xFFFFFFFFu
int hagrid_traverse_grid_filtered(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris,
                                  const void* rays, const void* filters, const void* tri_masks,
                                  void* hits, int num_rays, int k, uint32_t flags);

/* Extension (no reference counterpart): NEAREST-SURFACE queries -- for every point of a batch the triangle nearest to it, how far it is and where
 * on it (distance fields, contact and collision in simulation loops, snapping points to a surface; Embree's rtcPointQuery, Open3D's
 * compute_closest_points).  points holds 16 bytes per query: float32 x, y, z, r.  results holds 32 bytes per query:
 *   {float32 qx, qy, qz, d2}, {int32 id, int32 feature, float32 side, 0}.
 * The squared distance d2_j from p to triangle j, the closest point q, the feature that holds it (0 face, 1 / 2 / 3 edge v0v1 / v1v2 / v2v0, end
 * points included) and side = sign(dot(p - q, n)) as +1, -1 or 0 are what point_tri and tri_side of include/hagrid/closest.h compute: float32
 * without contraction, operation for operation (hagrid_amd/scene.py: closest_points states the same in numpy -- the same bits).  side is the sign
 * of the FACE normal of the winning triangle, not a robust inside / outside at edges and vertices.  A triangle whose stored normal is (0, 0, 0)
 * has no surface and takes no part (the degenerate triangles hagrid_scene_assemble makes for bad indices are such); a NaN d2 is never accepted.
 * With r2 = r * r (+inf allowed) the answer is, among all triangles with d2_j <= r2, the smallest in the order (d2 ascending, id ascending);
 * if there is none: id -1, d2 = r2, q = p, feature = side = 0.  r < 0 is an INACTIVE query (id -1, d2 = -1); a NaN coordinate gives id -1.
 * One launch walks the CONSTRUCTION format from the cell that holds p outwards and prunes only what cannot win, so the results are those of the
 * brute force over all triangles, bit for bit (the argument: include/hagrid/closest.h).  The traversal image, ray binning and
 * the hints kept for the nearest-hit path are neither used nor touched.  counters: NULL, or DEVICE int64[4] to which the batch totals are ADDED
 * (queries, cells visited, triangles tested, sub-blocks pruned): clear it first.  Asynchronous on the context's stream.
 * HAGRID_EINVAL: a null grid, null or misaligned (16 bytes; counters 8) buffers, flags != 0, num_points < 0, a grid released by
 * hagrid_grid_release_for_traversal.  num_points = 0 is HAGRID_OK (null buffers are then fine). */
int hagrid_closest_points(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* points, void* results,
                          int num_points, void* counters, uint32_t flags);

/* Extension (no reference counterpart): NEIGHBOUR queries -- for every point of a batch the k NEAREST triangles within its radius, nearest first, paged
 * (a particle of radius r against a mesh needs every triangle within r; the vertex-face proximity pairs of a cloth step; blending and voting over several
 * neighbours).  points are the records of hagrid_closest_points (x, y, z, r; r2 = r * r, +inf allowed); d2 is point_tri's, the same bits.  Triangle j is a
 * CANDIDATE of query i when it has a surface (stored normal != 0), its d2 is not NaN, d2 <= r2, the pair is not skipped by the labels, and (d2, j) sorts
 * strictly AFTER the query's cursor in the order (d2 ascending, id ascending).  With m candidates and 1 <= k <= HAGRID_MAX_NEAREST:
 *   entries  DEVICE, 8 bytes per slot {float32 d2; int32 id}, 8-byte aligned (NULL if records is given): the slots [i*k, i*k + k) hold the min(k, m)
 *            smallest candidates in that order; unused slots d2 = r2, id -1.  An INACTIVE query (r < 0): k slots d2 = -1, id -1.  A NaN coordinate or a
 *            NaN radius: id -1, d2 = r2 everywhere.
 *   records  NULL, or DEVICE k x 32 bytes per query, 16-byte aligned: slot (i, j) holds the 32-byte record of hagrid_closest_points for that triangle
 *            (q, d2, id, feature, side); an unused slot q = p, the slot's d2, id -1, feature = side = 0.
 *   cursors  NULL (no cursor for anyone), or DEVICE 8 bytes per query in the entry layout, 8-byte aligned.  A cursor with d2 = -1 excludes nothing (every
 *            candidate has d2 >= 0); a cursor with a NaN d2 excludes everything.  The cursor for page n + 1 is the LAST slot of page n.  A list that is
 *            not full is the last page: its empty entry (id -1, d2 = r2) is NOT to be used as a cursor -- it would exclude nothing it should.
 *   query_labels DEVICE int32[num_points], tri_labels DEVICE int32[3 per scene triangle], both given or both NULL, 4-byte aligned: pair (i, j) is SKIPPED
 *            when query_labels[i] >= 0 equals one of triangle j's three labels.  With a mesh's vertices as queries, label = vertex index and the mesh's
 *            index triples as triangle labels a vertex does not see the triangles it belongs to (the convention of hagrid_overlap_tris).
 * Promises: the list for k is a prefix of the list for k + 1; the pages concatenated are the full sorted list of all candidates; the answer is that of the
 * brute force over all triangles (hagrid_amd/scene.py: nearest_tris), and that of the unlabelled query over the scene with the skipped triangles deleted,
 * ids unchanged; with k = 1, no cursor and no labels, entries are (d2, id) of hagrid_closest_points and records its whole 32-byte output, bit for bit.
 * THIS entry point has no exact count of the ball's content and no "k + 1 says more": the walk prunes at the k-th best and never sees the rest.  A full list
 * means "ask again"; the whole ball at once, counted and in CSR form, is hagrid_ball_refs below.  counters: NULL, or DEVICE int64[5] (8-byte aligned) to which the batch totals are ADDED: queries, cells visited, triangles tested,
 * sub-blocks pruned, lists that came back full -- the last one tells a paging caller with one scalar whether another page is needed.
 * Asynchronous on the context's stream; walks the CONSTRUCTION format (include/hagrid/closest.h); the traversal image, ray binning and the
 * hints kept for the nearest-hit path are neither used nor touched.  HAGRID_EINVAL: everything hagrid_closest_points refuses (a released grid, a bad
 * shift), k < 1 or k > HAGRID_MAX_NEAREST, any flag, entries and records both NULL, one label array without the other, a misaligned buffer.
 * HAGRID_ERANGE: num_points * k beyond 2^31 - 1.  num_points = 0 is HAGRID_OK (null buffers are then fine). */
#define HAGRID_MAX_NEAREST 8
int hagrid_nearest_tris(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* points, int num_points, int k,
                        const void* cursors, const void* query_labels, const void* tri_labels, void* entries, void* records,
                        void* counters, uint32_t flags);

/* Extension (no reference counterpart): BALL LISTS -- EVERY triangle within r of each point, sorted, in CSR form, without paging (radius-neighbour lists:
 * particle-mesh contact, cloth proximity, blending over all neighbours).  Additive: HAGRID_ABI_VERSION stays 3.  The list of query i is the candidates of
 * hagrid_nearest_tris without a cursor, ALL of them, in the order (d2 ascending, id ascending), d2 point_tri's bits, labels as there; r < 0, a NaN coordinate
 * or a NaN radius gives an empty list.  Three staged, asynchronous entry points; the caller owns every buffer and both scans (none of them asks for memory):
 *   hagrid_ball_refs (count) -> exclusive scan -> hagrid_ball_refs (fill) -> hagrid_unique_lists -> exclusive scan -> hagrid_compact_lists.
 * An entry is 8 bytes {float32 d2; int32 id} as hagrid_nearest_tris'; the EMPTY entry is {+inf, -1}.  A SEGMENT i of a buffer of `capacity` entries is the
 * slots [offsets[i], offsets[i + 1]) (offsets DEVICE int64[n + 1], 8-byte aligned): its ROOM is the range's length, and 0 if that is negative or the range
 * leaves [0, capacity] -- the rule of hagrid_list_crossings.  Nothing outside a segment is read or written.
 *
 * hagrid_ball_refs: the walk of hagrid_nearest_tris with a bound that stays r2 (include/hagrid/closest.h, "the whole ball").  A REFERENCE of query i is one
 * accepted offer: a triangle arrives once per visit of a cell that lists it, so R_i, the number of references, is a property of the grid and the walk, not of
 * the scene; R_i >= m_i, the list's length; the ids among the references are exactly the candidates; equal ids carry equal d2 bits.
 *   count mode  offsets NULL, entries NULL, capacity 0: counts[i] = R_i (counts DEVICE int32[num_points], 4-byte aligned).
 *   fill mode   offsets given: the first min(R_i, room) references in walk order, then the EMPTY entry in every slot left over; counts may be NULL.  With
 *               offsets the exclusive sums of count mode's counts every slot is written exactly once.
 *   counters    NULL, or DEVICE int64[6] ADDED to: queries, cells visited, triangles tested, sub-blocks pruned, references written, queries with R_i > room
 *               (count mode adds 0 to the last two).
 * HAGRID_EINVAL: everything hagrid_nearest_tris refuses of its grid, points, labels and flags; a negative capacity; count mode with entries or a capacity;
 * count mode without counts; fill mode with entries NULL and capacity > 0; a misaligned buffer.  num_points = 0 is HAGRID_OK.
 *
 * hagrid_unique_lists (needs no grid; include/hagrid/unique_lists.h): every segment in place -- entries with id < 0 or a NaN d2 are dropped, the rest sorted
 * by (d2 by float comparison, id), entries equal in id reduced to one (CONTRACT: equal ids in one segment carry equal d2 bits), the m_i survivors at the front,
 * EMPTY in every other slot, counts[i] = m_i (DEVICE int32[num_lists]).  counters: NULL, or DEVICE int64[4] ADDED to: lists, slots, survivors, lists sorted
 * in global memory (longer than the on-chip capacity).
 * hagrid_compact_lists: copies the first min(counts[i], room of the source, room of the destination) entries of segment i to out_offsets[i] of out_entries
 * and fills the rest of the destination's room with EMPTY.  counters: NULL, or DEVICE int64[4] ADDED to: lists, entries copied, lists cut short, 0.
 * Both: HAGRID_EINVAL for a flag, negative num_lists or capacity, NULL offsets or counts, NULL entries with a capacity > 0, a misaligned buffer. */
int hagrid_ball_refs(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* points, int num_points,
                     const void* query_labels, const void* tri_labels, const void* offsets, void* counts, void* entries,
                     int64_t capacity, void* counters, uint32_t flags);
int hagrid_unique_lists(hagrid_ctx* ctx, int num_lists, const void* offsets, void* entries, int64_t capacity, void* counts,
                        void* counters, uint32_t flags);
int hagrid_compact_lists(hagrid_ctx* ctx, int num_lists, const void* offsets, const void* entries, int64_t capacity,
                         const void* counts, const void* out_offsets, void* out_entries, int64_t out_capacity, void* counters,
                         uint32_t flags);

/* Extension (no reference counterpart): CAPSULE queries -- for every SEGMENT of a batch the k nearest triangles within its radius, nearest first, paged
 * (the edge-edge half of a cloth or rod step's proximity pairs; a character's or a robot link's capsule; "does this cable, or this line of sight, clear
 * the mesh by r").  An additive extension: HAGRID_ABI_VERSION stays 3.  segments holds 32 bytes per query, 16-byte aligned:
 *   float32 ax, ay, az, r;  bx, by, bz, 0.
 * r2 = r * r (+inf allowed).  d2 is the squared distance between the segment a -> b and the triangle as seg_tri of include/hagrid/capsule.h computes it:
 * float32 without contraction, operation for operation (hagrid_amd/scene.py: segment_pairs, segment_tris state the same in numpy -- the same bits), the
 * smallest of: the two ends against the triangle (point_tri), the segment against the triangle's three edges, and 0 where the segment pierces the face.
 * With a == b it is point_tri's d2, bit for bit.  r < 0 is an INACTIVE query (k slots d2 = -1, id -1); a NaN or infinite coordinate or a NaN radius gives
 * id -1, d2 = r2 everywhere; neither walks.  entries, cursors, the candidate rule, the order (d2 ascending, id ascending), unused slots (d2 = r2, id -1),
 * 1 <= k <= HAGRID_MAX_NEAREST and paging are exactly those of hagrid_nearest_tris.
 *   query_labels DEVICE int32[2 per segment] (the edge's two vertex indices; -1: an unused slot), tri_labels DEVICE int32[3 per scene triangle], both
 *            given or both NULL: pair (i, j) is SKIPPED when one of the query's labels >= 0 equals one of triangle j's three.  With a mesh's own edges
 *            as queries and its index triples as triangle labels an edge does not see the triangles that share a vertex with it.
 *   records  NULL, or DEVICE k x 32 bytes per query, 16-byte aligned: {float32 qx, qy, qz, d2}, {int32 id, int32 feature, float32 side, float32 s} --
 *            the record of hagrid_closest_points with s in the word that is 0 there.  q is the closest point ON THE TRIANGLE, s in [0, 1] the parameter
 *            of the closest point c = a + (b - a) * s ON THE SEGMENT, feature 0 face / 1, 2, 3 edge (as hagrid_closest_points) / 4 the segment pierces
 *            the face (d2 = 0, q = the point of piercing), side = sign(dot(c - q, n)).  An unused slot: q = a, the slot's d2, id -1, feature = side = 0,
 *            s = +0.  Made again from the winners' ids after the walk.
 *   counters NULL, or DEVICE int64[5] as hagrid_nearest_tris: queries, cells visited, triangles tested, sub-blocks pruned, lists that came back full.
 * Promises: the lists are those of the brute force over all triangles, bit for bit; the list for k is a prefix of the list for k + 1; the pages
 * concatenated are all candidates, sorted; the labelled answer is the unlabelled answer over the scene without the skipped triangles, ids unchanged;
 * with a == b, the first label of each pair set and the second -1, entries and records are hagrid_nearest_tris' for the points (a, r), bit for bit --
 * hence at k = 1 without cursor or labels hagrid_closest_points' output.  This entry point has no exact count of the capsule's content (as hagrid_nearest_tris; ball lists are for points).
 * Asynchronous on the context's stream; walks the CONSTRUCTION format (include/hagrid/capsule.h); the traversal image, ray binning and the
 * hints kept for the nearest-hit path are neither used nor touched.  HAGRID_EINVAL and HAGRID_ERANGE (num_segments * k beyond 2^31 - 1): everything
 * hagrid_nearest_tris refuses.  num_segments = 0 is HAGRID_OK (null buffers are then fine). */
int hagrid_segment_tris(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* segments, int num_segments, int k,
                        const void* cursors, const void* query_labels, const void* tri_labels, void* entries, void* records,
                        void* counters, uint32_t flags);

/* Extension (no reference counterpart): BOX-OVERLAP queries -- for every axis-aligned box of a batch, which triangles meet it (contact candidates,
 * culling, sparse-volume allocation, surface voxelization).  Triangle j MEETS the box [lo, hi] exactly when intersect_tri_box<true, true>(v0, e1, e2, n,
 * lo, hi) of include/hagrid/prims.h says so: the triangle's plane, the three box axes and the nine cross axes, float32 without contraction in the
 * expression order of that header (as a truth value: the reference's intersect_prim_cell AND the bounds check).  A box record is 32 bytes, the layout
 * of BBox: float32 min.xyz, int32 first (the pad slot after min; only ids >= first are reported, zero bits = everything), float32 max.xyz, pad 0.
 * With S_i = {j >= first : j meets box i}, m = |S_i| and 1 <= k <= HAGRID_MAX_OVERLAP_IDS:
 *   ids[i*k .. i*k + k-1]  (int32) the min(k, m) smallest ids of S_i, ascending; unused slots -1;
 *   counts[i]              (int32, counts may be NULL) min(m, k + 1): k + 1 says "there are more".
 * So the list for k is a prefix of the list for k + 1, and a caller pages through S_i with first = last id + 1.  The whole of S_i at once, counted and in CSR
 * form, is hagrid_box_refs below (a triangle is referenced by several cells; include/hagrid/overlap.h).  An INACTIVE box -- a NaN bound, or
 * min > max on an axis -- has count 0 and ids -1; a box with min == max is a point.  Before the test every box is CLIPPED to the grid box grown
 * by 2^-16 of its largest |coordinate| (no triangle lies outside the grid box, so nothing is lost; a box inside keeps its bits): infinite and huge bounds
 * are legal and mean "no bound on this side", and a box beyond the grid meets nothing.  flags: 0 or HAGRID_OVERLAP_ANY (k must be 1): the walk stops at the first triangle that meets the box; ids[i] is SOME member of S_i or -1,
 * counts[i] is 0 or 1.  One launch walks the CONSTRUCTION format over the box's voxel range (hagrid_amd/csrc/overlap.hip); the results are those of the
 * brute force over all triangles against the clipped box.  The traversal image, ray binning and the hints kept for the nearest-hit path are neither used nor touched.
 * counters: NULL, or DEVICE int64[4] to which the batch totals are ADDED (boxes, cells visited, triangle / box tests evaluated, sub-blocks pruned):
 * clear it first.  Asynchronous on the context's stream.
 * hagrid_overlap_lattice makes the boxes itself: voxel (x, y, z) of the n[0] x n[1] x n[2] lattice, x fastest, is lo = origin + float(c) * size,
 * hi = origin + float(c + 1) * size per axis (neighbouring voxels share their faces bit for bit), first = 0; origin, size and n are HOST arrays of 3.
 * HAGRID_EINVAL: a null grid or one released by hagrid_grid_release_for_traversal, k out of range, HAGRID_OVERLAP_ANY with k != 1, an unknown flag, null
 * or misaligned buffers (triangles and boxes 16 bytes; ids 16 bytes for k = 4 and k = 8, else 4; counts 4; counters 8), num_boxes < 0, a lattice with n <= 0 on an axis or more than 2^31 - 1
 * voxels, a voxel size that is not positive and finite, an origin that is not finite.  num_boxes = 0 is HAGRID_OK (null buffers are then fine). */
#define HAGRID_MAX_OVERLAP_IDS 8
#define HAGRID_OVERLAP_ANY 1u
int hagrid_overlap_boxes(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* boxes, int num_boxes, int k,
                         void* ids, void* counts, void* counters, uint32_t flags);
int hagrid_overlap_lattice(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const float* origin, const float* size, const int* n, int k,
                           void* ids, void* counts, void* counters, uint32_t flags);

/* Extension (no reference counterpart): CONTACT queries -- for every triangle of a batch, which triangles of the scene it touches (collision between two
 * meshes: Embree's rtcCollide; self-intersection diagnosis).  A query is a 48-byte Tri record A.  Triangles a and b MEET exactly when tri_meets(a, b) of
 * include/hagrid/tri_tri.h says so: no axis of the separating-axis test -- the two stored normals, the nine cross products of an edge of a with an edge of b,
 * the six in-plane edge normals -- strictly separates their projections; float32 without contraction in the expression order of that header.  With
 *   S_i = {j >= first[i] : pair (i, j) is not skipped, triangle j has a surface, triangle j meets box(A_i), tri_meets(A_i, triangle j)},
 * m = |S_i| and 1 <= k <= HAGRID_MAX_OVERLAP_IDS, ids, counts, paging and HAGRID_OVERLAP_ANY are those of hagrid_overlap_boxes.  box(A) is A's bounding box
 * grown by the grid's margin (2^-16 of the largest |coordinate| of the grid box) on every side and clipped as every box is; "meets box" is the test of
 * hagrid_overlap_boxes.  In exact arithmetic the precondition removes nothing (a shared point lies in A's box and in the grid); it makes the walk's answer
 * the brute force's and huge query triangles legal.  first: NULL (0 everywhere) or DEVICE int32[num_queries]; first[i] = i + 1 with the
 * scene's own array as queries reports every pair once.  query_labels: DEVICE int32[3 * num_queries], tri_labels: DEVICE int32[3 per scene triangle], both
 * given or both NULL: pair (i, j) is SKIPPED when a label >= 0 of query i equals a label of triangle j -- with a mesh's index triples as labels a triangle
 * itself and every neighbour that shares a vertex with it, with body ids as labels the contacts inside one body.  A scene triangle whose stored normal is
 * (0, 0, 0) has no surface and takes no part; a query that is not admissible (a float or a derived vertex that is not finite) or whose stored normal is
 * (0, 0, 0) is INACTIVE: count 0, ids -1.  `queries` may be the scene's own array.  counters: as for boxes; the third total counts the pairs offered to
 * tri_meets.  HAGRID_EINVAL: as for hagrid_overlap_boxes (queries 16-byte aligned, first and the labels 4), and one label array without the other.
 * num_queries = 0 is HAGRID_OK. */
int hagrid_overlap_tris(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* queries, int num_queries, const void* first,
                        const void* query_labels, const void* tri_labels, int k, void* ids, void* counts, void* counters, uint32_t flags);

/* Extension (no reference counterpart): ORIENTED-BOX queries -- for every rotated (or sheared) box of a batch, which triangles of the scene meet it (a rigid
 * body's bounding box, a robot link, a plank or a camera-aligned slab against a mesh; "is this rotated region empty?").  A record is 64 bytes, four float4:
 * float32 c.xyz and int32 first (the pad slot, as a box record carries it), then float32 u.xyz, v.xyz, w.xyz, each with pad 0: the box is
 * {c + a u + b v + g w : |a|, |b|, |g| <= 1}.  The axes need be neither normalised nor orthogonal; nothing is divided or normalised.  A triangle MEETS the
 * box exactly when obb_meets of include/hagrid/obb.h says so: no axis of the separating-axis test -- the three face normals of the box, the stored normal
 * of the triangle, the nine cross products of a box axis with a triangle edge -- strictly separates them; float32 without contraction in the expression
 * order of that header, exact on half-integer coordinates up to 16.  With
 *   S_i = {j >= first_i : pair (i, j) is not skipped, triangle j has a surface, triangle j meets aabb(box_i), obb_meets(box_i, triangle j)},
 * m = |S_i| and 1 <= k <= HAGRID_MAX_OVERLAP_IDS, ids, counts, paging and HAGRID_OVERLAP_ANY are those of hagrid_overlap_boxes.  aabb(box) is
 * c -+ (|u| + |v| + |w|) per component, grown by the grid's margin on every side and clipped as every box is; in exact arithmetic it removes nothing.  A
 * record with a component that is not finite is INACTIVE: count 0, ids -1.  A zero axis (a flat box) is legal; the test is then conservative where the pair
 * is coplanar.  query_labels: DEVICE int32[num_obbs], tri_labels: DEVICE int32[3 per scene triangle], both given or both NULL: pair (i, j) is SKIPPED when
 * the label of box i is >= 0 and is one of the three of triangle j -- with body ids as labels a body's box does not see the body's own triangles.  The
 * walk also leaves out every block of the grid that a face normal of the box separates from the box, so a thin diagonal box does not visit its bounding
 * box.  counters: as for boxes; the third total counts the pairs offered to obb_meets.  HAGRID_EINVAL: as for hagrid_overlap_boxes
 * (records 16-byte aligned, labels 4), and one label array without the other.  num_obbs = 0 is HAGRID_OK. */
int hagrid_overlap_obbs(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* obbs, int num_obbs, const void* query_labels,
                        const void* tri_labels, int k, void* ids, void* counts, void* counters, uint32_t flags);

/* Extension (no reference counterpart): OVERLAP LISTS -- EVERY triangle that meets each box, contact query or oriented box, ascending by id, in CSR form,
 * without paging (all contact pairs between two meshes, all self-intersections, everything inside a rigid body's box).  Additive: HAGRID_ABI_VERSION stays 3.
 * For query i the set S_i is EXACTLY the one hagrid_overlap_boxes, hagrid_overlap_tris and hagrid_overlap_obbs define -- `first`, the clip to the grown grid
 * box, the pair tests, labels, inactive queries (the empty list) as there -- and the list is ALL of S_i, ascending: what the pages of the k-list concatenate
 * to.  There is no k and no HAGRID_OVERLAP_ANY: flags must be 0.  The protocol is the ball lists', with one of these three as stage 1:
 *   hagrid_*_refs (count) -> exclusive scan -> hagrid_*_refs (fill) -> hagrid_unique_lists -> exclusive scan -> hagrid_compact_lists;
 * the caller owns every buffer and both scans, and none of the three asks for memory.  A REFERENCE of query i is one member of S_i as the walk meets it: a
 * triangle arrives once per visit of a cell that lists it and only the cell tested last is recognised (include/hagrid/overlap.h, THE DUPLICATE MODEL), so
 * R_i, the number of references, is a property of the grid and the walk; R_i >= m_i = |S_i|; the set of ids among the references is exactly S_i.  Stage 1
 * writes the 8-byte entry {+0.0f, id}: the distance word is a constant, so hagrid_unique_lists sorts by id alone and its contract (equal ids carry equal d2
 * bits) holds trivially; the EMPTY entry stays {+inf, -1}.  Segments, their room and the two modes are hagrid_ball_refs':
 *   count mode  offsets NULL, entries NULL, capacity 0: counts[i] = R_i (counts DEVICE int32[n], 4-byte aligned).
 *   fill mode   offsets given (DEVICE int64[n + 1]): the first min(R_i, room) references in walk order, then the EMPTY entry in every slot of the segment that
 *               is left; nothing outside the segment is written; counts may be NULL.
 *   counters    NULL, or DEVICE int64[6] ADDED to: queries, cells visited, tests evaluated (the meaning of the third total of the k-list query of the same
 *               shape), sub-blocks pruned, references written, queries with R_i > room (count mode adds 0 to the last two).
 * Records, alignment and label rules: hagrid_box_refs takes the boxes of hagrid_overlap_boxes (`first` in the record's pad slot), hagrid_tri_refs the queries,
 * first and labels of hagrid_overlap_tris, hagrid_obb_refs the records (`first` in the pad slot) and labels of hagrid_overlap_obbs.  The lattice form is left
 * out: scene.lattice_boxes gives the same boxes explicitly.  HAGRID_EINVAL: what the k-list query of the same shape refuses of its grid, records and labels,
 * and what hagrid_ball_refs refuses: any flag, a negative capacity, count mode with entries or a capacity, count mode without counts, fill mode with entries
 * NULL and capacity > 0, a misaligned buffer.  n = 0 is HAGRID_OK.  Asynchronous on the context's stream; the CONSTRUCTION format is walked; the traversal
 * image, ray binning and the hints kept for the nearest-hit path are neither used nor touched (hagrid_amd/csrc/overlap_lists.hip). */
int hagrid_box_refs(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* boxes, int num_boxes,
                    const void* offsets, void* counts, void* entries, int64_t capacity, void* counters, uint32_t flags);
int hagrid_tri_refs(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* queries, int num_queries, const void* first,
                    const void* query_labels, const void* tri_labels, const void* offsets, void* counts, void* entries,
                    int64_t capacity, void* counters, uint32_t flags);
int hagrid_obb_refs(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* obbs, int num_obbs,
                    const void* query_labels, const void* tri_labels, const void* offsets, void* counts, void* entries,
                    int64_t capacity, void* counters, uint32_t flags);

/* Extension (no reference counterpart): CROSSING queries -- ALL the surfaces a ray crosses, and from that whether a point lies inside a closed surface
 * (thickness and path length through a solid, signed distance = hagrid_closest_points + inside, solid voxelization = hagrid_overlap_lattice + inside;
 * Embree's rtcIntersect with a collecting filter, Open3D's compute_occupancy).  Ray i CROSSES triangle j exactly when intersect_prim_ray of
 * include/hagrid/prims.h accepts the pair with the ray's OWN [tmin, tmax) -- the intersection set of hagrid_traverse_grid_multi; its value is t, its
 * FACING the sign bit of det = dot(normal, dir): leaving when clear, entering when set (an accepted pair never has det == 0).  With the m crossings of the
 * ray sorted by (t ascending, id ascending) as c_0 .. c_{m-1}, records[i] is 16 bytes in the layout of Hit (so hagrid_shade_hits reads it: GRAY / HEAT = the
 * crossing-count picture, DEPTH = the first surface):
 *   int32 count = m;  float32 t_first = t of c_0 (the bits of tmax when m = 0);
 *   float32 length = the float32 sum, in order, of t_{2p+1} - t_{2p} over the pairs p = 0, 1, .. with 2p + 1 < m, starting from +0 (the length of the ray inside
 *   the solid when it starts outside a closed surface; an unpaired last crossing adds nothing);  int32 winding = #leaving - #entering.
 * A ray that is not admissible or inactive (tmax = -1) takes no cell step: count 0, t = the bits of tmax, length +0, winding 0.  m is NOT bounded:
 * the walk keeps a page of the eight smallest crossings after a cursor, folds it into the record and goes on (include/hagrid/crossings.h); the
 * records are those of the brute force over all triangles, bit for bit.  One launch walks the CONSTRUCTION format in buffer order (hagrid_amd/csrc/crossings.hip);
 * the traversal image, hagrid_set_ray_binning, tile packets, the learned tile order and the hints kept for the nearest-hit path are neither used nor touched.
 * counters: NULL, or DEVICE int64[4] to which the batch totals are ADDED (items, cells visited, triangle tests, pages flushed): clear it first.
 * hagrid_points_inside: points holds 16 bytes per point, float32 x, y, z, reach.  For each of m = num_dirs in {1, 3} directions d (dirs: HOST floats, m * 3;
 * NULL with num_dirs = 0 means the three defaults (3, 1, 2) / sqrt 14, (-2, 4, 3) / sqrt 29, (1, -5, 2) / sqrt 30) the ray is org = p, tmin = 0, dir = d, tmax = reach
 * (+inf is allowed and the normal case).  The vote of d is count & 1, with HAGRID_INSIDE_WINDING it is winding != 0.  inside[i] (int32) is 1 when 2 * votes > m, else
 * 0; -1 for an INACTIVE point (reach < 0, a NaN reach, a NaN or infinite coordinate), which takes no walk.  records: NULL, or DEVICE n * m records (direction
 * fastest) that receive the per-ray records.  The answer means something for CLOSED surfaces only; a point ON the surface gets whatever the formula gives
 * (tmin = 0 accepts t = 0).  hagrid_inside_lattice uses the centre of voxel (x, y, z) of the n[0] x n[1] x n[2] lattice, x fastest, as the point: origin +
 * (float(c) + 0.5f) * size per axis, reach +inf; origin, size and n are HOST arrays of 3.  All three are asynchronous on the context's stream.
 * HAGRID_EINVAL: a null grid or one released by hagrid_grid_release_for_traversal; a context with "traverse.id_is_steps" = 1; null or misaligned buffers
 * (triangles, rays, points and records 16 bytes; inside 4; counters 8); an unknown flag (hagrid_count_crossings has none); a negative count; num_dirs not 1 or 3
 * (0 is allowed with dirs == NULL); a direction that is not finite or has no component to walk along; a lattice with n <= 0 on an axis or more than 2^31 - 1
 * voxels, a voxel size that is not positive and finite, an origin that is not finite.  HAGRID_ERANGE: num_points * m beyond 2^31 - 1.  A count of 0 is HAGRID_OK
 * (null buffers are then fine). */
int hagrid_count_crossings(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* rays, void* records,
                           int num_rays, void* counters, uint32_t flags);
/* hagrid_list_crossings: the crossings THEMSELVES, all of them, sorted (Open3D's list_intersections; the all-hits query of Embree and OptiX users): layered
 * transparency beyond eight layers, per-layer thickness, line integrals with a material per segment, ray stabbing, hole and overlap diagnosis.  The list of ray i
 * is c_0 .. c_{m-1} above.  An ENTRY is 8 bytes: float32 t; int32 key = id * 2 + entering (id = key >> 1, entering = key & 1).  The EMPTY entry is t = the bits
 * of the ray's tmax, key = -1.  `entries` holds `capacity` entries (DEVICE, 8-byte aligned; NULL only with capacity 0).
 *   CSR form: offsets = DEVICE int64[num_rays + 1], 8-byte aligned, stride = 0.  Ray i owns the slots [offsets[i], offsets[i+1]); its ROOM is their number, and 0
 *   if that is negative, if offsets[i] < 0 or if offsets[i+1] > capacity -- such a ray writes nothing, whatever the offsets say.
 *   Stride form: offsets = NULL, stride = S >= 1.  Ray i owns [i * S, (i + 1) * S); num_rays * S <= capacity is checked on the host.  This is multi-hit without
 *   the bound of eight, and what a caller without a scan uses.
 * A ray writes its first min(m, room) entries into the first slots of its range and the empty entry into every slot left over; nothing outside its range is
 * written, and what room r gets is a prefix of what room r + 1 gets.  With offsets = the exclusive sums of the counts hagrid_count_crossings gave for the same
 * rays and grid, every slot is written exactly once and there is no empty entry: count, scan, fill.  A ray that is not admissible or inactive has m = 0: its
 * slots, if any, get empty entries.  records: NULL, or DEVICE num_rays records, 16-byte aligned -- exactly those of hagrid_count_crossings, bit for bit; a list
 * that did not fit shows as record.id > room.  counters: NULL, or DEVICE int64[6], ADDED to: the four above, then entries written (without empty ones) and rays
 * with m > room.  The list does not depend on the page: the brute force of include/hagrid/crossings.h with the same sink defines it.  Asynchronous on the
 * context's stream; the traversal image, ray binning and the hints are neither used nor touched.  HAGRID_EINVAL: as above, and a negative capacity, both or
 * neither of offsets and stride >= 1, misaligned offsets or entries, any flag.  HAGRID_ERANGE: num_rays * stride > capacity.  num_rays = 0 is HAGRID_OK. */
int hagrid_list_crossings(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* rays, int num_rays,
                          const void* offsets, int stride, void* entries, int64_t capacity, void* records, void* counters, uint32_t flags);
#define HAGRID_INSIDE_WINDING 1u
int hagrid_points_inside(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const void* points, int num_points,
                         const float* dirs, int num_dirs, void* inside, void* records, void* counters, uint32_t flags);
int hagrid_inside_lattice(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const float* origin, const float* size, const int* n,
                          const float* dirs, int num_dirs, void* inside, void* records, void* counters, uint32_t flags);
/* hagrid_fill_lattice: the inside of a closed surface on a lattice by SCAN LINES -- one ray per voxel ROW instead of one to three per voxel (solid voxelization,
 * the sign of a distance field on a lattice).  origin, size, n: as for hagrid_inside_lattice, the same checks, the same voxel order (x fastest).  axes: a mask, 1 = x,
 * 2 = y, 4 = z; 0 means 7.  For every requested axis a, every row of the lattice along a gets ONE ray: org = the centre of the row's voxel 0, dir = +e_a, tmin = -inf,
 * tmax = +inf.  Voxel c of the row lies at tc(c) = centre_a(c) - centre_a(0) (float32, one subtraction).  The row's state BEFORE c is taken over the crossings of the
 * row ray with t < tc(c), strictly: their count & 1, with HAGRID_INSIDE_WINDING (#leaving - #entering) != 0; its FINAL state is the same expression over all its
 * crossings.  A row whose final state is 1 ends inside a surface that should be closed (a miscounted crossing, or an open surface): it ABSTAINS.  Otherwise its vote
 * for voxel c is the state before c.  inside[voxel] (int32, 4-byte aligned) is 1 when 2 * votes > valid, else 0, and -1 when valid = 0: valid = the requested axes
 * whose row through the voxel did not abstain, votes = those of them that vote 1.  A row whose ray is not admissible (overflowed centres) has no crossings and votes
 * 0.  The answer means something for CLOSED surfaces only; a centre ON the surface gets what the formula gives.  HAGRID_INSIDE_WINDING is the recommended rule: a row
 * through an edge that two triangles of one face share is accepted by both, which parity counts as no surface at all and the winding number counts right
 * (DESIGN.md 4.11).  workspace: DEVICE, one byte per voxel, required when more than one axis is requested, else it may be NULL; its content afterwards is
 * unspecified.  records: NULL, or DEVICE records of the row rays (16-byte aligned), bit for bit those of hagrid_count_crossings: axis after axis in ascending order,
 * within an axis the lower remaining axis fastest.  counters: NULL, or DEVICE int64[5], ADDED to: rows, cells visited, triangle tests, pages flushed, rows that
 * abstained.  One launch per requested axis, asynchronous on the context's stream; the traversal image, ray binning and the hints are neither used nor touched.
 * HAGRID_EINVAL: as for hagrid_inside_lattice, and an axes bit beyond 7, a missing workspace with more than one axis, a misaligned inside. */
int hagrid_fill_lattice(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const float* origin, const float* size, const int* n,
                        uint32_t axes, void* inside, void* workspace, void* records, void* counters, uint32_t flags);

/* Extension (no reference counterpart): the DISTANCE LATTICE by scatter -- the magnitude of a narrow-band distance field on a lattice, made by the triangles
 * instead of by one walk per voxel (a signed field = this + hagrid_fill_lattice; Open3D's compute_distance on a voxel grid, the narrow band of a level set).
 * origin, size, n: as for hagrid_inside_lattice, the same checks, the same voxel order (x fastest), the same centres.  band: finite, >= 0.  The answer of voxel
 * e is EXACTLY the answer of hagrid_closest_points for the query (centre(e), r = band): among the triangles with a surface and d2 <= band * band the smallest
 * in (d2, id); none: id -1, d2 = band * band, q = the centre.  Every triangle visits the voxels whose centres can lie within the band of its bounding box (the
 * rule and why it is conservative in float32: include/hagrid/distance.h) in tasks of at most 2048 voxels and takes the minimum of the key
 * (bits of d2) << 32 | id into the voxel's slot by a 64-bit atomic; a minimum does not depend on the order of arrival, so the result is deterministic.
 *   grid       supplies the triangle count (the largest id it refers to), the scene box for the margin and the promise that the scene is admissible; its
 *              cells are not walked.  A grid released by hagrid_grid_release_for_traversal is refused.
 *   workspace  DEVICE, 8 bytes per voxel, 8-byte aligned, required.  The call initialises it; its content afterwards is unspecified.
 *   ids, d2    DEVICE int32 / float32 per voxel, 4-byte aligned; either may be NULL.
 *   records    NULL, or DEVICE 32 bytes per voxel, 16-byte aligned: the records of hagrid_closest_points, bit for bit (q, feature and side made again for the
 *              winner by point_tri / tri_side).  At least one of ids, d2 and records must be given.
 *   counters   NULL, or DEVICE int64[4], ADDED to: triangles whose voxel box is not empty, tasks, (triangle, voxel) pairs with d2 <= band * band, voxels
 *              with an answer.  None depends on timing.
 * On the context's stream.  With the traversal image of this grid in the context (hagrid_setup_traversal) there is no host round trip; without it one word (the
 * largest id) is read back first.  One temporary of 4 bytes per triangle comes from the context's pool.
 * HAGRID_EINVAL: the lattice errors of hagrid_inside_lattice; a null, released or incomplete grid; a band that is negative, NaN or infinite; a null or
 * misaligned workspace; ids, d2 and records all NULL; misaligned buffers (triangles and records 16 bytes, ids and d2 4, counters 8); any flag.
 * HAGRID_ENOMEM (the temporary, the status words of the scan over it): ids, d2, records and counters are UNCHANGED -- the kernel that writes them
 * was not launched; the workspace is the call's to scribble on, as always. */
int hagrid_distance_lattice(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const float* origin, const float* size, const int* n,
                            float band, void* workspace, void* ids, void* d2, void* records, void* counters, uint32_t flags);

/* Extension (no reference counterpart): spatial binning of the ray batch before traversal.  mode 0 (default): rays
 * are traversed in buffer order, as the reference does.  mode 1: each hagrid_traverse_grid call first bins the rays by
 * the position where they enter the grid (512 Morton-ordered bins, counting sort on the device) and traverses them in
 * bin order; hits are written to the rays' original slots, results are identical.  Pays for batches without spatial
 * order (random origins / directions: ~2.3x); costs a few percent on batches that are already coherent.  mode 2: automatic --
 * the binning passes run, but image-ordered batches (see "traverse.image_width") skip them, and a batch whose neighbouring
 * rays mostly share a bin (bounce rays in image order, ...) is traversed in buffer order; the decision is taken on the device,
 * the call stays asynchronous. */
int hagrid_set_ray_binning(hagrid_ctx* ctx, int mode);

/* Options: behaviour a caller may want to change; the defaults are the reference's behaviour at the tuned speed.  Keys:
 * "traverse.image": what hagrid_setup_traversal builds -- 2 (default) and 1 = the traversal image, 0 = nothing (traversal walks the construction format);
 * "traverse.image_max_mb": size limit of the image in MB (0, default = max(1 GB, 8x the arrays it replaces)); an image beyond it is not built;
 * "traverse.image_width": tile packets -- a batch in image order (ray y * w + x, as gen_rays of main.cpp:55-66 writes it) is traversed with
 *   one 8 x 8 pixel tile per wavefront instead of a 64 x 1 strip; 0 (default) = the row length w is looked for on the device (constant
 *   (origin, direction) step along a row; for batches of 4M rays or more also from the origins alone -- bounce rays in the image order of
 *   their primary hits), > 0 = w given by the caller, -1 = off.  It only steers the lane <-> ray assignment: hits never depend on it;
 * "traverse.tile_order": -1 (default) / 1 = launches over a ray buffer the context has traversed before dispatch their 8 x 8 tiles longest
 *   first, by the costs the previous launches left (the order is dropped on the device when the buffer holds other rays than the ones it was
 *   learned on; with -1 it is also held against the default order by measurement -- event pairs around launches, polled, nobody waits -- and not
 *   followed where it loses); 0 = every launch in the default order -- like the row length it only steers which wavefront takes which rays,
 *   hits never depend on it.  In either order the context MEASURES, over the first dozen launches of a launch shape and again every 1024
 *   launches, which share of the tiles starts with four lanes per ray (a scheduling choice: same hits); what it finds belongs to the scene and
 *   the shape of the launch, not to the rays, so a camera that moves keeps it;
 * "traverse.id_is_steps": 1 = hagrid_traverse_grid stores the traversal step count in Hit.id, exactly what the reference's kernel leaves
 *   there (traverse.cu:80,93) for its viewer's heat-map display (main.cpp:100-107); 0 (default) = the primitive id or -1 that ray.h:22
 *   documents; t is the same either way;
 * "expand.subset_only": 1 (default) = the reference's compiled setting; 0 = the precise expansion of expand.cu:39-57,96-127 -- this one
 *   changes the grid, not the hits.
 * Returns HAGRID_EINVAL for an unknown key or a value out of range.  (Which of several equivalent kernels / record forms / dispatch
 * geometries runs is not an option of the product: the parity tests force each of them through the test library, csrc/kat/hagrid_amd_kat.h.
 * ABI version 3: the keys "traverse.variant|narrow|image_uniform|image_slim|tail|quad_tail|tail_dual|tile_order_rounds|super_tile|
 * xcd_chunk|row_cache|lds_pad" and "merge.narrow_cells" of version 2 moved there; version 2 had moved the known-answer test hooks out of this library.) */
int hagrid_set_option(hagrid_ctx* ctx, const char* key, int value);

/* The traversal image this context holds for `grid`: format4 = { flat (1: a record per voxel; 2: the general layout, a slim record per voxel-map entry), bit 0: uniform (table-free) | bit 1: the compact table layout is held next to a much bigger uniform one (binned batches gather from it), bits per packed
 * reference id of slim 16-byte records (0: 32-byte records), bytes per record }, *image_bytes = its size (table + blocks, both layouts); either
 * pointer may be NULL.  HAGRID_EINVAL when the context holds no image of this grid. */
int hagrid_traversal_image_info(hagrid_ctx* ctx, const hagrid_grid* grid, int32_t* format4, int64_t* image_bytes);

/* ---- frames on the device (the per-frame work of the reference's front-end, main.cpp:591-621: gen_rays, traverse_grid, update_surface) ---- */
/* Camera in, pixels out, nothing crossing the bus.  Every pointer below except `cam`, `bbox_min`, `bbox_max` is a DEVICE pointer (16-byte
 * aligned where it holds rays or hits, 4-byte aligned for pixels and counts); all work is enqueued on the context's stream; nothing here
 * synchronises with the host or copies to it.  The arithmetic is float32 without contraction, operation for operation that of
 * hagrid_amd/scene.py (make_rays_primary, make_rays_bounce, make_rays_incoherent, shade_hits, shade_occlusion): the same bits.  The per-ray
 * functions are include/hagrid/frame.h, callable from host code too. */
typedef struct hagrid_camera { float eye[3], dir[3], right[3], up[3]; } hagrid_camera;      /* main.cpp:19-24; gen_camera of main.cpp:42-50 fills it */

/* gen_rays (main.cpp:52-66) for the pixels first .. first+count-1 of a width x height image (pixel = y * width + x), ray i = pixel first+i:
 * kx = 2*x/float(w) - 1, ky = 1 - 2*y/float(h), dir = cam.dir + cam.right*kx + cam.up*ky, org = eye, tmin = 0, tmax = clip. */
int hagrid_gen_primary_rays(hagrid_ctx* ctx, const hagrid_camera* cam, float clip, int width, int height,
                            int64_t first, int count, void* rays);

/* The diffuse-bounce rule of BASELINE configuration 5 (scene.make_rays_bounce); ray i draws its random numbers by its global index first+i.
 * Rays with a hit (hits[i].id >= 0, a PRIMITIVE id -- not a step count of "traverse.id_is_steps"): org = p + 1e-4*n, a cosine-weighted
 * direction about the normal that faces the ray, tmin = 0, tmax = `tmax`.  Rays without: with HAGRID_BOUNCE_REDRAW_MISSES an incoherent ray
 * as scene.make_rays_incoherent draws it (origin uniform in the box, tmin = 0, tmax = FLT_MAX: configuration 5); else an INACTIVE ray:
 * org = 0, dir = (0,0,1), tmin = 0, tmax = -1, for which traversal answers id -1, t -1.  out_rays must not be `rays`. */
#define HAGRID_BOUNCE_REDRAW_MISSES 1u
int hagrid_gen_bounce_rays(hagrid_ctx* ctx, const void* tris, const void* rays, const void* hits, int num_rays,
                           uint64_t seed, uint64_t first, const float bbox_min[3], const float bbox_max[3],
                           float tmax, uint32_t flags, void* out_rays);

/* update_surface (main.cpp:68-111): 4 bytes per pixel, B G R A, A = 255.  mode:
 *   HAGRID_SHADE_DEPTH  B=G=R = uint8(min(255.0f * t / clip, 255.0f))  (negative values give 0; clip <= 0 is HAGRID_EINVAL)
 *   HAGRID_SHADE_GRAY   B=G=R = uint8(min(255, id))
 *   HAGRID_SHADE_HEAT   the reference's five-colour gradient of min(100, max(id, 0)) / 100.0f
 * GRAY and HEAT read Hit.id as it is; with "traverse.id_is_steps" = 1 they are the reference viewer's pictures. */
enum { HAGRID_SHADE_DEPTH = 0, HAGRID_SHADE_GRAY = 1, HAGRID_SHADE_HEAT = 2 };
int hagrid_shade_hits(hagrid_ctx* ctx, const void* hits, int num_hits, int mode, float clip, void* bgra);

/* The picture of the hit lists of hagrid_traverse_grid_multi (k records per pixel): every surface a layer of the given opacity in its
 * depth colour, composited front to back over white, in float32, operation for operation (scene.shade_layers):
 *   acc = 0, T = 1; for each slot j < k with id >= 0: c = min(max(255.0f * t_j / clip, 0.0f), 255.0f), acc = acc + (T * opacity) * c,
 *   T = T * (1.0f - opacity); then acc = acc + T * 255.0f; B = G = R = uint8(min(acc, 255.0f)), A = 255.
 * With opacity = 1 a pixel that hit is the HAGRID_SHADE_DEPTH pixel of its first slot.  HAGRID_EINVAL: clip <= 0, opacity outside (0, 1],
 * k outside 1 .. HAGRID_MAX_HITS. */
int hagrid_shade_layers(hagrid_ctx* ctx, const void* hits, int num_rays, int k, float clip, float opacity, void* bgra);

/* Ambient occlusion: counts[i] += occlusion_hits[i].id >= 0 (int32 per ray), and the picture B=G=R = hits[i].id >= 0 ?
 * 255 * (samples - counts[i]) / samples : 0 in integer arithmetic (counts clamped to 0 .. samples), A = 255; `hits` are the PRIMARY hits there. */
int hagrid_accumulate_occlusion(hagrid_ctx* ctx, const void* occlusion_hits, int num_rays, void* counts);
int hagrid_shade_occlusion(hagrid_ctx* ctx, const void* hits, const void* counts, int num_rays, int samples, void* bgra);

/* One frame, all on the stream: primary rays -> hagrid_traverse_grid_ex -> pixels.  ao_samples = 0: hagrid_shade_hits(mode).
 * ao_samples = S > 0: counts = 0; for s in 0 .. S-1: bounce rays (seed + s, first 0, tmax = ao_radius, misses inactive) -> traversal with
 * HAGRID_TRAVERSE_ANY_HIT -> accumulate; then hagrid_shade_occlusion (mode is ignored; refused while "traverse.id_is_steps" = 1, the bounce
 * rays need primitive ids).  The caller owns the workspace (hagrid_frame_workspace_bytes, 16-byte aligned); its sections, each at the next
 * multiple of 256 bytes: rays (32 B per pixel) at offset 0, the primary hits (16 B) behind them, and with ao_samples > 0 the bounce rays
 * (32 B), the occlusion hits (16 B) and the counts (4 B) -- so a caller can read the hits of the frame it just rendered. */
size_t hagrid_frame_workspace_bytes(int width, int height, int ao_samples);
int hagrid_render_frame(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const hagrid_camera* cam, float clip,
                        int width, int height, int mode, int ao_samples, float ao_radius, uint64_t seed,
                        void* workspace, void* bgra);

/* ---- scenes on the device: indexed meshes and instance transforms -> the Tri array (the reference packs it on the host, main.cpp:246-275) ---- */
/* Extension: what comes BEFORE hagrid_build_grid in a frame loop.  A scene is a list of triangle meshes (vertex buffer + index triples, both
 * already on the device -- e.g. torch tensors a simulation or a skinning step rewrites every frame) and a list of instances, each placing one
 * mesh by a 3 x 4 matrix.  hagrid_scene_assemble turns it into the 48-byte Tri records hagrid_build_grid takes, in ONE launch on the
 * context's stream, without a host round trip: 12 bytes per index triple in, 48 bytes per triangle out, nothing crossing the bus.  The
 * arithmetic is float32 without contraction, operation for operation (include/hagrid/assemble.h, callable from host code too;
 * hagrid_amd/scene.py: assemble_tris states it in numpy -- the same bits):
 *   - with a transform M (12 floats, row-major, last column = translation): x' = ((M[0]*x + M[1]*y) + M[2]*z) + M[3], rows 1 and 2
 *     likewise with M[4..7], M[8..11]; with transforms == NULL the vertices are used as they are (not multiplied by an identity: -0 stays -0);
 *   - then main.cpp:259-267 on the three (transformed) vertices: e1 = v0 - v1, e2 = v2 - v0, n = cross(e1, e2), record = v0, n.x, e1, n.y, e2, n.z.
 * A triangle that names a vertex outside 0 .. num_vertices-1 is NEVER read out of bounds: it becomes the degenerate triangle on its mesh's
 * vertex 0 (transformed; e1 = e2 = n = 0: no ray hits it and it stays inside the scene's box) and is counted for hagrid_scene_bad_indices. */
typedef struct hagrid_mesh {        /* one triangle mesh; the two pointers are DEVICE pointers */
    const void* vertices;           /* float32 x, y, z per vertex, vertex_stride bytes apart; 4-byte aligned */
    const void* indices;            /* int32 triples (4-byte aligned), or NULL: triangle p uses vertices 3p, 3p+1, 3p+2 */
    int32_t num_vertices, num_tris;
    int32_t vertex_stride;          /* >= 12, a multiple of 4 (12: a [V,3] tensor, 16: [V,4]) */
    int32_t reserved;               /* 0 */
} hagrid_mesh;                      /* 32 bytes */
typedef struct hagrid_scene hagrid_scene;

/* meshes, instance_mesh: HOST arrays, read during the call.  instance_mesh[i] = the mesh instance i places; NULL = one instance per mesh,
 * in order (num_instances must then be num_meshes).  The scene keeps ADDRESSES, not copies: what the vertex and index buffers hold is read at
 * every hagrid_scene_assemble, so a caller may rewrite vertices between frames (and must keep the buffers alive).  Its small tables (mesh
 * records, instance -> mesh, first triangle of every instance) live in a pool buffer of ctx; hagrid_scene_destroy returns it.  A scene is used
 * with the context it was created in: hagrid_scene_assemble / _bad_indices with another context are HAGRID_EINVAL, _destroy with another one
 * (or after that context was destroyed) releases the handle only.
 * HAGRID_EINVAL (and *out = NULL): a null `out`, null `meshes` with num_meshes > 0, negative counts, a mesh with a stride below 12 or not a
 * multiple of 4, a non-zero `reserved`, num_vertices == 0 with num_tris > 0, a null or misaligned vertex buffer of a mesh that has triangles, a
 * misaligned index buffer, indices == NULL with 3 * num_tris beyond 2^31 - 1, instance_mesh[i] outside 0 .. num_meshes-1, instance_mesh ==
 * NULL with num_instances != num_meshes.  HAGRID_ERANGE: more than 2^31 - 1 output triangles.  A scene without triangles is HAGRID_OK.
 * HAGRID_ENOMEM (the pool buffer of the tables): *out = NULL, nothing is kept.  hagrid_scene_assemble itself allocates nothing. */
int hagrid_scene_create(hagrid_ctx* ctx, const hagrid_mesh* meshes, int num_meshes,
                        const int32_t* instance_mesh, int num_instances, hagrid_scene** out);
void hagrid_scene_destroy(hagrid_ctx* ctx, hagrid_scene* scene);
/* First output triangle of instance i; i = num_instances gives the total.  Instances are laid out in order, each with its mesh's triangles
 * in mesh order.  HAGRID_EINVAL for a null scene or an instance outside 0 .. num_instances. */
int hagrid_scene_first_tri(const hagrid_scene* scene, int instance);
/* transforms: DEVICE, 12 float32 per instance (4-byte aligned), or NULL.  tris: DEVICE, 48 bytes per output triangle, 16-byte aligned.
 * origins: DEVICE int32 pairs (instance, triangle within its mesh) per output triangle (4-byte aligned), or NULL.  Asynchronous on the
 * context's stream.  A scene without triangles launches nothing and accepts tris == NULL. */
int hagrid_scene_assemble(hagrid_ctx* ctx, hagrid_scene* scene, const void* transforms, void* tris, void* origins);
/* Synchronous: how many output triangles of the hagrid_scene_assemble calls since the last query named a vertex outside
 * 0 .. num_vertices-1; resets the count. */
int hagrid_scene_bad_indices(hagrid_ctx* ctx, hagrid_scene* scene, int64_t* count);


#ifdef __cplusplus
}
#endif
#endif /* HAGRID_AMD_H */
