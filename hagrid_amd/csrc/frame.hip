// frame.hip -- a frame on the device: primary rays, bounce rays, shading, ambient occlusion (include/hagrid_amd.h "frames on the device").
//
// ONE streaming kernel with launch-uniform modes (the two ray generators, the picture of hits, the layered picture of multi-hit lists and the two ambient-occlusion steps: the product library's kernel budget), one ray or pixel per lane, 256 lanes per block.  The arithmetic is include/hagrid/frame.h (the same functions a
// host program calls); the kernels only move the records: a Ray is two float4 and a Hit one, loaded and stored as such (16-byte accesses,
// what the traversal kernels read: rays[2 * i], rays[2 * i + 1]), a pixel is one 32-bit word.  Mode, miss rule and flags are kernel
// arguments, not template parameters.  hagrid_render_frame strings them together with hagrid_traverse_grid_ex on the
// context's stream; nothing here waits for the device or copies to the host.
#include "ctx.h"

#include "hagrid/frame.h"

using namespace hagrid_impl;
namespace hf = hagrid::frame;
using hagrid::Hit;
using hagrid::Ray;
using hagrid::vec3;

namespace {

constexpr int kBlock = 256;

__device__ inline void store_ray(float4* __restrict__ rays, int i, const Ray& r) {
    rays[2 * size_t(i)] = make_float4(r.org.x, r.org.y, r.org.z, r.tmin);
    rays[2 * size_t(i) + 1] = make_float4(r.dir.x, r.dir.y, r.dir.z, r.tmax);
}

// Everything this file launches is one kernel (the product library's kernel budget): `shade`, `hits`, `k` and `samples` are
// launch-uniform, every branch on them is taken by whole launches.
// shade == 0, the two ray generators: hits == nullptr: the primary ray of pixel first + i (hagrid_gen_primary_rays; cam, clip, w, h); else the bounce ray
// of hit i (hagrid_gen_bounce_rays; tris: 12 floats per triangle, the normal in words 3, 7, 11 -- the only gather of this file).  The arithmetic is
// hf::primary_ray / hf::bounce_ray either way: the rays are the bits they were.
// shade != 0, the two shading entry points and the two ambient-occlusion steps: k == 0: the pixel of hit i (hagrid_shade_hits); k > 0: the layered picture
// of the k Hit records of pixel i, read where they lie (the list of pixel i starts at hits[i * k]: hagrid_shade_layers; mode is not used).  k < 0: ambient
// occlusion -- samples == 0: counts[i] += hits[i].id >= 0 (`hits` are occlusion hits, bgra is not touched); samples > 0: the pixel of primary hit i and counts[i].
struct FrameArgs {
    hf::Camera cam; float clip; int w, h;                                   // primary (clip: shading as well)
    const float* __restrict__ tris; const float4* __restrict__ rays; const float4* __restrict__ hits;      // bounce (hits: shading as well)
    unsigned long long seed; vec3 lo, hi; float tmax; unsigned flags;
    unsigned long long first; int n;
    float4* __restrict__ out;
    int shade, mode, k, samples; float opacity; int* __restrict__ counts; uint32_t* __restrict__ bgra;      // shading
};

__global__ void __launch_bounds__(kBlock) frame_kernel(const FrameArgs a) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    if (a.shade) {
        if (a.k == 0) {
            const float4 hv = a.hits[i];
            a.bgra[i] = hf::shade_hit(Hit(__float_as_int(hv.x), hv.y, hv.z, hv.w), a.mode, a.clip);
        } else if (a.k > 0) {
            a.bgra[i] = hf::shade_layers(reinterpret_cast<const Hit*>(a.hits) + size_t(i) * size_t(a.k), a.k, a.clip, a.opacity);
        } else {
            const int id = __float_as_int(a.hits[i].x);
            if (a.samples == 0) a.counts[i] += id >= 0 ? 1 : 0;
            else a.bgra[i] = hf::shade_occlusion(id, a.counts[i], a.samples);
        }
        return;
    }
    Ray r;
    if (!a.hits) {
        r = hf::primary_ray(a.cam, a.clip, a.w, a.h, (long long)a.first + i);
    } else {
        const float4 hv = a.hits[i];
        const int id = __float_as_int(hv.x);
        if (id >= 0) {
            const float4 p = a.rays[2 * size_t(i)], q = a.rays[2 * size_t(i) + 1];
            const float* t = a.tris + 12 * size_t(id);
            r = hf::bounce_ray(Ray(vec3(p.x, p.y, p.z), p.w, vec3(q.x, q.y, q.z), q.w), hv.y, vec3(t[3], t[7], t[11]), a.seed, a.first + uint64_t(i), a.tmax);
        } else if (a.flags & HAGRID_BOUNCE_REDRAW_MISSES) {
            r = hf::incoherent_ray(a.lo, a.hi, a.seed ^ 0x6D69737300000000ull, a.first + uint64_t(i), 0.0f, FLT_MAX);
        } else {
            r = hf::inactive_ray();
        }
    }
    store_ray(a.out, i, r);
}

/// a shading launch: the arguments frame_kernel's shade modes read
inline FrameArgs shade_args(const void* hits, int n, int mode, float clip, int k, float opacity, void* counts, int samples, void* bgra) {
    FrameArgs a = {};
    a.shade = 1; a.hits = static_cast<const float4*>(hits); a.n = n; a.mode = mode; a.clip = clip; a.k = k; a.opacity = opacity;
    a.counts = static_cast<int*>(counts); a.samples = samples; a.bgra = static_cast<uint32_t*>(bgra);
    return a;
}

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// the sections of a frame workspace (include/hagrid_amd.h: hagrid_render_frame), offsets in bytes
struct FrameLayout { size_t rays, hits, bounce, occ_hits, counts, total; };
inline FrameLayout frame_layout(size_t n, bool ao) {
    FrameLayout l;
    l.rays = 0;
    l.hits = up256(32 * n);
    l.bounce = l.occ_hits = l.counts = 0;
    l.total = l.hits + up256(16 * n);
    if (ao) {
        l.bounce = l.total;
        l.occ_hits = l.bounce + up256(32 * n);
        l.counts = l.occ_hits + up256(16 * n);
        l.total = l.counts + up256(4 * n);
    }
    return l;
}

} // namespace

extern "C" int hagrid_gen_primary_rays(hagrid_ctx* ctx, const hagrid_camera* cam, float clip, int width, int height, int64_t first, int count, void* rays) {
    if (!ctx) return HAGRID_EINVAL;
    if (!cam || !rays) HG_FAIL(ctx, HAGRID_EINVAL, "gen_primary_rays: null camera or ray buffer");
    if (!aligned(rays, 16)) HG_FAIL(ctx, HAGRID_EINVAL, "gen_primary_rays: the ray buffer is not 16-byte aligned");
    if (width <= 0 || height <= 0 || count <= 0) HG_FAIL(ctx, HAGRID_EINVAL, "gen_primary_rays: width, height and count must be positive");
    if (first < 0 || first + int64_t(count) > int64_t(width) * int64_t(height)) HG_FAIL(ctx, HAGRID_EINVAL, "gen_primary_rays: the pixel range [first, first + count) leaves the image");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    trav_image_source_touched(ctx, rays, size_t(count) * 32);
    FrameArgs a = {};
    memcpy(&a.cam, cam, sizeof(a.cam));
    a.clip = clip; a.w = width; a.h = height; a.first = (unsigned long long)first; a.n = count; a.out = static_cast<float4*>(rays);
    frame_kernel<<<grid_blocks(count, kBlock), kBlock, 0, ctx->stream>>>(a);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

extern "C" int hagrid_gen_bounce_rays(hagrid_ctx* ctx, const void* tris, const void* rays, const void* hits, int num_rays, uint64_t seed, uint64_t first,
                                      const float bbox_min[3], const float bbox_max[3], float tmax, uint32_t flags, void* out_rays) {
    if (!ctx) return HAGRID_EINVAL;
    if (!tris || !rays || !hits || !out_rays) HG_FAIL(ctx, HAGRID_EINVAL, "gen_bounce_rays: null triangle, ray, hit or output buffer");
    if (!bbox_min || !bbox_max) HG_FAIL(ctx, HAGRID_EINVAL, "gen_bounce_rays: null bounding box");
    if (!aligned(tris, 4) || !aligned(rays, 16) || !aligned(hits, 16) || !aligned(out_rays, 16)) HG_FAIL(ctx, HAGRID_EINVAL, "gen_bounce_rays: ray and hit buffers must be 16-byte aligned");
    if (num_rays <= 0) HG_FAIL(ctx, HAGRID_EINVAL, "gen_bounce_rays: num_rays must be positive");
    if (out_rays == rays) HG_FAIL(ctx, HAGRID_EINVAL, "gen_bounce_rays: out_rays must not be the input rays");
    if (flags & ~HAGRID_BOUNCE_REDRAW_MISSES) HG_FAIL(ctx, HAGRID_EINVAL, "gen_bounce_rays: unknown flag");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    trav_image_source_touched(ctx, out_rays, size_t(num_rays) * 32);
    FrameArgs a = {};
    a.tris = static_cast<const float*>(tris); a.rays = static_cast<const float4*>(rays); a.hits = static_cast<const float4*>(hits);
    a.seed = seed; a.lo = vec3(bbox_min[0], bbox_min[1], bbox_min[2]); a.hi = vec3(bbox_max[0], bbox_max[1], bbox_max[2]); a.tmax = tmax; a.flags = flags;
    a.first = first; a.n = num_rays; a.out = static_cast<float4*>(out_rays);
    frame_kernel<<<grid_blocks(num_rays, kBlock), kBlock, 0, ctx->stream>>>(a);
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

extern "C" int hagrid_shade_hits(hagrid_ctx* ctx, const void* hits, int num_hits, int mode, float clip, void* bgra) {
    if (!ctx) return HAGRID_EINVAL;
    if (!hits || !bgra) HG_FAIL(ctx, HAGRID_EINVAL, "shade_hits: null hit or pixel buffer");
    if (!aligned(hits, 16) || !aligned(bgra, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "shade_hits: hits must be 16-byte aligned, pixels 4-byte aligned");
    if (num_hits <= 0) HG_FAIL(ctx, HAGRID_EINVAL, "shade_hits: num_hits must be positive");
    if (mode != HAGRID_SHADE_DEPTH && mode != HAGRID_SHADE_GRAY && mode != HAGRID_SHADE_HEAT) HG_FAIL(ctx, HAGRID_EINVAL, "shade_hits: unknown mode");
    if (mode == HAGRID_SHADE_DEPTH && !(clip > 0.0f)) HG_FAIL(ctx, HAGRID_EINVAL, "shade_hits: the depth picture needs clip > 0");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    trav_image_source_touched(ctx, bgra, size_t(num_hits) * 4);
    frame_kernel<<<grid_blocks(num_hits, kBlock), kBlock, 0, ctx->stream>>>(shade_args(hits, num_hits, mode, clip, 0, 0.0f, nullptr, 0, bgra));
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

extern "C" int hagrid_shade_layers(hagrid_ctx* ctx, const void* hits, int num_rays, int k, float clip, float opacity, void* bgra) {
    if (!ctx) return HAGRID_EINVAL;
    if (!hits || !bgra) HG_FAIL(ctx, HAGRID_EINVAL, "shade_layers: null hit or pixel buffer");
    if (!aligned(hits, 16) || !aligned(bgra, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "shade_layers: hits must be 16-byte aligned, pixels 4-byte aligned");
    if (num_rays <= 0) HG_FAIL(ctx, HAGRID_EINVAL, "shade_layers: num_rays must be positive");
    if (k < 1 || k > HAGRID_MAX_HITS) HG_FAIL(ctx, HAGRID_EINVAL, "shade_layers: k must be 1 .. HAGRID_MAX_HITS");
    if (!(clip > 0.0f)) HG_FAIL(ctx, HAGRID_EINVAL, "shade_layers: the depth colours need clip > 0");
    if (!(opacity > 0.0f && opacity <= 1.0f)) HG_FAIL(ctx, HAGRID_EINVAL, "shade_layers: opacity must be in (0, 1]");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    trav_image_source_touched(ctx, bgra, size_t(num_rays) * 4);
    frame_kernel<<<grid_blocks(num_rays, kBlock), kBlock, 0, ctx->stream>>>(shade_args(hits, num_rays, 0, clip, k, opacity, nullptr, 0, bgra));
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

extern "C" int hagrid_accumulate_occlusion(hagrid_ctx* ctx, const void* occlusion_hits, int num_rays, void* counts) {
    if (!ctx) return HAGRID_EINVAL;
    if (!occlusion_hits || !counts) HG_FAIL(ctx, HAGRID_EINVAL, "accumulate_occlusion: null hit or count buffer");
    if (!aligned(occlusion_hits, 16) || !aligned(counts, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "accumulate_occlusion: hits must be 16-byte aligned, counts 4-byte aligned");
    if (num_rays <= 0) HG_FAIL(ctx, HAGRID_EINVAL, "accumulate_occlusion: num_rays must be positive");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    trav_image_source_touched(ctx, counts, size_t(num_rays) * 4);
    frame_kernel<<<grid_blocks(num_rays, kBlock), kBlock, 0, ctx->stream>>>(shade_args(occlusion_hits, num_rays, 0, 0.0f, -1, 0.0f, counts, 0, nullptr));
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

extern "C" int hagrid_shade_occlusion(hagrid_ctx* ctx, const void* hits, const void* counts, int num_rays, int samples, void* bgra) {
    if (!ctx) return HAGRID_EINVAL;
    if (!hits || !counts || !bgra) HG_FAIL(ctx, HAGRID_EINVAL, "shade_occlusion: null hit, count or pixel buffer");
    if (!aligned(hits, 16) || !aligned(counts, 4) || !aligned(bgra, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "shade_occlusion: hits must be 16-byte aligned, counts and pixels 4-byte aligned");
    if (num_rays <= 0 || samples <= 0) HG_FAIL(ctx, HAGRID_EINVAL, "shade_occlusion: num_rays and samples must be positive");
    HG_HIP(ctx, hipSetDevice(ctx->device));
    trav_image_source_touched(ctx, bgra, size_t(num_rays) * 4);
    frame_kernel<<<grid_blocks(num_rays, kBlock), kBlock, 0, ctx->stream>>>(shade_args(hits, num_rays, 0, 0.0f, -1, 0.0f, const_cast<void*>(counts), samples, bgra));
    HG_DBG(ctx);
    HG_HIP(ctx, hipGetLastError());
    return HAGRID_OK;
}

extern "C" size_t hagrid_frame_workspace_bytes(int width, int height, int ao_samples) {
    if (width <= 0 || height <= 0 || ao_samples < 0 || int64_t(width) * int64_t(height) > int64_t(INT32_MAX)) return 0;
    return frame_layout(size_t(width) * size_t(height), ao_samples > 0).total;
}

extern "C" int hagrid_render_frame(hagrid_ctx* ctx, const hagrid_grid* grid, const void* tris, const hagrid_camera* cam, float clip, int width, int height,
                                   int mode, int ao_samples, float ao_radius, uint64_t seed, void* workspace, void* bgra) {
    if (!ctx) return HAGRID_EINVAL;
    if (!grid || !tris || !cam || !workspace || !bgra) HG_FAIL(ctx, HAGRID_EINVAL, "render_frame: null grid, triangles, camera, workspace or pixel buffer");
    if (width <= 0 || height <= 0 || int64_t(width) * int64_t(height) > int64_t(INT32_MAX)) HG_FAIL(ctx, HAGRID_EINVAL, "render_frame: width and height must be positive and width * height fit 31 bits");
    if (ao_samples < 0) HG_FAIL(ctx, HAGRID_EINVAL, "render_frame: ao_samples must not be negative");
    if (!aligned(workspace, 16) || !aligned(bgra, 4)) HG_FAIL(ctx, HAGRID_EINVAL, "render_frame: the workspace must be 16-byte aligned, the pixels 4-byte aligned");
    if (ao_samples == 0) {
        if (mode != HAGRID_SHADE_DEPTH && mode != HAGRID_SHADE_GRAY && mode != HAGRID_SHADE_HEAT) HG_FAIL(ctx, HAGRID_EINVAL, "render_frame: unknown mode");
        if (mode == HAGRID_SHADE_DEPTH && !(clip > 0.0f)) HG_FAIL(ctx, HAGRID_EINVAL, "render_frame: the depth picture needs clip > 0");
    } else if (ctx->opt_id_is_steps) {
        HG_FAIL(ctx, HAGRID_EINVAL, "render_frame: ambient occlusion needs primitive ids in the hits (\"traverse.id_is_steps\" is 1)");
    }
    const int n = width * height;
    const FrameLayout l = frame_layout(size_t(n), ao_samples > 0);
    char* ws = static_cast<char*>(workspace);
    void* rays = ws + l.rays;
    void* hits = ws + l.hits;
    HG_TRY(hagrid_gen_primary_rays(ctx, cam, clip, width, height, 0, n, rays));
    HG_TRY(hagrid_traverse_grid_ex(ctx, grid, tris, rays, hits, n, 0u));
    if (ao_samples == 0) return hagrid_shade_hits(ctx, hits, n, mode, clip, bgra);
    void* bounce = ws + l.bounce;
    void* occ = ws + l.occ_hits;
    void* counts = ws + l.counts;
    HG_HIP(ctx, hipMemsetAsync(counts, 0, size_t(n) * 4, ctx->stream));
    for (int s = 0; s < ao_samples; s++) {
        HG_TRY(hagrid_gen_bounce_rays(ctx, tris, rays, hits, n, seed + uint64_t(s), 0, grid->bbox_min, grid->bbox_max, ao_radius, 0u, bounce));
        HG_TRY(hagrid_traverse_grid_ex(ctx, grid, tris, bounce, occ, n, HAGRID_TRAVERSE_ANY_HIT));
        HG_TRY(hagrid_accumulate_occlusion(ctx, occ, n, counts));
    }
    return hagrid_shade_occlusion(ctx, hits, counts, n, ao_samples, bgra);
}
