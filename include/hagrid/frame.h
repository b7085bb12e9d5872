// hagrid/frame.h -- the per-frame work around traverse_grid: camera -> primary rays, hits -> bounce rays, hits -> pixels.
//
// The reference does this on the host in its front-end (src/main.cpp:42-111: gen_camera, gen_rays, gradient, update_surface);
// here the same formulas are HOST DEVICE inline functions, one ray or pixel each.  The gfx950 kernels of
// hagrid_amd/csrc/frame.hip call them, and so can a host program: both give the bits of hagrid_amd/scene.py
// (make_rays_primary, make_rays_bounce, make_rays_incoherent, shade_hits, shade_occlusion) -- float32, no contraction
// (-ffp-contract=off), every sum in the order written.  Below them, shims over the C ABI on device pointers.
//
// Everything lives in hagrid::frame, and NO other header of this directory includes this one: a program written against
// the reference declares its own global Camera / gen_camera / gen_rays next to `using namespace hagrid`.
#ifndef HAGRID_FRAME_H
#define HAGRID_FRAME_H

#include <cfloat>

#include "build.h"
#include "grid.h"
#include "mem_manager.h"
#include "prims.h"
#include "ray.h"
#include "vec.h"

namespace hagrid {
namespace frame {

/// main.cpp:19-24, in the member order of hagrid_camera (include/hagrid_amd.h)
struct Camera {
    vec3 eye, dir, right, up;
};
static_assert(sizeof(Camera) == sizeof(hagrid_camera), "Camera / hagrid_camera layout");

/// gen_camera (main.cpp:42-50); host only (tanf)
inline Camera gen_camera(const vec3& eye, const vec3& center, const vec3& up, float fov, float ratio) {
    Camera cam;
    const float f = tanf(float(M_PI * fov / 360));
    cam.dir = normalize(center - eye);
    cam.right = normalize(cross(cam.dir, up)) * (f * ratio);
    cam.up = normalize(cross(cam.right, cam.dir)) * f;
    cam.eye = eye;
    return cam;
}

enum ShadeMode { SHADE_DEPTH = HAGRID_SHADE_DEPTH, SHADE_GRAY = HAGRID_SHADE_GRAY, SHADE_HEAT = HAGRID_SHADE_HEAT };

// ---- one ray / one pixel ---------------------------------------------------------------------------------------------------

/// float32 in [0,1): (splitmix64(seed + (index + 1) * golden) >> 40) * 2^-24 (scene.uniform01)
HOST DEVICE inline float uniform01(uint64_t seed, uint64_t index) {
    uint64_t z = seed + (index + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return float(uint32_t(z >> 40)) * (1.0f / 16777216.0f);
}

/// gen_rays (main.cpp:52-66) for one pixel of a w x h image, pixel = y * w + x
HOST DEVICE inline Ray primary_ray(const Camera& cam, float clip, int w, int h, int64_t pixel) {
    const int x = int(pixel % w), y = int(pixel / w);
    const float kx = float(2 * x) / float(w) - 1.0f;
    const float ky = 1.0f - float(2 * y) / float(h);
    return Ray(cam.eye, 0.0f, cam.dir + cam.right * kx + cam.up * ky, clip);
}

/// scene.make_rays_incoherent for the ray of global index `index`: origin uniform in the box, direction drawn from the cube
/// [-1,1]^3 until 0.01 < |d|^2 <= 1 (64 attempts, then (0,0,1)), not normalised
HOST DEVICE inline Ray incoherent_ray(const vec3& lo, const vec3& hi, uint64_t seed, uint64_t index, float tmin, float tmax) {
    const vec3 uo(uniform01(seed, index * 3), uniform01(seed, index * 3 + 1), uniform01(seed, index * 3 + 2));
    Ray r(lo + uo * (hi - lo), tmin, vec3(0.0f, 0.0f, 1.0f), tmax);
    const uint64_t dseed = seed ^ 0x6469720000000000ull;
    for (int attempt = 0; attempt < 64; attempt++) {
        const uint64_t base = (index * 64 + uint64_t(attempt)) * 3;
        const vec3 d(2.0f * uniform01(dseed, base) - 1.0f, 2.0f * uniform01(dseed, base + 1) - 1.0f, 2.0f * uniform01(dseed, base + 2) - 1.0f);
        const float l2 = d.x * d.x + d.y * d.y + d.z * d.z;
        if (l2 > 0.01f && l2 <= 1.0f) { r.dir = d; break; }
    }
    return r;
}

/// the ray traversal answers with id -1, t -1: an empty interval
HOST DEVICE inline Ray inactive_ray() { return Ray(vec3(0.0f, 0.0f, 0.0f), 0.0f, vec3(0.0f, 0.0f, 1.0f), -1.0f); }

/// the (unnormalised) normal a Tri carries in its fourth words (prims.h:13-25)
HOST DEVICE inline vec3 tri_normal(const Tri& t) { return vec3(t.nx, t.ny, t.nz); }

/// scene.make_rays_bounce for a ray that hit at distance t the triangle with normal n_raw: origin lifted 1e-4 normals off the surface,
/// direction cosine-weighted about the normal that faces the ray, from the two random numbers of the global ray index
HOST DEVICE inline Ray bounce_ray(const Ray& r, float t, const vec3& n_raw, uint64_t seed, uint64_t index, float tmax) {
    const vec3 p = r.org + r.dir * t;
    const float nn = n_raw.x * n_raw.x + n_raw.y * n_raw.y + n_raw.z * n_raw.z;
    const float ln = std::sqrt(nn < 1e-30f ? 1e-30f : nn);
    vec3 n = n_raw / ln;
    if (n.x * r.dir.x + n.y * r.dir.y + n.z * r.dir.z > 0.0f) n = vec3(-n.x, -n.y, -n.z);
    const float u0 = uniform01(seed, index * 2), u1 = uniform01(seed, index * 2 + 1);
    // a point of the unit disk without trigonometry: radius sqrt(u0), the angle through the rational parametrisation of the
    // half circle by s in [-1,1), mirrored by the lowest bit of the index
    const float s = 2.0f * u1 - 1.0f;
    const float half = float(uint32_t(index & 1)) * 2.0f - 1.0f;
    const float cx = (1.0f - s * s) / (1.0f + s * s) * half;
    const float cy = 2.0f * s / (1.0f + s * s);
    const float rad = std::sqrt(u0);
    const float dx = rad * cx, dy = rad * cy;
    const float one_minus = 1.0f - u0;
    const float dz = std::sqrt(one_minus < 0.0f ? 0.0f : one_minus);
    const vec3 a = std::fabs(n.x) > 0.5f ? vec3(0.0f, 1.0f, 0.0f) : vec3(1.0f, 0.0f, 0.0f);
    vec3 tx = cross(a, n);
    tx = tx / std::sqrt(tx.x * tx.x + tx.y * tx.y + tx.z * tx.z);
    const vec3 ty = cross(n, tx);
    return Ray(p + 1e-4f * n, 0.0f, tx * dx + ty * dy + n * dz, tmax);
}

/// B | G << 8 | R << 16 | A << 24: the four bytes of a pixel as one little-endian word
HOST DEVICE inline uint32_t pack_bgra(uint32_t b, uint32_t g, uint32_t r) { return (b & 255u) | (g & 255u) << 8 | (r & 255u) << 16 | 255u << 24; }

/// gradient (main.cpp:68-88): blue, cyan, dark green, yellow, red over k in [0,1]
HOST DEVICE inline uint32_t gradient(float k) {
    const float g[5][3] = {{0.0f, 0.0f, 255.0f}, {0.0f, 255.0f, 255.0f}, {0.0f, 128.0f, 0.0f}, {255.0f, 255.0f, 0.0f}, {255.0f, 0.0f, 0.0f}};
    const int n = 5;
    const float s = 1.0f / n;
    const int i = min(n - 1, int(k * n));
    const int j = min(n - 1, i + 1);
    const float t = (k - i * s) / s;
    const float cr = (1.0f - t) * g[i][0] + t * g[j][0], cg = (1.0f - t) * g[i][1] + t * g[j][1], cb = (1.0f - t) * g[i][2] + t * g[j][2];
    return pack_bgra(uint32_t(cb), uint32_t(cg), uint32_t(cr));
}

/// update_surface (main.cpp:90-111) for one hit
HOST DEVICE inline uint32_t shade_hit(const Hit& hit, int mode, float clip) {
    if (mode == SHADE_DEPTH) {
        const float v = min(max(255.0f * hit.t / clip, 0.0f), 255.0f);
        const uint32_t c = uint32_t(v);
        return pack_bgra(c, c, c);
    }
    if (mode == SHADE_GRAY) {
        const uint32_t c = uint32_t(min(255, hit.id));             // -1 wraps to 255, as the reference's uint8_t does
        return pack_bgra(c, c, c);
    }
    return gradient(float(min(100, max(hit.id, 0))) / 100.0f);
}

/// the pixel of a ray's sorted hit list (k records, hagrid_traverse_grid_multi): every surface a layer of the given opacity in its
/// depth colour (shade_hit's depth mode), composited front to back over white; every sum in the order written (scene.shade_layers)
HOST DEVICE inline uint32_t shade_layers(const Hit* hits, int k, float clip, float opacity) {
    float acc = 0.0f, T = 1.0f;
    for (int j = 0; j < k; j++) {
        if (hits[j].id < 0) continue;
        const float c = min(max(255.0f * hits[j].t / clip, 0.0f), 255.0f);
        acc = acc + (T * opacity) * c;
        T = T * (1.0f - opacity);
    }
    acc = acc + T * 255.0f;
    const uint32_t g = uint32_t(min(acc, 255.0f));
    return pack_bgra(g, g, g);
}

/// the ambient-occlusion pixel of a primary hit whose `samples` occlusion rays were blocked `count` times
HOST DEVICE inline uint32_t shade_occlusion(int primary_id, int count, int samples) {
    const int c = primary_id >= 0 ? 255 * (samples - min(max(count, 0), samples)) / samples : 0;
    return pack_bgra(uint32_t(c), uint32_t(c), uint32_t(c));
}

// ---- shims over the C ABI: device pointers, the current MemManager's context and stream, asynchronous ----------------------

namespace detail {
inline hagrid_camera to_pod(const Camera& c) {
    hagrid_camera p;
    std::memcpy(&p, &c, sizeof(p));
    return p;
}
} // namespace detail

/// gen_rays (main.cpp:52-66) into device memory: the rays of the pixels first .. first + count - 1
inline void gen_rays(const Camera& cam, Ray* rays, float clip, int w, int h, int64_t first, int count) {
    const hagrid_camera p = detail::to_pod(cam);
    hagrid::detail::check(hagrid::detail::current_ctx(), hagrid_gen_primary_rays(hagrid::detail::current_ctx(), &p, clip, w, h, first, count, rays));
}
inline void gen_rays(const Camera& cam, Ray* rays, float clip, int w, int h) { gen_rays(cam, rays, clip, w, h, 0, w * h); }

/// bounce rays of `rays` / `hits` into out_rays; redraw_misses: rays without a hit become incoherent rays, else inactive ones
inline void gen_bounce_rays(const Tri* tris, const Ray* rays, const Hit* hits, int num_rays, uint64_t seed, uint64_t first,
                            const BBox& bbox, float tmax, bool redraw_misses, Ray* out_rays) {
    const float lo[3] = {bbox.min.x, bbox.min.y, bbox.min.z}, hi[3] = {bbox.max.x, bbox.max.y, bbox.max.z};
    hagrid::detail::check(hagrid::detail::current_ctx(), hagrid_gen_bounce_rays(hagrid::detail::current_ctx(), tris, rays, hits, num_rays, seed, first, lo, hi, tmax,
                                                                                  redraw_misses ? HAGRID_BOUNCE_REDRAW_MISSES : 0u, out_rays));
}

/// update_surface (main.cpp:90-111) into a device buffer of 4 bytes per pixel (B G R A)
inline void shade_hits(const Hit* hits, int num_hits, ShadeMode mode, float clip, void* bgra) {
    hagrid::detail::check(hagrid::detail::current_ctx(), hagrid_shade_hits(hagrid::detail::current_ctx(), hits, num_hits, int(mode), clip, bgra));
}

/// the layered picture of num_rays hit lists of k records each (traverse_grid_multi) into a device buffer of 4 bytes per pixel
inline void shade_layers(const Hit* hits, int num_rays, int k, float clip, float opacity, void* bgra) {
    hagrid::detail::check(hagrid::detail::current_ctx(), hagrid_shade_layers(hagrid::detail::current_ctx(), hits, num_rays, k, clip, opacity, bgra));
}

inline size_t frame_workspace_bytes(int w, int h, int ao_samples) { return hagrid_frame_workspace_bytes(w, h, ao_samples); }

/// one frame: camera in, pixels out (hagrid_render_frame).  The rays of the frame are at workspace_rays(), its hits at workspace_hits().
inline void render_frame(const Grid& grid, const Tri* tris, const Camera& cam, float clip, int w, int h, ShadeMode mode,
                         int ao_samples, float ao_radius, uint64_t seed, void* workspace, void* bgra) {
    const hagrid_grid g = hagrid::detail::to_pod(grid);
    const hagrid_camera p = detail::to_pod(cam);
    hagrid::detail::check(hagrid::detail::current_ctx(), hagrid_render_frame(hagrid::detail::current_ctx(), &g, tris, &p, clip, w, h, int(mode), ao_samples, ao_radius, seed, workspace, bgra));
}
inline Ray* workspace_rays(void* workspace) { return static_cast<Ray*>(workspace); }
inline Hit* workspace_hits(void* workspace, int w, int h) {
    const size_t ray_bytes = (size_t(w) * size_t(h) * sizeof(Ray) + 255) / 256 * 256;
    return reinterpret_cast<Hit*>(static_cast<char*>(workspace) + ray_bytes);
}

} // namespace frame
} // namespace hagrid

#endif // HAGRID_FRAME_H
