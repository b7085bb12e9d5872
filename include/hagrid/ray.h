// hagrid/ray.h -- Ray (32 B) and Hit (16 B) records (API mirror of the reference's src/ray.h:9-33).
//
// Deliberate difference from the reference binary: traverse_grid leaves the PRIMITIVE id in Hit::id
// (-1 when nothing was hit), which is what this struct documents and what intersect_prim_ray stores;
// the reference kernel overwrites it with its step counter (traverse.cu:93).  The step counter is
// available through hagrid_traverse_grid_stats (include/hagrid_amd.h).
#ifndef HAGRID_RAY_H
#define HAGRID_RAY_H

#include "vec.h"

namespace hagrid {

/// org + t * dir, t in [tmin, tmax]
struct Ray {
    vec3 org; float tmin;
    vec3 dir; float tmax;
    HOST DEVICE Ray() {}
    HOST DEVICE Ray(const vec3& o, float t0, const vec3& d, float t1) : org(o), tmin(t0), dir(d), tmax(t1) {}
};

/// id is -1 if there is no hit
struct Hit {
    int id; float t, u, v;
    HOST DEVICE Hit() {}
    HOST DEVICE Hit(int id_, float t_, float u_, float v_) : id(id_), t(t_), u(u_), v(v_) {}
};

static_assert(sizeof(Ray) == 32 && sizeof(Hit) == 16, "Ray/Hit layout");

/// The ray classification every traversal prologue starts with ("admissible rays").
/// Gives every zero of dir the sign +, so that the exit planes of the walk (dir >= 0) and the infinities of
/// safe_rcp (the sign bit) agree whatever sign the caller's zero had, and returns whether the ray may enter the
/// cell walk: org and dir finite, a component of dir whose reciprocal is finite (so not the zero direction, nor one whose components are
/// all below about 2^-128 = 2.94e-39: no cell has an exit parameter along it), tmin and tmax not NaN.  A ray that may not is a miss.
/// Tests on the bits, which no floating-point option of a compiler can fold away.
HOST DEVICE inline bool admit_ray(const vec3& org, vec3& dir, float tmin, float tmax) {
    dir.x = dir.x == 0.0f ? 0.0f : dir.x;
    dir.y = dir.y == 0.0f ? 0.0f : dir.y;
    dir.z = dir.z == 0.0f ? 0.0f : dir.z;
    const uint32_t e = 0x7f800000u, m = 0x7fffffffu;
    const bool finite = ((as<uint32_t>(org.x) & e) != e) & ((as<uint32_t>(org.y) & e) != e) & ((as<uint32_t>(org.z) & e) != e) &
                        ((as<uint32_t>(dir.x) & e) != e) & ((as<uint32_t>(dir.y) & e) != e) & ((as<uint32_t>(dir.z) & e) != e);
    // a direction to walk along: a component whose reciprocal is finite (|x| from about 2^-128 on; walk_rcp is NaN for +-0 and for what overflows)
    const float rx = walk_rcp(dir.x), ry = walk_rcp(dir.y), rz = walk_rcp(dir.z);
    const bool moves = ((as<uint32_t>(rx) & m) <= e) | ((as<uint32_t>(ry) & m) <= e) | ((as<uint32_t>(rz) & m) <= e);          // not NaN
    const bool window = ((as<uint32_t>(tmin) & m) <= e) & ((as<uint32_t>(tmax) & m) <= e);
    return finite & moves & window;
}

} // namespace hagrid

#endif // HAGRID_RAY_H
