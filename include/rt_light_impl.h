/*
 * rt_light_impl.h -- the per-pixel arithmetic of rt_hit_surfaces* and
 * rt_light_hits* (DESIGN.md §3.1a), of the shadow term, rt_shadow_hits*
 * and rt_light_hits_shadowed* (§3.1b), of the mirror bounce,
 * rt_reflect_hits* and rt_light_hits_reflected* (§3.1c), and of the two
 * together, rt_shadow_hits_reflected* and rt_light_hits_shadowed_reflected*
 * (§3.1d), and of the mirror chain, rt_bounce_hits* and rt_light_hits_mirrored*
 * (§3.1e): one text for the host functions (csrc/rt_light.cpp) and the kernels
 * (csrc/rt_light.hip, csrc/rt_shadow.hip, csrc/rt_reflect.hip,
 * csrc/rt_shadow_reflect.hip, csrc/rt_mirror.hip; how a wave walks through it is
 * csrc/rt_light_device.inc), and their shared argument check.
 * Internal: not installed, not part of the ABI.
 *
 * Every fp32 operation is written on its own and rounds once; both builds
 * use -ffp-contract=off, the device's '/' and sqrtf are IEEE
 * (-fhip-fp32-correctly-rounded-divide-sqrt).  Sums are parenthesised in the
 * order DESIGN.md states.  NaN compares false everywhere.
 */
#ifndef RT_LIGHT_IMPL_H
#define RT_LIGHT_IMPL_H

#include <math.h>
#include <stdint.h>

#include "rt_hip.h"

/* rt_light_device.inc defines this as `__host__ __device__ inline` before including */
#ifndef RT_LIGHT_FN
#define RT_LIGHT_FN inline
#endif

namespace rt_light {

/* The common checks of the entry points (0 or RT_ERR_INVALID_ARG):
 * NULL pointers, width / rows (the pixel-coordinate limits of
 * rt_args::check_args), counts, and arrays missing for a non-zero count,
 * lights included.  csrc/rt_light.cpp. */
int check(const rt_hit* hits, const rt_scene* scene, const float* ray_dir, int32_t width,
          int32_t row_begin, int32_t row_end, const void* out);
/* The settings of the lit chain entry points, host and device: the format,
 * max_bounces, shadows, and a NULL reflectivity where a chain could read it.
 * `scene` may be NULL (refused by the checks behind). */
int check_chain_settings(const rt_scene* scene, const float* reflectivity, int32_t max_bounces,
                         int32_t shadows, int32_t out_format);
/* The host's scan of a reflectivity array (NULL: none): every value in [0, 1]
 * (NaN is refused too); `mirrors`: one of them is not 0. */
int check_reflectivity(const rt_scene& scene, const float* reflectivity, bool& mirrors);

constexpr double kEpsilon = 0.000001;  // MainState.cpp:15
constexpr float kFar = 300000.0f;      // MainState.cpp:345

// (int)f as x86-64 cvttss2si: truncation, NaN / out of range -> INT32_MIN.
RT_LIGHT_FN int32_t cvt_i32(float f) {
    return (f >= -2147483648.0f && f < 2147483648.0f) ? static_cast<int32_t>(f) : INT32_MIN;
}

// The Texture packing (MainState.cpp:1026-1036).
RT_LIGHT_FN uint32_t pack_rgba8(const int32_t p[4]) {
    return static_cast<uint32_t>(static_cast<uint8_t>(p[0])) |
           (static_cast<uint32_t>(static_cast<uint8_t>(p[1])) << 8) |
           (static_cast<uint32_t>(static_cast<uint8_t>(p[2])) << 16) | 0xFF000000u;
}

// The reference's fp64 Moeller-Trumbore test (MainState.cpp:257-298), the
// text of intersect_tri in the generic kernel (rt_trace.inc).
RT_LIGHT_FN int intersect_tri(const double* orig, const double* dir, const double* v0,
                              const double* v1, const double* v2, double* t) {
    double e1[3], e2[3], tv[3], pv[3], qv[3];
    e1[0] = v1[0] - v0[0]; e1[1] = v1[1] - v0[1]; e1[2] = v1[2] - v0[2];
    e2[0] = v2[0] - v0[0]; e2[1] = v2[1] - v0[1]; e2[2] = v2[2] - v0[2];
    pv[0] = dir[1] * e2[2] - dir[2] * e2[1];
    pv[1] = dir[2] * e2[0] - dir[0] * e2[2];
    pv[2] = dir[0] * e2[1] - dir[1] * e2[0];
    const double det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
    if (det > -kEpsilon && det < kEpsilon) return 0;
    const double inv_det = 1.0 / det;
    tv[0] = orig[0] - v0[0]; tv[1] = orig[1] - v0[1]; tv[2] = orig[2] - v0[2];
    const double u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv_det;
    if (u < 0.0 || u > 1.0) return 0;
    qv[0] = tv[1] * e1[2] - tv[2] * e1[1];
    qv[1] = tv[2] * e1[0] - tv[0] * e1[2];
    qv[2] = tv[0] * e1[1] - tv[1] * e1[0];
    const double v = (dir[0] * qv[0] + dir[1] * qv[1] + dir[2] * qv[2]) * inv_det;
    if (v < 0.0 || u + v > 1.0) return 0;
    *t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv_det;
    return 1;
}

struct Vec3 {
    float x, y, z;
};

// m / |m|, |m| = sqrtf((x*x + y*y) + z*z), three divisions
RT_LIGHT_FN Vec3 normalise(Vec3 m) {
    const float len = sqrtf((m.x * m.x + m.y * m.y) + m.z * m.z);
    return Vec3{m.x / len, m.y / len, m.z / len};
}

// n turned against the ray: negated where (n . d) > 0
RT_LIGHT_FN Vec3 face(Vec3 n, Vec3 d) {
    const float s = (n.x * d.x + n.y * d.y) + n.z * d.z;
    if (s > 0.0f) return Vec3{-n.x, -n.y, -n.z};
    return n;
}

// The hit point of pixel (ox, oy): o + t * d with o.z = 0.
RT_LIGHT_FN Vec3 hit_point(float ox, float oy, Vec3 d, float t) {
    return Vec3{ox + t * d.x, oy + t * d.y, 0.0f + t * d.z};
}

// Cube pixels: the first of the cube's twelve triangles (float4[36] at
// `verts`) whose fp64 test hits with (float)t == the frame's t, and its
// unit normal (unfaced).  No match: triangle -1, normal 0.
RT_LIGHT_FN rt_surface cube_surface(const float* verts, float ox, float oy, Vec3 d, float t) {
    const double o[3] = {ox, oy, 0.0};
    const double dir[3] = {d.x, d.y, d.z};
    int tri = -1;
    for (int k = 0; k < 12; ++k) {
        const float* a = verts + 12 * k;
        const float* b = a + 4;
        const float* c = a + 8;
        const double v0[3] = {a[0], a[1], a[2]}, v1[3] = {b[0], b[1], b[2]},
                     v2[3] = {c[0], c[1], c[2]};
        double td;
        if (intersect_tri(o, dir, v0, v1, v2, &td) == 1 && static_cast<float>(td) == t) {
            tri = k;
            break;
        }
    }
    if (tri < 0) return rt_surface{0.0f, 0.0f, 0.0f, -1};
    // (after the loop: on the device the lanes of a wave leave it at different
    // k, and the normal is then computed once, not once per distinct k)
    const float* a = verts + 12 * tri;
    const float* b = a + 4;
    const float* c = a + 8;
    const Vec3 e1{b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const Vec3 e2{c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const Vec3 n = normalise(Vec3{e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z,
                                  e1.x * e2.y - e1.y * e2.x});
    return rt_surface{n.x, n.y, n.z, tri};
}

// The float4[36] of cube `obj` (NULL when `obj` is no cube).
RT_LIGHT_FN const float* cube_verts(const rt_scene& s, int32_t obj) {
    return obj >= 0 && obj < s.num_cubes ? s.cube_vertices + 144 * static_cast<int64_t>(obj)
                                         : nullptr;
}

// The surface of one pixel.  `obj` is already range-checked: -1 (nothing
// hit) or a colour slot of `s`; `verts` = cube_verts(s, obj).  `p` is the
// pixel's hit point.
RT_LIGHT_FN rt_surface surface(const rt_scene& s, int32_t obj, const float* verts, float ox,
                               float oy, Vec3 d, float t, Vec3 p) {
    if (obj < 0) return rt_surface{0.0f, 0.0f, 0.0f, -1};
    rt_surface r;
    if (obj < s.num_cubes) {
        r = cube_surface(verts, ox, oy, d, t);
    } else {
        const float* c = s.sphere_origins + 4 * static_cast<int64_t>(obj - s.num_cubes);
        const Vec3 n = normalise(Vec3{p.x - c[0], p.y - c[1], p.z - c[2]});
        r = rt_surface{n.x, n.y, n.z, -1};
    }
    const Vec3 n = face(Vec3{r.nx, r.ny, r.nz}, d);
    return rt_surface{n.x, n.y, n.z, r.triangle};
}

// The lighting factor of a hit pixel with at least one light: the clamped
// sum of the positive cosines between n and the directions to the lights
// (float4 each, w ignored).
RT_LIGHT_FN float light_factor(Vec3 n, Vec3 p, const float* lights, int32_t num_lights) {
    float k = 0.0f;
    for (int32_t i = 0; i < num_lights; ++i) {
        const float* l = lights + 4 * static_cast<int64_t>(i);
        const Vec3 L{l[0] - p.x, l[1] - p.y, l[2] - p.z};
        const float ll = sqrtf((L.x * L.x + L.y * L.y) + L.z * L.z);
        const float c = ((n.x * L.x + n.y * L.y) + n.z * L.z) / ll;
        if (c > 0.0f) k = k + c;
    }
    if (k > 1.0f) k = 1.0f;
    return k;
}

// rt_shade_hits' pixel (MainState.cpp:396-407) with the ramp scaled by k.
RT_LIGHT_FN void shade_lit(float t, float k, Vec3 colour, int32_t out[4]) {
    out[0] = out[1] = out[2] = 0;
    out[3] = 255;
    if (t == kFar) return;
    const float normalised = (t - 0.0f) / (180.0f - 0.0f);
    const float scalar = 255.0f - (normalised * 255.0f);
    const float lit = scalar * k;
    out[0] = cvt_i32(lit * colour.x);
    out[1] = cvt_i32(lit * colour.y);
    out[2] = cvt_i32(lit * colour.z);
}

// One lit pixel (int32x4).  `obj` and `verts` as for surface().
RT_LIGHT_FN void lit_pixel(const rt_scene& s, int32_t obj, const float* verts, float ox, float oy,
                           Vec3 d, float t, int32_t out[4]) {
    // closestColour starts as (0, 0, 0, 255) (MainState.cpp:344)
    Vec3 colour{0.0f, 0.0f, 0.0f};
    if (obj >= 0) {
        const float* c = obj < s.num_cubes
                             ? s.cube_colours + 4 * static_cast<int64_t>(obj)
                             : s.sphere_colours + 4 * static_cast<int64_t>(obj - s.num_cubes);
        colour = Vec3{c[0], c[1], c[2]};
    }
    float k = 1.0f;
    if (s.num_lights > 0 && obj >= 0) {
        const Vec3 p = hit_point(ox, oy, d, t);
        const rt_surface n = surface(s, obj, verts, ox, oy, d, t, p);
        k = light_factor(Vec3{n.nx, n.ny, n.nz}, p, s.lights, s.num_lights);
    }
    shade_lit(t, k, colour, out);
}

/* ---- the shadow term ------------------------------------
 * For a hit pixel and a light that faces it (c > 0): is the segment from the
 * hit point p to the light, p + s * L with s in (0, 1), cut by any object
 * other than the pixel's own?
 *
 * The pixel's own object is never an occluder, and that is exact, not a
 * bias: cubes and spheres are convex, and a point of a convex surface that
 * faces the light sees it without entering its own object again.  A scene
 * with a non-convex primitive would need its own object tested too.
 *
 * "Any" does not depend on the order of the tests, so the callers may test
 * in any order and stop at the first occluder. */

// One triangle (three float4 at `tri`): the fp64 test on p and the
// un-normalised L as doubles, strictly between the hit point and the light
// (the light sits at parameter 1).
RT_LIGHT_FN bool occluded_by_tri(const double* p, const double* L, const float* tri) {
    const double v0[3] = {tri[0], tri[1], tri[2]}, v1[3] = {tri[4], tri[5], tri[6]},
                 v2[3] = {tri[8], tri[9], tri[10]};
    double td;
    return intersect_tri(p, L, v0, v1, v2, &td) == 1 && td > 0.0 && td < 1.0;
}

// One sphere (float4 centre, radius r), all fp32: the roots of
// a*s*s - 2*b*s + q = 0.  Non-finite values compare false: not occluded.
RT_LIGHT_FN bool occluded_by_sphere(Vec3 p, Vec3 L, const float* centre, float r) {
    const Vec3 m{centre[0] - p.x, centre[1] - p.y, centre[2] - p.z};
    const float a = (L.x * L.x + L.y * L.y) + L.z * L.z;
    const float b = (m.x * L.x + m.y * L.y) + m.z * L.z;
    const float q = ((m.x * m.x + m.y * m.y) + m.z * m.z) - r * r;
    const float disc = b * b - a * q;
    if (!(disc >= 0.0f)) return false;
    const float sq = sqrtf(disc);
    const float s0 = (b - sq) / a;
    const float s1 = (b + sq) / a;
    return (s0 > 0.0f && s0 < 1.0f) || (s1 > 0.0f && s1 < 1.0f);
}

// The cull policy of a walk: cube(o, d, j, segment) says whether the ray
// (o, d: the doubles of its floats; segment: the shadow walk's (0, 1), else the
// bounce's (0, inf)) has to test cube j.  A policy with kGroups also walks the
// spheres itself (rt_sphere_groups_impl.h); the others leave them to the walk's
// own loop.  This one keeps every cube: the unculled walks.  The wave's walks of
// csrc/rt_light_device.inc take the same policies.
struct KeepAll {
    static constexpr bool kGroups = false;
    RT_LIGHT_FN bool cube(const double*, const double*, int32_t, bool) const { return true; }
};
// The policy of a ray-query kernel's cull arguments (csrc/rt_rays_device.inc): none.
RT_LIGHT_FN KeepAll cull_of() { return KeepAll{}; }
// What a launch checks of its policy's arguments (the host, after the unculled checks).
inline int check_cull(const rt_scene*, KeepAll) { return RT_OK; }

// Does any object but `obj` (range-checked: a colour slot of `s`) occlude
// the light at p + L?  The loops index 0 .. count-1 only; `obj` is compared.
template <typename Cull = KeepAll>
RT_LIGHT_FN bool light_occluded(const rt_scene& s, int32_t obj, Vec3 p, Vec3 L,
                                const Cull& cull = Cull()) {
    const double pd[3] = {p.x, p.y, p.z};
    const double Ld[3] = {L.x, L.y, L.z};
    for (int32_t j = 0; j < s.num_cubes; ++j) {
        if (j == obj || !cull.cube(pd, Ld, j, true)) continue;
        const float* v = s.cube_vertices + 144 * static_cast<int64_t>(j);
        for (int k = 0; k < 12; ++k)
            if (occluded_by_tri(pd, Ld, v + 12 * k)) return true;
    }
    if constexpr (Cull::kGroups) {
        return cull.occluded_by_spheres(s, pd, Ld, obj, p, L);
    } else {
        for (int32_t i = 0; i < s.num_spheres; ++i) {
            if (static_cast<int64_t>(s.num_cubes) + i == obj) continue;
            if (occluded_by_sphere(p, L, s.sphere_origins + 4 * static_cast<int64_t>(i),
                                   s.sphere_radius[i]))
                return true;
        }
        return false;
    }
}

// The two walks of a pixel function, as one value: light_occluded and
// bounce_walk (defined behind bounce_walk below).  The pixel functions that walk
// are templates over it with this pair as the default; the *_accel calls pass
// rt_accel_impl.h's culled pair, so each level loop has one text.
struct Walks;

// Bit i: light i faces the pixel (c > 0) and is occluded.  At most 32 lights
// (the callers refuse more); n is the faced normal of a hit pixel.
template <typename W = Walks>
RT_LIGHT_FN uint32_t shadow_mask(const rt_scene& s, int32_t obj, Vec3 n, Vec3 p,
                                 const W& w = W()) {
    uint32_t mask = 0;
    for (int32_t i = 0; i < s.num_lights && i < 32; ++i) {
        const float* l = s.lights + 4 * static_cast<int64_t>(i);
        const Vec3 L{l[0] - p.x, l[1] - p.y, l[2] - p.z};
        const float ll = sqrtf((L.x * L.x + L.y * L.y) + L.z * L.z);
        const float c = ((n.x * L.x + n.y * L.y) + n.z * L.z) / ll;
        if (c > 0.0f && w.occluded(s, obj, p, L)) mask |= 1u << i;
    }
    return mask;
}

// light_factor with the occluded lights left out of the sum.
template <typename W = Walks>
RT_LIGHT_FN float shadowed_factor(const rt_scene& s, int32_t obj, Vec3 n, Vec3 p,
                                  const W& w = W()) {
    float k = 0.0f;
    for (int32_t i = 0; i < s.num_lights; ++i) {
        const float* l = s.lights + 4 * static_cast<int64_t>(i);
        const Vec3 L{l[0] - p.x, l[1] - p.y, l[2] - p.z};
        const float ll = sqrtf((L.x * L.x + L.y * L.y) + L.z * L.z);
        const float c = ((n.x * L.x + n.y * L.y) + n.z * L.z) / ll;
        if (c > 0.0f && !w.occluded(s, obj, p, L)) k = k + c;
    }
    if (k > 1.0f) k = 1.0f;
    return k;
}

// The colour of slot `obj` ((0, 0, 0) for -1), as lit_pixel reads it.
RT_LIGHT_FN Vec3 slot_colour(const rt_scene& s, int32_t obj) {
    if (obj < 0) return Vec3{0.0f, 0.0f, 0.0f};
    const float* c = obj < s.num_cubes
                         ? s.cube_colours + 4 * static_cast<int64_t>(obj)
                         : s.sphere_colours + 4 * static_cast<int64_t>(obj - s.num_cubes);
    return Vec3{c[0], c[1], c[2]};
}

// lit_pixel with shadowed_factor in place of light_factor.
template <typename W = Walks>
RT_LIGHT_FN void lit_pixel_shadowed(const rt_scene& s, int32_t obj, const float* verts, float ox,
                                    float oy, Vec3 d, float t, int32_t out[4], const W& w = W()) {
    float k = 1.0f;
    if (s.num_lights > 0 && obj >= 0) {
        const Vec3 p = hit_point(ox, oy, d, t);
        const rt_surface n = surface(s, obj, verts, ox, oy, d, t, p);
        k = shadowed_factor(s, obj, Vec3{n.nx, n.ny, n.nz}, p, w);
    }
    shade_lit(t, k, slot_colour(s, obj), out);
}

// The mask of one pixel (0 for a miss or without lights).
template <typename W = Walks>
RT_LIGHT_FN uint32_t shadow_pixel(const rt_scene& s, int32_t obj, const float* verts, float ox,
                                  float oy, Vec3 d, float t, const W& w = W()) {
    if (s.num_lights <= 0 || obj < 0) return 0;
    const Vec3 p = hit_point(ox, oy, d, t);
    const rt_surface n = surface(s, obj, verts, ox, oy, d, t, p);
    return shadow_mask(s, obj, Vec3{n.nx, n.ny, n.nz}, p, w);
}

/* ---- the mirror bounce -----------------------------------
 * For a hit pixel: the closest hit of the ray that leaves the hit point p
 * along the mirrored direction R, over every object but the pixel's own.
 *
 * Leaving the own object out is exact for the reason given above for the
 * shadow term: cubes and spheres are convex and n . R = -(n . d) >= 0 for the
 * faced normal, so the mirrored ray leaves its own surface and cannot enter
 * its own object again.  A non-convex primitive would need its own object
 * tested too. */

// d mirrored at the faced unit normal n; not normalised.  n = 0 gives d.
RT_LIGHT_FN Vec3 mirror_dir(Vec3 n, Vec3 d) {
    const float s = (n.x * d.x + n.y * d.y) + n.z * d.z;
    const float f = s + s;
    return Vec3{d.x - f * n.x, d.y - f * n.y, d.z - f * n.z};
}

// One triangle (three float4 at `tri`): the fp64 test on p and R as doubles.
// A candidate iff it returns 1 with td > 0; its parameter is (float)td.
RT_LIGHT_FN bool bounce_tri(const double* p, const double* R, const float* tri, float* sf) {
    const double v0[3] = {tri[0], tri[1], tri[2]}, v1[3] = {tri[4], tri[5], tri[6]},
                 v2[3] = {tri[8], tri[9], tri[10]};
    double td;
    if (intersect_tri(p, R, v0, v1, v2, &td) != 1 || !(td > 0.0)) return false;
    *sf = static_cast<float>(td);
    return true;
}

// One sphere: the quadratic of occluded_by_sphere with R in place of L.  The
// near root where it is ahead of p, else the far one (p inside the sphere).
RT_LIGHT_FN bool bounce_sphere(Vec3 p, Vec3 R, const float* centre, float r, float* sf) {
    const Vec3 m{centre[0] - p.x, centre[1] - p.y, centre[2] - p.z};
    const float a = (R.x * R.x + R.y * R.y) + R.z * R.z;
    const float b = (m.x * R.x + m.y * R.y) + m.z * R.z;
    const float q = ((m.x * m.x + m.y * m.y) + m.z * m.z) - r * r;
    const float disc = b * b - a * q;
    if (!(disc >= 0.0f)) return false;
    const float sq = sqrtf(disc);
    const float s0 = (b - sq) / a;
    const float s1 = (b + sq) / a;
    if (s0 > 0.0f) {
        *sf = s0;
        return true;
    }
    if (s1 > 0.0f) {
        *sf = s1;
        return true;
    }
    return false;
}

// The closest hit of a bounce: its parameter along R (kFar: nothing), the
// colour slot and, for a cube, the triangle.
struct Bounce {
    float best;
    int32_t obj2, tri2;
};

// The walk from p along R over every object but `obj` (range-checked: a
// colour slot of `s`; compared, never an index): cubes 0 .. nc-1 with
// triangles 0 .. 11, then spheres 0 .. ns-1.  A candidate is taken iff
// sf < best, so ties go to the first in that order (the reference's rule).
// A cull policy leaves out cubes (and groups of spheres) it proves missed.
template <typename Cull = KeepAll>
RT_LIGHT_FN Bounce bounce_walk(const rt_scene& s, int32_t obj, Vec3 p, Vec3 R,
                               const Cull& cull = Cull()) {
    Bounce b{kFar, -1, -1};
    const double pd[3] = {p.x, p.y, p.z};
    const double Rd[3] = {R.x, R.y, R.z};
    float sf;
    for (int32_t j = 0; j < s.num_cubes; ++j) {
        if (j == obj || !cull.cube(pd, Rd, j, false)) continue;
        const float* v = s.cube_vertices + 144 * static_cast<int64_t>(j);
        for (int k = 0; k < 12; ++k)
            if (bounce_tri(pd, Rd, v + 12 * k, &sf) && sf < b.best) b = Bounce{sf, j, k};
    }
    if constexpr (Cull::kGroups) {
        return cull.bounce_spheres(s, pd, Rd, obj, p, R, b);
    } else {
        for (int32_t i = 0; i < s.num_spheres; ++i) {
            if (static_cast<int64_t>(s.num_cubes) + i == obj) continue;
            if (bounce_sphere(p, R, s.sphere_origins + 4 * static_cast<int64_t>(i),
                              s.sphere_radius[i], &sf) &&
                sf < b.best)
                b = Bounce{sf, s.num_cubes + i, -1};
        }
        return b;
    }
}

// A pair of walks over one cull policy.
template <typename Cull>
struct WalksOver {
    Cull cull;
    RT_LIGHT_FN bool occluded(const rt_scene& s, int32_t obj, Vec3 p, Vec3 L) const {
        return light_occluded(s, obj, p, L, cull);
    }
    RT_LIGHT_FN Bounce bounce(const rt_scene& s, int32_t obj, Vec3 p, Vec3 R) const {
        return bounce_walk(s, obj, p, R, cull);
    }
};
// The unculled pair (declared in front of shadow_mask above).
struct Walks : WalksOver<KeepAll> {};

// The unit normal at the bounce's hit point p2, turned against R.  `obj2` is
// a colour slot of `s` and `tri2` a triangle of that cube (bounce_walk's).
RT_LIGHT_FN Vec3 bounce_normal(const rt_scene& s, int32_t obj2, int32_t tri2, Vec3 p2, Vec3 R) {
    Vec3 n;
    if (obj2 < s.num_cubes) {
        const float* a = s.cube_vertices + 144 * static_cast<int64_t>(obj2) + 12 * tri2;
        const float* b = a + 4;
        const float* c = a + 8;
        const Vec3 e1{b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        const Vec3 e2{c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        n = normalise(Vec3{e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z,
                           e1.x * e2.y - e1.y * e2.x});
    } else {
        const float* c = s.sphere_origins + 4 * static_cast<int64_t>(obj2 - s.num_cubes);
        n = normalise(Vec3{p2.x - c[0], p2.y - c[1], p2.z - c[2]});
    }
    return face(n, R);
}

// The mirrored pixel after the walk: the unshadowed lit pixel (ramp of t
// scaled by k, as shade_lit) blended by r with what the bounce `b` met.  For
// a hit pixel with t != kFar.
RT_LIGHT_FN void shade_mirrored(const rt_scene& s, int32_t obj, float t, float k, Vec3 p, Vec3 R,
                                Bounce b, float r, int32_t out[4]) {
    const float normalised = (t - 0.0f) / (180.0f - 0.0f);
    const float scalar = 255.0f - (normalised * 255.0f);
    const float lit = scalar * k;
    const Vec3 colour = slot_colour(s, obj);
    float lit2 = 0.0f;
    Vec3 colour2{0.0f, 0.0f, 0.0f};
    if (b.obj2 >= 0) {
        const Vec3 p2{p.x + b.best * R.x, p.y + b.best * R.y, p.z + b.best * R.z};
        float k2 = 1.0f;
        if (s.num_lights > 0)
            k2 = light_factor(bounce_normal(s, b.obj2, b.tri2, p2, R), p2, s.lights, s.num_lights);
        const float t2 = t + b.best;
        const float normalised2 = (t2 - 0.0f) / (180.0f - 0.0f);
        float scalar2 = 255.0f - (normalised2 * 255.0f);
        // beyond the ramp's end a mirrored object adds nothing, not negative light
        if (!(scalar2 > 0.0f)) scalar2 = 0.0f;
        lit2 = scalar2 * k2;
        colour2 = slot_colour(s, b.obj2);
    }
    const float a[3] = {lit * colour.x, lit * colour.y, lit * colour.z};
    const float m[3] = {lit2 * colour2.x, lit2 * colour2.y, lit2 * colour2.z};
    for (int c = 0; c < 3; ++c) out[c] = cvt_i32(a[c] + r * (m[c] - a[c]));
    out[3] = 255;
}

// The bounce of one pixel ((kFar, -1) for a miss).  `obj`, `verts` as for surface().
RT_LIGHT_FN Bounce bounce_pixel(const rt_scene& s, int32_t obj, const float* verts, float ox,
                                float oy, Vec3 d, float t) {
    if (obj < 0) return Bounce{kFar, -1, -1};
    const Vec3 p = hit_point(ox, oy, d, t);
    const rt_surface n = surface(s, obj, verts, ox, oy, d, t, p);
    return bounce_walk(s, obj, p, mirror_dir(Vec3{n.nx, n.ny, n.nz}, d));
}

// One mirrored lit pixel (int32x4), r != 0.  A miss, and t == kFar, are lit_pixel's.
RT_LIGHT_FN void lit_pixel_reflected(const rt_scene& s, int32_t obj, const float* verts, float ox,
                                     float oy, Vec3 d, float t, float r, int32_t out[4]) {
    if (obj < 0 || t == kFar) {
        lit_pixel(s, obj, verts, ox, oy, d, t, out);
        return;
    }
    const Vec3 p = hit_point(ox, oy, d, t);
    const rt_surface sf = surface(s, obj, verts, ox, oy, d, t, p);
    const Vec3 n{sf.nx, sf.ny, sf.nz};
    float k = 1.0f;
    if (s.num_lights > 0) k = light_factor(n, p, s.lights, s.num_lights);
    const Vec3 R = mirror_dir(n, d);
    shade_mirrored(s, obj, t, k, p, R, bounce_walk(s, obj, p, R), r, out);
}

/* ---- shadows and the mirror bounce together --------------
 * The mirrored pixel with the shadow term in both places: the shadowed factor
 * at the hit point p and the shadowed factor at the point p2 the bounce meets.
 *
 * Who is left out at p2: the bounce's object obj2, always, and nothing else;
 * the primary pixel's own object is an occluder at p2 like any other.  That is
 * exact where the bounce arrives from outside obj2 (the argument of the shadow
 * term above).  It is not exact where it arrives from inside obj2 (the far
 * root of a sphere p lies in, a triangle of an intersecting cube met from
 * within): there n2 is turned inward and obj2's far side could hide a facing
 * light.  The rule is "leave obj2 out" all the same. */

// The point the bounce meets, as shade_mirrored computes it.
RT_LIGHT_FN Vec3 bounce_point(Vec3 p, Vec3 R, float best) {
    return Vec3{p.x + best * R.x, p.y + best * R.y, p.z + best * R.z};
}

// shade_mirrored with both factors given: k at the hit point, k2 at the point
// the bounce `b` met (read only where it met something).  For a hit pixel
// with t != kFar.
RT_LIGHT_FN void shade_mirrored_factors(const rt_scene& s, int32_t obj, float t, float k, Bounce b,
                                        float k2, float r, int32_t out[4]) {
    const float normalised = (t - 0.0f) / (180.0f - 0.0f);
    const float scalar = 255.0f - (normalised * 255.0f);
    const float lit = scalar * k;
    const Vec3 colour = slot_colour(s, obj);
    float lit2 = 0.0f;
    Vec3 colour2{0.0f, 0.0f, 0.0f};
    if (b.obj2 >= 0) {
        const float t2 = t + b.best;
        const float normalised2 = (t2 - 0.0f) / (180.0f - 0.0f);
        float scalar2 = 255.0f - (normalised2 * 255.0f);
        // beyond the ramp's end a mirrored object adds nothing, not negative light
        if (!(scalar2 > 0.0f)) scalar2 = 0.0f;
        lit2 = scalar2 * k2;
        colour2 = slot_colour(s, b.obj2);
    }
    const float a[3] = {lit * colour.x, lit * colour.y, lit * colour.z};
    const float m[3] = {lit2 * colour2.x, lit2 * colour2.y, lit2 * colour2.z};
    for (int c = 0; c < 3; ++c) out[c] = cvt_i32(a[c] + r * (m[c] - a[c]));
    out[3] = 255;
}

// One mirrored, shadowed lit pixel (int32x4), r != 0.  A miss, and t == kFar,
// are lit_pixel_shadowed's.
RT_LIGHT_FN void lit_pixel_shadowed_reflected(const rt_scene& s, int32_t obj, const float* verts,
                                              float ox, float oy, Vec3 d, float t, float r,
                                              int32_t out[4]) {
    if (obj < 0 || t == kFar) {
        lit_pixel_shadowed(s, obj, verts, ox, oy, d, t, out);
        return;
    }
    const Vec3 p = hit_point(ox, oy, d, t);
    const rt_surface sf = surface(s, obj, verts, ox, oy, d, t, p);
    const Vec3 n{sf.nx, sf.ny, sf.nz};
    float k = 1.0f;
    if (s.num_lights > 0) k = shadowed_factor(s, obj, n, p);
    const Vec3 R = mirror_dir(n, d);
    const Bounce b = bounce_walk(s, obj, p, R);
    float k2 = 1.0f;
    if (b.obj2 >= 0 && s.num_lights > 0) {
        const Vec3 p2 = bounce_point(p, R, b.best);
        k2 = shadowed_factor(s, b.obj2, bounce_normal(s, b.obj2, b.tri2, p2, R), p2);
    }
    shade_mirrored_factors(s, obj, t, k, b, k2, r, out);
}

// The mask at the point the bounce meets (0 for a miss, without lights, and
// where the bounce meets nothing).  t is not looked at, as in bounce_pixel.
RT_LIGHT_FN uint32_t shadow_reflect_pixel(const rt_scene& s, int32_t obj, const float* verts,
                                          float ox, float oy, Vec3 d, float t) {
    if (s.num_lights <= 0 || obj < 0) return 0;
    const Vec3 p = hit_point(ox, oy, d, t);
    const rt_surface n = surface(s, obj, verts, ox, oy, d, t, p);
    const Vec3 R = mirror_dir(Vec3{n.nx, n.ny, n.nz}, d);
    const Bounce b = bounce_walk(s, obj, p, R);
    if (b.obj2 < 0) return 0;
    const Vec3 p2 = bounce_point(p, R, b.best);
    return shadow_mask(s, b.obj2, bounce_normal(s, b.obj2, b.tri2, p2, R), p2);
}

/* ---- mirror chains, reflectivity per object --------------
 * The bounce taken again from the point it meets, level by level.  Level 0 is
 * the pixel; from level j the chain goes on iff j < max_bounces and
 * reflectivity[obj_j] != 0, along R_j = mirror_dir(n_j, D_j), by bounce_walk
 * with obj_j alone left out: the primary object and every earlier one are
 * candidates again.  What it meets is level j + 1: obj2, bounce_point,
 * bounce_normal, D = R_j, T = T_j + best.
 *
 * Leaving only the current object out is exact where the bounce arrived from
 * outside it, and has §3.1d's inexactness where it arrived from inside (the
 * far root of a sphere, a triangle of an intersecting cube met from within):
 * the next bounce and the shadow walk there leave that object out all the
 * same. */

// reflectivity[obj] as the chain reads it: a value not in [0, 1], NaN
// included, is 0 (the host functions refuse such an array; a kernel cannot).
// -0 stays -0 and ends the chain like 0.
RT_LIGHT_FN float slot_reflectivity(const float* reflectivity, int32_t obj) {
    const float r = reflectivity[obj];
    return (r >= 0.0f && r <= 1.0f) ? r : 0.0f;
}

// The ramp of a level at depth T, as shade_mirrored_factors writes it; from
// level 1 on clamped at 0 from below (NaN: 0).
RT_LIGHT_FN float chain_scalar(float T, bool clamped) {
    const float normalised = (T - 0.0f) / (180.0f - 0.0f);
    float scalar = 255.0f - (normalised * 255.0f);
    if (clamped && !(scalar > 0.0f)) scalar = 0.0f;
    return scalar;
}

// The own colour of a level: (scalar * k) * colour.
RT_LIGHT_FN Vec3 chain_colour(float scalar, float k, Vec3 colour) {
    const float lit = scalar * k;
    return Vec3{lit * colour.x, lit * colour.y, lit * colour.z};
}

// One step of the backward blend: a + r * (C - a) per channel.
RT_LIGHT_FN Vec3 chain_blend(Vec3 a, float r, Vec3 C) {
    return Vec3{a.x + r * (C.x - a.x), a.y + r * (C.y - a.y), a.z + r * (C.z - a.z)};
}

// The level the bounce `b` from p along R met, in place: its point, faced
// normal and object.  R is the direction the level was reached along, which
// the next bounce mirrors at the new normal: the second form keeps it as D.
RT_LIGHT_FN void next_level(const rt_scene& s, Bounce b, Vec3 R, Vec3& p, Vec3& n, int32_t& obj) {
    const Vec3 p2 = bounce_point(p, R, b.best);
    n = bounce_normal(s, b.obj2, b.tri2, p2, R);
    p = p2;
    obj = b.obj2;
}
RT_LIGHT_FN void next_level(const rt_scene& s, Bounce b, Vec3 R, Vec3& p, Vec3& n, Vec3& D,
                            int32_t& obj) {
    next_level(s, b, R, p, n, obj);
    D = R;
}

// The geometry of bounce number `bounce` (j .. RT_MAX_BOUNCES) of a chain whose
// bounce number j leaves the reached level (p, n, D, obj), followed without
// regard to reflectivity, lights or t.  (kFar, -1) where this bounce or an
// earlier one met nothing.
template <typename W>
RT_LIGHT_FN Bounce bounce_chain_from(const rt_scene& s, Vec3 p, Vec3 n, Vec3 D, int32_t obj,
                                     int32_t j, int32_t bounce, const W& w) {
    for (;; ++j) {
        const Vec3 R = mirror_dir(n, D);
        const Bounce b = w.bounce(s, obj, p, R);
        if (b.obj2 < 0 || j >= bounce) return b;
        next_level(s, b, R, p, n, D, obj);
    }
}

// The geometry of bounce number `bounce` (1 .. RT_MAX_BOUNCES) of one pixel's
// chain; (kFar, -1) for a miss too.
template <typename W = Walks>
RT_LIGHT_FN Bounce bounce_chain_pixel(const rt_scene& s, int32_t obj, const float* verts, float ox,
                                      float oy, Vec3 d, float t, int32_t bounce,
                                      const W& w = W()) {
    if (obj < 0) return Bounce{kFar, -1, -1};
    const Vec3 p = hit_point(ox, oy, d, t);
    const rt_surface sf = surface(s, obj, verts, ox, oy, d, t, p);
    return bounce_chain_from(s, p, Vec3{sf.nx, sf.ny, sf.nz}, d, obj, 1, bounce, w);
}

// The level loop and the backward blend of a chain of at most `max_bounces`
// (0 .. RT_MAX_BOUNCES) bounces from the reached level 0 (p, n, D, obj) at depth
// T, into the int32x4 pixel.  `reflectivity` is read at the slots of levels
// below max_bounces only.
template <typename W>
RT_LIGHT_FN void lit_chain_from(const rt_scene& s, Vec3 p, Vec3 n, Vec3 D, int32_t obj, float T,
                                const float* reflectivity, int32_t max_bounces, bool shadows,
                                int32_t out[4], const W& w) {
    Vec3 a[RT_MAX_BOUNCES];  // the levels the chain went on from
    float r[RT_MAX_BOUNCES];
    Vec3 C{0.0f, 0.0f, 0.0f};
    int32_t j = 0;
    for (;; ++j) {
        float k = 1.0f;
        if (s.num_lights > 0)
            k = shadows ? shadowed_factor(s, obj, n, p, w)
                        : light_factor(n, p, s.lights, s.num_lights);
        const Vec3 own = chain_colour(chain_scalar(T, j >= 1), k, slot_colour(s, obj));
        const float rj = j < max_bounces ? slot_reflectivity(reflectivity, obj) : 0.0f;
        if (!(rj != 0.0f)) {  // by depth or by a matte object: C_J = a_J
            C = own;
            break;
        }
        a[j] = own;
        r[j] = rj;
        const Vec3 R = mirror_dir(n, D);
        const Bounce b = w.bounce(s, obj, p, R);
        if (b.obj2 < 0) {  // by a miss after level j: C_{j+1} = (0, 0, 0)
            ++j;
            break;
        }
        next_level(s, b, R, p, n, D, obj);
        T = T + b.best;
    }
    for (int32_t l = j - 1; l >= 0; --l) C = chain_blend(a[l], r[l], C);
    out[0] = cvt_i32(C.x);
    out[1] = cvt_i32(C.y);
    out[2] = cvt_i32(C.z);
    out[3] = 255;
}

// One pixel of the mirrored frame (int32x4): the chain from the hit frame's
// level 0.  A miss, and t == kFar, are lit_pixel's (with `shadows`,
// lit_pixel_shadowed's).
template <typename W = Walks>
RT_LIGHT_FN void lit_pixel_mirrored(const rt_scene& s, int32_t obj, const float* verts, float ox,
                                    float oy, Vec3 d, float t, const float* reflectivity,
                                    int32_t max_bounces, bool shadows, int32_t out[4],
                                    const W& w = W()) {
    if (obj < 0 || t == kFar) {
        if (shadows)
            lit_pixel_shadowed(s, obj, verts, ox, oy, d, t, out, w);
        else
            lit_pixel(s, obj, verts, ox, oy, d, t, out);
        return;
    }
    const Vec3 p = hit_point(ox, oy, d, t);
    const rt_surface sf = surface(s, obj, verts, ox, oy, d, t, p);
    lit_chain_from(s, p, Vec3{sf.nx, sf.ny, sf.nz}, d, obj, t, reflectivity, max_bounces, shadows,
                   out, w);
}

}  // namespace rt_light

#endif /* RT_LIGHT_IMPL_H */
