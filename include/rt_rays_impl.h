/*
 * rt_rays_impl.h -- the ray queries, rt_cast_rays* / rt_occlude_rays* /
 * rt_camera_rays* / rt_cast_camera* (DESIGN.md §3.1f): the camera arithmetic
 * and the handling of a ray's `skip`, one text for the host functions
 * (csrc/rt_light.cpp) and the kernels (csrc/rt_rays.hip), and their shared
 * argument checks.  The walks themselves are rt_light_impl.h's bounce_walk and
 * light_occluded, as they are.  Internal: not installed, not part of the ABI.
 *
 * The conventions are rt_light_impl.h's: every fp32 operation is written on its
 * own and rounds once, no contraction, sums in the written order.
 */
#ifndef RT_RAYS_IMPL_H
#define RT_RAYS_IMPL_H

#include "rt_light_impl.h"

namespace rt_light {

/* The checks of the ray entry points (RT_OK, RT_ERR_INVALID_ARG or
 * RT_ERR_UNSUPPORTED), everything the host can see: NULL pointers (`triangle`
 * may be NULL), n < 0, the scene checks of check(), the alignment of every
 * pointer (rays 16 bytes, `out` by `out_align`, triangle 4), and more rays
 * than one launch of the light pass takes (2^39).  csrc/rt_light.cpp. */
int check_rays(const rt_ray* rays, int64_t n, const rt_scene* scene, const void* out,
               uintptr_t out_align, const int32_t* triangle);
/* The same for the camera calls: the camera (normalise is 0 or 1), the band
 * checks of check(), and `scene` where the call takes one (`with_scene`). */
int check_camera(const rt_camera* camera, const rt_scene* scene, bool with_scene, int32_t width,
                 int32_t row_begin, int32_t row_end, const void* out, uintptr_t out_align,
                 const int32_t* triangle);

// Is `p` off a multiple of `align` bytes?  (NULL is not.)
inline bool misaligned(const void* p, uintptr_t align) {
    return reinterpret_cast<uintptr_t>(p) % align != 0;
}

// One launch's grid: 2^31 - 1 workgroups of 256 rays.
constexpr int64_t kMaxRays = static_cast<int64_t>(INT32_MAX) * 256;

struct Ray {
    Vec3 o, d;
};

// A ray's `skip` as the kernels read it: an id outside [-1, nc + ns) is no
// object.  (The host functions refuse such a ray.)  In front of every
// comparison: `own - num_cubes` in the sphere loop must not overflow.
RT_LIGHT_FN int32_t ray_skip(const rt_scene& s, int32_t skip) {
    return (skip < -1 || static_cast<int64_t>(skip) >= static_cast<int64_t>(s.num_cubes) +
                                                           s.num_spheres)
               ? -1
               : skip;
}

// The ray of pixel (fx, fy) of an affine camera: per component
// (a0 + fx * au) + fy * av for the origin and the direction, then, with
// `normalise`, d / |d| as normalise() writes it.
RT_LIGHT_FN Ray camera_ray(const rt_camera& c, float fx, float fy) {
    Ray r;
    r.o = Vec3{(c.o0[0] + fx * c.ou[0]) + fy * c.ov[0], (c.o0[1] + fx * c.ou[1]) + fy * c.ov[1],
               (c.o0[2] + fx * c.ou[2]) + fy * c.ov[2]};
    r.d = Vec3{(c.d0[0] + fx * c.du[0]) + fy * c.dv[0], (c.d0[1] + fx * c.du[1]) + fy * c.dv[1],
               (c.d0[2] + fx * c.du[2]) + fy * c.dv[2]};
    if (c.normalise) r.d = normalise(r.d);
    return r;
}

}  // namespace rt_light

#endif /* RT_RAYS_IMPL_H */
