/*
 * rt_camera_light_impl.h -- the light pass of a camera view, rt_light_camera*
 * and rt_bounce_camera* (DESIGN.md §3.1i): the per-pixel functions, one text
 * for the unculled and the culled walks (templates over rt_light_impl.h's Walks
 * / rt_accel_impl.h's CulledWalks), and the argument checks the host functions
 * (csrc/rt_camera_light.cpp) share with the kernels' launch
 * (csrc/rt_camera_light.hip).  Internal: not installed, not part of the ABI.
 *
 * A camera pixel is the mirror chain of rt_light_impl.h with level 0 found by
 * a cast of the pixel's own ray, camera_ray(cam, x, y), instead of read from a
 * hit frame: no triangle is identified again (cube_surface) and no hit frame
 * is stored.  The level loop and the backward blend are rt_light_impl.h's
 * lit_chain_from and bounce_chain_from, the text lit_pixel_mirrored and
 * bounce_chain_pixel run from the hit frame's level 0.
 *
 * Known limit, as for every bounce: a level reached from inside an object (the
 * eye inside a sphere, whose far root the cast takes) still leaves that object
 * out of the next walk and of the shadow walks there.
 *
 * The conventions are rt_light_impl.h's: every fp32 operation is written on its
 * own and rounds once, no contraction, sums in the written order.
 */
#ifndef RT_CAMERA_LIGHT_IMPL_H
#define RT_CAMERA_LIGHT_IMPL_H

#include "rt_accel_impl.h"
#include "rt_rays_impl.h"

namespace rt_light {

/* The checks of rt_light_camera* / rt_bounce_camera* (RT_OK,
 * RT_ERR_INVALID_ARG or RT_ERR_UNSUPPORTED), everything the host can see:
 * check_camera() with `out` aligned to `out_align`, and a non-NULL `accel`
 * aligned to 16 bytes.  csrc/rt_camera_light.cpp. */
int check_camera_light(const rt_camera* camera, const rt_scene* scene, const rt_cube_bound* accel,
                       int32_t width, int32_t row_begin, int32_t row_end, const void* out,
                       uintptr_t out_align);

// rt_bounce_camera's pixel: the cast's hit for bounce 0, else the hit of that
// bounce of the chain (bounce_chain_from, from the level the cast reached);
// (kFar, -1) where it or an earlier level met nothing.
template <typename W>
RT_LIGHT_FN Bounce bounce_camera_pixel(const rt_scene& s, Ray ray, int32_t bounce, const W& w) {
    const Bounce b0 = w.bounce(s, -1, ray.o, ray.d);
    if (b0.obj2 < 0 || bounce <= 0) return b0;
    Vec3 p = ray.o, n{0.0f, 0.0f, 0.0f};
    int32_t obj = -1;
    next_level(s, b0, ray.d, p, n, obj);
    return bounce_chain_from(s, p, n, ray.d, obj, 1, bounce, w);
}

// rt_light_camera's pixel (int32x4): level 0 by the cast, then the chain
// (lit_chain_from).  `reflectivity` is read at the slots of levels below
// max_bounces only.
template <typename W>
RT_LIGHT_FN void lit_camera_pixel(const rt_scene& s, Ray ray, const float* reflectivity,
                                  int32_t max_bounces, bool shadows, int32_t out[4], const W& w) {
    out[0] = out[1] = out[2] = 0;  // rt_shade_hits' miss pixel
    out[3] = 255;
    const Bounce b0 = w.bounce(s, -1, ray.o, ray.d);
    if (b0.obj2 < 0) return;
    Vec3 p = ray.o, n{0.0f, 0.0f, 0.0f};
    int32_t obj = -1;
    next_level(s, b0, ray.d, p, n, obj);
    lit_chain_from(s, p, n, ray.d, obj, b0.best, reflectivity, max_bounces, shadows, out, w);
}

}  // namespace rt_light

#endif /* RT_CAMERA_LIGHT_IMPL_H */
