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
 * is stored.  The level loop and the backward blend are lit_pixel_mirrored's,
 * restated here so that rt_light_impl.h and everything compiled from it stay
 * as they are.
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
/* The settings of rt_light_camera*: the format, max_bounces, shadows, and a
 * NULL reflectivity where a chain could read it.  `scene` may be NULL (refused
 * by check_camera_light). */
int check_camera_lit(const rt_scene* scene, const float* reflectivity, int32_t max_bounces,
                     int32_t shadows, int32_t out_format);

// The level the bounce `b` from p along R met, in place: point, faced normal
// and object.  R is the direction the level was reached along: the caller
// keeps it as D and mirrors it at the new normal for the next bounce.
RT_LIGHT_FN void camera_next_level(const rt_scene& s, Bounce b, Vec3 R, Vec3& p, Vec3& n,
                                   int32_t& obj) {
    const Vec3 p2 = bounce_point(p, R, b.best);
    n = bounce_normal(s, b.obj2, b.tri2, p2, R);
    p = p2;
    obj = b.obj2;
}

// rt_bounce_camera's pixel: the cast's hit for bounce 0, else the hit of that
// bounce of the chain (bounce_chain_pixel started from the cast); (kFar, -1)
// where it or an earlier level met nothing.
template <typename W>
RT_LIGHT_FN Bounce bounce_camera_pixel(const rt_scene& s, Ray ray, int32_t bounce, const W& w) {
    Vec3 p = ray.o, R = ray.d, n{0.0f, 0.0f, 0.0f};
    int32_t obj = -1;
    for (int32_t j = 0;; ++j) {
        const Bounce b = w.bounce(s, obj, p, R);
        if (b.obj2 < 0 || j >= bounce) return b;
        camera_next_level(s, b, R, p, n, obj);
        R = mirror_dir(n, R);
    }
}

// rt_light_camera's pixel (int32x4): level 0 by the cast, then
// lit_pixel_mirrored's level loop and backward blend.  `reflectivity` is read
// at the slots of levels below max_bounces only.
template <typename W>
RT_LIGHT_FN void lit_camera_pixel(const rt_scene& s, Ray ray, const float* reflectivity,
                                  int32_t max_bounces, bool shadows, int32_t out[4], const W& w) {
    out[0] = out[1] = out[2] = 0;  // rt_shade_hits' miss pixel
    out[3] = 255;
    const Bounce b0 = w.bounce(s, -1, ray.o, ray.d);
    if (b0.obj2 < 0) return;
    Vec3 p = ray.o, n{0.0f, 0.0f, 0.0f}, D = ray.d;
    int32_t obj = -1;
    camera_next_level(s, b0, D, p, n, obj);
    float T = b0.best;
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
        camera_next_level(s, b, R, p, n, obj);
        D = R;
        T = T + b.best;
    }
    for (int32_t l = j - 1; l >= 0; --l) C = chain_blend(a[l], r[l], C);
    out[0] = cvt_i32(C.x);
    out[1] = cvt_i32(C.y);
    out[2] = cvt_i32(C.z);
}

}  // namespace rt_light

#endif /* RT_CAMERA_LIGHT_IMPL_H */
