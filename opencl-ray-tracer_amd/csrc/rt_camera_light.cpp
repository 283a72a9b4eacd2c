// rt_camera_light.cpp -- the light pass of a camera view on the host
// (DESIGN.md §3.1i): rt_light_camera and rt_bounce_camera, and the argument
// checks they share with rt_camera_light.hip.  One pixel loop over the pixel
// functions of include/rt_camera_light_impl.h, which take the unculled walks
// (accel == NULL) or the culled ones.  rt_light_run.h's loop reads a hit frame,
// which these calls do not have; its Lit and its store_pixel are used as they are.
// Plain C++, no HIP; built with -ffp-contract=off like rt_light.cpp.
#include "rt_camera_light_impl.h"
#include "rt_hip.h"
#include "rt_light_run.h"

namespace rt_light {

int check_camera_light(const rt_camera* camera, const rt_scene* scene, const rt_cube_bound* accel,
                       int32_t width, int32_t row_begin, int32_t row_end, const void* out,
                       uintptr_t out_align) {
    const int rc =
        check_camera(camera, scene, true, width, row_begin, row_end, out, out_align, nullptr);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(accel) % 16 != 0) return RT_ERR_INVALID_ARG;
    return RT_OK;
}

namespace {

// The pixel loop of both calls: `pixel(ray)` per pixel of the band, row-major;
// what it returns is stored by store_pixel.
template <typename PixelFn>
void run_camera(const rt_camera& cam, int32_t width, int32_t row_begin, int32_t row_end,
                int32_t fmt, void* out, PixelFn pixel) {
    int64_t i = 0;
    for (int32_t y = row_begin; y < row_end; ++y)
        for (int32_t x = 0; x < width; ++x, ++i)
            store_pixel(out, i, fmt,
                        pixel(camera_ray(cam, static_cast<float>(x), static_cast<float>(y))));
}

template <typename W>
void bounce_camera(const rt_camera& cam, const rt_scene& s, int32_t width, int32_t row_begin,
                   int32_t row_end, int32_t bounce, rt_hit* out, const W& w) {
    run_camera(cam, width, row_begin, row_end, 0, out, [&](const Ray& ray) {
        const Bounce b = bounce_camera_pixel(s, ray, bounce, w);
        return rt_hit{b.best, b.obj2};
    });
}

template <typename W>
void light_camera(const rt_camera& cam, const rt_scene& s, int32_t width, int32_t row_begin,
                  int32_t row_end, const float* reflectivity, int32_t max_bounces, bool shadows,
                  int32_t fmt, void* out, const W& w) {
    run_camera(cam, width, row_begin, row_end, fmt, out, [&](const Ray& ray) {
        Lit l;
        lit_camera_pixel(s, ray, reflectivity, max_bounces, shadows, l.p, w);
        return l;
    });
}

}  // namespace
}  // namespace rt_light

extern "C" {

using namespace rt_light;

int rt_bounce_camera(const rt_camera* camera, const rt_scene* scene, const rt_cube_bound* accel,
                     int32_t width, int32_t row_begin, int32_t row_end, int32_t bounce,
                     rt_hit* out) {
    if (bounce < 0 || bounce > RT_MAX_BOUNCES) return RT_ERR_INVALID_ARG;
    const int rc = check_camera_light(camera, scene, accel, width, row_begin, row_end, out,
                                      sizeof(rt_hit));
    if (rc) return rc;
    if (accel)
        bounce_camera(*camera, *scene, width, row_begin, row_end, bounce, out, CulledWalks{accel});
    else
        bounce_camera(*camera, *scene, width, row_begin, row_end, bounce, out, Walks{});
    return RT_OK;
}

int rt_light_camera(const rt_camera* camera, const rt_scene* scene, const rt_cube_bound* accel,
                    int32_t width, int32_t row_begin, int32_t row_end, const float* reflectivity,
                    int32_t max_bounces, int32_t shadows, int32_t out_format, void* out) {
    int rc = check_chain_settings(scene, reflectivity, max_bounces, shadows, out_format);
    if (!rc)
        rc = check_camera_light(camera, scene, accel, width, row_begin, row_end, out,
                                out_format == RT_FORMAT_I32X4 ? 16 : 4);
    bool mirrors = false;
    if (!rc) rc = check_reflectivity(*scene, reflectivity, mirrors);
    if (rc) return rc;
    // without an array no slot can be read (an empty scene): depth 0
    const int32_t depth = reflectivity ? max_bounces : 0;
    if (accel)
        light_camera(*camera, *scene, width, row_begin, row_end, reflectivity, depth, shadows != 0,
                     out_format, out, CulledWalks{accel});
    else
        light_camera(*camera, *scene, width, row_begin, row_end, reflectivity, depth, shadows != 0,
                     out_format, out, Walks{});
    return RT_OK;
}

}  // extern "C"
