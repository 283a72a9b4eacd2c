// rt_light_accel.cpp -- the culled light pass on the host:
// rt_shadow_hits_accel, rt_bounce_hits_accel and rt_light_hits_mirrored_accel.
// rt_light.cpp's functions of the same names without `_accel`, word for word in
// what they return: the same pixel loop (include/rt_light_run.h) over the same
// pixel functions (include/rt_light_impl.h), which take the culled walks of
// include/rt_accel_impl.h in place of the unculled ones, behind the same
// checks of the settings and the reflectivity array (rt_light.cpp).
// Plain C++, no HIP; built with -ffp-contract=off like rt_light.cpp.
#include "rt_accel_impl.h"
#include "rt_hip.h"
#include "rt_light_run.h"

namespace {

using namespace rt_light;

// The unculled call's checks, then the record's.
int check_light_accel(const rt_hit* hits, const rt_scene* scene, const float* ray_dir,
                      int32_t width, int32_t row_begin, int32_t row_end, bool mask,
                      const rt_cube_bound* accel, const void* out) {
    const int rc = check(hits, scene, ray_dir, width, row_begin, row_end, out);
    if (rc) return rc;
    if (mask && scene->num_lights > 32) return RT_ERR_UNSUPPORTED;
    return check_accel(scene, accel);
}

}  // namespace

extern "C" {

int rt_shadow_hits_accel(const rt_hit* hits, const rt_scene* scene, const rt_cube_bound* accel,
                         const float ray_dir[4], int32_t width, int32_t row_begin,
                         int32_t row_end, uint32_t* out) {
    const int rc =
        check_light_accel(hits, scene, ray_dir, width, row_begin, row_end, true, accel, out);
    if (rc) return rc;
    return run(hits, scene, ray_dir, width, row_begin, row_end, true, 0, out,
               [w = CulledWalks{accel}](const auto&... a) { return shadow_pixel(a..., w); });
}

int rt_bounce_hits_accel(const rt_hit* hits, const rt_scene* scene, const rt_cube_bound* accel,
                         const float ray_dir[4], int32_t width, int32_t row_begin,
                         int32_t row_end, int32_t bounce, rt_hit* out) {
    if (bounce < 1 || bounce > RT_MAX_BOUNCES) return RT_ERR_INVALID_ARG;
    const int rc =
        check_light_accel(hits, scene, ray_dir, width, row_begin, row_end, false, accel, out);
    if (rc) return rc;
    return run(hits, scene, ray_dir, width, row_begin, row_end, false, 0, out,
               [bounce, w = CulledWalks{accel}](const auto&... a) {
                   const Bounce b = bounce_chain_pixel(a..., bounce, w);
                   return rt_hit{b.best, b.obj2};
               });
}

int rt_light_hits_mirrored_accel(const rt_hit* hits, const rt_scene* scene,
                                 const rt_cube_bound* accel, const float ray_dir[4],
                                 int32_t width, int32_t row_begin, int32_t row_end,
                                 const float* reflectivity, int32_t max_bounces, int32_t shadows,
                                 int32_t out_format, void* out) {
    int rc = check_chain_settings(scene, reflectivity, max_bounces, shadows, out_format);
    if (!rc)
        rc = check_light_accel(hits, scene, ray_dir, width, row_begin, row_end, false, accel, out);
    bool mirrors = false;
    if (!rc) rc = check_reflectivity(*scene, reflectivity, mirrors);
    if (rc) return rc;
    const CulledWalks w{accel};
    if (max_bounces == 0 || !mirrors) {  // no bounce walk
        if (!shadows)  // rt_light_hits' frame: no walk at all
            return rt_light_hits(hits, scene, ray_dir, width, row_begin, row_end, out_format, out);
        return run(hits, scene, ray_dir, width, row_begin, row_end, false, out_format, out,
                   [w](const auto&... a) {
                       Lit l;
                       lit_pixel_shadowed(a..., l.p, w);
                       return l;
                   });
    }
    return run(hits, scene, ray_dir, width, row_begin, row_end, false, out_format, out,
               [=](const auto&... a) {
                   Lit l;
                   lit_pixel_mirrored(a..., reflectivity, max_bounces, shadows != 0, l.p, w);
                   return l;
               });
}

}  // extern "C"
