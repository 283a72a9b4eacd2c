// rt_light.cpp -- rt_hit_surfaces / rt_light_hits, the shadow term's
// rt_shadow_hits / rt_light_hits_shadowed and the mirror bounce's
// rt_reflect_hits / rt_light_hits_reflected and the two together,
// rt_shadow_hits_reflected / rt_light_hits_shadowed_reflected, and the mirror
// chain's rt_bounce_hits / rt_light_hits_mirrored, on the host, and
// the argument checks they share with the device entry points (the launch of
// rt_light_device.inc, for every kernel over a hit frame) and with the culled
// and the camera calls (check_chain_settings, check_reflectivity).  One pixel
// loop, run() of include/rt_light_run.h; each function is its argument checks
// and the per-pixel call it hands to the loop.  Behind them the ray queries, rt_cast_rays / rt_occlude_rays /
// rt_camera_rays / rt_cast_camera: the loops of include/rt_rays_run.h over the
// unculled walks and the camera text of include/rt_rays_impl.h, and the checks
// they share with rt_rays.hip.
// Plain C++, no HIP.  The arithmetic is include/rt_light_impl.h, the text the
// kernel compiles too; built with -ffp-contract=off like rt_scene.cpp.
#include "rt_args.h"
#include "rt_hip.h"
#include "rt_light_impl.h"
#include "rt_light_run.h"
#include "rt_rays_impl.h"
#include "rt_rays_run.h"

namespace rt_light {

int check(const rt_hit* hits, const rt_scene* scene, const float* ray_dir, int32_t width,
          int32_t row_begin, int32_t row_end, const void* out) {
    if (!hits || !scene || !ray_dir || !out) return RT_ERR_INVALID_ARG;
    // a band of a frame of row_end rows: rt_render's own limits and counts
    if (rt_args::check_args(scene, width, row_end, row_begin, row_end, RT_FORMAT_I32X4))
        return RT_ERR_INVALID_ARG;
    if (scene->num_lights > 0 && !scene->lights) return RT_ERR_INVALID_ARG;
    return RT_OK;
}

int check_chain_settings(const rt_scene* scene, const float* reflectivity, int32_t max_bounces,
                         int32_t shadows, int32_t out_format) {
    if (out_format != RT_FORMAT_I32X4 && out_format != RT_FORMAT_RGBA8) return RT_ERR_INVALID_ARG;
    if (max_bounces < 0 || max_bounces > RT_MAX_BOUNCES) return RT_ERR_INVALID_ARG;
    if (shadows != 0 && shadows != 1) return RT_ERR_INVALID_ARG;
    // the array may be missing only where no slot of it can be read
    if (!reflectivity && max_bounces > 0 && scene &&
        static_cast<int64_t>(scene->num_cubes) + scene->num_spheres > 0)
        return RT_ERR_INVALID_ARG;
    return RT_OK;
}

int check_reflectivity(const rt_scene& scene, const float* reflectivity, bool& mirrors) {
    const int64_t n_slots = static_cast<int64_t>(scene.num_cubes) + scene.num_spheres;
    mirrors = false;
    if (reflectivity)
        for (int64_t i = 0; i < n_slots; ++i) {
            if (!(reflectivity[i] >= 0.0f && reflectivity[i] <= 1.0f)) return RT_ERR_INVALID_ARG;
            mirrors = mirrors || reflectivity[i] != 0.0f;
        }
    return RT_OK;
}

int check_rays(const rt_ray* rays, int64_t n, const rt_scene* scene, const void* out,
               uintptr_t out_align, const int32_t* triangle) {
    if (!rays || !scene || !out || n < 0) return RT_ERR_INVALID_ARG;
    // the scene alone: rt_render's counts and arrays, on a frame of one pixel
    if (rt_args::check_args(scene, 1, 1, 0, 1, RT_FORMAT_I32X4)) return RT_ERR_INVALID_ARG;
    if (scene->num_lights > 0 && !scene->lights) return RT_ERR_INVALID_ARG;
    if (misaligned(rays, 16) || misaligned(out, out_align) || misaligned(triangle, 4))
        return RT_ERR_INVALID_ARG;
    return n > kMaxRays ? RT_ERR_UNSUPPORTED : RT_OK;
}

int check_camera(const rt_camera* camera, const rt_scene* scene, bool with_scene, int32_t width,
                 int32_t row_begin, int32_t row_end, const void* out, uintptr_t out_align,
                 const int32_t* triangle) {
    if (!camera || !out || (with_scene && !scene)) return RT_ERR_INVALID_ARG;
    if (camera->normalise != 0 && camera->normalise != 1) return RT_ERR_INVALID_ARG;
    const rt_scene none{};  // rt_camera_rays: the band checks alone
    const rt_scene* s = with_scene ? scene : &none;
    if (rt_args::check_args(s, width, row_end, row_begin, row_end, RT_FORMAT_I32X4))
        return RT_ERR_INVALID_ARG;
    if (s->num_lights > 0 && !s->lights) return RT_ERR_INVALID_ARG;
    if (misaligned(out, out_align) || misaligned(triangle, 4)) return RT_ERR_INVALID_ARG;
    return static_cast<int64_t>(row_end - row_begin) * width > kMaxRays ? RT_ERR_UNSUPPORTED
                                                                        : RT_OK;
}

}  // namespace rt_light

extern "C" {

using namespace rt_light;

// ---- the ray queries -------------------------------------------

// The closest hit of every ray: bounce_walk from o along d, `skip` left out.
int rt_cast_rays(const rt_ray* rays, int64_t n, const rt_scene* scene, rt_hit* out_hits,
                 int32_t* out_triangle) {
    const int rc = check_rays(rays, n, scene, out_hits, sizeof(rt_hit), out_triangle);
    return rc ? rc : cast_rays(rays, n, *scene, out_hits, out_triangle, Walks{});
}

// Is the open segment (o, o + d) of every ray cut: light_occluded, `skip` left out.
int rt_occlude_rays(const rt_ray* rays, int64_t n, const rt_scene* scene, uint8_t* out_occluded) {
    const int rc = check_rays(rays, n, scene, out_occluded, 1, nullptr);
    return rc ? rc : occlude_rays(rays, n, *scene, out_occluded, Walks{});
}

// The rays of a band of a camera's frame, row-major.
int rt_camera_rays(const rt_camera* camera, int32_t width, int32_t row_begin, int32_t row_end,
                   rt_ray* out_rays) {
    const int rc =
        check_camera(camera, nullptr, false, width, row_begin, row_end, out_rays, 16, nullptr);
    if (rc) return rc;
    int64_t i = 0;
    for (int32_t y = row_begin; y < row_end; ++y)
        for (int32_t x = 0; x < width; ++x, ++i) {
            const Ray r = camera_ray(*camera, static_cast<float>(x), static_cast<float>(y));
            out_rays[i] = rt_ray{r.o.x, r.o.y, r.o.z, -1, r.d.x, r.d.y, r.d.z, 0.0f};
        }
    return RT_OK;
}

// rt_cast_rays on rt_camera_rays' rays, without the rays.
int rt_cast_camera(const rt_camera* camera, const rt_scene* scene, int32_t width,
                   int32_t row_begin, int32_t row_end, rt_hit* out_hits, int32_t* out_triangle) {
    const int rc = check_camera(camera, scene, true, width, row_begin, row_end, out_hits,
                                sizeof(rt_hit), out_triangle);
    return rc ? rc
              : cast_camera(*camera, *scene, width, row_begin, row_end, out_hits, out_triangle,
                            Walks{});
}

// The geometry of one bounce of the mirror chain.
int rt_bounce_hits(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                   int32_t width, int32_t row_begin, int32_t row_end, int32_t bounce,
                   rt_hit* out) {
    if (bounce < 1 || bounce > RT_MAX_BOUNCES) return RT_ERR_INVALID_ARG;
    return run(hits, scene, ray_dir, width, row_begin, row_end, false, 0, out,
               [bounce](const auto&... a) {
                   const Bounce b = bounce_chain_pixel(a..., bounce);
                   return rt_hit{b.best, b.obj2};
               });
}

// The lit frame with a mirror chain and one reflectivity per colour slot.
int rt_light_hits_mirrored(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                           int32_t width, int32_t row_begin, int32_t row_end,
                           const float* reflectivity, int32_t max_bounces, int32_t shadows,
                           int32_t out_format, void* out) {
    int rc = check_chain_settings(scene, reflectivity, max_bounces, shadows, out_format);
    if (!rc) rc = check(hits, scene, ray_dir, width, row_begin, row_end, out);
    bool mirrors = false;
    if (!rc) rc = check_reflectivity(*scene, reflectivity, mirrors);
    if (rc) return rc;
    if (max_bounces == 0 || !mirrors)  // rt_light_hits' / rt_light_hits_shadowed's frame, no walk
        return shadows ? rt_light_hits_shadowed(hits, scene, ray_dir, width, row_begin, row_end,
                                                out_format, out)
                       : rt_light_hits(hits, scene, ray_dir, width, row_begin, row_end,
                                       out_format, out);
    return run(hits, scene, ray_dir, width, row_begin, row_end, false, out_format, out,
               [=](const auto&... a) {
                   Lit l;
                   lit_pixel_mirrored(a..., reflectivity, max_bounces, shadows != 0, l.p);
                   return l;
               });
}

// The mask at the point the bounce meets.
int rt_shadow_hits_reflected(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                             int32_t width, int32_t row_begin, int32_t row_end, uint32_t* out) {
    return run(hits, scene, ray_dir, width, row_begin, row_end, true, 0, out,
               [](const auto&... a) { return shadow_reflect_pixel(a...); });
}

int rt_light_hits_shadowed_reflected(const rt_hit* hits, const rt_scene* scene,
                                     const float ray_dir[4], int32_t width, int32_t row_begin,
                                     int32_t row_end, float reflectivity, int32_t out_format,
                                     void* out) {
    if (out_format != RT_FORMAT_I32X4 && out_format != RT_FORMAT_RGBA8) return RT_ERR_INVALID_ARG;
    if (!(reflectivity >= 0.0f && reflectivity <= 1.0f)) return RT_ERR_INVALID_ARG;  // NaN too
    if (reflectivity == 0.0f)  // rt_light_hits_shadowed's frame, neither the bounce nor its walk
        return rt_light_hits_shadowed(hits, scene, ray_dir, width, row_begin, row_end, out_format,
                                      out);
    return run(hits, scene, ray_dir, width, row_begin, row_end, false, out_format, out,
               [r = reflectivity](const auto&... a) {
                   Lit l;
                   lit_pixel_shadowed_reflected(a..., r, l.p);
                   return l;
               });
}

// The bounce's rt_hit per pixel.
int rt_reflect_hits(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                    int32_t width, int32_t row_begin, int32_t row_end, rt_hit* out) {
    return run(hits, scene, ray_dir, width, row_begin, row_end, false, 0, out,
               [](const auto&... a) {
                   const Bounce b = bounce_pixel(a...);
                   return rt_hit{b.best, b.obj2};
               });
}

int rt_light_hits_reflected(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                            int32_t width, int32_t row_begin, int32_t row_end, float reflectivity,
                            int32_t out_format, void* out) {
    if (out_format != RT_FORMAT_I32X4 && out_format != RT_FORMAT_RGBA8) return RT_ERR_INVALID_ARG;
    if (!(reflectivity >= 0.0f && reflectivity <= 1.0f)) return RT_ERR_INVALID_ARG;  // NaN too
    if (reflectivity == 0.0f)  // rt_light_hits' frame, no walk
        return rt_light_hits(hits, scene, ray_dir, width, row_begin, row_end, out_format, out);
    return run(hits, scene, ray_dir, width, row_begin, row_end, false, out_format, out,
               [r = reflectivity](const auto&... a) {
                   Lit l;
                   lit_pixel_reflected(a..., r, l.p);
                   return l;
               });
}

// The uint32 mask per pixel.
int rt_shadow_hits(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                   int32_t width, int32_t row_begin, int32_t row_end, uint32_t* out) {
    return run(hits, scene, ray_dir, width, row_begin, row_end, true, 0, out,
               [](const auto&... a) { return shadow_pixel(a...); });
}

int rt_light_hits_shadowed(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                           int32_t width, int32_t row_begin, int32_t row_end, int32_t out_format,
                           void* out) {
    if (out_format != RT_FORMAT_I32X4 && out_format != RT_FORMAT_RGBA8) return RT_ERR_INVALID_ARG;
    return run(hits, scene, ray_dir, width, row_begin, row_end, false, out_format, out,
               [](const auto&... a) {
                   Lit l;
                   lit_pixel_shadowed(a..., l.p);
                   return l;
               });
}

int rt_hit_surfaces(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4],
                    int32_t width, int32_t row_begin, int32_t row_end, rt_surface* out) {
    return run(hits, scene, ray_dir, width, row_begin, row_end, false, 0, out,
               [](const rt_scene& s, int32_t obj, const float* verts, float ox, float oy, Vec3 d,
                  float t) { return surface(s, obj, verts, ox, oy, d, t, hit_point(ox, oy, d, t)); });
}

int rt_light_hits(const rt_hit* hits, const rt_scene* scene, const float ray_dir[4], int32_t width,
                  int32_t row_begin, int32_t row_end, int32_t out_format, void* out) {
    if (out_format != RT_FORMAT_I32X4 && out_format != RT_FORMAT_RGBA8) return RT_ERR_INVALID_ARG;
    return run(hits, scene, ray_dir, width, row_begin, row_end, false, out_format, out,
               [](const auto&... a) {
                   Lit l;
                   lit_pixel(a..., l.p);
                   return l;
               });
}

}  // extern "C"
