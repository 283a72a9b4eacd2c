/*
 * rt_rays_run.h -- the loops of the host functions of the ray queries
 * (csrc/rt_light.cpp, csrc/rt_accel.cpp, csrc/rt_sphere_groups.cpp): rays to
 * hits, rays to occluded bytes, a camera's band to hits, and rays to kept
 * counts, one text each for the plain, the *_accel and the *_grouped calls.
 * Templates over a pair of walks (rt_light_impl.h's Walks, rt_accel_impl.h's
 * CulledWalks, rt_sphere_groups_impl.h's GroupedWalks), in the spirit of run()
 * of rt_light_run.h.  Every loop runs behind its caller's argument checks.
 * Host only.  Internal: not installed, not part of the ABI.
 */
#ifndef RT_RAYS_RUN_H
#define RT_RAYS_RUN_H

#include "rt_hip.h"
#include "rt_rays_impl.h"

namespace rt_light {

// The closest hit of every ray: w.bounce from o along d, `skip` left out.  A
// ray whose `skip` is no object of the scene ends the call.
template <typename W>
int cast_rays(const rt_ray* rays, int64_t n, const rt_scene& s, rt_hit* out_hits,
              int32_t* out_triangle, const W& w) {
    for (int64_t i = 0; i < n; ++i) {
        const rt_ray& r = rays[i];
        if (ray_skip(s, r.skip) != r.skip) return RT_ERR_INVALID_ARG;
        const Bounce b = w.bounce(s, r.skip, Vec3{r.ox, r.oy, r.oz}, Vec3{r.dx, r.dy, r.dz});
        out_hits[i] = rt_hit{b.best, b.obj2};
        if (out_triangle) out_triangle[i] = b.tri2;
    }
    return RT_OK;
}

// Is the open segment (o, o + d) of every ray cut: w.occluded, `skip` left out.
template <typename W>
int occlude_rays(const rt_ray* rays, int64_t n, const rt_scene& s, uint8_t* out_occluded,
                 const W& w) {
    for (int64_t i = 0; i < n; ++i) {
        const rt_ray& r = rays[i];
        if (ray_skip(s, r.skip) != r.skip) return RT_ERR_INVALID_ARG;
        out_occluded[i] =
            w.occluded(s, r.skip, Vec3{r.ox, r.oy, r.oz}, Vec3{r.dx, r.dy, r.dz}) ? 1 : 0;
    }
    return RT_OK;
}

// cast_rays on the rays of a band of a camera's frame, row-major, without the rays.
template <typename W>
int cast_camera(const rt_camera& camera, const rt_scene& s, int32_t width, int32_t row_begin,
                int32_t row_end, rt_hit* out_hits, int32_t* out_triangle, const W& w) {
    int64_t i = 0;
    for (int32_t y = row_begin; y < row_end; ++y)
        for (int32_t x = 0; x < width; ++x, ++i) {
            const Ray r = camera_ray(camera, static_cast<float>(x), static_cast<float>(y));
            const Bounce b = w.bounce(s, -1, r.o, r.d);
            out_hits[i] = rt_hit{b.best, b.obj2};
            if (out_triangle) out_triangle[i] = b.tri2;
        }
    return RT_OK;
}

// Per ray the number of records j in 0 .. count-1 with keep(o, d, j, skip):
// o, d the doubles of the ray's floats.
template <typename Keep>
int count_kept(const rt_ray* rays, int64_t n, const rt_scene& s, int32_t count,
               int32_t* out_count, Keep keep) {
    for (int64_t i = 0; i < n; ++i) {
        const rt_ray& r = rays[i];
        if (ray_skip(s, r.skip) != r.skip) return RT_ERR_INVALID_ARG;
        const double o[3] = {r.ox, r.oy, r.oz}, d[3] = {r.dx, r.dy, r.dz};
        int32_t kept = 0;
        for (int32_t j = 0; j < count; ++j)
            if (keep(o, d, j, r.skip)) ++kept;
        out_count[i] = kept;
    }
    return RT_OK;
}

}  // namespace rt_light

#endif /* RT_RAYS_RUN_H */
