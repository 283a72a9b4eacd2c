// rt_accel.cpp -- the culled ray queries on the host:
// rt_accel_build, rt_accel_kept, rt_cast_rays_accel, rt_occlude_rays_accel and
// rt_cast_camera_accel, and the argument checks they share with rt_accel.hip.
// Plain loops over include/rt_accel_impl.h, the text the kernels compile too.
// Plain C++, no HIP; built with -ffp-contract=off like rt_light.cpp.
#include "rt_accel_impl.h"
#include "rt_args.h"
#include "rt_hip.h"

namespace rt_light {

namespace {
bool misaligned(const void* p, uintptr_t align) {
    return reinterpret_cast<uintptr_t>(p) % align != 0;
}
}  // namespace

int check_accel_build(const rt_scene* scene, const rt_cube_bound* out) {
    if (!scene) return RT_ERR_INVALID_ARG;
    // the scene alone, as check_rays() checks it
    if (rt_args::check_args(scene, 1, 1, 0, 1, RT_FORMAT_I32X4)) return RT_ERR_INVALID_ARG;
    if (scene->num_lights > 0 && !scene->lights) return RT_ERR_INVALID_ARG;
    return check_accel(scene, out);
}

int check_accel(const rt_scene* scene, const rt_cube_bound* accel) {
    if (scene->num_cubes > 0 && (!accel || misaligned(accel, 16))) return RT_ERR_INVALID_ARG;
    return RT_OK;
}

}  // namespace rt_light

extern "C" {

using namespace rt_light;

int rt_accel_build(const rt_scene* scene, rt_cube_bound* out) {
    const int rc = check_accel_build(scene, out);
    if (rc) return rc;
    for (int32_t j = 0; j < scene->num_cubes; ++j)
        out[j] = cube_bound(scene->cube_vertices + 144 * static_cast<int64_t>(j));
    return RT_OK;
}

// Per ray the number of cubes other than `skip` that the keep test keeps.
int rt_accel_kept(const rt_ray* rays, int64_t n, const rt_scene* scene,
                  const rt_cube_bound* accel, int32_t segment, int32_t* out_count) {
    if (segment != 0 && segment != 1) return RT_ERR_INVALID_ARG;
    int rc = check_rays(rays, n, scene, out_count, 4, nullptr);
    if (!rc) rc = check_accel(scene, accel);
    if (rc) return rc;
    const rt_scene& s = *scene;
    for (int64_t i = 0; i < n; ++i) {
        const rt_ray& r = rays[i];
        if (ray_skip(s, r.skip) != r.skip) return RT_ERR_INVALID_ARG;
        const double o[3] = {r.ox, r.oy, r.oz}, d[3] = {r.dx, r.dy, r.dz};
        int32_t kept = 0;
        for (int32_t j = 0; j < s.num_cubes; ++j)
            if (j != r.skip && cube_kept(o, d, accel[j], segment != 0)) ++kept;
        out_count[i] = kept;
    }
    return RT_OK;
}

int rt_cast_rays_accel(const rt_ray* rays, int64_t n, const rt_scene* scene,
                       const rt_cube_bound* accel, rt_hit* out_hits, int32_t* out_triangle) {
    int rc = check_rays(rays, n, scene, out_hits, sizeof(rt_hit), out_triangle);
    if (!rc) rc = check_accel(scene, accel);
    if (rc) return rc;
    const rt_scene& s = *scene;
    for (int64_t i = 0; i < n; ++i) {
        const rt_ray& r = rays[i];
        if (ray_skip(s, r.skip) != r.skip) return RT_ERR_INVALID_ARG;
        const Bounce b = bounce_walk_culled(s, accel, r.skip, Vec3{r.ox, r.oy, r.oz},
                                            Vec3{r.dx, r.dy, r.dz});
        out_hits[i] = rt_hit{b.best, b.obj2};
        if (out_triangle) out_triangle[i] = b.tri2;
    }
    return RT_OK;
}

int rt_occlude_rays_accel(const rt_ray* rays, int64_t n, const rt_scene* scene,
                          const rt_cube_bound* accel, uint8_t* out_occluded) {
    int rc = check_rays(rays, n, scene, out_occluded, 1, nullptr);
    if (!rc) rc = check_accel(scene, accel);
    if (rc) return rc;
    const rt_scene& s = *scene;
    for (int64_t i = 0; i < n; ++i) {
        const rt_ray& r = rays[i];
        if (ray_skip(s, r.skip) != r.skip) return RT_ERR_INVALID_ARG;
        out_occluded[i] = light_occluded_culled(s, accel, r.skip, Vec3{r.ox, r.oy, r.oz},
                                                Vec3{r.dx, r.dy, r.dz})
                              ? 1
                              : 0;
    }
    return RT_OK;
}

int rt_cast_camera_accel(const rt_camera* camera, const rt_scene* scene,
                         const rt_cube_bound* accel, int32_t width, int32_t row_begin,
                         int32_t row_end, rt_hit* out_hits, int32_t* out_triangle) {
    int rc = check_camera(camera, scene, true, width, row_begin, row_end, out_hits, sizeof(rt_hit),
                          out_triangle);
    if (!rc) rc = check_accel(scene, accel);
    if (rc) return rc;
    int64_t i = 0;
    for (int32_t y = row_begin; y < row_end; ++y)
        for (int32_t x = 0; x < width; ++x, ++i) {
            const Ray r = camera_ray(*camera, static_cast<float>(x), static_cast<float>(y));
            const Bounce b = bounce_walk_culled(*scene, accel, -1, r.o, r.d);
            out_hits[i] = rt_hit{b.best, b.obj2};
            if (out_triangle) out_triangle[i] = b.tri2;
        }
    return RT_OK;
}

}  // extern "C"
