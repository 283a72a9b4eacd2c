// rt_sphere_groups.cpp -- the ray queries culled by grouped sphere bounds on
// the host: rt_sphere_groups_count, rt_sphere_groups_build,
// rt_sphere_groups_kept, rt_cast_rays_grouped, rt_occlude_rays_grouped and
// rt_cast_camera_grouped, and the argument checks they share with
// rt_sphere_groups.hip.  The loops of include/rt_rays_run.h over GroupedWalks of
// include/rt_sphere_groups_impl.h, the text the kernels compile too.  Plain C++, no HIP; built with
// -ffp-contract=off like rt_accel.cpp.
#include <algorithm>
#include <vector>

#include "rt_args.h"
#include "rt_hip.h"
#include "rt_rays_run.h"
#include "rt_sphere_groups_impl.h"

namespace rt_light {

int check_sphere_groups_build(const rt_scene* scene, int32_t group_size,
                              const rt_sphere_group* out) {
    if (!scene || group_size < 1 || group_size > kGroupMax) return RT_ERR_INVALID_ARG;
    // the scene alone, as check_rays() checks it
    if (rt_args::check_args(scene, 1, 1, 0, 1, RT_FORMAT_I32X4)) return RT_ERR_INVALID_ARG;
    if (scene->num_lights > 0 && !scene->lights) return RT_ERR_INVALID_ARG;
    if (scene->num_spheres > 0 && (!out || misaligned(out, 16))) return RT_ERR_INVALID_ARG;
    return RT_OK;
}

int check_sphere_groups(const rt_scene* scene, const rt_sphere_group* groups,
                        int32_t num_groups) {
    bool counted = false;
    for (int32_t g = 1; g <= kGroupMax; ++g)
        counted = counted || num_groups == sphere_groups_count(scene->num_spheres, g);
    if (!counted) return RT_ERR_INVALID_ARG;
    if (scene->num_spheres > 0 && (!groups || misaligned(groups, 16))) return RT_ERR_INVALID_ARG;
    return RT_OK;
}

}  // namespace rt_light

extern "C" {

using namespace rt_light;

int32_t rt_sphere_groups_count(int32_t num_spheres, int32_t group_size) {
    return sphere_groups_count(num_spheres, group_size);
}

int64_t rt_sphere_groups_workspace_bytes(int32_t num_spheres) {
    return sphere_groups_workspace_bytes(num_spheres);
}

int rt_sphere_groups_build(const rt_scene* scene, int32_t group_size, rt_sphere_group* out) {
    const int rc = check_sphere_groups_build(scene, group_size, out);
    if (rc) return rc;
    const int32_t n = scene->num_spheres;
    if (n == 0) return RT_OK;
    const float* ctr = scene->sphere_origins;
    const float* rad = scene->sphere_radius;
    float mn[3] = {0.0f, 0.0f, 0.0f}, mx[3] = {0.0f, 0.0f, 0.0f};
    bool any = false;
    for (int32_t i = 0; i < n; ++i) {
        const float* c = ctr + 4 * static_cast<int64_t>(i);
        if (!sphere_finite(c, rad[i])) continue;
        for (int a = 0; a < 3; ++a) {
            if (!any || c[a] < mn[a]) mn[a] = c[a];
            if (!any || c[a] > mx[a]) mx[a] = c[a];
        }
        any = true;
    }
    const GroupFrame frame = group_frame(mn, mx, any);
    std::vector<uint32_t> key(n);
    std::vector<int32_t> order(n);
    for (int32_t i = 0; i < n; ++i) {
        key[i] = sphere_key(ctr + 4 * static_cast<int64_t>(i), rad[i], frame);
        order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(),
                     [&](int32_t a, int32_t b) { return key[a] < key[b]; });
    const int32_t groups = sphere_groups_count(n, group_size);
    for (int32_t g = 0; g < groups; ++g) {
        const int32_t first = g * group_size;
        const int32_t count = n - first < group_size ? n - first : group_size;
        out[g] = sphere_group(ctr, rad, order.data() + first, count);
    }
    return RT_OK;
}

// Per ray the number of groups that the keep test keeps.
int rt_sphere_groups_kept(const rt_ray* rays, int64_t n, const rt_scene* scene,
                          const rt_sphere_group* groups, int32_t num_groups, int32_t segment,
                          int32_t* out_count) {
    if (segment != 0 && segment != 1) return RT_ERR_INVALID_ARG;
    int rc = check_rays(rays, n, scene, out_count, 4, nullptr);
    if (!rc) rc = check_sphere_groups(scene, groups, num_groups);
    if (rc) return rc;
    return count_kept(rays, n, *scene, num_groups, out_count,
                      [=](const double* o, const double* d, int32_t g, int32_t) {
                          return group_kept(o, d, groups[g], segment != 0);
                      });
}

int rt_cast_rays_grouped(const rt_ray* rays, int64_t n, const rt_scene* scene,
                         const rt_cube_bound* accel, const rt_sphere_group* groups,
                         int32_t num_groups, rt_hit* out_hits, int32_t* out_triangle) {
    int rc = check_rays(rays, n, scene, out_hits, sizeof(rt_hit), out_triangle);
    if (!rc) rc = check_accel(scene, accel);
    if (!rc) rc = check_sphere_groups(scene, groups, num_groups);
    return rc ? rc
              : cast_rays(rays, n, *scene, out_hits, out_triangle,
                          GroupedWalks{accel, groups, num_groups});
}

int rt_occlude_rays_grouped(const rt_ray* rays, int64_t n, const rt_scene* scene,
                            const rt_cube_bound* accel, const rt_sphere_group* groups,
                            int32_t num_groups, uint8_t* out_occluded) {
    int rc = check_rays(rays, n, scene, out_occluded, 1, nullptr);
    if (!rc) rc = check_accel(scene, accel);
    if (!rc) rc = check_sphere_groups(scene, groups, num_groups);
    return rc ? rc
              : occlude_rays(rays, n, *scene, out_occluded,
                             GroupedWalks{accel, groups, num_groups});
}

int rt_cast_camera_grouped(const rt_camera* camera, const rt_scene* scene,
                           const rt_cube_bound* accel, const rt_sphere_group* groups,
                           int32_t num_groups, int32_t width, int32_t row_begin, int32_t row_end,
                           rt_hit* out_hits, int32_t* out_triangle) {
    int rc = check_camera(camera, scene, true, width, row_begin, row_end, out_hits, sizeof(rt_hit),
                          out_triangle);
    if (!rc) rc = check_accel(scene, accel);
    if (!rc) rc = check_sphere_groups(scene, groups, num_groups);
    return rc ? rc
              : cast_camera(*camera, *scene, width, row_begin, row_end, out_hits, out_triangle,
                            GroupedWalks{accel, groups, num_groups});
}

}  // extern "C"
