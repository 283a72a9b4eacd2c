// rt_sphere_groups.hip -- rt_sphere_groups_build_device and
// rt_cast_rays_grouped_device / rt_occlude_rays_grouped_device /
// rt_cast_camera_grouped_device: the ray queries culled by cube records AND by
// grouped sphere bounds on the device.  The kernels of
// rt_accel.hip with the sphere loop replaced by a loop over the groups' records:
// the keep test of include/rt_sphere_groups_impl.h in front of a group's
// members, the text the host functions compile.
//
// The walks stay wave-uniform: group and member are loop counters, so the
// record (64 bytes), the member index, the centre and the radius come through
// scalar loads, once per wave.  A lane that does not keep a group does not
// test it; the ballot skips a group where no lane of the wave keeps it.
//
// The walks are rt_light_device.inc's over WaveGroupCull below: CubeCull of
// rt_accel_impl.h in the cube phase, and the loop over the groups in place
// of the walks' own sphere loop.  The ray prologues, cast_kernel,
// occlude_kernel, the launch and the builds' reduce are rt_rays_device.inc's;
// here the kernels take the cube records, the group records and their count as
// cull arguments.  Not preloaded by rt_init (§3.1g Device).
#include "rt_light_device.inc"
#include "rt_accel_impl.h"
#include "rt_sphere_groups_impl.h"

namespace {

// CubeCull's cube phase, and the sphere phase over the groups: a lane tests the
// members of group g iff it takes part and its ray keeps the group.
struct WaveGroupCull : rt_light::CubeCull {
    static constexpr bool kGroups = true;
    const rt_sphere_group* __restrict__ groups;
    int32_t num_groups;
    // occluder_walk's sphere phase, entered with a pending lane in the wave;
    // its early-outs stay.
    __device__ __forceinline__ bool occluder_spheres(const rt_scene& s, const double* pd,
                                                     const double* Ld, rt_light::Vec3 p,
                                                     rt_light::Vec3 L, int32_t own,
                                                     bool pending) const {
        const int32_t own_sp = own - s.num_cubes;
        for (int32_t g = 0; g < num_groups; ++g) {
            const rt_sphere_group& G = groups[g];
            const bool mine = pending && rt_light::group_kept(pd, Ld, G, true);
            if (__ballot(mine) == 0) continue;
            const int32_t count = G.count;
            for (int k = 0; k < rt_light::kGroupMax && k < count; ++k) {
                const int32_t sp = G.member[k];
                if ((uint32_t)sp >= (uint32_t)s.num_spheres) continue;  // (uniform)
                if (mine && pending && own_sp != sp &&
                    rt_light::occluded_by_sphere(p, L, s.sphere_origins + 4 * (int64_t)sp,
                                                 s.sphere_radius[sp]))
                    pending = false;
                if (__ballot(mine && pending) == 0) break;
            }
            if (__ballot(pending) == 0) break;
        }
        return pending;
    }
};
__device__ __forceinline__ WaveGroupCull cull_of(const rt_cube_bound* accel,
                                             const rt_sphere_group* groups, int32_t num_groups) {
    return WaveGroupCull{{accel}, groups, num_groups};
}

// wave_bounce_walk for WaveGroupCull: the shared walk's cube phase, then the groups.
// Its own text, not a sphere phase of the policy as occluder_spheres is: that
// wording missed the timing rule in cast_kernel (profiles/rays_shared/README.md).
__device__ __forceinline__ rt_light::Bounce wave_bounce_walk(const rt_scene& s, rt_light::Vec3 p,
                                                             rt_light::Vec3 R, int32_t own,
                                                             bool casts, WaveGroupCull cull) {
    const rt_cube_bound* __restrict__ accel = cull.accel;
    const rt_sphere_group* __restrict__ groups = cull.groups;
    const int32_t num_groups = cull.num_groups;
    rt_light::Bounce b{rt_light::kFar, -1, -1};
    const double pd[3] = {p.x, p.y, p.z};
    const double Rd[3] = {R.x, R.y, R.z};
    float sf;
    for (int32_t j = 0; j < s.num_cubes; ++j) {
        const bool mine = casts && own != j && rt_light::cube_kept(pd, Rd, accel[j], false);
        if (__ballot(mine) == 0) continue;
        const float* v = s.cube_vertices + 144 * (int64_t)j;
        for (int tri = 0; tri < 12; ++tri)
            if (mine && rt_light::bounce_tri(pd, Rd, v + 12 * tri, &sf) && sf < b.best)
                b = rt_light::Bounce{sf, j, tri};
    }
    // (sphere sp is object num_cubes + sp; own < 2^31 so the difference fits)
    const int32_t own_sp = own - s.num_cubes;
    for (int32_t g = 0; g < num_groups; ++g) {
        const rt_sphere_group& G = groups[g];
        const bool mine = casts && rt_light::group_kept(pd, Rd, G, false);
        if (__ballot(mine) == 0) continue;
        const int32_t count = G.count;
        for (int k = 0; k < rt_light::kGroupMax && k < count; ++k) {
            const int32_t sp = G.member[k];
            // (uniform) a foreign record's index is no sphere: nothing is read through it
            if ((uint32_t)sp >= (uint32_t)s.num_spheres) continue;
            if (mine && own_sp != sp &&
                rt_light::bounce_sphere(p, R, s.sphere_origins + 4 * (int64_t)sp,
                                        s.sphere_radius[sp], &sf) &&
                rt_light::sphere_takes(b, sf, s.num_cubes + sp, s.num_cubes))
                b = rt_light::Bounce{sf, s.num_cubes + sp, -1};
        }
    }
    return b;
}

}  // namespace

#include "rt_rays_device.inc"

namespace {

// ---- the build: the workspace is a GroupFrame (16 bytes), then num_spheres
// keys, then num_spheres sphere indices in sorted order ------------------------

__device__ __forceinline__ uint32_t* ws_keys(void* ws) {
    return reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + 16);
}
__device__ __forceinline__ int32_t* ws_order(void* ws, int32_t n) {
    return reinterpret_cast<int32_t*>(ws_keys(ws) + n);
}

// Part 1, one workgroup: the minima and maxima of the finite spheres' centres
// (neither depends on the order) and from them rt_light::group_frame.
__global__ void __launch_bounds__(256)
groups_frame_kernel(const float* __restrict__ sphere_origins,
                    const float* __restrict__ sphere_radius, int32_t n, void* __restrict__ ws) {
    __shared__ float part[4][7];
    const float inf = __builtin_huge_valf();
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf}, any = 0.0f;
    for (int32_t i = (int32_t)threadIdx.x; i < n; i += 256) {
        const float4 c = reinterpret_cast<const float4*>(sphere_origins)[i];
        const float ctr[3] = {c.x, c.y, c.z};
        if (!rt_light::sphere_finite(ctr, sphere_radius[i])) continue;
        any = 1.0f;
        for (int a = 0; a < 3; ++a) {
            if (ctr[a] < mn[a]) mn[a] = ctr[a];
            if (ctr[a] > mx[a]) mx[a] = ctr[a];
        }
    }
    const MinOf fmin_{};
    const MaxOf fmax_{};
    for (int a = 0; a < 3; ++a) {
        mn[a] = lanes_reduce(mn[a], 32, fmin_);
        mx[a] = lanes_reduce(mx[a], 32, fmax_);
    }
    any = lanes_reduce(any, 32, fmax_);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) part[wave][a] = mn[a], part[wave][3 + a] = mx[a];
        part[wave][6] = any;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            for (int a = 0; a < 3; ++a) {
                mn[a] = fmin_(mn[a], part[w][a]);
                mx[a] = fmax_(mx[a], part[w][3 + a]);
            }
            any = fmax_(any, part[w][6]);
        }
        const rt_light::GroupFrame f = rt_light::group_frame(mn, mx, any != 0.0f);
        *reinterpret_cast<float4*>(ws) = make_float4(f.mn[0], f.mn[1], f.mn[2], f.ext);
    }
}

// Part 2a, one lane per sphere: its key.
__global__ void __launch_bounds__(256)
groups_key_kernel(const float* __restrict__ sphere_origins,
                  const float* __restrict__ sphere_radius, int32_t n, void* __restrict__ ws) {
    const int32_t i = (int32_t)blockIdx.x * 256 + (int32_t)threadIdx.x;  // (< 2^31: the grid)
    if (i >= n) return;
    const float4 fr = *reinterpret_cast<const float4*>(ws);
    const rt_light::GroupFrame f{{fr.x, fr.y, fr.z}, fr.w};
    const float4 c = reinterpret_cast<const float4*>(sphere_origins)[i];
    const float ctr[3] = {c.x, c.y, c.z};
    ws_keys(ws)[i] = rt_light::sphere_key(ctr, sphere_radius[i], f);
}

// Part 2b, one lane per sphere: its rank in the order by (key, index), the
// number of pairs below its own, counted over all keys in a uniform loop
// (scalar loads; n * n compares in all), and its index into that position.
__global__ void __launch_bounds__(256)
groups_rank_kernel(int32_t n, void* __restrict__ ws) {
    const int32_t i = (int32_t)blockIdx.x * 256 + (int32_t)threadIdx.x;
    const uint32_t* __restrict__ keys = ws_keys(ws);
    const bool live = i < n;
    const uint32_t mine = live ? keys[i] : 0u;
    int32_t rank = 0;
    for (int32_t j = 0; j < n; ++j) {
        const uint32_t kj = keys[j];
        rank += (kj < mine || (kj == mine && j < i)) ? 1 : 0;
    }
    if (live) ws_order(ws, n)[rank] = i;  // (rank < n: the pairs are distinct)
}

// Part 3, eight lanes per record, 32 records per workgroup: lane l of a record
// holds position g * group_size + l of the order (idle from group_size or the
// end of the order on); rt_light::sphere_group across the eight lanes.  The
// first lane stores the 32-byte head as two 16-byte stores, every lane one
// member slot.
__global__ void __launch_bounds__(256)
groups_record_kernel(const float* __restrict__ sphere_origins,
                     const float* __restrict__ sphere_radius, int32_t n, int32_t group_size,
                     int32_t num_groups, const void* __restrict__ ws,
                     rt_sphere_group* __restrict__ out) {
    const int32_t l = (int32_t)threadIdx.x & 7;
    const int32_t g = (int32_t)blockIdx.x * 32 + (int32_t)(threadIdx.x >> 3);
    const bool record = g < num_groups;
    const int32_t pos = record ? g * group_size + l : 0;  // (< n + 8)
    const bool holds = record && l < group_size && pos < n;
    const int32_t* order =
        reinterpret_cast<const int32_t*>(static_cast<const char*>(ws) + 16) + n;
    const int32_t idx = holds ? order[pos] : INT32_MAX;
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf}, ar = 0.0f, bad = 0.0f;
    if (holds && (uint32_t)idx < (uint32_t)n) {
        const float4 c = reinterpret_cast<const float4*>(sphere_origins)[idx];
        const float ctr[3] = {c.x, c.y, c.z};
        const float r = sphere_radius[idx];
        if (rt_light::sphere_finite(ctr, r)) {
            ar = fabsf(r);
            for (int a = 0; a < 3; ++a) {
                lo[a] = rt_light::member_lo(ctr[a], r);
                hi[a] = rt_light::member_hi(ctr[a], r);
            }
        } else {
            bad = 1.0f;
        }
    }
    const MinOf fmin_{};
    const MaxOf fmax_{};
    for (int a = 0; a < 3; ++a) {
        lo[a] = lanes_reduce(lo[a], 4, fmin_);
        hi[a] = lanes_reduce(hi[a], 4, fmax_);
    }
    ar = lanes_reduce(ar, 4, fmax_);
    bad = lanes_reduce(bad, 4, fmax_);
    // the lane's slot: the number of the record's lanes in front of it by (index, lane)
    int32_t slot = 0, count = 0;
    for (int j = 0; j < 8; ++j) {
        const int32_t other = __shfl(idx, j, 8);
        slot += (other < idx || (other == idx && j < l)) ? 1 : 0;
        count += other != INT32_MAX ? 1 : 0;
    }
    if (!record) return;
    rt_sphere_group* o = out + g;
    if (l == 0) {
        float4 a, b;
        if (bad != 0.0f) {
            a = make_float4(-inf, -inf, -inf, inf);
            b = make_float4(inf, inf, inf, 0.0f);
        } else {
            // (+ 0.0f: a zero bound is +0 whichever of -0 and +0 the order met first)
            a = make_float4(lo[0] + 0.0f, lo[1] + 0.0f, lo[2] + 0.0f, ar);
            b = make_float4(hi[0] + 0.0f, hi[1] + 0.0f, hi[2] + 0.0f, 0.0f);
        }
        b.w = __int_as_float(count);
        reinterpret_cast<float4*>(o)[0] = a;
        reinterpret_cast<float4*>(o)[1] = b;
    }
    o->member[slot] = holds ? idx : -1;  // (slot < 8: eight distinct (index, lane) pairs)
}

}  // namespace

extern "C" {

int rt_sphere_groups_build_device(rt_ctx* ctx, const rt_scene* device_scene, int32_t group_size,
                                  rt_sphere_group* device_out, void* device_workspace,
                                  int64_t workspace_bytes, void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    const int rc = rt_light::check_sphere_groups_build(device_scene, group_size, device_out);
    if (rc) return rc;
    const int32_t n = device_scene->num_spheres;
    if (n == 0) return RT_OK;
    if (!device_workspace || reinterpret_cast<uintptr_t>(device_workspace) % 16 != 0 ||
        workspace_bytes < rt_light::sphere_groups_workspace_bytes(n))
        return RT_ERR_INVALID_ARG;
    const int32_t num_groups = rt_light::sphere_groups_count(n, group_size);
    const float* ctr = device_scene->sphere_origins;
    const float* rad = device_scene->sphere_radius;
    const int64_t per_sphere = ((int64_t)n + 255) / 256;
    return launch_rays(ctx, 1, 1, stream, [&](dim3, hipStream_t st) {
        groups_frame_kernel<<<dim3(1), dim3(256), 0, st>>>(ctr, rad, n, device_workspace);
        groups_key_kernel<<<dim3((unsigned)per_sphere), dim3(256), 0, st>>>(ctr, rad, n,
                                                                             device_workspace);
        groups_rank_kernel<<<dim3((unsigned)per_sphere), dim3(256), 0, st>>>(n, device_workspace);
        groups_record_kernel<<<dim3((unsigned)((num_groups + 31) / 32)), dim3(256), 0, st>>>(
            ctr, rad, n, group_size, num_groups, device_workspace, device_out);
    });
}

int rt_cast_rays_grouped_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                                const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                const rt_sphere_group* device_groups, int32_t num_groups,
                                rt_hit* device_out_hits, int32_t* device_out_triangle,
                                void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = rt_light::check_rays(device_rays, n, device_scene, device_out_hits, sizeof(rt_hit),
                                  device_out_triangle);
    if (!rc) rc = rt_light::check_accel(device_scene, device_accel);
    if (!rc) rc = rt_light::check_sphere_groups(device_scene, device_groups, num_groups);
    if (rc) return rc;
    return launch_rays(ctx, n, 256, stream, [&](dim3 grid, hipStream_t st) {
        cast_kernel<kFromRays, const rt_cube_bound*, const rt_sphere_group*, int32_t>
            <<<grid, dim3(256), 0, st>>>(
            device_rays, device_out_hits, device_out_triangle, device_accel, device_groups,
            num_groups, n, 1, 0, rt_camera{}, *device_scene);
    });
}

int rt_occlude_rays_grouped_device(rt_ctx* ctx, const rt_ray* device_rays, int64_t n,
                                   const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                   const rt_sphere_group* device_groups, int32_t num_groups,
                                   uint8_t* device_out_occluded, void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = rt_light::check_rays(device_rays, n, device_scene, device_out_occluded, 1, nullptr);
    if (!rc) rc = rt_light::check_accel(device_scene, device_accel);
    if (!rc) rc = rt_light::check_sphere_groups(device_scene, device_groups, num_groups);
    if (rc) return rc;
    return launch_rays(ctx, n, 256, stream, [&](dim3 grid, hipStream_t st) {
        occlude_kernel<const rt_cube_bound*, const rt_sphere_group*, int32_t>
            <<<grid, dim3(256), 0, st>>>(device_rays, device_out_occluded, device_accel,
                                         device_groups, num_groups, n, *device_scene);
    });
}

int rt_cast_camera_grouped_device(rt_ctx* ctx, const rt_camera* camera,
                                  const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                  const rt_sphere_group* device_groups, int32_t num_groups,
                                  int32_t width, int32_t row_begin, int32_t row_end,
                                  rt_hit* device_out_hits, int32_t* device_out_triangle,
                                  void* stream) {
    if (!ctx) return RT_ERR_INVALID_ARG;
    int rc = rt_light::check_camera(camera, device_scene, true, width, row_begin, row_end,
                                    device_out_hits, sizeof(rt_hit), device_out_triangle);
    if (!rc) rc = rt_light::check_accel(device_scene, device_accel);
    if (!rc) rc = rt_light::check_sphere_groups(device_scene, device_groups, num_groups);
    if (rc) return rc;
    const int64_t n = (int64_t)(row_end - row_begin) * width;
    return launch_rays(ctx, n, 256, stream, [&](dim3 grid, hipStream_t st) {
        cast_kernel<kFromCamera, const rt_cube_bound*, const rt_sphere_group*, int32_t>
            <<<grid, dim3(256), 0, st>>>(
            nullptr, device_out_hits, device_out_triangle, device_accel, device_groups,
            num_groups, n, width, row_begin, *camera, *device_scene);
    });
}

}  // extern "C"
