// rt_accel_walks.inc -- the wave's walks of rt_light_device.inc with the keep
// test of include/rt_accel_impl.h in front of a cube's twelve triangle tests
// (DESIGN.md §3.1g, §3.1h): what the culled ray queries (rt_accel.hip) and the
// culled light pass (rt_light_accel.hip, rt_shadow_accel.hip) share.  Included
// once by each, behind rt_light_device.inc and rt_accel_impl.h; not a
// standalone translation unit.
//
// The walks stay wave-uniform: cube, triangle and sphere are loop counters, so
// the scene and the record (320 bytes per cube) come through scalar loads, once
// per wave.  A lane that does not keep a cube does not test it: the ballot
// skips the cube where no lane of the wave keeps it.  Spheres keep their
// unculled loop.

namespace {

// wave_bounce_walk of rt_light_device.inc with the keep test: a lane tests
// cube j iff it casts, j is not its own and its ray keeps the cube.
__device__ __forceinline__ rt_light::Bounce wave_bounce_walk_culled(
    const rt_scene& s, const rt_cube_bound* __restrict__ accel, rt_light::Vec3 p,
    rt_light::Vec3 R, int32_t own, bool casts) {
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
    // (sphere sp is object num_cubes + sp; own < 2^31 so the sum fits)
    for (int32_t sp = 0; sp < s.num_spheres; ++sp)
        if (casts && own - s.num_cubes != sp &&
            rt_light::bounce_sphere(p, R, s.sphere_origins + 4 * (int64_t)sp, s.sphere_radius[sp],
                                    &sf) &&
            sf < b.best)
            b = rt_light::Bounce{sf, s.num_cubes + sp, -1};
    return b;
}

// occluder_walk of rt_light_device.inc with the keep test; its early-outs stay.
__device__ __forceinline__ bool occluder_walk_culled(const rt_scene& s,
                                                     const rt_cube_bound* __restrict__ accel,
                                                     const double* pd, rt_light::Vec3 p,
                                                     rt_light::Vec3 L, int32_t own, bool pending) {
    if (__ballot(pending) == 0) return pending;
    const double Ld[3] = {L.x, L.y, L.z};
    for (int32_t j = 0; j < s.num_cubes; ++j) {
        const bool mine = pending && own != j && rt_light::cube_kept(pd, Ld, accel[j], true);
        if (__ballot(mine) == 0) continue;
        const float* v = s.cube_vertices + 144 * (int64_t)j;
        for (int tri = 0; tri < 12; ++tri) {
            if (mine && pending && rt_light::occluded_by_tri(pd, Ld, v + 12 * tri))
                pending = false;
            if (__ballot(mine && pending) == 0) break;
        }
        if (__ballot(pending) == 0) break;
    }
    if (__ballot(pending) != 0) {
        for (int32_t sp = 0; sp < s.num_spheres; ++sp) {
            if (pending && own - s.num_cubes != sp &&
                rt_light::occluded_by_sphere(p, L, s.sphere_origins + 4 * (int64_t)sp,
                                             s.sphere_radius[sp]))
                pending = false;
            if (__ballot(pending) == 0) break;
        }
    }
    return pending;
}

// light_walk of rt_light_device.inc over occluder_walk_culled.
template <bool kMask>
__device__ __forceinline__ float light_walk_culled(const rt_scene& s,
                                                   const rt_cube_bound* __restrict__ accel,
                                                   rt_light::Vec3 p, rt_light::Vec3 nrm,
                                                   int32_t own, bool active, uint32_t& mask) {
    using rt_light::Vec3;
    float k = 0.0f;
    const double pd[3] = {p.x, p.y, p.z};
    for (int32_t li = 0; li < s.num_lights; ++li) {
        const float* l = s.lights + 4 * (int64_t)li;
        const Vec3 L{l[0] - p.x, l[1] - p.y, l[2] - p.z};
        const float ll = sqrtf((L.x * L.x + L.y * L.y) + L.z * L.z);
        const float c = ((nrm.x * L.x + nrm.y * L.y) + nrm.z * L.z) / ll;
        const bool faces = active && c > 0.0f;
        const bool pending = occluder_walk_culled(s, accel, pd, p, L, own, faces);
        if (faces) {
            if (pending)
                k = k + c;  // not occluded
            else if (kMask)
                mask |= 1u << (li & 31);  // (li < 32: the launch refuses more lights)
        }
    }
    if (k > 1.0f) k = 1.0f;
    return active ? k : 1.0f;
}

}  // namespace
