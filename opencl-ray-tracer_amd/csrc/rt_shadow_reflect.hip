// rt_shadow_reflect.hip -- rt_shadow_hits_reflected_device /
// rt_light_hits_shadowed_reflected_device: the deferred light pass with all of
// its terms, on the device: shadowed direct light at the hit
// point p, the mirror bounce, shadowed direct light at the point p2 the bounce
// meets, blended.
//
// One kernel template over the output (mask at p2, int32x4, RGBA8): the pixel
// prologue, the surface step, three phases, one 4- or 16-byte store.  No
// workspace, one launch.
//
// Every phase sits behind a wave-uniform guard; a wave that has nothing to do
// in a phase never enters it:
//   1. the shadow walk at p (lit instances with lights);
//   2. the bounce walk (the mask instance, or reflectivity != 0);
//   3. the shadow walk at p2 (lights, and a lane of the wave whose bounce met
//      something): n2 and p2 are gathered by obj2 / tri2 first, then the walk
//      of phase 1 runs with own object obj2 over the lanes whose bounce met
//      something.
// Between phases 2 and 3, and in the shade, a lane reads the bounce's triangle
// or centre and its colour by obj2 / tri2: values the bounce walk took from
// its own loop counters, in range by construction.
//
// rt_init does not load this translation unit's code object: the runtime
// loads it at the first launch of one of its kernels.
#include "rt_light_device.inc"

namespace {

enum { kOutMask2 = 2 };

// `s` holds device pointers.  `refl`: the lit forms' reflectivity.
template <int kOut>
__global__ void __launch_bounds__(256)
shadow_reflect_kernel(const rt_hit* __restrict__ hits, void* __restrict__ out, int64_t n,
                      int32_t width, int32_t row_begin, float dx, float dy, float dz, float refl,
                      rt_scene s) {
    using rt_light::Vec3;
    const int64_t i = pixel_index();
    if (i >= n) return;
    const Vec3 d{dx, dy, dz};
    float ox, oy;
    int32_t obj;
    const float t = load_pixel(hits, i, n, width, row_begin, s, ox, oy, obj);
    const bool hit = obj >= 0;
    constexpr bool kMask = kOut == kOutMask2;
    // the lanes that take part: the lit forms leave t == kFar to shade_lit,
    // which writes black whatever the factor
    const bool casts = kMask ? hit : hit && !(t == rt_light::kFar);
    const bool lights = s.num_lights > 0;             // (uniform)
    const bool mirrors = kMask || refl != 0.0f;       // (uniform) a kernel argument
    const bool work = kMask ? lights : (mirrors || lights);  // (uniform) the mask is 0 without lights

    float k = 1.0f, k2 = 1.0f;
    uint32_t mask = 0, unused = 0;
    rt_light::Bounce b{rt_light::kFar, -1, -1};
    if (work && __ballot(casts) != 0) {  // (uniform)
        Vec3 p{0.0f, 0.0f, 0.0f}, nrm{0.0f, 0.0f, 0.0f};
        if (casts) {
            p = rt_light::hit_point(ox, oy, d, t);
            nrm = surface_step(s, obj, ox, oy, d, t, p);
        }
        // phase 1: the shadowed factor at p
        if (!kMask && lights) k = light_walk<false>(s, p, nrm, obj, casts, unused);  // (uniform)
        if (mirrors) {  // (uniform)
            // phase 2: the bounce walk.  wave_bounce_walk()'s text, kept here:
            // calling it, in any of three wordings, made the mask instance
            // 0.3-0.5 % slower with three lights (profiles/light_shared/)
            const Vec3 R = rt_light::mirror_dir(nrm, d);
            const double pd[3] = {p.x, p.y, p.z};
            const double Rd[3] = {R.x, R.y, R.z};
            float sf;
            for (int32_t j = 0; j < s.num_cubes; ++j) {
                // the lane's own cube is skipped whole; a cube no lane has to
                // test is skipped by the wave
                const bool mine = casts && obj != j;
                if (__ballot(mine) == 0) continue;
                const float* v = s.cube_vertices + 144 * (int64_t)j;
                for (int tri = 0; tri < 12; ++tri)
                    if (mine && rt_light::bounce_tri(pd, Rd, v + 12 * tri, &sf) && sf < b.best)
                        b = rt_light::Bounce{sf, j, tri};
            }
            // (sphere sp is object num_cubes + sp; obj < 2^31 so the sum fits)
            for (int32_t sp = 0; sp < s.num_spheres; ++sp)
                if (casts && obj - s.num_cubes != sp &&
                    rt_light::bounce_sphere(p, R, s.sphere_origins + 4 * (int64_t)sp,
                                            s.sphere_radius[sp], &sf) &&
                    sf < b.best)
                    b = rt_light::Bounce{sf, s.num_cubes + sp, -1};
            // phase 3: the shadowed factor (the mask) at p2
            const bool met = b.obj2 >= 0;
            if (lights && __ballot(met) != 0) {  // (uniform)
                Vec3 p2{0.0f, 0.0f, 0.0f}, n2{0.0f, 0.0f, 0.0f};
                if (met) {
                    p2 = rt_light::bounce_point(p, R, b.best);
                    n2 = rt_light::bounce_normal(s, b.obj2, b.tri2, p2, R);
                }
                k2 = light_walk<kMask>(s, p2, n2, b.obj2, met, mask);
            }
        }
    }
    if constexpr (kMask) {
        reinterpret_cast<uint32_t*>(out)[i] = mask;
    } else {
        int32_t lit[4];
        if (mirrors && casts)
            rt_light::shade_mirrored_factors(s, obj, t, k, b, k2, refl, lit);
        else
            rt_light::shade_lit(t, k, rt_light::slot_colour(s, obj), lit);
        store_lit<kOut>(out, i, lit);
    }
}

}  // namespace

extern "C" {

int rt_shadow_hits_reflected_device(rt_ctx* ctx, const rt_hit* device_hits,
                                    const rt_scene* device_scene, const float ray_dir[4],
                                    int32_t width, int32_t row_begin, int32_t row_end,
                                    uint32_t* device_out, void* stream) {
    return launch(KeepAll{}, 0, shadow_reflect_kernel<kOutMask2>, 4, true, ctx, device_hits,
                  device_scene, ray_dir, width, row_begin, row_end, device_out, stream, 0.0f);
}

int rt_light_hits_shadowed_reflected_device(rt_ctx* ctx, const rt_hit* device_hits,
                                            const rt_scene* device_scene, const float ray_dir[4],
                                            int32_t width, int32_t row_begin, int32_t row_end,
                                            float reflectivity, int32_t out_format,
                                            void* device_out, void* stream) {
    return launch_lit(KeepAll{}, 0, shadow_reflect_kernel<kOutI32x4>,
                      shadow_reflect_kernel<kOutRgba8>, out_format, ctx, device_hits,
                      device_scene, ray_dir, width, row_begin, row_end, device_out, stream,
                      reflectivity);
}

}  // extern "C"
