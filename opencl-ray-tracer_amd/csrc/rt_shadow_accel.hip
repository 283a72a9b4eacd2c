// rt_shadow_accel.hip -- rt_shadow_hits_accel_device: the shadow mask of the
// deferred light pass over the prebuilt cube records, on the device
// (DESIGN.md §3.1h).  shadow_kernel's mask form (rt_shadow.hip; each keeps its
// text, profiles/chain_shared/README.md) with light_walk culled by CubeCull of rt_accel_impl.h: a lane tests
// a cube for a light only where the cube is not its own and the keep test of
// include/rt_accel_impl.h keeps it for the lane's segment to that light.  The
// mask is rt_shadow_hits_device's word for word.
//
// A kernel of its own, in a translation unit of its own, by the resource
// report and the clock: here the keep test's loop over the record's normals is
// unrolled (the compiler's choice, as in rt_accel.hip), which the lit kernels
// of rt_light_accel.hip cannot afford without spilling scalar registers, and
// which is 8 % faster for this kernel (profiles/light_accel/).  `out` is the
// last kernel argument: read once at the end, it would otherwise sit in a
// preloaded scalar register pair through the walk.
//
// rt_init does not load this translation unit's code object: the runtime
// loads it at the first launch of its kernel.
#include "rt_light_device.inc"
#include "rt_accel_impl.h"

namespace {

using rt_light::CubeCull;

// `s` holds device pointers, `accel` its s.num_cubes records.
__global__ void __launch_bounds__(256)
shadow_accel_kernel(const rt_hit* __restrict__ hits, const rt_cube_bound* __restrict__ accel,
                    int64_t n, int32_t width, int32_t row_begin, float dx, float dy, float dz,
                    rt_scene s, void* __restrict__ out) {
    using rt_light::Vec3;
    const int64_t i = pixel_index();
    if (i >= n) return;
    const Vec3 d{dx, dy, dz};
    float ox, oy;
    int32_t obj;
    const float t = load_pixel(hits, i, n, width, row_begin, s, ox, oy, obj);
    const bool hit = obj >= 0;

    uint32_t mask = 0;
    if (s.num_lights > 0 && __ballot(hit) != 0) {  // (uniform) else: no walk at all
        Vec3 p{0.0f, 0.0f, 0.0f}, nrm{0.0f, 0.0f, 0.0f};
        if (hit) {
            p = rt_light::hit_point(ox, oy, d, t);
            nrm = surface_step(s, obj, ox, oy, d, t, p);
        }
        light_walk<true>(s, p, nrm, obj, hit, mask, CubeCull{accel});
    }
    reinterpret_cast<uint32_t*>(out)[i] = mask;
}

}  // namespace

extern "C" {

int rt_shadow_hits_accel_device(rt_ctx* ctx, const rt_hit* device_hits,
                                const rt_scene* device_scene, const rt_cube_bound* device_accel,
                                const float ray_dir[4], int32_t width, int32_t row_begin,
                                int32_t row_end, uint32_t* device_out, void* stream) {
    return launch(CubeCull{device_accel}, 0, shadow_accel_kernel, 4, true, ctx, device_hits,
                  device_scene, ray_dir, width, row_begin, row_end, device_out, stream);
}

}  // extern "C"
