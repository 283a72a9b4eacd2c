// rt_light.hip -- rt_hit_surfaces_device / rt_light_hits_device: surface
// normals, triangle ids and diffuse lighting from an RT_FORMAT_HIT frame, on
// the device.
//
// One kernel template over the output (rt_surface, int32x4, RGBA8): the pixel
// prologue, a surface step of its own, one 16-byte or 4-byte store.  A cube
// pixel runs up to twelve fp64 triangle tests to find which triangle gave its
// t (what bounds the kernel: it is compute-bound on them); a
// sphere pixel needs one normalisation.  The lights are indexed by the loop
// counter alone, so every lane reads the same address (scalar loads).
#include "rt_light_device.inc"

namespace {

enum { kOutSurface = 2 };

// `s` holds device pointers.
template <int kOut>
__global__ void __launch_bounds__(256)
light_kernel(const rt_hit* __restrict__ hits, void* __restrict__ out, int64_t n, int32_t width,
             int32_t row_begin, float dx, float dy, float dz, rt_scene s) {
    const int64_t i = pixel_index();
    if (i >= n) return;
    const rt_light::Vec3 d{dx, dy, dz};
    float ox, oy;
    int32_t obj;
    const float t = load_pixel(hits, i, n, width, row_begin, s, ox, oy, obj);
    const auto pixel = [&](const float* verts) {
        if constexpr (kOut == kOutSurface) {
            const rt_surface v = rt_light::surface(s, obj, verts, ox, oy, d, t,
                                                   rt_light::hit_point(ox, oy, d, t));
            reinterpret_cast<float4*>(out)[i] =
                make_float4(v.nx, v.ny, v.nz, __uint_as_float((uint32_t)v.triangle));
        } else {
            int32_t p[4];
            rt_light::lit_pixel(s, obj, verts, ox, oy, d, t, p);
            store_lit<kOut>(out, i, p);
        }
    };
    const float* verts = rt_light::cube_verts(s, obj);
    // surface_step's wave-uniform pointer, in a form of its own: the whole
    // pixel twice, once per pointer, and not one pixel behind a chosen
    // pointer.  11-17 % off the kernel at config 3 (profiles/light/).  Any
    // wave whose cube lanes hold more than one cube takes the per-lane
    // pointer; the arithmetic is the same.
    int c0 = 0;
    bool one = false;
    if (verts && (kOut == kOutSurface || s.num_lights > 0)) {  // the cube lanes that test triangles
        c0 = __builtin_amdgcn_readfirstlane(obj);
        one = __ballot(obj != c0) == 0;
    }
    if (one)
        pixel(s.cube_vertices + 144 * (int64_t)c0);
    else
        pixel(verts);
}

}  // namespace

namespace rt_internal {
int preload_light_kernels() {
    return preload({reinterpret_cast<const void*>(light_kernel<kOutI32x4>),
                    reinterpret_cast<const void*>(light_kernel<kOutRgba8>),
                    reinterpret_cast<const void*>(light_kernel<kOutSurface>)});
}
}  // namespace rt_internal

extern "C" {

int rt_hit_surfaces_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                           const float ray_dir[4], int32_t width, int32_t row_begin,
                           int32_t row_end, rt_surface* device_out, void* stream) {
    return launch(KeepAll{}, 0, light_kernel<kOutSurface>, 16, false, ctx, device_hits,
                  device_scene, ray_dir, width, row_begin, row_end, device_out, stream);
}

int rt_light_hits_device(rt_ctx* ctx, const rt_hit* device_hits, const rt_scene* device_scene,
                         const float ray_dir[4], int32_t width, int32_t row_begin,
                         int32_t row_end, int32_t out_format, void* device_out, void* stream) {
    return launch_lit(KeepAll{}, 0, light_kernel<kOutI32x4>, light_kernel<kOutRgba8>, out_format,
                      ctx, device_hits, device_scene, ray_dir, width, row_begin, row_end,
                      device_out, stream);
}

}  // extern "C"
