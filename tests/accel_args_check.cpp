// accel_args_check.cpp -- rt_accel_build / rt_accel_kept / rt_cast_rays_accel /
// rt_occlude_rays_accel / rt_cast_camera_accel (csrc/rt_accel.cpp with
// csrc/rt_light.cpp and csrc/rt_args.cpp) as a stand-alone program on
// tests/light_check.h: tests/test_accel.py builds it with
// -fsanitize=address,undefined and runs it.  No GPU.
//
//   - exactly-sized heap arrays for the records, the rays and every output,
//     16-byte aligned as the contract asks, at n = 0, 1 and 257;
//   - the culled calls against the unculled ones, byte for byte, on the scene
//     of the shadow term's four kinds, and the kept counts of known rays;
//   - a scene of all NULLs with a NULL accel; a cube with a NaN vertex;
//   - a camera's band;
//   - the argument checks.
// Exit 0 and "accel args check ok" on success.
#include <new>

#include "light_check.h"

using namespace light_check;

namespace {

template <class T>
struct Exact {
    T* p;
    explicit Exact(size_t n)
        : p(static_cast<T*>(::operator new[](n * sizeof(T), std::align_val_t(16)))) {}
    ~Exact() { ::operator delete[](p, std::align_val_t(16)); }
    T& operator[](size_t i) { return p[i]; }
};

rt_ray ray(float ox, float oy, float oz, float dx, float dy, float dz, int32_t skip = -1) {
    return rt_ray{ox, oy, oz, skip, dx, dy, dz, 0.0f};
}

}  // namespace

int main() {
    static_assert(sizeof(rt_cube_bound) == 320, "the record");
    KindsScene kinds;
    const rt_scene& s = kinds.s;
    const rt_scene empty{};
    Exact<rt_cube_bound> accel(2);
    CHECK(rt_accel_build(&s, accel.p) == RT_OK);
    CHECK(accel[0].lo[0] == -6.0f && accel[0].hi[2] == -50.0f && accel[0].emax2 == 2 * 140.0f * 140.0f);
    CHECK(accel[1].lo[2] == -15.0f && accel[1].hi[1] == 70.0f && accel[1].reserved == 0.0f);
    CHECK(rt_accel_build(&empty, nullptr) == RT_OK);

    for (int n : {0, 1, 257}) {
        Exact<rt_ray> rays((size_t)n);
        Exact<rt_hit> hits((size_t)n), want((size_t)n);
        Exact<int32_t> tri((size_t)n), want_tri((size_t)n), kept((size_t)n);
        Exact<uint8_t> occ((size_t)n), want_occ((size_t)n);
        for (int i = 0; i < n; ++i) rays[i] = ray(0.5f * i, 20.0f, 0.0f, 0.0f, 0.0f, -1.0f);
        CHECK(rt_cast_rays(rays.p, n, &s, want.p, want_tri.p) == RT_OK);
        CHECK(rt_occlude_rays(rays.p, n, &s, want_occ.p) == RT_OK);
        CHECK(rt_cast_rays_accel(rays.p, n, &s, accel.p, hits.p, tri.p) == RT_OK);
        CHECK(rt_occlude_rays_accel(rays.p, n, &s, accel.p, occ.p) == RT_OK);
        CHECK(rt_accel_kept(rays.p, n, &s, accel.p, 0, kept.p) == RT_OK);
        CHECK(std::memcmp(hits.p, want.p, sizeof(rt_hit) * n) == 0);
        CHECK(std::memcmp(tri.p, want_tri.p, sizeof(int32_t) * n) == 0);
        CHECK(std::memcmp(occ.p, want_occ.p, (size_t)n) == 0);
        // x up to 128, y = 20: over the face, beside the box (y 58..70)
        for (int i = 0; i < n; ++i) CHECK(kept[i] == 1 && hits[i].object == 0);
        CHECK(rt_accel_kept(rays.p, n, &s, accel.p, 1, kept.p) == RT_OK);
        for (int i = 0; i < n; ++i) CHECK(kept[i] == 0);  // the segment ends at z = -1
        CHECK(rt_cast_rays_accel(rays.p, n, &s, accel.p, hits.p, nullptr) == RT_OK);
        CHECK(std::memcmp(hits.p, want.p, sizeof(rt_hit) * n) == 0);
        // a scene of all NULLs, a NULL accel
        CHECK(rt_cast_rays_accel(rays.p, n, &empty, nullptr, hits.p, tri.p) == RT_OK);
        CHECK(rt_occlude_rays_accel(rays.p, n, &empty, nullptr, occ.p) == RT_OK);
        CHECK(rt_accel_kept(rays.p, n, &empty, nullptr, 0, kept.p) == RT_OK);
        for (int i = 0; i < n; ++i)
            CHECK(is_miss(hits[i]) && tri[i] == -1 && occ[i] == 0 && kept[i] == 0);
    }
    {
        const int n = 4;
        Exact<rt_ray> rays(n);
        Exact<rt_hit> hits(n);
        Exact<int32_t> tri(n), kept(n);
        Exact<uint8_t> occ(n);
        rays[0] = ray(91.0f, 64.0f, 0.0f, 0.0f, 0.0f, -100.0f);     // the box, then the face
        rays[1] = ray(91.0f, 64.0f, 0.0f, 0.0f, 0.0f, -100.0f, 1);  // the box left out
        rays[2] = ray(91.0f, 64.0f, 0.0f, 0.0f, 0.0f, 1.0f);        // away from everything
        rays[3] = ray(NAN, 64.0f, 0.0f, 0.0f, 0.0f, -1.0f);         // the fallback: both kept
        CHECK(rt_cast_rays_accel(rays.p, n, &s, accel.p, hits.p, tri.p) == RT_OK);
        CHECK(rt_occlude_rays_accel(rays.p, n, &s, accel.p, occ.p) == RT_OK);
        CHECK(rt_accel_kept(rays.p, n, &s, accel.p, 0, kept.p) == RT_OK);
        CHECK(hits[0].object == 1 && std::fabs(hits[0].t - 0.03f) < 1e-6f && occ[0] == 1 && kept[0] == 2);
        CHECK(hits[1].object == 0 && hits[1].t == 0.5f && occ[1] == 1 && kept[1] == 1);
        CHECK(is_miss(hits[2]) && occ[2] == 0 && kept[2] == 0);
        CHECK(is_miss(hits[3]) && occ[3] == 0 && kept[3] == 2);

        // a cube with a NaN vertex is always kept
        kinds.verts[144 + 5] = NAN;
        CHECK(rt_accel_build(&s, accel.p) == RT_OK);
        CHECK(accel[1].emax2 == INFINITY && accel[1].lo[0] == -INFINITY && accel[1].hi[2] == INFINITY);
        CHECK(rt_accel_kept(rays.p, n, &s, accel.p, 0, kept.p) == RT_OK);
        CHECK(kept[2] == 1);
        kinds.verts[144 + 5] = 58.0f;
        CHECK(rt_accel_build(&s, accel.p) == RT_OK);

        // ---- arguments ----------------------------------------------------------
        const rt_cube_bound* off =
            reinterpret_cast<const rt_cube_bound*>(reinterpret_cast<const char*>(accel.p) + 8);
        CHECK(rt_accel_build(nullptr, accel.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_accel_build(&s, nullptr) == RT_ERR_INVALID_ARG);
        CHECK(rt_accel_build(&s, const_cast<rt_cube_bound*>(off)) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_accel(rays.p, n, &s, nullptr, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_accel(rays.p, n, &s, off, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_accel(nullptr, n, &s, accel.p, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_accel(rays.p, n, nullptr, accel.p, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_accel(rays.p, n, &s, accel.p, nullptr, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_accel(rays.p, -1, &s, accel.p, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays_accel(rays.p, n, &s, nullptr, occ.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays_accel(rays.p, n, &s, off, occ.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays_accel(rays.p, n, &s, accel.p, nullptr) == RT_ERR_INVALID_ARG);
        CHECK(rt_accel_kept(rays.p, n, &s, nullptr, 0, kept.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_accel_kept(rays.p, n, &s, accel.p, 2, kept.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_accel_kept(rays.p, n, &s, accel.p, -1, kept.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_accel_kept(rays.p, n, &s, accel.p, 0, nullptr) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_accel(rays.p, ((int64_t)1 << 39), &s, accel.p, hits.p, tri.p) ==
              RT_ERR_UNSUPPORTED);
        for (int32_t skip : {KindsScene::slots, -2, INT32_MAX, INT32_MIN}) {
            rays[n - 1].skip = skip;
            CHECK(rt_cast_rays_accel(rays.p, n, &s, accel.p, hits.p, tri.p) == RT_ERR_INVALID_ARG);
            CHECK(rt_occlude_rays_accel(rays.p, n, &s, accel.p, occ.p) == RT_ERR_INVALID_ARG);
            CHECK(rt_accel_kept(rays.p, n, &s, accel.p, 0, kept.p) == RT_ERR_INVALID_ARG);
        }
        rt_scene bad = s;
        bad.num_cubes = -1;
        CHECK(rt_accel_build(&bad, accel.p) == RT_ERR_INVALID_ARG);
        bad = s;
        bad.cube_vertices = nullptr;
        CHECK(rt_accel_build(&bad, accel.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_accel(rays.p, 1, &bad, accel.p, hits.p, tri.p) == RT_ERR_INVALID_ARG);
    }
    {
        const int w = 128, rb = 60, re = 68, n = w * (re - rb);
        rt_camera cam{};
        cam.ou[0] = cam.ov[1] = 1.0f;
        cam.d0[2] = kDir[2];
        Exact<rt_hit> hits(n), want(n);
        Exact<int32_t> tri(n), want_tri(n);
        CHECK(rt_cast_camera(&cam, &s, w, rb, re, want.p, want_tri.p) == RT_OK);
        CHECK(rt_cast_camera_accel(&cam, &s, accel.p, w, rb, re, hits.p, tri.p) == RT_OK);
        CHECK(std::memcmp(hits.p, want.p, sizeof(rt_hit) * n) == 0);
        CHECK(std::memcmp(tri.p, want_tri.p, sizeof(int32_t) * n) == 0);
        CHECK(rt_cast_camera_accel(&cam, &s, accel.p, w, rb, re, hits.p, nullptr) == RT_OK);
        CHECK(std::memcmp(hits.p, want.p, sizeof(rt_hit) * n) == 0);
        CHECK(rt_cast_camera_accel(&cam, &empty, nullptr, w, rb, re, hits.p, tri.p) == RT_OK);
        for (int i = 0; i < n; ++i) CHECK(is_miss(hits[i]) && tri[i] == -1);
        CHECK(rt_cast_camera_accel(nullptr, &s, accel.p, w, rb, re, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera_accel(&cam, nullptr, accel.p, w, rb, re, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera_accel(&cam, &s, nullptr, w, rb, re, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera_accel(&cam, &s, accel.p, w, rb, re, nullptr, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera_accel(&cam, &s, accel.p, 0, rb, re, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera_accel(&cam, &s, accel.p, w, re, rb, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
    }
    return finish("accel");
}
