// rays_args_check.cpp -- rt_cast_rays / rt_occlude_rays / rt_camera_rays /
// rt_cast_camera (csrc/rt_light.cpp with csrc/rt_args.cpp) as a stand-alone
// program on tests/light_check.h: tests/test_rays.py builds it with
// -fsanitize=address,undefined and runs it.  No GPU.
//
//   - exactly-sized heap arrays for the rays and every output, 16-byte aligned
//     as the contract asks (an overrun on either side is reported), at n = 0, 1
//     and 257;
//   - the face, the box and the two spheres of the shadow term's scene, known
//     rays: onto the face, onto the pole of sphere 0, past everything, from
//     inside sphere 0, with the face left out;
//   - NULL out_triangle;
//   - a scene of all NULLs;
//   - a camera's band into exactly-sized arrays, and rt_cast_camera on it;
//   - the argument checks.
// Exit 0 and "rays args check ok" on success.
#include <new>

#include "light_check.h"

using namespace light_check;

namespace {

// T[n] at a 16-byte boundary, of exactly n * sizeof(T) bytes
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
    KindsScene kinds;
    const rt_scene& s = kinds.s;
    const rt_scene empty{};

    for (int n : {0, 1, 257}) {
        Exact<rt_ray> rays((size_t)n);
        Exact<rt_hit> hits((size_t)n), again((size_t)n);
        Exact<int32_t> tri((size_t)n);
        Exact<uint8_t> occ((size_t)n);
        // down the rows of the frame's column x = i / 2: onto the face (t = 50 from z = 0)
        for (int i = 0; i < n; ++i) rays[i] = ray(0.5f * i, 20.0f, 0.0f, 0.0f, 0.0f, -1.0f);
        CHECK(rt_cast_rays(rays.p, n, &s, hits.p, tri.p) == RT_OK);
        CHECK(rt_cast_rays(rays.p, n, &s, again.p, nullptr) == RT_OK);
        CHECK(rt_occlude_rays(rays.p, n, &s, occ.p) == RT_OK);
        for (int i = 0; i < n; ++i) {
            CHECK(hits[i].object == 0 && hits[i].t == 50.0f && tri[i] >= 0 && tri[i] < 12);
            CHECK(std::memcmp(&hits[i], &again[i], sizeof(rt_hit)) == 0);
            CHECK(occ[i] == 0);  // the segment ends at z = -1
        }
        // a scene of all NULLs: nothing to hit
        CHECK(rt_cast_rays(rays.p, n, &empty, hits.p, tri.p) == RT_OK);
        CHECK(rt_occlude_rays(rays.p, n, &empty, occ.p) == RT_OK);
        for (int i = 0; i < n; ++i) CHECK(is_miss(hits[i]) && tri[i] == -1 && occ[i] == 0);
    }
    {
        const int n = 6;
        Exact<rt_ray> rays(n);
        Exact<rt_hit> hits(n);
        Exact<int32_t> tri(n);
        Exact<uint8_t> occ(n);
        rays[0] = ray(64.0f, 64.0f, 0.0f, 0.0f, 0.0f, -2.0f);      // the pole of sphere 0: 18 / 2
        rays[1] = ray(64.0f, 64.0f, 0.0f, 0.0f, 0.0f, 1.0f);       // away from everything
        rays[2] = ray(64.0f, 64.0f, -30.0f, 0.0f, 0.0f, -1.0f);    // from its centre: the far root
        rays[3] = ray(20.0f, 20.0f, 0.0f, 0.0f, 0.0f, -100.0f, 0); // the face left out
        rays[4] = ray(20.0f, 20.0f, 0.0f, 0.0f, 0.0f, -100.0f);    // the face at 0.5
        rays[5] = ray(64.0f, 64.0f, 0.0f, 0.0f, 0.0f, -100.0f, 2); // sphere 0 left out: the face
        CHECK(rt_cast_rays(rays.p, n, &s, hits.p, tri.p) == RT_OK);
        CHECK(rt_occlude_rays(rays.p, n, &s, occ.p) == RT_OK);
        CHECK(hits[0].object == 2 && hits[0].t == 9.0f && tri[0] == -1 && occ[0] == 0);
        CHECK(is_miss(hits[1]) && tri[1] == -1 && occ[1] == 0);
        CHECK(hits[2].object == 2 && hits[2].t == 12.0f && occ[2] == 0);
        CHECK(is_miss(hits[3]) && occ[3] == 0);
        CHECK(hits[4].object == 0 && hits[4].t == 0.5f && tri[4] >= 0 && occ[4] == 1);
        CHECK(hits[5].object == 0 && hits[5].t == 0.5f && occ[5] == 1);

        // ---- arguments ----------------------------------------------------------
        CHECK(rt_cast_rays(nullptr, n, &s, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays(rays.p, n, nullptr, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays(rays.p, n, &s, nullptr, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays(rays.p, -1, &s, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays(nullptr, n, &s, occ.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays(rays.p, n, nullptr, occ.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays(rays.p, n, &s, nullptr) == RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays(rays.p, -1, &s, occ.p) == RT_ERR_INVALID_ARG);
        const rt_ray* off = reinterpret_cast<const rt_ray*>(reinterpret_cast<const char*>(rays.p) + 8);
        CHECK(rt_cast_rays(off, 1, &s, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays(off, 1, &s, occ.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays(rays.p, 1, &s, reinterpret_cast<rt_hit*>(&hits[0].object), tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays(rays.p, 1, &s, hits.p,
                           reinterpret_cast<int32_t*>(reinterpret_cast<char*>(tri.p) + 2)) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays(rays.p, ((int64_t)1 << 39), &s, hits.p, tri.p) == RT_ERR_UNSUPPORTED);
        for (int32_t skip : {KindsScene::slots, -2, INT32_MAX, INT32_MIN}) {
            rays[n - 1].skip = skip;
            CHECK(rt_cast_rays(rays.p, n, &s, hits.p, tri.p) == RT_ERR_INVALID_ARG);
            CHECK(rt_occlude_rays(rays.p, n, &s, occ.p) == RT_ERR_INVALID_ARG);
        }
        rays[n - 1].skip = KindsScene::slots - 1;
        CHECK(rt_cast_rays(rays.p, n, &s, hits.p, tri.p) == RT_OK);
        rt_scene bad = s;
        bad.num_spheres = -1;
        CHECK(rt_cast_rays(rays.p, n, &bad, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        bad = s;
        bad.cube_vertices = nullptr;
        CHECK(rt_occlude_rays(rays.p, n, &bad, occ.p) == RT_ERR_INVALID_ARG);
    }
    {
        // rows 60..67 of the scene's 128-wide frame through the library's own rays
        const int w = 128, rb = 60, re = 68, n = w * (re - rb);
        // (written out: rt_camera_reference is csrc/rt_scene.cpp's)
        rt_camera cam{};
        cam.ou[0] = cam.ov[1] = 1.0f;
        cam.d0[2] = kDir[2];
        Exact<rt_ray> rays(n);
        Exact<rt_hit> hits(n), direct(n);
        Exact<int32_t> tri(n), direct_tri(n);
        CHECK(rt_camera_rays(&cam, w, rb, re, rays.p) == RT_OK);
        CHECK(rt_cast_rays(rays.p, n, &s, hits.p, tri.p) == RT_OK);
        CHECK(rt_cast_camera(&cam, &s, w, rb, re, direct.p, direct_tri.p) == RT_OK);
        CHECK(std::memcmp(hits.p, direct.p, sizeof(rt_hit) * n) == 0);
        CHECK(std::memcmp(tri.p, direct_tri.p, sizeof(int32_t) * n) == 0);
        CHECK(rt_cast_camera(&cam, &s, w, rb, re, direct.p, nullptr) == RT_OK);
        CHECK(std::memcmp(hits.p, direct.p, sizeof(rt_hit) * n) == 0);
        CHECK(rays[0].ox == 0.0f && rays[0].oy == 60.0f && rays[n - 1].ox == 127.0f &&
              rays[n - 1].oy == 67.0f && rays[5].skip == -1 && rays[5].dz == -1.0f);
        CHECK(hits[4 * w + 64].object == 2 && hits[4 * w + 64].t == 18.0f);  // the pole of sphere 0
        CHECK(hits[5].object == 0 && hits[5].t == 50.0f);
        CHECK(rt_cast_camera(&cam, &empty, w, rb, re, direct.p, direct_tri.p) == RT_OK);
        for (int i = 0; i < n; ++i) CHECK(is_miss(direct[i]) && direct_tri[i] == -1);

        CHECK(rt_camera_rays(nullptr, w, rb, re, rays.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_camera_rays(&cam, w, rb, re, nullptr) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera(nullptr, &s, w, rb, re, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera(&cam, nullptr, w, rb, re, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera(&cam, &s, w, rb, re, nullptr, tri.p) == RT_ERR_INVALID_ARG);
        const int32_t top = 1 << 24;
        const int32_t shapes[][3] = {{0, rb, re},      {-1, rb, re}, {top + 1, 0, 1}, {w, -1, re - 1},
                                     {w, re, re},      {w, re, rb},  {w, top, top + 1}};
        for (const auto& shape : shapes) {
            CHECK(rt_camera_rays(&cam, shape[0], shape[1], shape[2], rays.p) == RT_ERR_INVALID_ARG);
            CHECK(rt_cast_camera(&cam, &s, shape[0], shape[1], shape[2], hits.p, tri.p) ==
                  RT_ERR_INVALID_ARG);
        }
        CHECK(rt_camera_rays(&cam, top, 0, top, rays.p) == RT_ERR_UNSUPPORTED);
        for (int32_t normalise : {2, -1}) {
            rt_camera odd = cam;
            odd.normalise = normalise;
            CHECK(rt_camera_rays(&odd, w, rb, re, rays.p) == RT_ERR_INVALID_ARG);
            CHECK(rt_cast_camera(&odd, &s, w, rb, re, hits.p, tri.p) == RT_ERR_INVALID_ARG);
        }
    }
    return finish("rays");
}
