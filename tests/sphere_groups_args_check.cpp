// sphere_groups_args_check.cpp -- rt_sphere_groups_build / rt_sphere_groups_kept /
// rt_cast_rays_grouped / rt_occlude_rays_grouped / rt_cast_camera_grouped
// (csrc/rt_sphere_groups.cpp with csrc/rt_accel.cpp, csrc/rt_light.cpp and
// csrc/rt_args.cpp) as a stand-alone program on tests/light_check.h:
// tests/test_sphere_groups.py builds it with -fsanitize=address,undefined and
// runs it.  No GPU.
//
//   - exactly-sized heap arrays for the records, the rays and every output,
//     16-byte aligned as the contract asks, at n = 0, 1 and 257, and for a
//     scene of 19 spheres at every group_size (a last record that is not full);
//   - the grouped calls against the unculled ones, byte for byte, on the scene
//     of the shadow term's four kinds, and the kept counts of known rays;
//   - a scene of all NULLs with NULL records; a sphere with a NaN radius;
//     records with member indices outside the scene;
//   - a camera's band;
//   - the argument checks.
// Exit 0 and "sphere groups args check ok" on success.
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
    static_assert(sizeof(rt_sphere_group) == 64, "the record");
    KindsScene kinds;
    const rt_scene& s = kinds.s;
    const rt_scene empty{};
    CHECK(rt_sphere_groups_count(2, 1) == 2 && rt_sphere_groups_count(2, 8) == 1);
    CHECK(rt_sphere_groups_count(0, 8) == 0 && rt_sphere_groups_count(9, 8) == 2);
    CHECK(rt_sphere_groups_count(-1, 8) == -1 && rt_sphere_groups_count(2, 0) == -1 &&
          rt_sphere_groups_count(2, 9) == -1);
    CHECK(rt_sphere_groups_count(INT32_MAX, 1) == INT32_MAX);
    CHECK(rt_sphere_groups_workspace_bytes(2) == 32 && rt_sphere_groups_workspace_bytes(-1) == -1);
    Exact<rt_cube_bound> accel(2);
    CHECK(rt_accel_build(&s, accel.p) == RT_OK);
    Exact<rt_sphere_group> groups(2), one(1);
    CHECK(rt_sphere_groups_build(&s, 1, groups.p) == RT_OK);
    CHECK(rt_sphere_groups_build(&s, 8, one.p) == RT_OK);
    // sphere 0: (64, 64, -30) r 12; sphere 1: (118, 64, 12) r 4
    CHECK(groups[0].count == 1 && groups[1].count == 1 && one[0].count == 2);
    CHECK(one[0].member[0] == 0 && one[0].member[1] == 1 && one[0].member[2] == -1 &&
          one[0].member[7] == -1);
    CHECK(one[0].lo[0] == 52.0f && one[0].hi[0] == 122.0f && one[0].lo[2] == -42.0f &&
          one[0].hi[2] == 16.0f && one[0].rmax == 12.0f);
    CHECK(rt_sphere_groups_build(&empty, 8, nullptr) == RT_OK);

    for (int n : {0, 1, 257}) {
        Exact<rt_ray> rays((size_t)n);
        Exact<rt_hit> hits((size_t)n), want((size_t)n);
        Exact<int32_t> tri((size_t)n), want_tri((size_t)n), kept((size_t)n);
        Exact<uint8_t> occ((size_t)n), want_occ((size_t)n);
        // down the z axis at y = 64: over the face, through sphere 0 around x = 64
        for (int i = 0; i < n; ++i) rays[i] = ray(0.5f * i, 64.0f, 0.0f, 0.0f, 0.0f, -100.0f);
        CHECK(rt_cast_rays(rays.p, n, &s, want.p, want_tri.p) == RT_OK);
        CHECK(rt_occlude_rays(rays.p, n, &s, want_occ.p) == RT_OK);
        for (rt_sphere_group* g : {groups.p, one.p}) {
            const int32_t ng = g == groups.p ? 2 : 1;
            CHECK(rt_cast_rays_grouped(rays.p, n, &s, accel.p, g, ng, hits.p, tri.p) == RT_OK);
            CHECK(rt_occlude_rays_grouped(rays.p, n, &s, accel.p, g, ng, occ.p) == RT_OK);
            CHECK(std::memcmp(hits.p, want.p, sizeof(rt_hit) * n) == 0);
            CHECK(std::memcmp(tri.p, want_tri.p, sizeof(int32_t) * n) == 0);
            CHECK(std::memcmp(occ.p, want_occ.p, (size_t)n) == 0);
            CHECK(rt_cast_rays_grouped(rays.p, n, &s, accel.p, g, ng, hits.p, nullptr) == RT_OK);
            CHECK(std::memcmp(hits.p, want.p, sizeof(rt_hit) * n) == 0);
        }
        CHECK(rt_sphere_groups_kept(rays.p, n, &s, groups.p, 2, 0, kept.p) == RT_OK);
        for (int i = 0; i < n; ++i) {
            const float x = 0.5f * i;
            if (x > 53.0f && x < 75.0f) CHECK(kept[i] >= 1 && hits[i].object == 2);
            if (x < 40.0f) CHECK(kept[i] == 0);  // sphere 0's box begins at x = 52
        }
        CHECK(rt_sphere_groups_kept(rays.p, n, &s, groups.p, 2, 1, kept.p) == RT_OK);
        // a scene of all NULLs, NULL records
        CHECK(rt_cast_rays_grouped(rays.p, n, &empty, nullptr, nullptr, 0, hits.p, tri.p) == RT_OK);
        CHECK(rt_occlude_rays_grouped(rays.p, n, &empty, nullptr, nullptr, 0, occ.p) == RT_OK);
        CHECK(rt_sphere_groups_kept(rays.p, n, &empty, nullptr, 0, 0, kept.p) == RT_OK);
        for (int i = 0; i < n; ++i)
            CHECK(is_miss(hits[i]) && tri[i] == -1 && occ[i] == 0 && kept[i] == 0);
    }
    {
        // 19 spheres on a curve, every group_size: exactly-sized records
        const int ns = 19;
        Exact<float> org(4 * ns), rad(ns), col(4 * ns);
        for (int i = 0; i < ns; ++i) {
            org[4 * i] = 10.0f * ((7 * i) % ns);
            org[4 * i + 1] = 3.0f * i;
            org[4 * i + 2] = -20.0f - ((5 * i) % 7);
            org[4 * i + 3] = 1.0f;
            rad[i] = 1.0f + 0.25f * i;
            for (int c = 0; c < 4; ++c) col[4 * i + c] = 0.5f;
        }
        rt_scene many{};
        many.num_spheres = ns;
        many.sphere_origins = org.p;
        many.sphere_radius = rad.p;
        many.sphere_colours = col.p;
        const int n = 64;
        Exact<rt_ray> rays(n);
        Exact<rt_hit> hits(n), want(n);
        Exact<uint8_t> occ(n), want_occ(n);
        Exact<int32_t> kept(n);
        // towards sphere i % ns, further off its centre with every round: hits and misses
        for (int i = 0; i < n; ++i)
            rays[i] = ray(org[4 * (i % ns)] + 1.5f * (i / ns), org[4 * (i % ns) + 1], 0.0f, 0.0f,
                          0.0f, -50.0f);
        CHECK(rt_cast_rays(rays.p, n, &many, want.p, nullptr) == RT_OK);
        CHECK(rt_occlude_rays(rays.p, n, &many, want_occ.p) == RT_OK);
        int met = 0;
        for (int i = 0; i < n; ++i) met += want[i].object >= 0;
        CHECK(met >= 5);
        for (int32_t gs = 1; gs <= 8; ++gs) {
            const int32_t ng = rt_sphere_groups_count(ns, gs);
            Exact<rt_sphere_group> g((size_t)ng);
            CHECK(rt_sphere_groups_build(&many, gs, g.p) == RT_OK);
            int members = 0;
            for (int32_t k = 0; k < ng; ++k) members += g[k].count;
            CHECK(members == ns && g[ng - 1].count == ns - (ng - 1) * gs);
            CHECK(rt_cast_rays_grouped(rays.p, n, &many, nullptr, g.p, ng, hits.p, nullptr) ==
                  RT_OK);
            CHECK(rt_occlude_rays_grouped(rays.p, n, &many, nullptr, g.p, ng, occ.p) == RT_OK);
            CHECK(rt_sphere_groups_kept(rays.p, n, &many, g.p, ng, 0, kept.p) == RT_OK);
            CHECK(std::memcmp(hits.p, want.p, sizeof(rt_hit) * n) == 0);
            CHECK(std::memcmp(occ.p, want_occ.p, (size_t)n) == 0);
            for (int i = 0; i < n; ++i) CHECK(kept[i] >= (want[i].object >= 0) && kept[i] <= ng);
            if (gs == 8) {
                // a NaN radius: its group is always kept, the results stay the unculled ones
                rad[4] = NAN;
                CHECK(rt_sphere_groups_build(&many, gs, g.p) == RT_OK);
                CHECK(g[ng - 1].rmax == INFINITY && g[ng - 1].lo[1] == -INFINITY);
                CHECK(rt_cast_rays(rays.p, n, &many, want.p, nullptr) == RT_OK);
                CHECK(rt_cast_rays_grouped(rays.p, n, &many, nullptr, g.p, ng, hits.p, nullptr) ==
                      RT_OK);
                CHECK(std::memcmp(hits.p, want.p, sizeof(rt_hit) * n) == 0);
                CHECK(rt_sphere_groups_kept(rays.p, n, &many, g.p, ng, 0, kept.p) == RT_OK);
                for (int i = 0; i < n; ++i) CHECK(kept[i] >= 1);
                // foreign member indices and counts: nothing is read through them
                for (int32_t k = 0; k < ng; ++k) {
                    g[k].count = 1000;
                    g[k].member[0] = -7;
                    g[k].member[7] = ns;
                    g[k].member[3] = INT32_MAX;
                }
                CHECK(rt_cast_rays_grouped(rays.p, n, &many, nullptr, g.p, ng, hits.p, nullptr) ==
                      RT_OK);
                CHECK(rt_occlude_rays_grouped(rays.p, n, &many, nullptr, g.p, ng, occ.p) == RT_OK);
                rad[4] = 2.0f;
            }
        }
    }
    {
        const int n = 4;
        Exact<rt_ray> rays(n);
        Exact<rt_hit> hits(n);
        Exact<int32_t> tri(n), kept(n);
        Exact<uint8_t> occ(n);
        rays[0] = ray(64.0f, 64.0f, 0.0f, 0.0f, 0.0f, -100.0f);     // the pole of sphere 0
        rays[1] = ray(64.0f, 64.0f, 0.0f, 0.0f, 0.0f, -100.0f, 2);  // sphere 0 left out
        rays[2] = ray(20.0f, 20.0f, 0.0f, 0.0f, 0.0f, 1.0f);        // a line beside both boxes
        rays[3] = ray(NAN, 64.0f, 0.0f, 0.0f, 0.0f, -1.0f);         // the fallback: both kept
        CHECK(rt_cast_rays_grouped(rays.p, n, &s, accel.p, groups.p, 2, hits.p, tri.p) == RT_OK);
        CHECK(rt_occlude_rays_grouped(rays.p, n, &s, accel.p, groups.p, 2, occ.p) == RT_OK);
        CHECK(rt_sphere_groups_kept(rays.p, n, &s, groups.p, 2, 0, kept.p) == RT_OK);
        CHECK(hits[0].object == 2 && std::fabs(hits[0].t - 0.18f) < 1e-6f && occ[0] == 1 &&
              kept[0] == 1);
        CHECK(hits[1].object == 0 && hits[1].t == 0.5f && occ[1] == 1 && kept[1] == 1);
        CHECK(is_miss(hits[2]) && occ[2] == 0 && kept[2] == 0);
        CHECK(is_miss(hits[3]) && occ[3] == 0 && kept[3] == 2);

        // ---- arguments ----------------------------------------------------------
        rt_sphere_group* off =
            reinterpret_cast<rt_sphere_group*>(reinterpret_cast<char*>(groups.p) + 8);
        CHECK(rt_sphere_groups_build(nullptr, 1, groups.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_sphere_groups_build(&s, 1, nullptr) == RT_ERR_INVALID_ARG);
        CHECK(rt_sphere_groups_build(&s, 1, off) == RT_ERR_INVALID_ARG);
        for (int32_t gs : {0, 9, -1, INT32_MIN, INT32_MAX})
            CHECK(rt_sphere_groups_build(&s, gs, groups.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_grouped(rays.p, n, &s, accel.p, nullptr, 2, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_grouped(rays.p, n, &s, accel.p, off, 2, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        for (int32_t ng : {0, 3, -1, INT32_MAX})
            CHECK(rt_cast_rays_grouped(rays.p, n, &s, accel.p, groups.p, ng, hits.p, tri.p) ==
                  RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_grouped(rays.p, n, &s, nullptr, groups.p, 2, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_grouped(nullptr, n, &s, accel.p, groups.p, 2, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_grouped(rays.p, n, nullptr, accel.p, groups.p, 2, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_grouped(rays.p, n, &s, accel.p, groups.p, 2, nullptr, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_grouped(rays.p, -1, &s, accel.p, groups.p, 2, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays_grouped(rays.p, n, &s, accel.p, nullptr, 2, occ.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays_grouped(rays.p, n, &s, accel.p, off, 2, occ.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays_grouped(rays.p, n, &s, accel.p, groups.p, 3, occ.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_occlude_rays_grouped(rays.p, n, &s, accel.p, groups.p, 2, nullptr) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_sphere_groups_kept(rays.p, n, &s, nullptr, 2, 0, kept.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_sphere_groups_kept(rays.p, n, &s, groups.p, 2, 2, kept.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_sphere_groups_kept(rays.p, n, &s, groups.p, 2, -1, kept.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_sphere_groups_kept(rays.p, n, &s, groups.p, 2, 0, nullptr) == RT_ERR_INVALID_ARG);
        CHECK(rt_sphere_groups_kept(rays.p, n, &empty, nullptr, 1, 0, kept.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_grouped(rays.p, ((int64_t)1 << 39), &s, accel.p, groups.p, 2, hits.p,
                                   tri.p) == RT_ERR_UNSUPPORTED);
        for (int32_t skip : {KindsScene::slots, -2, INT32_MAX, INT32_MIN}) {
            rays[n - 1].skip = skip;
            CHECK(rt_cast_rays_grouped(rays.p, n, &s, accel.p, groups.p, 2, hits.p, tri.p) ==
                  RT_ERR_INVALID_ARG);
            CHECK(rt_occlude_rays_grouped(rays.p, n, &s, accel.p, groups.p, 2, occ.p) ==
                  RT_ERR_INVALID_ARG);
            CHECK(rt_sphere_groups_kept(rays.p, n, &s, groups.p, 2, 0, kept.p) ==
                  RT_ERR_INVALID_ARG);
        }
        rt_scene bad = s;
        bad.num_spheres = -1;
        CHECK(rt_sphere_groups_build(&bad, 1, groups.p) == RT_ERR_INVALID_ARG);
        bad = s;
        bad.sphere_radius = nullptr;
        CHECK(rt_sphere_groups_build(&bad, 1, groups.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_rays_grouped(rays.p, 1, &bad, accel.p, groups.p, 2, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
    }
    {
        const int w = 128, rb = 60, re = 68, n = w * (re - rb);
        rt_camera cam{};
        cam.ou[0] = cam.ov[1] = 1.0f;
        cam.d0[2] = kDir[2];
        Exact<rt_hit> hits(n), want(n);
        Exact<int32_t> tri(n), want_tri(n);
        CHECK(rt_cast_camera(&cam, &s, w, rb, re, want.p, want_tri.p) == RT_OK);
        CHECK(rt_cast_camera_grouped(&cam, &s, accel.p, groups.p, 2, w, rb, re, hits.p, tri.p) ==
              RT_OK);
        CHECK(std::memcmp(hits.p, want.p, sizeof(rt_hit) * n) == 0);
        CHECK(std::memcmp(tri.p, want_tri.p, sizeof(int32_t) * n) == 0);
        CHECK(rt_cast_camera_grouped(&cam, &s, accel.p, one.p, 1, w, rb, re, hits.p, nullptr) ==
              RT_OK);
        CHECK(std::memcmp(hits.p, want.p, sizeof(rt_hit) * n) == 0);
        CHECK(rt_cast_camera_grouped(&cam, &empty, nullptr, nullptr, 0, w, rb, re, hits.p, tri.p) ==
              RT_OK);
        for (int i = 0; i < n; ++i) CHECK(is_miss(hits[i]) && tri[i] == -1);
        CHECK(rt_cast_camera_grouped(nullptr, &s, accel.p, groups.p, 2, w, rb, re, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera_grouped(&cam, nullptr, accel.p, groups.p, 2, w, rb, re, hits.p,
                                     tri.p) == RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera_grouped(&cam, &s, accel.p, nullptr, 2, w, rb, re, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera_grouped(&cam, &s, accel.p, groups.p, 3, w, rb, re, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera_grouped(&cam, &s, accel.p, groups.p, 2, w, rb, re, nullptr, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera_grouped(&cam, &s, accel.p, groups.p, 2, 0, rb, re, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_cast_camera_grouped(&cam, &s, accel.p, groups.p, 2, w, re, rb, hits.p, tri.p) ==
              RT_ERR_INVALID_ARG);
    }
    return finish("sphere groups");
}
