// light_args_check.cpp -- rt_hit_surfaces / rt_light_hits (csrc/rt_light.cpp
// with csrc/rt_args.cpp) as a stand-alone program on tests/light_check.h:
// tests/test_light_hits.py builds it with -fsanitize=address,undefined and
// runs it.  No GPU.
//
//   - exactly-sized heap arrays for the frame, the scene and every output
//     (an overrun on either side is reported);
//   - empty scenes with NULL arrays;
//   - a one-row band at a large row_begin (the 64-bit pixel arithmetic);
//   - known pixels: a sphere under a light straight ahead and behind it, a
//     cube face seen head on, a foreign t;
//   - the argument checks.
// Exit 0 and "light args check ok" on success.
#include "light_check.h"

using namespace light_check;

namespace {

bool is_zero_surface(const rt_surface& s) {
    return s.nx == 0.0f && s.ny == 0.0f && s.nz == 0.0f && s.triangle == -1;
}

}  // namespace

int main() {
    static_assert(sizeof(rt_surface) == 16, "four 32-bit words per pixel");

    // ---- one cube (slot 0), one sphere (slot 1), one light -----------------
    // the cube: x, y in [0, 8], z in [-60, -40]; two triangles per face, only
    // the front face (z = -40) matters for rays along -z
    std::unique_ptr<float[]> verts(new float[144]);
    {
        const float lo[3] = {0.0f, 0.0f, -60.0f}, hi[3] = {8.0f, 8.0f, -40.0f};
        box(verts.get(), lo, hi);
    }
    std::unique_ptr<float[]> cube_col(new float[4]{1.0f, 0.5f, 0.25f, 255.0f});
    std::unique_ptr<float[]> sph_org(new float[4]{32.0f, 24.0f, -50.0f, 1.0f});
    std::unique_ptr<float[]> sph_rad(new float[1]{20.0f});
    std::unique_ptr<float[]> sph_col(new float[4]{1.0f, 1.0f, 1.0f, 255.0f});
    std::unique_ptr<float[]> light(new float[4]{32.0f, 24.0f, 0.0f, 1.0f});
    rt_scene s{};
    s.num_cubes = 1;
    s.cube_vertices = verts.get();
    s.cube_colours = cube_col.get();
    s.num_spheres = 1;
    s.sphere_origins = sph_org.get();
    s.sphere_radius = sph_rad.get();
    s.sphere_colours = sph_col.get();
    s.num_lights = 1;
    s.lights = light.get();

    // row 24 of a 64-wide frame: pixel 4 is on the cube's front face (t = 40),
    // pixel 32 under the sphere's centre (t = 30), the rest misses
    {
        const int w = 64;
        std::unique_ptr<rt_hit[]> hits(new rt_hit[w]);
        for (int i = 0; i < w; ++i) hits[i] = rt_hit{300000.0f, -1};
        hits[32] = rt_hit{30.0f, 1};
        std::unique_ptr<rt_surface[]> surf(new rt_surface[w]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * w]);
        std::unique_ptr<uint32_t[]> words(new uint32_t[w]);
        CHECK(rt_hit_surfaces(hits.get(), &s, kDir, w, 24, 25, surf.get()) == RT_OK);
        CHECK(surf[32].nx == 0.0f && surf[32].ny == 0.0f && surf[32].nz == 1.0f &&
              surf[32].triangle == -1);
        CHECK(is_zero_surface(surf[0]) && is_zero_surface(surf[w - 1]));
        CHECK(rt_light_hits(hits.get(), &s, kDir, w, 24, 25, RT_FORMAT_I32X4, px.get()) == RT_OK);
        // k = 1: scalar = 255 - 30 / 180 * 255 = 212.5
        CHECK(px[4 * 32] == 212 && px[4 * 32 + 1] == 212 && px[4 * 32 + 3] == 255);
        CHECK(std::memcmp(&px[0], kBlack, sizeof kBlack) == 0);
        light[2] = -200.0f;  // behind the sphere: k = 0
        CHECK(rt_light_hits(hits.get(), &s, kDir, w, 24, 25, RT_FORMAT_RGBA8, words.get()) ==
              RT_OK);
        CHECK(words[32] == 0xFF000000u && words[0] == 0xFF000000u);
        light[2] = 0.0f;
    }
    // row 4: the cube face, and the same pixel with a t no triangle gives
    {
        const int w = 8;
        std::unique_ptr<rt_hit[]> hits(new rt_hit[w]);
        for (int i = 0; i < w; ++i) hits[i] = rt_hit{40.0f, 0};
        hits[5].t = 40.000004f;  // one ulp above 40
        std::unique_ptr<rt_surface[]> surf(new rt_surface[w]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * w]);
        CHECK(rt_hit_surfaces(hits.get(), &s, kDir, w, 4, 5, surf.get()) == RT_OK);
        for (int i = 1; i < w; ++i) {
            if (i == 5) continue;
            CHECK(surf[i].nx == 0.0f && surf[i].ny == 0.0f && surf[i].nz == 1.0f);
            CHECK(surf[i].triangle == 6 || surf[i].triangle == 11);
        }
        CHECK(is_zero_surface(surf[5]));
        CHECK(rt_light_hits(hits.get(), &s, kDir, w, 4, 5, RT_FORMAT_I32X4, px.get()) == RT_OK);
        CHECK(std::memcmp(&px[4 * 5], kBlack, sizeof kBlack) == 0);
        CHECK(px[4 * 3] > 0 && px[4 * 3 + 3] == 255);
    }
    // a one-row band at the last legal row: row_end = 2^24
    {
        const int w = 3;
        const int32_t rb = (1 << 24) - 1;
        std::unique_ptr<rt_hit[]> hits(new rt_hit[w]{{300000.0f, -1}, {50.0f, 1}, {50.0f, 0}});
        std::unique_ptr<rt_surface[]> surf(new rt_surface[w]);
        std::unique_ptr<uint32_t[]> words(new uint32_t[w]);
        CHECK(rt_hit_surfaces(hits.get(), &s, kDir, w, rb, rb + 1, surf.get()) == RT_OK);
        CHECK(is_zero_surface(surf[0]) && is_zero_surface(surf[2]));  // no triangle up there
        CHECK(surf[1].triangle == -1 && surf[1].ny > 0.99f);         // p.y is far past the centre
        CHECK(rt_light_hits(hits.get(), &s, kDir, w, rb, rb + 1, RT_FORMAT_RGBA8, words.get()) ==
              RT_OK);
        CHECK(words[0] == 0xFF000000u);
        CHECK(rt_hit_surfaces(hits.get(), &s, kDir, w, rb + 1, rb + 2, surf.get()) ==
              RT_ERR_INVALID_ARG);
    }

    // ---- arguments -------------------------------------------------------------
    auto own = [](const Call& c) {
        return rt_hit_surfaces(c.hits, c.scene, c.dir, c.w, c.rb, c.re, (rt_surface*)c.out);
    };
    auto lit = [](const Call& c, int32_t fmt) {
        return rt_light_hits(c.hits, c.scene, c.dir, c.w, c.rb, c.re, fmt, c.out);
    };
    {
        std::unique_ptr<rt_hit[]> hits(new rt_hit[4]{{300000.0f, -1}, {50.0f, 1}, {50.0f, 0},
                                                     {300000.0f, -1}});
        std::unique_ptr<rt_surface[]> surf(new rt_surface[4]);
        std::unique_ptr<int32_t[]> px(new int32_t[16]);
        const Call to_px{hits.get(), &s, kDir, 2, 0, 2, px.get()};
        refused_formats(lit, to_px);
        refusals([&](const Call& c) { return lit(c, 0); }, to_px, &hits[3], 2);
        refusals(own, Call{hits.get(), &s, kDir, 2, 0, 2, surf.get()}, &hits[3], 2);
    }
    empty_scene<rt_surface>(light.get(), own, lit, is_zero_surface);
    return finish("light");
}
