// shadow_args_check.cpp -- rt_shadow_hits / rt_light_hits_shadowed
// (csrc/rt_light.cpp with csrc/rt_args.cpp) as a stand-alone program like
// light_args_check.cpp: tests/test_shadow_hits.py builds it with
// -fsanitize=address,undefined and runs it.  No GPU.
//
//   - exactly-sized heap arrays for the frame, the scene and every output
//     (an overrun on either side is reported);
//   - the scene of the four occluder / receiver kinds, a band of it, known
//     pixels: a face pixel behind sphere 0, one that sees the light, the
//     sphere's pole behind the box;
//   - an empty scene with NULL arrays, with and without lights;
//   - 32 and 33 lights;
//   - the argument checks.
// Exit 0 and "shadow args check ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "rt_hip.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, \
                         #cond);                                                 \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

const float kDir[4] = {0.0f, 0.0f, -1.0f, -1.0f};
const int32_t kBlack[4] = {0, 0, 0, 255};

// an axis-aligned box as a cube's float4[36], Cube.cpp's corner order
void box(float* verts, const float lo[3], const float hi[3]) {
    // corner bit0 = x, bit1 = y, bit2 = z (set = hi)
    const unsigned char corners[36] = {0, 4, 6, 3, 0, 2, 5, 0, 1, 3, 1, 0, 0, 6, 2, 5, 4, 0,
                                       6, 4, 5, 7, 1, 3, 1, 7, 5, 7, 3, 2, 7, 2, 6, 7, 6, 5};
    for (int k = 0; k < 36; ++k) {
        for (int a = 0; a < 3; ++a) verts[4 * k + a] = (corners[k] >> a & 1u) ? hi[a] : lo[a];
        verts[4 * k + 3] = 1.0f;
    }
}

}  // namespace

int main() {
    // ---- the four kinds: cube 0 (the face z = -50), cube 1 (the box), sphere
    // 0 (slot 2), sphere 1 (slot 3, only occludes), one light ---------------
    std::unique_ptr<float[]> verts(new float[2 * 144]);
    {
        const float lo0[3] = {-6.0f, -6.0f, -70.0f}, hi0[3] = {134.0f, 134.0f, -50.0f};
        const float lo1[3] = {85.0f, 58.0f, -15.0f}, hi1[3] = {97.0f, 70.0f, -3.0f};
        box(verts.get(), lo0, hi0);
        box(verts.get() + 144, lo1, hi1);
    }
    std::unique_ptr<float[]> cube_col(new float[8]{1.0f, 0.7f, 0.3f, 255.0f, 0.3f, 0.5f, 1.0f, 255.0f});
    std::unique_ptr<float[]> sph_org(new float[8]{64.0f, 64.0f, -30.0f, 1.0f, 118.0f, 64.0f, 12.0f, 1.0f});
    std::unique_ptr<float[]> sph_rad(new float[2]{12.0f, 4.0f});
    std::unique_ptr<float[]> sph_col(new float[8]{0.2f, 0.9f, 0.4f, 255.0f, 0.9f, 0.9f, 0.1f, 255.0f});
    std::unique_ptr<float[]> light(new float[4]{154.0f, 64.0f, 40.0f, 1.0f});
    rt_scene s{};
    s.num_cubes = 2;
    s.cube_vertices = verts.get();
    s.cube_colours = cube_col.get();
    s.num_spheres = 2;
    s.sphere_origins = sph_org.get();
    s.sphere_radius = sph_rad.get();
    s.sphere_colours = sph_col.get();
    s.num_lights = 1;
    s.lights = light.get();

    // rows 60..67 of the 128-wide frame, every pixel on the face (t = 50) but
    // (64, 64): the pole of sphere 0 (t = 18)
    {
        const int w = 128, rb = 60, re = 68, n = w * (re - rb);
        std::unique_ptr<rt_hit[]> hits(new rt_hit[n]);
        for (int i = 0; i < n; ++i) hits[i] = rt_hit{50.0f, 0};
        hits[4 * w + 64] = rt_hit{18.0f, 2};
        hits[7 * w + 127] = rt_hit{300000.0f, -1};
        std::unique_ptr<uint32_t[]> mask(new uint32_t[n]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> plain(new int32_t[4 * n]);
        std::unique_ptr<uint32_t[]> words(new uint32_t[n]);
        CHECK(rt_shadow_hits(hits.get(), &s, kDir, w, rb, re, mask.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed(hits.get(), &s, kDir, w, rb, re, RT_FORMAT_I32X4, px.get()) ==
              RT_OK);
        CHECK(rt_light_hits_shadowed(hits.get(), &s, kDir, w, rb, re, RT_FORMAT_RGBA8,
                                     words.get()) == RT_OK);
        CHECK(rt_light_hits(hits.get(), &s, kDir, w, rb, re, RT_FORMAT_I32X4, plain.get()) == RT_OK);
        // (38, 64): the segment to the light passes the centre of sphere 0
        CHECK(mask[4 * w + 38] == 1u);
        CHECK(std::memcmp(&px[4 * (4 * w + 38)], kBlack, sizeof kBlack) == 0);
        CHECK(words[4 * w + 38] == 0xFF000000u);
        CHECK(plain[4 * (4 * w + 38)] > 0);
        // (5, 60) sees the light
        CHECK(mask[5] == 0u && px[4 * 5] > 0);
        CHECK(std::memcmp(&px[4 * 5], &plain[4 * 5], 16) == 0);
        // the pole of sphere 0: behind the box
        CHECK(mask[4 * w + 64] == 1u && plain[4 * (4 * w + 64)] > 0);
        CHECK(std::memcmp(&px[4 * (4 * w + 64)], kBlack, sizeof kBlack) == 0);
        // the miss
        CHECK(mask[n - 1] == 0u && words[n - 1] == 0xFF000000u);
        for (int i = 0; i < n; ++i) {
            CHECK(mask[i] <= 1u);
            if (!mask[i]) CHECK(std::memcmp(&px[4 * i], &plain[4 * i], 16) == 0);
        }

        // ---- 32 and 33 lights -------------------------------------------------
        std::unique_ptr<float[]> many(new float[4 * 33]);
        for (int i = 0; i < 33; ++i) {
            many[4 * i] = 154.0f - 5.0f * i;
            many[4 * i + 1] = 64.0f;
            many[4 * i + 2] = 40.0f;
            many[4 * i + 3] = 1.0f;
        }
        rt_scene m = s;
        m.lights = many.get();
        m.num_lights = 33;
        CHECK(rt_shadow_hits(hits.get(), &m, kDir, w, rb, re, mask.get()) == RT_ERR_UNSUPPORTED);
        CHECK(rt_light_hits_shadowed(hits.get(), &m, kDir, w, rb, re, RT_FORMAT_I32X4, px.get()) ==
              RT_OK);
        CHECK(rt_light_hits_shadowed(hits.get(), &m, kDir, w, rb, re, RT_FORMAT_RGBA8,
                                     words.get()) == RT_OK);
        m.num_lights = 32;
        std::unique_ptr<float[]> many32(new float[4 * 32]);
        std::memcpy(many32.get(), many.get(), sizeof(float) * 4 * 32);
        m.lights = many32.get();
        CHECK(rt_shadow_hits(hits.get(), &m, kDir, w, rb, re, mask.get()) == RT_OK);
        CHECK((mask[4 * w + 38] & 1u) == 1u);

        // ---- arguments ----------------------------------------------------------
        CHECK(rt_shadow_hits(nullptr, &s, kDir, w, rb, re, mask.get()) == RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits(hits.get(), nullptr, kDir, w, rb, re, mask.get()) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits(hits.get(), &s, nullptr, w, rb, re, mask.get()) == RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits(hits.get(), &s, kDir, w, rb, re, nullptr) == RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits(hits.get(), &s, kDir, 0, rb, re, mask.get()) == RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits(hits.get(), &s, kDir, w, -1, re, mask.get()) == RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits(hits.get(), &s, kDir, w, re, re, mask.get()) == RT_ERR_INVALID_ARG);
        CHECK(rt_light_hits_shadowed(hits.get(), &s, kDir, w, rb, re, 0, nullptr) ==
              RT_ERR_INVALID_ARG);
        for (int32_t fmt : {2, (int32_t)RT_FORMAT_HIT, 4, -1})
            CHECK(rt_light_hits_shadowed(hits.get(), &s, kDir, w, rb, re, fmt, px.get()) ==
                  RT_ERR_INVALID_ARG);
        rt_scene bad = s;
        bad.lights = nullptr;
        CHECK(rt_shadow_hits(hits.get(), &bad, kDir, w, rb, re, mask.get()) == RT_ERR_INVALID_ARG);
        bad = s;
        bad.num_lights = -1;
        CHECK(rt_light_hits_shadowed(hits.get(), &bad, kDir, w, rb, re, 0, px.get()) ==
              RT_ERR_INVALID_ARG);
        for (int32_t obj : {4, -2, INT32_MAX, INT32_MIN}) {
            hits[n - 1].object = obj;
            CHECK(rt_shadow_hits(hits.get(), &s, kDir, w, rb, re, mask.get()) ==
                  RT_ERR_INVALID_ARG);
            CHECK(rt_light_hits_shadowed(hits.get(), &s, kDir, w, rb, re, 0, px.get()) ==
                  RT_ERR_INVALID_ARG);
        }
    }

    // ---- an empty scene with NULL arrays: every pixel a miss -----------------
    {
        rt_scene empty{};
        const int w = 5, rows = 3;
        std::unique_ptr<rt_hit[]> hits(new rt_hit[w * rows]);
        for (int i = 0; i < w * rows; ++i) hits[i] = rt_hit{300000.0f, -1};
        std::unique_ptr<uint32_t[]> mask(new uint32_t[w * rows]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * w * rows]);
        for (int with_light = 0; with_light < 2; ++with_light) {
            empty.lights = with_light ? light.get() : nullptr;
            empty.num_lights = with_light;
            CHECK(rt_shadow_hits(hits.get(), &empty, kDir, w, 0, rows, mask.get()) == RT_OK);
            CHECK(rt_light_hits_shadowed(hits.get(), &empty, kDir, w, 0, rows, RT_FORMAT_I32X4,
                                         px.get()) == RT_OK);
            for (int i = 0; i < w * rows; ++i) {
                CHECK(mask[i] == 0u);
                CHECK(std::memcmp(&px[4 * i], kBlack, sizeof kBlack) == 0);
            }
        }
        // any object is out of range in an empty scene
        hits[w * rows - 1].object = 0;
        CHECK(rt_shadow_hits(hits.get(), &empty, kDir, w, 0, rows, mask.get()) ==
              RT_ERR_INVALID_ARG);
    }
    if (failures) return 1;
    std::printf("shadow args check ok\n");
    return 0;
}
