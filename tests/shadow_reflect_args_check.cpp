// shadow_reflect_args_check.cpp -- rt_shadow_hits_reflected /
// rt_light_hits_shadowed_reflected (csrc/rt_light.cpp with csrc/rt_args.cpp) as
// a stand-alone program like reflect_args_check.cpp:
// tests/test_shadow_reflect_hits.py builds it with -fsanitize=address,undefined
// and runs it.  No GPU.
//
//   - exactly-sized heap arrays for the frame, the scene and every output
//     (an overrun on either side is reported);
//   - the face, the box and the two spheres of the shadow term's scene, a
//     band of it: the face under the unseen sphere (a bounce point no light
//     faces), the flank of sphere 0 (a bounce point on the face), a miss; the
//     identities with rt_light_hits_shadowed, rt_light_hits_reflected and the
//     two masks;
//   - an empty scene with NULL arrays, with and without lights;
//   - reflectivity 0, 0.25 and 1, and the refused ones; 33 lights;
//   - the argument checks.
// Exit 0 and "shadow reflect args check ok" on success.
#include <cmath>
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
    // ---- cube 0 (the face z = -50), cube 1 (the box), sphere 0 (slot 2),
    // sphere 1 (slot 3, in front of the ray origins), one light ----------------
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
    // (64, 64), the pole of sphere 0 (t = 18), (75, 64) on its flank and a miss
    {
        const int w = 128, rb = 60, re = 68, n = w * (re - rb);
        std::unique_ptr<rt_hit[]> hits(new rt_hit[n]);
        for (int i = 0; i < n; ++i) hits[i] = rt_hit{50.0f, 0};
        hits[4 * w + 64] = rt_hit{18.0f, 2};
        hits[4 * w + 75] = rt_hit{30.0f - std::sqrt(23.0f), 2};
        hits[7 * w + 127] = rt_hit{300000.0f, -1};
        std::unique_ptr<rt_hit[]> bounce(new rt_hit[n]);
        std::unique_ptr<uint32_t[]> mask(new uint32_t[n]);
        std::unique_ptr<uint32_t[]> mask2(new uint32_t[n]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> full(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> zero(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> shadowed(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> mirrored(new int32_t[4 * n]);
        std::unique_ptr<uint32_t[]> words(new uint32_t[n]);
        CHECK(rt_reflect_hits(hits.get(), &s, kDir, w, rb, re, bounce.get()) == RT_OK);
        CHECK(rt_shadow_hits(hits.get(), &s, kDir, w, rb, re, mask.get()) == RT_OK);
        CHECK(rt_shadow_hits_reflected(hits.get(), &s, kDir, w, rb, re, mask2.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed_reflected(hits.get(), &s, kDir, w, rb, re, 0.25f,
                                               RT_FORMAT_I32X4, px.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed_reflected(hits.get(), &s, kDir, w, rb, re, 1.0f,
                                               RT_FORMAT_I32X4, full.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed_reflected(hits.get(), &s, kDir, w, rb, re, 0.0f,
                                               RT_FORMAT_I32X4, zero.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed_reflected(hits.get(), &s, kDir, w, rb, re, 0.25f,
                                               RT_FORMAT_RGBA8, words.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed(hits.get(), &s, kDir, w, rb, re, RT_FORMAT_I32X4,
                                     shadowed.get()) == RT_OK);
        CHECK(rt_light_hits_reflected(hits.get(), &s, kDir, w, rb, re, 0.25f, RT_FORMAT_I32X4,
                                      mirrored.get()) == RT_OK);
        // reflectivity 0: rt_light_hits_shadowed's frame
        CHECK(std::memcmp(zero.get(), shadowed.get(), sizeof(int32_t) * 4 * n) == 0);
        // (118, 64): straight back from z = -50 to the lowest point of sphere 1,
        // whose normal there points down: the light above faces away, k2 = 0
        CHECK(bounce[4 * w + 118].object == 3 && mask2[4 * w + 118] == 0);
        CHECK(std::memcmp(&full[4 * (4 * w + 118)], kBlack, sizeof kBlack) == 0);
        // the flank of sphere 0 mirrors down onto the face, which faces the light
        CHECK(bounce[4 * w + 75].object == 0);
        // the miss
        CHECK(mask2[n - 1] == 0 && words[n - 1] == 0xFF000000u);
        CHECK(std::memcmp(&px[4 * (n - 1)], kBlack, sizeof kBlack) == 0);
        int shadowed_at_p = 0, differ = 0;
        for (int i = 0; i < n; ++i) {
            CHECK(mask2[i] <= 1u);  // one light
            CHECK(bounce[i].object >= 0 || mask2[i] == 0);
            CHECK(px[4 * i + 3] == 255 && (words[i] >> 24) == 0xFFu);
            // no light hidden at p nor at p2: rt_light_hits_reflected's pixel
            if (mask[i] == 0 && mask2[i] == 0)
                CHECK(std::memcmp(&px[4 * i], &mirrored[4 * i], 16) == 0);
            shadowed_at_p += mask[i] != 0;
            differ += std::memcmp(&px[4 * i], &mirrored[4 * i], 16) != 0;
        }
        CHECK(shadowed_at_p > 0 && differ > 0);

        // without lights: rt_light_hits_reflected's frame, and no mask
        {
            rt_scene dark = s;
            dark.num_lights = 0;
            dark.lights = nullptr;
            CHECK(rt_light_hits_shadowed_reflected(hits.get(), &dark, kDir, w, rb, re, 0.25f,
                                                   RT_FORMAT_I32X4, px.get()) == RT_OK);
            CHECK(rt_light_hits_reflected(hits.get(), &dark, kDir, w, rb, re, 0.25f,
                                          RT_FORMAT_I32X4, mirrored.get()) == RT_OK);
            CHECK(std::memcmp(px.get(), mirrored.get(), sizeof(int32_t) * 4 * n) == 0);
            CHECK(rt_shadow_hits_reflected(hits.get(), &dark, kDir, w, rb, re, mask2.get()) ==
                  RT_OK);
            for (int i = 0; i < n; ++i) CHECK(mask2[i] == 0);
        }

        // 33 lights: the lit forms work, the mask is refused
        {
            std::unique_ptr<float[]> many(new float[4 * 33]);
            for (int i = 0; i < 33; ++i) {
                many[4 * i] = 154.0f - 4.0f * i;
                many[4 * i + 1] = 64.0f;
                many[4 * i + 2] = 40.0f;
                many[4 * i + 3] = 1.0f;
            }
            rt_scene bright = s;
            bright.num_lights = 33;
            bright.lights = many.get();
            CHECK(rt_light_hits_shadowed_reflected(hits.get(), &bright, kDir, w, rb, re, 0.25f,
                                                   RT_FORMAT_RGBA8, words.get()) == RT_OK);
            CHECK(rt_shadow_hits_reflected(hits.get(), &bright, kDir, w, rb, re, mask2.get()) ==
                  RT_ERR_UNSUPPORTED);
            bright.num_lights = 32;
            CHECK(rt_shadow_hits_reflected(hits.get(), &bright, kDir, w, rb, re, mask2.get()) ==
                  RT_OK);
        }

        // ---- arguments ----------------------------------------------------------
        CHECK(rt_shadow_hits_reflected(nullptr, &s, kDir, w, rb, re, mask2.get()) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits_reflected(hits.get(), nullptr, kDir, w, rb, re, mask2.get()) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits_reflected(hits.get(), &s, nullptr, w, rb, re, mask2.get()) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits_reflected(hits.get(), &s, kDir, w, rb, re, nullptr) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits_reflected(hits.get(), &s, kDir, 0, rb, re, mask2.get()) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits_reflected(hits.get(), &s, kDir, w, -1, re, mask2.get()) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_shadow_hits_reflected(hits.get(), &s, kDir, w, re, re, mask2.get()) ==
              RT_ERR_INVALID_ARG);
        for (float r : {0.0f, 0.5f}) {
            CHECK(rt_light_hits_shadowed_reflected(hits.get(), &s, kDir, w, rb, re, r, 0,
                                                   nullptr) == RT_ERR_INVALID_ARG);
            CHECK(rt_light_hits_shadowed_reflected(nullptr, &s, kDir, w, rb, re, r, 0, px.get()) ==
                  RT_ERR_INVALID_ARG);
            for (int32_t fmt : {2, (int32_t)RT_FORMAT_HIT, 4, -1})
                CHECK(rt_light_hits_shadowed_reflected(hits.get(), &s, kDir, w, rb, re, r, fmt,
                                                       px.get()) == RT_ERR_INVALID_ARG);
        }
        for (float r : {-0.1f, 1.5f, NAN, INFINITY, -INFINITY, std::nextafter(1.0f, 2.0f)})
            for (int32_t fmt : {(int32_t)RT_FORMAT_I32X4, (int32_t)RT_FORMAT_RGBA8})
                CHECK(rt_light_hits_shadowed_reflected(hits.get(), &s, kDir, w, rb, re, r, fmt,
                                                       px.get()) == RT_ERR_INVALID_ARG);
        rt_scene bad = s;
        bad.lights = nullptr;
        CHECK(rt_shadow_hits_reflected(hits.get(), &bad, kDir, w, rb, re, mask2.get()) ==
              RT_ERR_INVALID_ARG);
        bad = s;
        bad.num_lights = -1;
        CHECK(rt_light_hits_shadowed_reflected(hits.get(), &bad, kDir, w, rb, re, 0.5f, 0,
                                               px.get()) == RT_ERR_INVALID_ARG);
        for (int32_t obj : {4, -2, INT32_MAX, INT32_MIN}) {
            hits[n - 1].object = obj;
            CHECK(rt_shadow_hits_reflected(hits.get(), &s, kDir, w, rb, re, mask2.get()) ==
                  RT_ERR_INVALID_ARG);
            for (float r : {0.0f, 0.5f})
                CHECK(rt_light_hits_shadowed_reflected(hits.get(), &s, kDir, w, rb, re, r, 0,
                                                       px.get()) == RT_ERR_INVALID_ARG);
        }
    }

    // ---- an empty scene with NULL arrays: every pixel a miss -----------------
    {
        rt_scene empty{};
        const int w = 5, rows = 3;
        std::unique_ptr<rt_hit[]> hits(new rt_hit[w * rows]);
        for (int i = 0; i < w * rows; ++i) hits[i] = rt_hit{300000.0f, -1};
        std::unique_ptr<uint32_t[]> mask2(new uint32_t[w * rows]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * w * rows]);
        std::unique_ptr<uint32_t[]> words(new uint32_t[w * rows]);
        for (int with_light = 0; with_light < 2; ++with_light) {
            empty.lights = with_light ? light.get() : nullptr;
            empty.num_lights = with_light;
            CHECK(rt_shadow_hits_reflected(hits.get(), &empty, kDir, w, 0, rows, mask2.get()) ==
                  RT_OK);
            CHECK(rt_light_hits_shadowed_reflected(hits.get(), &empty, kDir, w, 0, rows, 1.0f,
                                                   RT_FORMAT_I32X4, px.get()) == RT_OK);
            CHECK(rt_light_hits_shadowed_reflected(hits.get(), &empty, kDir, w, 0, rows, 0.0f,
                                                   RT_FORMAT_RGBA8, words.get()) == RT_OK);
            for (int i = 0; i < w * rows; ++i) {
                CHECK(mask2[i] == 0 && words[i] == 0xFF000000u);
                CHECK(std::memcmp(&px[4 * i], kBlack, sizeof kBlack) == 0);
            }
        }
        // any object is out of range in an empty scene
        hits[w * rows - 1].object = 0;
        CHECK(rt_shadow_hits_reflected(hits.get(), &empty, kDir, w, 0, rows, mask2.get()) ==
              RT_ERR_INVALID_ARG);
    }
    if (failures) return 1;
    std::printf("shadow reflect args check ok\n");
    return 0;
}
