// mirror_args_check.cpp -- rt_bounce_hits / rt_light_hits_mirrored
// (csrc/rt_light.cpp with csrc/rt_args.cpp) as a stand-alone program like
// shadow_reflect_args_check.cpp: tests/test_mirror_hits.py builds it with
// -fsanitize=address,undefined and runs it.  No GPU.
//
//   - exactly-sized heap arrays for the frame, the scene, the reflectivity
//     array and every output (an overrun on either side is reported);
//   - the face, the box and the two spheres of the shadow term's scene, a
//     band of it: the face under the unseen sphere is thrown straight back
//     into it and from it straight back onto the face, to and fro up to the
//     cap; the identities with rt_reflect_hits,
//     rt_light_hits_reflected, rt_light_hits_shadowed_reflected,
//     rt_light_hits and rt_light_hits_shadowed;
//   - an empty scene with NULL arrays, the reflectivity array among them;
//   - every depth and bounce number, and the refused ones; the refused
//     reflectivities; the argument checks.
// Exit 0 and "mirror args check ok" on success.
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
    const int slots = 4;
    // the face and the unseen sphere are mirrors, sphere 0 mirrors a quarter,
    // the box is matte
    std::unique_ptr<float[]> refl(new float[slots]{1.0f, 0.0f, 0.25f, 1.0f});

    // rows 60..67 of the 128-wide frame, every pixel on the face (t = 50) but
    // (64, 64), the pole of sphere 0 (t = 18), (75, 64) on its flank and a miss
    {
        const int w = 128, rb = 60, re = 68, n = w * (re - rb);
        std::unique_ptr<rt_hit[]> hits(new rt_hit[n]);
        for (int i = 0; i < n; ++i) hits[i] = rt_hit{50.0f, 0};
        hits[4 * w + 64] = rt_hit{18.0f, 2};
        hits[4 * w + 75] = rt_hit{30.0f - std::sqrt(23.0f), 2};
        hits[7 * w + 127] = rt_hit{300000.0f, -1};
        std::unique_ptr<rt_hit[]> first(new rt_hit[n]);
        std::unique_ptr<rt_hit[]> bounce(new rt_hit[n]);
        std::unique_ptr<rt_hit[]> reflect(new rt_hit[n]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> other(new int32_t[4 * n]);
        std::unique_ptr<uint32_t[]> words(new uint32_t[n]);
        std::unique_ptr<uint32_t[]> words2(new uint32_t[n]);

        // the bounce frames: 1 is rt_reflect_hits', a later one misses where an earlier did
        CHECK(rt_reflect_hits(hits.get(), &s, kDir, w, rb, re, reflect.get()) == RT_OK);
        CHECK(rt_bounce_hits(hits.get(), &s, kDir, w, rb, re, 1, first.get()) == RT_OK);
        CHECK(std::memcmp(first.get(), reflect.get(), sizeof(rt_hit) * n) == 0);
        // (118, 64): the face, straight back into the lowest point of sphere 1, and
        // from there straight back onto the face: the primary object is a candidate again
        CHECK(first[4 * w + 118].object == 3 && first[4 * w + 118].t == 58.0f);
        CHECK(rt_bounce_hits(hits.get(), &s, kDir, w, rb, re, 2, bounce.get()) == RT_OK);
        CHECK(bounce[4 * w + 118].object == 0 && bounce[4 * w + 118].t == 58.0f);
        int second = 0;
        for (int i = 0; i < n; ++i) {
            if (first[i].object < 0) CHECK(bounce[i].object == -1 && bounce[i].t == 300000.0f);
            second += bounce[i].object >= 0;
        }
        CHECK(second > 0);
        for (int32_t b = 1; b <= RT_MAX_BOUNCES; ++b) {
            CHECK(rt_bounce_hits(hits.get(), &s, kDir, w, rb, re, b, bounce.get()) == RT_OK);
            CHECK(bounce[n - 1].object == -1 && bounce[n - 1].t == 300000.0f);  // the miss
            CHECK(bounce[4 * w + 118].object == (b % 2 ? 3 : 0));                // to and fro
        }
        for (int32_t b : {0, -1, RT_MAX_BOUNCES + 1, INT32_MAX, INT32_MIN})
            CHECK(rt_bounce_hits(hits.get(), &s, kDir, w, rb, re, b, bounce.get()) ==
                  RT_ERR_INVALID_ARG);

        // every depth, shadows off and on, both formats; the miss stays black
        for (int32_t depth = 0; depth <= RT_MAX_BOUNCES; ++depth)
            for (int32_t shadows = 0; shadows < 2; ++shadows) {
                CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, refl.get(), depth,
                                             shadows, RT_FORMAT_I32X4, px.get()) == RT_OK);
                CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, refl.get(), depth,
                                             shadows, RT_FORMAT_RGBA8, words.get()) == RT_OK);
                CHECK(std::memcmp(&px[4 * (n - 1)], kBlack, sizeof kBlack) == 0);
                CHECK(words[n - 1] == 0xFF000000u);
                for (int i = 0; i < n; ++i) CHECK(px[4 * i + 3] == 255 && (words[i] >> 24) == 0xFFu);
            }
        // the second bounce shows at (118, 64), and nowhere the first bounce missed
        CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, refl.get(), 1, 1,
                                     RT_FORMAT_I32X4, px.get()) == RT_OK);
        CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, refl.get(), 2, 1,
                                     RT_FORMAT_I32X4, other.get()) == RT_OK);
        CHECK(std::memcmp(&px[4 * (4 * w + 118)], &other[4 * (4 * w + 118)], 16) != 0);
        for (int i = 0; i < n; ++i)
            if (first[i].object < 0) CHECK(std::memcmp(&px[4 * i], &other[4 * i], 16) == 0);

        // one bounce, one reflectivity everywhere: the one-bounce functions' frames
        for (float r : {0.25f, 1.0f, 0.0f, -0.0f}) {
            std::unique_ptr<float[]> uniform(new float[slots]{r, r, r, r});
            CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, uniform.get(), 1, 0,
                                         RT_FORMAT_I32X4, px.get()) == RT_OK);
            CHECK(rt_light_hits_reflected(hits.get(), &s, kDir, w, rb, re, r, RT_FORMAT_I32X4,
                                          other.get()) == RT_OK);
            CHECK(std::memcmp(px.get(), other.get(), sizeof(int32_t) * 4 * n) == 0);
            CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, uniform.get(), 1, 1,
                                         RT_FORMAT_RGBA8, words.get()) == RT_OK);
            CHECK(rt_light_hits_shadowed_reflected(hits.get(), &s, kDir, w, rb, re, r,
                                                   RT_FORMAT_RGBA8, words2.get()) == RT_OK);
            CHECK(std::memcmp(words.get(), words2.get(), sizeof(uint32_t) * n) == 0);
        }
        // no bounce: rt_light_hits' and rt_light_hits_shadowed's frames, the array NULL or not
        for (int32_t shadows = 0; shadows < 2; ++shadows) {
            if (shadows)
                CHECK(rt_light_hits_shadowed(hits.get(), &s, kDir, w, rb, re, RT_FORMAT_I32X4,
                                             other.get()) == RT_OK);
            else
                CHECK(rt_light_hits(hits.get(), &s, kDir, w, rb, re, RT_FORMAT_I32X4,
                                    other.get()) == RT_OK);
            for (const float* array : {(const float*)nullptr, (const float*)refl.get()}) {
                CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, array, 0, shadows,
                                             RT_FORMAT_I32X4, px.get()) == RT_OK);
                CHECK(std::memcmp(px.get(), other.get(), sizeof(int32_t) * 4 * n) == 0);
            }
            std::unique_ptr<float[]> zeros(new float[slots]{0.0f, -0.0f, 0.0f, -0.0f});
            CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, zeros.get(), 8, shadows,
                                         RT_FORMAT_I32X4, px.get()) == RT_OK);
            CHECK(std::memcmp(px.get(), other.get(), sizeof(int32_t) * 4 * n) == 0);
        }

        // ---- arguments ----------------------------------------------------------
        CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, nullptr, 1, 0, 0, px.get()) ==
              RT_ERR_INVALID_ARG);  // a scene with objects, a depth: the array is needed
        for (int32_t depth : {-1, RT_MAX_BOUNCES + 1, INT32_MAX, INT32_MIN})
            CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, refl.get(), depth, 0, 0,
                                         px.get()) == RT_ERR_INVALID_ARG);
        for (int32_t shadows : {-1, 2, INT32_MAX})
            CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, refl.get(), 1, shadows, 0,
                                         px.get()) == RT_ERR_INVALID_ARG);
        for (int32_t fmt : {2, (int32_t)RT_FORMAT_HIT, 4, -1})
            for (int32_t depth : {0, 2})
                CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, refl.get(), depth, 0,
                                             fmt, px.get()) == RT_ERR_INVALID_ARG);
        for (float r : {-0.1f, 1.5f, NAN, INFINITY, -INFINITY, std::nextafter(1.0f, 2.0f)})
            for (int slot : {0, 1, slots - 1}) {
                std::unique_ptr<float[]> bad(new float[slots]{1.0f, 0.0f, 0.25f, 1.0f});
                bad[slot] = r;
                for (int32_t fmt : {(int32_t)RT_FORMAT_I32X4, (int32_t)RT_FORMAT_RGBA8})
                    CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, bad.get(), 2, 1,
                                                 fmt, px.get()) == RT_ERR_INVALID_ARG);
            }
        CHECK(rt_light_hits_mirrored(nullptr, &s, kDir, w, rb, re, refl.get(), 2, 0, 0, px.get()) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_light_hits_mirrored(hits.get(), nullptr, kDir, w, rb, re, refl.get(), 2, 0, 0,
                                     px.get()) == RT_ERR_INVALID_ARG);
        CHECK(rt_light_hits_mirrored(hits.get(), &s, nullptr, w, rb, re, refl.get(), 2, 0, 0,
                                     px.get()) == RT_ERR_INVALID_ARG);
        CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, refl.get(), 2, 0, 0,
                                     nullptr) == RT_ERR_INVALID_ARG);
        CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, 0, rb, re, refl.get(), 2, 0, 0,
                                     px.get()) == RT_ERR_INVALID_ARG);
        CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, re, re, refl.get(), 2, 0, 0,
                                     px.get()) == RT_ERR_INVALID_ARG);
        CHECK(rt_bounce_hits(nullptr, &s, kDir, w, rb, re, 1, bounce.get()) == RT_ERR_INVALID_ARG);
        CHECK(rt_bounce_hits(hits.get(), nullptr, kDir, w, rb, re, 1, bounce.get()) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_bounce_hits(hits.get(), &s, nullptr, w, rb, re, 1, bounce.get()) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_bounce_hits(hits.get(), &s, kDir, w, rb, re, 1, nullptr) == RT_ERR_INVALID_ARG);
        CHECK(rt_bounce_hits(hits.get(), &s, kDir, w, -1, re, 1, bounce.get()) ==
              RT_ERR_INVALID_ARG);
        rt_scene bad = s;
        bad.lights = nullptr;
        CHECK(rt_light_hits_mirrored(hits.get(), &bad, kDir, w, rb, re, refl.get(), 2, 0, 0,
                                     px.get()) == RT_ERR_INVALID_ARG);
        bad = s;
        bad.num_spheres = -1;
        CHECK(rt_light_hits_mirrored(hits.get(), &bad, kDir, w, rb, re, refl.get(), 2, 0, 0,
                                     px.get()) == RT_ERR_INVALID_ARG);
        for (int32_t obj : {4, -2, INT32_MAX, INT32_MIN}) {
            hits[n - 1].object = obj;
            CHECK(rt_bounce_hits(hits.get(), &s, kDir, w, rb, re, 2, bounce.get()) ==
                  RT_ERR_INVALID_ARG);
            for (int32_t depth : {0, 2})
                CHECK(rt_light_hits_mirrored(hits.get(), &s, kDir, w, rb, re, refl.get(), depth, 0,
                                             0, px.get()) == RT_ERR_INVALID_ARG);
        }
    }

    // ---- an empty scene with NULL arrays: every pixel a miss -----------------
    {
        rt_scene empty{};
        const int w = 5, rows = 3;
        std::unique_ptr<rt_hit[]> hits(new rt_hit[w * rows]);
        for (int i = 0; i < w * rows; ++i) hits[i] = rt_hit{300000.0f, -1};
        std::unique_ptr<rt_hit[]> bounce(new rt_hit[w * rows]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * w * rows]);
        std::unique_ptr<uint32_t[]> words(new uint32_t[w * rows]);
        for (int with_light = 0; with_light < 2; ++with_light) {
            empty.lights = with_light ? light.get() : nullptr;
            empty.num_lights = with_light;
            CHECK(rt_bounce_hits(hits.get(), &empty, kDir, w, 0, rows, 8, bounce.get()) == RT_OK);
            CHECK(rt_light_hits_mirrored(hits.get(), &empty, kDir, w, 0, rows, nullptr, 8, 1,
                                         RT_FORMAT_I32X4, px.get()) == RT_OK);
            CHECK(rt_light_hits_mirrored(hits.get(), &empty, kDir, w, 0, rows, nullptr, 0, 0,
                                         RT_FORMAT_RGBA8, words.get()) == RT_OK);
            for (int i = 0; i < w * rows; ++i) {
                CHECK(bounce[i].object == -1 && bounce[i].t == 300000.0f);
                CHECK(words[i] == 0xFF000000u);
                CHECK(std::memcmp(&px[4 * i], kBlack, sizeof kBlack) == 0);
            }
        }
        // any object is out of range in an empty scene
        hits[w * rows - 1].object = 0;
        CHECK(rt_bounce_hits(hits.get(), &empty, kDir, w, 0, rows, 1, bounce.get()) ==
              RT_ERR_INVALID_ARG);
        CHECK(rt_light_hits_mirrored(hits.get(), &empty, kDir, w, 0, rows, nullptr, 1, 0, 0,
                                     px.get()) == RT_ERR_INVALID_ARG);
    }
    if (failures) return 1;
    std::printf("mirror args check ok\n");
    return 0;
}
