// mirror_args_check.cpp -- rt_bounce_hits / rt_light_hits_mirrored
// (csrc/rt_light.cpp with csrc/rt_args.cpp) as a stand-alone program on
// tests/light_check.h: tests/test_mirror_hits.py builds it with
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
#include "light_check.h"

using namespace light_check;

int main() {
    KindsScene kinds;
    const rt_scene& s = kinds.s;
    const int slots = KindsScene::slots;
    // the face and the unseen sphere are mirrors, sphere 0 mirrors a quarter,
    // the box is matte
    std::unique_ptr<float[]> refl(new float[slots]{1.0f, 0.0f, 0.25f, 1.0f});
    auto bounce_at = [](int32_t b) {
        return [b](const Call& c) {
            return rt_bounce_hits(c.hits, c.scene, c.dir, c.w, c.rb, c.re, b, (rt_hit*)c.out);
        };
    };
    auto lit_at = [](const float* array, int32_t depth, int32_t shadows) {
        return [=](const Call& c, int32_t fmt) {
            return rt_light_hits_mirrored(c.hits, c.scene, c.dir, c.w, c.rb, c.re, array, depth,
                                          shadows, fmt, c.out);
        };
    };
    {
        Band band(true);
        const int w = Band::w, rb = Band::rb, re = Band::re, n = Band::n;
        rt_hit* hits = band.hits.get();
        std::unique_ptr<rt_hit[]> first(new rt_hit[n]);
        std::unique_ptr<rt_hit[]> bounce(new rt_hit[n]);
        std::unique_ptr<rt_hit[]> reflect(new rt_hit[n]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> other(new int32_t[4 * n]);
        std::unique_ptr<uint32_t[]> words(new uint32_t[n]);
        std::unique_ptr<uint32_t[]> words2(new uint32_t[n]);

        // the bounce frames: 1 is rt_reflect_hits', a later one misses where an earlier did
        CHECK(rt_reflect_hits(hits, &s, kDir, w, rb, re, reflect.get()) == RT_OK);
        CHECK(rt_bounce_hits(hits, &s, kDir, w, rb, re, 1, first.get()) == RT_OK);
        CHECK(std::memcmp(first.get(), reflect.get(), sizeof(rt_hit) * n) == 0);
        // (118, 64): the face, straight back into the lowest point of sphere 1, and
        // from there straight back onto the face: the primary object is a candidate again
        CHECK(first[Band::kUnder].object == 3 && first[Band::kUnder].t == 58.0f);
        CHECK(rt_bounce_hits(hits, &s, kDir, w, rb, re, 2, bounce.get()) == RT_OK);
        CHECK(bounce[Band::kUnder].object == 0 && bounce[Band::kUnder].t == 58.0f);
        int second = 0;
        for (int i = 0; i < n; ++i) {
            if (first[i].object < 0) CHECK(is_miss(bounce[i]));
            second += bounce[i].object >= 0;
        }
        CHECK(second > 0);
        for (int32_t b = 1; b <= RT_MAX_BOUNCES; ++b) {
            CHECK(rt_bounce_hits(hits, &s, kDir, w, rb, re, b, bounce.get()) == RT_OK);
            CHECK(is_miss(bounce[n - 1]));                                // the miss
            CHECK(bounce[Band::kUnder].object == (b % 2 ? 3 : 0));        // to and fro
        }
        for (int32_t b : {0, -1, RT_MAX_BOUNCES + 1, INT32_MAX, INT32_MIN})
            CHECK(rt_bounce_hits(hits, &s, kDir, w, rb, re, b, bounce.get()) ==
                  RT_ERR_INVALID_ARG);

        // every depth, shadows off and on, both formats; the miss stays black
        for (int32_t depth = 0; depth <= RT_MAX_BOUNCES; ++depth)
            for (int32_t shadows = 0; shadows < 2; ++shadows) {
                CHECK(rt_light_hits_mirrored(hits, &s, kDir, w, rb, re, refl.get(), depth, shadows,
                                             RT_FORMAT_I32X4, px.get()) == RT_OK);
                CHECK(rt_light_hits_mirrored(hits, &s, kDir, w, rb, re, refl.get(), depth, shadows,
                                             RT_FORMAT_RGBA8, words.get()) == RT_OK);
                CHECK(is_black(&px[4 * (n - 1)]));
                CHECK(words[n - 1] == 0xFF000000u);
                for (int i = 0; i < n; ++i) CHECK(px[4 * i + 3] == 255 && (words[i] >> 24) == 0xFFu);
            }
        // the second bounce shows at (118, 64), and nowhere the first bounce missed
        CHECK(rt_light_hits_mirrored(hits, &s, kDir, w, rb, re, refl.get(), 1, 1, RT_FORMAT_I32X4,
                                     px.get()) == RT_OK);
        CHECK(rt_light_hits_mirrored(hits, &s, kDir, w, rb, re, refl.get(), 2, 1, RT_FORMAT_I32X4,
                                     other.get()) == RT_OK);
        CHECK(std::memcmp(&px[4 * Band::kUnder], &other[4 * Band::kUnder], 16) != 0);
        for (int i = 0; i < n; ++i)
            if (first[i].object < 0) CHECK(std::memcmp(&px[4 * i], &other[4 * i], 16) == 0);

        // one bounce, one reflectivity everywhere: the one-bounce functions' frames
        for (float r : {0.25f, 1.0f, 0.0f, -0.0f}) {
            std::unique_ptr<float[]> uniform(new float[slots]{r, r, r, r});
            CHECK(rt_light_hits_mirrored(hits, &s, kDir, w, rb, re, uniform.get(), 1, 0,
                                         RT_FORMAT_I32X4, px.get()) == RT_OK);
            CHECK(rt_light_hits_reflected(hits, &s, kDir, w, rb, re, r, RT_FORMAT_I32X4,
                                          other.get()) == RT_OK);
            CHECK(std::memcmp(px.get(), other.get(), sizeof(int32_t) * 4 * n) == 0);
            CHECK(rt_light_hits_mirrored(hits, &s, kDir, w, rb, re, uniform.get(), 1, 1,
                                         RT_FORMAT_RGBA8, words.get()) == RT_OK);
            CHECK(rt_light_hits_shadowed_reflected(hits, &s, kDir, w, rb, re, r, RT_FORMAT_RGBA8,
                                                   words2.get()) == RT_OK);
            CHECK(std::memcmp(words.get(), words2.get(), sizeof(uint32_t) * n) == 0);
        }
        // no bounce: rt_light_hits' and rt_light_hits_shadowed's frames, the array NULL or not
        for (int32_t shadows = 0; shadows < 2; ++shadows) {
            if (shadows)
                CHECK(rt_light_hits_shadowed(hits, &s, kDir, w, rb, re, RT_FORMAT_I32X4,
                                             other.get()) == RT_OK);
            else
                CHECK(rt_light_hits(hits, &s, kDir, w, rb, re, RT_FORMAT_I32X4, other.get()) ==
                      RT_OK);
            for (const float* array : {(const float*)nullptr, (const float*)refl.get()}) {
                CHECK(rt_light_hits_mirrored(hits, &s, kDir, w, rb, re, array, 0, shadows,
                                             RT_FORMAT_I32X4, px.get()) == RT_OK);
                CHECK(std::memcmp(px.get(), other.get(), sizeof(int32_t) * 4 * n) == 0);
            }
            std::unique_ptr<float[]> zeros(new float[slots]{0.0f, -0.0f, 0.0f, -0.0f});
            CHECK(rt_light_hits_mirrored(hits, &s, kDir, w, rb, re, zeros.get(), 8, shadows,
                                         RT_FORMAT_I32X4, px.get()) == RT_OK);
            CHECK(std::memcmp(px.get(), other.get(), sizeof(int32_t) * 4 * n) == 0);
        }

        // ---- arguments ----------------------------------------------------------
        const Call to_px{hits, &s, kDir, w, rb, re, px.get()};
        // a scene with objects, a depth: the array is needed
        CHECK(lit_at(nullptr, 1, 0)(to_px, 0) == RT_ERR_INVALID_ARG);
        for (int32_t depth : {-1, RT_MAX_BOUNCES + 1, INT32_MAX, INT32_MIN})
            CHECK(lit_at(refl.get(), depth, 0)(to_px, 0) == RT_ERR_INVALID_ARG);
        for (int32_t shadows : {-1, 2, INT32_MAX})
            CHECK(lit_at(refl.get(), 1, shadows)(to_px, 0) == RT_ERR_INVALID_ARG);
        for (float r : {-0.1f, 1.5f, NAN, INFINITY, -INFINITY, std::nextafter(1.0f, 2.0f)})
            for (int slot : {0, 1, slots - 1}) {
                std::unique_ptr<float[]> bad(new float[slots]{1.0f, 0.0f, 0.25f, 1.0f});
                bad[slot] = r;
                for (int32_t fmt : {(int32_t)RT_FORMAT_I32X4, (int32_t)RT_FORMAT_RGBA8})
                    CHECK(lit_at(bad.get(), 2, 1)(to_px, fmt) == RT_ERR_INVALID_ARG);
            }
        for (int32_t depth : {0, 2}) {
            auto lit = lit_at(refl.get(), depth, 0);
            refused_formats(lit, to_px);
            refusals([&](const Call& c) { return lit(c, 0); }, to_px, &hits[n - 1], slots);
        }
        for (int32_t b : {1, 2})
            refusals(bounce_at(b), Call{hits, &s, kDir, w, rb, re, bounce.get()}, &hits[n - 1],
                     slots);
    }
    empty_scene<rt_hit>(
        kinds.light.get(), bounce_at(8),
        [&](const Call& c, int32_t fmt) {
            return fmt == RT_FORMAT_RGBA8 ? lit_at(nullptr, 0, 0)(c, fmt)
                                          : lit_at(nullptr, 8, 1)(c, fmt);
        },
        [](const rt_hit& h) { return is_miss(h); });
    return finish("mirror");
}
