// shadow_reflect_args_check.cpp -- rt_shadow_hits_reflected /
// rt_light_hits_shadowed_reflected (csrc/rt_light.cpp with csrc/rt_args.cpp) as
// a stand-alone program on tests/light_check.h:
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
#include "light_check.h"

using namespace light_check;

int main() {
    KindsScene kinds;
    const rt_scene& s = kinds.s;
    auto own = [](const Call& c) {
        return rt_shadow_hits_reflected(c.hits, c.scene, c.dir, c.w, c.rb, c.re, (uint32_t*)c.out);
    };
    auto lit_at = [](float r) {
        return [r](const Call& c, int32_t fmt) {
            return rt_light_hits_shadowed_reflected(c.hits, c.scene, c.dir, c.w, c.rb, c.re, r, fmt,
                                                    c.out);
        };
    };
    {
        Band band(true);
        const int w = Band::w, rb = Band::rb, re = Band::re, n = Band::n;
        rt_hit* hits = band.hits.get();
        std::unique_ptr<rt_hit[]> bounce(new rt_hit[n]);
        std::unique_ptr<uint32_t[]> mask(new uint32_t[n]);
        std::unique_ptr<uint32_t[]> mask2(new uint32_t[n]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> full(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> zero(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> shadowed(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> mirrored(new int32_t[4 * n]);
        std::unique_ptr<uint32_t[]> words(new uint32_t[n]);
        CHECK(rt_reflect_hits(hits, &s, kDir, w, rb, re, bounce.get()) == RT_OK);
        CHECK(rt_shadow_hits(hits, &s, kDir, w, rb, re, mask.get()) == RT_OK);
        CHECK(rt_shadow_hits_reflected(hits, &s, kDir, w, rb, re, mask2.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed_reflected(hits, &s, kDir, w, rb, re, 0.25f, RT_FORMAT_I32X4,
                                               px.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed_reflected(hits, &s, kDir, w, rb, re, 1.0f, RT_FORMAT_I32X4,
                                               full.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed_reflected(hits, &s, kDir, w, rb, re, 0.0f, RT_FORMAT_I32X4,
                                               zero.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed_reflected(hits, &s, kDir, w, rb, re, 0.25f, RT_FORMAT_RGBA8,
                                               words.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed(hits, &s, kDir, w, rb, re, RT_FORMAT_I32X4, shadowed.get()) ==
              RT_OK);
        CHECK(rt_light_hits_reflected(hits, &s, kDir, w, rb, re, 0.25f, RT_FORMAT_I32X4,
                                      mirrored.get()) == RT_OK);
        // reflectivity 0: rt_light_hits_shadowed's frame
        CHECK(std::memcmp(zero.get(), shadowed.get(), sizeof(int32_t) * 4 * n) == 0);
        // (118, 64): straight back from z = -50 to the lowest point of sphere 1,
        // whose normal there points down: the light above faces away, k2 = 0
        CHECK(bounce[Band::kUnder].object == 3 && mask2[Band::kUnder] == 0);
        CHECK(is_black(&full[4 * Band::kUnder]));
        // the flank of sphere 0 mirrors down onto the face, which faces the light
        CHECK(bounce[Band::kFlank].object == 0);
        // the miss
        CHECK(mask2[n - 1] == 0 && words[n - 1] == 0xFF000000u);
        CHECK(is_black(&px[4 * (n - 1)]));
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
            CHECK(rt_light_hits_shadowed_reflected(hits, &dark, kDir, w, rb, re, 0.25f,
                                                   RT_FORMAT_I32X4, px.get()) == RT_OK);
            CHECK(rt_light_hits_reflected(hits, &dark, kDir, w, rb, re, 0.25f, RT_FORMAT_I32X4,
                                          mirrored.get()) == RT_OK);
            CHECK(std::memcmp(px.get(), mirrored.get(), sizeof(int32_t) * 4 * n) == 0);
            CHECK(rt_shadow_hits_reflected(hits, &dark, kDir, w, rb, re, mask2.get()) == RT_OK);
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
            CHECK(rt_light_hits_shadowed_reflected(hits, &bright, kDir, w, rb, re, 0.25f,
                                                   RT_FORMAT_RGBA8, words.get()) == RT_OK);
            CHECK(rt_shadow_hits_reflected(hits, &bright, kDir, w, rb, re, mask2.get()) ==
                  RT_ERR_UNSUPPORTED);
            bright.num_lights = 32;
            CHECK(rt_shadow_hits_reflected(hits, &bright, kDir, w, rb, re, mask2.get()) == RT_OK);
        }

        // ---- arguments ----------------------------------------------------------
        refusals(own, Call{hits, &s, kDir, w, rb, re, mask2.get()}, &hits[n - 1],
                 KindsScene::slots);
        reflectivity_refusals(lit_at, Call{hits, &s, kDir, w, rb, re, px.get()}, &hits[n - 1],
                              KindsScene::slots);
    }
    empty_scene<uint32_t>(
        kinds.light.get(), own,
        [&](const Call& c, int32_t fmt) {
            return lit_at(fmt == RT_FORMAT_RGBA8 ? 0.0f : 1.0f)(c, fmt);
        },
        [](uint32_t m) { return m == 0u; });
    return finish("shadow reflect");
}
