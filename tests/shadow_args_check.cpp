// shadow_args_check.cpp -- rt_shadow_hits / rt_light_hits_shadowed
// (csrc/rt_light.cpp with csrc/rt_args.cpp) as a stand-alone program on
// tests/light_check.h: tests/test_shadow_hits.py builds it with
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
#include "light_check.h"

using namespace light_check;

int main() {
    KindsScene kinds;
    const rt_scene& s = kinds.s;
    auto own = [](const Call& c) {
        return rt_shadow_hits(c.hits, c.scene, c.dir, c.w, c.rb, c.re, (uint32_t*)c.out);
    };
    auto lit = [](const Call& c, int32_t fmt) {
        return rt_light_hits_shadowed(c.hits, c.scene, c.dir, c.w, c.rb, c.re, fmt, c.out);
    };
    {
        Band band(false);
        const int w = Band::w, rb = Band::rb, re = Band::re, n = Band::n;
        rt_hit* hits = band.hits.get();
        std::unique_ptr<uint32_t[]> mask(new uint32_t[n]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> plain(new int32_t[4 * n]);
        std::unique_ptr<uint32_t[]> words(new uint32_t[n]);
        CHECK(rt_shadow_hits(hits, &s, kDir, w, rb, re, mask.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed(hits, &s, kDir, w, rb, re, RT_FORMAT_I32X4, px.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed(hits, &s, kDir, w, rb, re, RT_FORMAT_RGBA8, words.get()) ==
              RT_OK);
        CHECK(rt_light_hits(hits, &s, kDir, w, rb, re, RT_FORMAT_I32X4, plain.get()) == RT_OK);
        // (38, 64): the segment to the light passes the centre of sphere 0
        CHECK(mask[Band::kBehind] == 1u);
        CHECK(is_black(&px[4 * Band::kBehind]));
        CHECK(words[Band::kBehind] == 0xFF000000u);
        CHECK(plain[4 * Band::kBehind] > 0);
        // (5, 60) sees the light
        CHECK(mask[Band::kSees] == 0u && px[4 * Band::kSees] > 0);
        CHECK(std::memcmp(&px[4 * Band::kSees], &plain[4 * Band::kSees], 16) == 0);
        // the pole of sphere 0: behind the box
        CHECK(mask[Band::kPole] == 1u && plain[4 * Band::kPole] > 0);
        CHECK(is_black(&px[4 * Band::kPole]));
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
        CHECK(rt_shadow_hits(hits, &m, kDir, w, rb, re, mask.get()) == RT_ERR_UNSUPPORTED);
        CHECK(rt_light_hits_shadowed(hits, &m, kDir, w, rb, re, RT_FORMAT_I32X4, px.get()) == RT_OK);
        CHECK(rt_light_hits_shadowed(hits, &m, kDir, w, rb, re, RT_FORMAT_RGBA8, words.get()) ==
              RT_OK);
        m.num_lights = 32;
        std::unique_ptr<float[]> many32(new float[4 * 32]);
        std::memcpy(many32.get(), many.get(), sizeof(float) * 4 * 32);
        m.lights = many32.get();
        CHECK(rt_shadow_hits(hits, &m, kDir, w, rb, re, mask.get()) == RT_OK);
        CHECK((mask[Band::kBehind] & 1u) == 1u);

        // ---- arguments ----------------------------------------------------------
        refusals(own, Call{hits, &s, kDir, w, rb, re, mask.get()}, &hits[n - 1], KindsScene::slots);
        const Call to_px{hits, &s, kDir, w, rb, re, px.get()};
        refused_formats(lit, to_px);
        refusals([&](const Call& c) { return lit(c, 0); }, to_px, &hits[n - 1], KindsScene::slots);
    }
    empty_scene<uint32_t>(kinds.light.get(), own, lit, [](uint32_t m) { return m == 0u; });
    return finish("shadow");
}
