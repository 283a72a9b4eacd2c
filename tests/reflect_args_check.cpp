// reflect_args_check.cpp -- rt_reflect_hits / rt_light_hits_reflected
// (csrc/rt_light.cpp with csrc/rt_args.cpp) as a stand-alone program on
// tests/light_check.h: tests/test_reflect_hits.py builds it with
// -fsanitize=address,undefined and runs it.  No GPU.
//
//   - exactly-sized heap arrays for the frame, the scene and every output
//     (an overrun on either side is reported);
//   - the face, the box and the two spheres of the shadow term's scene, a
//     band of it, known pixels: the face under the unseen sphere, a face pixel
//     that mirrors nothing, the pole and the rim of sphere 0, a miss;
//   - an empty scene with NULL arrays, with and without lights;
//   - reflectivity 0, 0.25 and 1, and the refused ones;
//   - the argument checks.
// Exit 0 and "reflect args check ok" on success.
#include "light_check.h"

using namespace light_check;

int main() {
    KindsScene kinds;
    const rt_scene& s = kinds.s;
    auto own = [](const Call& c) {
        return rt_reflect_hits(c.hits, c.scene, c.dir, c.w, c.rb, c.re, (rt_hit*)c.out);
    };
    auto lit_at = [](float r) {
        return [r](const Call& c, int32_t fmt) {
            return rt_light_hits_reflected(c.hits, c.scene, c.dir, c.w, c.rb, c.re, r, fmt, c.out);
        };
    };
    {
        Band band(true);
        const int w = Band::w, rb = Band::rb, re = Band::re, n = Band::n;
        rt_hit* hits = band.hits.get();
        std::unique_ptr<rt_hit[]> bounce(new rt_hit[n]);
        std::unique_ptr<int32_t[]> px(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> full(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> plain(new int32_t[4 * n]);
        std::unique_ptr<int32_t[]> zero(new int32_t[4 * n]);
        std::unique_ptr<uint32_t[]> words(new uint32_t[n]);
        CHECK(rt_reflect_hits(hits, &s, kDir, w, rb, re, bounce.get()) == RT_OK);
        CHECK(rt_light_hits_reflected(hits, &s, kDir, w, rb, re, 0.25f, RT_FORMAT_I32X4,
                                      px.get()) == RT_OK);
        CHECK(rt_light_hits_reflected(hits, &s, kDir, w, rb, re, 1.0f, RT_FORMAT_I32X4,
                                      full.get()) == RT_OK);
        CHECK(rt_light_hits_reflected(hits, &s, kDir, w, rb, re, 0.0f, RT_FORMAT_I32X4,
                                      zero.get()) == RT_OK);
        CHECK(rt_light_hits_reflected(hits, &s, kDir, w, rb, re, 0.25f, RT_FORMAT_RGBA8,
                                      words.get()) == RT_OK);
        CHECK(rt_light_hits(hits, &s, kDir, w, rb, re, RT_FORMAT_I32X4, plain.get()) == RT_OK);
        // reflectivity 0: rt_light_hits' frame
        CHECK(std::memcmp(zero.get(), plain.get(), sizeof(int32_t) * 4 * n) == 0);
        // (118, 64): straight back from z = -50 to the lowest point of sphere 1, z = 8
        CHECK(bounce[Band::kUnder].object == 3 && bounce[Band::kUnder].t == 58.0f);
        CHECK(std::memcmp(&px[4 * Band::kUnder], &plain[4 * Band::kUnder], 16) != 0);
        // (5, 60) mirrors nothing: a + r * (0 - a)
        CHECK(is_miss(bounce[Band::kSees]) && plain[4 * Band::kSees] > 0);
        CHECK(px[4 * Band::kSees] > 0 && px[4 * Band::kSees] < plain[4 * Band::kSees]);
        CHECK(is_black(&full[4 * Band::kSees]));
        // the pole of sphere 0 mirrors straight back, past everything
        CHECK(is_miss(bounce[Band::kPole]));
        // its flank mirrors down onto the face
        CHECK(bounce[Band::kFlank].object == 0 && bounce[Band::kFlank].t > 20.0f &&
              bounce[Band::kFlank].t < 100.0f);
        // the miss
        CHECK(is_miss(bounce[n - 1]) && words[n - 1] == 0xFF000000u);
        CHECK(is_black(&px[4 * (n - 1)]));
        for (int i = 0; i < n; ++i) {
            CHECK(bounce[i].object >= -1 && bounce[i].object < 4);
            CHECK(hits[i].object < 0 || bounce[i].object != hits[i].object);
            CHECK(px[4 * i + 3] == 255 && (words[i] >> 24) == 0xFFu);
        }

        // ---- arguments ----------------------------------------------------------
        refusals(own, Call{hits, &s, kDir, w, rb, re, bounce.get()}, &hits[n - 1],
                 KindsScene::slots);
        reflectivity_refusals(lit_at, Call{hits, &s, kDir, w, rb, re, px.get()}, &hits[n - 1],
                              KindsScene::slots);
    }
    empty_scene<rt_hit>(
        kinds.light.get(), own,
        [&](const Call& c, int32_t fmt) {
            return lit_at(fmt == RT_FORMAT_RGBA8 ? 0.0f : 1.0f)(c, fmt);
        },
        [](const rt_hit& h) { return is_miss(h); });
    return finish("reflect");
}
