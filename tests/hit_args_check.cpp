// hit_args_check.cpp -- RT_FORMAT_HIT through the host half of the C ABI
// (csrc/rt_args.cpp, csrc/rt_scene.cpp), as a stand-alone program like
// tests/asan/rt_asan_check.cpp: tests/test_hit_format.py builds it with
// -fsanitize=address,undefined next to those two sources and runs it.  No GPU.
//
//   - check_args / check_reserve accept format 3 and still reject 2 and 4;
//   - pixel_bytes / frame_bytes of the three formats;
//   - rt_shade_hits on exactly-sized heap arrays (an overrun is reported):
//     both output formats, a miss, an object out of range on either side.
// Exit 0 and "hit args check ok" on success.
#include <cstdint>
#include <cstdio>
#include <memory>

#include "rt_args.h"
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

}  // namespace

int main() {
    static_assert(RT_FORMAT_HIT == 3, "the value is part of the ABI");
    static_assert(sizeof(rt_hit) == 8, "two 32-bit words per pixel");
    rt_scene empty{};
    using rt_args::check_args;
    using rt_args::check_reserve;
    CHECK(check_args(&empty, 8, 8, 0, 8, RT_FORMAT_HIT) == RT_OK);
    CHECK(check_args(&empty, 8, 8, 0, 8, 2) == RT_ERR_INVALID_ARG);
    CHECK(check_args(&empty, 8, 8, 0, 8, 4) == RT_ERR_INVALID_ARG);
    CHECK(check_args(&empty, 8, 8, 0, 8, -1) == RT_ERR_INVALID_ARG);
    CHECK(check_reserve(640, 480, 3, 2, RT_FORMAT_HIT) == RT_OK);
    CHECK(check_reserve(640, 480, 3, 2, 2) == RT_ERR_INVALID_ARG);
    CHECK(check_reserve(640, 480, 3, 2, 4) == RT_ERR_INVALID_ARG);
    CHECK(rt_args::pixel_bytes(RT_FORMAT_I32X4) == 16);
    CHECK(rt_args::pixel_bytes(RT_FORMAT_RGBA8) == 4);
    CHECK(rt_args::pixel_bytes(RT_FORMAT_HIT) == 8);
    CHECK(rt_args::frame_bytes(3, 2, RT_FORMAT_HIT) == 48);
    CHECK(rt_args::frame_bytes(3, 2, RT_FORMAT_RGBA8) == 24);
    CHECK(rt_args::frame_bytes(1 << 14, 1 << 14, RT_FORMAT_HIT) == (size_t)1 << 31);

    // rt_shade_hits: one cube (slot 0), two spheres (slots 1, 2)
    std::unique_ptr<float[]> cube_col(new float[4]{1.0f, 0.5f, 0.25f, 255.0f});
    std::unique_ptr<float[]> sph_col(new float[8]{0.5f, 0.5f, 0.5f, 255.0f, 0.0f, 1.0f, 2.0f, 255.0f});
    rt_scene s{};
    s.num_cubes = 1;
    s.cube_colours = cube_col.get();
    s.num_spheres = 2;
    s.sphere_colours = sph_col.get();
    std::unique_ptr<rt_hit[]> hits(new rt_hit[4]{{90.0f, 0}, {300000.0f, -1}, {0.0f, 2}, {180.0f, 1}});
    std::unique_ptr<int32_t[]> px(new int32_t[16]);
    std::unique_ptr<uint32_t[]> words(new uint32_t[4]);
    CHECK(rt_shade_hits(hits.get(), 4, &s, RT_FORMAT_I32X4, px.get()) == RT_OK);
    // t = 90: scalar 127.5; the miss; t = 0: scalar 255; t = 180: scalar 0
    const int32_t want[16] = {127, 63, 31, 255, 0, 0, 0, 255, 0, 255, 510, 255, 0, 0, 0, 255};
    for (int i = 0; i < 16; ++i) CHECK(px[i] == want[i]);
    CHECK(rt_shade_hits(hits.get(), 4, &s, RT_FORMAT_RGBA8, words.get()) == RT_OK);
    CHECK(words[0] == 0xFF1F3F7Fu && words[1] == 0xFF000000u && words[2] == 0xFFFEFF00u);
    CHECK(rt_shade_hits(hits.get(), 0, &s, RT_FORMAT_I32X4, px.get()) == RT_OK);
    CHECK(rt_shade_hits(hits.get(), 4, &s, RT_FORMAT_HIT, px.get()) == RT_ERR_INVALID_ARG);
    CHECK(rt_shade_hits(hits.get(), 4, &s, 2, px.get()) == RT_ERR_INVALID_ARG);
    CHECK(rt_shade_hits(nullptr, 4, &s, RT_FORMAT_I32X4, px.get()) == RT_ERR_INVALID_ARG);
    CHECK(rt_shade_hits(hits.get(), -1, &s, RT_FORMAT_I32X4, px.get()) == RT_ERR_INVALID_ARG);
    for (int32_t bad : {3, -2, INT32_MAX, INT32_MIN}) {
        hits[3].object = bad;
        CHECK(rt_shade_hits(hits.get(), 4, &s, RT_FORMAT_I32X4, px.get()) == RT_ERR_INVALID_ARG);
        CHECK(rt_shade_hits(hits.get(), 4, &s, RT_FORMAT_RGBA8, words.get()) == RT_ERR_INVALID_ARG);
    }
    if (failures) return 1;
    std::printf("hit args check ok\n");
    return 0;
}
