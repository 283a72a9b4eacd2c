// light_check.h -- what the light pass's five stand-alone check programs
// (tests/{light,shadow,reflect,shadow_reflect,mirror}_args_check.cpp) share:
// CHECK and the failure count, box() and is_miss(), the scene of the shadow
// term's four kinds in exactly-sized heap arrays, the band of rows 60..67 of
// its 128-wide frame, the refusals every host entry point owes its caller and
// the empty-scene section.  tests/light_contract.py builds each program with
// -fsanitize=address,undefined and runs it.  No GPU.
//
// Every array is a `new[]` of its exact size, so that an overrun by one
// element on either side is reported.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "rt_hip.h"

namespace light_check {

inline int failures = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, \
                         #cond);                                                 \
            ++light_check::failures;                                             \
        }                                                                        \
    } while (0)

const float kDir[4] = {0.0f, 0.0f, -1.0f, -1.0f};
const int32_t kBlack[4] = {0, 0, 0, 255};

// an axis-aligned box as a cube's float4[36], Cube.cpp's corner order
inline void box(float* verts, const float lo[3], const float hi[3]) {
    // corner bit0 = x, bit1 = y, bit2 = z (set = hi)
    const unsigned char corners[36] = {0, 4, 6, 3, 0, 2, 5, 0, 1, 3, 1, 0, 0, 6, 2, 5, 4, 0,
                                       6, 4, 5, 7, 1, 3, 1, 7, 5, 7, 3, 2, 7, 2, 6, 7, 6, 5};
    for (int k = 0; k < 36; ++k) {
        for (int a = 0; a < 3; ++a) verts[4 * k + a] = (corners[k] >> a & 1u) ? hi[a] : lo[a];
        verts[4 * k + 3] = 1.0f;
    }
}

inline bool is_miss(const rt_hit& h) { return h.t == 300000.0f && h.object == -1; }
inline bool is_black(const int32_t* px) { return std::memcmp(px, kBlack, sizeof kBlack) == 0; }

// The four kinds: cube 0 (the face z = -50), cube 1 (the box), sphere 0 (slot
// 2), sphere 1 (slot 3, in front of the ray origins: no primary ray sees it),
// one light.
struct KindsScene {
    static constexpr int slots = 4;
    std::unique_ptr<float[]> verts{new float[2 * 144]};
    std::unique_ptr<float[]> cube_col{new float[8]{1.0f, 0.7f, 0.3f, 255.0f, 0.3f, 0.5f, 1.0f, 255.0f}};
    std::unique_ptr<float[]> sph_org{new float[8]{64.0f, 64.0f, -30.0f, 1.0f, 118.0f, 64.0f, 12.0f, 1.0f}};
    std::unique_ptr<float[]> sph_rad{new float[2]{12.0f, 4.0f}};
    std::unique_ptr<float[]> sph_col{new float[8]{0.2f, 0.9f, 0.4f, 255.0f, 0.9f, 0.9f, 0.1f, 255.0f}};
    std::unique_ptr<float[]> light{new float[4]{154.0f, 64.0f, 40.0f, 1.0f}};
    rt_scene s{};

    KindsScene() {
        const float lo0[3] = {-6.0f, -6.0f, -70.0f}, hi0[3] = {134.0f, 134.0f, -50.0f};
        const float lo1[3] = {85.0f, 58.0f, -15.0f}, hi1[3] = {97.0f, 70.0f, -3.0f};
        box(verts.get(), lo0, hi0);
        box(verts.get() + 144, lo1, hi1);
        s.num_cubes = 2;
        s.cube_vertices = verts.get();
        s.cube_colours = cube_col.get();
        s.num_spheres = 2;
        s.sphere_origins = sph_org.get();
        s.sphere_radius = sph_rad.get();
        s.sphere_colours = sph_col.get();
        s.num_lights = 1;
        s.lights = light.get();
    }
};

// Rows 60..67 of the scene's 128-wide frame, every pixel on the face (t = 50)
// but kPole, the pole of sphere 0 (t = 18), with `flank` kFlank on its flank,
// and kMiss, the last pixel.  kSees (5, 60) sees the light; the segment from
// kBehind (38, 64) to the light passes the centre of sphere 0; kUnder (118,
// 64) lies straight under sphere 1.
struct Band {
    static constexpr int w = 128, rb = 60, re = 68, n = w * (re - rb);
    static constexpr int kPole = 4 * w + 64, kFlank = 4 * w + 75, kUnder = 4 * w + 118,
                         kBehind = 4 * w + 38, kSees = 5, kMiss = n - 1;
    std::unique_ptr<rt_hit[]> hits{new rt_hit[n]};

    explicit Band(bool flank) {
        for (int i = 0; i < n; ++i) hits[i] = rt_hit{50.0f, 0};
        hits[kPole] = rt_hit{18.0f, 2};
        if (flank) hits[kFlank] = rt_hit{30.0f - std::sqrt(23.0f), 2};
        hits[kMiss] = rt_hit{300000.0f, -1};
    }
};

// The arguments every host entry point of the light pass takes; what follows
// row_end (a reflectivity, a bounce number, a format, ...) is the caller's.
struct Call {
    const rt_hit* hits;
    const rt_scene* scene;
    const float* dir;
    int32_t w, rb, re;
    void* out;
};

// `fn(Call)` serves `ok` and refuses: each pointer NULL; widths and rows out
// of range; negative counts and arrays missing for a non-zero count; an
// object id outside [-1, slots) in `*last`, a pixel of ok.hits (put back
// afterwards).
template <class F>
void refusals(F fn, const Call& ok, rt_hit* last, int32_t slots) {
    CHECK(fn(ok) == RT_OK);
    Call c = ok;
    for (int pointer = 0; pointer < 4; ++pointer) {
        c = ok;
        if (pointer == 0) c.hits = nullptr;
        if (pointer == 1) c.scene = nullptr;
        if (pointer == 2) c.dir = nullptr;
        if (pointer == 3) c.out = nullptr;
        CHECK(fn(c) == RT_ERR_INVALID_ARG);
    }
    const int32_t top = 1 << 24;
    const int32_t shapes[][3] = {{0, ok.rb, ok.re},     {-1, ok.rb, ok.re},    {top + 1, 0, 1},
                                 {ok.w, -1, ok.re - 1}, {ok.w, ok.re, ok.re},  {ok.w, ok.re, ok.rb},
                                 {ok.w, top, top + 1}};
    for (const auto& shape : shapes) {
        c = ok;
        c.w = shape[0], c.rb = shape[1], c.re = shape[2];
        CHECK(fn(c) == RT_ERR_INVALID_ARG);
    }
    for (int field = 0; field < 6; ++field) {
        rt_scene bad = *ok.scene;
        if (field == 0) bad.lights = nullptr;
        if (field == 1) bad.num_lights = -1;
        if (field == 2) bad.num_cubes = -1;
        if (field == 3) bad.num_spheres = -1;
        if (field == 4) bad.cube_vertices = nullptr;
        if (field == 5) bad.sphere_origins = nullptr;
        c = ok;
        c.scene = &bad;
        CHECK(fn(c) == RT_ERR_INVALID_ARG);
    }
    const int32_t kept = last->object;
    for (int32_t obj : {slots, -2, INT32_MAX, INT32_MIN}) {
        last->object = obj;
        CHECK(fn(ok) == RT_ERR_INVALID_ARG);
    }
    last->object = kept;
    CHECK(fn(ok) == RT_OK);
}

// `lit(Call, format)` refuses every format but the two lit ones.
template <class Lit>
void refused_formats(Lit lit, const Call& ok) {
    CHECK(lit(ok, RT_FORMAT_I32X4) == RT_OK);
    for (int32_t fmt : {2, (int32_t)RT_FORMAT_HIT, 4, -1})
        CHECK(lit(ok, fmt) == RT_ERR_INVALID_ARG);
}

// The lit entry point of a pass with one reflectivity, `lit_at(r)(Call,
// format)`: the refusals with and without a second ray, and every r outside
// [0, 1].
template <class LitAt>
void reflectivity_refusals(LitAt lit_at, const Call& ok, rt_hit* last, int32_t slots) {
    for (float r : {0.0f, 0.5f}) {
        refused_formats(lit_at(r), ok);
        refusals([&](const Call& c) { return lit_at(r)(c, 0); }, ok, last, slots);
    }
    for (float r : {-0.1f, 1.5f, NAN, INFINITY, -INFINITY, std::nextafter(1.0f, 2.0f)})
        for (int32_t fmt : {(int32_t)RT_FORMAT_I32X4, (int32_t)RT_FORMAT_RGBA8})
            CHECK(lit_at(r)(ok, fmt) == RT_ERR_INVALID_ARG);
}

// An empty scene with NULL arrays, without a light and with `light`: every
// pixel a miss.  `own(Call)` writes T per pixel, each `is_empty`; `lit(Call,
// format)` writes (0, 0, 0, 255) / 0xFF000000.  Any object is out of range.
template <class T, class Own, class Lit, class IsEmpty>
void empty_scene(const float* light, Own own, Lit lit, IsEmpty is_empty) {
    rt_scene empty{};
    const int w = 5, rows = 3;
    std::unique_ptr<rt_hit[]> hits(new rt_hit[w * rows]);
    for (int i = 0; i < w * rows; ++i) hits[i] = rt_hit{300000.0f, -1};
    std::unique_ptr<T[]> mine(new T[w * rows]);
    std::unique_ptr<int32_t[]> px(new int32_t[4 * w * rows]);
    std::unique_ptr<uint32_t[]> words(new uint32_t[w * rows]);
    const Call call{hits.get(), &empty, kDir, w, 0, rows, nullptr};
    auto into = [&](void* out) {
        Call c = call;
        c.out = out;
        return c;
    };
    for (int with_light = 0; with_light < 2; ++with_light) {
        empty.lights = with_light ? light : nullptr;
        empty.num_lights = with_light;
        CHECK(own(into(mine.get())) == RT_OK);
        CHECK(lit(into(px.get()), RT_FORMAT_I32X4) == RT_OK);
        CHECK(lit(into(words.get()), RT_FORMAT_RGBA8) == RT_OK);
        for (int i = 0; i < w * rows; ++i) {
            CHECK(is_empty(mine[i]));
            CHECK(is_black(&px[4 * i]));
            CHECK(words[i] == 0xFF000000u);
        }
    }
    hits[w * rows - 1].object = 0;
    CHECK(own(into(mine.get())) == RT_ERR_INVALID_ARG);
    CHECK(lit(into(px.get()), RT_FORMAT_I32X4) == RT_ERR_INVALID_ARG);
}

// "<name> args check ok" and exit status 0, or 1 after a failed CHECK
inline int finish(const char* name) {
    if (failures) return 1;
    std::printf("%s args check ok\n", name);
    return 0;
}

}  // namespace light_check
