// light_accel_args_check.cpp -- rt_shadow_hits_accel / rt_bounce_hits_accel /
// rt_light_hits_mirrored_accel (csrc/rt_light_accel.cpp with csrc/rt_accel.cpp,
// csrc/rt_light.cpp and csrc/rt_args.cpp) as a stand-alone program on
// tests/light_check.h: tests/test_light_accel.py builds it with
// -fsanitize=address,undefined and runs it.  No GPU.
//
//   - exactly-sized heap arrays for the records, the hit frame, the
//     reflectivity and every output, at 1 x 1, 257 x 3 and a band of rows
//     60..67 of the 128-wide frame;
//   - every culled call against its unculled call, byte for byte, depth 8
//     included, on the scene of the shadow term's four kinds;
//   - a scene without cubes and the empty scene, both with a NULL accel;
//   - the argument checks.
// Exit 0 and "light accel args check ok" on success.
#include <new>

#include "light_check.h"

using namespace light_check;

namespace {

template <class T>
struct Exact {
    T* p;
    size_t n;
    explicit Exact(size_t n_)
        : p(static_cast<T*>(::operator new[](n_ * sizeof(T), std::align_val_t(16)))), n(n_) {}
    ~Exact() { ::operator delete[](p, std::align_val_t(16)); }
    T& operator[](size_t i) { return p[i]; }
    size_t bytes() const { return n * sizeof(T); }
};

// Every output of the three culled calls on `hits` (w x (re - rb)) against the
// unculled calls; `accel` may be NULL where the scene has no cubes.
void compare(const rt_hit* hits, const rt_scene& s, const rt_cube_bound* accel, const float* refl,
             int w, int rb, int re) {
    const size_t n = (size_t)w * (size_t)(re - rb);
    Exact<uint32_t> mask(n), want_mask(n), rgba(n), want_rgba(n);
    Exact<rt_hit> bounce(n), want_bounce(n);
    Exact<int32_t> lit(4 * n), want_lit(4 * n);
    CHECK(rt_shadow_hits_accel(hits, &s, accel, kDir, w, rb, re, mask.p) == RT_OK);
    CHECK(rt_shadow_hits(hits, &s, kDir, w, rb, re, want_mask.p) == RT_OK);
    CHECK(std::memcmp(mask.p, want_mask.p, mask.bytes()) == 0);
    for (int b : {1, 2, 8}) {
        CHECK(rt_bounce_hits_accel(hits, &s, accel, kDir, w, rb, re, b, bounce.p) == RT_OK);
        CHECK(rt_bounce_hits(hits, &s, kDir, w, rb, re, b, want_bounce.p) == RT_OK);
        CHECK(std::memcmp(bounce.p, want_bounce.p, bounce.bytes()) == 0);
    }
    for (int depth : {0, 1, 8})
        for (int shadows = 0; shadows < 2; ++shadows) {
            CHECK(rt_light_hits_mirrored_accel(hits, &s, accel, kDir, w, rb, re, refl, depth,
                                               shadows, RT_FORMAT_I32X4, lit.p) == RT_OK);
            CHECK(rt_light_hits_mirrored(hits, &s, kDir, w, rb, re, refl, depth, shadows,
                                         RT_FORMAT_I32X4, want_lit.p) == RT_OK);
            CHECK(std::memcmp(lit.p, want_lit.p, lit.bytes()) == 0);
            CHECK(rt_light_hits_mirrored_accel(hits, &s, accel, kDir, w, rb, re, refl, depth,
                                               shadows, RT_FORMAT_RGBA8, rgba.p) == RT_OK);
            CHECK(rt_light_hits_mirrored(hits, &s, kDir, w, rb, re, refl, depth, shadows,
                                         RT_FORMAT_RGBA8, want_rgba.p) == RT_OK);
            CHECK(std::memcmp(rgba.p, want_rgba.p, rgba.bytes()) == 0);
        }
}

}  // namespace

int main() {
    KindsScene kinds;
    const rt_scene& s = kinds.s;
    Exact<rt_cube_bound> accel(2);
    CHECK(rt_accel_build(&s, accel.p) == RT_OK);
    Exact<float> refl(KindsScene::slots);
    for (int i = 0; i < KindsScene::slots; ++i) refl[i] = 1.0f;  // every object a mirror

    {  // 1 x 1: the pole of sphere 0
        Exact<rt_hit> hits(1);
        hits[0] = rt_hit{18.0f, 2};
        compare(hits.p, s, accel.p, refl.p, 1, 0, 1);
    }
    {  // 257 x 3: rows 63..65, the face everywhere, misses at the ends
        const int w = 257, rb = 63, re = 66;
        Exact<rt_hit> hits((size_t)w * (re - rb));
        for (int i = 0; i < w * (re - rb); ++i)
            hits[i] = (i % w < 134) ? rt_hit{50.0f, 0} : rt_hit{300000.0f, -1};
        hits[w + 91] = rt_hit{3.0f, 1};  // on the box
        compare(hits.p, s, accel.p, refl.p, w, rb, re);
        Exact<uint32_t> mask(hits.n);
        CHECK(rt_shadow_hits_accel(hits.p, &s, accel.p, kDir, w, rb, re, mask.p) == RT_OK);
        int shadowed = 0;
        for (size_t i = 0; i < hits.n; ++i) shadowed += mask[i] != 0;
        CHECK(shadowed > 0 && shadowed < w * (re - rb));
    }
    Band band(true);
    compare(band.hits.get(), s, accel.p, refl.p, Band::w, Band::rb, Band::re);
    {  // what the band is there for: the box's shadow, and a bounce that meets something
        Exact<uint32_t> mask(Band::n);
        Exact<rt_hit> bounce(Band::n);
        CHECK(rt_shadow_hits_accel(band.hits.get(), &s, accel.p, kDir, Band::w, Band::rb, Band::re,
                                   mask.p) == RT_OK);
        CHECK(mask[Band::kSees] == 0 && mask[Band::kBehind] == 1 && mask[Band::kMiss] == 0);
        CHECK(rt_bounce_hits_accel(band.hits.get(), &s, accel.p, kDir, Band::w, Band::rb, Band::re,
                                   1, bounce.p) == RT_OK);
        CHECK(bounce[Band::kUnder].object == 3 && is_miss(bounce[Band::kMiss]));
    }
    {  // no cubes: the spheres alone, a NULL accel
        rt_scene spheres = s;
        spheres.num_cubes = 0;
        spheres.cube_vertices = spheres.cube_colours = nullptr;
        Exact<rt_hit> hits(Band::n);
        for (int i = 0; i < Band::n; ++i) hits[i] = rt_hit{300000.0f, -1};
        hits[Band::kPole] = rt_hit{18.0f, 0};
        compare(hits.p, spheres, nullptr, refl.p, Band::w, Band::rb, Band::re);
        const rt_scene empty{};
        hits[Band::kPole] = rt_hit{300000.0f, -1};
        compare(hits.p, empty, nullptr, nullptr, Band::w, Band::rb, Band::re);
    }

    // ---- arguments --------------------------------------------------------------------
    Exact<int32_t> out(4 * Band::n);
    const Call ok{band.hits.get(), &s, kDir, Band::w, Band::rb, Band::re, out.p};
    rt_hit* last = &band.hits[Band::n - 1];
    const rt_cube_bound* a = accel.p;
    auto own_mask = [&](const Call& c) {
        return rt_shadow_hits_accel(c.hits, c.scene, a, c.dir, c.w, c.rb, c.re,
                                    static_cast<uint32_t*>(c.out));
    };
    auto own_bounce = [&](const Call& c) {
        return rt_bounce_hits_accel(c.hits, c.scene, a, c.dir, c.w, c.rb, c.re, 2,
                                    static_cast<rt_hit*>(c.out));
    };
    auto lit = [&](const Call& c, int32_t fmt) {
        return rt_light_hits_mirrored_accel(c.hits, c.scene, a, c.dir, c.w, c.rb, c.re, refl.p, 2,
                                            1, fmt, c.out);
    };
    refusals(own_mask, ok, last, KindsScene::slots);
    refusals(own_bounce, ok, last, KindsScene::slots);
    refusals([&](const Call& c) { return lit(c, RT_FORMAT_RGBA8); }, ok, last, KindsScene::slots);
    refused_formats(lit, ok);
    const rt_cube_bound* off =
        reinterpret_cast<const rt_cube_bound*>(reinterpret_cast<const char*>(accel.p) + 8);
    for (const rt_cube_bound* bad : {static_cast<const rt_cube_bound*>(nullptr), off}) {
        a = bad;
        CHECK(own_mask(ok) == RT_ERR_INVALID_ARG);
        CHECK(own_bounce(ok) == RT_ERR_INVALID_ARG);
        CHECK(lit(ok, RT_FORMAT_I32X4) == RT_ERR_INVALID_ARG);
    }
    a = accel.p;
    for (int b : {0, 9, -1})
        CHECK(rt_bounce_hits_accel(ok.hits, &s, a, kDir, ok.w, ok.rb, ok.re, b,
                                   static_cast<rt_hit*>(ok.out)) == RT_ERR_INVALID_ARG);
    for (int depth : {-1, 9})
        CHECK(rt_light_hits_mirrored_accel(ok.hits, &s, a, kDir, ok.w, ok.rb, ok.re, refl.p, depth,
                                           0, 0, ok.out) == RT_ERR_INVALID_ARG);
    for (int shadows : {-1, 2})
        CHECK(rt_light_hits_mirrored_accel(ok.hits, &s, a, kDir, ok.w, ok.rb, ok.re, refl.p, 2,
                                           shadows, 0, ok.out) == RT_ERR_INVALID_ARG);
    CHECK(rt_light_hits_mirrored_accel(ok.hits, &s, a, kDir, ok.w, ok.rb, ok.re, nullptr, 2, 0, 0,
                                       ok.out) == RT_ERR_INVALID_ARG);
    refl[1] = 1.5f;
    CHECK(lit(ok, RT_FORMAT_I32X4) == RT_ERR_INVALID_ARG);
    refl[1] = 1.0f;
    {  // 33 lights: the mask alone
        std::unique_ptr<float[]> lights(new float[4 * 33]);
        for (int i = 0; i < 33; ++i) {
            lights[4 * i] = 4.0f * i, lights[4 * i + 1] = 64.0f;
            lights[4 * i + 2] = 40.0f, lights[4 * i + 3] = 1.0f;
        }
        rt_scene many = s;
        many.num_lights = 33;
        many.lights = lights.get();
        Call c = ok;
        c.scene = &many;
        CHECK(own_mask(c) == RT_ERR_UNSUPPORTED);
        CHECK(own_bounce(c) == RT_OK);
        CHECK(lit(c, RT_FORMAT_RGBA8) == RT_OK);
        many.num_lights = 32;
        CHECK(own_mask(c) == RT_OK);
    }
    return finish("light accel");
}
