// camera_light_args_check.cpp -- rt_light_camera / rt_bounce_camera
// (csrc/rt_camera_light.cpp with csrc/rt_accel.cpp, csrc/rt_light.cpp,
// csrc/rt_args.cpp and csrc/rt_scene.cpp) as a stand-alone program on
// tests/light_check.h:
// tests/test_camera_light.py builds it with -fsanitize=address,undefined and
// runs it.  No GPU.
//
//   - exactly-sized heap arrays for the records, the reflectivity and every
//     output, at 1 x 1, 257 x 3 (a band) and 37 x 29, through the reference
//     camera and a pinhole;
//   - culled against unculled, byte for byte, depth 8 included;
//   - the reference camera against rt_light_hits_mirrored / rt_bounce_hits on
//     rt_cast_camera's frame;
//   - a scene without cubes and the empty scene, a NULL accel and a NULL
//     reflectivity;
//   - the argument checks.
// Exit 0 and "camera light args check ok" on success.
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

// Every output of both calls through `cam`, culled (where `accel`) against
// unculled; with `deferred`, also against the deferred pass on the cast's frame
// (the reference camera).  Returns the pixels whose ray met something.
int compare(const rt_camera& cam, const rt_scene& s, const rt_cube_bound* accel, const float* refl,
            int w, int rb, int re, bool deferred) {
    const size_t n = (size_t)w * (size_t)(re - rb);
    Exact<rt_hit> cast(n), bounce(n), want_bounce(n);
    Exact<int32_t> lit(4 * n), want_lit(4 * n);
    Exact<uint32_t> rgba(n), want_rgba(n);
    CHECK(rt_cast_camera(&cam, &s, w, rb, re, cast.p, nullptr) == RT_OK);
    int hit = 0;
    for (size_t i = 0; i < n; ++i) hit += cast[i].object >= 0;
    for (int b : {0, 1, 2, 8}) {
        CHECK(rt_bounce_camera(&cam, &s, nullptr, w, rb, re, b, want_bounce.p) == RT_OK);
        if (b == 0) CHECK(std::memcmp(want_bounce.p, cast.p, cast.bytes()) == 0);
        if (accel) {
            CHECK(rt_bounce_camera(&cam, &s, accel, w, rb, re, b, bounce.p) == RT_OK);
            CHECK(std::memcmp(bounce.p, want_bounce.p, bounce.bytes()) == 0);
        }
        if (deferred && b >= 1) {
            CHECK(rt_bounce_hits(cast.p, &s, kDir, w, rb, re, b, bounce.p) == RT_OK);
            CHECK(std::memcmp(bounce.p, want_bounce.p, bounce.bytes()) == 0);
        }
    }
    for (int depth : {0, 1, 8})
        for (int shadows = 0; shadows < 2; ++shadows) {
            CHECK(rt_light_camera(&cam, &s, nullptr, w, rb, re, refl, depth, shadows,
                                  RT_FORMAT_I32X4, want_lit.p) == RT_OK);
            CHECK(rt_light_camera(&cam, &s, nullptr, w, rb, re, refl, depth, shadows,
                                  RT_FORMAT_RGBA8, want_rgba.p) == RT_OK);
            for (size_t i = 0; i < n; ++i) {
                const int32_t* px = &want_lit[4 * i];  // the Texture packing
                const uint32_t packed = (uint32_t)(uint8_t)px[0] | (uint32_t)(uint8_t)px[1] << 8 |
                                        (uint32_t)(uint8_t)px[2] << 16 | 0xFF000000u;
                CHECK(packed == want_rgba[i]);
            }
            if (accel) {
                CHECK(rt_light_camera(&cam, &s, accel, w, rb, re, refl, depth, shadows,
                                      RT_FORMAT_I32X4, lit.p) == RT_OK);
                CHECK(std::memcmp(lit.p, want_lit.p, lit.bytes()) == 0);
                CHECK(rt_light_camera(&cam, &s, accel, w, rb, re, refl, depth, shadows,
                                      RT_FORMAT_RGBA8, rgba.p) == RT_OK);
                CHECK(std::memcmp(rgba.p, want_rgba.p, rgba.bytes()) == 0);
            }
            if (deferred) {
                CHECK(rt_light_hits_mirrored(cast.p, &s, kDir, w, rb, re, refl, depth, shadows,
                                             RT_FORMAT_I32X4, lit.p) == RT_OK);
                CHECK(std::memcmp(lit.p, want_lit.p, lit.bytes()) == 0);
            }
        }
    return hit;
}

}  // namespace

int main() {
    KindsScene kinds;
    const rt_scene& s = kinds.s;
    Exact<rt_cube_bound> accel(2);
    CHECK(rt_accel_build(&s, accel.p) == RT_OK);
    Exact<float> refl(KindsScene::slots);
    for (int i = 0; i < KindsScene::slots; ++i) refl[i] = 1.0f;  // every object a mirror

    rt_camera ref{}, pin{}, pin1{};
    CHECK(rt_camera_reference(kDir, &ref) == RT_OK);
    const float eye[3] = {150.0f, 20.0f, 60.0f}, target[3] = {80.0f, 64.0f, -40.0f};
    const float up[3] = {0.0f, -1.0f, 0.0f};
    CHECK(rt_camera_pinhole(eye, target, up, 60.0f, 37, 29, &pin) == RT_OK);
    CHECK(rt_camera_pinhole(eye, target, up, 60.0f, 1, 1, &pin1) == RT_OK);

    CHECK(compare(pin1, s, accel.p, refl.p, 1, 0, 1, false) == 1);  // 1 x 1: on the face
    CHECK(compare(ref, s, accel.p, refl.p, 257, 63, 66, true) > 300);  // rows 63..65
    const int seen = compare(pin, s, accel.p, refl.p, 37, 0, 29, false);
    CHECK(seen > 100 && seen < 37 * 29);
    CHECK(compare(pin, s, accel.p, refl.p, 37, 5, 17, false) > 50);
    CHECK(compare(ref, s, accel.p, refl.p, Band::w, Band::rb, Band::re, true) > 500);
    {  // no cubes: the spheres alone, a NULL accel; the empty scene, a NULL reflectivity
        rt_scene spheres = s;
        spheres.num_cubes = 0;
        spheres.cube_vertices = spheres.cube_colours = nullptr;
        CHECK(compare(ref, spheres, nullptr, refl.p, Band::w, Band::rb, Band::re, true) > 10);
        const rt_scene empty{};
        CHECK(compare(pin, empty, nullptr, nullptr, 37, 0, 29, false) == 0);
        Exact<int32_t> px(4 * 37 * 29);
        CHECK(rt_light_camera(&pin, &empty, nullptr, 37, 0, 29, nullptr, 8, 1, 0, px.p) == RT_OK);
        for (int i = 0; i < 37 * 29; ++i) CHECK(is_black(&px[4 * i]));
    }

    // ---- arguments --------------------------------------------------------------------
    const int w = 37, rb = 5, re = 17;
    Exact<int32_t> out(4 * (size_t)w * (re - rb));
    const rt_cube_bound* a = accel.p;
    struct CamCall {
        const rt_camera* cam;
        const rt_scene* scene;
        int32_t w, rb, re;
        void* out;
    };
    const CamCall ok{&pin, &s, w, rb, re, out.p};
    auto bounce = [&](const CamCall& c, int32_t b) {
        return rt_bounce_camera(c.cam, c.scene, a, c.w, c.rb, c.re, b, static_cast<rt_hit*>(c.out));
    };
    auto lit = [&](const CamCall& c, int32_t fmt) {
        return rt_light_camera(c.cam, c.scene, a, c.w, c.rb, c.re, refl.p, 2, 1, fmt, c.out);
    };
    auto both = [&](const CamCall& c, int want) {
        CHECK(bounce(c, 2) == want);
        CHECK(lit(c, RT_FORMAT_I32X4) == want);
        CHECK(lit(c, RT_FORMAT_RGBA8) == want);
    };
    both(ok, RT_OK);
    for (int pointer = 0; pointer < 3; ++pointer) {
        CamCall c = ok;
        if (pointer == 0) c.cam = nullptr;
        if (pointer == 1) c.scene = nullptr;
        if (pointer == 2) c.out = nullptr;
        both(c, RT_ERR_INVALID_ARG);
    }
    const int32_t top = 1 << 24;
    const int32_t shapes[][3] = {{0, rb, re},      {-1, rb, re},  {top + 1, 0, 1}, {w, -1, re - 1},
                                 {w, re, re},      {w, re, rb},   {w, top, top + 1}};
    for (const auto& shape : shapes) {
        CamCall c = ok;
        c.w = shape[0], c.rb = shape[1], c.re = shape[2];
        both(c, RT_ERR_INVALID_ARG);
    }
    for (int field = 0; field < 6; ++field) {
        rt_scene bad = s;
        if (field == 0) bad.lights = nullptr;
        if (field == 1) bad.num_lights = -1;
        if (field == 2) bad.num_cubes = -1;
        if (field == 3) bad.num_spheres = -1;
        if (field == 4) bad.cube_vertices = nullptr;
        if (field == 5) bad.sphere_origins = nullptr;
        CamCall c = ok;
        c.scene = &bad;
        both(c, RT_ERR_INVALID_ARG);
    }
    for (int32_t normalise : {2, -1}) {
        rt_camera bad = pin;
        bad.normalise = normalise;
        CamCall c = ok;
        c.cam = &bad;
        both(c, RT_ERR_INVALID_ARG);
    }
    for (int32_t fmt : {2, (int32_t)RT_FORMAT_HIT, 4, -1}) CHECK(lit(ok, fmt) == RT_ERR_INVALID_ARG);
    {  // out: 16 / 4 / 8 bytes
        CamCall c = ok;
        c.out = reinterpret_cast<char*>(out.p) + 8;
        CHECK(lit(c, RT_FORMAT_I32X4) == RT_ERR_INVALID_ARG);
        c.out = reinterpret_cast<char*>(out.p) + 2;
        CHECK(lit(c, RT_FORMAT_RGBA8) == RT_ERR_INVALID_ARG);
        c.out = reinterpret_cast<char*>(out.p) + 4;
        CHECK(bounce(c, 2) == RT_ERR_INVALID_ARG);
    }
    a = reinterpret_cast<const rt_cube_bound*>(reinterpret_cast<const char*>(accel.p) + 8);
    both(ok, RT_ERR_INVALID_ARG);  // a misaligned accel
    a = nullptr;
    both(ok, RT_OK);  // NULL: unculled
    a = accel.p;
    for (int b : {9, -1}) CHECK(bounce(ok, b) == RT_ERR_INVALID_ARG);
    CHECK(bounce(ok, 0) == RT_OK && bounce(ok, 8) == RT_OK);
    for (int depth : {-1, 9})
        CHECK(rt_light_camera(&pin, &s, a, w, rb, re, refl.p, depth, 0, 0, out.p) ==
              RT_ERR_INVALID_ARG);
    for (int shadows : {-1, 2})
        CHECK(rt_light_camera(&pin, &s, a, w, rb, re, refl.p, 2, shadows, 0, out.p) ==
              RT_ERR_INVALID_ARG);
    CHECK(rt_light_camera(&pin, &s, a, w, rb, re, nullptr, 2, 0, 0, out.p) == RT_ERR_INVALID_ARG);
    CHECK(rt_light_camera(&pin, &s, a, w, rb, re, nullptr, 0, 0, 0, out.p) == RT_OK);
    for (float r : {-0.1f, 1.5f, NAN, INFINITY}) {
        refl[1] = r;
        CHECK(lit(ok, RT_FORMAT_I32X4) == RT_ERR_INVALID_ARG);
    }
    refl[1] = 1.0f;
    {  // 33 lights are served
        std::unique_ptr<float[]> lights(new float[4 * 33]);
        for (int i = 0; i < 33; ++i) {
            lights[4 * i] = 4.0f * i, lights[4 * i + 1] = 64.0f;
            lights[4 * i + 2] = 40.0f, lights[4 * i + 3] = 1.0f;
        }
        rt_scene many = s;
        many.num_lights = 33;
        many.lights = lights.get();
        CamCall c = ok;
        c.scene = &many;
        both(c, RT_OK);
    }
    return finish("camera light");
}
