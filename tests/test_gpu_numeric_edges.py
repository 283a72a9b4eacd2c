"""Parity at the numeric edges of the binned kernels' input domain.

The rest of the suite varies frame sizes, primitive counts and path knobs but
feeds the kernels ordinary values: one ray direction (0, 0, -1, -1), colours
in [0, 1], depths of a few hundred units.  Here the *values* leave that range:
every direction shape `binned_ok` accepts (rt_device.hip), colours and depths
whose (int) store leaves the int32 range (shade_pixels' ballot-gated fix-up,
MainState.cpp:396-407 and :952-955), depths on both sides of div180's 2^-100
switch, and spheres on both sides of each condition of SphRec::fast
(prep_sphere).  Every case is rendered by every kernel of the path matrix
(PATHS) in both formats and compared bit for bit with the CPU oracle
(oracle/rt_oracle.c: any ray_dir, x86's (int) restated in cvt_i32).

`test_case_conditions` (no GPU) asserts on the oracle frames that each case
really produces what it is there for (hits, INT32_MIN channels beside
in-range ones, pixels won by the edge objects); the GPU test asserts the same
conditions before it compares.
"""
import numpy as np
import pytest

from gpu_support import (F32, FUSED_MAX_PRIMS, H, PATHS, REF_DIR, W, base_scene, n_prims,
                         render_all_paths)

gpu = pytest.mark.gpu

INT_MIN = -(1 << 31)


# ---------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------
def _clone(pkg, s):
    return pkg.Scene(s.sphere_origins.copy(), s.sphere_radius.copy(), s.sphere_colours.copy(),
                     s.cube_vertices.copy(), s.cube_colours.copy())


def _add_spheres(pkg, s, spheres):
    """Append (origin4, radius, colour4) spheres: last in the reference's order."""
    so = np.array([x[0] for x in spheres], F32).reshape(-1, 4)
    sr = np.array([x[1] for x in spheres], F32)
    sc = np.array([x[2] for x in spheres], F32).reshape(-1, 4)
    return pkg.Scene(np.concatenate([s.sphere_origins, so]), np.concatenate([s.sphere_radius, sr]),
                     np.concatenate([s.sphere_colours, sc]), s.cube_vertices.copy(),
                     s.cube_colours.copy())


def _add_cube(pkg, s, ops, colour):
    v = pkg.cube_packed(ops).reshape(1, 36, 4)
    return pkg.Scene(s.sphere_origins.copy(), s.sphere_radius.copy(), s.sphere_colours.copy(),
                     np.concatenate([s.cube_vertices, v]),
                     np.concatenate([s.cube_colours, np.array([colour], F32)]))


def _spheres_only(pkg, s):
    return pkg.Scene(s.sphere_origins.copy(), s.sphere_radius.copy(), s.sphere_colours.copy())


def _spheres_only_last(s):
    """The scene's last sphere alone."""
    return type(s)(s.sphere_origins[-1:], s.sphere_radius[-1:], s.sphere_colours[-1:])


# Builders: (pkg, base) -> (scene, [scene without one group of edge objects, ...])
def plain(pkg, b):
    return _clone(pkg, b), []


def mirror(pkg, b):
    s = _clone(pkg, b)
    s.sphere_origins[:, 2] *= F32(-1)
    s.cube_vertices[..., 2] *= F32(-1)
    return s, []


def layers(z_sign):
    """Occlusion for the depth culls (the base's objects are smaller than a
    wave tile, so nothing in it ever covers one): a front sphere and a front
    cube face that cover whole tiles, spheres and cubes behind them (dropped
    once a tile is covered), later nearer ones that must still win, a sphere
    with t0 == 0 and one around the origin plane.  The culls' bounds (SphRec::
    tmin_key, TriDepth / tri_t_bounds) take D and w as variables; a bound
    that is not conservative for them drops a primitive that wins pixels."""
    def build(pkg, b):
        del b
        spheres = ([((40, 40, -70, 1), 68, (1, .2, .2, 255))] +
                   [((25 + 5 * i, 30 + 2 * i, -72 - 3 * i, 1), 50 + 4 * i, (.2, 1, .1 * i, 255))
                    for i in range(10)] +
                   [((40, 40, -70, 1), 68, (0, 0, 1, 255)),
                    ((70, 50, -12, 1), 14, (1, 0, 1, 255)),
                    ((20, 60, -4, 1), 4, (.5, .5, .5, 255)),
                    ((60, 20, -2, 1), 9, (.9, .9, .1, 255))])
        cubes = ([([("scale", 70, 90, 6), ("rotate", .05, .1, .02), ("translate", 75, 40, -25)],
                   (.3, .6, .9, 255))] +
                 [([("scale", 20 + 4 * i, 25, 8), ("rotate", .3 * i, .2, .1 * i),
                    ("translate", 60 + 6 * i, 20 + 10 * i, -45 - 10 * i)], (.9, .1 * i, .3, 255))
                  for i in range(5)] +
                 [([("scale", 9, 9, 9), ("rotate", .4, .5, .6), ("translate", 85, 60, -10)],
                   (.1, .9, .9, 255))])
        front = pkg.Scene(np.array([x[0] for x in spheres], F32),
                          np.array([x[1] for x in spheres], F32),
                          np.array([x[2] for x in spheres], F32),
                          np.array([pkg.cube_packed(c[0]) for c in cubes], F32),
                          np.array([c[1] for c in cubes], F32))
        front.sphere_origins[:, 2] *= F32(z_sign)
        front.cube_vertices[..., 2] *= F32(z_sign)
        behind = pkg.Scene(front.sphere_origins[1:], front.sphere_radius[1:],
                           front.sphere_colours[1:], front.cube_vertices[1:],
                           front.cube_colours[1:])
        late = pkg.Scene(front.sphere_origins[:-3], front.sphere_radius[:-3],
                         front.sphere_colours[:-3], front.cube_vertices[:-1],
                         front.cube_colours[:-1])
        return front, [behind, late]
    return build


def sphere_w(value):
    """Every second sphere's origin w (the reference uploads 1): Lw = w - 1
    enters tca through Lw * dw and dist2 through Lw^2."""
    def build(pkg, b):
        s = _clone(pkg, b)
        s.sphere_origins[::2, 3] = F32(value)
        return s, []
    return build


def near_z(scale):
    """The whole scene's z scaled: with |D| = 1e-4 the base's depths give
    t = z / D above kFar (300000) almost everywhere; at z / 25 the cubes'
    t is 12,000 .. 43,000 and they are drawn."""
    def build(pkg, b):
        s = _clone(pkg, b)
        s.sphere_origins[:, 2] *= F32(scale)
        s.cube_vertices[..., 2] *= F32(scale)
        return s, []
    return build


def colour(value, z_scale=1.0):
    """Every second sphere's green and every second cube's red channel: waves
    mix lanes in and out of the int range.  z_scale: the scene's depths scaled
    first (1e7: scalar * 1e7 crosses 2^31 at t = 28.4, nearer than almost all
    of the base, whose t is 11 .. 100; at half the depth the crossing lies in
    the middle of the scene and both sides are well populated)."""
    def build(pkg, b):
        s, _ = near_z(z_scale)(pkg, b)
        s.sphere_colours[::2, 1] = F32(value)
        s.cube_colours[::2, 0] = F32(value)
        return s, []
    return build


def zero_times_inf(pkg, b):
    """A flat cube at z = +3e38: t = -3e38, normalised * 255 overflows, scalar
    = +inf; its colour (0, .5, .7) gives 0 * inf = NaN, inf, inf.  All three
    are INT32_MIN in the reference; the NaN takes cvt_i32_fast's NaN leg."""
    s = _add_cube(pkg, b, [("scale", 40, 30, 1), ("translate", 48, 40, 3e38)], (0, .5, .7, 255))
    return s, [_clone(pkg, b)]


def cube_z(scale):
    """Cube vertices' z scaled (in float32, as a host would store them)."""
    def build(pkg, b):
        s = _clone(pkg, b)
        s.cube_vertices[..., 2] *= F32(scale)
        return s, [_spheres_only(pkg, b)]
    return build


def far_spheres(pkg, b):
    """Spheres at z = -1e15: Lx^2 + Ly^2 is absorbed by kzw = 1e30 and kzw -
    tca2 = 0, so each covers every pixel with t0 = 1e15 - r.  r = 1e15 gives
    t0 == 0 (never taken, MainState.cpp:383); one float above gives t0 = -1
    ulp(1e15) = -6.7e7 and must beat everything placed before it."""
    r = F32(1e15)
    s = _add_spheres(pkg, b, [((20, 20, -1e15, 1), r, (.25, 1, .5, 255)),
                              ((48, 40, -1e15, 1), np.nextafter(r, F32(np.inf)),
                               (1, .5, .25, 255))])
    return s, [_clone(pkg, b)]


def huge_sphere(pkg, b):
    """Radius 1e20, placed last: r2 = inf, arg = inf, t0 = -inf from finite
    inputs.  (r2 - dist2 is +inf at every pixel, so it covers the frame.)"""
    s = _add_spheres(pkg, b, [((48, 40, -50, 1), 1e20, (1, .5, .25, 255))])
    return s, [_clone(pkg, b)]


def tiny_guard(pkg, b):
    """r2 on both sides of 2^-70 (SphRec::fast's lower limit), centred on
    integer pixels at z = -1 so each wins exactly its centre pixel.  Far
    below the limit the frame can see the sqrt only through t0 == 0 (never
    taken, MainState.cpp:383): at z = -2^-70 (kzw = tca2 = 2^-140, denormal)
    a sphere of radius 2^-71 wins its pixel with t0 = 2^-71, and one of
    radius 2^-70 (r2 denormal, thc == tca, t0 == 0) must not be drawn;
    flushed denormals or an inexact sqrt draw it."""
    r, z = F32(2.0 ** -35), -2.0 ** -70
    inside = ((30, 20, -1, 1), r, (.9, .6, .3, 255))
    outside = ((60, 50, -1, 1), np.nextafter(r, F32(0)), (.3, .6, .9, 255))
    denormal = ((10, 70, z, 1), 2.0 ** -71, (.6, .9, .3, 255))
    undrawn = ((80, 10, z, 1), 2.0 ** -70, (.3, .9, .6, 255))
    every = [inside, outside, denormal, undrawn]
    return (_add_spheres(pkg, b, every),
            [_add_spheres(pkg, b, [x for x in every if x is not gone])
             for gone in (inside, outside, denormal)])


def big_guard(lz, lw, r, t_est):
    """One sphere with |values| near 2^100, placed last.  Its t0 does not
    depend on the pixel (Lx^2 + Ly^2 is absorbed), so it wins every pixel or
    none; its colour is scaled so that the channels stay inside the int
    range and a one-ulp error of the sqrt (2^27 at 2^50) changes them."""
    def build(pkg, b):
        c = 1.5e9 / (255.0 * t_est / 180.0)
        s = _add_spheres(pkg, b, [((48, 40, lz, 1.0 + lw), r, (c, c / 2, c / 4, 255))])
        return s, [_clone(pkg, b)]
    return build


_A = 2.0 ** 50
_UP = 1.0 + 2.0 ** -21  # radius over |Lz|: thc - tca = 2^-21 tca, t0 < 0
_GUARDS = {
    # r2, kzw, tca2 all just inside 2^100: a^2 = 2^100 (1 - 2^-19), r2 = a^2 (1 + 2^-20)
    "guard_all_inside": big_guard(-_A * (1 - 2.0 ** -20), 0.0, _A * (1 - 2.0 ** -20) * _UP,
                                  _A * 2.0 ** -21),
    # r2 = 2^100 (1 - 2^-21)(1 + 2^-20) > 2^100, kzw = tca2 just inside
    "guard_r2_outside": big_guard(-_A * (1 - 2.0 ** -22), 0.0, _A * (1 - 2.0 ** -22) * _UP,
                                  _A * 2.0 ** -21),
    # Lz = Lw = -a: tca = 2a, tca2 = 4a^2 just inside / outside, kzw = 2a^2 and
    # r2 = 2a^2 (1 + 2^-20) inside; thc = 2a sqrt(1 + 2^-21), t0 = -2a 2^-22
    "guard_tca2_inside": big_guard(-_A / 2 * (1 - 2.0 ** -20), -_A / 2 * (1 - 2.0 ** -20),
                                   2.0 ** 0.5 * _A / 2 * (1 - 2.0 ** -20) * _UP, _A * 2.0 ** -22),
    "guard_tca2_outside": big_guard(-_A / 2 * 1.2, -_A / 2 * 1.2, 2.0 ** 0.5 * _A / 2 * 1.2 * _UP,
                                    1.2 * _A * 2.0 ** -22),
    # Lz = -0.8 2^50, Lw = +0.7 2^50: kzw = 1.13 2^100 outside, tca2 = 0.01 2^100
    # inside.  A sphere can only win with thc > tca, i.e. r2 > kzw, so r2 is
    # outside too: r = 1.1 sqrt(kzw), t0 = (0.1 - 0.497) 2^50
    "guard_kzw_outside": big_guard(-0.8 * _A, 0.7 * _A, 1.1 * (0.64 + 0.49) ** 0.5 * _A,
                                   0.397 * _A),
}

# kind: "dir" (5 % hits), "miss" (no hit), "colour" (in range, 5 % hits),
# "range" (colour out of range: INT32_MIN beside in-range), "depth" (>= 100
# pixels won per group of edge objects), "guard" (>= 1 pixel won per sphere)
CASES = {}


def _case(name, build, kind, d=REF_DIR, size=(W, H), rows=None):
    assert name not in CASES
    CASES[name] = dict(build=build, kind=kind, d=d, size=size, rows=rows)


_case("dir_D-2", plain, "dir", d=(0, 0, -2, -1))
_case("dir_D-0.37", plain, "dir", d=(0, 0, -0.37, -1))
_case("dir_D+1_mirror", mirror, "dir", d=(0, 0, 1, -1))
_case("dir_D+2.5_mirror", mirror, "dir", d=(0, 0, 2.5, -1))
_case("dir_negative_zero_xy", plain, "dir", d=(-0.0, -0.0, -1, -1))
_case("dir_w0", plain, "dir", d=(0, 0, -1, 0))
for _w in (3, -2):
    _case(f"dir_w3_sphere_w{_w}", sphere_w(_w), "dir", d=(0, 0, -1, 3))
    _case(f"dir_ref_sphere_w{_w}", sphere_w(_w), "dir")
_case("dir_D-1e-4_det_near_epsilon", near_z(0.04), "dir", d=(0, 0, -1e-4, -1))
_case("dir_D1e-30_all_miss", plain, "miss", d=(0, 0, 1e-30, 1))
_case("dir_D-1e20", plain, "dir", d=(0, 0, -1e20, -1))
_case("dir_D-3e38", plain, "dir", d=(0, 0, -3e38, -1))
_case("dir_D-0.37_101x77_band", plain, "dir", d=(0, 0, -0.37, -1), size=(101, 77), rows=(13, 70))
_case("dir_D+2.5_mirror_101x77_band", mirror, "dir", d=(0, 0, 2.5, -1), size=(101, 77),
      rows=(13, 70))

# (kind "depth": the front coverers, and the late nearer objects, each win
# >= 100 pixels)
_case("layers_ref", layers(1), "depth")
_case("layers_D-2", layers(1), "depth", d=(0, 0, -2, -1))
_case("layers_D-0.37", layers(1), "depth", d=(0, 0, -0.37, -1))
_case("layers_D+1_mirror", layers(-1), "depth", d=(0, 0, 1, -1))
_case("layers_D+2.5_mirror", layers(-1), "depth", d=(0, 0, 2.5, -1))
_case("layers_D+0.37_mirror_101x77_band", layers(-1), "depth", d=(0, 0, 0.37, -1), size=(101, 77),
      rows=(13, 70))
_case("layers_w3", layers(1), "depth", d=(0, 0, -1, 3))

_case("colour_-1", colour(-1.0), "colour")
_case("colour_1e7", colour(1e7, 0.5), "range")
_case("colour_1e8", colour(1e8), "range")
_case("colour_3e38", colour(3e38), "range")
_case("colour_+inf", colour(np.inf), "range")
_case("colour_-inf", colour(-np.inf), "range")
_case("colour_nan", colour(np.nan), "range")
_case("colour_denormal", colour(1e-40), "colour")
_case("colour_0_times_inf", zero_times_inf, "range")
_case("colour_1e7_101x77_band", colour(1e7, 0.5), "range", size=(101, 77), rows=(13, 70))
_case("colour_nan_101x77_band", colour(np.nan), "range", size=(101, 77), rows=(13, 70))

_case("depth_cube_z_1e-37", cube_z(1e-37), "depth")
_case("depth_cube_z_1e-41_denormal", cube_z(1e-41), "depth")
_case("depth_spheres_z-1e15", far_spheres, "depth")
_case("depth_sphere_r1e20", huge_sphere, "depth")
# (z * +1e30 leaves the cubes at t = +3e31, behind kFar, never drawn; on the
# mirrored side t = -3e31 and the scaled cubes beat everything they cover)
_case("depth_cube_z_-1e30", cube_z(-1e30), "depth")

_case("guard_r2_2^-70", tiny_guard, "guard")
for _name, _build in _GUARDS.items():
    _case(_name, _build, "guard")


def _hit(frame):
    return (frame != np.array([0, 0, 0, 255], np.int32)).any(-1)


def oracle_frames(pkg, oracle, name):
    """(scene, frame, fused scene, its frame) of a case, conditions asserted."""
    c = CASES[name]
    (w, h), d = c["size"], np.asarray(c["d"], F32)
    out = []
    for fused in (False, True):
        scene, without = c["build"](pkg, base_scene(pkg, fused))
        frame = oracle.trace(scene, w, h, rows=c["rows"], ray_dir=d)
        check_conditions(name, oracle, frame, scene, without,
                         near_z(0.5)(pkg, base_scene(pkg, fused))[0]
                         if name.startswith("colour_1e7") else None)
        out += [scene, frame]
    assert n_prims(out[2]) <= FUSED_MAX_PRIMS
    return out


def check_conditions(name, oracle, frame, scene, without, plain_scene):
    c = CASES[name]
    (w, h), d, kind = c["size"], np.asarray(c["d"], F32), c["kind"]
    hit = _hit(frame)
    n_px = frame.shape[0] * frame.shape[1]
    if kind == "miss":
        assert hit.sum() == 0, name
        return
    assert hit.sum() >= 0.05 * n_px, f"{name}: {hit.sum()} of {n_px} pixels hit"
    rgb = frame[..., :3]
    if kind == "range":
        n_min = int((rgb == INT_MIN).sum())
        n_ok = int((hit & (rgb != INT_MIN).all(-1)).sum())
        assert n_min >= 100 and n_ok >= 100, f"{name}: {n_min} INT32_MIN channels, {n_ok} in range"
    if plain_scene is not None:  # the 1e7 cases: channels on both sides of 2^31
        touched = (frame != oracle.trace(plain_scene, w, h, rows=c["rows"], ray_dir=d)).any(-1)
        n_pos = int(((rgb > 0) & touched[..., None]).sum())
        assert n_pos >= 100, f"{name}: {n_pos} positive in-range channels"
    for i, other in enumerate(without):
        won = (frame != oracle.trace(other, w, h, rows=c["rows"], ray_dir=d)).any(-1)
        need = 100 if kind == "depth" else 1
        assert won.sum() >= need, f"{name}: edge group {i} wins {won.sum()} pixels"
        if name == "guard_r2_2^-70":  # the t0 == 0 sphere's pixel (80, 10) stays as it was
            assert np.array_equal(frame[10, 80], oracle.trace(without[0], w, h, ray_dir=d)[10, 80])
            assert not _hit(oracle.trace(_spheres_only_last(scene), w, h, ray_dir=d)).any()
        if name in _GUARDS:  # ulp-sensitive, in-range channels (see big_guard)
            assert (rgb[won] != INT_MIN).all() and (np.abs(rgb[won]) > 1 << 24).all(), name
    if kind in ("depth", "guard"):
        assert without, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_conditions(pkg, oracle, name):
    """Each case does what it is in the table for, on the oracle's frames
    (full scene and its <= 128-primitive variant); no GPU."""
    oracle_frames(pkg, oracle, name)


def test_case_table_is_complete():
    """Every class of case is in the table, in the numbers it was written with."""
    kinds = [c["kind"] for c in CASES.values()]
    assert kinds.count("miss") == 1 and kinds.count("range") >= 8 and kinds.count("depth") == 5 + 7
    assert kinds.count("guard") == 1 + len(_GUARDS) and kinds.count("dir") >= 15
    assert sum(c["rows"] == (13, 70) and c["size"] == (101, 77) for c in CASES.values()) >= 2


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_numeric_edge_parity(pkg, rt, oracle, name):
    """Every case x every kernel of PATHS x both formats equals the oracle's
    frame bit for bit; directions binned_ok accepts stay on the binned path."""
    c = CASES[name]
    scene, want, fused_scene, fused_want = oracle_frames(pkg, oracle, name)
    (w, h) = c["size"]
    n = render_all_paths(rt, oracle, scene, w, h, rows=c["rows"], ray_dir=c["d"], want=want,
                         fused_scene=fused_scene, fused_want=fused_want, label=name)
    assert n == 2 * len(PATHS)
