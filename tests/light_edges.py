"""The light pass over its whole input domain: the case table -- TEST
INFRASTRUCTURE ONLY.

rt_hit_surfaces* / rt_light_hits*  take any ray direction,
any float in a light, any t and, on the device, any object id.  `CASES` lists
what tests/test_light_edges.py (host functions) and
tests/test_gpu_light_edges.py (the kernel) both run: each entry names its
scene, frame, rows, direction, lights, where its hit frame comes from, and the
*classes* of pixel, wave or intermediate value the numpy restatement
(tests/light_ref.py) must show in it, each with a minimum count.  A case
whose reference does not reach its counts fails before any parity is looked at.

`reference(pkg, oracle, name)` builds (once per process) everything both
modules compare with; `class_counts(ref)` counts the classes.  Importing this
module needs no GPU and no library.
"""
from types import SimpleNamespace

import numpy as np

import light_ref as lr
from gpu_support import H, W
from hit_ref import K_FAR, REF_DIR
from light_device import OUTPUTS  # the three output kinds both modules run every case on
from light_ref import ONE_LIGHT, THREE_LIGHTS, one_cube

F32 = np.float32
INT_MIN = -(1 << 31)
TINY = np.finfo(F32).tiny  # 2^-126: below it a float is denormal
LIMIT = 1 << 24  # the last width / row count with exact float pixel coordinates
WINDOW = 4096    # columns of the 2^24-wide row the restatement is computed for
CASES = {}
_REFS = {}


def _case(name, section, scene, size, d, lights, classes, rows=None, frame="hit_ref",
          render=False, scene_key=None):
    """scene: pkg -> Scene without lights (scene_key names it for the hit
    cache).  lights: a list of float4, or f(ref without lights) -> list.
    frame: "hit_ref" (the reference's frame), a function (valid frame, scene)
    -> (foreign frame, counts by class) or "far_columns".  render: the GPU
    module also renders the frame with fmt="hit" (generic_kernel) and checks it
    against hit_ref.  classes: {class: minimum count} ("lights": the exact
    number of lights)."""
    assert name not in CASES
    CASES[name] = dict(section=section, scene=scene, size=size, d=tuple(d), lights=lights,
                       classes=classes, rows=rows, frame=frame, render=render,
                       scene_key=scene_key or scene.__name__)


# ---------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------
def _moved(scene, dx=0.0, dy=0.0, z_scale=1.0):
    """`scene` with z scaled, then moved in x and y (float32, as a host would)."""
    s = type(scene)(scene.sphere_origins.copy(), scene.sphere_radius.copy(),
                    scene.sphere_colours.copy(), scene.cube_vertices.copy(),
                    scene.cube_colours.copy())
    for a in (s.sphere_origins, s.cube_vertices):
        a[..., 2] *= F32(z_scale)
        a[..., 0] += F32(dx)
        a[..., 1] += F32(dy)
    return s


def _with(pkg, scene, spheres=(), cubes=()):
    """`scene` plus (origin4, radius, colour4) spheres and (ops, colour4) cubes, last in order."""
    so = np.array([x[0] for x in spheres], F32).reshape(-1, 4)
    sr = np.array([x[1] for x in spheres], F32).reshape(-1)
    sc = np.array([x[2] for x in spheres], F32).reshape(-1, 4)
    cv = np.array([pkg.cube_packed(c[0]) for c in cubes], F32).reshape(-1, 36, 4)
    cc = np.array([c[1] for c in cubes], F32).reshape(-1, 4)
    return pkg.Scene(np.concatenate([scene.sphere_origins, so]),
                     np.concatenate([scene.sphere_radius, sr]),
                     np.concatenate([scene.sphere_colours, sc]),
                     np.concatenate([scene.cube_vertices, cv]),
                     np.concatenate([scene.cube_colours, cc]))


def base(pkg):
    return lr.base(pkg)


def base_mirrored(pkg):
    return _moved(lr.base(pkg), z_scale=-1.0)


def _rewound(scene):
    """Every second cube's triangles with v1 and v2 exchanged: the same
    surface, m = e1 x e2 reversed.  (A cube's faces all wind one way, so the
    facing step turns either every visible normal of a scene or none.)"""
    v = scene.cube_vertices.reshape(-1, 12, 3, 4)
    v[1::2] = v[1::2][:, :, [0, 2, 1]]
    return scene


def base_rewound(pkg):
    return _rewound(lr.base(pkg))


def base_mirrored_rewound(pkg):
    return _rewound(_moved(lr.base(pkg), z_scale=-1.0))


def base_near_rewound(pkg):
    """z / 25, as base_near: the reference's sphere test takes d for a unit
    vector, and with |d.xyz| well above 1 it marks every pixel of a sphere at
    the base scene's depths (the spheres then hide every cube); at depths of
    0.4 .. 4 the silhouettes stay finite.  Moved 3 columns right: under
    d = (1.5, 0.2, -1) a hit at depth t is seen 1.5 t columns left of its object."""
    return _rewound(_moved(lr.base(pkg), dx=3.0, z_scale=0.04))


def base_near(pkg):
    """z / 25 (tests/test_gpu_numeric_edges.py near_z): with |d.z| = 1e-4 the
    cubes' t = z / d.z stays below 300000 and they are drawn."""
    return _moved(lr.base(pkg), z_scale=0.04)


# the colour of the objects of section 2: at t = 0 a channel is (int)(255 k
# colour), up to 2.04e9, so one ulp of k (6e-8 of it) moves a channel by 100
BRIGHT = (8e6, 4e6, 2e6, 255)


def slab(ex, along_x=False):
    """A cube 200 long, 2 ex wide and 2 deep, tilted by 0.3 about its long
    axis, centred on column 0 (rows 0..63) or, along_x, on row 0 (columns
    0..63): every pixel centre of that column / row is inside it."""
    def build(pkg):
        if along_x:
            ops = [("scale", 200, ex, 1), ("rotate", 0, 0.3, 0), ("translate", 32, 0, -30)]
        else:
            ops = [("scale", ex, 200, 1), ("rotate", 0.3, 0, 0), ("translate", 0, 32, -30)]
        return one_cube(pkg, ops, BRIGHT)
    build.__name__ = f"slab_{ex:g}_{'x' if along_x else 'y'}"
    return build


def tiny_cube(pkg):
    """A cube of edge 2e-13 around (0, 0, -1e-12), turned about all three
    axes: every component of every face's m is a non-zero number of about
    4e-26 whose square is 0 in fp32."""
    return one_cube(pkg, [("scale", 1e-13, 1e-13, 1e-13), ("rotate", 0.3, 0.5, 0.2),
                          ("translate", 0, 0, -1e-12)], BRIGHT)


def tiny_sphere(r):
    def build(pkg):
        return lr.one_sphere(pkg, (0, 0, -r, 1), 1.5 * r, BRIGHT)
    build.__name__ = f"tiny_sphere_{r:g}"
    return build


def point_sphere(pkg):
    """Radius 1e-6 at depth 100: t = 100 - 1e-6 rounds to 100, the hit point
    is the centre itself and v = 0."""
    return lr.one_sphere(pkg, (1, 1, -100, 1), 1e-6, BRIGHT)


def lights_scene(pkg):
    """The base scene plus, nearer than all of it, a sphere centred on pixel
    (10, 70) and a cube face square to the rays around pixel (85, 10): under
    both centres the normal is exactly (0, 0, 1)."""
    return _with(pkg, lr.base(pkg),
                 spheres=[((10, 70, -8, 1), 5, (0.9, 0.8, 0.7, 255))],
                 cubes=[([("scale", 6, 6, 2), ("translate", 85, 10, -6)], (0.7, 0.8, 0.9, 255))])


# --- waves: width 64, a row is a wave ----------------------------------------
WAVE_H = 128
_R2 = 2.0 ** 0.5


def wave_scene(pkg):
    """Two cubes whose faces are square to the rays, turned by 45 degrees in
    the image plane.  A covers x + y < 65.5.  B, at the same depth, overlaps A
    by a hair (equal t there: A, the first, wins) and covers x + y > 65.5
    where x - y > -64.5; below that line nothing is hit.  So at width 64 the
    seam moves one lane per row: rows 0..2 are all A, row 3 is A but for lane
    63, row 65 is B but for lane 0, rows 66.. lose one more leading lane to
    the misses each, and row 127 has lane 63 alone in B.  One-pixel spheres in
    front of the cubes: the even lanes of row 1 (A between them), lanes 0..62
    of row 68 (lane 63 stays the wave's only cube lane), every lane of row 70."""
    a = 100.0
    # A: |u| <= a, v <= a with u = (x - y) / sqrt 2, v = (x + y) / sqrt 2 about its centre
    va = 65.5 / _R2 - a        # v of A's centre: its v = +a edge is x + y = 65.5
    ua = 0.0
    ub = -64.5 / _R2 + a       # B's u = -a edge is x - y = -64.5
    vb = va + 2 * a - 0.01

    def centre(u, v):
        return (u + v) / _R2, (v - u) / _R2

    cubes = [([("scale", a, a, 10), ("rotate", 0, 0, np.pi / 4),
               ("translate", *centre(u, v), -50)], col)
             for u, v, col in ((ua, va, (1.0, 0.5, 0.25, 255)), (ub, vb, (0.25, 0.5, 1.0, 255)))]
    lanes = [(x, 1) for x in range(0, 64, 2)] + [(x, 68) for x in range(63)] + \
            [(x, 70) for x in range(64)]
    spheres = [((x, y, -20, 1), 0.45, (0.3 + 0.01 * x, 0.9, 0.4, 255)) for x, y in lanes]
    return _with(pkg, pkg.Scene(), spheres=spheres, cubes=cubes)


# --- coordinate limits -------------------------------------------------------
def far_rows_scene(pkg):
    """The base scene moved down so that its rows 40..44 are the frame's last five."""
    return _moved(lr.base(pkg), dy=float(LIMIT - 45))


def far_columns_scene(pkg):
    """Large objects on row 0 in the last 4096 columns of a 2^24-wide frame."""
    x = float(LIMIT)
    return _with(pkg, pkg.Scene(),
                 spheres=[((x - 3000, 0, -500, 1), 400, (1.0, 0.5, 0.25, 255)),
                          ((x - 40, 3, -60, 1), 30, (0.25, 1.0, 0.5, 255))],
                 cubes=[([("scale", 600, 50, 10), ("rotate", 0.2, 0.3, 0.0),
                          ("translate", x - 1400, 0, -100)], (0.5, 0.25, 1.0, 255))])


# ---------------------------------------------------------------------------
# Lights
# ---------------------------------------------------------------------------
def seventy_lights(centre=(48.0, 40.0, 0.0), spread=60.0):
    """70 lights on a spiral around `centre`, most of them in front of the scene."""
    i = np.arange(70, dtype=np.float64)
    a = i * 2.399963
    r = spread * np.sqrt((i + 0.5) / 70)
    z = centre[2] + np.where(i % 7 == 6, -150.0, 30.0 + 3.0 * i)
    return np.stack([centre[0] + r * np.cos(a), centre[1] + r * np.sin(a), z,
                     np.ones_like(i)], 1).astype(F32).tolist()


def on_hit_points(ref):
    """A light exactly on the hit point of the first resolved cube pixel and of
    the first sphere pixel, and an ordinary one."""
    out = []
    for mask in (ref.cube & (ref.surf["triangle"] >= 0), ref.sphere):
        y, x = (int(v[0]) for v in np.nonzero(mask))
        out.append((ref.p[0][y, x], ref.p[1][y, x], ref.p[2][y, x], 1.0))
    return out + ONE_LIGHT


def octant_lights(ref):
    """Eight lights, one in each octant around the hit point of pixel (0, 0)."""
    p = [float(c[0, 0]) for c in ref.p]
    return [(p[0] + sx * 50, p[1] + sy * 50, p[2] + sz * 50, 1.0)
            for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]


SLAB_LIGHTS = [(5, 30, 20, 1), (1, 60, -60, 1)]  # one in front, one behind: 0 < k < 1
SLAB_X_LIGHTS = [(30, 5, 20, 1), (60, 1, -60, 1)]
NEAR_LIGHTS = [(2, 1, 3, 1), (-1, 0, 1, 1), (0, 2, -3, 1)]


# ---------------------------------------------------------------------------
# Foreign hit frames: a valid frame with words overwritten
# ---------------------------------------------------------------------------
def _pixels(mask, n):
    ys, xs = np.nonzero(mask)
    step = max(1, len(ys) // n)
    return list(zip(ys[::step][:n].tolist(), xs[::step][:n].tolist()))


_T_KINDS = ("t_up", "t_down", "t_nan", "t_inf", "t_minus_inf", "t_far", "object_-1")


def foreign_t(hits, scene):
    """On cube pixels and on sphere pixels: t one float up, one float down,
    NaN, +inf, -inf and 300000; and object -1 beside the real t.  The host
    accepts all of these."""
    h = np.array(hits)
    nc = scene.num_cubes
    counts = {}
    for kind, mask in (("cube", (h["object"] >= 0) & (h["object"] < nc)),
                       ("sphere", h["object"] >= nc)):
        px = _pixels(mask, 28)
        assert len(px) == 28
        for i, (y, x) in enumerate(px):
            t = hits["t"][y, x]
            m = i % 7
            if m == 6:
                h["object"][y, x] = -1
            else:
                h["t"][y, x] = (np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf)),
                                F32(np.nan), F32(np.inf), F32(-np.inf), K_FAR)[m]
            key = f"{kind}_{_T_KINDS[m]}"
            counts[key] = counts.get(key, 0) + 1
    return h, counts


def foreign_ids(hits, scene):
    """Object ids just outside [-1, nc + ns) on cube, sphere and miss pixels:
    nc + ns, nc + ns + 1 and -2.  The host refuses the frame; the kernel
    treats them as -1."""
    h = np.array(hits)
    nc, n = scene.num_cubes, scene.num_cubes + scene.num_spheres
    counts = {}
    for kind, mask in (("cube", (h["object"] >= 0) & (h["object"] < nc)),
                       ("sphere", h["object"] >= nc), ("miss", h["object"] == -1)):
        px = _pixels(mask, 12)
        assert len(px) == 12
        for i, (y, x) in enumerate(px):
            h["object"][y, x] = (n, n + 1, -2)[i % 3]
            key = f"{kind}_id_{('n', 'n+1', '-2')[i % 3]}"
            counts[key] = counts.get(key, 0) + 1
    return h, counts


_FOREIGN_T = {f"{k}_{m}": 4 for k in ("cube", "sphere") for m in _T_KINDS}
_FOREIGN_T["cube_unresolved"] = 20  # no triangle reproduces the five kinds of t that are not 300000
_FOREIGN_IDS = {f"{k}_id_{m}": 4 for k in ("cube", "sphere", "miss") for m in ("n", "n+1", "-2")}


# ---------------------------------------------------------------------------
# The table
# ---------------------------------------------------------------------------
_OBLIQUE = {"cube": 100, "sphere": 100, "miss": 100, "cube_flipped": 1, "cube_not_flipped": 1}
_DIR = {"cube": 100, "sphere": 100, "miss": 100}
_S = (W, H)

# 1. directions: the base scene, 96 x 80, three lights
_case("dir_oblique", 1, base_rewound, _S, (0.3, -0.2, -1, -1), THREE_LIGHTS, _OBLIQUE,
      render=True)
_case("dir_oblique_mirrored", 1, base_mirrored_rewound, _S, (-0.3, 0.2, 1, -1), THREE_LIGHTS,
      _OBLIQUE, render=True)
_case("dir_oblique_wide", 1, base_near_rewound, _S, (1.5, 0.2, -1, -1), THREE_LIGHTS, _OBLIQUE,
      render=True)
_case("dir_zeros_-0+0-1", 1, base, _S, (-0.0, 0.0, -1, -1), THREE_LIGHTS, _DIR)
_case("dir_zeros_+0-0+1", 1, base_mirrored, _S, (0.0, -0.0, 1, -1), THREE_LIGHTS, _DIR)
_case("dir_scaled_-4", 1, base_near, _S, (0, 0, -4, -1), THREE_LIGHTS, _DIR)
_case("dir_scaled_-1e-4", 1, base_near, _S, (0, 0, -1e-4, -1), THREE_LIGHTS, _DIR)
# the reference's sphere test marks every pixel: all of them sphere pixels, every normal NaN
_case("dir_scaled_-1e30", 1, base, _S, (0, 0, -1e30, -1), THREE_LIGHTS,
      {"sphere": W * H, "sphere_nan_normal": W * H})

# 2a. denormal m*m: (ex, layout).  "column": 2 x 64, the slab's pixels are the
# even lanes of two waves; "waves": 64 x 64, lane 0 of 64 waves; "lanes":
# 64 x 1, the 64 lanes of one wave
_BIG = (0, 0, -1e15, 0)
# (at ex = 1e-21 the squares, 5.6e-38 and 5.8e-37, are still normal numbers, two
# and six binades above 2^-126; from 1e-22 on they and their sum are denormal,
# and at 1e-23 the smaller square keeps 12 bits)
for _ex, _cls in ((1e-19, "msq_normal"), (1e-21, "msq_near_denormal"), (1e-22, "msq_denormal"),
                  (1e-23, "msq_denormal")):
    _c = {"cube": 64, _cls: 64, "normal_finite": 64, "k_partial": 1}
    _case(f"denormal_{_ex:g}_column", 2, slab(_ex), (2, 64), _BIG, SLAB_LIGHTS, _c)
    _case(f"denormal_{_ex:g}_waves", 2, slab(_ex), (64, 64), _BIG, SLAB_LIGHTS,
          dict(_c, waves_with_one_cube_lane=64))
    _case(f"denormal_{_ex:g}_lanes", 2, slab(_ex, True), (64, 1), _BIG, SLAB_X_LIGHTS,
          dict(_c, waves_all_one_cube=1))
# 2b. m*m = 0: len = 0.  The slab's m.x is 0, so its normal is (NaN, inf, inf)
# and every cosine NaN; the tiny cube's is (inf, inf, inf) in some signs
_case("underflow_slab", 2, slab(1e-30), (2, 64), (0, 0, -1e25, 0), SLAB_LIGHTS,
      {"cube": 64, "msq_zero": 64, "normal_nan": 64, "normal_inf": 64, "c_nan": 64})
_case("underflow_tiny_cube", 2, tiny_cube, (2, 2), (0, 0, -1e25, 0), octant_lights,
      {"cube": 1, "msq_zero": 1, "normal_all_inf": 1, "c_plus_inf": 1, "c_minus_inf": 1,
       "c_nan": 1, "k_clamped_from_inf": 1})
# 2c. tiny spheres on pixel (0, 0), and v = 0
for _r in (1e-18, 1e-19, 1e-20, 1e-21, 1e-22):
    _case(f"tiny_sphere_{_r:g}", 2, tiny_sphere(_r), (4, 4), REF_DIR, NEAR_LIGHTS,
          {"sphere": 1, "t_tiny_negative": 1, "normal_finite": 1})
_case("sphere_hit_point_is_centre", 2, point_sphere, (4, 4), REF_DIR, NEAR_LIGHTS,
      {"sphere": 1, "sphere_nan_normal": 1})

# 3. lights
_HITS = {"cube": 100, "sphere": 100, "miss": 100}
_case("light_on_hit_points", 3, lights_scene, _S, REF_DIR, on_hit_points,
      dict(_HITS, ll_zero=2, c_nan=2))
_case("light_1e20", 3, lights_scene, _S, REF_DIR, [(1e20, 40, 200, 1), (48, -1e20, 1e20, 1)],
      dict(_HITS, ll_inf=200, c_zero=200))
_case("light_inf_nan", 3, lights_scene, _S, REF_DIR,
      [(np.inf, 40, 200, 1), (48, -np.inf, 200, 1), (48, 40, np.nan, 1), (48, 40, 200, 1)],
      dict(_HITS, ll_inf=200, c_nan=200, k_partial=100))
_case("light_denormal", 3, lights_scene, _S, REF_DIR,
      [(1e-40, 1e-45, 200, 1), (-1e-42, 80, 1e-39, 1)], dict(_HITS, k_partial=100))
_case("light_w_nan", 3, lights_scene, _S, REF_DIR,
      [tuple(l[:3]) + (np.nan,) for l in THREE_LIGHTS], dict(_HITS, k_partial=100, k_clamped=100))
_case("light_seventy", 3, lights_scene, _S, REF_DIR, seventy_lights((250.0, 40.0, -40.0), 60.0),
      dict(_HITS, k_clamped=100, k_partial=100, lights=70))
_case("light_sum_exactly_one", 3, lights_scene, _S, REF_DIR,
      [(10, 70, -60, 1), (10, 70, 40, 1), (85, 10, -90, 1)],
      dict(_HITS, sum_exactly_one=1, k_partial=100))

# 4. foreign hit frames
_case("foreign_t", 4, base, _S, REF_DIR, THREE_LIGHTS, dict(_HITS, **_FOREIGN_T), frame=foreign_t)
_case("foreign_ids", 4, base, _S, REF_DIR, THREE_LIGHTS, dict(_HITS, **_FOREIGN_IDS),
      frame=foreign_ids)

# 5. wave composition
_W64 = {"waves_all_A": 1, "waves_A_lane63_B": 1, "waves_B_lane0_A": 1,
        "waves_only_cube_lane_63_after_miss": 1, "waves_only_cube_lane_63_after_sphere": 1,
        "waves_interleaved": 1, "waves_all_sphere": 1}
_W61 = {"waves_two_cubes": 50, "waves_first_lane_no_cube": 10, "last_wave_partial_with_cube": 1}
for _n, _l in ((0, []), (1, [(30, 40, 60, 1)]), (70, seventy_lights((32, 60, 0), 50))):
    _case(f"waves_64_{_n}_lights", 5, wave_scene, (64, WAVE_H), REF_DIR, _l, dict(_W64, lights=_n))
    _case(f"waves_61_{_n}_lights", 5, wave_scene, (61, WAVE_H), REF_DIR, _l, dict(_W61, lights=_n),
          rows=(0, 100))

# 6. coordinate limits
_case("limit_rows", 6, far_rows_scene, (67, LIMIT), REF_DIR, [(30, LIMIT - 3, 200, 1)],
      {"cube": 10, "sphere": 10, "miss": 10, "k_partial": 10}, rows=(LIMIT - 5, LIMIT))
_case("limit_columns", 6, far_columns_scene, (LIMIT, 1), REF_DIR, [(LIMIT - 1500, 0, 300, 1)],
      {"hit": 1000, "cube": 100, "sphere": 100, "miss": 100, "k_partial": 100},
      frame="far_columns")


# ---------------------------------------------------------------------------
# The reference of a case
# ---------------------------------------------------------------------------
def _freeze(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


def _restate(oracle, scene, hits, rb, d, x_begin=0):
    """Everything the restatement says about a frame whose ids are in range."""
    nc, ns = scene.num_cubes, scene.num_spheres
    obj = hits["object"]
    assert ((obj >= -1) & (obj < nc + ns)).all()
    r = SimpleNamespace(scene=scene, hits=hits, rb=rb, d=d, x_begin=x_begin)
    r.cube, r.sphere, r.miss = (obj >= 0) & (obj < nc), obj >= nc, obj == -1
    r.p = lr.hit_points(hits, rb, d, x_begin)
    r.flipped = np.zeros(hits.shape, bool)
    r.surf = lr.surfaces_ref(oracle, scene, hits, rb, d, x_begin, flipped=r.flipped)
    r.terms = {}
    r.k = lr.light_factor_ref(scene, hits, r.surf, rb, d, x_begin, terms=r.terms)
    r.lit = lr.lit_ref(oracle, scene, hits, rb, d, surf=r.surf, x_begin=x_begin, k=r.k)
    r.rgba8 = oracle.pack_rgba8(r.lit)
    return r


def reference(pkg, oracle, name):
    """The case's scene (with its lights), the frame `hits` the functions
    under test are given, whether the host accepts it, and the restatement
    of it: `surf`, `lit`, `rgba8`, the classes' ingredients.  For a foreign
    frame the restatement is of `hits` with the out-of-range ids as -1.  For
    "far_columns" `hits` is the whole 2^24-wide row and the restatement covers
    its last WINDOW columns (`x_begin`); everything before is a miss."""
    if name in _REFS:
        return _REFS[name]
    c = CASES[name]
    (w, h), d = c["size"], c["d"]
    rb, re = c["rows"] or (0, h)
    bare = c["scene"](pkg)
    window = c["frame"] == "far_columns"
    x_begin, ww = (w - WINDOW, WINDOW) if window else (0, w)
    valid = lr.cached_hits(oracle, c["scene_key"], bare, ww, h, (rb, re), d, x_begin)
    lights = c["lights"]
    if callable(lights):
        lights = lights(_restate(oracle, bare, valid, rb, d, x_begin))
    scene = lr.with_lights(bare, lights)
    given, counts, host_ok = valid, {}, True
    if callable(c["frame"]):
        given, counts = c["frame"](valid, scene)
        obj = given["object"]
        outside = (obj < -1) | (obj >= scene.num_cubes + scene.num_spheres)
        host_ok = not outside.any()
        mapped = np.array(given)
        mapped["object"][outside] = -1
    else:
        mapped = valid
    r = _restate(oracle, scene, mapped, rb, d, x_begin)
    r.name, r.w, r.h, r.rows = name, w, h, (rb, re)
    r.counts, r.host_ok, r.valid = counts, host_ok, valid
    if window:  # the whole row: misses, then the window
        given = np.empty((re - rb, w), valid.dtype)
        given["t"], given["object"] = K_FAR, -1
        given[:, x_begin:] = valid
    r.given = given
    _REFS[name] = _freeze(r)
    return r


# ---------------------------------------------------------------------------
# Classes
# ---------------------------------------------------------------------------
def tri_msq(scene):
    """Per cube and triangle: m = e1 x e2 (nc x 12 x 3) and (m.x*m.x + m.y*m.y)
    + m.z*m.z (nc x 12), in fp32 as §3.1a writes them."""
    v = np.ascontiguousarray(scene.cube_vertices, F32).reshape(-1, 12, 3, 4)[..., :3]
    e1, e2 = v[:, :, 1] - v[:, :, 0], v[:, :, 2] - v[:, :, 0]
    with np.errstate(all="ignore"):
        m = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1],
                      e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                      e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)
        return m, (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]


def tri_regime(scene):
    """Per cube and triangle, where normalise's squares and sums lie: 1 every
    one a normal number of at least 2^-120, 2 every one normal but one within
    six binades of the denormals, 3 a square or a partial sum denormal, 4 the
    sum 0 though m is not."""
    m, msq = tri_msq(scene)
    with np.errstate(all="ignore"):
        sq = m * m
        parts = np.concatenate([sq, (sq[..., 0] + sq[..., 1])[..., None], msq[..., None]], -1)
    denormal = ((parts > 0) & (parts < TINY)).any(-1)
    out = np.where(((parts > 0) & (parts < F32(2.0 ** -120))).any(-1), 2, 1)
    out = np.where(denormal, 3, out)
    return np.where((msq == 0) & (m != 0).any(-1), 4, out).astype(np.int8)


def _waves(r):
    """The frame's object ids by wave (n_waves x 64, -9 in the lanes past the
    last pixel), cube lanes, sphere lanes."""
    obj = r.hits["object"].reshape(-1)
    pad = (-len(obj)) % 64
    o = np.concatenate([obj, np.full(pad, -9, obj.dtype)]).reshape(-1, 64)
    nc = r.scene.num_cubes
    return o, (o >= 0) & (o < nc), o >= nc


def class_counts(r):
    """{class: count} of everything any case asks for, from the restatement alone."""
    s, nc = r.surf, r.scene.num_cubes
    hit = ~r.miss
    normal = np.stack([s["nx"], s["ny"], s["nz"]], -1)
    resolved = r.cube & (s["triangle"] >= 0)
    regime = np.zeros(r.hits.shape, np.int8)
    regime[resolved] = tri_regime(r.scene)[r.hits["object"][resolved], s["triangle"][resolved]]
    out = dict(r.counts)
    out.update({
        "hit": hit.sum(), "cube": resolved.sum(), "cube_unresolved": (r.cube & ~resolved).sum(),
        "sphere": r.sphere.sum(), "miss": r.miss.sum(),
        "cube_flipped": (resolved & r.flipped).sum(),
        "cube_not_flipped": (resolved & ~r.flipped).sum(),
        "sphere_nan_normal": (r.sphere & np.isnan(normal).all(-1)).sum(),
        "normal_finite": (hit & np.isfinite(normal).all(-1) & (normal != 0).any(-1)).sum(),
        "normal_nan": (hit & np.isnan(normal).any(-1)).sum(),
        "normal_inf": (hit & np.isinf(normal).any(-1)).sum(),
        "normal_all_inf": (hit & np.isinf(normal).all(-1)).sum(),
        "msq_normal": (regime == 1).sum(), "msq_near_denormal": (regime == 2).sum(),
        "msq_denormal": (regime == 3).sum(), "msq_zero": (regime == 4).sum(),
        "t_tiny_negative": (hit & (r.hits["t"] < 0) & (r.hits["t"] > -1e-17)).sum(),
        "lights": len(r.scene.lights),
    })
    if len(r.scene.lights):
        ll, c, total = r.terms["ll"], r.terms["c"], r.terms["sum"]
        out.update({
            "ll_zero": ((ll == 0) & hit).sum(), "ll_inf": (np.isinf(ll) & hit).any(0).sum(),
            "c_nan": (np.isnan(c) & hit).any(0).sum(), "c_zero": ((c == 0) & hit).any(0).sum(),
            "c_plus_inf": ((c == np.inf) & hit).sum(), "c_minus_inf": ((c == -np.inf) & hit).sum(),
            "k_partial": (hit & (total > 0) & (total < 1)).sum(),
            "k_clamped": (hit & (total > 1)).sum(),
            "k_clamped_from_inf": (hit & (total == np.inf) & (r.k == 1)).sum(),
            "sum_exactly_one": (hit & (total == 1) & (c > 0).any(0)).sum(),
        })
    o, cube, sph = _waves(r)
    a, b = o == 0, o == 1
    only63 = cube[:, 63] & ~cube[:, :63].any(1)
    one_cube_id = np.array([len(set(row[cm].tolist())) == 1 for row, cm in zip(o, cube)])
    switches = (cube[:, 1:] != cube[:, :-1]).sum(1)
    out.update({
        "waves_all_A": a.all(1).sum(),
        "waves_A_lane63_B": (a[:, :63].all(1) & b[:, 63]).sum(),
        "waves_B_lane0_A": (a[:, 0] & b[:, 1:].all(1)).sum(),
        "waves_only_cube_lane_63_after_miss": (only63 & (o[:, 0] == -1)).sum(),
        "waves_only_cube_lane_63_after_sphere": (only63 & sph[:, 0]).sum(),
        "waves_interleaved": (one_cube_id & (switches >= 40) & (cube | sph).all(1)).sum(),
        "waves_all_sphere": sph.all(1).sum(),
        "waves_two_cubes": (a.any(1) & b.any(1)).sum(),
        "waves_first_lane_no_cube": (~cube[:, 0] & cube.any(1)).sum(),
        "last_wave_partial_with_cube": int((o[-1] == -9).any() and cube[-1].any()),
        "waves_with_one_cube_lane": (cube.sum(1) == 1).sum(),
        "waves_all_one_cube": (cube.all(1) & one_cube_id).sum(),
    })
    return {k: int(v) for k, v in out.items()}


def missing_classes(r):
    """'' or the classes of the case whose count the restatement does not reach."""
    have = class_counts(r)
    short = {k: (have.get(k, 0), need) for k, need in CASES[r.name]["classes"].items()
             if (have.get(k, 0) != need if k == "lights" else have.get(k, 0) < need)}
    return "" if not short else f"{r.name}: (found, needed) {short}"


# ---------------------------------------------------------------------------
# The comparison rule
# ---------------------------------------------------------------------------
def surfaces_differ(got, want):
    """'' or where two surface frames differ: `triangle` exact; a normal
    component as raw words wherever `want` holds a number (signed zeros,
    denormals and infinities included), NaN where `want` holds NaN (the sign of
    a NaN an operation creates is not specified)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"layout {got.dtype} {got.shape} vs {want.dtype} {want.shape}"
    bad = got["triangle"] != want["triangle"]
    for f in ("nx", "ny", "nz"):
        nan = np.isnan(want[f])
        bad |= np.where(nan, ~np.isnan(got[f]), got[f].view(np.uint32) != want[f].view(np.uint32))
    if not bad.any():
        return ""
    ys, xs = np.nonzero(bad)
    return (f"{int(bad.sum())} pixels differ, first at (x={xs[0]}, y={ys[0]}): "
            f"{got[ys[0], xs[0]]} vs {want[ys[0], xs[0]]}")


def differ(what, got, want):
    """The rule for one output kind: lit frames are raw words, no exemption."""
    return surfaces_differ(got, want) if what == "surface" else lr.eq(got, want)
