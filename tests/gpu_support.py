"""What the GPU tests share -- TEST INFRASTRUCTURE ONLY.

The diagnostics knobs of `RayTracer` in one table with one scope that sets and
resets them (`knobs`), the path matrix every parity test walks (`PATHS`,
`render_all_paths`), and the scenes, uploads and comparisons more than one
test module uses.  Importing it needs no GPU and no library.
"""
import contextlib
import os

import numpy as np

F32 = np.float32
W, H = 96, 80
REF_DIR = (0.0, 0.0, -1.0, -1.0)
THREADS = min(16, os.cpu_count() or 1)

# ---------------------------------------------------------------------------
# The diagnostics knobs
# ---------------------------------------------------------------------------
# every set_<name> of RayTracer and the argument that means "the library's
# default" (negative: the compiled-in default of the cull knobs)
DEFAULTS = dict(small_path=True, small_fused=1, trace_bin=0, trace_split=0, coarse_cull=-1,
                coarse_cull_tri=-1, coarse_cull_overdraw=-1, tile_variant=0, coarse_waves=0,
                bin_masks=True, list_budget=0)
# setters `knobs` leaves alone (test_knob_table_is_complete: there is no third kind)
KNOB_EXCLUSIONS = (
    "trace_mode",    # exists in RT_DIAG builds only
    "verdict_copy",  # can return RT_ERR_UNSUPPORTED; its own test sets it, on its own context
)


def _set_all(rt, values):
    for name, value in values.items():
        getattr(rt, "set_" + name)(value)


@contextlib.contextmanager
def _knob_scope(rt, values):
    try:
        _set_all(rt, values)
        yield rt
    finally:
        _set_all(rt, DEFAULTS)


def knobs(rt, **settings):
    """`with knobs(rt, trace_split=2, ...):` -- inside the block every knob of
    DEFAULTS holds its default or the value named here; afterwards, however
    the block ends, every one holds its default.  `rt`: any RayTracer.  A
    name that is not in DEFAULTS is a TypeError, before any setter is called."""
    unknown = sorted(set(settings) - set(DEFAULTS))
    if unknown:
        raise TypeError(f"no such diagnostics knob: {', '.join(unknown)}")
    return _knob_scope(rt, dict(DEFAULTS, **settings))


# ---------------------------------------------------------------------------
# Comparing frames
# ---------------------------------------------------------------------------
def diff_report(got, want):
    bad = (got != want).any(-1) if got.ndim == 3 else (got != want)
    n = int(bad.sum())
    if n:
        ys, xs = np.nonzero(bad)
        return (f"{n} pixels differ, first at (x={xs[0]}, y={ys[0]}): "
                f"{got[ys[0], xs[0]]} vs {want[ys[0], xs[0]]}")
    return ""


def oracle_frame(oracle, scene, w, h, rows=None, fmt="i32x4", **kw):
    """The oracle's frame in the format a render was asked for."""
    want = oracle.trace(scene, w, h, rows=rows, **kw)
    return oracle.pack_rgba8(want) if fmt == "rgba8" else want


# ---------------------------------------------------------------------------
# The path matrix: every kernel that shades pixels, by the diagnostics knobs.
# (name, render path, knobs, kernel it must run)
# ---------------------------------------------------------------------------
_COARSE = dict(small_path=False, trace_bin=2)
# every depth cull forced on: every bin, spheres and triangles, every frame
FORCED_CULLS = dict(coarse_cull=1, coarse_cull_tri=1, coarse_cull_overdraw=0)
PATHS = [
    ("generic", "generic", dict(), "generic_kernel"),
    ("frame_small", "auto", dict(small_fused=2), "frame_small_kernel"),
    ("trace_small", "auto", dict(small_fused=0), "trace_small_kernel"),
    ("trace3", "auto", dict(_COARSE, trace_split=1), "trace3_kernel"),
    ("trace3_culls", "auto", dict(_COARSE, trace_split=1, **FORCED_CULLS), "trace3_kernel"),
    ("trace3_split2", "auto", dict(_COARSE, trace_split=2), "trace3_split_kernel"),
    ("trace3_split4", "auto", dict(_COARSE, trace_split=4), "trace3_split_kernel"),
    ("trace_bin", "auto", dict(small_path=False, trace_bin=1), "trace_bin_kernel"),
    ("trace3_wide", "auto", dict(_COARSE, trace_split=1, tile_variant=2), "trace3_kernel"),
    ("trace3_wide_culls", "auto", dict(_COARSE, trace_split=1, tile_variant=2, **FORCED_CULLS),
     "trace3_kernel"),
]
FUSED_MAX_PRIMS = 128  # frame_small_kernel: at most two 64-primitive chunks


def n_prims(scene):
    return 12 * scene.num_cubes + scene.num_spheres


def render_all_paths(rt, oracle, scene, w, h, rows=None, ray_dir=None, want=None,
                     fused_scene=None, fused_want=None, label=""):
    """Render `scene` through every entry of PATHS in both formats and compare
    each frame bit for bit with the oracle's (`want`, computed here when not
    given; RGBA8 against oracle.pack_rgba8 of it).  Asserts the path taken
    and the kernel that ran.  frame_small_kernel takes at most 128
    primitives: larger scenes must bring a `fused_scene` variant of at most
    that many, rendered in its place on that path (no scene is excused).
    An empty scene runs no small-scene kernel and no trace_bin_kernel: it
    goes to the coarse path's trace (trace3_split_kernel on these small
    frames unless the split knob is 1).  Each entry runs in its own `knobs`
    scope.  Returns the number of frames compared."""
    kw = dict(rows=rows, ray_dir=None if ray_dir is None else np.asarray(ray_dir, F32))
    if want is None:
        want = oracle.trace(scene, w, h, **kw)
    wants = {id(scene): (want, oracle.pack_rgba8(want))}
    if n_prims(scene) > FUSED_MAX_PRIMS:
        assert fused_scene is not None and n_prims(fused_scene) <= FUSED_MAX_PRIMS, \
            f"{label}: {n_prims(scene)} primitives need a <= 128-primitive variant"
        if fused_want is None:
            fused_want = oracle.trace(fused_scene, w, h, **kw)
        wants[id(fused_scene)] = (fused_want, oracle.pack_rgba8(fused_want))
    compared = 0
    for name, path, settings, kernel in PATHS:
        sc = scene
        if name == "frame_small" and n_prims(scene) > FUSED_MAX_PRIMS:
            sc = fused_scene
        if n_prims(sc) == 0 and path != "generic":
            kernel = "trace3_kernel" if settings.get("trace_split") == 1 else "trace3_split_kernel"
        with knobs(rt, **settings):
            for fmt, expect in zip(("i32x4", "rgba8"), wants[id(sc)]):
                got, t = rt.render(sc, w, h, fmt=fmt, path=path, **kw)
                where = f"{label} {name}/{fmt}"
                assert t.path == ("generic" if path == "generic" else "binned"), where
                assert rt.last_kernel() == kernel, f"{where}: ran {rt.last_kernel()}"
                assert got.shape == expect.shape, where
                assert not diff_report(got, expect), f"{where}: {diff_report(got, expect)}"
                compared += 1
    return compared


# ---------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------
def base_scene(pkg, fused=False):
    """The base scene: 40 spheres + 10 cubes (160 primitives) on 96 x 80.
    fused=True: its first 20 spheres and 8 cubes (116 primitives), the
    variant frame_small_kernel renders; the case builders add at most 12."""
    s = pkg.Scene.synthetic(W, H, 40, 10, seed=7, k=0.3)
    if fused:
        s = pkg.Scene(s.sphere_origins[:20], s.sphere_radius[:20], s.sphere_colours[:20],
                      s.cube_vertices[:8], s.cube_colours[:8])
    return s


def tie_scene(pkg, w, h, n, seed):
    """Dense spheres plus exact duplicates (equal t everywhere: the first in
    order must win, MainState.cpp:386-391) and concentric copies."""
    rng = np.random.default_rng(seed)
    so = np.zeros((n, 4), np.float32)
    so[:, 0] = rng.uniform(0, w, n)
    so[:, 1] = rng.uniform(0, h, n)
    so[:, 2] = -rng.uniform(20, 100, n)
    r = rng.uniform(5, 30, n).astype(np.float32) * (w / 64)
    sc = np.concatenate([rng.uniform(0.05, 1, (n, 3)), np.full((n, 1), 255)], 1).astype(np.float32)
    dup = rng.choice(n, n // 8, replace=False)
    so = np.concatenate([so, so[dup]])
    r = np.concatenate([r, r[dup]])
    sc = np.concatenate([sc, sc[dup][:, [2, 0, 1, 3]]])
    return pkg.Scene(so, r, sc)


def cube_tie_scene(pkg, w, h, seed, spheres=30, cubes=160, duplicates=40):
    """Dense cubes plus exact duplicates recoloured (their triangles tie at
    every pixel: the first cube must win, MainState.cpp:386-391), and a few
    spheres."""
    base = pkg.Scene.synthetic(w, h, spheres, cubes, seed=seed, k=w / 640 * 3)
    rng = np.random.default_rng(seed)
    dup = rng.choice(len(base.cube_vertices), duplicates, replace=False)
    cv = np.concatenate([base.cube_vertices, base.cube_vertices[dup]])
    cc = np.concatenate([base.cube_colours, base.cube_colours[dup][:, [2, 0, 1, 3]]])
    return pkg.Scene(base.sphere_origins, base.sphere_radius, base.sphere_colours, cv, cc)


# the golden fixtures with whole frames (config 3's holds a hash only)
SMALL_FIXTURES = ["scene1_640x480", "scene2_640x480", "scene3_640x480", "config1_512x512",
                  "config2_1920x1080", "config2s_1920x1080"]


def scene_from(pkg, spheres=(), cubes=()):
    so = np.array([s[0] for s in spheres], F32).reshape(-1, 4)
    sr = np.array([s[1] for s in spheres], F32)
    sc = np.array([s[2] for s in spheres], F32).reshape(-1, 4)
    cv = np.array([pkg.cube_packed(c[0]) for c in cubes], F32).reshape(-1, 36, 4)
    cc = np.array([c[1] for c in cubes], F32).reshape(-1, 4)
    return pkg.Scene(so, sr, sc, cv, cc)


# name: scene_from's arguments (the device tests and the reference kernel's)
EDGE_CASES = {
    "empty": dict(),
    "spheres_only": dict(spheres=[((40, 30, -50, 1), 20, (1, .5, .25, 255)),
                                  ((60, 30, -20, 1), 25, (.1, .9, .3, 255))]),
    "cubes_only": dict(cubes=[([("scale", 15, 15, 15), ("rotate", .3, .7, .1),
                                ("translate", 50, 35, -40)], (.2, .4, .9, 255))]),
    # origin inside a sphere and cubes crossing z = 0: t < 0, values > 255
    "behind_origin": dict(spheres=[((50, 40, -10, 1), 40, (1, 1, 1, 255))],
                          cubes=[([("scale", 30, 30, 30), ("rotate", .5, .2, .9),
                                   ("translate", 30, 30, 5)], (1, .5, 1, 255))]),
    # far objects: shade < 0, negative int channels
    "far": dict(spheres=[((50, 40, -900, 1), 30, (1, 1, 1, 255))],
                cubes=[([("scale", 20, 20, 20), ("rotate", .1, .2, .3),
                         ("translate", 20, 20, -2000)], (1, 1, 1, 255))]),
    # spheres in front of the origin plane never hit (tca < 0), and off-screen
    "culled": dict(spheres=[((50, 40, 30, 1), 30, (1, 1, 1, 255)),
                            ((-500, 40, -30, 1), 30, (1, 1, 1, 255)),
                            ((50, 4000, -30, 1), 30, (1, 1, 1, 255))]),
    # edge-on slivers: |det| near EPSILON, culling bound must stay conservative
    "slivers": dict(cubes=[([("scale", 40, 1e-3, 40), ("translate", 50, 40.5, -30)],
                            (1, .2, .2, 255)),
                           ([("scale", 40, 1e-3, 40), ("rotate", 1e-4, 0, 0.3),
                             ("translate", 50, 30, -30)], (1, .6, .2, 255)),
                           ([("scale", 1e-4, 30, 30), ("rotate", 0, 1e-5, 0),
                             ("translate", 30, 20, -30)], (.2, 1, .2, 255)),
                           ([("scale", 3e-3, 3e-3, 3e-3), ("translate", 10, 10, -5)],
                            (.7, .7, .2, 255)),
                           ([("scale", 25, 25, 2e-6), ("translate", 70, 50, -30)],
                            (.2, .2, 1, 255))]),
    # exact ties: identical spheres / duplicate cubes, first primitive must win
    "ties": dict(spheres=[((50, 40, -50, 1), 20, (1, 0, 0, 255)),
                          ((50, 40, -50, 1), 20, (0, 1, 0, 255))],
                 cubes=[([("scale", 10, 10, 10), ("translate", 20, 20, -30)], (0, 0, 1, 255)),
                        ([("scale", 10, 10, 10), ("translate", 20, 20, -30)], (1, 1, 0, 255))]),
    # sphere origin w != 1 and a zero radius
    "odd_w": dict(spheres=[((50, 40, -50, 3), 20, (1, .3, .3, 255)),
                           ((20, 20, -50, 1), 0, (1, 1, 1, 255))]),
    # depth culling: a big front sphere, layers behind it (culled once the
    # tile is covered), spheres whose lower bound equals the front depth,
    # a later nearer one that must still win, t0 == 0 and t < 0 spheres
    "depth_layers": dict(spheres=[((50, 40, -30, 1), 60, (1, .2, .2, 255))] +
                         [((45 + 3 * i, 35 + 2 * i, -30 - i, 1), 20 + i, (.2, 1, .2, 255))
                          for i in range(12)] +
                         [((50, 40, -30, 1), 60, (0, 0, 1, 255)),
                          ((50, 40, -90, 1), 60, (0, 1, 1, 255)),
                          ((30, 30, -95, 1), 90, (1, 1, 0, 255)),
                          ((60, 50, -10, 1), 10, (1, 0, 1, 255)),
                          ((20, 60, -4, 1), 4, (.5, .5, .5, 255))]),
}


SCENE_ARRAYS = ("sphere_origins", "sphere_radius", "sphere_colours", "cube_vertices",
                "cube_colours", "lights")


def device_scene(torch, scene):
    """`scene` on cuda:0: (dict for the *_device calls, the tensors that own
    the memory).  Empty arrays (lights, mostly) are not uploaded: their
    address stays NULL."""
    keep = {k: torch.from_numpy(np.array(getattr(scene, k), F32)).to("cuda:0")
            for k in SCENE_ARRAYS if getattr(scene, k).size}
    ds = {k: v.data_ptr() for k, v in keep.items()}
    ds.update(num_spheres=scene.num_spheres, num_cubes=scene.num_cubes,
              num_lights=len(scene.lights))
    return ds, keep
