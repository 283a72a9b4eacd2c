"""RT_FORMAT_HIT on the GPU: every pixel-writing kernel returns the
reference's (t, object) per pixel.

The reference frame is tests/hit_ref.py (the oracle's per-primitive functions
in `collide`'s loop order; tests/test_hit_format.py pins it to the oracle's
colour frames).  Frames are compared as raw 32-bit words, both fields.  An
object id sees what no colour frame can: which of two candidates of equal t
and equal colour won (strict `<`, cubes before spheres, the
split kernel's merge, the depth culls' strict bounds).
"""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from gpu_support import FUSED_MAX_PRIMS, PATHS, base_scene, device_scene, knobs, n_prims
from hit_ref import K_FAR, distinct_colours, hit_ref, words

gpu = pytest.mark.gpu
F32 = np.float32
_CACHE = {}


def _ref(oracle, key, scene, w, h, rows=None):
    """hit_ref, computed once per (scene key, frame) and never modified."""
    k = (key, w, h, rows)
    if k not in _CACHE:
        r = hit_ref(oracle, scene, w, h, rows=rows)
        r.setflags(write=False)
        _CACHE[k] = r
    return _CACHE[k]


def _diff(got, want):
    bad = (words(got) != words(want)).any(-1)
    if not bad.any():
        return ""
    ys, xs = np.nonzero(bad)
    return (f"{int(bad.sum())} pixels differ, first at (x={xs[0]}, y={ys[0]}): "
            f"{got[ys[0], xs[0]]} vs {want[ys[0], xs[0]]}")


def _render_paths(pkg, rt, scene, want, w, h, rows=None, fused=None, only=None, label=""):
    """`scene` as a hit frame through every entry of PATHS (`only`: those
    names), each compared with `want`; frame_small_kernel takes `fused` =
    (scene, want) when the scene has more than 128 primitives.  Asserts the
    kernel that ran.  Returns the number of frames compared."""
    n = 0
    for name, path, settings, kernel in PATHS:
        if only is not None and name not in only:
            continue
        sc, expect = scene, want
        if name == "frame_small" and n_prims(scene) > FUSED_MAX_PRIMS:
            sc, expect = fused
            assert n_prims(sc) <= FUSED_MAX_PRIMS
        if n_prims(sc) == 0 and path != "generic":
            kernel = "trace3_kernel" if settings.get("trace_split") == 1 else "trace3_split_kernel"
        with knobs(rt, **settings):
            got, t = rt.render(sc, w, h, rows=rows, fmt="hit", path=path)
            where = f"{label} {name}"
            assert t.path == ("generic" if path == "generic" else "binned"), where
            assert rt.last_kernel() == kernel, f"{where}: ran {rt.last_kernel()}"
            assert got.dtype == pkg.HIT_DTYPE and got.shape == expect.shape, where
            assert not _diff(got, expect), f"{where}: {_diff(got, expect)}"
            n += 1
    return n


# --- 1. every kernel --------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h,rows", [(96, 80, None), (83, 45, (7, 38))],
                         ids=["96x80", "83x45_rows_7_38"])
def test_every_kernel_returns_the_reference_hits(pkg, rt, oracle, w, h, rows):
    """96 x 80, and 83 x 45 rows [7, 38): partial tiles in x and y, a band
    offset, and the wide build's 128-pixel span wider than the frame."""
    scene, small = distinct_colours(base_scene(pkg)), distinct_colours(base_scene(pkg, fused=True))
    want = _ref(oracle, "base", scene, w, h, rows)
    want_small = _ref(oracle, "base_fused", small, w, h, rows)
    for r in (want, want_small):
        objs = np.unique(r["object"])
        assert objs[0] == -1 and len(objs) > 8, objs
    n = _render_paths(pkg, rt, scene, want, w, h, rows=rows, fused=(small, want_small),
                      label=f"{w}x{h}")
    assert n == len(PATHS)


# --- 2. ties that colours cannot see ---------------------------------------
TIE_XY = (66, 32)  # the pixel where the sphere's t0 equals the cube face's t


def hit_tie_scene(pkg):
    """One colour for everything.  18 spheres + 7 cubes of the base scene,
    then: a copy of sphere 3 (sphere index 18), a copy of cube 1 (cube index
    7), and a sphere / cube pair of equal t: an axis-aligned cube (the unit
    cube spans -1 .. 1) whose front
    face is z = -40 (t = 40 exactly) around a sphere of radius 10 centred at
    z = -50, whose t0 = tca - thc = 50 - 10 at the pixel under its centre.
    128 primitives: every kernel takes the same scene."""
    b = base_scene(pkg)
    cx, cy = TIE_XY
    so = np.concatenate([b.sphere_origins[:18], b.sphere_origins[3:4],
                         np.array([[cx, cy, -50, 1]], F32)])
    sr = np.concatenate([b.sphere_radius[:18], b.sphere_radius[3:4], np.array([10], F32)])
    face = pkg.cube_packed([("scale", 15, 15, 10), ("translate", cx, cy, -50)]).reshape(1, 36, 4)
    cv = np.concatenate([b.cube_vertices[:7], b.cube_vertices[1:2], face])
    colour = np.array([0.9, 0.6, 0.3, 255], F32)
    s = pkg.Scene(so, sr, np.tile(colour, (len(sr), 1)), cv, np.tile(colour, (len(cv), 1)))
    assert n_prims(s) == FUSED_MAX_PRIMS
    return s


def tie_reference(pkg, oracle):
    """(scene, hit_ref) with the ties asserted on the reference itself."""
    if "tie" in _CACHE:
        return _CACHE["tie"]
    s = hit_tie_scene(pkg)
    w, h = 96, 80
    ref = _ref(oracle, "tie", s, w, h)
    nc = s.num_cubes
    obj = ref["object"]

    def without(spheres, cubes):
        return pkg.Scene(s.sphere_origins[spheres], s.sphere_radius[spheres],
                         s.sphere_colours[spheres], s.cube_vertices[cubes], s.cube_colours[cubes])

    all_s, all_c = np.arange(s.num_spheres), np.arange(nc)
    # identical spheres 3 and 18: without the first, the copy wins exactly
    # the pixels the first wins (same t), so every one of them is a tie
    r = hit_ref(oracle, without(all_s[all_s != 3], all_c), w, h)
    won = obj == nc + 3
    assert won.sum() > 20 and not (obj == nc + 18).any()
    assert (r["object"][won] == nc + 17).all()          # (the copy, one index lower)
    assert np.array_equal(r["t"][won].view(np.uint32), ref["t"][won].view(np.uint32))
    # identical cubes 1 and 7
    r = hit_ref(oracle, without(all_s, all_c[all_c != 1]), w, h)
    won = obj == 1
    assert won.sum() > 20 and not (obj == 7).any()
    assert (r["object"][won] == 6).all()
    assert np.array_equal(r["t"][won].view(np.uint32), ref["t"][won].view(np.uint32))
    # the sphere (index 19) against the cube face (cube 8) at TIE_XY
    x, y = TIE_XY
    r = hit_ref(oracle, without(all_s, all_c[:8]), w, h)
    assert r["object"][y, x] == 8 + 19 and obj[y, x] == 8
    assert r["t"][y, x] == ref["t"][y, x] == F32(40.0)
    _CACHE["tie"] = (s, ref)
    return _CACHE["tie"]


def test_tie_scene_holds_the_ties(pkg, oracle):
    """No GPU: the reference frame really has the three ties, and the lower
    index / the cube wins each."""
    tie_reference(pkg, oracle)


@gpu
def test_ties_go_to_the_first_candidate(pkg, rt, oracle):
    scene, want = tie_reference(pkg, oracle)
    assert _render_paths(pkg, rt, scene, want, 96, 80, label="ties") == len(PATHS)


# --- 3. non-finite scene data ------------------------------------------------
def _nonfinite(pkg, kind):
    s = distinct_colours(base_scene(pkg, fused=True))
    if kind == "nan_radius":
        s.sphere_radius[5] = np.nan
    else:
        s.cube_vertices[2, 7, 0] = np.inf
    return s


@gpu
@pytest.mark.parametrize("kind", ["nan_radius", "inf_vertex"])
def test_nonfinite_scene_runs_the_reference_verbatim(pkg, rt, oracle, kind):
    """The binned kernels' "scene is not finite" path (collide_generic) in
    the hit format, every binned kernel and the generic one."""
    scene = _nonfinite(pkg, kind)
    want = _ref(oracle, kind, scene, 96, 80)
    assert (want["object"] >= 0).sum() > 500
    assert _render_paths(pkg, rt, scene, want, 96, 80, label=kind) == len(PATHS)


# --- 4. empty scene ----------------------------------------------------------
@gpu
def test_empty_scene_is_all_misses(pkg, rt):
    want = np.empty((45, 83), pkg.HIT_DTYPE)
    want["t"], want["object"] = K_FAR, -1
    assert _render_paths(pkg, rt, pkg.Scene(), want, 83, 45, label="empty") == len(PATHS)


# --- 5. the automatic choice at size ----------------------------------------
@gpu
@pytest.mark.parametrize("k", [2.0, 0.3])
def test_automatic_choice_at_size(pkg, k):
    """1280 x 1024, 256 spheres + 64 cubes on fresh contexts.  A fresh
    context's first binned frame runs prep -> coarse -> trace3_kernel, which
    reports the frame's box overdraw; a hit frame then skips the coarse
    kernel (trace_bin_kernel) while that stays below 1 frame (DESIGN.md
    §3.5): at k = 0.3, not at config 3's density k = 2 (overdraw 2.8).
    Shading either frame on the host gives the library's own int32x4 and
    RGBA8 frames bit for bit (other tests pin those to the oracle)."""
    w, h = 1280, 1024
    scene = pkg.Scene.synthetic(w, h, 256, 64, seed=3, k=k)
    with pkg.RayTracer(0) as a:
        colour = [a.render(scene, w, h)[0].copy() for _ in range(2)][-1]
        tex, _ = a.render(scene, w, h, fmt="rgba8")
    kernels = []
    with pkg.RayTracer(0) as fresh:
        fresh.reserve(w, h, 256, 64, fmt="hit")
        for _ in range(2):
            hits, t = fresh.render(scene, w, h, fmt="hit")
            kernels.append(fresh.last_kernel())
            assert t.path == "binned"
            assert np.array_equal(pkg.shade_hits(hits, scene, "i32x4"), colour), kernels
            assert np.array_equal(pkg.shade_hits(hits, scene, "rgba8"), tex), kernels
            assert np.array_equal(hits["object"] == -1, hits["t"] == K_FAR)
            assert hits["object"].max() < 320 and hits["object"].min() >= -1
        overdraw = fresh.last_overdraw()
    assert (overdraw < 1.0) == (k < 1.0) and overdraw < 4.0, overdraw
    second = "trace_bin_kernel" if overdraw < 1.0 else "trace3_kernel"
    assert kernels == ["trace3_kernel", second], kernels
    assert (hits["object"] >= 0).sum() > 1000


# --- 6. rt_render_multi -------------------------------------------------------
@gpu
def test_render_multi_two_contexts(pkg, rt, oracle):
    scene = distinct_colours(base_scene(pkg))
    single, _ = rt.render(scene, 96, 80, fmt="hit")
    assert not _diff(single, _ref(oracle, "base", scene, 96, 80))
    with pkg.RayTracer(0) as a, pkg.RayTracer(0) as b:
        for rows in (None, (7, 38)):
            multi, times = pkg.render_multi([a, b], scene, 96, 80, rows=rows, fmt="hit")
            rb, re = rows or (0, 80)
            assert multi.dtype == pkg.HIT_DTYPE and len(times) == 2
            assert not _diff(multi, single[rb:re]), _diff(multi, single[rb:re])


# --- 7. rt_render_device -------------------------------------------------------
@gpu
def test_render_device_band_leaves_the_rest_untouched(pkg, rt, oracle):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    scene = distinct_colours(base_scene(pkg))
    w, h, rb, re = 83, 45, 7, 38
    ds, keep = device_scene(torch, scene)
    sentinel = 0x5A5A5A5A
    frame = torch.full((h, w, 2), sentinel, dtype=torch.int32, device=dev)
    assert frame.data_ptr() % 8 == 0
    out_ptr = frame.data_ptr() + rb * w * 8
    stream = torch.cuda.current_stream().cuda_stream
    for variant in (0, 2):  # by frame size (16 x 16 tiles), then the wide build
        frame.fill_(sentinel)
        with knobs(rt, tile_variant=variant):
            rt.render_device(ds, w, h, (rb, re), out_ptr, fmt="hit", stream=stream)
            torch.cuda.synchronize()
        got = frame.cpu().numpy().view(np.uint32)
        assert (got[:rb] == sentinel).all() and (got[re:] == sentinel).all(), variant
        want = _ref(oracle, "base", scene, w, h, (rb, re))
        assert np.array_equal(got[rb:re], words(want)), variant
    del keep


# --- 8. the headless driver ------------------------------------------------------
@gpu
def test_headless_hit_format(pkg, tmp_path):
    """rt_headless --format hit: its PPM (rt_shade_hits of the hit frame) is
    byte for byte the --format i32x4 PPM of reference scene 3, its FNV line
    hashes the frame's words, and --pick prints the frame's pixel."""
    exe = Path(pkg.library_path()).parent / "rt_headless"
    assert exe.exists(), "build() makes rt_headless"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(exe.parent) + ":" + env.get("LD_LIBRARY_PATH", "")
    scene = pkg.Scene.reference(3)
    with pkg.RayTracer(0) as fresh:
        frame, _ = fresh.render(scene, 640, 480, fmt="hit")
    ys, xs = np.nonzero(frame["object"] >= 0)
    assert len(ys) > 1000
    px, py = int(xs[len(xs) // 2]), int(ys[len(ys) // 2])

    def run(*args):
        r = subprocess.run([str(exe), "--scene", "3", "--seed", "1", *args], capture_output=True,
                           text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout

    out = run("--format", "hit", "--ppm", str(tmp_path / "hit.ppm"), "--pick", f"{px},{py}")
    run("--format", "i32x4", "--ppm", str(tmp_path / "i32x4.ppm"))
    assert (tmp_path / "hit.ppm").read_bytes() == (tmp_path / "i32x4.ppm").read_bytes()
    assert f"hit fnv1a64 {pkg.fnv1a64(frame):016x}" in out, out
    want = f"pick {px},{py} object {int(frame[py, px]['object'])} t "
    line = [ln for ln in out.splitlines() if ln.startswith("pick ")]
    assert len(line) == 1 and line[0].startswith(want), out
    assert F32(float(line[0].split(" t ")[1])) == frame[py, px]["t"], out
    miss = np.argwhere(frame["object"] < 0)[0]
    out = run("--format", "hit", "--pick", f"{miss[1]},{miss[0]}")
    assert f"pick {miss[1]},{miss[0]} object -1 t 300000" in out, out
    # --pick is for hit frames
    r = subprocess.run([str(exe), "--pick", "1,1"], capture_output=True, text=True, env=env,
                       timeout=60)
    assert r.returncode == 2
