"""rt_hit_surfaces / rt_light_hits without a GPU: the host functions against
the numpy restatement (tests/light_ref.py), the zero-lights invariant against
`shade_hits` and the oracle, exact cases, and the argument contract.

Every comparison is on raw 32-bit words: the arithmetic is fully specified
(DESIGN.md §3.1a), so there are no tolerances.
"""
import shutil

import numpy as np
import pytest

import light_contract as lc
import light_ref as lr
from gpu_support import H, W
from hit_ref import REF_DIR, hit_ref
from light_ref import ONE_LIGHT, THREE_LIGHTS, base, edge_scenes, eq, one_cube, one_sphere

ENTRIES = lc.ENTRIES["light"]
F32 = np.float32
INT_MIN = -(1 << 31)
UP_DIR = (0.0, 0.0, 1.0, 0.0)
# (key, w, h, rows, ray_dir): the frames of the base scene
FRAMES = [("96x80", W, H, None, REF_DIR), ("83x45_rows_7_38", 83, 45, (7, 38), REF_DIR),
          ("96x80_dir_0_0_1_0", W, H, None, UP_DIR)]
FRAME_IDS = [f[0] for f in FRAMES]


def classes(scene, hits):
    obj = hits["object"]
    return (obj >= 0) & (obj < scene.num_cubes), obj >= scene.num_cubes, obj == -1


# --- 0. the restatement is not vacuous --------------------------------------
@pytest.mark.parametrize("key,w,h,rows,d", FRAMES, ids=FRAME_IDS)
def test_light_ref_covers_every_class(pkg, oracle, key, w, h, rows, d):
    scene = base(pkg)
    assert scene.num_spheres == 40 and scene.num_cubes == 10
    hits = lr.cached_hits(oracle, "base", scene, w, h, rows, d)
    surf = lr.surfaces_ref(oracle, scene, hits, rows[0] if rows else 0, d)
    cube, sphere, miss = classes(scene, hits)
    assert cube.sum() > 0 and (surf["triangle"][cube] >= 0).all()  # every cube pixel resolves
    assert (surf["triangle"][~cube] == -1).all()
    if d == REF_DIR:
        assert sphere.sum() > 0 and miss.sum() > 0
    for f in ("nx", "ny", "nz"):
        assert not np.isnan(surf[f]).any()
    if key == "96x80":
        assert set(np.unique(surf["triangle"][cube]).tolist()) == set(range(12))


def test_light_ref_factor_spans_its_range(pkg, oracle):
    scene = base(pkg)
    hits = lr.cached_hits(oracle, "base", scene, W, H)
    surf = lr.surfaces_ref(oracle, scene, hits)
    hit = hits["object"] >= 0
    k1 = lr.light_factor_ref(lr.with_lights(scene, ONE_LIGHT), hits, surf)
    assert ((k1 > 0) & (k1 < 1) & hit).sum() > 100 and ((k1 == 0) & hit).sum() > 0
    k3 = lr.light_factor_ref(lr.with_lights(scene, THREE_LIGHTS), hits, surf)
    assert ((k3 == 1) & hit).sum() > 100 and ((k3 > 0) & (k3 < 1) & hit).sum() > 100
    assert (k1[~hit] == 1).all() and (k3[~hit] == 1).all()


# --- 1. surfaces --------------------------------------------------------------
@pytest.mark.parametrize("key,w,h,rows,d", FRAMES, ids=FRAME_IDS)
def test_hit_surfaces_equal_the_restatement(pkg, oracle, key, w, h, rows, d):
    scene = base(pkg)
    hits = lr.cached_hits(oracle, "base", scene, w, h, rows, d)
    want = lr.surfaces_ref(oracle, scene, hits, rows[0] if rows else 0, d)
    got = pkg.hit_surfaces(hits, scene, rows=rows, ray_dir=d)
    assert got.dtype == pkg.SURFACE_DTYPE and got.shape == hits.shape
    assert not eq(got, want), eq(got, want)


# --- 2. zero lights: the reference's frame ------------------------------------
@pytest.mark.parametrize("i", range(4), ids=["base", "minus_inf", "past_int32", "nan_colour"])
def test_zero_lights_is_the_reference_frame(pkg, oracle, i):
    key, scene, w, h, d = edge_scenes(pkg)[i]
    assert len(scene.lights) == 0
    hits = lr.cached_hits(oracle, key, scene, w, h, None, d)
    assert (hits["object"] >= 0).sum() > 50
    want = oracle.trace(scene, w, h, ray_dir=np.asarray(d, F32))
    if key == "minus_inf":
        assert np.isneginf(hits["t"]).sum() > 50
    if key != "base":
        assert (want[..., :3] == INT_MIN).any()
    for fmt, ref in (("i32x4", want), ("rgba8", oracle.pack_rgba8(want))):
        got = pkg.light_hits(hits, scene, fmt, ray_dir=d)
        assert got.dtype == ref.dtype and not eq(got, ref), f"{key} {fmt}: {eq(got, ref)}"
        shaded = pkg.shade_hits(hits, scene, fmt)
        assert not eq(got, shaded), f"{key} {fmt} vs shade_hits: {eq(got, shaded)}"


# --- 3. lights ------------------------------------------------------------------
@pytest.mark.parametrize("lights", [ONE_LIGHT, THREE_LIGHTS], ids=["one_light", "three_lights"])
@pytest.mark.parametrize("key,w,h,rows,d", FRAMES[:2], ids=FRAME_IDS[:2])
def test_light_hits_equal_the_restatement(pkg, oracle, key, w, h, rows, d, lights):
    scene = lr.with_lights(base(pkg), lights)
    hits = lr.cached_hits(oracle, "base", scene, w, h, rows, d)
    want = lr.lit_ref(oracle, scene, hits, rows[0] if rows else 0, d)
    unlit = pkg.shade_hits(hits, scene)
    assert (want != unlit).any(-1).sum() > 100  # the lights do change pixels
    for fmt, ref in (("i32x4", want), ("rgba8", oracle.pack_rgba8(want))):
        got = pkg.light_hits(hits, scene, fmt, rows=rows, ray_dir=d)
        assert not eq(got, ref), f"{fmt}: {eq(got, ref)}"


def test_light_hits_minus_inf_with_lights(pkg, oracle):
    """t = -inf: p is NaN, every cosine is NaN, k = 0; the ramp is +inf and
    inf * 0 = NaN, so every channel of those pixels is INT32_MIN."""
    key, scene, w, h, d = edge_scenes(pkg)[1]
    scene = lr.with_lights(scene, THREE_LIGHTS)
    hits = lr.cached_hits(oracle, key, scene, w, h, None, d)
    neg = np.isneginf(hits["t"])
    assert neg.sum() > 50
    want = lr.lit_ref(oracle, scene, hits, 0, d)
    assert (want[neg][:, :3] == INT_MIN).all()
    for fmt, ref in (("i32x4", want), ("rgba8", oracle.pack_rgba8(want))):
        got = pkg.light_hits(hits, scene, fmt, ray_dir=d)
        assert not eq(got, ref), f"{fmt}: {eq(got, ref)}"


# --- 4. exact cases -----------------------------------------------------------
def test_axis_aligned_face_normal_and_triangles(pkg, oracle):
    """A cube of scale (15, 15, 10) at z = -50: the face at z = -40 is seen
    head on, its normal after facing is exactly (0, 0, 1), and the pixels
    split between that face's two triangles."""
    scene = one_cube(pkg, [("scale", 15, 15, 10), ("translate", 32, 24, -50)], (1, 1, 1, 255))
    hits = hit_ref(oracle, scene, 64, 48)
    on = hits["object"] == 0
    assert on.sum() > 500 and (hits["t"][on] == 40).all()
    tri_z = scene.cube_vertices.reshape(12, 3, 4)[:, :, 2]
    face = set(np.nonzero((tri_z == -40).all(1))[0].tolist())
    assert len(face) == 2
    surf = pkg.hit_surfaces(hits, scene)
    assert set(np.unique(surf["triangle"][on]).tolist()) == face
    assert (surf["nx"][on] == 0).all() and (surf["ny"][on] == 0).all()
    assert (surf["nz"][on] == 1).all()
    assert (lr.words(surf[~on]) == np.array([0, 0, 0, 0xFFFFFFFF], np.uint32)).all()


def sphere_and_light(pkg, light_z):
    s = one_sphere(pkg, (32, 24, -50, 1), 20, (1.0, 0.5, 0.25, 255))
    return lr.with_lights(s, [(32, 24, light_z, 1)])


def test_light_on_the_axis_leaves_the_centre_pixel_unlit_value(pkg, oracle):
    """Under the centre n = (0, 0, 1) and the light is straight ahead: k = 1."""
    scene = sphere_and_light(pkg, 0)
    hits = hit_ref(oracle, scene, 64, 48)
    assert hits[24, 32]["object"] == 0 and hits[24, 32]["t"] == 30
    lit, unlit = pkg.light_hits(hits, scene), pkg.shade_hits(hits, scene)
    assert lit[24, 32].tolist() == unlit[24, 32].tolist() and lit[24, 32, 0] > 100
    on = hits["object"] == 0
    assert (lit[on][:, 0] < unlit[on][:, 0]).sum() > 500  # and dimmer towards the rim


def test_light_behind_the_sphere_gives_black(pkg, oracle):
    scene = sphere_and_light(pkg, -200)
    hits = hit_ref(oracle, scene, 64, 48)
    on = hits["object"] == 0
    assert on.sum() > 500
    lit = pkg.light_hits(hits, scene)
    assert (lit[on] == (0, 0, 0, 255)).all()
    assert (pkg.light_hits(hits, scene, "rgba8")[on] == 0xFF000000).all()


# --- 5. contract ------------------------------------------------------------------
def test_foreign_t_resolves_to_no_triangle(pkg, oracle):
    scene = lr.with_lights(base(pkg), ONE_LIGHT)
    hits = lr.cached_hits(oracle, "base", scene, W, H).copy()
    cube, _, _ = classes(scene, hits)
    y, x = (int(v[0]) for v in np.nonzero(cube))
    before = pkg.hit_surfaces(hits, scene)[y, x]
    assert before["triangle"] >= 0
    for towards in (np.inf, -np.inf):
        h = hits.copy()
        h["t"][y, x] = np.nextafter(hits["t"][y, x], F32(towards))
        s = pkg.hit_surfaces(h, scene)[y, x]
        assert lr.words(s).reshape(-1).tolist() == [0, 0, 0, 0xFFFFFFFF]  # n = +0, triangle -1
        for fmt, black in (("i32x4", [0, 0, 0, 255]), ("rgba8", 0xFF000000)):
            assert np.array_equal(pkg.light_hits(h, scene, fmt)[y, x], black)


def test_object_out_of_range_is_refused(pkg):
    lc.objects_out_of_range(pkg, ENTRIES)


def test_formats_widths_and_rows_are_refused(pkg):
    lc.formats_widths_rows_and_pointers(pkg, ENTRIES)


def test_device_entries_refuse_a_null_context(pkg):
    """Before any HIP call: this runs without a GPU."""
    lc.device_entries_refuse_bad_arguments(pkg, ENTRIES)


def test_python_mirror_names(pkg):
    assert pkg.SURFACE_DTYPE == lr.surface_dtype() and pkg.SURFACE_DTYPE.itemsize == 16
    assert "SURFACE_DTYPE" in pkg.__all__
    lc.names(pkg, ENTRIES)


# --- 6. under the sanitizers ------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_light_arguments_under_sanitizers(tmp_path):
    """tests/light_args_check.cpp: exactly-sized heap arrays, empty scenes
    with NULL arrays, a one-row band at a large row_begin."""
    lc.run_args_check(tmp_path, "light")
