"""rt_shadow_hits_reflected / rt_light_hits_shadowed_reflected without a GPU:
the host functions against the numpy restatement (tests/shadow_reflect_ref.py)
of DESIGN.md §3.1d.

Every comparison is on raw 32-bit words; there are no tolerances and no words
are masked.  Every case first asserts on the restatement that it contains what
it is there for.  No created NaN reaches an output word: a mask is built from
comparisons, which NaN fails, and a lit channel goes through (int), which turns
every NaN into INT32_MIN.

The Python names: the host function of the lit form is
`light_hits_shadowed_reflected`, not a `shadows=` argument of
`light_hits_reflected`, whose parameter list tests/test_reflect_hits.py pins;
the device method is `light_hits_reflected_device(..., shadows=True)`.
"""
import shutil

import numpy as np
import pytest

import light_contract as lc
import light_ref as lr
import reflect_ref as rr
import shadow_ref as sr
import shadow_reflect_ref as srr
from gpu_support import H, W
from hit_ref import K_FAR, REF_DIR
from light_ref import ONE_LIGHT, THREE_LIGHTS, base, eq

F32 = np.float32
REFLECTIVITIES = (0.25, 1.0)
ENTRIES = lc.ENTRIES["shadow_reflect"]
restated = srr.restated


def compare(pkg, oracle, scene, hits, c, rows=None, d=REF_DIR, label=""):
    """The mask at p2 and both lit formats, at r = 0, 0.25 and 1, of the host
    functions against the restatement `c`."""
    if len(scene.lights) <= 32:
        got = pkg.shadow_hits_reflected(hits, scene, rows=rows, ray_dir=d)
        assert got.dtype == np.uint32 and got.shape == hits.shape
        assert not eq(got, c.mask2), f"{label} mask: {eq(got, c.mask2)}"
    for refl in (0.0,) + REFLECTIVITIES:
        want = c.mirrored(refl)
        for fmt, ref in (("i32x4", want), ("rgba8", oracle.pack_rgba8(want))):
            got = pkg.light_hits_shadowed_reflected(hits, scene, refl, fmt, rows=rows, ray_dir=d)
            assert got.dtype == ref.dtype and not eq(got, ref), \
                f"{label} r={refl} {fmt}: {eq(got, ref)}"


# --- 1. the restatement of the shadow term at arbitrary points ------------------------------
def test_shadow_at_reproduces_shadow_ref(pkg, oracle):
    """shadow_at fed the primary points: shadow_ref.shadow_ref's mask and k."""
    scene = sr.kinds_scene(pkg)
    hits = lr.cached_hits(oracle, "shadow_kinds", scene, sr.KINDS_W, sr.KINDS_H)
    want = sr.shadow_ref(oracle, scene, hits)
    assert want.by_cube.sum() > 100 and want.by_sphere.sum() > 100
    assert ((want.k > 0) & (want.k < 1)).sum() > 1000
    got = srr.shadow_at(scene, hits["object"].astype(np.int32),
                        (want.surf["nx"], want.surf["ny"], want.surf["nz"]),
                        lr.hit_points(hits, 0, REF_DIR))
    assert np.array_equal(got.mask, want.mask)
    assert np.array_equal(got.k.view(np.uint32), want.k.view(np.uint32))
    assert np.array_equal(got.occluded, want.occluded) and np.array_equal(got.cast, want.cast)


# --- 2. the classes of pixels ------------------------------------------------------------------
def test_the_classes(pkg, oracle):
    scene = srr.class_scene(pkg)
    hits, c = restated(oracle, "shadow_reflect_class", scene, srr.CLASS_W, srr.CLASS_H)
    srr.class_facts(scene, hits, c)
    compare(pkg, oracle, scene, hits, c, label="classes")
    for refl, least in ((0.25, 1000), (1.0, 100)):  # the restatement: 7943 and 538 pixels
        got = pkg.light_hits_shadowed_reflected(hits, scene, refl)
        shadowed = pkg.light_hits(hits, scene, shadows=True)
        mirrored = pkg.light_hits_reflected(hits, scene, refl)
        assert ((got != shadowed).any(-1) & (got != mirrored).any(-1)).sum() >= least, refl
    # the mask is shadow_hits' mask only by accident: another point, another own object
    assert (pkg.shadow_hits_reflected(hits, scene) != pkg.shadow_hits(hits, scene)).sum() >= 500


# --- 3. identities -------------------------------------------------------------------------------
def zero_cases(pkg):
    cases = [(f"base_{len(l)}", lr.with_lights(base(pkg), l), W, H, REF_DIR, "base")
             for l in ([], ONE_LIGHT, THREE_LIGHTS)]
    for key, scene, w, h, d in lr.edge_scenes(pkg):
        if key in ("minus_inf", "nan_colour"):
            cases.append((key, lr.with_lights(scene, THREE_LIGHTS), w, h, d, "shadow_edge_" + key))
    return {c[0]: c for c in cases}


@pytest.mark.parametrize("name", ["base_0", "base_1", "base_3", "minus_inf", "nan_colour"])
def test_reflectivity_zero_is_the_shadowed_frame(pkg, oracle, name):
    _, scene, w, h, d, key = zero_cases(pkg)[name]
    hits = lr.cached_hits(oracle, key, scene, w, h, None, d)
    assert (hits["object"] >= 0).sum() > 100
    if name == "minus_inf":
        assert np.isneginf(hits["t"]).sum() > 50
    if name == "nan_colour":
        assert np.isnan(scene.sphere_colours).any()
    for refl in (0.0, -0.0):
        for fmt in ("i32x4", "rgba8"):
            got = pkg.light_hits_shadowed_reflected(hits, scene, refl, fmt, ray_dir=d)
            want = pkg.light_hits(hits, scene, fmt, ray_dir=d, shadows=True)
            assert got.dtype == want.dtype and not eq(got, want), f"{name} {fmt}: {eq(got, want)}"
    if name in ("base_1", "base_3"):
        assert eq(pkg.light_hits_shadowed_reflected(hits, scene, 0.25),
                  pkg.light_hits(hits, scene, shadows=True))  # r = 0.25 is another frame


@pytest.mark.parametrize("name", ["class", "base"])
def test_without_lights_it_is_the_mirrored_frame(pkg, oracle, name):
    scene, w, h, key = {"class": (srr.class_scene(pkg, ()), srr.CLASS_W, srr.CLASS_H,
                                  "shadow_reflect_class"),
                        "base": (base(pkg), W, H, "base")}[name]
    assert len(scene.lights) == 0
    hits = lr.cached_hits(oracle, key, scene, w, h)
    assert (pkg.reflect_hits(hits, scene)["object"] >= 0).sum() > 300
    for refl in REFLECTIVITIES:
        for fmt in ("i32x4", "rgba8"):
            got = pkg.light_hits_shadowed_reflected(hits, scene, refl, fmt)
            want = pkg.light_hits_reflected(hits, scene, refl, fmt)
            assert not eq(got, want), f"{name} r={refl} {fmt}: {eq(got, want)}"
    assert not pkg.shadow_hits_reflected(hits, scene).any()


def test_a_single_object_casts_no_shadow(pkg, oracle):
    scene = srr.single_object_scene(pkg)
    hits, c = restated(oracle, "shadow_reflect_single", scene, 64, 48)
    assert (hits["object"] == 0).sum() > 1000 and ((c.k > 0) & (c.k < 1)).sum() > 200
    compare(pkg, oracle, scene, hits, c, label="single")
    for refl in REFLECTIVITIES:
        assert not eq(pkg.light_hits_shadowed_reflected(hits, scene, refl),
                      pkg.light_hits_reflected(hits, scene, refl))
    assert not pkg.shadow_hits_reflected(hits, scene).any()


@pytest.mark.parametrize("name", ["class", "base"])
def test_the_mask_is_zero_where_the_bounce_misses(pkg, oracle, name):
    scene, w, h, key = {"class": (srr.class_scene(pkg), srr.CLASS_W, srr.CLASS_H,
                                  "shadow_reflect_class"),
                        "base": (lr.with_lights(base(pkg), THREE_LIGHTS), W, H, "base")}[name]
    hits = lr.cached_hits(oracle, key, scene, w, h)
    missed = pkg.reflect_hits(hits, scene)["object"] == -1
    mask = pkg.shadow_hits_reflected(hits, scene)
    assert (missed & (hits["object"] >= 0)).sum() >= 1000 and (mask != 0).sum() >= 50
    assert not mask[missed].any()


# --- 4. the special scenes ------------------------------------------------------------------------
def test_inside_a_sphere_pins_the_exclusion_rule(pkg, oracle):
    """The bounce leaves sphere 1's front inside sphere 0 and meets sphere 0
    from within (the far root): n2 is turned inward, the second light faces
    p2, and the segment to it leaves sphere 0 through its far side.  The rule
    leaves obj2 = sphere 0 out, so the light counts: k2 > 0, the mask bit clear."""
    scene = sr.intersecting_spheres(pkg, srr.INSIDE_LIGHTS)
    hits, c = restated(oracle, "shadow_edge_p_inside_a_sphere", scene, 64, 48)
    from_within = c.refl.far_root & (c.refl.bounce["object"] == 0) & (hits["object"] == 1)
    assert from_within.sum() > 100  # the restatement: 193
    L = tuple(F32(v) - a for v, a in zip(srr.INSIDE_LIGHTS[1][:3], c.p2))
    with np.errstate(all="ignore"):
        through_own = sr.sphere_occludes(c.p2, L, scene.sphere_origins[0], scene.sphere_radius[0])
    pinned = from_within & c.at_p2.cast[1] & through_own
    assert pinned.sum() >= 50  # the restatement: 65
    # (where sphere 1, the pixel's own object, stands in the way it hides the light)
    by_own = c.at_p2.by_object[1, 1]
    pinned &= ~by_own
    assert pinned.sum() >= 30 and (by_own & from_within).sum() >= 5
    assert not c.at_p2.occluded[1][pinned].any() and (c.k2[pinned] > 0).all()
    compare(pkg, oracle, scene, hits, c, label="inside a sphere")
    assert not (pkg.shadow_hits_reflected(hits, scene)[pinned] & 2).any()


@pytest.mark.parametrize("name", srr.SPECIAL_NAMES)
def test_special_scenes(pkg, oracle, name):
    scenes = srr.special_scenes(pkg)
    assert sorted(scenes) == sorted(srr.SPECIAL_NAMES)
    scene, key = scenes[name]
    hits, c = restated(oracle, key, scene, 64, 48)
    o2 = c.refl.bounce["object"]
    if name == "twins":  # ties go to cube 0, and cube 1 then shadows what cube 0 shows
        assert (o2 == 0).sum() >= 20 and not (o2 == 1).any()
        assert c.at_p2.cast[:, o2 == 0].any()
    elif name == "sphere_tie":
        y, x = rr.TIE_PIXEL
        assert o2[y, x] == 0 and (o2 == 2).sum() >= 50
    elif name == "ramp":
        past = (hits["t"] + c.refl.bounce["t"] > 180) & (o2 == 1)
        assert past.sum() >= 200 and (c.refl.scalar2[past] < 0).all()
        assert (c.mirrored(1.0)[past] == (0, 0, 0, 255)).all()
    else:
        assert c.refl.far_root.sum() > 100 and c.at_p.occluded.sum() > 50
    compare(pkg, oracle, scene, hits, c, label=name)


@pytest.mark.parametrize("lights", [ONE_LIGHT, THREE_LIGHTS], ids=["1", "3"])
def test_base_scene(pkg, oracle, lights):
    scene = lr.with_lights(base(pkg), lights)
    hits, c = restated(oracle, "base", scene, W, H)
    assert min(v.sum() for v in c.refl.kinds.values()) >= 50
    assert c.at_p2.occluded.any(0).sum() >= 20 and (c.at_p2.cast & ~c.at_p2.occluded).sum() >= 100
    compare(pkg, oracle, scene, hits, c, label="base")


# --- 5. numeric edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rr.EDGE_NAMES)
def test_numeric_edges(pkg, oracle, name):
    """Every case of reflect_ref.edge_cases; tests/reflect_ref.py's
    check_edge says what each holds."""
    cases = rr.edge_cases(pkg)
    assert sorted(cases) == sorted(rr.EDGE_NAMES)
    scene, w, h, d, key = cases[name]
    hits, c = restated(oracle, key, scene, w, h, None, d)
    rr.check_edge(name, scene, hits, c.refl)
    if name in ("light_on_a_hit_point", "light_at_nan", "light_at_denormals",
                "light_inside_a_sphere", "light_on_a_triangle", "dir_oblique"):
        assert c.mask2.any()  # a finite light is hidden from some bounce point
    if name == "light_at_inf":
        assert not c.mask2.any()  # no light faces anything
    compare(pkg, oracle, scene, hits, c, d=d, label=name)


# --- 6. bands ----------------------------------------------------------------------------------------
def test_a_band_is_a_slice_of_the_frame(pkg, oracle):
    scene = srr.class_scene(pkg)
    w, h, rows = srr.CLASS_W, srr.CLASS_H, (21, 109)
    hits, c = restated(oracle, "shadow_reflect_class", scene, w, h)
    band = np.ascontiguousarray(hits[rows[0]:rows[1]])
    assert (c.mask2[rows[0]:rows[1]] != 0).sum() >= 300
    got = pkg.shadow_hits_reflected(band, scene, rows=rows)
    assert not eq(got, c.mask2[rows[0]:rows[1]])
    for fmt in ("i32x4", "rgba8"):
        whole = pkg.light_hits_shadowed_reflected(hits, scene, 0.25, fmt)
        got = pkg.light_hits_shadowed_reflected(band, scene, 0.25, fmt, rows=rows)
        assert not eq(got, whole[rows[0]:rows[1]]), fmt
    # the same band taken for rows 0..88 is another picture
    assert eq(pkg.shadow_hits_reflected(band, scene), c.mask2[rows[0]:rows[1]])


# --- 7. more than 32 lights --------------------------------------------------------------------------
def test_33_lights(pkg, oracle):
    lights = [(154 - 4 * i, 64 + (i % 5), 40, 1) for i in range(33)]
    scene = sr.kinds_scene(pkg, lights)
    rows = (60, 68)
    hits, c = restated(oracle, "shadow_kinds", scene, sr.KINDS_W, sr.KINDS_H, rows)
    assert c.hit2.sum() >= 20 and c.at_p2.occluded[32].any() and c.at_p.occluded[32].any()
    compare(pkg, oracle, scene, hits, c, rows=rows, label="33 lights")  # the lit forms
    lc.more_than_32_lights(pkg, ENTRIES, scene, hits, rows)


# --- 8. the argument contract ---------------------------------------------------------------------
def test_object_out_of_range_is_refused(pkg):
    lc.objects_out_of_range(pkg, ENTRIES)


def test_reflectivity_outside_0_1_is_refused(pkg):
    scene = lr.with_lights(base(pkg), ONE_LIGHT)
    hits = np.zeros((2, 3), pkg.HIT_DTYPE)
    hits["t"], hits["object"] = K_FAR, -1
    for refl in (0.0, 1.0, 0.5, float(np.nextafter(F32(1), F32(0)))):
        assert pkg.light_hits_shadowed_reflected(hits, scene, refl).shape == (2, 3, 4)
    for refl in (-0.1, 1.5, float("nan"), float(np.nextafter(F32(1), F32(2))), -1e-30,
                 float("inf")):
        for fmt in ("i32x4", "rgba8"):
            lc.refused(pkg, lambda: pkg.light_hits_shadowed_reflected(hits, scene, refl, fmt))


def test_formats_widths_rows_and_pointers_are_refused(pkg):
    lc.formats_widths_rows_and_pointers(pkg, ENTRIES)


def test_device_entries_refuse_bad_arguments_before_any_hip_call(pkg):
    lc.device_entries_refuse_bad_arguments(pkg, ENTRIES)


def test_python_names(pkg):
    lc.names(pkg, ENTRIES)


# --- 9. under the sanitizers ----------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shadow_reflect_arguments_under_sanitizers(tmp_path):
    """tests/shadow_reflect_args_check.cpp: exactly-sized heap arrays, the
    shadow term's scene, an empty scene with NULL arrays, a band, the refusals."""
    lc.run_args_check(tmp_path, "shadow_reflect")
