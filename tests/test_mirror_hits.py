"""rt_bounce_hits / rt_light_hits_mirrored without a GPU: the host functions
against the numpy restatement (tests/mirror_ref.py) of DESIGN.md §3.1e, and
against the host functions of §3.1a-d where the section says they agree.

Every comparison is on raw 32-bit words; there are no tolerances and no words
are masked.  Every case first asserts on the restatement that its scene holds
what it is there for (the restatement's counts stand beside the bounds).
"""
import ctypes
import shutil

import numpy as np
import pytest

import light_contract as lc
import light_ref as lr
import mirror_ref as mr
import reflect_ref as rr
from gpu_support import H, W
from hit_ref import K_FAR, REF_DIR
from light_ref import ONE_LIGHT, THREE_LIGHTS, base, eq

F32 = np.float32
ENTRIES = lc.ENTRIES["mirror"]
restated, mixed = mr.restated, mr.mixed


def compare(pkg, oracle, scene, hits, c, refl, rows=None, d=REF_DIR, label="",
            depths=mr.DEPTHS, bounces=(1, 2, 8)):
    """The bounce frames and, at every depth, shadows off and on, both lit
    formats of the host functions against the restatement `c`."""
    for b in bounces:
        got = pkg.bounce_hits(hits, scene, b, rows=rows, ray_dir=d)
        want = c.bounce(b)
        assert got.dtype == want.dtype and not eq(got, want), f"{label} bounce {b}: {eq(got, want)}"
    for depth in depths:
        for shadows in (False, True):
            want = c.lit(refl, depth, shadows)
            for fmt, ref in (("i32x4", want), ("rgba8", oracle.pack_rgba8(want))):
                got = pkg.light_hits_mirrored(hits, scene, refl, depth, fmt, shadows, rows=rows,
                                              ray_dir=d)
                assert got.dtype == ref.dtype and not eq(got, ref), \
                    f"{label} depth={depth} shadows={shadows} {fmt}: {eq(got, ref)}"


# --- 1. the three scenes ---------------------------------------------------------------------
def test_chain_scene(pkg, oracle):
    scene = mr.chain_scene(pkg)
    hits, c = restated(oracle, mr.CHAIN_KEY, scene, mr.CHAIN_W, mr.CHAIN_H)
    mr.chain_facts(c)
    compare(pkg, oracle, scene, hits, c, mr.CHAIN_REFLECTIVITY, label="chain")
    one = pkg.light_hits_mirrored(hits, scene, mr.CHAIN_REFLECTIVITY, 1)
    two = pkg.light_hits_mirrored(hits, scene, mr.CHAIN_REFLECTIVITY, 2)
    assert (one != two).any(-1).sum() >= 100  # the second bounce shows


def test_corridor_scene(pkg, oracle):
    scene = mr.corridor_scene(pkg)
    hits, c = restated(oracle, "mirror_corridor", scene, mr.CORRIDOR_W, mr.CORRIDOR_H)
    mr.corridor_facts(c)
    compare(pkg, oracle, scene, hits, c, mr.CORRIDOR_REFLECTIVITY, label="corridor",
            bounces=range(1, mr.MAX_BOUNCES + 1))
    # past the ramp's end a level adds nothing, not negative light: two perfect
    # mirrors facing each other that deep are black, where the pixel's own ramp
    # (level 0 is not clamped) is not
    deep = c.bounce(mr.MAX_BOUNCES)["object"] >= 0
    lit = pkg.light_hits_mirrored(hits, scene, mr.CORRIDOR_REFLECTIVITY, 0)
    assert (lit[deep] != (0, 0, 0, 255)).any(-1).sum() >= 64
    got = pkg.light_hits_mirrored(hits, scene, mr.CORRIDOR_REFLECTIVITY, mr.MAX_BOUNCES)
    assert (got[deep] == (0, 0, 0, 255)).all()


def test_wave_scene(pkg, oracle):
    scene = mr.wave_scene(pkg)
    hits, c = restated(oracle, "mirror_wave", scene, mr.WAVE_W, mr.WAVE_H)
    mr.wave_facts(c)
    compare(pkg, oracle, scene, hits, c, mr.WAVE_REFLECTIVITY, label="wave")


# --- 2. directions and numeric edges ---------------------------------------------------------
@pytest.mark.parametrize("name", rr.EDGE_NAMES)
def test_numeric_edges(pkg, oracle, name):
    """Every case of reflect_ref.edge_cases (tests/reflect_ref.py's
    check_edge says what each holds), the oblique and scaled directions among
    them, with a reflectivity that changes from slot to slot."""
    scene, w, h, d, key = rr.edge_cases(pkg)[name]
    hits, c = restated(oracle, key, scene, w, h, None, d)
    assert (hits["object"] >= 0).sum() > 50
    compare(pkg, oracle, scene, hits, c, mixed(scene), d=d, label=name)


# --- 3. the identities with the one-bounce functions ------------------------------------------
def identity_scenes(pkg):
    return {"chain": (mr.chain_scene(pkg), mr.CHAIN_W, mr.CHAIN_H, mr.CHAIN_KEY),
            "chain_dark": (mr.chain_scene(pkg, ()), mr.CHAIN_W, mr.CHAIN_H, mr.CHAIN_KEY),
            "base": (lr.with_lights(base(pkg), THREE_LIGHTS), W, H, "base"),
            "base_dark": (base(pkg), W, H, "base")}


@pytest.mark.parametrize("name", ["chain", "chain_dark", "base", "base_dark"])
def test_one_bounce_with_one_reflectivity_is_the_reflected_frame(pkg, oracle, name):
    scene, w, h, key = identity_scenes(pkg)[name]
    hits = lr.cached_hits(oracle, key, scene, w, h)
    slots = scene.num_cubes + scene.num_spheres
    assert (pkg.reflect_hits(hits, scene)["object"] >= 0).sum() > 300
    for r in (0.25, 1.0, 0.0, -0.0):
        refl = np.full(slots, r, F32)
        for fmt in ("i32x4", "rgba8"):
            got = pkg.light_hits_mirrored(hits, scene, refl, 1, fmt)
            want = pkg.light_hits_reflected(hits, scene, r, fmt)
            assert got.dtype == want.dtype and not eq(got, want), f"r={r} {fmt}: {eq(got, want)}"
            got = pkg.light_hits_mirrored(hits, scene, refl, 1, fmt, shadows=True)
            want = pkg.light_hits_shadowed_reflected(hits, scene, r, fmt)
            assert not eq(got, want), f"shadowed r={r} {fmt}: {eq(got, want)}"
    # a second bounce is another frame
    ones = np.ones(slots, F32)
    assert eq(pkg.light_hits_mirrored(hits, scene, ones, 2),
              pkg.light_hits_reflected(hits, scene, 1.0))


@pytest.mark.parametrize("name", ["chain", "chain_dark", "base", "base_dark"])
def test_no_bounce_is_the_lit_frame(pkg, oracle, name):
    """max_bounces == 0 with any array (None too), and an all-zero array (0 or
    -0) at any depth."""
    scene, w, h, key = identity_scenes(pkg)[name]
    hits = lr.cached_hits(oracle, key, scene, w, h)
    slots = scene.num_cubes + scene.num_spheres
    for shadows in (False, True):
        for fmt in ("i32x4", "rgba8"):
            want = pkg.light_hits(hits, scene, fmt, shadows=shadows)
            cases = [(None, 0), (np.ones(slots, F32), 0), (mixed(scene), 0),
                     (np.zeros(slots, F32), 1), (np.zeros(slots, F32), 8),
                     (np.full(slots, -0.0, F32), 3)]
            for refl, depth in cases:
                got = pkg.light_hits_mirrored(hits, scene, refl, depth, fmt, shadows)
                assert got.dtype == want.dtype and not eq(got, want), \
                    f"{fmt} shadows={shadows} depth={depth}: {eq(got, want)}"
    assert eq(pkg.light_hits_mirrored(hits, scene, np.ones(slots, F32), 1), pkg.light_hits(hits, scene))


@pytest.mark.parametrize("name", ["chain", "base"])
def test_the_first_bounce_is_the_reflect_frame(pkg, oracle, name):
    scene, w, h, key = identity_scenes(pkg)[name]
    hits = lr.cached_hits(oracle, key, scene, w, h)
    got, want = pkg.bounce_hits(hits, scene, 1), pkg.reflect_hits(hits, scene)
    assert got.dtype == want.dtype == pkg.HIT_DTYPE and not eq(got, want), eq(got, want)
    second = pkg.bounce_hits(hits, scene, 2)
    assert eq(second, want) and (second["object"] >= 0).sum() >= 100
    # a bounce frame misses wherever the bounce before it did
    assert (second["object"][want["object"] < 0] == -1).all()
    assert (second["t"][second["object"] < 0] == K_FAR).all()


def test_depth_8_is_the_frame_at_the_longest_chain(pkg, oracle):
    """The base scene, every object a mirror: no chain takes more than seven
    walks, so depths 7 and 8 are one frame (and depth 3 is another)."""
    scene = lr.with_lights(base(pkg), THREE_LIGHTS)
    hits, c = restated(oracle, "base", scene, W, H)
    ones = np.ones(scene.num_cubes + scene.num_spheres, F32)
    walks, _, _ = c.stats(ones, 8)
    longest = int(walks.max())
    assert 3 <= longest < mr.MAX_BOUNCES  # 7
    for shadows in (False, True):
        at_8 = pkg.light_hits_mirrored(hits, scene, ones, 8, shadows=shadows)
        assert not eq(at_8, c.lit(ones, 8, shadows))
        assert not eq(pkg.light_hits_mirrored(hits, scene, ones, longest, shadows=shadows), at_8)
    assert eq(pkg.light_hits_mirrored(hits, scene, ones, 3), at_8)  # a shorter cap shows
    # (the last of those walks meets nothing: the deepest level is one below)
    deepest = max(j for j, lv in enumerate(c.levels) if (lv.obj >= 0).any())
    assert deepest == longest - 1
    assert not (pkg.bounce_hits(hits, scene, deepest + 1)["object"] >= 0).any()
    assert (pkg.bounce_hits(hits, scene, deepest)["object"] >= 0).any()


def test_a_band_is_a_slice_of_the_frame(pkg, oracle):
    scene = mr.chain_scene(pkg)
    w, h, rows = mr.CHAIN_W, mr.CHAIN_H, (21, 109)
    hits = lr.cached_hits(oracle, mr.CHAIN_KEY, scene, w, h)
    band = np.ascontiguousarray(hits[rows[0]:rows[1]])
    for fmt in ("i32x4", "rgba8"):
        whole = pkg.light_hits_mirrored(hits, scene, mr.CHAIN_REFLECTIVITY, 3, fmt, True)
        got = pkg.light_hits_mirrored(band, scene, mr.CHAIN_REFLECTIVITY, 3, fmt, True, rows=rows)
        assert not eq(got, whole[rows[0]:rows[1]]), fmt
    whole = pkg.bounce_hits(hits, scene, 2)
    assert not eq(pkg.bounce_hits(band, scene, 2, rows=rows), whole[rows[0]:rows[1]])
    assert eq(pkg.bounce_hits(band, scene, 2), whole[rows[0]:rows[1]])  # rows 0..88: another picture


# --- 4. the argument contract -------------------------------------------------------------------
def small_frame(pkg):
    scene, hits = lc.small_frame(pkg)
    return scene, hits, np.full(scene.num_cubes + scene.num_spheres, 0.5, F32)


refused = lc.refused


def test_depth_bounce_and_shadows_out_of_range_are_refused(pkg):
    scene, hits, refl = small_frame(pkg)
    for depth in range(mr.MAX_BOUNCES + 1):
        assert pkg.light_hits_mirrored(hits, scene, refl, depth).shape == (2, 3, 4)
    for depth in (-1, mr.MAX_BOUNCES + 1, 2**31 - 1, -2**31):
        refused(pkg, lambda: pkg.light_hits_mirrored(hits, scene, refl, depth))
    for b in range(1, mr.MAX_BOUNCES + 1):
        assert pkg.bounce_hits(hits, scene, b).shape == (2, 3)
    for b in (0, -1, mr.MAX_BOUNCES + 1, 2**31 - 1):
        refused(pkg, lambda: pkg.bounce_hits(hits, scene, b))
    assert pkg.RT_MAX_BOUNCES == mr.MAX_BOUNCES == 8
    lib, sc, d = pkg.library(), scene.as_c(), np.array(REF_DIR, F32)
    out = np.zeros((2, 3, 4), np.int32)
    for shadows, status in ((0, 0), (1, 0), (2, pkg.RT_ERR_INVALID_ARG), (-1, pkg.RT_ERR_INVALID_ARG)):
        assert lib.rt_light_hits_mirrored(hits.ctypes.data, ctypes.byref(sc), d.ctypes.data, 3, 0, 2,
                                          refl.ctypes.data, 1, shadows, 0,
                                          out.ctypes.data) == status, shadows


def test_reflectivity_arrays_are_checked(pkg):
    scene, hits, refl = small_frame(pkg)
    for ok in (0.0, -0.0, 1.0, float(np.nextafter(F32(1), F32(0)))):
        r = refl.copy()
        r[7] = ok
        assert pkg.light_hits_mirrored(hits, scene, r, 2).shape == (2, 3, 4)
    for bad in (-0.1, 1.5, float("nan"), float(np.nextafter(F32(1), F32(2))), -1e-30, float("inf")):
        for slot in (0, 7, len(refl) - 1):  # a slot no pixel holds is refused too
            r = refl.copy()
            r[slot] = bad
            for fmt in ("i32x4", "rgba8"):
                refused(pkg, lambda: pkg.light_hits_mirrored(hits, scene, r, 2, fmt))
    # NULL: only where no slot can be read
    refused(pkg, lambda: pkg.light_hits_mirrored(hits, scene, None, 1))
    assert pkg.light_hits_mirrored(hits, scene, None, 0).shape == (2, 3, 4)
    empty = lr.with_lights(pkg.Scene(), ONE_LIGHT)
    miss = np.zeros((2, 3), pkg.HIT_DTYPE)
    miss["t"], miss["object"] = K_FAR, -1
    assert (pkg.light_hits_mirrored(miss, empty, None, 8) == (0, 0, 0, 255)).all()
    with pytest.raises(ValueError):
        pkg.light_hits_mirrored(hits, scene, refl[:-1], 1)  # one value per slot


def test_object_out_of_range_is_refused(pkg):
    lc.objects_out_of_range(pkg, ENTRIES)


def test_formats_widths_rows_and_pointers_are_refused(pkg):
    lc.formats_widths_rows_and_pointers(pkg, ENTRIES)


def test_device_entries_refuse_bad_arguments_before_any_hip_call(pkg):
    lc.device_entries_refuse_bad_arguments(pkg, ENTRIES)


def test_python_names(pkg):
    assert "RT_MAX_BOUNCES" in pkg.__all__
    lc.names(pkg, ENTRIES)


# --- 5. under the sanitizers ----------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_mirror_arguments_under_sanitizers(tmp_path):
    """tests/mirror_args_check.cpp: exactly-sized heap arrays, the reflectivity
    array included, a chain of bounces, an empty scene with NULL arrays, the
    refusals."""
    lc.run_args_check(tmp_path, "mirror")
