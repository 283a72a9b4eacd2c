"""rt_hit_surfaces / rt_light_hits over their whole input domain, without a
GPU: every case of tests/light_edges.py -- oblique, signed-zero and scaled
directions, denormal and vanishing normals, lights that are zero, infinite,
NaN or seventy, foreign hit frames, every wave composition of the kernel's
wave-uniform path, the last rows and columns a frame can have -- first shows
its classes in the numpy restatement alone, then the host functions equal the
restatement word for word (DESIGN.md §3.1a's rule, light_edges.differ).

tests/test_gpu_light_edges.py runs the same table on the kernel.
"""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import light_edges as le
import light_ref as lr
from light_edges import CASES, OUTPUTS

NAMES = sorted(CASES)
INT_MIN = -(1 << 31)


def host(pkg, r, hits, what):
    if what == "surface":
        return pkg.hit_surfaces(hits, r.scene, rows=r.rows, ray_dir=r.d)
    return pkg.light_hits(hits, r.scene, what, rows=r.rows, ray_dir=r.d)


def want(r, what):
    return {"surface": r.surf, "i32x4": r.lit, "rgba8": r.rgba8}[what]


def check_window(r, what, got, label):
    """`got` (the whole frame) against the restatement: all of it, or, for the
    2^24-wide row, its last columns, with nothing hit in front of them."""
    x0 = r.x_begin
    diff = le.differ(what, got[:, x0:], want(r, what))
    assert not diff, f"{label} {what}: {diff}"
    if x0:
        empty = {"surface": np.array([0, 0, 0, 0xFFFFFFFF], np.uint32),
                 "i32x4": np.array([0, 0, 0, 255], np.uint32), "rgba8": np.uint32(0xFF000000)}[what]
        assert (lr.words(got[:, :x0]) == empty).all(), f"{label} {what}: a hit before the window"


# --- (a) the cases are what they are in the table for ---------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_conditions(pkg, oracle, name):
    """Every class of the case reaches its count, in the restatement alone."""
    r = le.reference(pkg, oracle, name)
    assert not le.missing_classes(r), le.missing_classes(r)
    c = CASES[name]
    assert r.given.shape == (r.rows[1] - r.rows[0], c["size"][0])
    if name == "light_w_nan":  # the reserved w does not matter: the frame of w = 1
        plain = lr.lit_ref(oracle, lr.with_lights(r.scene, lr.THREE_LIGHTS), r.hits, r.rb, r.d)
        assert not lr.eq(r.lit, plain) and np.isnan(r.scene.lights[:, 3]).all()
    if name == "dir_scaled_-1e30":  # t = -inf: k = 0 times an infinite ramp, NaN channels
        assert np.isneginf(r.hits["t"]).all() and (r.lit[..., :3] == INT_MIN).all()
    if name == "underflow_slab":  # NaN cosines only: k = 0, black
        assert (r.lit[:, 0] == (0, 0, 0, 255)).all()
    if name == "underflow_tiny_cube":  # k = inf clamped to 1: the unlit ramp
        assert np.array_equal(r.lit[0, 0], pkg.shade_hits(r.hits, r.scene)[0, 0])
    if name.startswith("foreign"):
        changed = (lr.words(r.given) != lr.words(r.valid)).any(-1).sum()
        assert changed == sum(r.counts.values()) and r.host_ok == (name == "foreign_t")
    if c["section"] == 2 and name.startswith("denormal"):  # one face, one normal
        assert len(np.unique(lr.words(r.surf[~r.miss]).reshape(-1, 4)[:, :3], axis=0)) == 1


@pytest.mark.parametrize("layout", ["column", "lanes"])
def test_denormal_normals_are_inexact(pkg, oracle, layout):
    """The restatement's slab normals against the exact unit normal of the
    same fp32 vertices (fp64).  Seven roundings (three squares, two sums, sqrt,
    division) keep an fp32 normal within 2 ulp while the squares keep their 24
    bits, which they do down to ex = 1e-22 (a denormal of 5.6e-40 still has
    18).  At ex = 1e-23 the smaller square, 5.6e-42, has 12 bits: the normal
    is finite, off by more than that and by less than 1e-4 of itself.  This is
    the regime in which a build that flushes denormals or expands sqrt or '/'
    inexactly parts from the written arithmetic."""
    off = {}
    for ex in ("1e-19", "1e-21", "1e-22", "1e-23"):
        r = le.reference(pkg, oracle, f"denormal_{ex}_{layout}")
        y, x = (int(v[0]) for v in np.nonzero(~r.miss))
        s = r.surf[y, x]
        v = r.scene.cube_vertices.reshape(12, 3, 4)[s["triangle"], :, :3].astype(np.float64)
        m = np.cross(v[1] - v[0], v[2] - v[0])
        n = m / np.linalg.norm(m)
        n = -n if np.dot(n, r.d[:3]) > 0 else n
        got = np.array([s["nx"], s["ny"], s["nz"]], np.float64)
        ulp = np.spacing(np.abs(n).astype(np.float32)).astype(np.float64)
        off[ex] = float(np.max(np.abs(got - n)[n != 0] / ulp[n != 0]))
        assert (got[n == 0] == 0).all() and np.isfinite(got).all()
        assert np.max(np.abs(got - n)) < 1e-4
    assert all(off[ex] <= 2 for ex in ("1e-19", "1e-21", "1e-22")), off
    assert off["1e-23"] > 2, off


# --- (b) the host functions against the restatement -------------------------------
@pytest.mark.parametrize("what", OUTPUTS)
@pytest.mark.parametrize("name", NAMES)
def test_host_equals_the_restatement(pkg, oracle, name, what):
    r = le.reference(pkg, oracle, name)
    if not r.host_ok:  # ids outside [-1, nc + ns): refused, as rt_shade_hits refuses them
        with pytest.raises(pkg.RtError) as e:
            host(pkg, r, r.given, what)
        assert e.value.status == pkg.RT_ERR_INVALID_ARG
        # and with those ids as -1 the host gives what the kernel must give
        check_window(r, what, host(pkg, r, r.hits, what), name + " ids as -1")
        return
    check_window(r, what, host(pkg, r, r.given, what), name)


# --- the table itself ---------------------------------------------------------------
def _parametrized(fn):
    """{argument names: values} of a test function's parametrize marks."""
    return {m.args[0]: list(m.args[1]) for m in fn.pytestmark if m.name == "parametrize"}


def test_case_table_is_complete():
    """Every section (directions, normals, lights, foreign frames, waves,
    coordinate limits) is in the table in the numbers it was written with,
    every case asks for classes, and both modules run every case on every
    output kind."""
    by = {}
    for name, c in CASES.items():
        by.setdefault(c["section"], []).append(name)
        assert c["classes"] and all(n >= 1 or k == "lights" for k, n in c["classes"].items()), name
        rows = c["rows"] or (0, c["size"][1])
        assert (c["size"][0] <= 128 and rows[1] - rows[0] <= 128) or c["section"] == 6, name
    assert sorted(by) == [1, 2, 3, 4, 5, 6]
    assert len(by[1]) == 8 and sum(CASES[n]["render"] for n in by[1]) == 3
    assert len(by[2]) == 4 * 3 + 2 + 5 + 1 and len(by[3]) == 7 and len(by[4]) == 2
    assert len(by[5]) == 6 and len(by[6]) == 2
    assert OUTPUTS == ("surface", "i32x4", "rgba8")
    here = _parametrized(test_host_equals_the_restatement)
    assert here == {"name": NAMES, "what": list(OUTPUTS)}
    assert _parametrized(test_case_conditions) == {"name": NAMES}
    spec = importlib.util.spec_from_file_location(
        "_gpu_light_edges", Path(__file__).with_name("test_gpu_light_edges.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert _parametrized(mod.test_device_equals_host_and_restatement) == {"name": NAMES}
    assert mod.OUTPUTS is OUTPUTS  # each of its cases loops over all of them and counts
    assert any(m.name == "gpu" for m in mod.test_device_equals_host_and_restatement.pytestmark)
