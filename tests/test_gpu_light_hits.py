"""rt_hit_surfaces_device / rt_light_hits_device on the GPU: the kernel
(csrc/rt_light.hip) against the host functions (csrc/rt_light.cpp), which
tests/test_light_hits.py pins to the numpy restatement and the oracle.

Device memory is torch tensors.  Every output sits inside a larger tensor
pre-filled with a pattern, and the words around it must come back unchanged
(the harness of tests/light_device.py, shared with test_gpu_light_edges.py).
Frames are compared as raw 32-bit words.
"""
import numpy as np
import pytest

import light_ref as lr
from gpu_support import H, SCENE_ARRAYS, W, base_scene, device_scene
from hit_ref import K_FAR, REF_DIR, distinct_colours
from light_device import PATTERN, compare_all, run_device, unguard, upload_hits
from light_ref import ONE_LIGHT, THREE_LIGHTS, edge_scenes, eq

gpu = pytest.mark.gpu
F32 = np.float32


# --- 1. the base scene: surfaces, 0 / 1 / 3 lights, both formats ----------------
@gpu
@pytest.mark.parametrize("w,h,rows", [(W, H, (0, H)), (83, 45, (7, 38))],
                         ids=["96x80", "83x45_rows_7_38"])
def test_device_equals_host_on_the_base_scene(pkg, rt, w, h, rows):
    torch = pytest.importorskip("torch")
    scene = distinct_colours(base_scene(pkg))
    hits, _ = rt.render(scene, w, h, rows=rows, fmt="hit", ray_dir=REF_DIR)
    nc = scene.num_cubes
    assert ((hits["object"] >= 0) & (hits["object"] < nc)).sum() > 100
    assert (hits["object"] >= nc).sum() > 100 and (hits["object"] == -1).sum() > 100
    for lights in ([], ONE_LIGHT, THREE_LIGHTS):
        sl = lr.with_lights(scene, lights)
        got = compare_all("light", pkg, rt, torch, sl, None, hits, w, rows,
                          label=f"{len(lights)} lights")
        cube = (hits["object"] >= 0) & (hits["object"] < nc)
        assert (got["surface"]["triangle"][cube] >= 0).all()
        if not lights:  # the trace's own colour frames
            for fmt in ("i32x4", "rgba8"):
                frame, _ = rt.render(scene, w, h, rows=rows, fmt=fmt, ray_dir=REF_DIR)
                assert not eq(got[fmt], frame), f"zero lights {fmt}: {eq(got[fmt], frame)}"
        else:
            unlit = pkg.shade_hits(hits, scene)
            assert (got["i32x4"] != unlit).any(-1).sum() > 100


# --- 2. grid edges --------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", [(1, 1), (257, 3), (83, 31)], ids=["1x1", "257x3", "83x31"])
def test_partial_waves_and_workgroups(pkg, rt, w, h):
    """Pixel counts that are no multiple of 64 or 256 (1, 771, 2573): the
    last workgroup is partly idle, and the guards around the output hold."""
    torch = pytest.importorskip("torch")
    assert (w * h) % 64 and (w * h) % 256
    scene = lr.with_lights(distinct_colours(base_scene(pkg)), ONE_LIGHT)
    if (w, h) == (1, 1):  # a lone pixel that does hit something: sphere 0 moved onto it
        scene.sphere_origins[0, :2] = 0
    hits, _ = rt.render(scene, w, h, fmt="hit", ray_dir=REF_DIR)
    assert (hits["object"] >= 0).any()
    compare_all("light", pkg, rt, torch, scene, None, hits, w, (0, h), label=f"{w}x{h}")


# --- 3. trace, then light, on one stream ------------------------------------------
@gpu
def test_trace_then_light_on_one_stream(pkg, rt, oracle):
    """render_device(fmt="hit") and light_hits_device back to back on a
    non-default stream, no host synchronisation in between: the host pipeline
    (hit_ref, then light_hits) gives the same frame."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(distinct_colours(base_scene(pkg)), THREE_LIGHTS)
    hits_ref = lr.cached_hits(oracle, "base", scene, W, H)
    ds, keep = device_scene(torch, scene)
    hd = torch.full((H, W, 2), PATTERN, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()  # uploads and fills are done before the stream starts
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rt.render_device(ds, W, H, (0, H), hd.data_ptr(), ray_dir=np.array(REF_DIR, F32),
                         fmt="hit", stream=stream.cuda_stream)
        bufs = {fmt: run_device("light", pkg, rt, torch, ds, hd, W, (0, H), fmt,
                                 stream=stream.cuda_stream) for fmt in ("i32x4", "rgba8")}
    stream.synchronize()
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), lr.words(hits_ref))
    for fmt, buf in bufs.items():
        got = unguard(torch, pkg, buf, W, (0, H), fmt)
        want = pkg.light_hits(hits_ref, scene, fmt)
        assert not eq(got, want), f"{fmt}: {eq(got, want)}"
    del keep


# --- 4. numeric edges -------------------------------------------------------------
@gpu
@pytest.mark.parametrize("i", [1, 3], ids=["minus_inf", "nan_colour"])
def test_numeric_edges_with_lights(pkg, rt, oracle, i):
    """t = -inf (p, every cosine and the lit ramp are NaN: INT32_MIN in every
    channel) and a NaN colour.  The lit frames are compared word for word.
    A NaN an operation creates has no specified sign (x86 sets it, gfx950
    does not), so the surfaces are compared word for word where the host's
    are numbers and must be NaN where the host's are."""
    torch = pytest.importorskip("torch")
    key, scene, w, h, d = edge_scenes(pkg)[i]
    scene = lr.with_lights(scene, THREE_LIGHTS)
    hits = lr.cached_hits(oracle, key, scene, w, h, None, d)
    ds, keep = device_scene(torch, scene)
    hd = upload_hits(torch, hits)
    for fmt in ("i32x4", "rgba8"):
        buf = run_device("light", pkg, rt, torch, ds, hd, w, (0, h), fmt, d)
        got = unguard(torch, pkg, buf, w, (0, h), fmt)
        want = pkg.light_hits(hits, scene, fmt, ray_dir=d)
        assert not eq(got, want), f"{key} {fmt}: {eq(got, want)}"
        if key == "minus_inf" and fmt == "i32x4":
            assert (got[np.isneginf(hits["t"])][:, :3] == -(1 << 31)).all()
    buf = run_device("light", pkg, rt, torch, ds, hd, w, (0, h), "surface", d)
    got = unguard(torch, pkg, buf, w, (0, h), "surface")
    want = pkg.hit_surfaces(hits, scene, ray_dir=d)
    assert np.array_equal(got["triangle"], want["triangle"])
    for f in ("nx", "ny", "nz"):
        nan = np.isnan(want[f])
        assert np.array_equal(np.isnan(got[f]), nan)
        assert np.array_equal(got[f][~nan].view(np.uint32), want[f][~nan].view(np.uint32))
    del keep


# --- 5. the empty scene -----------------------------------------------------------
@gpu
@pytest.mark.parametrize("lights", [[], ONE_LIGHT], ids=["no_lights", "one_light"])
def test_empty_scene(pkg, rt, lights):
    """NULL scene arrays: every pixel is (0, 0, 0, 255) / the zero surface."""
    torch = pytest.importorskip("torch")
    scene = lr.with_lights(pkg.Scene(), lights)
    w, h = 70, 9
    hits, _ = rt.render(scene, w, h, fmt="hit", ray_dir=REF_DIR)
    assert (hits["t"] == K_FAR).all() and (hits["object"] == -1).all()
    ds, _keep = device_scene(torch, scene)
    assert not any(ds.get(k) for k in SCENE_ARRAYS[:5])
    got = compare_all("light", pkg, rt, torch, scene, None, hits, w, (0, h), label="empty")
    assert (got["i32x4"] == (0, 0, 0, 255)).all() and (got["rgba8"] == 0xFF000000).all()
    assert (lr.words(got["surface"]) == np.array([0, 0, 0, 0xFFFFFFFF], np.uint32)).all()


# --- 6. whole waves on one cube, and mixed waves --------------------------------------
@gpu
def test_one_cube_fills_the_frame(pkg, rt):
    """128 x 128 behind one axis-aligned cube face, a sphere in front of it in
    a corner, one light: most waves hold pixels of the one cube only, the
    corner's waves mix cube and sphere pixels."""
    torch = pytest.importorskip("torch")
    w = h = 128
    face = pkg.cube_packed([("scale", 70, 70, 10), ("translate", 64, 64, -60)]).reshape(1, 36, 4)
    scene = pkg.Scene(np.array([[10, 10, -30, 1]], F32), np.array([12], F32),
                      np.array([[0.2, 0.9, 0.4, 255]], F32), face,
                      np.array([[1.0, 0.7, 0.3, 255]], F32), np.array([[100, 30, 40, 1]], F32))
    hits, _ = rt.render(scene, w, h, fmt="hit", ray_dir=REF_DIR)
    obj = hits["object"].reshape(-1, 64)  # one row of this view per wave
    assert (hits["object"] >= 0).all()
    assert (obj == 0).all(1).sum() > 200 and ((obj == 0).any(1) & (obj == 1).any(1)).sum() > 10
    got = compare_all("light", pkg, rt, torch, scene, None, hits, w, (0, h), label="one cube")
    cube = hits["object"] == 0
    front = set(np.nonzero((face.reshape(12, 3, 4)[:, :, 2] == -50).all(1))[0].tolist())
    assert len(front) == 2
    assert set(np.unique(got["surface"]["triangle"][cube]).tolist()) == front
    assert (got["surface"]["nz"][cube] == 1).all()
    lit, unlit = got["i32x4"], pkg.shade_hits(hits, scene)
    assert ((lit[..., 0] > 0) & (lit[..., 0] < unlit[..., 0])).sum() > 10000
