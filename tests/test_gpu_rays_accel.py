"""rt_accel_build_device / rt_cast_rays_accel_device / rt_occlude_rays_accel_device
/ rt_cast_camera_accel_device on the GPU: the kernels (csrc/rt_accel.hip)
against the host functions, culled (csrc/rt_accel.cpp) and unculled
(csrc/rt_light.cpp), which tests/test_accel.py and tests/test_rays.py pin to
the numpy restatements.

Device memory is torch tensors; every output sits between guard words (bytes
for the occlusion flags), and the guards, the ray buffer and the records must
come back unchanged.  Results are compared as raw words; no word is masked.
The guarded buffers and the ray upload are tests/test_gpu_rays.py's.
"""
import subprocess

import numpy as np
import pytest

import light_ref as lr
import rays_ref as yr
import test_gpu_rays as tg
from gpu_support import H, W, device_scene
from hit_ref import K_FAR
from light_device import PATTERN, check_scene_padding, padded_device_scene
from test_gpu_rays import (body_bytes, body_words, guarded_bytes, guarded_words, rays_unchanged,
                           read_cast, same, upload_rays)

gpu = pytest.mark.gpu
F32 = np.float32
RECORD_WORDS = 80  # 320 bytes


def odd_cubes(pkg, n, seed=5):
    """`n` synthetic cubes (and 7 spheres); with three or more, cube 1 has a
    NaN vertex coordinate and cube 2 an infinite one: always kept."""
    scene = pkg.Scene.synthetic(W, H, 7, n, seed=seed, k=0.3)
    if n >= 3:
        v = scene.cube_vertices.copy().reshape(n, 36, 4)
        v[1, 7, 1], v[2, 35, 2] = np.nan, -np.inf
        scene = pkg.Scene(scene.sphere_origins, scene.sphere_radius, scene.sphere_colours,
                          v.reshape(scene.cube_vertices.shape), scene.cube_colours)
    return scene


def device_build(pkg, rt, torch, ds, n_cubes, stream=0):
    buf, ptr = guarded_words(torch, RECORD_WORDS * n_cubes)
    if not stream:
        torch.cuda.synchronize()
    rt.build_accel_device(ds, ptr if n_cubes else 0, stream=stream)
    return buf, ptr


def records_of(pkg, torch, buf):
    return body_words(torch, buf).view(pkg.CUBE_BOUND_DTYPE)


# --- 1. the build kernel -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 67])
def test_build_equals_the_host(pkg, rt, n):
    """Workgroups with idle waves (1, 3, 5 cubes), a full one (4), a last
    partial one (5, 67), nothing to launch (0); the always-kept records."""
    torch = pytest.importorskip("torch")
    scene = odd_cubes(pkg, n)
    assert scene.num_cubes == n
    want = pkg.build_accel(scene)
    ds, keep = padded_device_scene(torch, scene)
    buf, ptr = device_build(pkg, rt, torch, ds, n)
    got = records_of(pkg, torch, buf)
    assert got.tobytes() == want.tobytes()
    if n >= 3:
        assert (got["emax2"][1:3] == np.inf).all() and np.isfinite(got["emax2"][0])
    check_scene_padding(torch, scene, keep)
    del keep


# --- 2. cast and occlude -------------------------------------------------------------------
def compare(pkg, rt, torch, scene, rays, ds=None, host_rays=None, label=""):
    """The records built on the device; cast (with and without triangles) and
    occlude through them against the host's culled AND unculled calls on
    `host_rays` (default `rays`).  Returns the device's (hits, tri, occ)."""
    keep = None
    if ds is None:
        ds, keep = device_scene(torch, scene)
    flat = np.ascontiguousarray(rays, pkg.RAY_DTYPE).reshape(-1)
    ref = flat if host_rays is None else np.ascontiguousarray(host_rays, pkg.RAY_DTYPE).reshape(-1)
    n, nc = flat.size, scene.num_cubes
    accel = pkg.build_accel(scene)
    acc_buf, acc_ptr = device_build(pkg, rt, torch, ds, nc)
    assert records_of(pkg, torch, acc_buf).tobytes() == accel.tobytes(), f"{label} records"
    rd = upload_rays(torch, pkg, flat)
    want, want_tri = pkg.cast_rays(ref, scene, triangles=True)
    culled, culled_tri = pkg.cast_rays_accel(ref, scene, accel, triangles=True)
    assert same(culled, want) and same(culled_tri, want_tri), f"{label} host culled = unculled"
    for triangles in (True, False):
        hits, hits_ptr = guarded_words(torch, 2 * n)
        tri, tri_ptr = guarded_words(torch, n) if triangles else (None, 0)
        torch.cuda.synchronize()
        rt.cast_rays_accel_device(rd.data_ptr(), n, ds, acc_ptr if nc else 0, hits_ptr, tri_ptr)
        got, got_tri = read_cast(pkg, torch, hits, tri)
        assert same(got, want), f"{label} hits (triangles={triangles})"
        if triangles:
            assert same(got_tri, want_tri), f"{label} triangles"
            first = got, got_tri
    flags, flags_ptr = guarded_bytes(torch, n)
    torch.cuda.synchronize()
    rt.occlude_rays_accel_device(rd.data_ptr(), n, ds, acc_ptr if nc else 0, flags_ptr)
    occ = body_bytes(torch, flags)
    assert same(occ, pkg.occlude_rays(ref, scene)), f"{label} occluded"
    assert same(occ, pkg.occlude_rays_accel(ref, scene, accel)), f"{label} occluded, host culled"
    rays_unchanged(torch, rd, flat)
    assert records_of(pkg, torch, acc_buf).tobytes() == accel.tobytes(), f"{label} records after"
    del keep
    return first[0], first[1], occ


def many(pkg):
    """70 cubes and 70 spheres."""
    return pkg.Scene.synthetic(W, H, 70, 70, seed=13, k=0.3)


@gpu
@pytest.mark.parametrize("n", tg.COUNTS)
def test_ray_counts(pkg, rt, n):
    torch = pytest.importorskip("torch")
    scene = many(pkg)
    rays = yr.random_rays(scene, 2573, 41)[:n]
    got, tri, occ = compare(pkg, rt, torch, scene, rays, label=f"n={n}")
    if n >= 255:
        assert (got["object"] >= 0).sum() >= 20 and (got["object"] == -1).sum() >= 20
        assert (tri >= 0).sum() >= 5 and 5 <= occ.sum() <= n - 5


def aimed(scene, cube, n, rng, spread=0.2):
    """`n` rays from in front of the frame towards cube `cube`'s centre."""
    v = scene.cube_vertices.reshape(-1, 36, 4)[cube, :, :3].astype(np.float64)
    c, s = v.mean(0), np.linalg.norm(v.max(0) - v.min(0))
    o = c + np.array([0.0, 0.0, 150.0]) + rng.uniform(-1, 1, (n, 3)) * 5
    d = c + rng.uniform(-spread, spread, (n, 3)) * s - o
    return yr.make_rays(o.T.astype(F32), (d * 2).T.astype(F32), -1)


def away(n, rng):
    """`n` rays that leave the scene: no cube lies along them."""
    o = np.array([-500.0, 40.0, 0.0]) + rng.uniform(-1, 1, (n, 3))
    d = np.array([-50.0, 0.0, 0.0]) + rng.uniform(-1, 1, (n, 3))
    return yr.make_rays(o.T.astype(F32), d.T.astype(F32), -1)


@gpu
def test_waves_by_what_their_lanes_keep(pkg, rt):
    """Wave 0: no lane keeps a cube.  Wave 1: exactly one lane does.  Wave 2:
    all lanes keep one cube.  Wave 3: fallback lanes (NaN and infinite
    directions) and lanes with directions of length 1e30 among culling lanes.
    Wave 4: the only cube a lane keeps is its skip."""
    torch = pytest.importorskip("torch")
    scene = many(pkg)
    nc, rng = scene.num_cubes, np.random.default_rng(17)
    accel = pkg.build_accel(scene)
    none = away(64, rng)
    one = away(64, rng)
    one[17] = aimed(scene, 0, 1, rng)[0]
    everyone = aimed(scene, 3, 64, rng)
    mixed = away(64, rng)
    mixed[1::2] = aimed(scene, 5, 64, rng)[1::2]
    mixed["dx"][4::16] = np.nan
    mixed["dz"][13::16] = -np.inf
    for f in ("dx", "dy", "dz"):
        mixed[f][9::16] = (mixed[f][9::16].astype(np.float64) * 1e28).astype(F32)
    # rays that keep exactly one cube and hit it: that cube becomes their skip
    pool = np.concatenate([aimed(scene, j, 64, rng, spread=0.05) for j in range(0, 40)])
    hit = pkg.cast_rays(pool, scene)["object"]
    lone = pool[(pkg.accel_kept(pool, scene, accel) == 1) & (hit >= 0) & (hit < nc)]
    assert len(lone) >= 128
    lone = lone[::len(lone) // 64][:64]
    lone["skip"] = pkg.cast_rays(lone, scene)["object"]
    rays = np.concatenate([none, one, everyone, mixed, lone])
    assert rays.shape == (320,)
    kept = pkg.accel_kept(rays, scene, accel).reshape(5, 64)
    assert (kept[0] == 0).all()
    assert (kept[1] > 0).sum() == 1 and kept[1, 17] >= 1
    assert (kept[2] >= 1).all()
    assert (kept[3, 4::16] == nc).all() and (kept[3, 13::16] == nc).all()  # the fallback
    assert (kept[3, 0::2][np.arange(32) % 8 != 2] == 0).all()  # the other lanes cull,
    assert (kept[3, 1::2][np.arange(32) % 8 != 6] < nc / 2).all()  # at length 1e30 too
    assert (kept[3, 9::16] >= 1).all()
    assert (kept[4] == 0).all() and len(set(lone["skip"])) >= 3
    got, tri, occ = compare(pkg, rt, torch, scene, rays, label="waves")
    obj = got["object"].reshape(5, 64)
    assert (obj[0] == -1).all() and obj[1, 17] >= 0 and (obj[2] >= 0).sum() >= 32
    assert not (obj[4] == lone["skip"]).any()


@gpu
def test_foreign_skip_ids(pkg, rt):
    """A skip outside [-1, nc + ns) is no object to the kernel: the host's
    result with those ids as -1.  On a padded scene."""
    torch = pytest.importorskip("torch")
    scene = lr.base(pkg)
    n_slots = yr.slots(scene)
    rays = yr.random_rays(scene, 771, 43)
    foreign = np.array([-2, n_slots, n_slots + 1, yr.I32_MIN, yr.I32_MAX, -3, 2 * n_slots],
                       np.int32)
    at = np.arange(0, len(rays), 5)
    rays["skip"][at] = foreign[np.arange(len(at)) % len(foreign)]
    outside = (rays["skip"] < -1) | (rays["skip"] >= n_slots)
    accel = pkg.build_accel(scene)
    for call in (pkg.cast_rays_accel, pkg.occlude_rays_accel, pkg.accel_kept):
        with pytest.raises(pkg.RtError) as e:
            call(rays, scene, accel)
        assert e.value.status == pkg.RT_ERR_INVALID_ARG
    mapped = rays.copy()
    mapped["skip"][outside] = -1
    ds, keep = padded_device_scene(torch, scene)
    got, tri, occ = compare(pkg, rt, torch, scene, rays, ds=ds, host_rays=mapped, label="foreign")
    assert (got["object"][outside] >= 0).sum() >= 10 and occ[outside].sum() >= 5
    check_scene_padding(torch, scene, keep)
    del keep


@gpu
@pytest.mark.parametrize("name", yr.EDGE_NAMES)
def test_edge_rays(pkg, rt, name):
    torch = pytest.importorskip("torch")
    scene = lr.base(pkg)
    compare(pkg, rt, torch, scene, yr.edge_rays(scene)[name], label=name)


@gpu
def test_always_kept_cubes(pkg, rt):
    torch = pytest.importorskip("torch")
    scene = odd_cubes(pkg, 18, seed=11)
    compare(pkg, rt, torch, scene, yr.random_rays(scene, 771, 53), label="always kept")


@gpu
def test_nothing_to_hit_nothing_to_cast(pkg, rt):
    """The empty scene and a scene of spheres alone with a NULL accel; n == 0
    is RT_OK and writes nothing."""
    torch = pytest.importorskip("torch")
    base = lr.base(pkg)
    rays = yr.random_rays(base, 257, 47, skips=[-1])
    got, tri, occ = compare(pkg, rt, torch, pkg.Scene(), rays, label="empty")
    assert (got["object"] == -1).all() and (got["t"] == K_FAR).all() and not occ.any()
    spheres = pkg.Scene(base.sphere_origins, base.sphere_radius, base.sphere_colours)
    got, tri, occ = compare(pkg, rt, torch, spheres, rays, label="spheres only")
    assert (got["object"] >= 0).sum() >= 20 and (tri == -1).all()
    ds, keep = device_scene(torch, base)
    acc_buf, acc_ptr = device_build(pkg, rt, torch, ds, base.num_cubes)
    rd = upload_rays(torch, pkg, rays)
    hits, hits_ptr = guarded_words(torch, 16)
    flags, flags_ptr = guarded_bytes(torch, 16)
    torch.cuda.synchronize()
    rt.cast_rays_accel_device(rd.data_ptr(), 0, ds, acc_ptr, hits_ptr, hits_ptr)
    rt.occlude_rays_accel_device(rd.data_ptr(), 0, ds, acc_ptr, flags_ptr)
    assert (body_words(torch, hits) == PATTERN).all()
    assert (body_bytes(torch, flags) == tg.BYTE_PATTERN).all()
    del keep


# --- 3. the fused camera cast ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("camera", ["reference", "pinhole"])
@pytest.mark.parametrize("rows", [None, (5, 17)], ids=["frame", "band"])
def test_camera(pkg, rt, camera, rows):
    """cast_camera_accel_device equals cast_rays_accel on camera_rays, the
    host's culled frame and the UNCULLED fused cast of the device."""
    torch = pytest.importorskip("torch")
    w, h = 37, 29
    scene = lr.base(pkg)
    cam = pkg.Camera.reference() if camera == "reference" else \
        pkg.Camera.pinhole((30, 20, 90), (32, 24, -40), (0, -1, 0), 50.0, w, h)
    band = rows or (0, h)
    n = (band[1] - band[0]) * w
    accel = pkg.build_accel(scene)
    want, want_tri = pkg.cast_rays_accel(pkg.camera_rays(cam, w, h, rows), scene, accel,
                                         triangles=True)
    assert same(want, pkg.cast_camera_accel(cam, scene, accel, w, h, rows))
    assert (want["object"] >= 0).sum() >= 20 and (want["object"] == -1).sum() >= 20
    ds, keep = device_scene(torch, scene)
    acc_buf, acc_ptr = device_build(pkg, rt, torch, ds, scene.num_cubes)
    results = []
    for culled in (True, False):
        for triangles in (True, False):
            hits, hits_ptr = guarded_words(torch, 2 * n)
            tri, tri_ptr = guarded_words(torch, n) if triangles else (None, 0)
            torch.cuda.synchronize()
            if culled:
                rt.cast_camera_accel_device(cam, ds, acc_ptr, w, band, hits_ptr, tri_ptr)
            else:
                rt.cast_camera_device(cam, ds, w, band, hits_ptr, tri_ptr)
            got, got_tri = read_cast(pkg, torch, hits, tri)
            assert same(got.reshape(want.shape), want), (culled, triangles)
            if triangles:
                assert same(got_tri.reshape(want.shape), want_tri), culled
            results.append(got)
    assert all(same(r, results[0]) for r in results)
    del keep


# --- 4. build, cast, occlude on one stream -----------------------------------------------------
@gpu
def test_build_cast_occlude_on_one_stream(pkg, rt):
    torch = pytest.importorskip("torch")
    scene = many(pkg)
    rays = yr.random_rays(scene, 2573, 59)
    n = rays.size
    ds, keep = device_scene(torch, scene)
    rd = upload_rays(torch, pkg, rays)
    acc_buf, acc_ptr = guarded_words(torch, RECORD_WORDS * scene.num_cubes)
    hits, hits_ptr = guarded_words(torch, 2 * n)
    tri, tri_ptr = guarded_words(torch, n)
    flags, flags_ptr = guarded_bytes(torch, n)
    torch.cuda.synchronize()  # uploads and fills are done before the stream starts
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rt.build_accel_device(ds, acc_ptr, stream=stream.cuda_stream)
        rt.cast_rays_accel_device(rd.data_ptr(), n, ds, acc_ptr, hits_ptr, tri_ptr,
                                  stream=stream.cuda_stream)
        rt.occlude_rays_accel_device(rd.data_ptr(), n, ds, acc_ptr, flags_ptr,
                                     stream=stream.cuda_stream)
    stream.synchronize()
    want, want_tri = pkg.cast_rays(rays, scene, triangles=True)
    occ = pkg.occlude_rays(rays, scene)
    assert (want["object"] >= 0).sum() >= 100 and 100 <= occ.sum() <= n - 100
    got, got_tri = read_cast(pkg, torch, hits, tri)
    assert same(got, want) and same(got_tri, want_tri) and same(body_bytes(torch, flags), occ)
    assert records_of(pkg, torch, acc_buf).tobytes() == pkg.build_accel(scene).tobytes()
    del keep


# --- 5. the headless driver ----------------------------------------------------------------------
@gpu
def test_headless_camera_accel_ppm(pkg, tmp_path):
    """rt_headless --camera ... --accel --ppm writes the bytes of the same
    command without --accel."""
    exe = pkg.PKG_DIR / "rt_headless"
    assert exe.exists()
    spec = "320,240,400,320,240,-100,70"
    outs = []
    for extra in ([], ["--accel"]):
        out = tmp_path / f"camera{len(extra)}.ppm"
        r = subprocess.run([str(exe), "--scene", "3", "--width", "64", "--height", "48",
                            "--camera", spec, *extra, "--ppm", str(out)], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append((out.read_bytes(), [l for l in r.stdout.splitlines() if "fnv1a64" in l]))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and outs[0][1]
    assert len(set(outs[0][0][15:])) >= 8  # a picture, not one colour
    bad = subprocess.run([str(exe), "--accel"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2
