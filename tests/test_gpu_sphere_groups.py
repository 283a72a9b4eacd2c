"""rt_sphere_groups_build_device / rt_cast_rays_grouped_device /
rt_occlude_rays_grouped_device / rt_cast_camera_grouped_device on the GPU: the
kernels (csrc/rt_sphere_groups.hip) against the host functions, grouped
(csrc/rt_sphere_groups.cpp), culled (csrc/rt_accel.cpp) and unculled
(csrc/rt_light.cpp), which tests/test_sphere_groups.py, tests/test_accel.py and
tests/test_rays.py pin to the numpy restatements.

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
import test_gpu_rays_accel as ta
import test_sphere_groups as ts
from gpu_support import H, W, device_scene
from hit_ref import K_FAR
from light_device import PATTERN, check_scene_padding, padded_device_scene
from test_gpu_rays import (BYTE_PATTERN, body_bytes, body_words, guarded_bytes, guarded_words,
                           rays_unchanged, read_cast, same, upload_rays)

gpu = pytest.mark.gpu
F32 = np.float32
RECORD_WORDS = 16  # 64 bytes


def odd_spheres(pkg, n, seed=5):
    """`n` spheres (and 3 cubes); from 9 on, sphere 1 has a NaN centre
    coordinate, sphere 4 an infinite radius and sphere 7 a negative one."""
    scene = pkg.Scene.synthetic(W, H, n, 3, seed=seed, k=0.3)
    if n >= 9:
        c, r = scene.sphere_origins.copy(), scene.sphere_radius.copy()
        c[1, 2], r[4], r[7] = np.nan, np.inf, -r[7]
        scene = pkg.Scene(c, r, scene.sphere_colours, scene.cube_vertices, scene.cube_colours)
    return scene


def device_groups(pkg, rt, torch, ds, n_spheres, group_size, stream=0):
    """The records built on the device between guard words, over a guarded
    workspace of exactly the documented size: (records tensor, address, count)."""
    lib = pkg.library()
    ng = lib.rt_sphere_groups_count(n_spheres, group_size)
    ws_bytes = lib.rt_sphere_groups_workspace_bytes(n_spheres)
    assert ws_bytes % 16 == 0
    buf, ptr = guarded_words(torch, RECORD_WORDS * ng)
    ws, ws_ptr = guarded_words(torch, ws_bytes // 4)
    if not stream:
        torch.cuda.synchronize()
    rt.build_sphere_groups_device(ds, group_size, ptr if n_spheres else 0,
                                  ws_ptr if n_spheres else 0, ws_bytes, stream=stream)
    return buf, ptr, ng, ws


def records_of(pkg, torch, buf):
    return body_words(torch, buf).view(pkg.SPHERE_GROUP_DTYPE)


# --- 1. the build kernels ------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 64, 65, 300])
def test_build_equals_the_host(pkg, rt, n):
    """Records with idle lanes (group_size 1 and 3, a last record that is not
    full), workgroups of the per-sphere kernels with idle lanes and a second
    workgroup (300), nothing to launch (0); the always-kept records."""
    torch = pytest.importorskip("torch")
    scene = odd_spheres(pkg, n)
    assert scene.num_spheres == n
    ds, keep = padded_device_scene(torch, scene)
    for group_size in (1, 3, 8):
        want = pkg.build_sphere_groups(scene, group_size)
        buf, ptr, ng, ws = device_groups(pkg, rt, torch, ds, n, group_size)
        got = records_of(pkg, torch, buf)
        assert ng == len(want) and got.tobytes() == want.tobytes(), group_size
        body_words(torch, ws)  # (the workspace's guards)
        if n >= 9:
            assert (got["rmax"] == np.inf).sum() >= 1
            # (the three non-finite spheres sort last: at most two records hold them)
            assert ng < 3 or np.isfinite(got["rmax"]).sum() >= 1
    check_scene_padding(torch, scene, keep)
    del keep


@gpu
def test_build_of_coincident_and_flat_scenes(pkg, rt):
    """Equal keys (the order falls back to the index), one axis and all axes of
    zero extent, centres at 1e6, radii of 1e-22."""
    torch = pytest.importorskip("torch")
    scenes = ts.record_scenes(pkg)
    for name in ("coincident", "one_point", "flat_x", "line_z", "signed_and_tiny", "at_1e6",
                 "zeros", "huge", "all_non_finite", "non_finite"):
        scene = scenes[name]
        ds, keep = device_scene(torch, scene)
        for group_size in (3, 8):
            want = pkg.build_sphere_groups(scene, group_size)
            buf, ptr, ng, ws = device_groups(pkg, rt, torch, ds, scene.num_spheres, group_size)
            assert records_of(pkg, torch, buf).tobytes() == want.tobytes(), (name, group_size)
        del keep


# --- 2. cast and occlude -------------------------------------------------------------------
def compare(pkg, rt, torch, scene, rays, ds=None, host_rays=None, label="", group_size=8):
    """The records built on the device; cast (with and without triangles) and
    occlude through them against the host's grouped, culled AND unculled calls
    on `host_rays` (default `rays`).  Returns the device's (hits, tri, occ)."""
    keep = None
    if ds is None:
        ds, keep = device_scene(torch, scene)
    flat = np.ascontiguousarray(rays, pkg.RAY_DTYPE).reshape(-1)
    ref = flat if host_rays is None else np.ascontiguousarray(host_rays, pkg.RAY_DTYPE).reshape(-1)
    n, nc, ns = flat.size, scene.num_cubes, scene.num_spheres
    accel, groups = pkg.build_accel(scene), pkg.build_sphere_groups(scene, group_size)
    acc_buf, acc_ptr = ta.device_build(pkg, rt, torch, ds, nc)
    grp_buf, grp_ptr, ng, ws = device_groups(pkg, rt, torch, ds, ns, group_size)
    assert records_of(pkg, torch, grp_buf).tobytes() == groups.tobytes(), f"{label} records"
    rd = upload_rays(torch, pkg, flat)
    want, want_tri = pkg.cast_rays(ref, scene, triangles=True)
    for host in (pkg.cast_rays_accel(ref, scene, accel, triangles=True),
                 pkg.cast_rays_grouped(ref, scene, accel, groups, triangles=True)):
        assert same(host[0], want) and same(host[1], want_tri), f"{label} host = unculled"
    for triangles in (True, False):
        hits, hits_ptr = guarded_words(torch, 2 * n)
        tri, tri_ptr = guarded_words(torch, n) if triangles else (None, 0)
        torch.cuda.synchronize()
        rt.cast_rays_grouped_device(rd.data_ptr(), n, ds, acc_ptr if nc else 0,
                                    grp_ptr if ns else 0, ng, hits_ptr, tri_ptr)
        got, got_tri = read_cast(pkg, torch, hits, tri)
        assert same(got, want), f"{label} hits (triangles={triangles})"
        if triangles:
            assert same(got_tri, want_tri), f"{label} triangles"
            first = got, got_tri
    flags, flags_ptr = guarded_bytes(torch, n)
    torch.cuda.synchronize()
    rt.occlude_rays_grouped_device(rd.data_ptr(), n, ds, acc_ptr if nc else 0,
                                   grp_ptr if ns else 0, ng, flags_ptr)
    occ = body_bytes(torch, flags)
    assert same(occ, pkg.occlude_rays(ref, scene)), f"{label} occluded"
    assert same(occ, pkg.occlude_rays_accel(ref, scene, accel)), f"{label} occluded, host culled"
    assert same(occ, pkg.occlude_rays_grouped(ref, scene, accel, groups)), f"{label} host grouped"
    rays_unchanged(torch, rd, flat)
    assert records_of(pkg, torch, grp_buf).tobytes() == groups.tobytes(), f"{label} records after"
    del keep
    return first[0], first[1], occ


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2573])
def test_ray_counts(pkg, rt, n):
    torch = pytest.importorskip("torch")
    scene = ta.many(pkg)
    rays = yr.random_rays(scene, 2573, 41)[:n]
    got, tri, occ = compare(pkg, rt, torch, scene, rays, label=f"n={n}")
    if n >= 255:
        nc = scene.num_cubes
        assert (got["object"] >= nc).sum() >= 20 and (got["object"] == -1).sum() >= 20
        assert (tri >= 0).sum() >= 5 and 5 <= occ.sum() <= n - 5


def aimed_at_sphere(scene, sphere, n, rng, spread=0.5):
    """`n` rays from in front of the frame towards sphere `sphere`."""
    c = scene.sphere_origins[sphere, :3].astype(np.float64)
    r = abs(float(scene.sphere_radius[sphere]))
    o = c + np.array([0.0, 0.0, 150.0]) + rng.uniform(-1, 1, (n, 3)) * 5
    d = c + rng.uniform(-spread, spread, (n, 3)) * r - o
    return yr.make_rays(o.T.astype(F32), (d * 2).T.astype(F32), -1)


@gpu
def test_waves_by_what_their_lanes_keep(pkg, rt):
    """Wave 0: no lane keeps a group.  Wave 1: exactly one lane does.  Wave 2:
    all lanes keep one group.  Wave 3: fallback lanes (NaN, infinite and zero
    directions) among culling lanes.  Wave 4: the lane's skip is the only
    member of its only kept group (groups of one sphere)."""
    torch = pytest.importorskip("torch")
    scene = ta.many(pkg)
    nc, rng = scene.num_cubes, np.random.default_rng(17)
    groups = pkg.build_sphere_groups(scene, 1)
    ng = len(groups)
    none = ta.away(64, rng)
    one = ta.away(64, rng)
    one[17] = aimed_at_sphere(scene, 0, 1, rng)[0]
    everyone = aimed_at_sphere(scene, 3, 64, rng)
    mixed = ta.away(64, rng)
    mixed[1::2] = aimed_at_sphere(scene, 5, 64, rng)[1::2]
    mixed["dx"][4::16] = np.nan
    mixed["dz"][13::16] = -np.inf
    for f in ("dx", "dy", "dz"):
        mixed[f][9::16] = 0.0
    pool = np.concatenate([aimed_at_sphere(scene, s, 64, rng, spread=0.2) for s in range(0, 40)])
    hit = pkg.cast_rays(pool, scene)["object"]
    lone = pool[(pkg.sphere_groups_kept(pool, scene, groups) == 1) & (hit >= nc)]
    assert len(lone) >= 128
    lone = lone[::len(lone) // 64][:64]
    lone["skip"] = pkg.cast_rays(lone, scene)["object"]
    rays = np.concatenate([none, one, everyone, mixed, lone])
    assert rays.shape == (320,)
    kept = pkg.sphere_groups_kept(rays, scene, groups).reshape(5, 64)
    assert (kept[0] == 0).all()
    assert (kept[1] > 0).sum() == 1 and kept[1, 17] >= 1
    assert (kept[2] >= 1).all()
    assert (kept[3, 4::16] == ng).all() and (kept[3, 13::16] == ng).all()  # the fallback
    assert (kept[3, 9::16] == ng).all()
    assert (kept[3, 0::2][np.arange(32) % 8 != 2] == 0).all()  # the other lanes cull
    assert (kept[4] == 1).all() and len(set(lone["skip"])) >= 3
    got, tri, occ = compare(pkg, rt, torch, scene, rays, label="waves", group_size=1)
    obj = got["object"].reshape(5, 64)
    assert (obj[0] == -1).all() and obj[1, 17] >= 0 and (obj[2] >= nc).sum() >= 32
    assert not (obj[4] == lone["skip"]).any()
    compare(pkg, rt, torch, scene, rays, label="waves, groups of 8", group_size=8)


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
    accel, groups = pkg.build_accel(scene), pkg.build_sphere_groups(scene, 3)
    for call in (pkg.cast_rays_grouped, pkg.occlude_rays_grouped):
        with pytest.raises(pkg.RtError) as e:
            call(rays, scene, accel, groups)
        assert e.value.status == pkg.RT_ERR_INVALID_ARG
    mapped = rays.copy()
    mapped["skip"][outside] = -1
    ds, keep = padded_device_scene(torch, scene)
    got, tri, occ = compare(pkg, rt, torch, scene, rays, ds=ds, host_rays=mapped, label="foreign",
                            group_size=3)
    assert (got["object"][outside] >= 0).sum() >= 10 and occ[outside].sum() >= 5
    check_scene_padding(torch, scene, keep)
    del keep


@gpu
@pytest.mark.parametrize("name", yr.EDGE_NAMES)
def test_edge_rays(pkg, rt, name):
    torch = pytest.importorskip("torch")
    scene = lr.base(pkg)
    compare(pkg, rt, torch, scene, yr.edge_rays(scene)[name], label=name, group_size=2)


@gpu
@pytest.mark.parametrize("family", ["tangent_casts", "tangent_segments", "surface_ends",
                                    "on_and_inside", "fallback"])
def test_never_rejects(pkg, rt, family):
    """tests/test_sphere_groups.py's families at one origin scale per decade
    (64 rays per sphere and decade): the kernels' words are the unculled
    host's."""
    torch = pytest.importorskip("torch")
    scene, c, r = ts.never_rejects_scene(pkg)
    rng = np.random.default_rng(3)
    parts = []
    for s in range(len(r)):
        o, d = ts.FAMILIES[family](c[s], r[s], rng, 7 * 64)
        parts.append(ts.rays_of(o, d))
    rays = np.concatenate(parts)
    got, tri, occ = compare(pkg, rt, torch, scene, rays, label=family, group_size=3)
    if family not in ("fallback",):
        assert (got["object"] >= 0).sum() >= 200


@gpu
def test_always_kept_groups(pkg, rt):
    torch = pytest.importorskip("torch")
    scene = odd_spheres(pkg, 40, seed=11)
    compare(pkg, rt, torch, scene, yr.random_rays(scene, 771, 53), label="always kept")


@gpu
def test_nothing_to_hit_nothing_to_cast(pkg, rt):
    """The empty scene and a scene of cubes alone with NULL groups; n == 0 is
    RT_OK and writes nothing."""
    torch = pytest.importorskip("torch")
    base = lr.base(pkg)
    rays = yr.random_rays(base, 257, 47, skips=[-1])
    got, tri, occ = compare(pkg, rt, torch, pkg.Scene(), rays, label="empty")
    assert (got["object"] == -1).all() and (got["t"] == K_FAR).all() and not occ.any()
    cubes = pkg.Scene(cube_vertices=base.cube_vertices, cube_colours=base.cube_colours)
    got, tri, occ = compare(pkg, rt, torch, cubes, rays, label="cubes only")
    assert (got["object"] >= 0).sum() >= 20
    spheres = pkg.Scene(base.sphere_origins, base.sphere_radius, base.sphere_colours)
    got, tri, occ = compare(pkg, rt, torch, spheres, rays, label="spheres only")
    assert (got["object"] >= 0).sum() >= 20 and (tri == -1).all()
    ds, keep = device_scene(torch, base)
    acc_buf, acc_ptr = ta.device_build(pkg, rt, torch, ds, base.num_cubes)
    grp_buf, grp_ptr, ng, ws = device_groups(pkg, rt, torch, ds, base.num_spheres, 8)
    rd = upload_rays(torch, pkg, rays)
    hits, hits_ptr = guarded_words(torch, 16)
    flags, flags_ptr = guarded_bytes(torch, 16)
    torch.cuda.synchronize()
    rt.cast_rays_grouped_device(rd.data_ptr(), 0, ds, acc_ptr, grp_ptr, ng, hits_ptr, hits_ptr)
    rt.occlude_rays_grouped_device(rd.data_ptr(), 0, ds, acc_ptr, grp_ptr, ng, flags_ptr)
    assert (body_words(torch, hits) == PATTERN).all()
    assert (body_bytes(torch, flags) == BYTE_PATTERN).all()
    del keep


# --- 3. the fused camera cast ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("camera", ["reference", "pinhole"])
@pytest.mark.parametrize("rows", [None, (5, 17)], ids=["frame", "band"])
def test_camera(pkg, rt, camera, rows):
    """cast_camera_grouped_device equals cast_rays_grouped on camera_rays, the
    host's grouped frame and the device's fused cast through the cube records
    alone."""
    torch = pytest.importorskip("torch")
    w, h = 37, 29
    scene = lr.base(pkg)
    cam = pkg.Camera.reference() if camera == "reference" else \
        pkg.Camera.pinhole((30, 20, 90), (32, 24, -40), (0, -1, 0), 50.0, w, h)
    band = rows or (0, h)
    n = (band[1] - band[0]) * w
    accel, groups = pkg.build_accel(scene), pkg.build_sphere_groups(scene, 4)
    want, want_tri = pkg.cast_rays_grouped(pkg.camera_rays(cam, w, h, rows), scene, accel, groups,
                                           triangles=True)
    assert same(want, pkg.cast_camera_grouped(cam, scene, accel, groups, w, h, rows))
    assert same(want, pkg.cast_camera(cam, scene, w, h, rows))
    assert (want["object"] >= 0).sum() >= 20 and (want["object"] == -1).sum() >= 20
    ds, keep = device_scene(torch, scene)
    acc_buf, acc_ptr = ta.device_build(pkg, rt, torch, ds, scene.num_cubes)
    grp_buf, grp_ptr, ng, ws = device_groups(pkg, rt, torch, ds, scene.num_spheres, 4)
    results = []
    for grouped in (True, False):
        for triangles in (True, False):
            hits, hits_ptr = guarded_words(torch, 2 * n)
            tri, tri_ptr = guarded_words(torch, n) if triangles else (None, 0)
            torch.cuda.synchronize()
            if grouped:
                rt.cast_camera_grouped_device(cam, ds, acc_ptr, grp_ptr, ng, w, band, hits_ptr,
                                              tri_ptr)
            else:
                rt.cast_camera_accel_device(cam, ds, acc_ptr, w, band, hits_ptr, tri_ptr)
            got, got_tri = read_cast(pkg, torch, hits, tri)
            assert same(got.reshape(want.shape), want), (grouped, triangles)
            if triangles:
                assert same(got_tri.reshape(want.shape), want_tri), grouped
            results.append(got)
    assert all(same(r, results[0]) for r in results)
    del keep


# --- 4. build, build, cast, occlude on one stream ----------------------------------------------
@gpu
def test_build_cast_occlude_on_one_stream(pkg, rt):
    torch = pytest.importorskip("torch")
    scene = ta.many(pkg)
    rays = yr.random_rays(scene, 2573, 59)
    n, ns = rays.size, scene.num_spheres
    lib = pkg.library()
    ng = lib.rt_sphere_groups_count(ns, 8)
    ws_bytes = lib.rt_sphere_groups_workspace_bytes(ns)
    ds, keep = device_scene(torch, scene)
    rd = upload_rays(torch, pkg, rays)
    acc_buf, acc_ptr = guarded_words(torch, ta.RECORD_WORDS * scene.num_cubes)
    grp_buf, grp_ptr = guarded_words(torch, RECORD_WORDS * ng)
    ws, ws_ptr = guarded_words(torch, ws_bytes // 4)
    hits, hits_ptr = guarded_words(torch, 2 * n)
    tri, tri_ptr = guarded_words(torch, n)
    flags, flags_ptr = guarded_bytes(torch, n)
    torch.cuda.synchronize()  # uploads and fills are done before the stream starts
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        rt.build_accel_device(ds, acc_ptr, stream=st)
        rt.build_sphere_groups_device(ds, 8, grp_ptr, ws_ptr, ws_bytes, stream=st)
        rt.cast_rays_grouped_device(rd.data_ptr(), n, ds, acc_ptr, grp_ptr, ng, hits_ptr, tri_ptr,
                                    stream=st)
        rt.occlude_rays_grouped_device(rd.data_ptr(), n, ds, acc_ptr, grp_ptr, ng, flags_ptr,
                                       stream=st)
    stream.synchronize()
    want, want_tri = pkg.cast_rays(rays, scene, triangles=True)
    occ = pkg.occlude_rays(rays, scene)
    assert (want["object"] >= 0).sum() >= 100 and 100 <= occ.sum() <= n - 100
    got, got_tri = read_cast(pkg, torch, hits, tri)
    assert same(got, want) and same(got_tri, want_tri) and same(body_bytes(torch, flags), occ)
    assert records_of(pkg, torch, grp_buf).tobytes() == pkg.build_sphere_groups(scene).tobytes()
    body_words(torch, ws)
    del keep


# --- 5. the headless driver ----------------------------------------------------------------------
@gpu
def test_headless_camera_groups_ppm(pkg, tmp_path):
    """rt_headless --camera ... --accel --groups --ppm writes the bytes of the
    same command with --accel alone."""
    exe = pkg.PKG_DIR / "rt_headless"
    assert exe.exists()
    spec = "320,240,400,320,240,-100,70"
    outs = []
    for extra in (["--accel"], ["--accel", "--groups"]):
        out = tmp_path / f"camera{len(extra)}.ppm"
        r = subprocess.run([str(exe), "--scene", "3", "--width", "64", "--height", "48",
                            "--camera", spec, *extra, "--ppm", str(out)], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append((out.read_bytes(), [l for l in r.stdout.splitlines() if "fnv1a64" in l]))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and outs[0][1]
    assert len(set(outs[0][0][15:])) >= 8  # a picture, not one colour
    for args in (["--groups"], ["--camera", spec, "--groups"]):
        bad = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2
