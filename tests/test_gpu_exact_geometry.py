"""The kernels of the ray queries and the surfaces against exact geometry
(tests/exact_ref.py), directly.

Not a second device-equals-host suite: what a kernel wrote is judged by
`exact_ref` itself, with the families, the caps and the judges of
tests/test_exact_geometry.py, so a defect that header, host function and
restatement share still shows.  Device memory is torch tensors; every output
sits between guard words (test_gpu_rays, light_device), the scene's arrays
between padding, and guards, padding, rays and hit frames must come back
unchanged.  Triangles are judged on a subsample of a few hundred rays (the
family's own); the other rays of a launch are looked at for NaN, foreign ids
and a triangle without a cube.

The file launches kernels of code objects that rt_init does not preload (the
camera light pass), as tests/test_gpu_camera_light.py does; DESIGN.md §3.1i
records what has been seen after such loads.
"""
import numpy as np
import pytest

import exact_ref as ex
import light_device as ld
import rays_ref as yr
import test_exact_geometry as te
import test_gpu_rays as tg
from test_gpu_camera_light import RECORD_WORDS as ACCEL_WORDS
from test_gpu_sphere_groups import device_groups

gpu = pytest.mark.gpu
N = 2573  # rays of a launch: partial waves, several workgroups
SPHERE_ROWS = ["sphere_50_3", "sphere_500_3", "sphere_500_30", "sphere_4096_30"]


def launch_rays(pkg, f, seed):
    """N rays: the family's own (judged in full), then seeded rays of the same
    scene.  Returns (rays, the number judged in full)."""
    own = f.rays[:N]
    if len(own) == N:
        return own, N
    more = yr.random_rays(f.scene, N - len(own), seed, box=((0, 96), (0, 80), (-110, 30)))
    return np.concatenate([own, np.ascontiguousarray(more, pkg.RAY_DTYPE).reshape(-1)]), len(own)


def plausible(f, t, obj, tri=None):
    """Every word of a cast: no NaN, no foreign id, a triangle iff a cube."""
    slots = f.geometry.nc + f.geometry.ns
    assert not np.isnan(t).any() and (obj >= -1).all() and (obj < slots).all()
    assert ((obj == -1) == (t == ex.K_FAR)).all()
    if tri is not None:
        assert ((tri >= 0) == ((obj >= 0) & (obj < f.geometry.nc))).all() and (tri < 12).all()


def judged(f, count, got, tri, label):
    plausible(f, got["t"], got["object"], tri)
    bad = ex.judge_cast(f.pairs, f.ref, got["t"], got["object"], tri, count=count)
    assert not bad, (label, bad)


# --- 1. cast_rays_device, with and without triangles -----------------------------------------
@gpu
def test_cast_rays_device(pkg, rt):
    torch = pytest.importorskip("torch")
    f = te.cast_family(pkg, "base_random")
    te.check_cast_caps(f)
    rays, count = launch_rays(pkg, f, 61)
    ds, keep = ld.padded_device_scene(torch, f.scene)
    rd = tg.upload_rays(torch, pkg, rays)
    got, tri = tg.read_cast(pkg, torch, *tg.device_cast(pkg, rt, torch, ds, rd, N))
    judged(f, count, got, tri, "with triangles")
    got, none = tg.read_cast(pkg, torch, *tg.device_cast(pkg, rt, torch, ds, rd, N,
                                                         triangles=False))
    assert none is None
    judged(f, count, got, None, "without triangles")
    tg.rays_unchanged(torch, rd, rays)
    ld.check_scene_padding(torch, f.scene, keep)
    del keep


@gpu
@pytest.mark.parametrize("name", SPHERE_ROWS)
def test_cast_rays_device_one_sphere(pkg, rt, name):
    torch = pytest.importorskip("torch")
    f = te.cast_family(pkg, name)
    te.check_cast_caps(f)
    rays, count = launch_rays(pkg, f, 0)
    assert count == N
    ds, keep = ld.padded_device_scene(torch, f.scene)
    rd = tg.upload_rays(torch, pkg, rays)
    got, tri = tg.read_cast(pkg, torch, *tg.device_cast(pkg, rt, torch, ds, rd, N))
    judged(f, count, got, tri, name)
    on = f.ref.status[:N] == ex.DECIDED_HIT
    err = np.abs(got["t"][on].astype(np.float64) - f.ref.t[:N][on])
    print(f"{name}: worst t error {(err / f.ref.t[:N][on]).max():.3g} relative, "
          f"{(err / f.ref.tol[:N][on]).max():.3g} of the tolerance")
    tg.rays_unchanged(torch, rd, rays)
    ld.check_scene_padding(torch, f.scene, keep)
    del keep


# --- 2. occlude_rays_device -------------------------------------------------------------------
@gpu
def test_occlude_rays_device(pkg, rt):
    torch = pytest.importorskip("torch")
    for name in ("base_segments", "ends"):
        f = te.segment_family(pkg, name)
        te.check_segment_caps(f)
        rays, count = launch_rays(pkg, f, 62)
        ds, keep = ld.padded_device_scene(torch, f.scene)
        rd = tg.upload_rays(torch, pkg, rays)
        flags = tg.body_bytes(torch, tg.device_occlude(pkg, rt, torch, ds, rd, N))
        assert np.isin(flags, (0, 1)).all()
        bad = ex.judge_occlude(f.ref, flags[:count])
        assert not bad, (name, bad)
        tg.rays_unchanged(torch, rd, rays)
        ld.check_scene_padding(torch, f.scene, keep)
        del keep


# --- 3. the culled casts, records built on the device ----------------------------------------
@gpu
def test_cast_rays_accel_and_grouped_device(pkg, rt):
    torch = pytest.importorskip("torch")
    f = te.cast_family(pkg, "base_random")
    te.check_cast_caps(f)
    rays, count = launch_rays(pkg, f, 63)
    ds, keep = ld.padded_device_scene(torch, f.scene)
    rd = tg.upload_rays(torch, pkg, rays)
    records, accel_ptr = tg.guarded_words(torch, ACCEL_WORDS * f.scene.num_cubes)
    torch.cuda.synchronize()
    rt.build_accel_device(ds, accel_ptr)
    groups, groups_ptr, ng, ws = device_groups(pkg, rt, torch, ds, f.scene.num_spheres, 8)
    built = (tg.body_words(torch, records).copy(), tg.body_words(torch, groups).copy())
    for label in ("accel", "grouped"):
        hits, hits_ptr = tg.guarded_words(torch, 2 * N)
        tri, tri_ptr = tg.guarded_words(torch, N)
        torch.cuda.synchronize()
        if label == "accel":
            rt.cast_rays_accel_device(rd.data_ptr(), N, ds, accel_ptr, hits_ptr, tri_ptr)
        else:
            rt.cast_rays_grouped_device(rd.data_ptr(), N, ds, accel_ptr, groups_ptr, ng, hits_ptr,
                                        tri_ptr)
        got, got_tri = tg.read_cast(pkg, torch, hits, tri)
        judged(f, count, got, got_tri, label)
    assert np.array_equal(tg.body_words(torch, records), built[0]), "cube records"
    assert np.array_equal(tg.body_words(torch, groups), built[1]), "group records"
    tg.body_words(torch, ws)  # (the workspace's guards)
    tg.rays_unchanged(torch, rd, rays)
    ld.check_scene_padding(torch, f.scene, keep)
    del keep


# --- 4. the camera launches through a pinhole ----------------------------------------------------
def pinhole_view(pkg):
    """The frame scene through a pinhole, with the exact hits of its rays."""
    if "pinhole" not in te._CACHE:
        scene = te.frame_scene(pkg)
        cam = pkg.Camera.pinhole((20, 16, 15), (18, 15, -25), (0, -1, 0), 40.0, te.FW, te.FH)
        rays = np.ascontiguousarray(pkg.camera_rays(cam, te.FW, te.FH), pkg.RAY_DTYPE).reshape(-1)
        geometry = ex.Geometry(scene)
        pairs = ex.Pairs(geometry, rays)
        f = te.SimpleNamespace(scene=scene, cam=cam, rays=rays, geometry=geometry, pairs=pairs,
                               ref=ex.closest(pairs), name="pinhole", kind="mixed")
        f.excluded = float((f.ref.status == ex.UNDECIDED).mean())
        f.hits = int((f.ref.status == ex.DECIDED_HIT).sum())
        f.misses = int((f.ref.status == ex.DECIDED_MISS).sum())
        te._CACHE["pinhole"] = f
    return te._CACHE["pinhole"]


@gpu
def test_cast_camera_device_and_bounce_0(pkg, rt):
    torch = pytest.importorskip("torch")
    f = pinhole_view(pkg)
    te.check_frame_caps(f)
    won = te.kinds_of(f.geometry, f.ref.obj[f.ref.status == ex.DECIDED_HIT])
    assert min(won.values()) >= 50, won
    n, rows = te.FW * te.FH, (0, te.FH)
    ds, keep = ld.padded_device_scene(torch, f.scene)
    hits, hits_ptr = tg.guarded_words(torch, 2 * n)
    tri, tri_ptr = tg.guarded_words(torch, n)
    torch.cuda.synchronize()
    rt.cast_camera_device(f.cam, ds, te.FW, rows, hits_ptr, tri_ptr)
    got, got_tri = tg.read_cast(pkg, torch, hits, tri)
    judged(f, n, got, got_tri, "cast_camera_device")
    frame, frame_ptr = tg.guarded_words(torch, 2 * n)
    torch.cuda.synchronize()
    rt.bounce_camera_device(f.cam, ds, 0, te.FW, rows, 0, frame_ptr)
    got = tg.body_words(torch, frame).view(pkg.HIT_DTYPE)
    judged(f, n, got, None, "bounce_camera_device, bounce 0")
    ld.check_scene_padding(torch, f.scene, keep)
    del keep


# --- 5. the light pass on hit frames -------------------------------------------------------------
def on_device(pkg, rt, torch, f, hits, p, what, **kw):
    """One launch of pass `p` on the hit frame `hits` (uploaded here; it must
    come back unchanged) over the padded scene: the unguarded output."""
    ds, keep = ld.padded_device_scene(torch, f.scene)
    hd = ld.upload_hits(torch, hits)
    buf = ld.run_device(p, pkg, rt, torch, ds, hd, te.FW, (0, te.FH), what, d=f.d, **kw)
    got = ld.unguard(torch, pkg, buf, te.FW, (0, te.FH), what)
    assert np.array_equal(hd.cpu().numpy().view(np.uint32), ld.words(hits)), "hit frame"
    ld.check_scene_padding(torch, f.scene, keep)
    del keep
    return got


@gpu
def test_hit_surfaces_device(pkg, rt):
    torch = pytest.importorskip("torch")
    f = te.frame(pkg, "frame", te.FRAME_DIRS["reference"])
    te.check_frame_caps(f)
    # the frame itself from the device, through the reference camera
    ds, keep = ld.padded_device_scene(torch, f.scene)
    buf, ptr = tg.guarded_words(torch, 2 * te.FW * te.FH)
    torch.cuda.synchronize()
    rt.cast_camera_device(pkg.Camera.reference(f.d), ds, te.FW, (0, te.FH), ptr)
    hits = tg.body_words(torch, buf).view(pkg.HIT_DTYPE).reshape(te.FH, te.FW).copy()
    ld.check_scene_padding(torch, f.scene, keep)
    del keep
    judged(f, te.FW * te.FH, hits.ravel(), None, "the frame")
    surf = on_device(pkg, rt, torch, f, hits, "light", "surface")
    bad = te.judge_surfaces(f, hits.ravel(), surf.ravel())
    assert not bad, bad


@gpu
def test_shadow_hits_device(pkg, rt):
    torch = pytest.importorskip("torch")
    f, hits, refs = te.shadow_case(pkg)
    mask = on_device(pkg, rt, torch, f, hits, "shadow", "mask")
    bad = te.judge_shadow(refs, mask.ravel())
    assert not bad, bad


@gpu
def test_bounce_hits_device_first_bounce(pkg, rt):
    torch = pytest.importorskip("torch")
    f, hits, b = te.bounce_case(pkg)
    got = on_device(pkg, rt, torch, f, hits, "mirror", "bounce", depth=1).ravel()
    plausible(f, got["t"], got["object"])
    bad = ex.judge_cast(b.pairs, b.ref, got["t"][b.at], got["object"][b.at])
    assert not bad, bad
