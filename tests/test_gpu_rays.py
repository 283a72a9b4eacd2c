"""rt_cast_rays_device / rt_occlude_rays_device / rt_camera_rays_device /
rt_cast_camera_device on the GPU: the kernels (csrc/rt_rays.hip) against the
host functions (csrc/rt_light.cpp), which tests/test_rays.py pins to the numpy
restatement (tests/rays_ref.py).

Device memory is torch tensors; every output sits between guard words (bytes
for the occlusion flags), and the guards and the ray buffer must come back
unchanged.  Results are compared as raw words; no word is masked.
"""
import subprocess

import numpy as np
import pytest

import light_ref as lr
import rays_ref as yr
import reflect_ref as rr
from gpu_support import H, W, device_scene
from hit_ref import K_FAR
from light_device import GUARD, PATTERN, check_scene_padding, padded_device_scene
from light_ref import words

gpu = pytest.mark.gpu
BYTE_PATTERN, BYTE_GUARD = 0x5A, 256  # the uint8 output's guard: 256 bytes on both sides
COUNTS = [1, 63, 64, 65, 255, 256, 257, 771, 2573]


# ---------------------------------------------------------------------------
# Guarded device buffers
# ---------------------------------------------------------------------------
def guarded_words(torch, n_words):
    """(tensor, address of its body): n_words int32 between GUARD words of PATTERN."""
    buf = torch.full((2 * GUARD + n_words,), PATTERN, dtype=torch.int32, device="cuda:0")
    assert (buf.data_ptr() + 4 * GUARD) % 16 == 0
    return buf, buf.data_ptr() + 4 * GUARD


def guarded_bytes(torch, n):
    """The byte-guard variant: n uint8 between BYTE_GUARD bytes of BYTE_PATTERN."""
    buf = torch.full((2 * BYTE_GUARD + n,), BYTE_PATTERN, dtype=torch.uint8, device="cuda:0")
    return buf, buf.data_ptr() + BYTE_GUARD


def body_words(torch, buf):
    torch.cuda.synchronize()  # every stream, the context's own included
    a = buf.cpu().numpy().view(np.uint32)
    assert (a[:GUARD] == PATTERN).all() and (a[-GUARD:] == PATTERN).all(), "wrote out of bounds"
    return a[GUARD:len(a) - GUARD]


def body_bytes(torch, buf):
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[:BYTE_GUARD] == BYTE_PATTERN).all() and (a[-BYTE_GUARD:] == BYTE_PATTERN).all(), \
        "wrote out of bounds"
    return a[BYTE_GUARD:len(a) - BYTE_GUARD]


def upload_rays(torch, pkg, rays):
    rays = np.ascontiguousarray(rays, pkg.RAY_DTYPE).reshape(-1)
    t = torch.from_numpy(np.concatenate([rays.view(np.int32), np.zeros(8, np.int32)])).to("cuda:0")
    assert t.data_ptr() % 16 == 0  # (never empty: one spare record)
    return t


def rays_unchanged(torch, rays_dev, rays):
    got = rays_dev.cpu().numpy()[:8 * rays.size].view(np.uint32)
    assert np.array_equal(got, words(np.ascontiguousarray(rays).reshape(-1)).reshape(-1)), "ray buffer"


def device_cast(pkg, rt, torch, ds, rays_dev, n, triangles=True, stream=0):
    """cast_rays_device into guarded tensors: ((hits, triangles) tensors)."""
    hits, hits_ptr = guarded_words(torch, 2 * n)
    tri, tri_ptr = guarded_words(torch, n) if triangles else (None, 0)
    if not stream:
        torch.cuda.synchronize()  # the fills and uploads are done
    rt.cast_rays_device(rays_dev.data_ptr(), n, ds, hits_ptr, tri_ptr, stream=stream)
    return hits, tri


def read_cast(pkg, torch, hits, tri):
    got = body_words(torch, hits).view(pkg.HIT_DTYPE)
    return got, (None if tri is None else body_words(torch, tri).view(np.int32))


def device_occlude(pkg, rt, torch, ds, rays_dev, n, stream=0):
    out, ptr = guarded_bytes(torch, n)
    if not stream:
        torch.cuda.synchronize()
    rt.occlude_rays_device(rays_dev.data_ptr(), n, ds, ptr, stream=stream)
    return out


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(words(got) if got.dtype.itemsize >= 4 else got,
                       words(want) if want.dtype.itemsize >= 4 else want)


def compare(pkg, rt, torch, scene, rays, ds=None, host_rays=None, label=""):
    """Cast with triangles, cast without, and occlude on the device against
    the host functions on `host_rays` (default `rays`); the ray buffer must
    come back unchanged.  Returns the device's (hits, triangles, occluded)."""
    keep = None
    if ds is None:
        ds, keep = device_scene(torch, scene)
    flat = np.ascontiguousarray(rays, pkg.RAY_DTYPE).reshape(-1)
    ref = flat if host_rays is None else np.ascontiguousarray(host_rays, pkg.RAY_DTYPE).reshape(-1)
    n = flat.size
    rd = upload_rays(torch, pkg, flat)
    want, want_tri = pkg.cast_rays(ref, scene, triangles=True)
    got, tri = read_cast(pkg, torch, *device_cast(pkg, rt, torch, ds, rd, n))
    assert same(got, want), f"{label} hits"
    assert same(tri, want_tri), f"{label} triangles"
    plain, none = read_cast(pkg, torch, *device_cast(pkg, rt, torch, ds, rd, n, triangles=False))
    assert none is None and same(plain, want), f"{label} hits without triangles"
    occ = body_bytes(torch, device_occlude(pkg, rt, torch, ds, rd, n))
    assert same(occ, pkg.occlude_rays(ref, scene)), f"{label} occluded"
    rays_unchanged(torch, rd, flat)
    del keep
    return got, tri, occ


# --- 1. ray counts: partial waves and workgroups -----------------------------------------
@gpu
@pytest.mark.parametrize("n", COUNTS)
def test_ray_counts(pkg, rt, n):
    torch = pytest.importorskip("torch")
    scene = lr.base(pkg)
    rays = yr.random_rays(scene, 2573, 41)[:n]
    got, tri, occ = compare(pkg, rt, torch, scene, rays, label=f"n={n}")
    if n >= 255:
        assert (got["object"] >= 0).sum() >= 20 and (got["object"] == -1).sum() >= 20
        assert (tri >= 0).sum() >= 5 and 5 <= occ.sum() <= n - 5


# --- 2. what a wave's lanes leave out -----------------------------------------------------
@gpu
def test_waves_by_what_their_lanes_skip(pkg, rt, oracle):
    """The hit-pixel rays of the mirror scene in pixel order (skip = the
    pixel's object), then the same rays with nothing left out: waves whose
    lanes all skip one cube, skip different cubes, skip spheres, skip nothing."""
    torch = pytest.importorskip("torch")
    scene = rr.mirror_scene(pkg)
    hits, r = rr.restated(oracle, "mirror", scene, rr.MIRROR_W, rr.MIRROR_H)
    rays, on = yr.bounce_rays(hits, r)
    assert len(rays) % 64 == 0
    free = rays.copy()
    free["skip"] = -1
    rays = np.concatenate([rays, free])
    skip, nc = rays["skip"].reshape(-1, 64), scene.num_cubes
    one_cube = ((skip == skip[:, :1]).all(1) & (skip[:, 0] >= 0) & (skip[:, 0] < nc)).sum()
    cubes = np.where((skip >= 0) & (skip < nc), skip, -1)
    several_cubes = sum(len(set(row[row >= 0])) >= 2 for row in cubes)
    spheres = (skip >= nc).any(1).sum()
    nothing = (skip == -1).all(1).sum()
    assert one_cube >= 50 and several_cubes >= 10 and spheres >= 20 and nothing >= 200
    got, tri, occ = compare(pkg, rt, torch, scene, rays, label="waves")
    half = len(rays) // 2
    assert same(got[:half], pkg.reflect_hits(hits, scene)[on])
    assert not same(got[:half], got[half:])  # leaving the own object out matters


# --- 3. foreign skip ids ------------------------------------------------------------------
@gpu
def test_foreign_skip_ids(pkg, rt):
    """A skip outside [-1, nc + ns) is no object to the kernel: the host
    refuses the rays, and gives the device's result with those ids as -1.  On
    a padded scene, whose padding must come back unchanged."""
    torch = pytest.importorskip("torch")
    scene = lr.base(pkg)
    n_slots = yr.slots(scene)
    rays = yr.random_rays(scene, 771, 43)
    foreign = np.array([-2, n_slots, n_slots + 1, yr.I32_MIN, yr.I32_MAX, -3, 2 * n_slots],
                       np.int32)
    at = np.arange(0, len(rays), 5)
    rays["skip"][at] = foreign[np.arange(len(at)) % len(foreign)]
    outside = (rays["skip"] < -1) | (rays["skip"] >= n_slots)
    assert outside.sum() == len(at) >= 150
    for call in (pkg.cast_rays, pkg.occlude_rays):
        with pytest.raises(pkg.RtError) as e:
            call(rays, scene)
        assert e.value.status == pkg.RT_ERR_INVALID_ARG
    mapped = rays.copy()
    mapped["skip"][outside] = -1
    ds, keep = padded_device_scene(torch, scene)
    got, tri, occ = compare(pkg, rt, torch, scene, rays, ds=ds, host_rays=mapped, label="foreign")
    assert (got["object"][outside] >= 0).sum() >= 10 and occ[outside].sum() >= 5
    check_scene_padding(torch, scene, keep)
    del keep


# --- 4. numeric edges -----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", yr.EDGE_NAMES)
def test_edge_rays(pkg, rt, name):
    torch = pytest.importorskip("torch")
    scene = lr.base(pkg)
    compare(pkg, rt, torch, scene, yr.edge_rays(scene)[name], label=name)


# --- 5. nothing to hit, nothing to cast ----------------------------------------------------
@gpu
def test_empty_scene_and_no_rays(pkg, rt):
    torch = pytest.importorskip("torch")
    scene = pkg.Scene()
    ds, keep = device_scene(torch, scene)
    assert not any(ds.get(k) for k in ("sphere_origins", "cube_vertices", "lights"))
    rays = yr.random_rays(lr.base(pkg), 257, 47, skips=[-1])
    got, tri, occ = compare(pkg, rt, torch, scene, rays, ds=ds, label="empty")
    assert (got["object"] == -1).all() and (got["t"] == K_FAR).all()
    assert (tri == -1).all() and not occ.any()
    # n == 0 is RT_OK and writes nothing
    base = lr.base(pkg)
    ds, keep = device_scene(torch, base)
    rd = upload_rays(torch, pkg, rays)
    hits, tri = device_cast(pkg, rt, torch, ds, rd, 0)
    assert body_words(torch, hits).size == 0 and body_words(torch, tri).size == 0
    hits, hits_ptr = guarded_words(torch, 16)
    flags, flags_ptr = guarded_bytes(torch, 16)
    torch.cuda.synchronize()
    rt.cast_rays_device(rd.data_ptr(), 0, ds, hits_ptr, hits_ptr)
    rt.occlude_rays_device(rd.data_ptr(), 0, ds, flags_ptr)
    assert (body_words(torch, hits) == PATTERN).all()
    assert (body_bytes(torch, flags) == BYTE_PATTERN).all()
    del keep


# --- 6. many candidates through the scalar loops -------------------------------------------
@gpu
def test_256_primitives(pkg, rt):
    """18 cubes and 40 spheres: 256 primitives, 2573 rays."""
    torch = pytest.importorskip("torch")
    scene = pkg.Scene.synthetic(W, H, 40, 18, seed=11, k=0.3)
    assert 12 * scene.num_cubes + scene.num_spheres == 256
    rays = yr.random_rays(scene, 2573, 53)
    got, tri, occ = compare(pkg, rt, torch, scene, rays, label="256 primitives")
    assert len(np.unique(got["object"])) >= 20 and occ.sum() >= 100


# --- 7. the camera ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h,rows", [(37, 29, None), (37, 29, (5, 17)), (257, 3, None)],
                         ids=["37x29", "37x29_band", "257x3"])
@pytest.mark.parametrize("normalise", [0, 1])
def test_camera(pkg, rt, w, h, rows, normalise):
    """camera_rays_device equals the host; cast_camera_device equals
    cast_rays_device on that buffer equals the host."""
    torch = pytest.importorskip("torch")
    scene = lr.base(pkg)
    cam = pkg.Camera(**dict(yr.generic_camera(normalise), o0=(30.0, 20.0, 40.0)))
    band = rows or (0, h)
    n = (band[1] - band[0]) * w
    want_rays = pkg.camera_rays(cam, w, h, rows)
    want, want_tri = pkg.cast_camera(cam, scene, w, h, rows, triangles=True)
    assert (want["object"] >= 0).sum() >= 20 and (want["object"] == -1).sum() >= 20
    ds, keep = device_scene(torch, scene)
    rays_buf, rays_ptr = guarded_words(torch, 8 * n)
    torch.cuda.synchronize()
    rt.camera_rays_device(cam, w, band, rays_ptr)
    got_rays = body_words(torch, rays_buf).view(pkg.RAY_DTYPE).reshape(want_rays.shape)
    assert same(got_rays, want_rays)
    # cast_rays_device on that buffer, in place
    hits, hits_ptr = guarded_words(torch, 2 * n)
    tri, tri_ptr = guarded_words(torch, n)
    torch.cuda.synchronize()
    rt.cast_rays_device(rays_ptr, n, ds, hits_ptr, tri_ptr)
    from_buffer, from_buffer_tri = read_cast(pkg, torch, hits, tri)
    assert same(body_words(torch, rays_buf).view(pkg.RAY_DTYPE).reshape(want_rays.shape), want_rays)
    # and the fused launch, with and without triangles
    for triangles in (True, False):
        hits, hits_ptr = guarded_words(torch, 2 * n)
        tri, tri_ptr = guarded_words(torch, n) if triangles else (None, 0)
        torch.cuda.synchronize()
        rt.cast_camera_device(cam, ds, w, band, hits_ptr, tri_ptr)
        fused, fused_tri = read_cast(pkg, torch, hits, tri)
        assert same(fused, from_buffer) and same(fused.reshape(want.shape), want)
        if triangles:
            assert same(fused_tri, from_buffer_tri) and same(fused_tri.reshape(want.shape), want_tri)
    del keep


# --- 8. rays, cast, occlude on one stream ------------------------------------------------------
@gpu
def test_camera_cast_occlude_on_one_stream(pkg, rt):
    """camera_rays_device -> cast_rays_device -> occlude_rays_device back to
    back on a non-default stream, no host synchronisation in between."""
    torch = pytest.importorskip("torch")
    scene = lr.base(pkg)
    # 40 units in front of the frame, looking back at it: segments of length 100
    cam = pkg.Camera(o0=(0, 0, 40), ou=(1, 0, 0), ov=(0, 1, 0), d0=(0.05, -0.05, -100.0))
    n = W * H
    ds, keep = device_scene(torch, scene)
    rays_buf, rays_ptr = guarded_words(torch, 8 * n)
    hits, hits_ptr = guarded_words(torch, 2 * n)
    tri, tri_ptr = guarded_words(torch, n)
    flags, flags_ptr = guarded_bytes(torch, n)
    torch.cuda.synchronize()  # uploads and fills are done before the stream starts
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rt.camera_rays_device(cam, W, (0, H), rays_ptr, stream=stream.cuda_stream)
        rt.cast_rays_device(rays_ptr, n, ds, hits_ptr, tri_ptr, stream=stream.cuda_stream)
        rt.occlude_rays_device(rays_ptr, n, ds, flags_ptr, stream=stream.cuda_stream)
    stream.synchronize()
    rays = pkg.camera_rays(cam, W, H)
    want, want_tri = pkg.cast_rays(rays, scene, triangles=True)
    occ = pkg.occlude_rays(rays, scene)
    assert (want["object"] >= 0).sum() >= 1000 and 1000 <= occ.sum() <= n - 1000
    assert same(body_words(torch, rays_buf).view(pkg.RAY_DTYPE).reshape(H, W), rays)
    got, got_tri = read_cast(pkg, torch, hits, tri)
    assert same(got.reshape(H, W), want) and same(got_tri.reshape(H, W), want_tri)
    assert same(body_bytes(torch, flags).reshape(H, W), occ)
    del keep


# --- 9. the headless driver ----------------------------------------------------------------------
@gpu
def test_headless_camera_ppm(pkg, tmp_path):
    """rt_headless --camera ... --ppm on reference scene 1 at 64 x 48: the PPM
    bytes are the Python pipeline's (pinhole -> cast_camera -> shade_hits)."""
    exe = pkg.PKG_DIR / "rt_headless"
    assert exe.exists()
    w, h = 64, 48
    eye, target, fov = (320.0, 240.0, 400.0), (320.0, 240.0, -100.0), 70.0
    out = tmp_path / "camera.ppm"
    spec = ",".join(str(v) for v in (*eye, *target, fov))
    r = subprocess.run([str(exe), "--scene", "1", "--width", str(w), "--height", str(h),
                        "--camera", spec, "--ppm", str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    scene = pkg.Scene.reference(1)
    cam = pkg.Camera.pinhole(eye, target, (0, -1, 0), fov, w, h)
    hits = pkg.cast_camera(cam, scene, w, h)
    assert (hits["object"] >= 0).sum() >= 100 and (hits["object"] == -1).sum() >= 100
    rgb = pkg.shade_hits(hits, scene)[..., :3].astype(np.uint8)  # the Texture's (uint8_t) wrap
    assert out.read_bytes() == f"P6\n{w} {h}\n255\n".encode() + rgb.tobytes()
    assert f"fnv1a64 {pkg.fnv1a64(pkg.shade_hits(hits, scene)):016x}" in r.stdout
