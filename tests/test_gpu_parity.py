"""GPU parity: librt_hip.so (through the C ABI) vs the oracle and the golden
fixtures, bit-exact on the int32x4 frame (the reference's pixels vector,
MainState.cpp:952-955).  Run on an MI355X with `pytest -m gpu`."""
import os
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN, SURVEY_FNV, golden_scene, load_golden, probe_fnv
from gpu_support import (EDGE_CASES, PATHS, SMALL_FIXTURES, THREADS, device_scene, diff_report,
                         knobs, render_all_paths, scene_from)

pytestmark = pytest.mark.gpu


def test_fp32_selftest(rt):
    """sqrtf and '/' on the device must be the correctly rounded IEEE ops the
    reference's x86 build uses (sphere thc, MainState.cpp:318; shade :403)."""
    rng = np.random.default_rng(0)
    x = np.concatenate([
        rng.uniform(0, 1e5, 1 << 20).astype(np.float32),
        rng.uniform(-1e3, 1e3, 1 << 18).astype(np.float32),
        (rng.standard_normal(1 << 18) * 1e-38).astype(np.float32),  # denormals
        np.array([0.0, -0.0, 1.0, 2.0, 180.0, 3.4e38, 1e-45], np.float32),
    ])
    s, q = rt.selftest_fp32(x)
    with np.errstate(invalid="ignore"):
        want_s = np.sqrt(x)
    want_q = x / np.float32(180.0)
    assert np.array_equal(s.view(np.uint32)[x >= 0], want_s.view(np.uint32)[x >= 0])
    assert np.isnan(s[x < 0]).all()
    assert np.array_equal(q.view(np.uint32), want_q.view(np.uint32))


@pytest.mark.parametrize("name", SMALL_FIXTURES)
@pytest.mark.parametrize("path", ["binned", "generic"])
def test_golden_frame(pkg, rt, name, path):
    g = load_golden(name)
    scene = golden_scene(pkg, g)
    w, h = int(g["width"]), int(g["height"])
    frame, t = rt.render(scene, w, h, ray_dir=g["ray_dir"], path=path)
    assert t.path == path
    assert not diff_report(frame, g["frame"]), diff_report(frame, g["frame"])


@pytest.mark.parametrize("scene_id", [1, 2, 3])
@pytest.mark.parametrize("path", ["binned", "generic"])
def test_survey_known_answer(pkg, rt, scene_id, path):
    """The device frame against the reference's own CPU frame as the survey's
    probe hashed it (no oracle in the loop): the FNV-1a-64 of
    all 1,228,800 int32 words equals the probe's known answer."""
    g = load_golden(f"scene{scene_id}_640x480")
    frame, t = rt.render(golden_scene(pkg, g), 640, 480, ray_dir=g["ray_dir"], path=path)
    assert t.path == path
    assert probe_fnv(frame) == SURVEY_FNV[scene_id]


@pytest.mark.parametrize("name", ["scene1_640x480", "scene3_640x480", "config2_1920x1080"])
def test_rgba8_texture(pkg, rt, oracle, name):
    """The Texture packing (MainState.cpp:1023-1037) produced on the device."""
    g = load_golden(name)
    w, h = int(g["width"]), int(g["height"])
    got, _ = rt.render(golden_scene(pkg, g), w, h, fmt="rgba8")
    want = oracle.pack_rgba8(g["frame"])
    assert np.array_equal(got, want)


def test_row_bands_assemble(pkg, rt):
    g = load_golden("scene3_640x480")
    scene = golden_scene(pkg, g)
    bands = [(0, 100), (100, 333), (333, 347), (347, 480)]
    parts = [rt.render(scene, 640, 480, rows=b)[0] for b in bands]
    assert np.array_equal(np.concatenate(parts), g["frame"])


def test_explicit_origins_match(pkg, rt):
    """The reference uploads rayOrigins (MainState.cpp:44-50, :841-855):
    passed explicitly they are recognised as the implicit grid on the device
    and keep the binned path; any other origin value (one pixel off, a -0.0
    z) takes the generic kernel.  Every frame equals the golden one where
    the rays are the same."""
    g = load_golden("scene2_640x480")
    scene = golden_scene(pkg, g)
    ys, xs = np.mgrid[0:480, 0:640]
    org = np.stack([xs, ys, np.zeros_like(xs), np.ones_like(xs)], -1).astype(np.float32)
    frame, t = rt.render(scene, 640, 480, ray_origins=org)
    assert t.path == "binned"
    assert np.array_equal(frame, g["frame"])
    band, t = rt.render(scene, 640, 480, rows=(100, 333), ray_origins=org)
    assert t.path == "binned" and np.array_equal(band, g["frame"][100:333])
    negz = org.copy()
    negz[5, 7, 2] = -0.0
    frame, t = rt.render(scene, 640, 480, ray_origins=negz)
    assert t.path == "generic"
    assert np.array_equal(frame, g["frame"])
    off = org.copy()
    off[479, 639, 0] = 639.5
    _, t = rt.render(scene, 640, 480, ray_origins=off)
    assert t.path == "generic"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_general_rays_vs_oracle(pkg, rt, oracle, seed):
    """Arbitrary directions and origins (kernel args 8-9 in full generality)."""
    rng = np.random.default_rng(seed)
    w, h = 96, 72
    scene = pkg.Scene.synthetic(w, h, 12, 6, seed=seed, k=0.3)
    d = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), -1.0, -1.0], np.float32)
    org = np.zeros((h, w, 4), np.float32)
    org[..., 0] = np.arange(w)[None, :] + rng.uniform(-0.5, 0.5, (h, w))
    org[..., 1] = np.arange(h)[:, None] + rng.uniform(-0.5, 0.5, (h, w))
    org[..., 2] = rng.uniform(-5, 5, (h, w))
    org[..., 3] = 1.0
    for origins in (None, org):
        got, t = rt.render(scene, w, h, ray_dir=d, ray_origins=origins)
        assert t.path == "generic"
        want = oracle.trace(scene, w, h, ray_dir=d, ray_origins=origins)
        assert not diff_report(got, want), diff_report(got, want)


@pytest.mark.parametrize("seed", range(6))
def test_dense_synthetic_vs_oracle(pkg, rt, oracle, seed):
    """Dense random scenes at awkward sizes (not multiples of the 32x32 bin)."""
    w, h = 333 + 17 * seed, 257 - 9 * seed
    scene = pkg.Scene.synthetic(w, h, 40 + 10 * seed, 12 + 4 * seed, seed=100 + seed,
                                k=w / 640 * (1 + seed % 3))
    got, t = rt.render(scene, w, h)
    assert t.path == "binned"
    want = oracle.trace(scene, w, h, threads=THREADS)
    assert not diff_report(got, want), diff_report(got, want)


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
@pytest.mark.parametrize("size", [(101, 77), (1, 1), (64, 64)])
def test_edge_cases(pkg, rt, oracle, case, size):
    """Every edge scene through every kernel of the path matrix
    (gpu_support.PATHS: generic, both small-scene kernels,
    trace3_kernel with and without the forced depth culls, the split trace,
    trace_bin_kernel, the wide tile build) in both formats, the kernel that
    ran asserted, each frame the oracle's bit for bit."""
    w, h = size
    scene = scene_from(pkg, **EDGE_CASES[case])
    n = render_all_paths(rt, oracle, scene, w, h, label=f"{case} {w}x{h}")
    assert n == 2 * len(PATHS)


def test_nonfinite_scene_falls_back_exactly(pkg, rt, oracle):
    """NaN / inf scene data: the binned launch detects it on the device and
    runs the verbatim reference algorithm (no CPU fallback)."""
    scene = scene_from(pkg, spheres=[((30, 30, -40, 1), np.inf, (1, .5, .5, 255)),
                                     ((60, 30, -40, 1), 10, (.5, 1, .5, 255))],
                       cubes=[([("scale", 10, 10, 10), ("translate", 40, 40, -30)],
                               (.5, .5, 1, 255))])
    scene.cube_vertices[0, 4, 0] = np.nan
    want = oracle.trace(scene, 90, 70)
    for small, fused in ((True, True), (True, False), (False, False)):
        with knobs(rt, small_path=small, small_fused=2 if fused else 0):
            got, t = rt.render(scene, 90, 70)
            assert t.path == "binned"
            assert np.array_equal(got, want), (small, fused)
    # a second chunk's primitive non-finite (frame_small_kernel's second
    # prep wave)
    big = pkg.Scene.synthetic(90, 70, 100, 0, seed=4, k=0.2)
    big.sphere_radius[90] = np.nan
    want = oracle.trace(big, 90, 70)
    for fused in (True, False):
        with knobs(rt, small_fused=2 if fused else 0):
            got, _ = rt.render(big, 90, 70)
            assert np.array_equal(got, want), fused


@pytest.mark.parametrize("w,h,ns,nc,k", [(512, 512, 4, 1, 1.0), (1920, 1080, 16, 4, 3.0),
                                         (1000, 777, 40, 2, 2.0), (333, 4100, 64, 0, 2.0),
                                         (4160, 70, 4, 5, 3.0), (777, 555, 16, 4, 2.5),
                                         (640, 480, 8, 10, 1.0), (1920, 1080, 32, 8, 3.0),
                                         (1500, 900, 65, 0, 2.0), (1920, 1080, 64, 16, 3.0),
                                         (2000, 1300, 100, 13, 2.0), (1920, 1080, 128, 32, 3.0),
                                         (1111, 999, 300, 10, 2.0), (3000, 700, 512, 0, 3.0),
                                         # frame_small_kernel's prep waves: triangles only
                                         # (two triangle waves, no sphere wave busy); two
                                         # sphere waves beside one triangle wave
                                         (800, 600, 0, 10, 2.0), (900, 700, 68, 5, 2.0)])
def test_small_scene_path(pkg, rt, oracle, w, h, ns, nc, k):
    """<= 512 primitives (up to 8 prep chunks): trace_small_kernel classifies
    each tile's candidates itself; <= 128 primitives: frame_small_kernel does
    prep, classification and trace in one kernel.  Same frames from all
    three and the general path and the oracle, whole frames, row bands and
    the Texture format; 513 primitives take the general path."""
    scene = pkg.Scene.synthetic(w, h, ns, nc, seed=w + ns, k=k)
    assert ns + 12 * nc <= 512
    frames = {}
    for small, fused in ((True, True), (True, False), (False, False)):
        with knobs(rt, small_path=small, small_fused=2 if fused else 0):
            full, t = rt.render(scene, w, h)
            assert t.path == "binned"
            band, _ = rt.render(scene, w, h, rows=(h // 3, h - h // 5))
            assert np.array_equal(band, full[h // 3:h - h // 5])
            tex, _ = rt.render(scene, w, h, fmt="rgba8")
            assert np.array_equal(tex, pkg.pack_rgba8(full))
            frames[small, fused] = full
    assert np.array_equal(frames[True, True], frames[False, False])
    assert np.array_equal(frames[True, False], frames[False, False])
    frames[True] = frames[True, True]
    want = oracle.trace(scene, w, h, threads=THREADS)
    assert not diff_report(frames[True], want), diff_report(frames[True], want)
    # one more primitive: the general path
    big = pkg.Scene.synthetic(w, h, 513 - 12 * nc, nc, seed=w, k=k)
    got, _ = rt.render(big, w, h)
    assert np.array_equal(got, oracle.trace(big, w, h, threads=THREADS))


def test_deterministic(pkg, rt):
    scene = pkg.Scene.synthetic(1024, 768, 128, 32, seed=9, k=1.6)
    a, _ = rt.render(scene, 1024, 768)
    b, _ = rt.render(scene, 1024, 768)
    assert np.array_equal(a, b)


def test_lights_do_not_change_pixels(pkg, rt):
    """The reference has no lighting model (MainState.h:97-106): lights are
    carried through the ABI and must not affect the frame."""
    s0 = pkg.Scene.synthetic(256, 200, 16, 4, seed=2, k=0.8, n_lights=0)
    s2 = pkg.Scene.synthetic(256, 200, 16, 4, seed=2, k=0.8, n_lights=2)
    assert np.array_equal(rt.render(s0, 256, 200)[0], rt.render(s2, 256, 200)[0])


@pytest.mark.parametrize("trace_bin,kernel", [(1, "trace_bin_kernel"), (2, "trace3_kernel")])
def test_config3_full_frame(pkg, oracle, trace_bin, kernel):
    """BASELINE config 3 at full size (4096^2, 256 spheres + 64 cubes, dense),
    the headline workload, on a FRESH context with the path pinned:
    rt_debug_set_trace_bin 1 = prep -> trace_bin_kernel (the kernel that
    produces the bench's `value`), 2 = prep -> coarse -> trace3_kernel.  The
    kernel that ran is asserted, and the whole frame's FNV-1a-64 equals the
    oracle's (tests/golden/config3_4096x4096.npz `fnv1a64`); its Texture form
    (RGBA8, MainState.cpp:1023-1037, the bench's second leg) equals the
    fixture's `fnv1a64_rgba8`.  On the trace_bin context, band renders
    assemble to the same frame and a row sample matches the oracle.
    Reference scope: MainState.cpp:858-907 (launch and readback)."""
    g = load_golden("config3_4096x4096")
    scene = golden_scene(pkg, g)
    w, h = int(g["width"]), int(g["height"])
    with pkg.RayTracer(0) as fresh, knobs(fresh, trace_bin=trace_bin):
        frame, t = fresh.render(scene, w, h)
        assert t.path == "binned"
        assert fresh.last_kernel() == kernel
        assert pkg.fnv1a64(frame) == int(g["fnv1a64"])
        # a second frame on the same context (after the first verdict)
        again, _ = fresh.render(scene, w, h)
        assert fresh.last_kernel() == kernel
        assert np.array_equal(again, frame)
        del again
        tex, _ = fresh.render(scene, w, h, fmt="rgba8")
        # RGBA8 at this overdraw (2.8 >= 1) takes the coarse path unless forced
        assert fresh.last_kernel() == kernel
        assert pkg.fnv1a64(tex) == int(g["fnv1a64_rgba8"])
        del tex
        if trace_bin == 1:
            half, _ = fresh.render(scene, w, h, rows=(1000, 3000))
            assert np.array_equal(half, frame[1000:3000])
            del half
    if trace_bin == 1:
        rows = list(range(0, h, 256)) + [h - 1]
        for r in rows[::4]:
            want = oracle.trace(scene, w, h, rows=(r, r + 1))
            assert np.array_equal(frame[r:r + 1], want), f"row {r}"


def test_config5_style_4096_spheres(pkg, rt, oracle):
    """Config 5's scene type (4096 spheres, no cubes) on a
    2048^2 frame: long candidate lists per coarse bin (several coarse-kernel
    LDS rounds), checked on a row sample, and band renders assemble to the
    full frame."""
    w = h = 2048
    scene = pkg.Scene.synthetic(w, h, 4096, 0, seed=5, k=w / 640)
    frame, t = rt.render(scene, w, h)
    assert t.path == "binned"
    for r in list(range(0, h, 173)) + [h - 1]:
        want = oracle.trace(scene, w, h, rows=(r, r + 1), threads=THREADS)
        assert np.array_equal(frame[r:r + 1], want), f"row {r}"
    bands = [rt.render(scene, w, h, rows=(b, min(b + 700, h)))[0] for b in range(0, h, 700)]
    assert np.array_equal(np.concatenate(bands), frame)


def test_config4_style_band_of_8192_frame(pkg, rt, oracle):
    """Config 4's layout: one rank's row band (rows 3072..4095 of an 8192^2
    frame, 192 spheres + 64 cubes over the whole frame) rendered on its
    own: band-relative tiles and coarse bins, primitives clamped to the
    band."""
    w = h = 8192
    scene = pkg.Scene.synthetic(w, h, 192, 64, seed=4, k=w / 640)
    rb, re = 3072, 4096
    band, t = rt.render(scene, w, h, rows=(rb, re))
    assert t.path == "binned" and band.shape == (re - rb, w, 4)
    for r in list(range(rb, re, 97)) + [re - 1]:
        want = oracle.trace(scene, w, h, rows=(r, r + 1), threads=THREADS)
        assert np.array_equal(band[r - rb:r - rb + 1], want), f"row {r}"


def test_device_api_into_torch(pkg, rt):
    """rt_render_device writing into a torch tensor on the current stream."""
    torch = pytest.importorskip("torch")
    g = load_golden("scene1_640x480")
    scene = golden_scene(pkg, g)
    ds, keep = device_scene(torch, scene)
    out = torch.empty((480, 640, 4), dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    rt.render_device(ds, 640, 480, (0, 480), out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), g["frame"])
    del keep


def test_candidate_lists_larger_than_lds_round(pkg, rt, oracle):
    """Hundreds of candidates in one 64x64 coarse bin: the coarse kernel
    classifies them in several LDS rounds (kRound = 64) and the trace walks
    them 8 at a time, the reference's primitive order preserved."""
    w, h = 100, 90
    scene = pkg.Scene.synthetic(w, h, 700, 40, seed=11, k=0.4)
    got, t = rt.render(scene, w, h)
    assert t.path == "binned"
    want = oracle.trace(scene, w, h, threads=THREADS)
    assert not diff_report(got, want), diff_report(got, want)


@pytest.mark.parametrize("scene_id", [1, 2, 3])
def test_headless_cpp_driver(pkg, scene_id, tmp_path):
    """The C++ host (host/rt_headless.cpp: MainState's createSceneN +
    executeRayTracerOpenCL flow through the C ABI) reproduces the golden
    frame: its FNV-1a-64 line and its PPM Texture dump (MainState.cpp:
    1026-1028 wrap)."""
    import subprocess

    exe = Path(pkg.library_path()).parent / "rt_headless"
    if not exe.exists():
        pytest.skip("rt_headless not built")
    g = load_golden(f"scene{scene_id}_640x480")
    ppm = tmp_path / "frame.ppm"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(exe.parent) + ":" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([str(exe), "--scene", str(scene_id), "--seed", "1", "--ppm", str(ppm)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"fnv1a64 {int(g['fnv1a64']):016x}" in r.stdout, r.stdout
    data = ppm.read_bytes()
    header = b"P6\n640 480\n255\n"
    assert data.startswith(header)
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(480, 640, 3)
    assert np.array_equal(rgb, g["frame"][..., :3].astype(np.uint8))


@pytest.mark.parametrize("scene_id,bands", [(1, 1), (2, 1), (3, 1), (3, 3)])
def test_headless_cpp_driver_rgba8(pkg, oracle, scene_id, bands, tmp_path):
    """The C++ host asking for the Texture format (rt_headless --format rgba8:
    rt_render_multi with RT_FORMAT_RGBA8 into a uint32 buffer, the layout
    SDL_CreateRGBSurfaceFrom(buf, w, h, 32, 4 w, 0xff, 0xff00, 0xff0000,
    0xff000000) wraps) gets exactly the oracle's Texture
    packing of the golden frame (MainState.cpp:1023-1037): the printed hash
    over the words and the PPM it writes from them."""
    import subprocess

    exe = Path(pkg.library_path()).parent / "rt_headless"
    if not exe.exists():
        pytest.skip("rt_headless not built")
    g = load_golden(f"scene{scene_id}_640x480")
    want = oracle.pack_rgba8(g["frame"])
    ppm = tmp_path / "texture.ppm"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(exe.parent) + ":" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([str(exe), "--scene", str(scene_id), "--seed", "1", "--format", "rgba8",
                        "--bands", str(bands), "--ppm", str(ppm)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"rgba8 fnv1a64 {pkg.fnv1a64(want):016x}" in r.stdout, r.stdout
    data = ppm.read_bytes()
    header = b"P6\n640 480\n255\n"
    assert data.startswith(header)
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(480, 640, 3)
    words = want.astype(np.uint32)
    assert np.array_equal(rgb, np.stack([(words >> (8 * c)) & 0xff for c in range(3)],
                                        -1).astype(np.uint8))
    assert np.all((words >> 24) == 0xff)


@pytest.mark.parametrize("scene_id", [1, 2, 3])
@pytest.mark.parametrize("bands", [1, 3])
def test_headless_known_answer(pkg, scene_id, bands):
    """rt_headless --known-answer: the C++ host checks its frame against the
    reference's own CPU frame as the survey's probe recorded it (SURVEY.md
    §8c), with no Python or oracle in the loop; one band and three bands
    (rt_render_multi) both match."""
    import subprocess

    exe = Path(pkg.library_path()).parent / "rt_headless"
    if not exe.exists():
        pytest.skip("rt_headless not built")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(exe.parent) + ":" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([str(exe), "--scene", str(scene_id), "--bands", str(bands),
                        "--known-answer"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"known answer scene {scene_id}: {SURVEY_FNV[scene_id]:016x}" in r.stdout, r.stdout
    assert "match" in r.stdout and "MISMATCH" not in r.stdout


@pytest.mark.parametrize("fmt,slots,w,h", [("i32x4", 2, 1280, 1024), ("rgba8", 3, 1280, 1024),
                                          ("rgba8", 2, 1280, 1024), ("i32x4", 2, 4096, 4096),
                                          ("rgba8", 2, 4096, 4096)])
def test_headless_cpp_driver_throughput(pkg, oracle, fmt, slots, w, h):
    """rt_headless --throughput: the bench's frame loop in C++ (device scene,
    slots on CU-masked streams, the automatic path -- trace_bin_kernel for
    int32x4 at this density) ends with every slot's last frame equal to the
    oracle's frame (hash), and reports a positive rate.  At 4096^2 (BASELINE
    config 3, the headline workload: the loop that produces `value`, 2
    CU-masked slots) the hash is the committed fixture's
    (tests/golden/config3_4096x4096.npz fnv1a64 / fnv1a64_rgba8)."""
    import re
    import subprocess

    exe = Path(pkg.library_path()).parent / "rt_headless"
    if not exe.exists():
        pytest.skip("rt_headless not built")
    if (w, h) == (4096, 4096):
        g = load_golden("config3_4096x4096")
        want_hash = int(g["fnv1a64" if fmt == "i32x4" else "fnv1a64_rgba8"])
        frames = "400"
    else:
        scene = pkg.Scene.synthetic(w, h, 256, 64, seed=3, k=w / 640)
        want = oracle.trace(scene, w, h, threads=THREADS)
        words = want if fmt == "i32x4" else oracle.pack_rgba8(want)
        want_hash = oracle.fnv(np.ascontiguousarray(words).view(np.int32))
        frames = "64"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(exe.parent) + ":" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([str(exe), "--synthetic", "256", "64", str(w / 640), "--seed", "3",
                        "--width", str(w), "--height", str(h), "--format", fmt,
                        "--throughput", frames, "--inflight", str(slots)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    hashes = re.findall(r"slot (\d+) fnv1a64 ([0-9a-f]{16})", r.stdout)
    assert len(hashes) == slots, r.stdout
    assert {hv for _, hv in hashes} == {f"{want_hash:016x}"}, r.stdout
    rate = float(re.search(r"([0-9.]+) Grays/s", r.stdout).group(1))
    assert rate > 0
    if fmt == "i32x4":
        assert "kernel 6" in r.stdout, r.stdout  # RT_KERNEL_TRACE_BIN


@pytest.mark.parametrize("args", [["--synthetic", "256", "64", "6.4", "--width", "1024",
                                   "--height", "768"],
                                  ["--synthetic", "40", "5", "2", "--width", "999",
                                   "--height", "333", "--rows", "17", "300"],
                                  ["--synthetic", "0", "0", "1", "--width", "64",
                                   "--height", "64"]])
def test_headless_cpp_driver_device_scene(pkg, args):
    """The C++ host building the synthetic scene on the device
    (rt_scene_synthetic_device) and rendering from the device arrays prints
    the same frame hash as with the host-built scene (whose frames the
    oracle checks in the tests above)."""
    import re
    import subprocess

    exe = Path(pkg.library_path()).parent / "rt_headless"
    if not exe.exists():
        pytest.skip("rt_headless not built")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(exe.parent) + ":" + env.get("LD_LIBRARY_PATH", "")
    hashes = []
    for extra in ([], ["--device-scene"]):
        r = subprocess.run([str(exe), "--seed", "9"] + args + extra, capture_output=True,
                           text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr
        hashes.append(re.search(r"fnv1a64 ([0-9a-f]{16})", r.stdout).group(1))
    assert "device scene" in r.stdout
    assert hashes[0] == hashes[1]


@pytest.mark.parametrize("bands", [3, 7])
def test_headless_cpp_driver_bands(pkg, bands, tmp_path):
    """rt_headless --bands: concurrent host threads, one rt_ctx each
    (several contexts on the one device here), tracing ragged row bands
    into the shared frame -- the same golden hash as the single render,
    for the whole frame and for a sub-range of rows."""
    import subprocess

    exe = Path(pkg.library_path()).parent / "rt_headless"
    if not exe.exists():
        pytest.skip("rt_headless not built")
    g = load_golden("scene3_640x480")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(exe.parent) + ":" + env.get("LD_LIBRARY_PATH", "")
    base = [str(exe), "--scene", "3", "--seed", "1", "--repeat", "2", "--bands", str(bands)]
    r = subprocess.run(base, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"fnv1a64 {int(g['fnv1a64']):016x}" in r.stdout, r.stdout
    assert r.stdout.count(" band ") == 2 * bands, r.stdout
    ppm = tmp_path / "rows.ppm"
    r = subprocess.run(base + ["--rows", "101", "333", "--ppm", str(ppm)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    data = ppm.read_bytes()
    header = b"P6\n640 232\n255\n"
    assert data.startswith(header)
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(232, 640, 3)
    assert np.array_equal(rgb, g["frame"][101:333, :, :3].astype(np.uint8))


def test_band_renders_weak_scaling_layout(pkg, rt, oracle):
    """bench.py's N=8 weak-scaling layout at reduced size: a 1024 x 8192
    frame with 8x the primitives, rendered as 8 row bands (each band's bin
    masks hold only its in-band primitives) -- bit-identical to the
    full-frame render and to the oracle on sampled rows."""
    w, h, ranks = 1024, 8192, 8
    scene = pkg.Scene.synthetic(w, h, 64 * ranks, 16 * ranks, seed=8, k=w / 640)
    full, t = rt.render(scene, w, h)
    assert t.path == "binned"
    for r in range(ranks):
        rb, re = r * h // ranks, (r + 1) * h // ranks
        band, _ = rt.render(scene, w, h, rows=(rb, re))
        assert np.array_equal(band, full[rb:re]), f"band {r}"
    for row in range(0, h, 509):
        want = oracle.trace(scene, w, h, rows=(row, row + 1), threads=THREADS)
        assert np.array_equal(full[row:row + 1], want), f"row {row}"


@pytest.mark.parametrize("w,h,ns,nc,k", [(640, 480, 60, 12, 1.0), (1000, 777, 500, 40, 1.2),
                                         (333, 4100, 200, 20, 2.0), (4160, 70, 300, 30, 3.0)])
def test_bin_masks_match_box_scan(pkg, rt, oracle, w, h, ns, nc, k):
    """Coarse binning from the separable bin-row / bin-column masks equals
    the scan of every box (the extreme-aspect path), on full frames and row
    bands, and both match the oracle."""
    scene = pkg.Scene.synthetic(w, h, ns, nc, seed=w + h, k=k)
    frames = {}
    for masks in (True, False):
        with knobs(rt, bin_masks=masks):
            full, t = rt.render(scene, w, h)
            assert t.path == "binned"
            band, _ = rt.render(scene, w, h, rows=(h // 3, h - h // 5))
            assert np.array_equal(band, full[h // 3:h - h // 5])
            frames[masks] = full
    assert np.array_equal(frames[True], frames[False])
    want = oracle.trace(scene, w, h, threads=THREADS)
    assert not diff_report(frames[True], want), diff_report(frames[True], want)


def test_error_paths_on_device(pkg, rt):
    """Status codes through the C ABI on a real device (rt_error_string
    convention, MainState.cpp:1101-1179 replaced): forcing the binned path
    on rays it cannot take is RT_ERR_UNSUPPORTED; bad sizes and rows are
    RT_ERR_INVALID_ARG; the context stays usable afterwards."""
    scene = pkg.Scene.reference(1, 1)
    w, h = 64, 48
    origins = np.zeros((h, w, 4), np.float32)
    origins[..., 0], origins[..., 1] = np.meshgrid(np.arange(w), np.arange(h))
    origins[..., 3] = 1.0
    shifted = origins.copy()
    shifted[..., 0] += 0.25  # not the implicit grid
    with pytest.raises(pkg.RtError) as e:
        rt.render(scene, w, h, ray_origins=shifted, path="binned")
    assert e.value.status == pkg.RT_ERR_UNSUPPORTED
    with pytest.raises(pkg.RtError) as e:
        rt.render(scene, w, h, ray_dir=np.float32([0.3, 0.0, -1.0, -1.0]), path="binned")
    assert e.value.status == pkg.RT_ERR_UNSUPPORTED
    for rows in ((10, 10), (-1, 5), (0, h + 1)):
        with pytest.raises(pkg.RtError) as e:
            rt.render(scene, w, h, rows=rows)
        assert e.value.status == pkg.RT_ERR_INVALID_ARG
    # explicit origins equal to the implicit grid (what the reference
    # uploads, MainState.cpp:44-50) keep the binned path; forcing the
    # generic kernel gives the same frame
    frame, t = rt.render(scene, w, h)
    same, t2 = rt.render(scene, w, h, ray_origins=origins)
    gen, t3 = rt.render(scene, w, h, ray_origins=origins, path="generic")
    assert (t.path, t2.path, t3.path) == ("binned", "binned", "generic")
    assert np.array_equal(frame, same) and np.array_equal(frame, gen)


def test_very_many_primitives(pkg, rt, oracle):
    """30,000 small spheres and 200 cubes on a 512^2 frame: hundreds of
    candidates per coarse bin (many coarse-kernel rounds, long lists)."""
    w = h = 512
    scene = pkg.Scene.synthetic(w, h, 30000, 200, seed=21, k=0.3)
    frame, t = rt.render(scene, w, h)
    assert t.path == "binned"
    for r in (0, 97, 255, 256, 400, 511):
        want = oracle.trace(scene, w, h, rows=(r, r + 1), threads=THREADS)
        assert np.array_equal(frame[r:r + 1], want), f"row {r}"


def _shifted(pkg, scene, dx=0.0, dy=0.0):
    """The scene translated by (dx, dy) in float32, as the host would
    store it (cube vertices already world-space, MainState.cpp:646-655)."""
    so = scene.sphere_origins.copy()
    so[:, 0] += np.float32(dx)
    so[:, 1] += np.float32(dy)
    cv = scene.cube_vertices.copy()
    cv[:, :, 0] += np.float32(dx)
    cv[:, :, 1] += np.float32(dy)
    return pkg.Scene(so, scene.sphere_radius, scene.sphere_colours, cv, scene.cube_colours)


@pytest.mark.parametrize("w,h", [(1 << 24, 1), (1 << 21, 3), (3, 1 << 21)])
def test_extreme_aspect_frames(pkg, rt, oracle, w, h):
    """The ABI's coordinate limit (2^24, the last width at which float
    pixel coordinates are exact) and extreme aspect ratios: one coarse row
    of up to 262,144 bins, or one coarse column of 32,768. Primitives sit
    at the far end of the long axis. Whole frame against the oracle, and
    binned == generic."""
    base = pkg.Scene.synthetic(min(w, 4096), min(h, 4096), 240, 24, seed=5, k=1.0)
    scene = _shifted(pkg, base, dx=max(w - 4096, 0), dy=max(h - 4096, 0))
    got, t = rt.render(scene, w, h)
    assert t.path == "binned"
    gen, t = rt.render(scene, w, h, path="generic")
    assert t.path == "generic"
    assert np.array_equal(got, gen)
    if w % 4096 == 0:
        # the oracle splits work by rows: give it the same rays as explicit
        # origins (exact integers below 2^24) folded into 4096-wide rows
        ys, xs = np.divmod(np.arange(w * h, dtype=np.int64), w)
        org = np.stack([xs, ys, np.zeros_like(xs), np.ones_like(xs)], -1).astype(np.float32)
        want = oracle.trace(scene, 4096, w * h // 4096, ray_origins=org,
                            threads=THREADS).reshape(h, w, 4)
    else:
        want = oracle.trace(scene, w, h, threads=THREADS)
    assert not diff_report(got, want), diff_report(got, want)
    assert (got[..., 0] != 0).sum() > 1000  # the far end really is drawn


def test_maximum_size_frames(pkg, rt, oracle):
    """A 16384 x 16400 frame (268.7 M rays, past the generic kernel's
    2^28-thread grid, so its grid-stride loop runs twice) in RGBA8 on both
    paths, bit-equal; and a 16384^2 int32x4 frame (4 GiB) on sampled rows
    against the oracle."""
    w = 16384
    scene = pkg.Scene.synthetic(w, w, 256, 64, seed=9, k=w / 640)
    a, t = rt.render(scene, w, 16400, fmt="rgba8")
    assert t.path == "binned"
    b, t = rt.render(scene, w, 16400, fmt="rgba8", path="generic")
    assert t.path == "generic"
    assert np.array_equal(a, b)
    del b
    rows = [0, 4095, 8191, 12288, 16383, 16399]
    want = oracle.trace_rows(scene, w, 16400, rows, threads=THREADS)
    assert np.array_equal(a[rows], oracle.pack_rgba8(want))
    del a
    full, t = rt.render(scene, w, w)
    assert t.path == "binned"
    want = oracle.trace_rows(scene, w, w, rows[:-1], threads=THREADS)
    assert np.array_equal(full[rows[:-1]], want)


def test_list_budget_bands(pkg, rt, oracle):
    """Frames whose coarse candidate lists would pass the workspace budget
    render as internal bands of whole coarse rows (band renders with their
    own bin masks), one after another on the stream: bit-identical to the unsplit
    frame, for full frames, row ranges and both formats."""
    w, h = 1000, 777
    scene = pkg.Scene.synthetic(w, h, 500, 40, seed=31, k=1.2)
    full, t = rt.render(scene, w, h)
    assert t.path == "binned"
    full8, _ = rt.render(scene, w, h, fmt="rgba8")
    n_prims = 12 * 40 + 500
    row_bytes = 8 * ((n_prims + 7) // 8 * 8 + 8) * ((w + 63) // 64)
    for budget in (1, 2 * row_bytes, 5 * row_bytes + 1):
        with knobs(rt, list_budget=budget):
            got, t = rt.render(scene, w, h)
            assert t.path == "binned"
            assert np.array_equal(got, full), budget
            got, _ = rt.render(scene, w, h, rows=(50, 700))
            assert np.array_equal(got, full[50:700]), budget
            got, _ = rt.render(scene, w, h, fmt="rgba8")
            assert np.array_equal(got, full8), budget
    # profiling counts the banded frame as one render, its bands summed
    with knobs(rt, list_budget=2 * row_bytes):
        rt.profile(True)
        try:
            rt.render(scene, w, h)
            prof = rt.profile_read()
        finally:
            rt.profile(False)
        assert prof["renders"] == 1 and prof["trace_ms"] > 0, prof
    want = oracle.trace(scene, w, h, threads=THREADS)
    assert not diff_report(full, want), diff_report(full, want)


def test_profile_slots_of_skipped_kernels(pkg, rt):
    """Per-kernel profiling: a kernel that does not run reads 0 ms (scenes of
    at most 128 primitives run one kernel, frame_small_kernel, in the trace
    slot; with it off, prep + trace_small_kernel skip the coarse kernel;
    empty scenes skip prep and coarse, the generic path both), the kernels
    that run read > 0."""
    small = pkg.Scene.synthetic(640, 480, 8, 2, seed=2, k=1.0)
    big = pkg.Scene.synthetic(640, 480, 500, 10, seed=2, k=1.0)
    cases = [(small, "binned", (False, False, True), True),
             (small, "binned", (True, False, True), False),
             (big, "binned", (True, True, True), True),
             (pkg.Scene(), "binned", (False, False, True), True),
             (small, "generic", (False, False, True), True)]
    for scene, path, ran, fused in cases:
        with knobs(rt, small_fused=2 if fused else 0):
            rt.profile(True)
            try:
                rt.render(scene, 640, 480, path=path)
                rt.render(scene, 640, 480, path=path)
                prof = rt.profile_read()
            finally:
                rt.profile(False)
        assert prof["renders"] == 2, prof
        for key, on in zip(("prep_ms", "bin_ms", "trace_ms"), ran):
            assert (prof[key] > 0) == on, (path, key, prof)


@pytest.mark.parametrize("n_ctx", [1, 2, 3, 5])
def test_render_multi_bands(pkg, rt, oracle, n_ctx):
    """rt_render_multi: the frame split over n contexts (all on the one GPU
    here, one host thread each) equals the single-context frame, for whole
    frames, odd row ranges, both formats and more contexts than rows."""
    scene = pkg.Scene.synthetic(700, 301, 300, 40, seed=n_ctx, k=1.5)
    tracers = [rt] + [pkg.RayTracer(0) for _ in range(n_ctx - 1)]
    try:
        full, _ = rt.render(scene, 700, 301)
        got, times = pkg.render_multi(tracers, scene, 700, 301)
        assert np.array_equal(got, full)
        assert len(times) == n_ctx and all(t.path == "binned" for t in times)
        got, _ = pkg.render_multi(tracers, scene, 700, 301, rows=(33, 290))
        assert np.array_equal(got, full[33:290])
        tex, _ = pkg.render_multi(tracers, scene, 700, 301, fmt="rgba8")
        assert np.array_equal(tex, pkg.pack_rgba8(full))
        got, times = pkg.render_multi(tracers, scene, 700, 301, rows=(100, 102))
        assert np.array_equal(got, full[100:102])
        assert sum(t.path == "idle" for t in times) == max(0, n_ctx - 2)
    finally:
        for t in tracers[1:]:
            t.close()
    want = oracle.trace(scene, 700, 301, threads=THREADS)
    assert not diff_report(full, want), diff_report(full, want)


_COLD = r"""
import json, sys
import numpy as np
sys.path.insert(0, {repo!r})
import __graft_entry__
pkg = __graft_entry__.load_package()
with np.load({golden!r}, allow_pickle=False) as z:
    g = {{k: z[k] for k in z.files}}
scene = pkg.Scene(g["sphere_origins"], g["sphere_radius"], g["sphere_colours"],
                  g["cube_vertices"], g["cube_colours"])
out = np.zeros((480, 640, 4), np.int32)
rt = pkg.RayTracer(0)            # the process's first context
res = []
for _ in range(3):
    out.fill(0)
    _, t = rt.render(scene, 640, 480, out=out)
    res.append(dict(kernel_us=t.kernel_us, total_us=t.total_us,
                    ok=bool(np.array_equal(out, g["frame"]))))
res.append(rt.last_kernel())
rt.close()
print(json.dumps(res))
"""


def test_first_render_is_not_cold(tmp_path):
    """The one-time setup is rt_init's (openCLInit's place, MainState.cpp:
    1290-1320, outside the trace timer :662-894): in a fresh process, the
    first rt_render of reference scene 1 at 640x480 on the first context
    spends at most 20x a warm call's kernel time (at least 250 us, at most
    1 ms; code objects loaded in rt_init, workspace reserved before the timed
    events), and every frame is the golden frame."""
    import json
    import subprocess
    import sys

    repo = str(Path(__file__).resolve().parents[1])
    code = _COLD.format(repo=repo, golden=str(GOLDEN / "scene1_640x480.npz"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       timeout=110, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    *calls, kernel = json.loads(r.stdout.strip().splitlines()[-1])
    print("first / second / third kernel_us:", [round(c["kernel_us"], 1) for c in calls])
    assert all(c["ok"] for c in calls)
    assert kernel == "frame_small_kernel"
    # a bound that a cold code-object load or an allocation inside the kernel
    # span breaks (round 3 measured 2.7 ms for those; warm calls take ~10 us,
    # the first 12-13 us): 20x the warm calls, at least 250 us (a fresh box's
    # clock ramp), never above 1 ms
    warm = min(c["kernel_us"] for c in calls[1:])
    assert calls[0]["kernel_us"] < min(1000.0, max(250.0, 20.0 * warm)), calls


def test_fresh_context_first_render(pkg):
    """A further context in the same process: its first render is warm too
    (rt_reserve sizes the workspace; nothing is allocated in the render)."""
    g = load_golden("scene3_640x480")
    scene = golden_scene(pkg, g)
    with pkg.RayTracer(0) as fresh:
        fresh.reserve(640, 480, scene.num_spheres, scene.num_cubes)
        out = np.zeros((480, 640, 4), np.int32)
        _, t1 = fresh.render(scene, 640, 480, out=out)
        ok1 = np.array_equal(out, g["frame"])
        _, t2 = fresh.render(scene, 640, 480, out=out)
    assert ok1 and np.array_equal(out, g["frame"])
    # (see test_first_render_is_not_cold)
    assert t1.kernel_us < min(1000.0, max(250.0, 20.0 * t2.kernel_us)), (t1, t2)


def test_trace_bin_automatic_choice(pkg, oracle):
    """The automatic path choice (rt_debug_set_trace_bin 0): a fresh context's
    first int32x4 frame of <= 1024 primitives above 4096 wave tiles runs prep
    -> coarse -> trace; the coarse kernel reports the frame's box overdraw
    to the host, and while it stays below 4 frames the next int32x4 frames
    skip the coarse kernel (trace_bin_kernel); a scene of high overdraw sends
    the next frame back to the coarse path (round 6: the kernels write the
    verdict into the host's mapped word themselves, every binned launch;
    before, a copy every 8th launch let up to 8 frames pass).  RGBA8 frames skip
    the coarse kernel only below 1 frame (config 3's density, 2.8, keeps
    it; a sparse scene does not).  Every frame is the oracle's, bit for bit.

    Round 4's version of this path faulted the GPU on a fresh context's first
    render: the page-locked verdict word was freed inside the first render's
    staging reservation and the verdict copy then landed in the freed page.
    The first render of a fresh context under every knob value is checked
    first."""
    low = pkg.Scene.synthetic(2048, 2048, 256, 64, seed=3, k=3.2)      # overdraw ~3
    high = pkg.Scene.synthetic(2048, 2048, 256, 64, seed=3, k=12.8)    # overdraw > 6
    want_low = oracle.trace(low, 2048, 2048, threads=THREADS)
    want_high = oracle.trace(high, 2048, 2048, threads=THREADS)
    for mode, first in ((0, "trace3_kernel"), (1, "trace_bin_kernel"), (2, "trace3_kernel")):
        with pkg.RayTracer(0) as fresh, knobs(fresh, trace_bin=mode):
            f, _ = fresh.render(low, 2048, 2048)
            assert fresh.last_kernel() == first, mode
            assert np.array_equal(f, want_low), mode
            f, _ = fresh.render(low, 2048, 2048)
            assert fresh.last_kernel() == ("trace3_kernel" if mode == 2 else "trace_bin_kernel")
            assert np.array_equal(f, want_low), mode
    rt = pkg.RayTracer(0)
    try:
        f1, _ = rt.render(low, 2048, 2048)
        assert rt.last_kernel() == "trace3_kernel"
        assert np.array_equal(f1, want_low)
        f2, _ = rt.render(low, 2048, 2048)
        assert rt.last_kernel() == "trace_bin_kernel"
        assert np.array_equal(f2, want_low)
        g, _ = rt.render(low, 2048, 2048, fmt="rgba8")
        assert rt.last_kernel() == "trace3_kernel"
        assert np.array_equal(g, oracle.pack_rgba8(want_low))
        # from its second frame on the high-overdraw scene is back on the
        # coarse path, and every frame is the oracle's
        kernels = []
        for _ in range(10):
            h, _ = rt.render(high, 2048, 2048)
            kernels.append(rt.last_kernel())
            assert np.array_equal(h, want_high), kernels
        assert kernels[0] == "trace_bin_kernel", kernels
        assert kernels[-1] == "trace3_kernel", kernels
        assert kernels.index("trace3_kernel") == 1, kernels
        assert set(kernels[1:]) == {"trace3_kernel"}, kernels
        # and a low-overdraw scene comes back to the no-coarse path
        kernels = []
        for _ in range(10):
            f, _ = rt.render(low, 2048, 2048)
            kernels.append(rt.last_kernel())
            assert np.array_equal(f, want_low), kernels
        assert kernels[0] == "trace3_kernel" and set(kernels[1:]) == {"trace_bin_kernel"}, kernels
        assert 2.0 < rt.last_overdraw() < 4.0, rt.last_overdraw()
    finally:
        rt.close()
    # RGBA8 below 1 frame of overdraw: the Texture skips the coarse kernel too
    sparse = pkg.Scene.synthetic(2048, 2048, 256, 64, seed=5, k=0.8)
    want_sparse = oracle.pack_rgba8(oracle.trace(sparse, 2048, 2048, threads=THREADS))
    with pkg.RayTracer(0) as fresh:
        g1, _ = fresh.render(sparse, 2048, 2048, fmt="rgba8")
        assert fresh.last_kernel() == "trace3_kernel"
        assert fresh.last_overdraw() < 1.0
        g2, _ = fresh.render(sparse, 2048, 2048, fmt="rgba8")
        assert fresh.last_kernel() == "trace_bin_kernel"
        assert np.array_equal(g1, want_sparse) and np.array_equal(g2, want_sparse)


def test_verdict_copy_fallback(pkg, oracle):
    """rt_debug_set_verdict_copy: the library's fallback where the device
    cannot map the page-locked verdict word (the kernels store the verdict in
    device memory, a 4-byte copy every 8th binned launch brings it over) still
    picks the paths, later: a jump to high overdraw leaves trace_bin_kernel
    within 8 frames; switched back to the kernels' own stores, the path
    follows from the next frame.  Every frame is the oracle's."""
    low = pkg.Scene.synthetic(2048, 2048, 256, 64, seed=3, k=3.2)
    high = pkg.Scene.synthetic(2048, 2048, 256, 64, seed=3, k=12.8)
    want_low = oracle.trace(low, 2048, 2048, threads=THREADS)
    want_high = oracle.trace(high, 2048, 2048, threads=THREADS)
    with pkg.RayTracer(0) as rt:
        rt.set_verdict_copy(True)
        kernels = []
        for scene, want, n in ((low, want_low, 2), (high, want_high, 10)):
            for _ in range(n):
                f, _ = rt.render(scene, 2048, 2048)
                kernels.append(rt.last_kernel())
                assert np.array_equal(f, want), kernels
        assert kernels[:3] == ["trace3_kernel", "trace_bin_kernel", "trace_bin_kernel"], kernels
        assert 3 < kernels.index("trace3_kernel", 2) <= 10, kernels
        assert kernels[-1] == "trace3_kernel", kernels
        rt.set_verdict_copy(False)
        kernels = []
        for _ in range(4):
            f, _ = rt.render(low, 2048, 2048)
            kernels.append(rt.last_kernel())
            assert np.array_equal(f, want_low), kernels
        assert kernels == ["trace3_kernel"] + ["trace_bin_kernel"] * 3, kernels
    lib = pkg.library()
    assert lib.rt_debug_set_verdict_copy(None, 0) == -1  # RT_ERR_INVALID_ARG


def test_last_kernel_names_the_path_taken(pkg, rt, oracle):
    """rt_last_kernel reports the kernel that actually ran (the bench's
    `kernel` label): frame_small_kernel for <= 128 primitives on a resident
    grid, trace_small_kernel for <= 512, trace3_kernel beyond (on frames of
    at most 4096 wave tiles trace3_split_kernel), generic_kernel for the
    brute-force path."""
    cases = [(pkg.Scene.synthetic(1920, 1080, 16, 4, seed=2, k=3.0), 1920, 1080, "auto",
              "frame_small_kernel"),
             (pkg.Scene.synthetic(4096, 1024, 100, 30, seed=5, k=6.4), 4096, 1024, "auto",
              "trace_small_kernel"),
             (pkg.Scene.synthetic(1024, 1024, 256, 64, seed=3, k=1.6), 1024, 1024, "auto",
              "trace3_split_kernel"),
             (pkg.Scene.synthetic(2048, 2048, 256, 64, seed=3, k=3.2), 2048, 2048, "auto",
              "trace3_kernel"),
             (pkg.Scene.synthetic(2048, 2048, 256, 64, seed=3, k=3.2), 2048, 2048, "bin",
              "trace_bin_kernel"),
             (pkg.Scene.synthetic(256, 128, 8, 2, seed=1, k=0.4), 256, 128, "generic",
              "generic_kernel")]
    for scene, w, h, path, want in cases:
        # (binned frames of <= 1024 primitives: trace_bin_kernel forced on for
        # "bin", off otherwise; its automatic choice is tested below)
        with knobs(rt, trace_bin=1 if path == "bin" else 2):
            frame, _ = rt.render(scene, w, h, path="auto" if path == "bin" else path)
        assert rt.last_kernel() == want, (w, h, scene.num_spheres, scene.num_cubes)
        if w * h <= 256 * 128:
            assert np.array_equal(frame, oracle.trace(scene, w, h))
