"""GPU parity at BASELINE's full-size multi-GPU configs, the explicit-origin
band upload, and the N>1 bench assemblies (rehearsed on one GPU).

Config 4 (8192^2, 192 spheres + 64 cubes, seed 4, dense) and config 5
(16384^2, 4096 spheres, seed 5, dense k = 25.6: about 11 spheres over each
pixel, the depth-cull-heavy regime) are rendered WHOLE on the device; a
deterministic row sample is compared bit-exactly with the oracle, and the
frame is compared with the 8 row bands the 8-rank layout renders
(rowbands.band_rows), so the assembled frame of an 8-GPU run is the one-GPU
frame."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gpu_support import (FORCED_CULLS, THREADS, cube_tie_scene, device_scene, knobs, oracle_frame,
                         tie_scene)

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]


def _full_frame_vs_oracle(pkg, rt, oracle, w, h, ns, nc, seed, rows, bands):
    torch = pytest.importorskip("torch")
    from opencl_ray_tracer_amd.rowbands import band_rows

    dev = torch.device("cuda:0")
    scene = pkg.Scene.synthetic(w, h, ns, nc, seed=seed, k=w / 640)
    ds, keep = device_scene(torch, scene)
    stream = torch.cuda.current_stream().cuda_stream
    frame = torch.empty((h, w, 4), dtype=torch.int32, device=dev)
    rt.render_device(ds, w, h, (0, h), frame.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    got = frame[torch.tensor(rows, device=dev)].cpu().numpy()
    want = oracle.trace_rows(scene, w, h, rows, threads=THREADS)
    for i, r in enumerate(rows):
        bad = int((got[i] != want[i]).any(-1).sum())
        assert bad == 0, f"row {r}: {bad} pixels differ"
    # the row bands of an n-rank run, each a band render, assemble to the frame
    band = torch.empty_like(frame[: (h + bands - 1) // bands])
    for r in range(bands):
        rb, re = band_rows(h, bands, r)
        rt.render_device(ds, w, h, (rb, re), band.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(band[: re - rb], frame[rb:re]), f"band {r} ({rb}..{re})"
    del frame, band, keep


def test_config4_full_frame(pkg, rt, oracle):
    """BASELINE config 4 at full size: 8192^2, 192 spheres + 64 cubes."""
    h = 8192
    rows = sorted({0, 1, 63, 64, 1023, 1024, h - 1} | set(range(17, h, 331)))
    _full_frame_vs_oracle(pkg, rt, oracle, 8192, h, 192, 64, 4, rows, bands=8)


def test_config5_full_frame(pkg, rt, oracle):
    """BASELINE config 5 at full size and density: 16384^2, 4096 spheres,
    k = 25.6 (about 11 spheres over each pixel: the depth-culled walk)."""
    h = 16384
    rows = sorted({0, 2047, 2048, 8192, h - 1} | set(range(331, h, 16384 // 20)))
    _full_frame_vs_oracle(pkg, rt, oracle, 16384, h, 4096, 0, 5, rows, bands=8)


@pytest.mark.parametrize("config", ["config4", "config5"])
def test_full_size_rgba8_is_packed_i32x4(pkg, rt, config):
    """The Texture (RGBA8) frame at BASELINE's full sizes equals the byte
    pack of the int32x4 frame (MainState.cpp:1026-1036: each channel's low
    byte, alpha 0xFF) at every pixel -- a size-independent property that
    carries the int32x4 oracle parity of the config 4 / 5 tests above to the
    second output format."""
    torch = pytest.importorskip("torch")
    w, ns, nc, seed = (8192, 192, 64, 4) if config == "config4" else (16384, 4096, 0, 5)
    h = w
    dev = torch.device("cuda:0")
    scene = pkg.Scene.synthetic(w, h, ns, nc, seed=seed, k=w / 640)
    ds, keep = device_scene(torch, scene)
    stream = torch.cuda.current_stream().cuda_stream
    full = torch.empty((h, w, 4), dtype=torch.int32, device=dev)
    tex = torch.empty((h, w), dtype=torch.int32, device=dev)
    rt.render_device(ds, w, h, (0, h), full.data_ptr(), stream=stream)
    rt.render_device(ds, w, h, (0, h), tex.data_ptr(), fmt="rgba8", stream=stream)
    torch.cuda.synchronize()
    alpha = torch.tensor(-16777216, dtype=torch.int32, device=dev)  # 0xFF000000
    for r0 in range(0, h, 1024):
        f = full[r0:r0 + 1024]
        packed = ((f[..., 0] & 255) | ((f[..., 1] & 255) << 8) | ((f[..., 2] & 255) << 16)
                  | alpha)
        bad = int((packed != tex[r0:r0 + 1024]).sum())
        assert bad == 0, f"rows {r0}..{r0 + 1024}: {bad} pixels differ"
    del full, tex, keep


def test_render_multi_explicit_origins_band_upload(pkg, rt, oracle):
    """rt_render_multi with explicit origins: each band uploads only its own
    rows of the origin array (MainState.cpp:841-855 uploads them all) and
    the frame equals the single-context one and the oracle."""
    rng = np.random.default_rng(11)
    w, h = 160, 97
    scene = pkg.Scene.synthetic(w, h, 20, 8, seed=11, k=0.4)
    d = np.array([0.1, -0.2, -1.0, -1.0], np.float32)
    org = np.zeros((h, w, 4), np.float32)
    org[..., 0] = np.arange(w)[None, :] + rng.uniform(-0.5, 0.5, (h, w))
    org[..., 1] = np.arange(h)[:, None] + rng.uniform(-0.5, 0.5, (h, w))
    org[..., 2] = rng.uniform(-3, 3, (h, w))
    org[..., 3] = 1.0
    full, t = rt.render(scene, w, h, ray_dir=d, ray_origins=org)
    assert t.path == "generic"
    assert np.array_equal(full, oracle.trace(scene, w, h, ray_dir=d, ray_origins=org))
    band, _ = rt.render(scene, w, h, rows=(40, 61), ray_dir=d, ray_origins=org)
    assert np.array_equal(band, full[40:61])
    tracers = [rt] + [pkg.RayTracer(0) for _ in range(2)]
    try:
        got, times = pkg.render_multi(tracers, scene, w, h, ray_dir=d, ray_origins=org)
        assert all(tt.path == "generic" for tt in times)
        assert np.array_equal(got, full)
        with pytest.raises(ValueError):
            pkg.render_multi(tracers, scene, w, h, ray_dir=d, ray_origins=org[:-1])
    finally:
        for tr in tracers[1:]:
            tr.close()


def test_device_origins_band(pkg, rt, oracle):
    """rt_render_device with full-frame device origins and a row band reads
    the band's own rows of them."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    w, h = 128, 90
    scene = pkg.Scene.synthetic(w, h, 16, 6, seed=12, k=0.5)
    ys, xs = np.mgrid[0:h, 0:w]
    org = np.stack([xs + 0.25, ys - 0.25, np.zeros_like(xs), np.ones_like(xs)],
                   -1).astype(np.float32)
    ds, keep = device_scene(torch, scene)
    dorg = torch.from_numpy(org).to(dev)
    out = torch.empty((30, w, 4), dtype=torch.int32, device=dev)
    rt.render_device(ds, w, h, (50, 80), out.data_ptr(), origins_ptr=dorg.data_ptr(),
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = oracle.trace(scene, w, h, rows=(50, 80), ray_origins=org)
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("world", [2])
def test_bench_rehearsal_assemblies(world, tmp_path):
    """bench.py at N>1 (rehearsal: every rank on cuda:0, gloo): both frame
    assemblies -- RCCL-style point-to-point into rank 0's frame, and the
    peer-store path through an IPC-mapped rank-0 frame (rt_shared_open) --
    produce a frame bit-identical to a one-GPU render, and the line carries
    the strong-scaling fields."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={world}", "--master-addr=127.0.0.1", "--master-port=29533",
           str(REPO / "bench.py"), "--gpus", str(world), "--rehearse", "--full", "--steps", "3",
           "--warmup", "1", "--width", "1024", "--height", "512"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([s for s in p.stdout.splitlines() if s.startswith("{")][-1])
    assert line["n_gpus"] == world and line["scaling"] == "strong"
    for how in ("rccl_p2p", "xgmi_peer_store"):
        assert line["assembly"][how]["frame_check"] == "bit-exact", line["assembly"]
        assert line["texture_rgba8"][how]["frame_check"] == "bit-exact"
        assert line["config4"][how]["frame_check"] == "bit-exact"
    # the app's host frame in both formats (`pixels`, the Texture), N ranks
    # and one GPU in the same run, with the ratio
    for fmt in ("i32x4", "rgba8"):
        hf = line["host_frame"][fmt]
        assert hf["frame_check"] == "bit-exact" and hf["format"] == fmt, hf
        assert hf["scaling"] == pytest.approx(hf["one_gpu"]["ms_per_step"] / hf["ms_per_step"],
                                              rel=2e-2)
    bal = line["assembly"]["xgmi_peer_store_balanced"]
    assert bal["frame_check"] == "bit-exact" and sum(bal["rows_per_rank"]) == 512, bal
    assert line["value"] == pytest.approx(1024 * 512 / (line["ms_per_step"] * 1e-3) / 1e6,
                                          rel=2e-3)
    # the CPU path beside the GPU numbers at N > 1 too (rank 0)
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] >= 1
    assert "phase_errors" not in line, line.get("phase_errors")
    # the scaling contract: against rank 0 alone in the
    # same run; no committed fixture holds this 1024 x 512 scene
    t1 = line["one_gpu"]["ms_per_step"]
    assert line["scaling_assembled"] == pytest.approx(t1 / line["ms_per_step"], rel=1e-3,
                                                      abs=1e-4)
    assert line["scaling_weak"] == pytest.approx(
        world * t1 / line["weak_scaling"]["ms_per_step"], rel=1e-3, abs=1e-4)
    assert "scaling_host_frame" in line["scaling_note"]
    assert line["frame_check_ref"] is None


def _no_launcher_env():
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    return env


def test_bench_rehearsal_without_launcher(tmp_path):
    """`python bench.py --gpus 2` with no torchrun (missing #1):
    bench.py starts its two ranks itself (both on cuda:0 in this rehearsal,
    gloo), exactly one line comes out with n_gpus 2, bit-exact assemblies and
    the scaling keys, and the status is 0."""
    cmd = [sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--rehearse", "--full",
           "--steps", "3", "--warmup", "1", "--width", "1024", "--height", "512", "--no-extras",
           "--no-cpu-baseline"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=_no_launcher_env(),
                       cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [s for s in p.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["value"] > 0
    for how in ("rccl_p2p", "xgmi_peer_store"):
        assert line["assembly"][how]["frame_check"] == "bit-exact", line["assembly"]
    assert line["scaling_assembled"] == pytest.approx(
        line["one_gpu"]["ms_per_step"] / line["ms_per_step"], rel=1e-3, abs=1e-4)
    assert "scaling_weak" in line and "scaling_note" in line


def test_bench_rehearsal_without_launcher_hang(tmp_path):
    """The same with one rank hanging in an assembly: status 3 from the
    parent, one line naming the phase."""
    cmd = [sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--rehearse", "--steps", "3",
           "--warmup", "1", "--width", "1024", "--height", "512", "--no-extras",
           "--no-cpu-baseline", "--pg-timeout", "300", "--phase-deadline", "20",
           "--fail-assembly", "xgmi_peer_store:1:hang"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=_no_launcher_env(),
                       cwd=tmp_path)
    assert p.returncode == 3, (p.returncode, p.stderr[-3000:])
    lines = [s for s in p.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    assert "timeout" in json.loads(lines[0])["assembly"]["xgmi_peer_store"]["error"]


def test_bench_rehearsal_forced_failure(tmp_path):
    """bench.py at N>1 with one assembly forced to raise on rank 1 only
    (rank 0 then waits in that assembly's collectives until the process
    group's timeout): the failure is recorded as {"error": ...} on every rank,
    the other assemblies still run, and rank 0 prints one line whose value
    comes from a bit-exact assembly."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node=2", "--master-addr=127.0.0.1", "--master-port=29534",
           str(REPO / "bench.py"), "--gpus", "2", "--rehearse", "--steps", "3",
           "--warmup", "1", "--width", "1024", "--height", "512", "--no-extras",
           "--no-cpu-baseline", "--pg-timeout", "15", "--fail-assembly", "rccl_p2p:1"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=tmp_path)
    assert p.returncode == 0, p.stderr[-3000:]  # a caught exception: every phase completed
    lines = [s for s in p.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert "error" in line["assembly"]["rccl_p2p"], line["assembly"]
    assert line["assembly"]["xgmi_peer_store"]["frame_check"] == "bit-exact"
    assert "assembly.rccl_p2p" in line["phase_errors"]
    assert line["value"] and line["config"]["parallelism"].endswith(
        ("xgmi_peer_store (rehearsal: shared cuda:0, gloo)",
         "xgmi_peer_store_balanced (rehearsal: shared cuda:0, gloo)"))


def test_bench_rehearsal_forced_hang(tmp_path):
    """bench.py at N>1 with one rank hanging inside an assembly (past the
    phase deadline, the data-path timeout longer): rank 0's watchdog prints
    exactly one line, the hung phase named in phase_errors, and the launcher
    gets a non-zero status -- a hang is never reported as success."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node=2", "--master-addr=127.0.0.1", "--master-port=29535",
           str(REPO / "bench.py"), "--gpus", "2", "--rehearse", "--steps", "3",
           "--warmup", "1", "--width", "1024", "--height", "512", "--no-extras",
           "--no-cpu-baseline", "--pg-timeout", "300", "--phase-deadline", "20",
           "--fail-assembly", "xgmi_peer_store:1:hang"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=env, cwd=tmp_path)
    assert p.returncode != 0, p.stderr[-3000:]
    lines = [s for s in p.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert "timeout" in line["assembly"]["xgmi_peer_store"]["error"]
    assert line["phase_errors"] == ["assembly.xgmi_peer_store"]
    assert line["assembly"]["rccl_p2p"]["frame_check"] == "bit-exact"  # the phase before


@pytest.mark.parametrize("case", ["dense", "dense_rgba8", "ties", "cubes_and_spheres",
                                  "dense_cubes", "cube_ties", "heavy_defaults"])
def test_coarse_depth_cull_exact(pkg, rt, oracle, case):
    """The coarse kernel's depth cull (per-tile cover bounds) drops only
    candidates that cannot win a pixel: frames with it on and off are
    identical and equal the oracle, in the dense regime where it drops most
    and with exact ties.  "heavy_defaults": a scene of 16x config 3's object
    density, whose box overdraw (about 40) passes the library's default
    triangle gate, rendered with the defaults."""
    fmt = "rgba8" if case.endswith("rgba8") else "i32x4"
    w, h = 640, 480
    if case == "ties":
        scene = tie_scene(pkg, w, h, 400, 3)
    elif case == "cubes_and_spheres":
        scene = pkg.Scene.synthetic(w, h, 300, 40, seed=9, k=w / 640 * 4)
    elif case == "dense_cubes":  # triangles cover and drop each other
        scene = pkg.Scene.synthetic(w, h, 60, 200, seed=10, k=w / 640 * 3)
    elif case == "cube_ties":
        scene = cube_tie_scene(pkg, w, h, 12)
    elif case == "heavy_defaults":  # config 3's scene generator at 16x the objects
        scene = pkg.Scene.synthetic(w, h, 4096, 1024, seed=3, k=6.4 * w / 4096)
    else:
        scene = pkg.Scene.synthetic(w, h, 1200, 0, seed=5, k=w / 640 * 4)
    with knobs(rt, coarse_cull=0, coarse_cull_tri=0):
        off, _ = rt.render(scene, w, h, fmt=fmt)
    with knobs(rt, **({} if case == "heavy_defaults" else FORCED_CULLS)):
        on, t = rt.render(scene, w, h, fmt=fmt)
    assert t.path == "binned"
    assert np.array_equal(on, off)
    assert np.array_equal(on, oracle_frame(oracle, scene, w, h, fmt=fmt, threads=THREADS))


@pytest.mark.parametrize("case", ["ties", "cube_ties", "dense_cubes", "dense_rgba8",
                                  "band", "wide"])
def test_trace_split_exact(pkg, rt, oracle, case):
    """trace3_split_kernel (2 or 4 waves per wave tile, each testing every
    2nd / 4th candidate the tile keeps, merged by smallest t then smallest
    slot) gives trace3_kernel's frame and the oracle's, with exact ties of
    spheres and of cubes (the first in primitive order must win,
    MainState.cpp:386-391), in both formats, on a row band and in the wide
    tile build."""
    fmt = "rgba8" if case.endswith("rgba8") else "i32x4"
    w, h, rows = 640, 480, (0, 480)
    if case == "ties":
        scene = tie_scene(pkg, w, h, 400, 4)
    elif case == "cube_ties":
        scene = cube_tie_scene(pkg, w, h, 13)
    elif case == "band":
        scene, rows = cube_tie_scene(pkg, w, h, 14), (77, 401)
    else:
        scene = pkg.Scene.synthetic(w, h, 120, 200, seed=11, k=w / 640 * 3)
    with pytest.raises(pkg.RtError):
        rt.set_trace_split(8)  # (at most 4 waves per tile: the merge's LDS)
    frames = {}
    fixed = dict(small_path=False)  # (every case takes the binned trace)
    if case == "wide":
        fixed.update(tile_variant=2)
    for split in (1, 2, 4):
        with knobs(rt, trace_split=split, **fixed):
            frames[split], t = rt.render(scene, w, h, rows=rows, fmt=fmt)
            assert t.path == "binned"
            assert rt.last_kernel() == ("trace3_kernel" if split == 1 else "trace3_split_kernel")
    want = oracle_frame(oracle, scene, w, h, rows=rows, fmt=fmt, threads=THREADS)
    for split, got in frames.items():
        assert np.array_equal(got, want), split


@pytest.mark.parametrize("case", ["ties", "cube_ties", "dense_culled", "dense_rgba8",
                                  "band", "box_scan", "wide"])
def test_coarse_waves_exact(pkg, rt, oracle, case):
    """coarse3_kernel with 1 / 2 / 4 waves per bin (the waves share the
    staging loads and the (candidate, tile) pair loops; wave 0 writes the
    list) gives the same frame, equal to the oracle: sphere and cube ties,
    the depth culls forced on in every bin (spheres and triangles), RGBA8, a
    row band, the box-scan path and the wide tile build."""
    fmt = "rgba8" if case.endswith("rgba8") else "i32x4"
    w, h, rows = 640, 480, (0, 480)
    if case == "ties":
        scene = tie_scene(pkg, w, h, 400, 5)
    elif case == "cube_ties":
        scene = cube_tie_scene(pkg, w, h, 15)
    elif case == "band":
        scene, rows = cube_tie_scene(pkg, w, h, 16), (33, 350)
    else:
        scene = pkg.Scene.synthetic(w, h, 300, 120, seed=12, k=w / 640 * 4)
    frames = {}
    fixed = dict(small_path=False)
    if case in ("dense_culled", "dense_rgba8", "ties", "cube_ties"):
        fixed.update(FORCED_CULLS)
    if case == "box_scan":
        fixed.update(bin_masks=False)
    if case == "wide":
        fixed.update(tile_variant=2)
    for cw in (1, 2, 4, 8):
        with knobs(rt, coarse_waves=cw, **fixed):
            frames[cw], t = rt.render(scene, w, h, rows=rows, fmt=fmt)
            assert t.path == "binned"
    want = oracle_frame(oracle, scene, w, h, rows=rows, fmt=fmt, threads=THREADS)
    for cw, got in frames.items():
        assert np.array_equal(got, want), cw


@pytest.mark.parametrize("case", ["ties", "cube_ties", "dense", "dense_rgba8", "band",
                                  "wide", "nonfinite"])
def test_trace_bin_exact(pkg, rt, oracle, case):
    """trace_bin_kernel (no coarse kernel: each wave tile packs its bin's
    candidates from the mask words, classifies them against itself and walks
    the kept ones in order) gives the oracle's frame: sphere and cube ties,
    RGBA8, a row band, the wide tile build, non-finite scene data (the
    reference verbatim)."""
    fmt = "rgba8" if case.endswith("rgba8") else "i32x4"
    w, h, rows = 640, 480, (0, 480)
    if case == "ties":
        scene = tie_scene(pkg, w, h, 400, 6)
    elif case in ("cube_ties", "band"):
        scene = cube_tie_scene(pkg, w, h, 17, spheres=30, cubes=60, duplicates=20)
        if case == "band":
            rows = (61, 377)
    else:
        scene = pkg.Scene.synthetic(w, h, 600, 30, seed=18, k=w / 640 * 4)
        if case == "nonfinite":
            so = np.array(scene.sphere_origins)
            so[7, 0] = np.nan
            scene = pkg.Scene(so, scene.sphere_radius, scene.sphere_colours,
                              scene.cube_vertices, scene.cube_colours)
    with knobs(rt, small_path=False, trace_bin=1, tile_variant=2 if case == "wide" else 0):
        got, t = rt.render(scene, w, h, rows=rows, fmt=fmt)
        assert t.path == "binned"
        assert rt.last_kernel() == "trace_bin_kernel"
    assert np.array_equal(got, oracle_frame(oracle, scene, w, h, rows=rows, fmt=fmt,
                                            threads=THREADS))


def test_render_into_registered_host_frame(pkg, rt):
    """rt_host_register: rt_render's download into a page-locked host frame
    (the app's `pixels` vector) gives the same frame, for bands too."""
    g_scene = pkg.Scene.synthetic(333, 200, 40, 10, seed=21, k=1.2)
    want, _ = rt.render(g_scene, 333, 200)
    buf = np.zeros((200, 333, 4), np.int32)
    pkg.host_register(buf)
    try:
        rt.render(g_scene, 333, 200, rows=(0, 77), out=buf[:77])
        rt.render(g_scene, 333, 200, rows=(77, 200), out=buf[77:])
    finally:
        pkg.host_unregister(buf)
    assert np.array_equal(buf, want)


@pytest.mark.parametrize("case", ["golden", "dense", "rgba8", "bands", "culled", "edges"])
def test_wide_tile_build_exact(pkg, rt, oracle, case):
    """The wide-tile (128x2) build (auto-selected for frames of >= 512 MiB) forced on
    small frames: bit-exact against the oracle / golden frames and against
    the 16x16 build, on awkward sizes, bands, both formats and the coarse
    depth cull."""
    from conftest import golden_scene, load_golden

    if case == "golden":
        with knobs(rt, tile_variant=2):
            for name in ("scene1_640x480", "scene3_640x480", "config2_1920x1080"):
                g = load_golden(name)
                got, t = rt.render(golden_scene(pkg, g), int(g["width"]), int(g["height"]))
                assert np.array_equal(got, g["frame"]), name
        return
    w, h = (333, 257) if case != "edges" else (130, 67)
    if case == "culled":
        scene = pkg.Scene.synthetic(640, 480, 1200, 0, seed=5, k=4.0)
        w, h = 640, 480
    elif case == "edges":
        scene = pkg.Scene.synthetic(w, h, 30, 12, seed=8, k=0.4)
    else:
        scene = pkg.Scene.synthetic(w, h, 60, 16, seed=104, k=w / 640 * 2)
    fmt = "rgba8" if case == "rgba8" else "i32x4"
    rows = (37, 201) if case == "bands" else (0, h)
    with knobs(rt, tile_variant=2):
        wide, t = rt.render(scene, w, h, rows=rows, fmt=fmt)
        assert t.path == "binned"
    with knobs(rt, tile_variant=1):
        narrow, _ = rt.render(scene, w, h, rows=rows, fmt=fmt)
    assert np.array_equal(wide, narrow)
    assert np.array_equal(wide, oracle_frame(oracle, scene, w, h, rows=rows, fmt=fmt,
                                             threads=THREADS))


# RT_SWEEP_SEEDS widens the sweep for one-off runs (profiles/r02/parity_sweep_4096.log)
@pytest.mark.parametrize("seed", list(range(int(os.environ.get("RT_SWEEP_SEEDS", "64")))))
def test_randomized_parity_sweep(pkg, rt, oracle, seed):
    """Seeded random frames against the oracle: frame sizes from 96 to 1500
    px a side, 1 to 600 spheres and 0 to 80 cubes at random densities, row
    bands, both formats, both tile builds, the depth culls forced on or left
    at their gates, the one-kernel small-scene path on / off / forced, bin
    masks or box scans, and 1 / 2 / 4 waves per wave tile in the trace and
    per coarse bin (or the frame-size choices).  Each
    knob is drawn independently from the seed's generator, so no two are
    tied to each other across the sweep."""
    rng = np.random.default_rng(1000 + seed)
    w = int(rng.integers(96, 1500))
    h = int(rng.integers(96, 1100))
    few = rng.random() < 0.25
    ns = int(rng.integers(1, 40)) if few else int(rng.integers(1, 600))
    nc = int(rng.integers(0, 6)) if few else int(rng.integers(0, 80))
    k = float(rng.uniform(0.3, 6.0)) * w / 640
    scene = pkg.Scene.synthetic(w, h, ns, nc, seed=seed, k=k)
    band = rng.random() < 0.35
    rows = ((int(rng.integers(0, h // 2)), int(rng.integers(h // 2 + 1, h + 1))) if band
            else (0, h))
    fmt = "rgba8" if rng.random() < 0.25 else "i32x4"
    tile = int(rng.integers(1, 3))
    small_fused = int(rng.integers(0, 3))
    cull_all = bool(rng.integers(0, 2))
    bin_masks = bool(rng.random() < 0.75)
    split = int(rng.choice([0, 1, 2, 4]))  # waves per wave tile in the binned trace
    coarse_waves = int(rng.choice([0, 1, 2, 4, 8]))  # waves per coarse bin
    trace_bin = int(rng.choice([0, 1, 2]))  # no coarse kernel: auto / always / never
    drawn = dict(trace_split=split, coarse_waves=coarse_waves, trace_bin=trace_bin,
                 tile_variant=tile, small_fused=small_fused, bin_masks=bin_masks,
                 **(FORCED_CULLS if cull_all else {}))
    with knobs(rt, **drawn):
        got, t = rt.render(scene, w, h, rows=rows, fmt=fmt)
    assert t.path == "binned"
    want = oracle_frame(oracle, scene, w, h, rows=rows, fmt=fmt, threads=THREADS)
    assert np.array_equal(got, want), (seed, w, h, ns, nc, k, rows, fmt, drawn)


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("rt_bench", REPO / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("case", ["whole", "sampled", "one_stream", "full"])
def test_bench_plain_run_and_dump_outputs(pkg, oracle, tmp_path, case):
    """A plain N=1 run (in this process: parse -> plain_run -> run_single)
    times --steps frames and measures nothing beside the headline: the line
    has the result keys and none of the --full ones.  --dump-outputs writes
    the last timed step's frame as float64: the whole frame when it has at
    most 2^20 pixels ("whole": 333x257), else the pixels at the fixed seeded
    positions ("sampled": 1200x900), equal to the oracle's frame either way;
    "one_stream": the one-stream loop as `value`'s loop (--inflight 1).
    "full": the same command with --full carries the other measurements and
    dumps the same frame."""
    torch = pytest.importorskip("torch")
    b = _bench_module()
    w, h = (1200, 900) if case == "sampled" else (333, 257)
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--warmup-ms", "1",
            "--width", str(w), "--height", str(h), "--spheres", "40", "--cubes", "10",
            "--seed", "31", "--dump-outputs", str(tmp_path / "out")]
    if case == "one_stream":
        argv += ["--inflight", "1"]
    if case == "full":
        argv += ["--full", "--cpu-threads", "2", "--app-calls", "2", "--sustained", "8"]
    args = b.plain_run(b.parse(argv))
    before = torch.cuda.current_stream()
    try:
        line = b.run_single(args, b.Ctx(args), pkg)
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(before)
    line = json.loads(json.dumps(line))
    assert line["steps"] == 3 and line["n_gpus"] == 1 and line["unit"] == "Mrays/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(w * h / (line["ms_per_step"] * 1e-3) / 1e6, rel=2e-2)
    loops = [line["one_stream"]["ms_per_step"]]
    if case != "one_stream":
        assert line["frames_in_flight"]["frame_check"] == "bit-exact"
        loops.append(line["frames_in_flight"]["ms_per_step"])
    else:
        assert line["frames_in_flight"] is None and line["dump_outputs"]["frame"] == "one_stream"
    assert line["ms_per_step"] == pytest.approx(min(loops), abs=1e-4)
    full_keys = {"roofline", "host_path", "cpu_baseline", "texture_rgba8", "frame_check_ref",
                 "profiled_pass_ms_per_step"}
    if case == "full":
        assert line["full"] is True and full_keys <= set(line)
        assert line["roofline"]["kernel_ms"] > 0 and line["cpu_baseline"]["value"] > 0
        assert line["frames_in_flight"]["sustained"]["steps"] == 8
        assert line["texture_rgba8"]["frames_in_flight"]["frame_check"] == "bit-exact"
    else:
        assert line["full"] is False and not (full_keys & set(line))
        assert "sustained" not in (line["frames_in_flight"] or {})
    files = sorted(p.name for p in (tmp_path / "out").iterdir())
    assert files == ["frame.npy"]
    got = np.load(tmp_path / "out" / "frame.npy")
    assert got.dtype == np.float64 and got.nbytes <= 64 << 20
    scene = pkg.Scene.synthetic(w, h, 40, 10, seed=31, k=w / 640.0)
    want = oracle.trace(scene, w, h, threads=THREADS).astype(np.float64)
    if case == "sampled":
        pos = np.sort(np.random.default_rng(b.DUMP_SEED).choice(w * h, b.DUMP_PIXELS,
                                                                replace=False))
        want = want.reshape(w * h, 4)[pos]
    assert got.shape == want.shape and np.array_equal(got, want)
