"""The culled ray queries beside their unculled twins, in one process: HIP-event
time per launch of each pair

  cast_camera_ref      rt_cast_camera[_accel]_device, the reference camera
  cast_camera_pinhole  the same with a pinhole camera in front of the frame
  cast_rays            rt_cast_rays[_accel]_device on the reference camera's rays
                       from a buffer (32 bytes per ray)
  cast_rays_permuted   the same buffer with its rays randomly permuted: a wave's
                       64 rays then go 64 different ways, and the wave-level
                       skip of a cube needs all of them to drop it
  occlude_rays         rt_occlude_rays[_accel]_device on one light's segments:
                       the facing hit pixels' (p, light - p, own object),
                       compacted in pixel order

and of rt_accel_build_device alone, interleaved round by round after warm-up.
Prints one JSON line.

    python scripts/accel_bench.py                    # config 3

Before anything is timed every culled output is compared with its unculled twin
word for word, and the records with the host's.  The kept-count histogram is
rt_accel_kept on a sample of each case's rays.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
LIGHT = (0.5, 0.5, 200.0)  # x, y in frame sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--spheres", type=int, default=256)
    ap.add_argument("--cubes", type=int, default=64)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--k", type=float, default=None, help="object scale (default width / 640)")
    ap.add_argument("--launches", type=int, default=4, help="timed launches per kernel and round")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sample", type=int, default=8192, help="rays of the kept-count histogram")
    args = ap.parse_args()
    import torch
    import __graft_entry__

    pkg = __graft_entry__.load_package()
    pkg.library()
    w, h = args.width, args.height
    n = w * h
    k = args.k if args.k is not None else w / 640.0
    scene = pkg.Scene.synthetic(w, h, args.spheres, args.cubes, seed=args.seed, k=k)
    scene.lights = np.array([(LIGHT[0] * w, LIGHT[1] * h, LIGHT[2], 1.0)], np.float32)
    names = ("sphere_origins", "sphere_radius", "sphere_colours", "cube_vertices", "cube_colours",
             "lights")
    keep = {name: torch.from_numpy(np.ascontiguousarray(getattr(scene, name))).to("cuda:0")
            for name in names if getattr(scene, name).size}
    ds = {name: v.data_ptr() for name, v in keep.items()}
    ds.update(num_spheres=args.spheres, num_cubes=args.cubes, num_lights=1)
    dev = dict(device="cuda:0")
    hits = torch.empty((h, w, 2), dtype=torch.int32, **dev)      # the config's hit frame
    surf = torch.empty((h, w, 4), dtype=torch.float32, **dev)    # its normals
    rays = torch.empty((n, 8), dtype=torch.int32, **dev)         # the reference camera's rays
    out = {c: torch.empty((n, 2), dtype=torch.int32, **dev) for c in ("culled", "unculled")}
    accel = torch.empty((max(args.cubes, 1), 80), dtype=torch.int32, **dev)  # 320 bytes each
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    d = pkg.primary_ray_dir()
    cam = pkg.Camera.reference(d)
    pin = pkg.Camera.pinhole((w / 2, h / 2, 1.2 * h), (w / 2, h / 2, -100.0 * k), (0, -1, 0), 50.0,
                             w, h)

    with pkg.RayTracer(0) as rt:
        with torch.cuda.stream(stream):
            rt.render_device(ds, w, h, (0, h), hits.data_ptr(), ray_dir=d, fmt="hit", stream=st)
            rt.hit_surfaces_device(hits.data_ptr(), ds, w, (0, h), surf.data_ptr(), ray_dir=d,
                                   stream=st)
            rt.camera_rays_device(cam, w, (0, h), rays.data_ptr(), stream=st)
            rt.build_accel_device(ds, accel.data_ptr(), stream=st)
            pin_rays = torch.empty_like(rays)  # (for the kept-count histogram only)
            rt.camera_rays_device(pin, w, (0, h), pin_rays.data_ptr(), stream=st)
        stream.synchronize()
        want = pkg.build_accel(scene)
        if accel.cpu().numpy().tobytes()[:want.nbytes] != want.tobytes():
            raise SystemExit("the device's records differ from the host's")
        permuted = rays[torch.randperm(n, generator=torch.Generator("cuda:0").manual_seed(1),
                                       **dev)].contiguous()
        # one light's segments: the facing hit pixels, in pixel order
        t = hits[..., 0].view(torch.float32)
        obj = hits[..., 1]
        xs = torch.arange(w, dtype=torch.float32, **dev)[None, :].expand(h, w)
        ys = torch.arange(h, dtype=torch.float32, **dev)[:, None].expand(h, w)
        p = torch.stack([xs + t * float(d[0]), ys + t * float(d[1]), t * float(d[2])], -1)
        light = torch.tensor(scene.lights[0, :3], **dev)
        L = light - p
        facing = (obj >= 0) & ((surf[..., :3] * L).sum(-1) > 0)
        seg = torch.zeros((int(facing.sum()), 8), dtype=torch.int32, **dev)
        seg.view(torch.float32)[:, 0:3] = p[facing]
        seg.view(torch.float32)[:, 4:7] = L[facing]
        seg[:, 3] = obj[facing]
        n_seg = seg.shape[0]
        flags = {c: torch.empty((n_seg,), dtype=torch.uint8, **dev) for c in ("culled", "unculled")}
        del p, L, xs, ys, surf
        torch.cuda.synchronize()
        a, hc, hu = accel.data_ptr(), out["culled"].data_ptr(), out["unculled"].data_ptr()

        # case -> (culled launch, unculled launch, the two outputs, rays for the histogram)
        cases = {
            "cast_camera_ref": (
                lambda: rt.cast_camera_accel_device(cam, ds, a, w, (0, h), hc, stream=st),
                lambda: rt.cast_camera_device(cam, ds, w, (0, h), hu, stream=st), out, rays, False),
            "cast_camera_pinhole": (
                lambda: rt.cast_camera_accel_device(pin, ds, a, w, (0, h), hc, stream=st),
                lambda: rt.cast_camera_device(pin, ds, w, (0, h), hu, stream=st), out, pin_rays,
                False),
            "cast_rays": (
                lambda: rt.cast_rays_accel_device(rays.data_ptr(), n, ds, a, hc, stream=st),
                lambda: rt.cast_rays_device(rays.data_ptr(), n, ds, hu, stream=st), out, rays,
                False),
            "cast_rays_permuted": (
                lambda: rt.cast_rays_accel_device(permuted.data_ptr(), n, ds, a, hc, stream=st),
                lambda: rt.cast_rays_device(permuted.data_ptr(), n, ds, hu, stream=st), out,
                permuted, False),
            "occlude_rays": (
                lambda: rt.occlude_rays_accel_device(seg.data_ptr(), n_seg, ds, a,
                                                     flags["culled"].data_ptr(), stream=st),
                lambda: rt.occlude_rays_device(seg.data_ptr(), n_seg, ds,
                                               flags["unculled"].data_ptr(), stream=st), flags, seg,
                True),
        }

        def timed(fn, count):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                   for _ in range(count)]
            with torch.cuda.stream(stream):
                for e0, e1 in evs:
                    e0.record()
                    fn()
                    e1.record()
            stream.synchronize()
            return [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]

        # warm-up, and culled = unculled word for word before anything is timed
        kept = {}
        for name, (culled, unculled, outputs, sample, segment) in cases.items():
            for c in outputs.values():
                c.fill_(0x5A)
            timed(culled, args.warmup)
            timed(unculled, args.warmup)
            if not torch.equal(outputs["culled"], outputs["unculled"]):
                raise SystemExit(f"{name}: the culled output differs from the unculled one")
            pick = np.random.default_rng(2).choice(len(sample), min(args.sample, len(sample)), False)
            picked = sample[torch.from_numpy(pick).to("cuda:0")].cpu().numpy()
            counts = pkg.accel_kept(np.ascontiguousarray(picked).view(pkg.RAY_DTYPE).reshape(-1),
                                    scene, want, segment)
            kept[name] = {"mean": round(float(counts.mean()), 3),
                          "histogram": np.bincount(counts, minlength=1).tolist()}
        build = lambda: rt.build_accel_device(ds, a, stream=st)  # noqa: E731
        timed(build, args.warmup)
        times = {f"{name}/{c}": [] for name in cases for c in ("culled", "unculled")}
        times["accel_build"] = []
        for _ in range(args.rounds):
            for name, (culled, unculled, *_rest) in cases.items():
                times[f"{name}/culled"] += timed(culled, args.launches)
                times[f"{name}/unculled"] += timed(unculled, args.launches)
            times["accel_build"] += timed(build, args.launches)

    result = {"frame": [w, h], "spheres": args.spheres, "cubes": args.cubes, "seed": args.seed,
              "k": k, "rays": n, "segments": n_seg, "launches": args.rounds * args.launches,
              "kept_of_cubes": kept, "us": {}, "unculled_over_culled": {}}
    for name, ts in times.items():
        q = statistics.quantiles(ts, n=4)
        result["us"][name] = {"median": round(statistics.median(ts), 1), "q1": round(q[0], 1),
                              "q3": round(q[2], 1), "min": round(min(ts), 1)}
    for name in cases:
        result["unculled_over_culled"][name] = round(
            result["us"][f"{name}/unculled"]["median"] / result["us"][f"{name}/culled"]["median"], 2)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
