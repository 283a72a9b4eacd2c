"""The ray queries culled by grouped sphere bounds beside their *_accel twins, in
one process: HIP-event time per launch of each pair

  cast_camera_ref      rt_cast_camera_{grouped,accel}_device, the reference camera
  cast_camera_pinhole  the same with a pinhole camera in front of the frame
  cast_rays            rt_cast_rays_{grouped,accel}_device on the reference
                       camera's rays from a buffer (32 bytes per ray)
  cast_rays_permuted   the same buffer with its rays randomly permuted: a wave's
                       64 rays then go 64 different ways, and the wave-level
                       skip of a group needs all of them to drop it
  occlude_rays         rt_occlude_rays_{grouped,accel}_device on one light's
                       segments: the facing hit pixels' (p, light - p, own
                       object), compacted in pixel order

for every --group-size in turn, and of rt_sphere_groups_build_device alone at
the scene's spheres and at --build-spheres, interleaved round by round after
warm-up.  The yardstick is the *_accel twin (the cube cull alone).  Prints one
JSON line per group size.

    python scripts/sphere_groups_bench.py                    # config 3

Before anything is timed the device's records are compared with the host's byte
for byte and every grouped output with its twin's word for word.  The
kept-count histogram is rt_sphere_groups_kept on a sample of each case's rays.
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
    ap.add_argument("--group-size", type=int, action="append", default=None)
    ap.add_argument("--build-spheres", type=int, default=4096,
                    help="a second scene's sphere count for the build's time alone")
    args = ap.parse_args()
    sizes = args.group_size or [4, 8]
    import torch
    import __graft_entry__

    pkg = __graft_entry__.load_package()
    lib = pkg.library()
    w, h = args.width, args.height
    n = w * h
    k = args.k if args.k is not None else w / 640.0
    scene = pkg.Scene.synthetic(w, h, args.spheres, args.cubes, seed=args.seed, k=k)
    scene.lights = np.array([(LIGHT[0] * w, LIGHT[1] * h, LIGHT[2], 1.0)], np.float32)
    dev = dict(device="cuda:0")

    def upload(sc):
        names = ("sphere_origins", "sphere_radius", "sphere_colours", "cube_vertices",
                 "cube_colours", "lights")
        held = {name: torch.from_numpy(np.ascontiguousarray(getattr(sc, name))).to("cuda:0")
                for name in names if getattr(sc, name).size}
        d = {name: v.data_ptr() for name, v in held.items()}
        d.update(num_spheres=sc.num_spheres, num_cubes=sc.num_cubes, num_lights=len(sc.lights))
        return d, held

    ds, keep = upload(scene)
    hits = torch.empty((h, w, 2), dtype=torch.int32, **dev)      # the config's hit frame
    surf = torch.empty((h, w, 4), dtype=torch.float32, **dev)    # its normals
    rays = torch.empty((n, 8), dtype=torch.int32, **dev)         # the reference camera's rays
    out = {c: torch.empty((n, 2), dtype=torch.int32, **dev) for c in ("grouped", "accel")}
    accel = torch.empty((max(args.cubes, 1), 80), dtype=torch.int32, **dev)  # 320 bytes each
    big = pkg.Scene.synthetic(w, h, args.build_spheres, 0, seed=args.seed, k=k)
    big_ds, big_keep = upload(big)
    most = max(args.spheres, args.build_spheres)
    records = torch.empty((max(most, 1), 16), dtype=torch.int32, **dev)      # 64 bytes each
    ws_bytes = lib.rt_sphere_groups_workspace_bytes(most)
    workspace = torch.empty((ws_bytes,), dtype=torch.uint8, **dev)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    d = pkg.primary_ray_dir()
    cam = pkg.Camera.reference(d)
    pin = pkg.Camera.pinhole((w / 2, h / 2, 1.2 * h), (w / 2, h / 2, -100.0 * k), (0, -1, 0), 50.0,
                             w, h)

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
        flags = {c: torch.empty((n_seg,), dtype=torch.uint8, **dev) for c in ("grouped", "accel")}
        del p, L, xs, ys, surf
        torch.cuda.synchronize()
        a, hg, ha = accel.data_ptr(), out["grouped"].data_ptr(), out["accel"].data_ptr()
        g = records.data_ptr()

        for group_size in sizes:
            ng = lib.rt_sphere_groups_count(args.spheres, group_size)
            build = lambda: rt.build_sphere_groups_device(  # noqa: E731
                ds, group_size, g, workspace.data_ptr(), ws_bytes, stream=st)
            build_big = lambda: rt.build_sphere_groups_device(  # noqa: E731
                big_ds, group_size, g, workspace.data_ptr(), ws_bytes, stream=st)
            # the second scene's records first, checked, then this scene's, which stay
            for fn, sc in ((build_big, big), (build, scene)):
                timed(fn, args.warmup)
                want = pkg.build_sphere_groups(sc, group_size)
                if records.cpu().numpy().tobytes()[:want.nbytes] != want.tobytes():
                    raise SystemExit(f"the device's records differ from the host's "
                                     f"({sc.num_spheres} spheres, groups of {group_size})")

            # case -> (grouped launch, accel launch, the two outputs, rays for the histogram)
            cases = {
                "cast_camera_ref": (
                    lambda: rt.cast_camera_grouped_device(cam, ds, a, g, ng, w, (0, h), hg,
                                                          stream=st),
                    lambda: rt.cast_camera_accel_device(cam, ds, a, w, (0, h), ha, stream=st),
                    out, rays, False),
                "cast_camera_pinhole": (
                    lambda: rt.cast_camera_grouped_device(pin, ds, a, g, ng, w, (0, h), hg,
                                                          stream=st),
                    lambda: rt.cast_camera_accel_device(pin, ds, a, w, (0, h), ha, stream=st),
                    out, pin_rays, False),
                "cast_rays": (
                    lambda: rt.cast_rays_grouped_device(rays.data_ptr(), n, ds, a, g, ng, hg,
                                                        stream=st),
                    lambda: rt.cast_rays_accel_device(rays.data_ptr(), n, ds, a, ha, stream=st),
                    out, rays, False),
                "cast_rays_permuted": (
                    lambda: rt.cast_rays_grouped_device(permuted.data_ptr(), n, ds, a, g, ng, hg,
                                                        stream=st),
                    lambda: rt.cast_rays_accel_device(permuted.data_ptr(), n, ds, a, ha,
                                                      stream=st), out, permuted, False),
                "occlude_rays": (
                    lambda: rt.occlude_rays_grouped_device(seg.data_ptr(), n_seg, ds, a, g, ng,
                                                           flags["grouped"].data_ptr(), stream=st),
                    lambda: rt.occlude_rays_accel_device(seg.data_ptr(), n_seg, ds, a,
                                                         flags["accel"].data_ptr(), stream=st),
                    flags, seg, True),
            }
            # warm-up, and grouped = accel word for word before anything is timed
            kept = {}
            for name, (grouped, twin, outputs, sample, segment) in cases.items():
                for c in outputs.values():
                    c.fill_(0x5A)
                timed(grouped, args.warmup)
                timed(twin, args.warmup)
                if not torch.equal(outputs["grouped"], outputs["accel"]):
                    raise SystemExit(f"{name}: the grouped output differs from its twin's")
                pick = np.random.default_rng(2).choice(len(sample), min(args.sample, len(sample)),
                                                       False)
                picked = sample[torch.from_numpy(pick).to("cuda:0")].cpu().numpy()
                counts = pkg.sphere_groups_kept(
                    np.ascontiguousarray(picked).view(pkg.RAY_DTYPE).reshape(-1), scene, want,
                    segment)
                kept[name] = {"mean": round(float(counts.mean()), 3),
                              "histogram": np.bincount(counts, minlength=1).tolist()}
            times = {f"{name}/{c}": [] for name in cases for c in ("grouped", "accel")}
            times["groups_build"], times["groups_build_big"] = [], []
            for _ in range(args.rounds):
                for name, (grouped, twin, *_rest) in cases.items():
                    times[f"{name}/grouped"] += timed(grouped, args.launches)
                    times[f"{name}/accel"] += timed(twin, args.launches)
                times["groups_build_big"] += timed(build_big, args.launches)
                times["groups_build"] += timed(build, args.launches)  # (last: the scene's records)

            result = {"frame": [w, h], "spheres": args.spheres, "cubes": args.cubes,
                      "seed": args.seed, "k": k, "rays": n, "segments": n_seg,
                      "group_size": group_size, "groups": ng, "build_big_spheres": args.build_spheres,
                      "launches": args.rounds * args.launches, "kept_of_groups": kept, "us": {},
                      "accel_over_grouped": {}}
            for name, ts in times.items():
                q = statistics.quantiles(ts, n=4)
                result["us"][name] = {"median": round(statistics.median(ts), 1),
                                      "q1": round(q[0], 1), "q3": round(q[2], 1),
                                      "min": round(min(ts), 1)}
            for name in cases:
                result["accel_over_grouped"][name] = round(
                    result["us"][f"{name}/accel"]["median"] /
                    result["us"][f"{name}/grouped"]["median"], 2)
            print(json.dumps(result), flush=True)
    del keep, big_keep


if __name__ == "__main__":
    main()
