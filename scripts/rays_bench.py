"""The ray queries beside the light-pass kernels that hold the same walks, in
one process: HIP-event time per launch of

  cast_camera     rt_cast_camera_device with the reference camera (no ray buffer)
  cast_rays       rt_cast_rays_device on the same rays, from a buffer that
                  rt_camera_rays_device wrote (32 bytes per ray)
  camera_rays     rt_camera_rays_device alone (the buffer's cost)
  reflect_hits    rt_reflect_hits_device on the config's hit frame: the same
                  closest-hit walk, over the hit pixels only
  occlude_rays    rt_occlude_rays_device on one light's segments: the facing
                  hit pixels' (p, light - p, own object), compacted in pixel order
  shadow_hits     rt_shadow_hits_device with that light: the same any-hit walk

interleaved round by round after warm-up.  Prints one JSON line.

    python scripts/rays_bench.py                    # config 3

Before anything is timed a band of cast_camera's frame is compared with the
host function word for word, cast_rays' frame with cast_camera's, and the
occlusion flags with the shadow mask's bit (the segments are built with torch
arithmetic, which may contract: the share that agrees is reported, not asserted).
The walk is the unculled one; the geometric cull is its own change.
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
    ap.add_argument("--check-rows", type=int, default=2)
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
    rays = torch.empty((n, 8), dtype=torch.float32, **dev)       # the camera's rays
    cast_a = torch.empty((n, 2), dtype=torch.int32, **dev)       # cast_camera
    cast_b = torch.empty((n, 2), dtype=torch.int32, **dev)       # cast_rays
    bounce = torch.empty((h, w, 2), dtype=torch.int32, **dev)
    mask = torch.empty((h, w), dtype=torch.int32, **dev)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    d = pkg.primary_ray_dir()
    cam = pkg.Camera.reference(d)

    with pkg.RayTracer(0) as rt:
        with torch.cuda.stream(stream):
            rt.render_device(ds, w, h, (0, h), hits.data_ptr(), ray_dir=d, fmt="hit", stream=st)
            rt.hit_surfaces_device(hits.data_ptr(), ds, w, (0, h), surf.data_ptr(), ray_dir=d,
                                   stream=st)
            rt.camera_rays_device(cam, w, (0, h), rays.data_ptr(), stream=st)
        stream.synchronize()
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
        flags = torch.empty((n_seg,), dtype=torch.uint8, **dev)
        del p, L, xs, ys
        torch.cuda.synchronize()

        kernels = {
            "cast_camera": lambda: rt.cast_camera_device(cam, ds, w, (0, h), cast_a.data_ptr(),
                                                         stream=st),
            "cast_rays": lambda: rt.cast_rays_device(rays.data_ptr(), n, ds, cast_b.data_ptr(),
                                                     stream=st),
            "camera_rays": lambda: rt.camera_rays_device(cam, w, (0, h), rays.data_ptr(),
                                                         stream=st),
            "reflect_hits": lambda: rt.reflect_hits_device(hits.data_ptr(), ds, w, (0, h),
                                                           bounce.data_ptr(), ray_dir=d, stream=st),
            "occlude_rays": lambda: rt.occlude_rays_device(seg.data_ptr(), n_seg, ds,
                                                           flags.data_ptr(), stream=st),
            "shadow_hits": lambda: rt.shadow_hits_device(hits.data_ptr(), ds, w, (0, h),
                                                         mask.data_ptr(), ray_dir=d, stream=st),
        }

        def timed(fn, count):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                   for _ in range(count)]
            with torch.cuda.stream(stream):
                for a, b in evs:
                    a.record()
                    fn()
                    b.record()
            stream.synchronize()
            return [a.elapsed_time(b) * 1e3 for a, b in evs]

        for fn in kernels.values():
            timed(fn, args.warmup)
        # a band of cast_camera against the host; cast_rays against cast_camera
        rows = (h // 2, min(h, h // 2 + args.check_rows))
        got = cast_a.view(h, w, 2)[rows[0]:rows[1]].cpu().numpy()
        want = pkg.cast_camera(cam, scene, w, h, rows)
        if not np.array_equal(got, np.ascontiguousarray(want).view(np.int32).reshape(got.shape)):
            raise SystemExit(f"cast_camera: rows {rows} differ from the host function")
        if not torch.equal(cast_a, cast_b):
            raise SystemExit("cast_rays' frame differs from cast_camera's")
        agree = float((flags.bool() == ((mask[facing] & 1) != 0)).float().mean())
        cast_obj = cast_a[:, 1]
        share = {"primary_hit": float((obj >= 0).float().mean()),
                 "cast_hit": float((cast_obj >= 0).float().mean()),
                 "cast_equals_hit_frame": float((cast_a.view(h, w, 2) == hits).all(-1).float()
                                                .mean()),
                 "segments_of_all_pixels": n_seg / n,
                 "segments_occluded": float(flags.float().mean()),
                 "flags_equal_shadow_bit": agree}
        times = {name: [] for name in kernels}
        for _ in range(args.rounds):
            for name, fn in kernels.items():
                times[name] += timed(fn, args.launches)

    result = {"frame": [w, h], "spheres": args.spheres, "cubes": args.cubes, "seed": args.seed,
              "k": k, "rays": n, "segments": n_seg, "shares": share,
              "launches": args.rounds * args.launches, "us": {}}
    for name, ts in times.items():
        q = statistics.quantiles(ts, n=4)
        result["us"][name] = {"median": round(statistics.median(ts), 1), "q1": round(q[0], 1),
                              "q3": round(q[2], 1), "min": round(min(ts), 1)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
