"""The light pass of a camera view, in one process: HIP-event
time per frame, on one stream, the two sides of a pair interleaved round by
round, at three settings (all with shadows):

  depth0            max_bounces 0
  depth1_r0.25      max_bounces 1, reflectivity 0.25 everywhere
  depth8_r1         max_bounces 8, every object a perfect mirror

  reference/<setting>   Camera.reference: `fused`, one culled
                        rt_light_camera_device launch, against `two_launches`,
                        the only way to that frame without it:
                        rt_cast_camera_accel_device into a hit frame, then
                        rt_light_hits_mirrored_accel_device over it
  pinhole/<setting>     a pinhole in front of the scene: rt_light_camera_device
                        `culled` against `unculled`

Prints one JSON line.

    python scripts/camera_light_bench.py          # config 3, three lights

Before anything is timed the two frames of every pair are compared word for
word over the whole frame, and the device-built records with the host's byte
for byte.  The first side of a pair is "faster" / "slower" where the quartile
ranges of the two sides' frames do not overlap, else "equal".
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
LIGHTS = [(0.5, 0.5, 200.0), (0.0, 0.0, 50.0), (1.25, 1.125, -20.0)]  # x, y in frame sizes
SETTINGS = (("depth0", "quarter", 0), ("depth1_r0.25", "quarter", 1), ("depth8_r1", "ones", 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--spheres", type=int, default=256)
    ap.add_argument("--cubes", type=int, default=64)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--k", type=float, default=None, help="object scale (default width / 640)")
    ap.add_argument("--launches", type=int, default=2, help="timed frames per side and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fov", type=float, default=50.0, help="the pinhole's, degrees over the height")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("at least three interleaved rounds")
    import torch
    import __graft_entry__

    pkg = __graft_entry__.load_package()
    pkg.library()
    w, h = args.width, args.height
    k = args.k if args.k is not None else w / 640.0
    scene = pkg.Scene.synthetic(w, h, args.spheres, args.cubes, seed=args.seed, k=k)
    scene.lights = np.array([(x * w, y * h, z, 1.0) for x, y, z in LIGHTS], np.float32)
    names = ("sphere_origins", "sphere_radius", "sphere_colours", "cube_vertices", "cube_colours",
             "lights")
    keep = {n: torch.from_numpy(np.ascontiguousarray(getattr(scene, n))).to("cuda:0")
            for n in names if getattr(scene, n).size}
    ds = {n: v.data_ptr() for n, v in keep.items()}
    ds.update(num_spheres=args.spheres, num_cubes=args.cubes, num_lights=len(LIGHTS))
    slots = args.spheres + args.cubes
    dev = dict(device="cuda:0")
    refl = {"quarter": torch.full((slots,), 0.25, dtype=torch.float32, **dev),
            "ones": torch.ones((slots,), dtype=torch.float32, **dev)}
    hits = torch.empty((h, w, 2), dtype=torch.int32, **dev)
    accel = torch.empty((max(args.cubes, 1), 80), dtype=torch.int32, **dev)  # 320 bytes each
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    d = pkg.primary_ray_dir()
    hp, a = hits.data_ptr(), accel.data_ptr()
    reference = pkg.Camera.reference(d)
    # in front of the frame's centre, far enough to see all of it, looking into the scene
    distance = 0.5 * h / np.tan(np.radians(args.fov) / 2)
    pinhole = pkg.Camera.pinhole((0.5 * w, 0.5 * h, distance), (0.5 * w, 0.5 * h, -100.0 * k),
                                 (0, -1, 0), args.fov, w, h)

    with pkg.RayTracer(0) as rt:
        with torch.cuda.stream(stream):
            rt.build_accel_device(ds, a, stream=st)
        stream.synchronize()
        want = pkg.build_accel(scene)
        if accel.cpu().numpy().tobytes()[:want.nbytes] != want.tobytes():
            raise SystemExit("the device's records differ from the host's")

        def frame():
            return torch.full((h, w, 4), 0x5A5A5A5A, dtype=torch.int32, **dev)

        def fused(cam, accel_ptr, out, r, depth):
            rt.light_camera_device(cam, ds, accel_ptr, w, (0, h), r, depth, out.data_ptr(),
                                   fmt="i32x4", shadows=True, stream=st)

        def two_launches(out, r, depth):
            rt.cast_camera_accel_device(reference, ds, a, w, (0, h), hp, stream=st)
            rt.light_hits_mirrored_accel_device(hp, ds, a, w, (0, h), out.data_ptr(), r, depth,
                                                ray_dir=d, stream=st, fmt="i32x4", shadows=True)

        # pair -> (first side's name, second side's, the two outputs, the two launches)
        pairs = {}
        for name, which, depth in SETTINGS:
            r = refl[which].data_ptr()
            o1, o2 = frame(), frame()
            pairs[f"reference/{name}"] = (
                "fused", "two_launches", (o1, o2),
                lambda o=o1, r=r, depth=depth: fused(reference, a, o, r, depth),
                lambda o=o2, r=r, depth=depth: two_launches(o, r, depth))
            o1, o2 = frame(), frame()
            pairs[f"pinhole/{name}"] = (
                "culled", "unculled", (o1, o2),
                lambda o=o1, r=r, depth=depth: fused(pinhole, a, o, r, depth),
                lambda o=o2, r=r, depth=depth: fused(pinhole, 0, o, r, depth))

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

        # one warm-up frame per side, and the pair's frames word for word
        shares = {}
        for name, (_, _, (o1, o2), first, second) in pairs.items():
            timed(first, 1)
            timed(second, 1)
            if not torch.equal(o1, o2):
                raise SystemExit(f"{name}: the two frames differ")
            if bool((o1 == 0x5A5A5A5A).all()):
                raise SystemExit(f"{name}: nothing was written")
            shares[name] = {"lit_pixels": float((o1[..., :3] != 0).any(-1).float().mean())}
        if accel.cpu().numpy().tobytes()[:want.nbytes] != want.tobytes():
            raise SystemExit("the records changed")
        times = {f"{name}/{side}": [] for name, p in pairs.items() for side in p[:2]}
        for _ in range(args.rounds):
            for name, (s1, s2, _, first, second) in pairs.items():
                times[f"{name}/{s1}"] += timed(first, args.launches)
                times[f"{name}/{s2}"] += timed(second, args.launches)

    # the share of the cubes a camera ray keeps, on a sample of each camera's rays
    kept = {}
    rng = np.random.default_rng(2)
    rows = np.sort(rng.choice(h, min(8, h), False))
    for cam_name, cam in (("reference", reference), ("pinhole", pinhole)):
        counts = np.concatenate([pkg.accel_kept(pkg.camera_rays(cam, w, h, (int(y), int(y) + 1)),
                                                scene, want).reshape(-1) for y in rows])
        kept[cam_name] = round(float(counts.mean()), 3)

    result = {"frame": [w, h], "spheres": args.spheres, "cubes": args.cubes, "seed": args.seed,
              "k": k, "lights": len(LIGHTS), "fov": args.fov, "rounds": args.rounds,
              "launches": args.rounds * args.launches, "shares": shares,
              "kept_of_cubes_per_camera_ray": kept, "us": {}, "pairs": {}}
    for name, ts in times.items():
        q = statistics.quantiles(ts, n=4)
        result["us"][name] = {"median": round(statistics.median(ts), 1), "q1": round(q[0], 1),
                              "q3": round(q[2], 1), "min": round(min(ts), 1),
                              "max": round(max(ts), 1)}
    for name, (s1, s2, *_) in pairs.items():
        f, s = result["us"][f"{name}/{s1}"], result["us"][f"{name}/{s2}"]
        verdict = "faster" if f["q3"] < s["q1"] else "slower" if f["q1"] > s["q3"] else "equal"
        result["pairs"][name] = {"first": s1, "second": s2, "verdict": verdict,
                                 f"{s2}_over_{s1}": round(s["median"] / f["median"], 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
