"""The mirror chain of the light pass beside the one-bounce
kernels, in one process: HIP-event time per launch, over one hit frame, on one
stream, interleaved round by round, of

  (a) rt_light_hits_shadowed_reflected_device at reflectivity 0.25 (the
      existing kernel: the figure the new one is read against),
  (b) rt_light_hits_mirrored_device at depth 1 with 0.25 everywhere and
      shadows: the same frame,
  (c) rt_light_hits_mirrored_device at depths 2, 4 and 8 with every object a
      perfect mirror, shadows on,
  (d) rt_bounce_hits_device at bounces 1 and 2 beside rt_reflect_hits_device.

Prints one JSON line.

    python scripts/mirror_bench.py               # config 3, three lights

Before anything is timed a band of every timed frame is compared word for word
with the host function (--check-rows rows, split over --check-threads
threads), and (a) and (b) with each other over the whole frame.
"""
import argparse
import json
import os
import statistics
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
LIGHTS = [(0.5, 0.5, 200.0), (0.0, 0.0, 50.0), (1.25, 1.125, -20.0)]  # x, y in frame sizes
REFLECTIVITY = 0.25
DEPTHS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--spheres", type=int, default=256)
    ap.add_argument("--cubes", type=int, default=64)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--k", type=float, default=None, help="object scale (default width / 640)")
    ap.add_argument("--lights", type=int, default=3, choices=(1, 2, 3))
    ap.add_argument("--launches", type=int, default=2, help="timed launches per kernel and round")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--check-threads", type=int, default=min(16, os.cpu_count() or 1))
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
    scene.lights = np.array([(x * w, y * h, z, 1.0) for x, y, z in LIGHTS[:args.lights]],
                            np.float32).reshape(-1, 4)
    names = ("sphere_origins", "sphere_radius", "sphere_colours", "cube_vertices", "cube_colours",
             "lights")
    keep = {n: torch.from_numpy(np.ascontiguousarray(getattr(scene, n))).to("cuda:0")
            for n in names if getattr(scene, n).size}
    ds = {n: v.data_ptr() for n, v in keep.items()}
    ds.update(num_spheres=args.spheres, num_cubes=args.cubes, num_lights=args.lights)
    slots = args.spheres + args.cubes
    refl = {"quarter": np.full(slots, REFLECTIVITY, np.float32), "ones": np.ones(slots, np.float32)}
    refl_dev = {n: torch.from_numpy(a).to("cuda:0") for n, a in refl.items()}
    hits = torch.empty((h, w, 2), dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    d = pkg.primary_ray_dir()

    def frame(words):
        return torch.empty((h, w, words), dtype=torch.int32, device="cuda:0")

    with pkg.RayTracer(0) as rt:
        def mirrored(out, which, depth):
            rt.light_hits_mirrored_device(hits.data_ptr(), ds, w, (0, h), out.data_ptr(),
                                          refl_dev[which].data_ptr(), depth, ray_dir=d, stream=st,
                                          fmt="i32x4", shadows=True)

        # name: (output, launch, the host function on a band)
        kernels = {}
        out = frame(4)
        kernels["shadowed_reflected_r0.25"] = (
            out, lambda out=out: rt.light_hits_reflected_device(
                hits.data_ptr(), ds, w, (0, h), out.data_ptr(), REFLECTIVITY, ray_dir=d,
                stream=st, fmt="i32x4", shadows=True),
            lambda band, rows: pkg.light_hits_shadowed_reflected(band, scene, REFLECTIVITY,
                                                                 rows=rows, ray_dir=d))
        out = frame(4)
        kernels["mirrored_depth1_r0.25"] = (
            out, lambda out=out: mirrored(out, "quarter", 1),
            lambda band, rows: pkg.light_hits_mirrored(band, scene, refl["quarter"], 1,
                                                       shadows=True, rows=rows, ray_dir=d))
        for depth in DEPTHS:
            out = frame(4)
            kernels[f"mirrored_depth{depth}_r1"] = (
                out, lambda out=out, depth=depth: mirrored(out, "ones", depth),
                lambda band, rows, depth=depth: pkg.light_hits_mirrored(
                    band, scene, refl["ones"], depth, shadows=True, rows=rows, ray_dir=d))
        out = frame(2)
        kernels["reflect_hits"] = (
            out, lambda out=out: rt.reflect_hits_device(hits.data_ptr(), ds, w, (0, h),
                                                        out.data_ptr(), ray_dir=d, stream=st),
            lambda band, rows: pkg.reflect_hits(band, scene, rows=rows, ray_dir=d))
        for b in (1, 2):
            out = frame(2)
            kernels[f"bounce_hits_{b}"] = (
                out, lambda out=out, b=b: rt.bounce_hits_device(hits.data_ptr(), ds, w, (0, h),
                                                                out.data_ptr(), b, ray_dir=d,
                                                                stream=st),
                lambda band, rows, b=b: pkg.bounce_hits(band, scene, b, rows=rows, ray_dir=d))

        def timed(fn, n):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                   for _ in range(n)]
            with torch.cuda.stream(stream):
                for a, b in evs:
                    a.record()
                    fn()
                    b.record()
            stream.synchronize()
            return [a.elapsed_time(b) * 1e3 for a, b in evs]

        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            rt.render_device(ds, w, h, (0, h), hits.data_ptr(), ray_dir=d, fmt="hit", stream=st)
        stream.synchronize()
        for _, fn, _ in kernels.values():
            timed(fn, args.warmup)

        # every timed frame against the host function on a band, in slices
        rows = (h // 2 - args.check_rows // 2, h // 2 - args.check_rows // 2 + args.check_rows)
        rows = (max(0, rows[0]), min(h, rows[1]))
        band = hits[rows[0]:rows[1]].cpu().numpy().view(pkg.HIT_DTYPE).reshape(-1, w)
        step = max(1, -(-(rows[1] - rows[0]) // args.check_threads))
        slices = [(r, min(rows[1], r + step)) for r in range(rows[0], rows[1], step)]
        with ThreadPoolExecutor(args.check_threads) as pool:
            for name, (out, _, host) in kernels.items():
                got = out[rows[0]:rows[1]].cpu().numpy()
                parts = pool.map(lambda s: host(np.ascontiguousarray(
                    band[s[0] - rows[0]:s[1] - rows[0]]), s), slices)
                want = np.concatenate([np.ascontiguousarray(p).view(np.int32).reshape(
                    -1, w, got.shape[-1]) for p in parts])
                if not np.array_equal(got, want):
                    raise SystemExit(f"{name}: rows {rows} differ from the host function")
        same = bool(torch.equal(kernels["shadowed_reflected_r0.25"][0],
                                kernels["mirrored_depth1_r0.25"][0]))
        if not same:
            raise SystemExit("depth 1 with one reflectivity is not the one-bounce kernel's frame")
        if not torch.equal(kernels["reflect_hits"][0], kernels["bounce_hits_1"][0]):
            raise SystemExit("bounce 1 is not the reflect kernel's frame")
        obj = hits[..., 1]
        shares = {"hit_pixels": float((obj >= 0).float().mean()),
                  "bounce_1_hits_of_all_pixels":
                      float((kernels["bounce_hits_1"][0][..., 1] >= 0).float().mean()),
                  "bounce_2_hits_of_all_pixels":
                      float((kernels["bounce_hits_2"][0][..., 1] >= 0).float().mean())}
        times = {name: [] for name in kernels}
        by_round = {name: [] for name in kernels}
        for _ in range(args.rounds):
            for name, (_, fn, _) in kernels.items():
                ts = timed(fn, args.launches)
                times[name] += ts
                by_round[name].append(round(statistics.median(ts), 1))

    result = {"frame": [w, h], "spheres": args.spheres, "cubes": args.cubes, "seed": args.seed,
              "k": k, "lights": args.lights, "checked_rows": list(rows), "shares": shares,
              "rounds": args.rounds, "launches": args.rounds * args.launches, "us": {},
              "round_medians_us": by_round}
    for name, ts in times.items():
        result["us"][name] = {"median": round(statistics.median(ts), 1),
                              "min": round(min(ts), 1), "max": round(max(ts), 1)}
    med = {name: v["median"] for name, v in result["us"].items()}
    a = by_round["shadowed_reflected_r0.25"]
    result["depth1_over_one_bounce_kernel"] = round(
        med["mirrored_depth1_r0.25"] / med["shadowed_reflected_r0.25"], 4)
    result["one_bounce_kernel_spread"] = [round(min(a) / statistics.median(a), 4),
                                          round(max(a) / statistics.median(a), 4)]
    result["us_per_added_level"] = {
        "2_to_4": round((med["mirrored_depth4_r1"] - med["mirrored_depth2_r1"]) / 2, 1),
        "4_to_8": round((med["mirrored_depth8_r1"] - med["mirrored_depth4_r1"]) / 4, 1)}
    result["bounce_1_over_reflect_hits"] = round(med["bounce_hits_1"] / med["reflect_hits"], 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
