"""The shadowed, mirrored light pass beside the kernels it
combines, in one process: HIP-event time per launch of the HIT trace, of
rt_light_hits_shadowed_device, of rt_light_hits_reflected_device (with the
scene's lights and without lights), and of the new kernel's three outputs at
reflectivity 0.5 (the mask at p2, i32x4, rgba8), of its i32x4 form at
reflectivity 0 (the shadow kernel's work) and without lights (the reflect
kernel's work), over one hit frame, interleaved round by round.  Prints one
JSON line.

    python scripts/shadow_reflect_bench.py               # config 3, one light
    python scripts/shadow_reflect_bench.py --lights 3

A band of each new output is checked against the host functions before
anything is timed.
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
OUT_WORDS = {"mask2": 1, "i32x4": 4, "rgba8": 1}
REFLECTIVITY = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--spheres", type=int, default=256)
    ap.add_argument("--cubes", type=int, default=64)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--k", type=float, default=None, help="object scale (default width / 640)")
    ap.add_argument("--lights", type=int, default=1, choices=(1, 2, 3))
    ap.add_argument("--launches", type=int, default=4, help="timed launches per kernel and round")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check-rows", type=int, default=4)
    args = ap.parse_args()
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
    dark = dict(ds, num_lights=0)
    hits = torch.empty((h, w, 2), dtype=torch.int32, device="cuda:0")
    frame = torch.empty((h, w, 4), dtype=torch.int32, device="cuda:0")  # the parent kernels
    bounce = torch.empty((h, w, 2), dtype=torch.int32, device="cuda:0")
    outs = {what: torch.empty((h, w, words), dtype=torch.int32, device="cuda:0")
            for what, words in OUT_WORDS.items()}
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    d = pkg.primary_ray_dir()

    with pkg.RayTracer(0) as rt:
        def reflected(scene_dict, out, refl, shadows):
            rt.light_hits_reflected_device(hits.data_ptr(), scene_dict, w, (0, h), out.data_ptr(),
                                           refl, ray_dir=d, stream=st, fmt="i32x4",
                                           shadows=shadows)

        def combined(what):
            out = outs[what].data_ptr()
            if what == "mask2":
                rt.shadow_hits_reflected_device(hits.data_ptr(), ds, w, (0, h), out, ray_dir=d,
                                                stream=st)
            else:
                rt.light_hits_reflected_device(hits.data_ptr(), ds, w, (0, h), out, REFLECTIVITY,
                                               ray_dir=d, stream=st, fmt=what, shadows=True)

        kernels = {
            "trace_hit": lambda: rt.render_device(ds, w, h, (0, h), hits.data_ptr(), ray_dir=d,
                                                  fmt="hit", stream=st),
            "shadowed_i32x4": lambda: rt.light_hits_device(hits.data_ptr(), ds, w, (0, h),
                                                           frame.data_ptr(), ray_dir=d, stream=st,
                                                           shadows=True),
            "reflected_i32x4": lambda: reflected(ds, frame, REFLECTIVITY, False),
            "reflected_i32x4_no_lights": lambda: reflected(dark, frame, REFLECTIVITY, False),
        }
        for what in OUT_WORDS:
            kernels["shadowed_reflected_" + what] = (lambda what=what: combined(what))
        kernels["shadowed_reflected_i32x4_r0"] = lambda: reflected(ds, frame, 0.0, True)
        kernels["shadowed_reflected_i32x4_no_lights"] = lambda: reflected(dark, frame,
                                                                          REFLECTIVITY, True)

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
        for name, fn in kernels.items():
            timed(fn, args.warmup)
            if name == "trace_hit":
                trace_kernel = rt.last_kernel()
        # a band of every new output against the host functions
        rows = (h // 2, min(h, h // 2 + args.check_rows))
        band = hits[rows[0]:rows[1]].cpu().numpy().view(pkg.HIT_DTYPE).reshape(-1, w)
        obj = hits[..., 1]
        share = {"cube": float(((obj >= 0) & (obj < args.cubes)).float().mean()),
                 "sphere": float((obj >= args.cubes).float().mean()),
                 "miss": float((obj < 0).float().mean())}
        for what in OUT_WORDS:
            got = outs[what][rows[0]:rows[1]].cpu().numpy()
            want = (pkg.shadow_hits_reflected(band, scene, rows=rows, ray_dir=d)
                    if what == "mask2"
                    else pkg.light_hits_shadowed_reflected(band, scene, REFLECTIVITY, what,
                                                           rows=rows, ray_dir=d))
            want = np.ascontiguousarray(want).view(np.int32).reshape(got.shape)
            if not np.array_equal(got, want):
                raise SystemExit(f"{what}: rows {rows} differ from the host function")
        with torch.cuda.stream(stream):
            rt.reflect_hits_device(hits.data_ptr(), ds, w, (0, h), bounce.data_ptr(), ray_dir=d,
                                   stream=st)
        stream.synchronize()
        met = bounce[..., 1] >= 0
        n_hit, n_met = max(1.0, float((obj >= 0).sum())), max(1.0, float(met.sum()))
        shadowed2 = outs["mask2"][..., 0] != 0
        shares = {"bounce_hits_of_all_pixels": float(met.float().mean()),
                  "bounce_hits_of_hit_pixels": float(met.sum()) / n_hit,
                  "shadowed_at_p2_of_all_pixels": float(shadowed2.float().mean()),
                  "shadowed_at_p2_of_bounce_hits": float(shadowed2.sum()) / n_met}
        times = {name: [] for name in kernels}
        for _ in range(args.rounds):
            for name, fn in kernels.items():
                times[name] += timed(fn, args.launches)

    result = {"frame": [w, h], "spheres": args.spheres, "cubes": args.cubes, "seed": args.seed,
              "k": k, "lights": args.lights, "reflectivity": REFLECTIVITY, "pixel_share": share,
              "shares": shares, "trace_kernel": trace_kernel,
              "launches": args.rounds * args.launches, "us": {}}
    for name, ts in times.items():
        q = statistics.quantiles(ts, n=4)
        result["us"][name] = {"median": round(statistics.median(ts), 1), "q1": round(q[0], 1),
                              "q3": round(q[2], 1), "min": round(min(ts), 1),
                              "max": round(max(ts), 1)}
    us = result["us"]
    result["sum_of_parents_us"] = round(us["shadowed_i32x4"]["median"] +
                                        us["reflected_i32x4"]["median"], 1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
