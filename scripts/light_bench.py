"""The deferred light pass beside the HIT trace it follows, in one process:
HIP-event time per launch of rt_render_device(fmt="hit"), then of
rt_hit_surfaces_device and rt_light_hits_device (i32x4, rgba8) over that hit
frame, interleaved round by round.  Prints one JSON line.

    python scripts/light_bench.py                    # config 3, one light
    python scripts/light_bench.py --lights 3 --launches 20 --rounds 5

`store_us` is the time the pass's bytes alone (8 B read + the pixel written)
would take at --rate TB/s (default 7.2: the plain frame-store rate of the
headline kernel's ablation, README).  A band of the device frames is checked
against the host functions before anything is timed.
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
OUT_BYTES = {"surface": 16, "i32x4": 16, "rgba8": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--spheres", type=int, default=256)
    ap.add_argument("--cubes", type=int, default=64)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--k", type=float, default=None, help="object scale (default width / 640)")
    ap.add_argument("--lights", type=int, default=1, choices=(0, 1, 2, 3))
    ap.add_argument("--launches", type=int, default=12, help="timed launches per kernel and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rate", type=float, default=7.2, help="TB/s of plain frame stores")
    ap.add_argument("--check-rows", type=int, default=48)
    args = ap.parse_args()
    import torch
    import __graft_entry__

    pkg = __graft_entry__.load_package()
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
    hits = torch.empty((h, w, 2), dtype=torch.int32, device="cuda:0")
    outs = {what: torch.empty((h * w * nbytes // 4,), dtype=torch.int32, device="cuda:0")
            for what, nbytes in OUT_BYTES.items()}
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    d = pkg.primary_ray_dir()

    with pkg.RayTracer(0) as rt:
        def trace():
            rt.render_device(ds, w, h, (0, h), hits.data_ptr(), ray_dir=d, fmt="hit", stream=st)

        def light(what):
            if what == "surface":
                rt.hit_surfaces_device(hits.data_ptr(), ds, w, (0, h), outs[what].data_ptr(),
                                       ray_dir=d, stream=st)
            else:
                rt.light_hits_device(hits.data_ptr(), ds, w, (0, h), outs[what].data_ptr(),
                                     ray_dir=d, stream=st, fmt=what)

        kernels = {"trace_hit": trace}
        kernels.update({what: (lambda what=what: light(what)) for what in OUT_BYTES})

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
        for fn in kernels.values():
            timed(fn, args.warmup)
        # a band of every output against the host functions
        rows = (h // 2, min(h, h // 2 + args.check_rows))
        band = hits[rows[0]:rows[1]].cpu().numpy().view(pkg.HIT_DTYPE).reshape(-1, w)
        obj = hits[..., 1]
        share = {"cube": float(((obj >= 0) & (obj < args.cubes)).float().mean()),
                 "sphere": float((obj >= args.cubes).float().mean()),
                 "miss": float((obj < 0).float().mean())}
        for what, nbytes in OUT_BYTES.items():
            got = outs[what].view(h, w, nbytes // 4)[rows[0]:rows[1]].cpu().numpy()
            want = (pkg.hit_surfaces(band, scene, rows=rows, ray_dir=d) if what == "surface"
                    else pkg.light_hits(band, scene, what, rows=rows, ray_dir=d))
            want = np.ascontiguousarray(want).view(np.int32).reshape(got.shape)
            if not np.array_equal(got, want):
                raise SystemExit(f"{what}: rows {rows} differ from the host function")
        times = {name: [] for name in kernels}
        for _ in range(args.rounds):
            for name, fn in kernels.items():
                times[name] += timed(fn, args.launches)
        kernel = rt.last_kernel()

    px = w * h
    result = {"frame": [w, h], "spheres": args.spheres, "cubes": args.cubes, "seed": args.seed,
              "k": k, "lights": args.lights, "pixel_share": share, "trace_kernel": kernel,
              "launches": args.rounds * args.launches, "rate_tbps": args.rate, "us": {}}
    for name, ts in times.items():
        q = statistics.quantiles(ts, n=4)
        entry = {"median": round(statistics.median(ts), 2), "q1": round(q[0], 2),
                 "q3": round(q[2], 2), "min": round(min(ts), 2)}
        if name in OUT_BYTES:
            nbytes = px * (8 + OUT_BYTES[name])
            entry["store_us"] = round(nbytes / (args.rate * 1e12) * 1e6, 2)
            entry["tbps"] = round(nbytes / (entry["median"] * 1e-6) / 1e12, 3)
        result["us"][name] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
