"""The culled light pass beside its unculled twins, in one
process: HIP-event time per launch, over one hit frame, on one stream, each
culled kernel interleaved with its twin round by round, of

  mask_1_light, mask_3_lights   rt_shadow_hits[_accel]_device
  bounce_1                      rt_bounce_hits[_accel]_device, bounce 1
  lit_depth1_r0.25              rt_light_hits_mirrored[_accel]_device at depth 1,
                                reflectivity 0.25 everywhere, shadows
  lit_depth{2,4,8}_r1           the same at depths 2, 4 and 8 with every object
                                a perfect mirror, shadows

Prints one JSON line.

    python scripts/light_accel_bench.py          # config 3, three lights

Before anything is timed every culled frame is compared with its twin word for
word over the whole frame, and the device-built records with the host's byte
for byte.  A pair is "faster" / "slower" where the quartile ranges of the two
kernels' launches do not overlap, else "equal".  The kept counts are
rt_accel_kept on a sample of the pass's rays: the level-1 bounce rays and each
light's shadow segments of the hit pixels.
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
    ap.add_argument("--launches", type=int, default=2, help="timed launches per kernel and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sample", type=int, default=8192, help="rays of each kept-count histogram")
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
    one_light = dict(ds, num_lights=1)
    slots = args.spheres + args.cubes
    dev = dict(device="cuda:0")
    refl = {"quarter": torch.full((slots,), REFLECTIVITY, dtype=torch.float32, **dev),
            "ones": torch.ones((slots,), dtype=torch.float32, **dev)}
    hits = torch.empty((h, w, 2), dtype=torch.int32, **dev)
    surf = torch.empty((h, w, 4), dtype=torch.float32, **dev)
    accel = torch.empty((max(args.cubes, 1), 80), dtype=torch.int32, **dev)  # 320 bytes each
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    d = pkg.primary_ray_dir()
    hp, a = hits.data_ptr(), accel.data_ptr()

    with pkg.RayTracer(0) as rt:
        with torch.cuda.stream(stream):
            rt.render_device(ds, w, h, (0, h), hp, ray_dir=d, fmt="hit", stream=st)
            rt.hit_surfaces_device(hp, ds, w, (0, h), surf.data_ptr(), ray_dir=d, stream=st)
            rt.build_accel_device(ds, a, stream=st)
        stream.synchronize()
        want = pkg.build_accel(scene)
        if accel.cpu().numpy().tobytes()[:want.nbytes] != want.tobytes():
            raise SystemExit("the device's records differ from the host's")

        # the sampled rays of the pass: level-1 bounces and each light's segments
        rng = np.random.default_rng(2)
        t = hits[..., 0].view(torch.float32)
        obj = hits[..., 1]
        xs = torch.arange(w, dtype=torch.float32, **dev)[None, :].expand(h, w)
        ys = torch.arange(h, dtype=torch.float32, **dev)[:, None].expand(h, w)
        dv = torch.tensor(np.asarray(d[:3], np.float32), **dev)
        p = torch.stack([xs + t * dv[0], ys + t * dv[1], t * dv[2]], -1)
        nrm = surf[..., :3]

        def sample(where, direction):
            idx = torch.nonzero(where.reshape(-1))[:, 0]
            pick = idx[torch.from_numpy(rng.choice(len(idx), min(args.sample, len(idx)),
                                                   False)).to("cuda:0")]
            rays = np.zeros(len(pick), pkg.RAY_DTYPE)
            po = p.reshape(-1, 3)[pick].cpu().numpy()
            di = direction.reshape(-1, 3)[pick].cpu().numpy()
            for c, f in enumerate(("ox", "oy", "oz")):
                rays[f] = po[:, c]
            for c, f in enumerate(("dx", "dy", "dz")):
                rays[f] = di[:, c]
            rays["skip"] = obj.reshape(-1)[pick].cpu().numpy()
            return rays, int(len(idx))

        def histogram(rays, segment):
            counts = pkg.accel_kept(rays, scene, want, segment)
            return {"mean": round(float(counts.mean()), 3),
                    "histogram": np.bincount(counts, minlength=1).tolist()}

        hit = obj >= 0
        s = (nrm * dv).sum(-1, keepdim=True)
        rays, n_bounce = sample(hit, dv - (s + s) * nrm)
        kept = {"bounce_1": histogram(rays, False)}
        n_segments = []
        for i in range(len(LIGHTS)):
            L = torch.tensor(scene.lights[i, :3], **dev) - p
            rays, n = sample(hit & ((nrm * L).sum(-1) > 0), L)
            kept[f"segments_light_{i}"] = histogram(rays, True)
            n_segments.append(n)
        del p, xs, ys, s, surf, nrm
        torch.cuda.synchronize()

        def frame(words):
            return {c: torch.full((h, w, words), 0x5A5A5A5A, dtype=torch.int32, **dev)
                    for c in ("culled", "unculled")}

        # pair -> (the two outputs, culled launch, unculled launch)
        pairs = {}
        for name, scene_dev in (("mask_1_light", one_light), ("mask_3_lights", ds)):
            out = frame(1)
            pairs[name] = (
                out,
                lambda out=out, sd=scene_dev: rt.shadow_hits_accel_device(
                    hp, sd, a, w, (0, h), out["culled"].data_ptr(), ray_dir=d, stream=st),
                lambda out=out, sd=scene_dev: rt.shadow_hits_device(
                    hp, sd, w, (0, h), out["unculled"].data_ptr(), ray_dir=d, stream=st))
        out = frame(2)
        pairs["bounce_1"] = (
            out,
            lambda out=out: rt.bounce_hits_accel_device(hp, ds, a, w, (0, h),
                                                        out["culled"].data_ptr(), 1, ray_dir=d,
                                                        stream=st),
            lambda out=out: rt.bounce_hits_device(hp, ds, w, (0, h), out["unculled"].data_ptr(), 1,
                                                  ray_dir=d, stream=st))
        for name, which, depth in [("lit_depth1_r0.25", "quarter", 1)] + \
                [(f"lit_depth{depth}_r1", "ones", depth) for depth in DEPTHS]:
            out = frame(4)
            r = refl[which].data_ptr()
            pairs[name] = (
                out,
                lambda out=out, r=r, depth=depth: rt.light_hits_mirrored_accel_device(
                    hp, ds, a, w, (0, h), out["culled"].data_ptr(), r, depth, ray_dir=d, stream=st,
                    fmt="i32x4", shadows=True),
                lambda out=out, r=r, depth=depth: rt.light_hits_mirrored_device(
                    hp, ds, w, (0, h), out["unculled"].data_ptr(), r, depth, ray_dir=d, stream=st,
                    fmt="i32x4", shadows=True))

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

        # one warm-up launch per kernel, and culled = unculled over the whole frame
        hits_before = hits.clone()
        for name, (out, culled, unculled) in pairs.items():
            timed(culled, 1)
            timed(unculled, 1)
            if not torch.equal(out["culled"], out["unculled"]):
                raise SystemExit(f"{name}: the culled frame differs from the unculled one")
            if bool((out["culled"] == 0x5A5A5A5A).all()):
                raise SystemExit(f"{name}: nothing was written")
        if not torch.equal(hits, hits_before):
            raise SystemExit("the hit frame changed")
        if accel.cpu().numpy().tobytes()[:want.nbytes] != want.tobytes():
            raise SystemExit("the records changed")
        shares = {"hit_pixels": float(hit.float().mean()),
                  "shadowed_by_light_0_of_hit_pixels": float(
                      ((pairs["mask_1_light"][0]["culled"][..., 0] & 1) != 0).float().sum()
                      / hit.float().sum()),
                  "bounce_1_hits_of_hit_pixels": float(
                      (pairs["bounce_1"][0]["culled"][..., 1] >= 0).float().sum()
                      / hit.float().sum())}
        times = {f"{name}/{c}": [] for name in pairs for c in ("culled", "unculled")}
        for _ in range(args.rounds):
            for name, (_, culled, unculled) in pairs.items():
                times[f"{name}/culled"] += timed(culled, args.launches)
                times[f"{name}/unculled"] += timed(unculled, args.launches)

    result = {"frame": [w, h], "spheres": args.spheres, "cubes": args.cubes, "seed": args.seed,
              "k": k, "lights": len(LIGHTS), "bounce_rays": n_bounce, "segments": n_segments,
              "rounds": args.rounds, "launches": args.rounds * args.launches, "shares": shares,
              "kept_of_cubes": kept, "us": {}, "pairs": {}}
    for name, ts in times.items():
        q = statistics.quantiles(ts, n=4)
        result["us"][name] = {"median": round(statistics.median(ts), 1), "q1": round(q[0], 1),
                              "q3": round(q[2], 1), "min": round(min(ts), 1),
                              "max": round(max(ts), 1)}
    for name in pairs:
        c, u = result["us"][f"{name}/culled"], result["us"][f"{name}/unculled"]
        verdict = "faster" if c["q3"] < u["q1"] else "slower" if c["q1"] > u["q3"] else "equal"
        result["pairs"][name] = {"verdict": verdict,
                                 "unculled_over_culled": round(u["median"] / c["median"], 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
