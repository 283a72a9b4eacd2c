"""Interleaved A/B of the frame stores' cache policy (rt_debug_set_store_policy)
in ONE process, inside the frames-in-flight loop bench.py times as `value`
(its inflight_step: a context, a stream and a frame buffer per slot).

    python scripts/store_policy_ab.py --policies default,large,auto --legs c3x2,c3x1
    RT_HIP_LIBRARY=.../librt_hip_sweep.so python scripts/store_policy_ab.py --policies 0,1,2,...

Policies are names (auto, default, large) or, on a library built with
profiles/store_policy/sweep.patch applied, the sweep's numbers:
0 default of the build, 1 nt, 2 sc0, 3 sc1, 4 sc0 sc1, 5 nt sc0, 6 nt sc1,
7 nt sc0 sc1, 8 plain.  Per leg and round every policy is set on every slot's
context, the loop re-ramped, and two windows timed the way bench.py times
them: K frames (--steps) and --long frames.  Every policy's frames must equal
the first policy's.  Prints one JSON line per leg: per policy the median, min
and max wall us per frame of both windows, and what the contexts reported
(rt_debug_last_store_policy).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

# leg: (width, height, spheres, cubes, seed, k, format, slots)
LEGS = {
    "c3x2": (4096, 4096, 256, 64, 3, 6.4, "i32x4", 2),   # bench.py's `value`
    "c3x1": (4096, 4096, 256, 64, 3, 6.4, "i32x4", 1),   # one stream, one buffer
    "c3sx2": (4096, 4096, 256, 64, 3, 1.0, "i32x4", 2),  # config 3 sparse
    "c3tx4": (4096, 4096, 256, 64, 3, 6.4, "rgba8", 4),  # the RGBA8 Texture leg
    "c4x1": (8192, 8192, 192, 64, 4, 12.8, "i32x4", 1),  # config 4
    "c5dx1": (16384, 16384, 4096, 0, 5, 25.6, "i32x4", 1),  # config 5 dense
    "c5sx1": (16384, 16384, 4096, 0, 5, 1.0, "i32x4", 1),   # config 5 sparse
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", default="default,large,auto")
    ap.add_argument("--legs", default="c3x2,c3x1,c3sx2,c3tx4,c4x1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--long", type=int, default=600)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import bench

    bargs = bench.parse([])
    c = bench.Ctx(bargs)
    pkg = bench.__graft_entry__.load_package()
    policies = [p if p in pkg.STORE_POLICIES else int(p) for p in args.policies.split(",")]
    for leg in args.legs.split(","):
        w, h, ns, nc, seed, k, fmt, slots = LEGS[leg]
        scene, ds = bench.device_scene(pkg, c, w, h, ns, nc, seed, k)
        step, frames, keep = bench.inflight_step(pkg, c, ds, w, h, fmt, "auto", slots)
        rts = keep[0]

        def use(policy):
            for rt in rts:
                rt.store_policy(policy)
            for _ in range(4 * slots):
                step()
            c.sync()

        ref, said = None, {}
        for p in policies:  # warm-up and parity
            use(p)
            said[str(p)] = sorted({rt.last_store_policy() for rt in rts}, key=str)
            got = [f.clone() for f in frames]
            if ref is None:
                ref = got
            elif not all(bool(c.torch.equal(a, b)) for a, b in zip(got, ref)):
                raise SystemExit(f"{leg}: policy {p}: frames differ from policy {policies[0]}")
        c.clock_ramp(step, bargs.warmup_ms)
        short = {str(p): [] for p in policies}
        long_ = {str(p): [] for p in policies}
        for r in range(args.rounds):
            for p in (policies if r % 2 == 0 else policies[::-1]):
                use(p)
                c.clock_ramp(step, 10.0)
                short[str(p)].append(c.timed(step, args.steps) * 1e3)
                if args.long:
                    long_[str(p)].append(c.timed(step, args.long) * 1e3)
        res = {"leg": leg, "frame": f"{w}x{h} {fmt}, {ns}+{nc}, seed {seed}, k {k}",
               "slots": slots, "kernel": rts[0].last_kernel(), "rounds": args.rounds,
               "steps": args.steps, "long": args.long, "reported": said}
        for p in policies:
            e = {"us": round(statistics.median(short[str(p)]), 2),
                 "min": round(min(short[str(p)]), 2), "max": round(max(short[str(p)]), 2)}
            if args.long:
                e.update(long_us=round(statistics.median(long_[str(p)]), 2),
                         long_min=round(min(long_[str(p)]), 2),
                         long_max=round(max(long_[str(p)]), 2))
            res[str(p)] = e
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        c.sync()
        for rt in rts:
            rt.close()
        if isinstance(keep[1], bench.HipStreams):
            keep[1].close()
        del frames, ds, step, keep, ref
        c.torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
