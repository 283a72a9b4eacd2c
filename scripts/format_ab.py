"""Interleaved per-format measurement in one process: wall us per frame and
per-kernel us (rt_profile_*) of hit / i32x4 / rgba8 frames, each on both
trace paths (trace_bin 1 = trace_bin_kernel, 2 = coarse + trace3_kernel).

    python scripts/format_ab.py --config c3 --formats hit,i32x4,rgba8 --rounds 9
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
CONFIGS = {
    "c3": (4096, 4096, 256, 64, 3, 6.4),
    "c4": (8192, 8192, 192, 64, 4, 12.8),
    # config 3's scene at other object sizes (box overdraw ~0.3 .. ~6)
    "c3r2": (4096, 4096, 256, 64, 3, 2.0),
    "c3r3": (4096, 4096, 256, 64, 3, 3.2),
    "c3r45": (4096, 4096, 256, 64, 3, 4.5),
    "c3r8": (4096, 4096, 256, 64, 3, 8.0),
    "c3k15": (4096, 4096, 256, 64, 3, 9.6),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--formats", default="hit,i32x4,rgba8")
    ap.add_argument("--modes", default="1,2")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--tag", default="")
    ap.add_argument("--inflight", type=int, default=1,
                    help="frames in flight: that many contexts, streams and frames, round-robin "
                         "(wall time only: per-kernel events would serialise them)")
    args = ap.parse_args()
    import torch
    import __graft_entry__

    pkg = __graft_entry__.load_package()
    dev = torch.device("cuda:0")
    n_slots = max(1, args.inflight)
    streams = [torch.cuda.Stream(dev) for _ in range(n_slots)]
    rts = [pkg.RayTracer(0) for _ in range(n_slots)]
    rt = rts[0]
    w, h, ns, nc, seed, k = CONFIGS[args.config]
    scene = pkg.Scene.synthetic(w, h, ns, nc, seed=seed, k=k)
    t = {n: torch.from_numpy(np.ascontiguousarray(getattr(scene, n))).to(dev)
         for n in ("sphere_origins", "sphere_radius", "sphere_colours", "cube_vertices",
                   "cube_colours")}
    ds = {n: v.data_ptr() for n, v in t.items()}
    ds.update(num_spheres=ns, num_cubes=nc)
    fmts = args.formats.split(",")
    modes = [int(m) for m in args.modes.split(",")]
    words = {"hit": 2, "i32x4": 4, "rgba8": 1}
    outs = {f: [torch.empty((h, w, words[f]), dtype=torch.int32, device=dev)
                for _ in range(n_slots)] for f in fmts}
    binds = {f: [rts[i].bind_render_device(ds, w, h, (0, h), outs[f][i].data_ptr(), fmt=f,
                                           stream=streams[i].cuda_stream)
                 for i in range(n_slots)] for f in fmts}
    turn = [0]

    def make_step(f):
        def step():
            binds[f][turn[0] % n_slots]()
            turn[0] += 1
        return step
    steps = {f: make_step(f) for f in fmts}

    def set_mode(m):
        for r in rts:
            r.set_trace_bin(m)
    keys = [(f, m) for f in fmts for m in modes]
    kernels = {}
    for f, m in keys:
        set_mode(m)
        for _ in range(3 * n_slots):
            steps[f]()
        torch.cuda.synchronize()
        kernels[(f, m)] = rt.last_kernel()
    # the hit frame shades to the colour frames (bit-exact check of what is timed)
    if "hit" in fmts and "i32x4" in fmts and h <= 4096:
        hits = outs["hit"][0].cpu().numpy().view(pkg.HIT_DTYPE).reshape(h, w)
        shaded = pkg.shade_hits(hits, scene, "i32x4")
        assert np.array_equal(shaded, outs["i32x4"][0].cpu().numpy()), "hit frame != i32x4 frame"
    walls = {key: [] for key in keys}
    kern = {key: {"prep_ms": [], "bin_ms": [], "trace_ms": []} for key in keys}
    for _ in range(args.rounds):
        for f, m in keys:
            set_mode(m)
            for _ in range(n_slots):
                steps[f]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                steps[f]()
            torch.cuda.synchronize()
            walls[(f, m)].append((time.perf_counter() - t0) * 1e6 / args.steps)
            if n_slots > 1:
                continue
            rt.profile(True)
            for _ in range(args.steps):
                steps[f]()
            p = rt.profile_read()
            rt.profile(False)
            for key in kern[(f, m)]:
                kern[(f, m)][key].append(p[key] * 1e3 / max(p["renders"], 1))
    res = {"config": args.config, "tag": args.tag, "library": os.path.relpath(pkg.library_path(), REPO),
           "frame": f"{w}x{h}, {ns}+{nc}, seed {seed}, k {k}", "rounds": args.rounds,
           "steps": args.steps, "inflight": n_slots, "box_overdraw": round(rt.last_overdraw(), 3)}
    for f, m in keys:
        x = walls[(f, m)]
        res[f"{f}/{kernels[(f, m)]}"] = {
            "wall_us": round(statistics.median(x), 1), "wall_min": round(min(x), 1),
            "wall_max": round(max(x), 1),
            **{key.replace("_ms", "_us"): round(statistics.median(v), 1)
               for key, v in kern[(f, m)].items() if v}}
    print(json.dumps(res), flush=True)
    for r in rts:
        r.close()


if __name__ == "__main__":
    main()
