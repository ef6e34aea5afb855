"""What DeepCache sampling (x_info["cache_interval"] / ["cache_depth"]) costs and buys at the bench geometry (t2i: 512x512 =
64x64x4 latent, batch 4, guided 7.5, 50 DDIM steps, bench.build_model's full-width random-init UNet), in one process.

    python tools/probes/deepcache_step_time.py [--steps 50] [--reps 3] [--intervals 2,3,5] [--depths 1,2,3]

Every configuration has a sampler of its own, warmed by one call that captures its step graphs and one that only replays them.
Then, per repetition and per (interval, depth), one uncached call and one cached call alternate; ms per call is the wall time of
a whole sample() call between two device synchronisations, so the per-call host work (tables, context K/V refresh) is in every
number alike.  ms per full / shallow step is measured on the kept graphs themselves: `--replays` back-to-back replays of the
step graph between two events (the full step of a cached call = forward + store + update).  Prints one JSON line: the uncached
call's values with their median and spread (max - min) over its repeats, per configuration the medians and the ratio of the
cached to the uncached ms per call, and the box calibration."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "versatile-diffusion_amd")]
os.environ.setdefault("VD_QUIET", "1")

import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--intervals", default="2,3,5")
    ap.add_argument("--depths", default="1,2,3")
    args = ap.parse_args()
    from lib.model_zoo.ddim import DDIMSampler
    device = torch.device("cuda:0")
    wl = bench.WORKLOADS["t2i"]
    B = wl["batch"]
    net = bench.build_model(device)
    ctx = bench.make_contexts(wl, B, device, 1)[0]
    shape = [B, 4, wl["side"], wl["side"]]
    xT = torch.randn(shape, generator=torch.Generator().manual_seed(3)).half().to(device)
    configs = [(n, k) for n in (int(v) for v in args.intervals.split(",")) for k in (int(v) for v in args.depths.split(","))]
    samplers = {cfg: DDIMSampler(net) for cfg in [None] + configs}

    def call(cfg):
        keys = {} if cfg is None else {"cache_interval": cfg[0], "cache_depth": cfg[1]}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        samplers[cfg].sample(steps=args.steps, shape=shape, x_info=dict({"type": "image", "xt": xT}, **keys), c_info=dict(ctx),
                             verbose=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def replay_ms(graph):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.replays):
            graph.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.replays

    for cfg in samplers:           # capture, then one call that only replays
        call(cfg)
        call(cfg)
    state = lambda cfg: next(iter(samplers[cfg]._static.values()))
    ms = {cfg: [] for cfg in samplers}
    full, shallow, plain_step = {cfg: [] for cfg in configs}, {cfg: [] for cfg in configs}, []
    for _ in range(args.reps):
        for cfg in configs:
            ms[None].append(call(None))
            ms[cfg].append(call(cfg))
            full[cfg].append(replay_ms(state(cfg)["graph"]))
            shallow[cfg].append(replay_ms(state(cfg)["graph_shallow"]))
        plain_step.append(replay_ms(state(None)["graph"]))
    med = statistics.median
    base = med(ms[None])
    out = {"probe": "deepcache_step_time", "geometry": "t2i 512x512, batch %d, guided 7.5, %d DDIM steps" % (B, args.steps),
           "uncached": {"ms_per_call": [round(v, 2) for v in ms[None]], "median": round(base, 2),
                        "spread": round(max(ms[None]) - min(ms[None]), 2), "ms_per_step_graph": round(med(plain_step), 3)},
           "cached": []}
    for cfg in configs:
        out["cached"].append({"interval": cfg[0], "depth": cfg[1], "ms_per_call": round(med(ms[cfg]), 2),
                              "ratio_to_uncached": round(med(ms[cfg]) / base, 4), "ms_per_full_step": round(med(full[cfg]), 3),
                              "ms_per_shallow_step": round(med(shallow[cfg]), 3),
                              "kept_bytes": state(cfg)["deep"].buf.numel() * 2})
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
