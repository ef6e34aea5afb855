"""What a windowed (MultiDiffusion) step costs at full width (bench.build_model's random-init UNet, guided 7.5, DDIM), in one
process: B = 1 on a 64x128 canvas in windows of 64 at stride 32 (3 windows, one forward of 3 slots) against (a) the plain call
on a 64x64 latent at batch 3 -- the same UNet batch without the two window kernels -- and (b) the plain call on the 64x128 latent
itself, whose self-attention sees the whole canvas.

    python tools/probes/window_step_time.py [--steps 10] [--reps 3] [--replays 20]

Every configuration has a sampler of its own, warmed by one call that captures its step graph and one that only replays it.
Then, per repetition, the three configurations alternate: ms per call is the wall time of a whole sample() call between two
device synchronisations, ms per step is `--replays` back-to-back replays of the kept step graph between two events.  Prints
one JSON line: per configuration the values with their median and spread (max - min), the differences of the windowed step to
(a) and (b), and the box calibration.  Run it under a time limit; the expectation to confirm or refute is that the windowed
step costs the batch-3 step plus two small launches per chunk."""
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replays", type=int, default=20)
    args = ap.parse_args()
    from lib.model_zoo.ddim import DDIMSampler
    device = torch.device("cuda:0")
    wl = bench.WORKLOADS["t2i"]
    net = bench.build_model(device)
    side = wl["side"]
    # name -> (latent shape, window keys)
    configs = {"windowed_64x128_w64_s32": ([1, 4, side, 2 * side], {"window": side, "window_stride": side // 2}),
               "plain_64x64_batch3": ([3, 4, side, side], {}),
               "plain_64x128": ([1, 4, side, 2 * side], {})}
    samplers = {name: DDIMSampler(net) for name in configs}
    inputs = {}
    for name, (shape, _) in configs.items():
        g = torch.Generator().manual_seed(3)
        inputs[name] = (torch.randn(shape, generator=g).half().to(device), bench.make_contexts(wl, shape[0], device, 1)[0])

    def call(name):
        shape, keys = configs[name]
        xT, ctx = inputs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        samplers[name].sample(steps=args.steps, shape=shape, x_info=dict({"type": "image", "xt": xT}, **keys), c_info=dict(ctx),
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

    for name in configs:           # capture, then one call that only replays
        call(name)
        call(name)
    state = lambda name: next(iter(samplers[name]._static.values()))
    wplan = state("windowed_64x128_w64_s32")["window"]["plan"]
    per_call, per_step = {n: [] for n in configs}, {n: [] for n in configs}
    for _ in range(args.reps):
        for name in configs:
            per_call[name].append(call(name))
            per_step[name].append(replay_ms(state(name)["graph"]))
    med = statistics.median
    spread = lambda v: max(v) - min(v)
    out = {"probe": "window_step_time", "geometry": "guided 7.5, %d DDIM steps, full-width UNet" % args.steps,
           "windows": {"n": wplan["n"], "forwards_per_step": wplan["nc"], "slots": wplan["m"]}, "configs": {}}
    for name in configs:
        out["configs"][name] = {"ms_per_step": [round(v, 3) for v in per_step[name]], "ms_per_step_median": round(med(per_step[name]), 3),
                                "ms_per_step_spread": round(spread(per_step[name]), 3),
                                "ms_per_call_median": round(med(per_call[name]), 2), "ms_per_call_spread": round(spread(per_call[name]), 2)}
    w = med(per_step["windowed_64x128_w64_s32"])
    out["windowed_minus_batch3_ms_per_step"] = round(w - med(per_step["plain_64x64_batch3"]), 3)
    out["windowed_over_plain_canvas"] = round(w / med(per_step["plain_64x128"]), 4)
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
