"""What a regional-prompt step costs at full width (bench.build_model's random-init UNet, guided 7.5, DDIM), in one process:
B = 1 on a 64x128 canvas in windows of 64 at stride 32 (3 windows, one forward of 3 slots) with R = 1, 2 and 3 regions (vertical
stripes of the canvas, one conditioning each) against the windowed call without regions.

    python tools/probes/region_step_time.py [--steps 10] [--reps 3] [--replays 20]

Every configuration has a sampler of its own, warmed by one call that captures its step graph and one that only replays it.
Then, per repetition, the configurations alternate: ms per call is the wall time of a whole sample() call between two device
synchronisations, ms per step is `--replays` back-to-back replays of the kept step graph between two events.  Prints one JSON
line: per configuration the values with their median and spread (max - min), the step of R regions over and minus R times the
windowed step, and the box calibration.  Run it under a time limit; the expectation to confirm or refute is that a step of R
regions costs R times the windowed step's forward plus R x nc merge launches."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "versatile-diffusion_amd")]
os.environ.setdefault("VD_QUIET", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def stripes(R, H, W):
    """fp32 [R, H, W]: R vertical stripes of (nearly) equal width, hard and complementary."""
    m = np.zeros((R, H, W), dtype=np.float32)
    edges = [round(r * W / R) for r in range(R + 1)]
    for r in range(R):
        m[r, :, edges[r]:edges[r + 1]] = 1.0
    return m


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
    shape = [1, 4, side, 2 * side]
    keys = {"window": side, "window_stride": side // 2}
    xT = torch.randn(shape, generator=torch.Generator().manual_seed(3)).half().to(device)
    ctx = bench.make_contexts(wl, 1, device, 1)[0]
    configs = {"windowed": (keys, dict(ctx))}         # name -> (x_info keys, c_info)
    for R in (1, 2, 3):
        conds = [ctx["conditioning"].roll(r, 1).contiguous() for r in range(R)]
        configs["regions_%d" % R] = (dict(keys, region_masks=stripes(R, side, 2 * side)), dict(ctx, conditioning=conds))
    samplers = {name: DDIMSampler(net) for name in configs}

    def call(name):
        x_keys, c_info = configs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        samplers[name].sample(steps=args.steps, shape=shape, x_info=dict({"type": "image", "xt": xT}, **x_keys),
                              c_info=dict(c_info), verbose=False)
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
    wplan = state("windowed")["window"]["plan"]
    per_call, per_step = {n: [] for n in configs}, {n: [] for n in configs}
    for _ in range(args.reps):
        for name in configs:
            per_call[name].append(call(name))
            per_step[name].append(replay_ms(state(name)["graph"]))
    med = statistics.median
    spread = lambda v: max(v) - min(v)
    out = {"probe": "region_step_time", "geometry": "guided 7.5, %d DDIM steps, full-width UNet, B = 1, canvas %dx%d" % (
        args.steps, side, 2 * side), "windows": {"n": wplan["n"], "forwards_per_step": wplan["nc"], "slots": wplan["m"]},
        "configs": {}}
    for name in configs:
        out["configs"][name] = {"ms_per_step": [round(v, 3) for v in per_step[name]], "ms_per_step_median": round(med(per_step[name]), 3),
                                "ms_per_step_spread": round(spread(per_step[name]), 3),
                                "ms_per_call_median": round(med(per_call[name]), 2), "ms_per_call_spread": round(spread(per_call[name]), 2)}
    w = med(per_step["windowed"])
    for R in (1, 2, 3):
        r = med(per_step["regions_%d" % R])
        out["regions_%d_over_windowed" % R] = round(r / w, 4)
        out["regions_%d_minus_R_windowed_ms_per_step" % R] = round(r - R * w, 3)
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
