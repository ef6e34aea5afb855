"""ms per replayed DPMSolverSampler (2M) step with FreeU (b1, b2, s1, s2) = (1.2, 1.4, 0.9, 0.2) and without it in one process,
bench geometry (t2i: 512x512 = 64x64x4 latent, batch 4, guided 7.5, bench.build_model's full-width random-init UNet), and the
FreeU kernel's own time at each of the ten skip loads it acts on at that geometry.

    python tools/probes/freeu_step_time.py [--steps 50] [--reps 7]

Each repetition is one whole sample() call on the kept step graph (every step replayed), the two settings alternating on ONE
sampler (they keep one graph each); ms/step = wall time of the call / steps, so the per-call host work (tables, context K/V
refresh) is in both numbers alike.  The call without the key launches what the sampler launched before FreeU existed.  The
kernel alone: per load geometry (8 rows = the guided batch) 50 launches captured into a graph, device events around 4 replays.
With FreeU a step also pays for what the copies lose: the GroupNorm behind each of the ten loads measures its input instead of
reading producer statistics.  Prints one JSON line: per setting the per-repetition values, their median and spread (max - min),
the difference of the medians, the kernel's microseconds per launch and geometry, their sum, and the box calibration."""
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

SETTING = (1.2, 1.4, 0.9, 0.2)
# (H = W, C0, C1, b, s) of output blocks 0 .. 9 at a 64 x 64 latent, width 320, multipliers (1, 2, 4, 4)
LOADS = [(8, 1280, 1280, 1.2, 0.9)] * 3 + [(16, 1280, 1280, 1.2, 0.9)] * 2 + [(16, 1280, 640, 1.2, 0.9), (32, 1280, 640, 1.2, 0.9),
                                                                              (32, 640, 640, 1.4, 0.2), (32, 640, 320, 1.4, 0.2),
                                                                              (64, 640, 320, 1.4, 0.2)]


def kernel_us(device, rows, launches=200):
    from vd_hip import ops
    out = {}
    for side, c0, c1, b, s in sorted(set(LOADS)):
        g = torch.Generator().manual_seed(side + c0 + c1)
        h = torch.randn((rows, side, side, c0), generator=g).half().to(device)
        x = torch.randn((rows, side, side, c1), generator=g).half().to(device)
        for _ in range(20):
            ops.freeu(h, x, b, s)
        # the launches replayed from a graph: an eager loop would time the wrapper's host work (two allocations, a ctypes call)
        graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                for _ in range(launches // 4):
                    ops.freeu(h, x, b, s)
        torch.cuda.current_stream().wait_stream(stream)
        graph.replay()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(4):
            graph.replay()
        stop.record()
        torch.cuda.synchronize()
        out["%dx%d_C0_%d_C1_%d" % (side, side, c0, c1)] = round(start.elapsed_time(stop) * 1e3 / (4 * (launches // 4)), 2)
    total = sum(out["%dx%d_C0_%d_C1_%d" % (side, side, c0, c1)] for side, c0, c1, _, _ in LOADS)
    return out, round(total, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    device = torch.device("cuda:0")
    wl = bench.WORKLOADS["t2i"]
    B = wl["batch"]
    net = bench.build_model(device)
    ctx = bench.make_contexts(wl, B, device, 1)[0]
    shape = [B, 4, wl["side"], wl["side"]]
    xT = torch.randn(shape, generator=torch.Generator().manual_seed(3)).half().to(device)
    sampler = DPMSolverSampler(net)
    settings = {"off": None, "freeu": SETTING}

    def call(name, steps):
        x_info = {"type": "image", "xt": xT}
        if settings[name] is not None:
            x_info["freeu"] = settings[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sampler.sample(steps=steps, shape=shape, x_info=x_info, c_info=dict(ctx), verbose=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for name in settings:          # capture (a step count that divides the 1000 training steps), then one call that only replays
        call(name, 4)
        call(name, args.steps)
    ms = {name: [] for name in settings}
    for _ in range(args.reps):
        for name in settings:
            ms[name].append(call(name, args.steps))
    out = {"probe": "freeu_step_time", "geometry": "t2i 512x512, batch %d, guided 7.5, DPM-Solver++(2M)" % B, "steps": args.steps,
           "setting": list(SETTING)}
    for name, v in ms.items():
        out[name] = {"ms_per_step": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                     "spread": round(max(v) - min(v), 3)}
    out["freeu_minus_off_median_ms"] = round(out["freeu"]["median"] - out["off"]["median"], 3)
    out["kernel_us_per_launch"], out["kernel_us_per_step"] = kernel_us(device, 2 * B)
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
