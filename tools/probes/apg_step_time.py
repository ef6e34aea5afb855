"""ms per replayed DPMSolverSampler (2M) step with adaptive projected guidance (eta 0, norm threshold 2.5, momentum -0.5) and without
it in ONE process, on bench.build_model's full-width random-init UNet, guided 7.5, at two geometries: the bench geometry (t2i:
512x512 = 64x64x4 latent, batch 4) and a 64x256 canvas (B = 1) in windows of 64 at stride 32; and the fold's own time per launch at
both.

    python tools/probes/apg_step_time.py [--steps 50] [--reps 5]

Each repetition is one whole sample() call on the kept step graph (every step replayed), the two settings alternating on ONE
sampler per geometry (they keep one graph each); ms/step = wall time of the call / steps, so the per-call host work (tables,
context K/V refresh) is in both numbers alike.  The call without the keys launches what the sampler launched before the feature
existed.  The fold alone: device events around 200 back-to-back launches on operands of that geometry, after a warm-up.  The
expectation to confirm or refute: one small launch per step (the guidance rescale's factor kernel is the comparable), on the canvas
as on the plain latent -- the fold sees the canvas prediction, not the windows.  Prints one JSON line: per geometry and setting the
per-repetition values, their median and spread (max - min), the difference of the medians, the fold's microseconds per launch, and
the box calibration."""
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

APG = {"apg_eta": 0.0, "apg_norm_threshold": 2.5, "apg_momentum": -0.5}


def fold_us(device, shape, launches=200):
    from vd_hip import ops
    g = torch.Generator().manual_seed(5)
    per = int(np.prod(shape[1:]))
    x = torch.randn(shape, generator=g).half().to(device)
    eps = torch.randn([2 * shape[0]] + list(shape[1:]), generator=g).half().to(device)
    v = torch.zeros(shape, dtype=torch.float32, device=device)
    s1, isa = np.sqrt(1.0 - 0.35), 1.0 / np.sqrt(0.35)
    coef = torch.tensor([s1, isa, 1.0 / (s1 * isa), -0.5, 2.5, 1.0, 0.0, 0.0], dtype=torch.float32, device=device)
    fac = torch.empty((shape[0], 4), dtype=torch.float32, device=device)
    for _ in range(20):
        ops.apg_fold(x, eps, v, coef, per, out_fac=fac)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        ops.apg_fold(x, eps, v, coef, per, out_fac=fac)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    device = torch.device("cuda:0")
    wl = bench.WORKLOADS["t2i"]
    side = wl["side"]
    net = bench.build_model(device)
    out = {"probe": "apg_step_time", "steps": args.steps, "setting": APG, "sampler": "DPM-Solver++(2M)", "guidance_scale": 7.5}
    # name -> (latent shape, window keys)
    geometries = {"bench_64x64_batch%d" % wl["batch"]: ([wl["batch"], 4, side, side], {}),
                  "canvas_64x256_w64_s32": ([1, 4, side, 4 * side], {"window": side, "window_stride": side // 2})}
    for label, (shape, wkeys) in geometries.items():
        ctx = dict(bench.make_contexts(wl, shape[0], device, 1)[0], unconditional_guidance_scale=7.5)
        xT = torch.randn(shape, generator=torch.Generator().manual_seed(3)).half().to(device)
        sampler = DPMSolverSampler(net)
        settings = {"off": dict(wkeys), "apg": dict(wkeys, **APG)}

        def call(name, steps):
            x_info = dict({"type": "image", "xt": xT}, **settings[name])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sampler.sample(steps=steps, shape=shape, x_info=x_info, c_info=dict(ctx), verbose=False)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps

        for name in settings:      # capture (a step count that divides the 1000 training steps), then one call that only replays
            call(name, 4)
            call(name, args.steps)
        ms = {name: [] for name in settings}
        for _ in range(args.reps):
            for name in settings:
                ms[name].append(call(name, args.steps))
        geo = {"shape": shape, "window_keys": wkeys}
        for name, v in ms.items():
            geo[name] = {"ms_per_step": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                         "spread": round(max(v) - min(v), 3)}
        geo["apg_minus_off_median_ms"] = round(geo["apg"]["median"] - geo["off"]["median"], 3)
        geo["fold_us"] = round(fold_us(device, shape), 2)
        out[label] = geo
        sampler.release_graphs()
        torch.cuda.empty_cache()
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
