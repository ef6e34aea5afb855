"""ms per replayed DPMSolverSampler (2M) step with the guidance rescale (phi = 0.7) and without it (phi = 0) in one process,
bench geometry (t2i: 512x512 = 64x64x4 latent, batch 4, guided 7.5, bench.build_model's full-width random-init UNet), and
the factor kernel's own time at that geometry.

    python tools/probes/rescale_step_time.py [--steps 50] [--reps 7]

Each repetition is one whole sample() call on the kept step graph (every step replayed), the two settings alternating on
ONE sampler (they keep one graph each); ms/step = wall time of the call / steps, so the per-call host work (tables, context
K/V refresh) is in both numbers alike.  phi = 0 launches what the sampler launched before the rescale existed.  The factor
kernel alone: device events around 200 back-to-back launches on the [e_u ; e_c] of that geometry, after a warm-up.
Prints one JSON line: per setting the per-repetition values, their median and spread (max - min), the difference of the
medians, the kernel's microseconds per launch and the box calibration."""
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


def factor_kernel_us(device, shape, launches=200):
    from vd_hip import ops
    B, per = shape[0], 1
    for s in shape[1:]:
        per *= s
    eps = torch.randn((2 * B * per,), generator=torch.Generator().manual_seed(5)).half().to(device)
    coef = torch.tensor([7.5], dtype=torch.float32, device=device)
    phi = torch.tensor([0.7], dtype=torch.float32, device=device)
    out = torch.empty((B,), dtype=torch.float32, device=device)
    for _ in range(20):
        ops.cfg_rescale_factor(eps, coef, phi, per, out=out)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        ops.cfg_rescale_factor(eps, coef, phi, per, out=out)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / launches


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
    settings = {"phi_0": 0.0, "phi_0.7": 0.7}

    def call(name, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sampler.sample(steps=steps, shape=shape, x_info={"type": "image", "xt": xT},
                       c_info=dict(ctx, guidance_rescale=settings[name]), verbose=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for name in settings:          # capture (a step count that divides the 1000 training steps), then one call that only replays
        call(name, 4)
        call(name, args.steps)
    ms = {name: [] for name in settings}
    for _ in range(args.reps):
        for name in settings:
            ms[name].append(call(name, args.steps))
    out = {"probe": "rescale_step_time", "geometry": "t2i 512x512, batch %d, guided 7.5, DPM-Solver++(2M)" % B,
           "steps": args.steps}
    for name, v in ms.items():
        out[name] = {"ms_per_step": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                     "spread": round(max(v) - min(v), 3)}
    out["rescale_minus_plain_median_ms"] = round(out["phi_0.7"]["median"] - out["phi_0"]["median"], 3)
    out["factor_kernel_us"] = round(factor_kernel_us(device, shape), 2)
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
