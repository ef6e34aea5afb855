"""ms per replayed step of UniPCSampler (order 2 with the corrector) and DPMSolverSampler (2M) in one process, bench geometry
(t2i: 512x512 = 64x64x4 latent, batch 4, guided 7.5, bench.build_model's full-width random-init UNet).

    python tools/probes/unipc_step_time.py [--steps 20] [--reps 7] [--order 2]

Each repetition is one whole sample() call on the kept step graph (every step replayed), the two samplers alternating;
ms/step = wall time of the call / steps, so the per-call host work (tables, context K/V refresh) is in both numbers alike.
The two steps differ in their last launch alone: the UniPC update reads and rewrites four fp32 state buffers where 2M has
one.  Prints one JSON line: per sampler the per-repetition values, their median and spread (max - min), the difference of
the medians, and the box calibration."""
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--order", type=int, default=2)
    args = ap.parse_args()
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    from lib.model_zoo.unipc import UniPCSampler
    device = torch.device("cuda:0")
    wl = bench.WORKLOADS["t2i"]
    B = wl["batch"]
    net = bench.build_model(device)
    ctx = bench.make_contexts(wl, B, device, 1)[0]
    shape = [B, 4, wl["side"], wl["side"]]
    xT = torch.randn(shape, generator=torch.Generator().manual_seed(3)).half().to(device)
    samplers = {"unipc": UniPCSampler(net, order=args.order), "dpmpp_2m": DPMSolverSampler(net)}

    def call(name, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        samplers[name].sample(steps=steps, shape=shape, x_info={"type": "image", "xt": xT}, c_info=dict(ctx), verbose=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for name in samplers:          # capture (a step count that divides the 1000 training steps), then one call that only replays
        call(name, 4)
        call(name, args.steps)
    ms = {name: [] for name in samplers}
    for _ in range(args.reps):
        for name in samplers:
            ms[name].append(call(name, args.steps))
    out = {"probe": "unipc_step_time", "geometry": "t2i 512x512, batch %d, guided 7.5" % B, "steps": args.steps,
           "order": args.order}
    for name, v in ms.items():
        out[name] = {"ms_per_step": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                     "spread": round(max(v) - min(v), 3)}
    out["unipc_minus_2m_median_ms"] = round(out["unipc"]["median"] - out["dpmpp_2m"]["median"], 3)
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
