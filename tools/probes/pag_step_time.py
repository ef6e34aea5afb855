"""ms per replayed DPMSolverSampler (2M) step with perturbed-attention guidance (pag_scale 3.0, the middle context block) and
without it in one process, on bench.build_model's full-width random-init UNet at two geometries: the guided bench geometry (t2i:
512x512 = 64x64x4 latent, batch 4, guidance 7.5: two replicas become three) and the unguided image-variation geometry (i2v: the
CLIP image context of 257 tokens, batch 8, guidance scale 1: one replica becomes two).

    python tools/probes/pag_step_time.py [--steps 50] [--reps 5]

Each repetition is one whole sample() call on the kept step graph (every step replayed), the two settings alternating on ONE
sampler per geometry (they keep one graph each); ms/step = wall time of the call / steps, so the per-call host work (tables,
context K/V refresh) is in both numbers alike.  The call without the keys launches what the sampler launched before the feature
existed.  From the row counts one expects about 3/2 and 2/1 (the perturbed replica is a whole forward; the identity attention of one
block and the fold are small beside it; with the key the first context block also runs its entry per replica instead of once per
sample).  Prints one JSON line: per geometry and setting the per-repetition values, their median and spread (max - min), the ratio
of the medians, and the box calibration."""
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

PAG_SCALE = 3.0
GEOMETRIES = [("t2i_guided", "t2i", 7.5), ("i2v_unguided", "i2v", 1.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    device = torch.device("cuda:0")
    net = bench.build_model(device)
    out = {"probe": "pag_step_time", "steps": args.steps, "pag_scale": PAG_SCALE, "pag_layers": "mid", "sampler": "DPM-Solver++(2M)"}
    for label, workload, scale in GEOMETRIES:
        wl = bench.WORKLOADS[workload]
        B = wl["batch"]
        ctx = dict(bench.make_contexts(wl, B, device, 1)[0], unconditional_guidance_scale=scale)
        shape = [B, 4, wl["side"], wl["side"]]
        xT = torch.randn(shape, generator=torch.Generator().manual_seed(3)).half().to(device)
        sampler = DPMSolverSampler(net)
        settings = {"off": {}, "pag": {"pag_scale": PAG_SCALE}}

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
        geo = {"geometry": "%s 512x512, batch %d, guidance scale %.1f, context %s x %d" % (workload, B, scale, wl["ctxs"][0][0], wl["ctxs"][0][1]),
               "replicas": {"off": 2 if scale != 1.0 else 1, "pag": 3 if scale != 1.0 else 2}}
        for name, v in ms.items():
            geo[name] = {"ms_per_step": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                         "spread": round(max(v) - min(v), 3)}
        geo["pag_over_off"] = round(geo["pag"]["median"] / geo["off"]["median"], 4)
        out[label] = geo
        sampler.release_graphs()
        torch.cuda.empty_cache()
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
