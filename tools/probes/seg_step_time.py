"""ms per replayed DPMSolverSampler (2M) step with smoothed energy guidance (seg_scale 3.0, the middle context block) at sigma =
infinity (the mean query) and at a finite sigma (1.0: 7 taps), with perturbed-attention guidance (pag_scale 3.0, the same block) and
with neither, in one process, on bench.build_model's full-width random-init UNet at pag_step_time.py's two geometries: the guided
bench geometry (t2i: 512x512 = 64x64x4 latent, batch 4, guidance 7.5: two replicas become three) and the unguided image-variation
geometry (i2v: the CLIP image context of 257 tokens, batch 8, guidance scale 1: one replica becomes two).

    python tools/probes/seg_step_time.py [--steps 50] [--reps 5]

Each repetition is one whole sample() call on the kept step graph (every step replayed), the four settings alternating, each on a
sampler of its own per geometry (a sampler keeps two graphs); ms/step = wall time of the call / steps, so the per-call host work
(tables, context K/V refresh) is in all numbers alike.  The call without the keys launches what the sampler launched before the
feature existed.  SEG runs PAG's row count, so one expects PAG's cost plus, per chosen layer, the blur launch and a softmax
attention instead of a copy.  The blur launch alone is timed too: ops.attention(blur_from=0, ...) minus ops.attention on the same
operands (both are the same vd_attention_f16 call behind the blur), median of --reps rounds of 200 calls between two events, at the
middle block's shape (8 x 8 tokens x 1280, the batch of one replica) and at a 64 x 64 x 320 layer, R = 3 and the mean.  Prints one
JSON line: per geometry and setting the per-repetition values, their median and spread (max - min), the ratios of the medians, the
blur timings, and the box calibration."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "versatile-diffusion_amd")]
os.environ.setdefault("VD_QUIET", "1")

import torch  # noqa: E402

import bench  # noqa: E402

SCALE = 3.0
FINITE_SIGMA = 1.0
GEOMETRIES = [("t2i_guided", "t2i", 7.5), ("i2v_unguided", "i2v", 1.0)]
SETTINGS = {"off": {}, "pag": {"pag_scale": SCALE}, "seg_inf": {"seg_scale": SCALE, "seg_blur_sigma": math.inf},
            "seg_finite": {"seg_scale": SCALE, "seg_blur_sigma": FINITE_SIGMA}}
BLUR_SHAPES = [("mid_8x8x1280", 8, 8, 8, 160, 4), ("level0_64x64x320", 64, 64, 8, 40, 4)]


def blur_alone(device, reps, calls=200):
    from lib.model_zoo.vd import seg_taps
    from vd_hip import ops
    out = {}
    R, w = seg_taps(FINITE_SIGMA)
    taps = torch.from_numpy(w).to(device)
    for label, gh, gw, heads, D, B in BLUR_SHAPES:
        C = heads * D
        qkv = torch.randn((B, gh * gw, 3 * C), generator=torch.Generator().manual_seed(1)).half().to(device)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        dst = torch.empty((B, gh * gw, C), dtype=torch.float16, device=device)
        qb = torch.empty((B * gh * gw * C,), dtype=torch.float16, device=device)
        variants = {"plain": {}, "R%d" % R: dict(blur_from=0, blur=(taps, R, gh, gw), qb=qb), "mean": dict(blur_from=0, blur=(None, -1, gh, gw), qb=qb)}
        us = {name: [] for name in variants}
        for _ in range(reps + 1):      # (the first round warms up)
            for name, kw in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    ops.attention(q, k, v, heads, out=dst, **kw)
                b.record()
                b.synchronize()
                us[name].append(a.elapsed_time(b) * 1e3 / calls)
        med = {name: statistics.median(v[1:]) for name, v in us.items()}
        out[label] = {"batch": B, "us_per_call": {name: round(m, 2) for name, m in med.items()},
                      "blur_launch_us": {name: round(med[name] - med["plain"], 2) for name in med if name != "plain"}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    device = torch.device("cuda:0")
    net = bench.build_model(device)
    out = {"probe": "seg_step_time", "steps": args.steps, "scale": SCALE, "layers": "mid", "finite_sigma": FINITE_SIGMA,
           "sampler": "DPM-Solver++(2M)"}
    for label, workload, scale in GEOMETRIES:
        wl = bench.WORKLOADS[workload]
        B = wl["batch"]
        ctx = dict(bench.make_contexts(wl, B, device, 1)[0], unconditional_guidance_scale=scale)
        shape = [B, 4, wl["side"], wl["side"]]
        xT = torch.randn(shape, generator=torch.Generator().manual_seed(3)).half().to(device)
        samplers = {name: DPMSolverSampler(net) for name in SETTINGS}

        def call(name, steps):
            x_info = dict({"type": "image", "xt": xT}, **SETTINGS[name])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            samplers[name].sample(steps=steps, shape=shape, x_info=x_info, c_info=dict(ctx), verbose=False)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps

        for name in SETTINGS:      # capture (a step count that divides the 1000 training steps), then one call that only replays
            call(name, 4)
            call(name, args.steps)
        ms = {name: [] for name in SETTINGS}
        for _ in range(args.reps):
            for name in SETTINGS:
                ms[name].append(call(name, args.steps))
        geo = {"geometry": "%s 512x512, batch %d, guidance scale %.1f, context %s x %d" % (workload, B, scale, wl["ctxs"][0][0], wl["ctxs"][0][1]),
               "replicas": {"off": 2 if scale != 1.0 else 1, "perturbed": 3 if scale != 1.0 else 2}}
        for name, v in ms.items():
            geo[name] = {"ms_per_step": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                         "spread": round(max(v) - min(v), 3)}
        for name in SETTINGS:
            if name != "off":
                geo[name + "_over_off"] = round(geo[name]["median"] / geo["off"]["median"], 4)
        geo["seg_inf_over_pag"] = round(geo["seg_inf"]["median"] / geo["pag"]["median"], 4)
        geo["seg_finite_over_pag"] = round(geo["seg_finite"]["median"] / geo["pag"]["median"], 4)
        out[label] = geo
        for s in samplers.values():
            s.release_graphs()
        torch.cuda.empty_cache()
    out["blur_alone"] = blur_alone(device, args.reps)
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
