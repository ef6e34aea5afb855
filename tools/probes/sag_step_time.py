"""ms per replayed DPMSolverSampler (2M) step with self-attention guidance (sag_scale 0.75, sigma 1.0) and without it in one process,
on bench.build_model's full-width random-init UNet at two geometries: the guided bench geometry (t2i: 512x512 = 64x64x4 latent,
batch 4, guidance 7.5: a forward on two replicas is followed by one on a single replica) and the unguided image-variation geometry
(i2v: the CLIP image context of 257 tokens, batch 8, guidance scale 1: one replica twice), and the isolated time of each of the three
launches the step adds (ops.sag_mass at the middle block's shape, ops.sag_degrade and ops.sag_fold at the latent's).

    python tools/probes/sag_step_time.py [--steps 50] [--reps 5]

Each repetition is one whole sample() call on the kept step graph (every step replayed), the two settings alternating on ONE
sampler per geometry (they keep one graph each); ms/step = wall time of the call / steps, so the per-call host work (tables,
context K/V refresh) is in both numbers alike.  The call without the keys launches what the sampler launched before the feature
existed.  From the row counts one expects about 3/2 guided and 2/1 unguided, plus a serial dependency: the second forward cannot
start before the first has ended, and at one replica it fills the chip less well than the first.  The isolated launches are timed
with events over 200 back-to-back launches after 20 warm-up launches.  Prints one JSON line: per geometry and setting the
per-repetition values, their median and spread (max - min), the ratio of the medians, the isolated launches in microseconds, and the
box calibration.  Nothing is asserted."""
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

SAG_SCALE = 0.75
GEOMETRIES = [("t2i_guided", "t2i", 7.5), ("i2v_unguided", "i2v", 1.0)]


def _event_us(fn, warm=20, n=200):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def isolated(net, B, side, device):
    """us per launch of the three entries at the shapes a step of batch B on a side x side latent gives them."""
    from lib.model_zoo.vd import sag_map_size, sag_taps
    from vd_hip import ops
    import numpy as np
    Hm, Wm = sag_map_size(net.diffuser["image"], side, side)
    heads, D = 8, 160                                                       # the full-width middle block
    g = torch.Generator().manual_seed(1)
    qkv = (torch.randn((B, Hm * Wm, 3 * heads * D), generator=g) * 0.5).half().to(device)
    x = torch.randn((B, 4, side, side), generator=g).half().to(device)
    eps = torch.randn((2 * B, 4, side, side), generator=g).half().to(device)
    mass = torch.empty((1, B, Hm * Wm), dtype=torch.float32, device=device)
    f32 = lambda v: torch.tensor(np.asarray(v, dtype=np.float32), device=device)
    ratio, taps, coef, w = f32([1.0]), f32(sag_taps(1.0)), f32([0.8, 0.6, 1.25]), f32([-0.1154])
    xd = torch.empty_like(x)
    C = heads * D
    out = {"map": [Hm, Wm], "mass_us": round(_event_us(lambda: ops.sag_mass(qkv[..., :C], qkv[..., C:2 * C], heads, out=mass[0])), 2)}
    out["degrade_us"] = round(_event_us(lambda: ops.sag_degrade(x, eps[:B], mass, ratio, taps, coef, Hm, Wm, out=xd)), 2)
    zero = torch.zeros_like(mass)
    out["degrade_unmasked_us"] = round(_event_us(lambda: ops.sag_degrade(x, eps[:B], zero, ratio, taps, coef, Hm, Wm, out=xd)), 2)
    out["fold_us"] = round(_event_us(lambda: ops.sag_fold(eps, xd, w)), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    device = torch.device("cuda:0")
    net = bench.build_model(device)
    out = {"probe": "sag_step_time", "steps": args.steps, "sag_scale": SAG_SCALE, "sag_blur_sigma": 1.0, "sampler": "DPM-Solver++(2M)"}
    for label, workload, scale in GEOMETRIES:
        wl = bench.WORKLOADS[workload]
        B = wl["batch"]
        ctx = dict(bench.make_contexts(wl, B, device, 1)[0], unconditional_guidance_scale=scale)
        shape = [B, 4, wl["side"], wl["side"]]
        xT = torch.randn(shape, generator=torch.Generator().manual_seed(3)).half().to(device)
        sampler = DPMSolverSampler(net)
        settings = {"off": {}, "sag": {"sag_scale": SAG_SCALE}}

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
               "forwards": {"off": "%d rows" % ((2 if scale != 1.0 else 1) * B), "sag": "%d rows, then %d rows" % ((2 if scale != 1.0 else 1) * B, B)}}
        for name, v in ms.items():
            geo[name] = {"ms_per_step": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                         "spread": round(max(v) - min(v), 3)}
        geo["sag_over_off"] = round(geo["sag"]["median"] / geo["off"]["median"], 4)
        geo["isolated_launches"] = isolated(net, B, wl["side"], device)
        out[label] = geo
        sampler.release_graphs()
        torch.cuda.empty_cache()
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
