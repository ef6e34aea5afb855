"""ms per replayed DPMSolverSampler (2M) step with HyperTile on and off (max_downsample 1) in one process, on bench.build_model's
full-width random-init UNet: the bench geometry (t2i: 512x512 = 64x64x4 latent, batch 4, guidance 7.5) at tile 32, the 768x768
geometry (96x96 latent, batch 4) at tile 48, and a plain 128x128 canvas (1024x1024) at batch 1 with tile 32 and tile 64; and the
isolated times of the two launches HyperTile adds and of the self-attention on the whole grid and on the tiles, at the 320-wide
level of each geometry.

    python tools/probes/hypertile_step_time.py [--steps 20] [--reps 3]

Each repetition is one whole sample() call on the kept step graph (every step replayed), the settings alternating, one sampler per
setting; ms/step = wall time of the call / steps, so the per-call host work is in every number alike.  The call without the key
launches what the sampler launched before the feature existed.  The isolated times are events around 20 back-to-back launches on
random data.  Prints one JSON line: per geometry and setting the per-repetition values, their median and spread (max - min), the
ratios of the medians, the isolated times in microseconds, and the box calibration."""
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

# (label, batch, H, W, tile sides)
GEOMETRIES = [("bench_64x64_b4", 4, 64, 64, [32]), ("t2i768_96x96_b4", 4, 96, 96, [48]), ("plain_128x128_b1", 1, 128, 128, [32, 64])]


def _us(fn, n=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / n, 1)


def isolated(device, B, H, W, tiles, C=320, heads=8):
    """The launches of one tiled block at width C: B samples (the shared CFG head runs attn1 once per guidance pair)."""
    from vd_hip import ops
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn((B, H * W, 3 * C), generator=g).half().to(device)
    out = {"attention_whole": _us(lambda: ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads))}
    for t in tiles:
        m = ops.tile_tokens(qkv, H, W, t, t)
        a = ops.attention(m[..., :C], m[..., C:2 * C], m[..., 2 * C:], heads)
        res = {"tiles": (H // t) * (W // t), "tile": _us(lambda: ops.tile_tokens(qkv, H, W, t, t)),
               "attention_tiled": _us(lambda: ops.attention(m[..., :C], m[..., C:2 * C], m[..., 2 * C:], heads)),
               "untile": _us(lambda: ops.untile_tokens(a, B, H, W, t, t))}
        res["block_total"] = round(res["tile"] + res["attention_tiled"] + res["untile"], 1)
        out["tile_%d" % t] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    device = torch.device("cuda:0")
    net = bench.build_model(device)
    wl = bench.WORKLOADS["t2i"]
    out = {"probe": "hypertile_step_time", "steps": args.steps, "max_downsample": 1, "sampler": "DPM-Solver++(2M)"}
    for label, B, H, W, tiles in GEOMETRIES:
        ctx = dict(bench.make_contexts(wl, B, device, 1)[0], unconditional_guidance_scale=7.5)
        shape = [B, 4, H, W]
        xT = torch.randn(shape, generator=torch.Generator().manual_seed(3)).half().to(device)
        settings = {"off": {}}
        settings.update({"tile_%d" % t: {"hypertile": t} for t in tiles})
        samplers = {name: DPMSolverSampler(net) for name in settings}

        def call(name, steps):
            x_info = dict({"type": "image", "xt": xT}, **settings[name])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, inter = samplers[name].sample(steps=steps, shape=shape, x_info=x_info, c_info=dict(ctx), verbose=False)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps, inter.get("hypertile_tiles")

        tiled = {}
        for name in settings:      # capture (a step count that divides the 1000 training steps), then one call that only replays
            call(name, 4)
            tiled[name] = call(name, args.steps)[1]
        ms = {name: [] for name in settings}
        for _ in range(args.reps):
            for name in settings:
                ms[name].append(call(name, args.steps)[0])
        geo = {"geometry": "t2i %dx%d latent, batch %d, guidance scale 7.5" % (H, W, B), "hypertile_tiles": tiled}
        for name, v in ms.items():
            geo[name] = {"ms_per_step": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                         "spread": round(max(v) - min(v), 3)}
        for name in list(settings)[1:]:
            geo[name]["over_off"] = round(geo[name]["median"] / geo["off"]["median"], 4)
        geo["isolated_us_width320"] = isolated(device, B, H, W, tiles)
        out[label] = geo
        print("[hypertile_step_time] %s done" % label, file=sys.stderr, flush=True)
        for sampler in samplers.values():
            sampler.release_graphs()
        torch.cuda.empty_cache()
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
