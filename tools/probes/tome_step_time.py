"""ms per replayed DPMSolverSampler (2M) step with token merging at ratio 0 / 0.25 / 0.5 (max_downsample 1) in one process, on
bench.build_model's full-width random-init UNet at two geometries: the bench geometry (t2i: 512x512 = 64x64x4 latent, batch 4,
guidance 7.5) and a plain 64x128 canvas (512x1024) at batch 1; and the isolated times of the four launches token merging adds
and of the self-attention at N and N - r rows, at the 320-wide level of either geometry.

    python tools/probes/tome_step_time.py [--steps 20] [--reps 3]

Each repetition is one whole sample() call on the kept step graph (every step replayed), the settings alternating, one sampler per
setting (a sampler keeps two graphs, there are three settings); ms/step = wall time of the call / steps, so the per-call host work is in every number
alike.  The call without the keys launches what the sampler launched before the feature existed.  The isolated times are events
around 20 back-to-back launches on random data (a random metric: the plan merges whatever it ranks first).  Prints one JSON
line: per geometry and setting the per-repetition values, their median and spread (max - min), the ratios of the medians, the
isolated times in microseconds, and the box calibration."""
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

RATIOS = [0.0, 0.25, 0.5]
GEOMETRIES = [("bench_64x64_b4", 4, 64, 64), ("plain_64x128_b1", 1, 64, 128)]


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


def isolated(device, B, H, W, C=320, heads=8):
    """The launches of one merging block at width C: B samples (the shared CFG head runs attn1 once per guidance pair)."""
    from vd_hip import ops
    g = torch.Generator().manual_seed(1)
    N = H * W
    h = torch.randn((B, N, C), generator=g).half().to(device)
    qkv = torch.randn((B, N, 3 * C), generator=g).half().to(device)
    out = {"attention_N": _us(lambda: ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads))}
    for ratio in RATIOS[1:]:
        r = min(int(N * ratio), N - N // 4)
        idx, mx = ops.tome_match(h, H, W)
        row_of = ops.tome_plan(idx, mx, H, W, r)
        m = ops.tome_merge(qkv, row_of, H, W, r)
        a = ops.attention(m[..., :C], m[..., C:2 * C], m[..., 2 * C:], heads)
        res = {"r": r, "match": _us(lambda: ops.tome_match(h, H, W)), "plan": _us(lambda: ops.tome_plan(idx, mx, H, W, r)),
               "merge": _us(lambda: ops.tome_merge(qkv, row_of, H, W, r)),
               "attention_N_minus_r": _us(lambda: ops.attention(m[..., :C], m[..., C:2 * C], m[..., 2 * C:], heads)),
               "unmerge": _us(lambda: ops.tome_unmerge(a, row_of, H, W, r))}
        res["block_total"] = round(sum(res[k] for k in ("match", "plan", "merge", "attention_N_minus_r", "unmerge")), 1)
        out["ratio_%g" % ratio] = res
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
    out = {"probe": "tome_step_time", "steps": args.steps, "ratios": RATIOS, "max_downsample": 1, "sampler": "DPM-Solver++(2M)"}
    for label, B, H, W in GEOMETRIES:
        ctx = dict(bench.make_contexts(wl, B, device, 1)[0], unconditional_guidance_scale=7.5)
        shape = [B, 4, H, W]
        xT = torch.randn(shape, generator=torch.Generator().manual_seed(3)).half().to(device)
        settings = {"ratio_%g" % r: ({"tome_ratio": r} if r else {}) for r in RATIOS}
        samplers = {name: DPMSolverSampler(net) for name in settings}

        def call(name, steps):
            x_info = dict({"type": "image", "xt": xT}, **settings[name])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, inter = samplers[name].sample(steps=steps, shape=shape, x_info=x_info, c_info=dict(ctx), verbose=False)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps, inter.get("tome_tokens")

        tokens = {}
        for name in settings:      # capture (a step count that divides the 1000 training steps), then one call that only replays
            call(name, 4)
            tokens[name] = call(name, args.steps)[1]
        ms = {name: [] for name in settings}
        for _ in range(args.reps):
            for name in settings:
                ms[name].append(call(name, args.steps)[0])
        geo = {"geometry": "t2i %dx%d latent, batch %d, guidance scale 7.5" % (H, W, B), "tome_tokens": tokens}
        for name, v in ms.items():
            geo[name] = {"ms_per_step": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                         "spread": round(max(v) - min(v), 3)}
        for name in list(settings)[1:]:
            geo[name]["over_off"] = round(geo[name]["median"] / geo["ratio_0"]["median"], 4)
        geo["isolated_us_width320"] = isolated(device, B, H, W)
        out[label] = geo
        for sampler in samplers.values():
            sampler.release_graphs()
        torch.cuda.empty_cache()
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
