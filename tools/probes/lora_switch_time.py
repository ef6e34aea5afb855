"""What switching a LoRA adapter costs, in ONE process, on bench.build_model's full-width random-init UNet at the bench geometry (t2i:
512x512 = 64x64x4 latent, batch 4, guided 7.5, DPMSolverSampler (2M)): a synthetic rank-16 adapter on every attention and
feed-forward projection (attn1 / attn2 to_q, to_k, to_v, to_out.0, the GEGLU proj, ff.net.2) of the transformer blocks the flow
walks -- for a text context those of diffuser.text.context_blocks, which sit between diffuser.image's data blocks.

    python tools/probes/lora_switch_time.py [--steps 20] [--reps 5]

Four things are timed, each `reps` times, the adapter alternating on / off:
  switch_ms          lora.set_adapters alone: one merge launch and one param.copy_ per layer, host wall time with a device
                     synchronise on either side (merge_us_per_layer: the same divided by the layer count)
  first_forward_ms   the first guided UNet forward after it: the kernel-layout packs of the touched layers are rebuilt
                     (pack_builds counts them), against steady_forward_ms, the same forward once more
  first_sample_ms    the first sample() after it: a new step graph is captured (the kept one was keyed on the old weights),
                     against steady_sample_ms, the same call once more (replay only)
  ms_per_step        a replayed step with the adapter on and with it off: merged weights cost nothing per step, so the two
                     must agree within the spread
Prints one JSON line with the per-repetition values, medians and spreads, and the box calibration."""
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

RANK, SCALE = 16, 0.75
PROJECTIONS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
               "ff.net.0.proj", "ff.net.2")


def synthetic_adapter(net, ctype, device):
    """up, down ~ N(0, 1) / sqrt(fan) so that the update has about a tenth of the weight's size at scale 0.75."""
    g = torch.Generator(device=device).manual_seed(7)
    mods = dict(net.named_modules())
    root = "diffuser.%s.context_blocks." % ctype
    tensors = {}
    for p, m in mods.items():
        if p.startswith(root) and any(p.endswith("." + s) for s in PROJECTIONS):
            n, k = m.weight.shape
            tensors[p + ".lora_down.weight"] = torch.randn((RANK, k), generator=g, device=device) / k ** 0.5
            tensors[p + ".lora_up.weight"] = torch.randn((n, RANK), generator=g, device=device) * (0.1 / RANK ** 0.5)
    return tensors


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(v):
    return {"values": [round(x, 3) for x in v], "median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from lib.model_zoo import lora
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    from lib.model_zoo.hip_layers import PackCache
    device = torch.device("cuda:0")
    wl = bench.WORKLOADS["t2i"]
    side, batch = wl["side"], wl["batch"]
    net = bench.build_model(device)
    ctype = wl["ctxs"][0][0]
    layers = lora.attach(net, "probe", synthetic_adapter(net, ctype, device))
    shape = [batch, 4, side, side]
    ctx = dict(bench.make_contexts(wl, batch, device, 1)[0], unconditional_guidance_scale=7.5)
    xT = torch.randn(shape, generator=torch.Generator().manual_seed(3)).half().to(device)
    x, t, cs = bench.forward_inputs(wl, batch, device)
    sampler = DPMSolverSampler(net)

    def sample():
        sampler.sample(steps=args.steps, shape=shape, x_info={"type": "image", "xt": xT}, c_info=dict(ctx), verbose=False)

    for _ in range(2):      # everything warm with the adapter off: packs, workspaces, the kept graph
        bench.run_forward(net, x, t, cs)
        sample()
    keys = ("switch_ms", "first_forward_ms", "steady_forward_ms", "first_sample_ms", "steady_sample_ms")
    ms = {state: {k: [] for k in keys} for state in ("on", "off")}
    builds = {"on": [], "off": []}
    for _ in range(args.reps):
        for state, want in (("on", {"probe": SCALE}), ("off", {})):
            ms[state]["switch_ms"].append(wall_ms(lambda: lora.set_adapters(net, want)))
            b0 = PackCache.builds
            ms[state]["first_forward_ms"].append(wall_ms(lambda: bench.run_forward(net, x, t, cs)))
            builds[state].append(PackCache.builds - b0)
            ms[state]["steady_forward_ms"].append(wall_ms(lambda: bench.run_forward(net, x, t, cs)))
            ms[state]["first_sample_ms"].append(wall_ms(sample))
            ms[state]["steady_sample_ms"].append(wall_ms(sample))
    out = {"probe": "lora_switch_time", "steps": args.steps, "rank": RANK, "layers": len(layers), "shape": shape,
           "sampler": "DPM-Solver++(2M)", "guidance_scale": 7.5,
           "merged_bytes": sum(dict(net.named_modules())[p].weight.numel() * 2 for p in layers)}
    for state in ms:
        out[state] = {k: summary(v) for k, v in ms[state].items()}
        out[state]["pack_builds"] = builds[state]
        out[state]["merge_us_per_layer"] = round(out[state]["switch_ms"]["median"] * 1e3 / len(layers), 2)
        out[state]["ms_per_step"] = summary([v / args.steps for v in ms[state]["steady_sample_ms"]])
    out["on_minus_off_ms_per_step"] = round(out["on"]["ms_per_step"]["median"] - out["off"]["ms_per_step"]["median"], 3)
    sampler.release_graphs()
    out["box_calibration"] = bench.box_calibration(device)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
