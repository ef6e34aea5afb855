"""What the tiled VAE decode costs at full width (KL-f8 with random-init weights, B = 1), in one process: the canvas latent
decoded in tiles of 64 at stride 48 with wrap (vae.decode_scaled(..., tile=64, tile_stride=48, tile_wrap=True)) against the plain
whole-canvas decode of the same latent, whose mid-block attention and GroupNorm see the whole canvas; and the blend kernel
(vd_tile_blend_f16) alone on buffers of the tiled call's shapes.

    python tools/probes/tile_vae_time.py [--canvas 64x256] [--tile-batches 8,1] [--reps 5] [--launches 50] [--skip-plain]

The tiled call runs once per value of --tile-batches (tile_batch: 8 is the default of the keys; 1 sends every tile through the
decoder alone and holds one tile's activations).  Every configuration is warmed by two calls; one that the library refuses (the
whole-canvas path above 2 GiB per operand) is reported as refused.  Then, per repetition, the configurations alternate: ms per
decode is the wall time of one call between two device synchronisations, the peak is torch.cuda.max_memory_allocated over that
call (reset before it).  The blend alone: `--launches` decodes' worth of the call's nc launches, captured into one graph and
replayed between two events (launched one by one from Python, the host's per-call cost would hide a kernel this short); its
bytes are what one decode's launches must move (the valid tiles, wgt per launch, inv_den once, the fp32 canvas written and
read back between launches, the image once), compared with the 256 MB copy of the box calibration from the same process and
with a device-to-device copy of the same number of bytes.  Prints one JSON line: per configuration the values with their
median and spread (max - min), the ratios to the whole-canvas call, the blend's rate and its share of the tiled call, and the
box calibration.  Run it under a time limit.  By pixel count the tiles cost (64 / 48)^2 = 1.8x the convolution work of a
canvas tiled on both axes while the attention term grows linearly instead of quadratically; which way the sum comes out is
what this measures."""
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


def build_vae(device, seed=0):
    """kl-f8 alone with bench.build_model's random initialisation (fan-in scaled normal weights, small biases)."""
    from lib.cfg_helper import model_cfg_bank
    from lib.model_zoo import get_model
    cfg = model_cfg_bank()("autokl_v1")
    cfg.pop("pth", None)
    torch.manual_seed(seed)
    with torch.device(device):
        vae = get_model()(cfg, verbose=False)
    g = torch.Generator(device=device).manual_seed(seed)
    with torch.no_grad():
        for name, p in vae.named_parameters():
            if p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g, device=device) / p[0].numel() ** 0.5)
            elif name.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g, device=device))
    return vae.half().to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--canvas", default="64x256", help="the canvas latent, HxW")
    ap.add_argument("--tile", type=int, default=64)
    ap.add_argument("--stride", type=int, default=48)
    ap.add_argument("--tile-batches", default="8,1", help="tile_batch values of the tiled call; the first is the one the blend is timed for")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--skip-plain", action="store_true", help="time the tiled call and the blend only")
    args = ap.parse_args()
    from lib.model_zoo import vae_tiles
    from vd_hip import ops
    device = torch.device("cuda:0")
    H, W = (int(v) for v in args.canvas.split("x"))
    vae = build_vae(device)
    keys = {"tile": args.tile, "tile_stride": args.stride, "tile_wrap": True}
    batches = [int(v) for v in args.tile_batches.split(",")]
    plan = vae_tiles.tile_plan(dict(keys, tile_batch=batches[0]), H, W, vae.factor)
    z = torch.randn((1, 4, H, W), generator=torch.Generator().manual_seed(3)).half().to(device)
    configs = {"tiled_batch%d" % b: dict(keys, tile_batch=b) for b in batches}
    first = "tiled_batch%d" % batches[0]
    if not args.skip_plain:
        configs["plain"] = {}

    def call(name):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(device)
        t0 = time.perf_counter()
        img = vae.decode_scaled(z, 1.0 / 0.18215, **configs[name])
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert tuple(img.shape) == (1, 3, 8 * H, 8 * W)
        return ms, torch.cuda.max_memory_allocated(device) / 2 ** 20

    from vd_hip.loader import VdHipError
    refused = {}
    for name in list(configs):
        try:
            call(name)
            call(name)
        except VdHipError as e:             # a canvas the whole-image path does not take is a result, not a crash
            refused[name] = str(e)
            del configs[name]
    ms, peak = {n: [] for n in configs}, {n: [] for n in configs}
    for _ in range(args.reps):
        for name in configs:
            m, p = call(name)
            ms[name].append(m)
            peak[name].append(p)

    # the blend alone, on buffers of the tiled call's shapes
    (PH, PW), (ph, pw), nc, m = plan["out_hw"], plan["tile_hw"], plan["nc"], plan["m"]
    tiles = torch.randn((1, m, ph, pw, 3), device=device).half()
    offs = torch.from_numpy(plan["blend"]).to(device)
    wgt, inv = (torch.from_numpy(a).to(device) for a in vae_tiles.tile_tables(plan))
    acc = torch.empty((1, 3, PH, PW), device=device, dtype=torch.float32) if nc > 1 else None
    out = torch.empty((1, 3, PH, PW), device=device, dtype=torch.float16)

    def blend_once():
        for k in range(nc):
            ops.tile_blend(tiles, offs[k], wgt, inv, PH, PW, plan["valid"][k], True, k == 0, k == nc - 1, acc=acc, out=out,
                           scale=0.5, shift=0.5, clamp01=True)

    # `--launches` decodes' worth of launches captured into one graph: replayed, the device runs them back to back and the
    # host's per-call cost (argument checks, ctypes) is off the clock
    blend_once()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.launches):
            blend_once()
    blend_ms = []
    for _ in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        blend_ms.append(e0.elapsed_time(e1) / args.launches)
    blend_ms = blend_ms[1:]                                               # the first round warms
    tile_bytes, canvas = 2 * 3 * ph * pw, PH * PW
    # valid tiles (fp16) + wgt per launch + inv_den once + acc written and read back between launches (fp32) + the image (fp16)
    moved = plan["n"] * tile_bytes + nc * 4 * ph * pw + 4 * canvas + (nc - 1) * 2 * 4 * 3 * canvas + 2 * 3 * canvas
    med = statistics.median
    spread = lambda v: max(v) - min(v)
    cal = bench.box_calibration(device)
    out_d = {"probe": "tile_vae_time", "canvas_latent": [H, W], "image": [8 * H, 8 * W],
             "tiles": {"tile": args.tile, "stride": args.stride, "wrap": True, "n": plan["n"], "passes": nc, "slots": m},
             "configs": {}}
    for name in configs:
        out_d["configs"][name] = {"ms": [round(v, 2) for v in ms[name]], "ms_median": round(med(ms[name]), 2),
                                  "ms_spread": round(spread(ms[name]), 2), "peak_mib_median": round(med(peak[name]), 1)}
    for name, why in refused.items():
        out_d["configs"][name] = {"refused": why}
    if "plain" in configs:
        out_d["tiled_over_plain_ms"] = {n: round(med(ms[n]) / med(ms["plain"]), 4) for n in configs if n != "plain"}
        out_d["tiled_over_plain_peak"] = {n: round(med(peak[n]) / med(peak["plain"]), 4) for n in configs if n != "plain"}
    b = med(blend_ms)
    src = torch.empty(moved // 2, dtype=torch.uint8, device=device).fill_(7)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.launches):
        dst.copy_(src)
    e1.record()
    e1.synchronize()
    copy_same = 2 * (moved // 2) / (e0.elapsed_time(e1) / args.launches) / 1e9
    out_d["blend"] = {"launches_per_decode": nc, "ms_per_decode": [round(v, 4) for v in blend_ms], "ms_median": round(b, 4),
                      "ms_spread": round(spread(blend_ms), 4), "bytes_per_decode": moved, "tbps": round(moved / b / 1e9, 4),
                      "share_of_copy_256mb": round(moved / b / 1e9 / cal["copy_256mb_tbps"], 4),
                      "copy_same_bytes_tbps": round(copy_same, 4), "share_of_copy_same_bytes": round(moved / b / 1e9 / copy_same, 4),
                      "share_of_tiled_decode": round(b / med(ms[first]), 5)}
    out_d["box_calibration"] = cal
    print(json.dumps(out_d))


if __name__ == "__main__":
    main()
