#!/usr/bin/env python
"""Headline benchmark: 512x512 images/sec at 50 DDIM steps (BASELINE.json metric), synthetic inputs.

    python bench.py --gpus N --steps K --warmup W [--workload t2i|i2v|dual|triple] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
(`python bench.py --gpus N` with N > 1 and no torchrun environment re-launches itself under torch.distributed.run with N
ranks, or exits non-zero when the node has fewer than N GPUs -- it never reports n_gpus: 1 for a --gpus N request.)

One "step" = one pass of the hot path over one batch: a guided (CFG 7.5) 50-step DDIM loop over the batch's latents,
followed by the KL-f8 decode.  The default workload is BASELINE.json configs[1] ("text-to-image 512x512, 50 DDIM steps,
bs=4 fp16, 1xMI355X": 4 latents of 64x64x4, text context [B,77,768]); --workload selects configs[2..4]: image variation
(bs 8, + VAE encode, image context L=257), dual-guided (text + image context mixing, 2 per GPU = bs 16 on 8 GPUs) and the
triple-context 768x768 blender (text + two masked images, L=514, 4 per GPU = bs 32 on 8 GPUs).  Context encoding (CLIP)
is outside the timed region.  Inputs (contexts, images, weights) are resident in HBM when timing
starts.  Every configuration goes through lib.model_zoo.sharded.vd_sample_sharded: the full-batch latent is drawn once
and sliced per rank, each rank samples its slice (per-GPU batch fixed: weak scaling), and the decoded images are
all-gathered over RCCL inside the timed region.

A plain run sets up, warms up, times the K steps and prints the JSON line: images/s (`value`), `ms_per_step`, the build of
the library and the whole-path rate derived from the timed steps.  --dump-outputs DIR writes the decoded images of the
last timed step (what a caller of the timed path receives) as DIR/images.npy in float32; every input is seeded, so two
runs with the same arguments see the same inputs and two builds can be compared output for output.

With --full the JSON line also carries
  unet_forward_ms_per_ddim_step_bsB -- BASELINE metric (ii): one guided DDIM step replayed from the sampler's HIP graph
  roofline      -- for the kernel that dominates a UNet forward of the workload: algorithmic FLOPs of its launches /
                   their measured duration (events on the launch stream), against the dense fp16 MFMA peak of MI355X
  cpu_baseline  -- the CPU fp32 oracle (oracle/vd_oracle.py, kind "port") timed on this host on a bounded sample
  other_workloads -- (default t2i run at N = 1 only) BASELINE configs[2..4] through the same code path, 1 warm-up + 2 timed
                   batches each, OUTSIDE the timed region of the headline value: images/s and ms per batch per workload
  box_calibration -- how fast THIS box is (the pool spreads +-4 %): vd_gemm_f16 at 8192^3 and a 256 MB copy, outside the
                   timed region, with the ratio to the round's evidence box
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "versatile-diffusion_amd"))
sys.path.insert(0, ROOT)
os.environ.setdefault("VD_QUIET", "1")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402

MFMA_FP16_PEAK_TFLOPS = 2500.0   # dense fp16/bf16, MI355X_MICROARCH.md chip-level table
PMC_TRAFFIC_FILE = "r06_pmc_traffic.json"
TRACE_FILE = "r06_trace_dominant.json"   # tools/trace_dominant.py: rocprofv3 kernel-trace average of the dominant kernel, digest-stamped   # tools/pmc_traffic.py; stamped with the digest of the library it was taken with
HBM_PEAK_GBS = 8000.0
UNET_GF_PER_SAMPLE = 803.3       # 64x64 latent, text ctx L=77
VAE_DECODE_GF = 2514.5


def build_model(device, seed=0):
    """vd_four_flow_v1-0's image path: openai_unet_2d_v1 + the text context blocks (openai_unet_0d_v1_c) + kl-f8,
    random-init weights of that architecture generated on the device (no checkpoints offline)."""
    from lib.cfg_helper import CfgDict, model_cfg_bank
    from lib.model_zoo import get_model
    bank = model_cfg_bank()
    vae = bank("autokl_v1")
    vae.pop("pth", None)
    cfg = CfgDict(type="vd_v2_0", args=CfgDict(
        vae_cfg_list=[["image", vae]], ctx_cfg_list=[["image", "ctx-image-placeholder"], ["text", "ctx-text-placeholder"]],
        diffuser_cfg_list=[["image", bank("openai_unet_2d_v1")], ["text", bank("openai_unet_0d_v1_c")]],
        global_layer_ptr="image", latent_scale_factor={"image": 0.18215}, beta_linear_start=0.00085,
        beta_linear_end=0.012, timesteps=1000, use_ema=False))
    torch.manual_seed(seed)
    with torch.device(device):
        net = get_model()(cfg, verbose=False)
    g = torch.Generator(device=device).manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() >= 2:   # fan-in scaled normal incl. the zero-initialised convs (else the UNet outputs 0)
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g, device=device) / fan_in ** 0.5)
            elif name.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g, device=device))
    net = net.half()
    net.to(device)
    return net


# ---- workloads = BASELINE.json configs[1..4] ----------------------------------------------------
# gf_fwd: algorithmic GFLOP of ONE UNet forward per sample (reference graph, torch flop counter)
FIDELITY = 0.02   # image-variation fidelity of the i2v workload: int(50 * 0.98) = 49 of the 50 DDIM steps run
WORKLOADS = {
    "t2i": dict(cfg=1, side=64, batch=4, global_fixed=False, ctxs=[("text", 77, 1.0)], gf_fwd=803.3, vae_dec=2514.5, vae_enc=0.0,
                desc="text-to-image 512x512 (64x64x4 latent), single text-context flow"),
    "i2v": dict(cfg=2, side=64, batch=8, global_fixed=False, ctxs=[("image", 257, 1.0)], gf_fwd=818.5, vae_dec=2514.5, vae_enc=1116.7,
                desc="image-variation 512x512: KL-f8 VAE encode of the input images -> q_sample -> DDIM with the CLIP "
                     "image context (L=257, zero unconditional context), fidelity 0.02 = 49 of 50 steps"),
    "dual": dict(cfg=3, side=64, batch=16, global_fixed=True, ctxs=[("text", 77, 0.5), ("image", 257, 0.5)], gf_fwd=1203.4,
                 vae_dec=2514.5, vae_enc=0.0,
                 desc="dual-guided text (L=77, ratio 0.5) + image (L=257, ratio 0.5) context mixing 512x512, global batch 16 "
                      "sharded on the batch axis"),
    "triple": dict(cfg=4, side=96, batch=32, global_fixed=True, ctxs=[("text", 77, 0.4), ("image", 514, 0.6)], gf_fwd=3417.1,
                   vae_dec=5754.3, vae_enc=0.0,
                   desc="triple-context image blender 768x768 (96x96x4 latent): text (L=77, ratio 0.4) + two masked images "
                        "(L=514, ratio 0.6), global batch 32 sharded on the batch axis"),
}


def make_contexts(wl, n, device, seed):
    """Synthetic CLIP-like contexts [n, L, 768] per context type + the unconditional ones the app uses (encoded empty
    prompt for text -- one row repeated, app.py:305; all-zeros for images, app.py:345,475,562)."""
    g = torch.Generator(device=device).manual_seed(seed)
    out = []
    for ctype, L, ratio in wl["ctxs"]:
        c = (torch.randn((n, L, 768), generator=g, device=device) * 0.5).half()
        if ctype == "text":
            u = (torch.randn((1, L, 768), generator=g, device=device) * 0.5).half().repeat(n, 1, 1)
        else:
            u = torch.zeros_like(c)
        out.append({"type": ctype, "conditioning": c, "unconditional_conditioning": u,
                    "unconditional_guidance_scale": 7.5, "ratio": ratio})
    return out


def one_batch(net, sampler, wl, ctxs, n_global, steps, seed, images=None):
    """One pass of the hot path over one batch: (VAE encode -> q_sample ->) guided DDIM loop -> KL-f8 decode ->
    all_gather, through lib.model_zoo.sharded.vd_sample_sharded: the full-batch latent is drawn ONCE with the reference's
    seed rule (torch.manual_seed(seed + 100), app.py:309) and sliced per rank, the decoded images are all-gathered."""
    from lib.model_zoo import sharded
    return sharded.vd_sample_sharded(net, sampler, steps, [n_global, 4, wl["side"], wl["side"]], ctxs, seed,
                                     images=images, fidelity=FIDELITY if images is not None else 0.)


def forward_inputs(wl, batch, device):
    side = wl["side"]
    x = torch.randn(2 * batch, 4, side, side, device=device, dtype=torch.float16)
    t = torch.full((2 * batch,), 501, device=device, dtype=torch.long)
    cs = [{"type": ct, "c": torch.randn(2 * batch, L, 768, device=device, dtype=torch.float16) * 0.5, "ratio": r}
          for ct, L, r in wl["ctxs"]]
    return x, t, cs


def run_forward(net, x, t, cs):
    if len(cs) == 1:
        return net.apply_model({"type": "image", "x": x}, t, cs[0])
    return net.apply_model_multicontext({"type": "image", "x": x}, t, cs)


def roofline_leg(net, wl, batch, device):
    """One instrumented UNet forward at the workload's shape (CFG batch 2B): per-launch events on the launch stream +
    algorithmic FLOPs per launch -> the kernel with the largest share of the forward and its fraction of the MFMA peak."""
    from vd_hip import ops
    x, t, cs = forward_inputs(wl, batch, device)
    for _ in range(2):
        run_forward(net, x, t, cs)
    torch.cuda.synchronize()
    agg = {}
    reps = 3
    for _ in range(reps):
        ops.profile_begin()
        run_forward(net, x, t, cs)
        for name, fl, by, ms in ops.profile_end():
            a = agg.setdefault(name, [0, 0.0, 0.0, 0.0])
            a[0] += 1; a[1] += fl; a[2] += by; a[3] += ms
    table = {n: dict(launches=a[0] // reps, gflop=a[1] / reps / 1e9, mbytes=a[2] / reps / 1e6, ms=a[3] / reps,
                     avg_us=1e3 * a[3] / a[0]) for n, a in agg.items()}
    dom = max(table, key=lambda n: table[n]["ms"])
    d = table[dom]
    achieved = d["gflop"] / d["ms"]  # GFLOP/ms == TFLOP/s
    # HBM-side bytes per launch come from separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; gfx950 corrections
    # applied) over tools/unet_forward.py -- PMC collection cannot run inside this process; null when not collected for
    # this kernel at this round's build
    traffic, traffic_note = None, None
    alg_bytes = d["mbytes"] * 1e6 / max(d["launches"], 1)   # unique operand bytes per launch (vd_hip/ops.py)
    try:
        from vd_hip.loader import lib_digest
        with open(os.path.join(ROOT, "profiles", PMC_TRAFFIC_FILE)) as f:
            pt = json.load(f)
        ent = pt["kernels"].get(dom)
        if pt.get("library_digest") != lib_digest():
            traffic_note = "profiles/%s was taken with another build of libvd_hip.so (digest %s, loaded %s): ignored" % (
                PMC_TRAFFIC_FILE, pt.get("library_digest"), lib_digest())
        elif ent and wl["cfg"] == 1:
            traffic = ent["hbm_side_bytes_per_launch"]
            traffic_note = "profiles/%s (library digest %s): %s" % (PMC_TRAFFIC_FILE, pt["library_digest"], pt["note"])
    except Exception as e:
        traffic_note = "no PMC traffic file: %s" % e
    # ONE stated clock for `achieved` / `frac`: HIP events around every launch of an eager forward (this process).  The
    # rocprofv3 kernel-trace average of the same kernel (bench command traced separately, profiles/) is carried next to it
    # when it was taken with the library that is loaded; the trace sees the kernel alone, the events include launch skew.
    gflop_per_launch = d["gflop"] / max(d["launches"], 1)
    trace = None
    try:
        from vd_hip.loader import lib_digest
        with open(os.path.join(ROOT, "profiles", TRACE_FILE)) as f:
            tr = json.load(f)
        if tr.get("library_digest") == lib_digest() and tr.get("kernel") == dom and wl["cfg"] == 1:
            tf = gflop_per_launch / (tr["avg_us"] * 1e-3)
            trace = {"avg_launch_us": tr["avg_us"], "achieved": round(tf, 1), "frac": round(tf / MFMA_FP16_PEAK_TFLOPS, 4),
                     "calls": tr.get("calls"), "source": "profiles/%s (rocprofv3 --kernel-trace of the bench command)" % TRACE_FILE}
    except Exception:
        trace = None
    roof = {"kernel": dom, "bound": "mfma", "achieved": round(achieved, 1), "peak": MFMA_FP16_PEAK_TFLOPS,
            "unit": "TFLOP/s", "frac": round(achieved / MFMA_FP16_PEAK_TFLOPS, 4),
            "clock": "HIP events on the launch stream around each launch of an eager forward, measured live by this run",
            "kernel_trace": trace, "traffic": traffic,
            "traffic_note": traffic_note, "algorithmic_bytes_per_launch": int(alg_bytes),
            "traffic_ratio": (round(traffic / alg_bytes, 2) if traffic else None),
            "launches_per_forward": d["launches"], "avg_launch_us": round(d["avg_us"], 1),
            "algorithmic_gflop_per_launch": round(d["gflop"] / max(d["launches"], 1), 2),
            "forward_ms_instrumented": round(sum(v["ms"] for v in table.values()), 3),
            "forward_algorithmic_tflop": round(2 * batch * wl["gf_fwd"] / 1e3, 3)}
    return roof, table


def graph_step_ms(net, sampler, wl, batch, steps, device, reps=20):
    """Device time of ONE guided DDIM step (CFG-batched UNet forward + CFG combine + DDIM update) replayed from the HIP
    graph the sampler uses -- BASELINE metric (ii), HIP events over `reps` warm replays."""
    from vd_hip import ops
    side = wl["side"]
    xs = torch.randn(batch, 4, side, side, device=device, dtype=torch.float16)
    x_next, p0 = torch.empty_like(xs), torch.empty_like(xs)
    ts = torch.full((2 * batch,), 501, device=device, dtype=torch.long)
    sampler.make_schedule(steps, verbose=False)
    coef = sampler._coef_table(steps, 7.5, device)[steps // 2].clone()
    cis = []
    for ct, L, r in wl["ctxs"]:
        cis.append({"type": ct, "c": torch.randn(2 * batch, L, 768, device=device, dtype=torch.float16) * 0.5, "ratio": r,
                    "kv_cache": {}})

    # as in DDIMSampler._loop_static: the t-only part of the forward is computed once per sample() for all steps, the captured
    # step reads its row from a static buffer
    emb_rows = None
    if getattr(sampler, "emb_hoist", False) and hasattr(net, "precompute_step_emb"):
        with torch.no_grad():
            pre = net.precompute_step_emb("image", ts[:1], multicontext=len(cis) > 1)
        if pre is not None:
            row = pre[0][0].clone()
            emb_rows = {di: row[o:o + c] for di, (o, c) in pre[1].items()}

    def body():
        xi = {"type": "image", "x": xs, "repeat": 2}
        if emb_rows is not None:
            xi["emb_rows"] = emb_rows
        eps = net.apply_model(xi, ts, cis[0]) if len(cis) == 1 else net.apply_model_multicontext(xi, ts, cis)
        ops.cfg_ddim_step_dev(xs, eps.contiguous(), coef, guided=True, x_prev=x_next, pred_x0=p0)

    with torch.no_grad():
        for _ in range(2):
            body()
        n0 = ops.LIB_CALLS[0]
        body()
        graph_step_ms.lib_calls = ops.LIB_CALLS[0] - n0   # calls into the C ABI per step (a split launch + its reduce = one call)
        graph = sampler._capture(body)
        if graph is None:
            return None
        graph.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


# reference values of box_calibration on the round-6 evidence box (profiles/r06_bench.json): the `ratio` fields of a later line say
# how fast THAT box is against it -- boxes of this pool spread +-4 %, more than a round's gain
CAL_REF = {"gemm_8192_tflops": 776.0, "copy_256mb_tbps": 5.318}


def box_calibration(device):
    """How fast is this box?  Outside every timed region, ~0.3 s: the library's own fp16 GEMM at 8192^3 (MFMA rate under power: what
    the chip sustains on this box today) and a 256 MB device-to-device copy (memory side).  A driver number divided by these is
    comparable across boxes and rounds; `ratio` is against CAL_REF where that is filled in."""
    from vd_hip import ops
    n = 8192
    a = torch.randn(n, n, device=device, dtype=torch.float16)
    w = torch.randn(n, n, device=device, dtype=torch.float16) * 0.02
    for _ in range(2):
        ops.gemm(a, w)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(6):
        ops.gemm(a, w)
    e1.record()
    torch.cuda.synchronize()
    g_ms = e0.elapsed_time(e1) / 6
    del a, w
    src = torch.empty(256 << 20, dtype=torch.uint8, device=device).fill_(7)
    dst = torch.empty_like(src)
    for _ in range(2):
        dst.copy_(src)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(10):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    c_ms = e0.elapsed_time(e1) / 10
    del src, dst
    out = {"gemm_8192_tflops": round(2.0 * n ** 3 / g_ms / 1e9, 1), "gemm_8192_ms": round(g_ms, 3),
           "copy_256mb_tbps": round(2.0 * (256 << 20) / c_ms / 1e9, 3), "copy_256mb_ms": round(c_ms, 4),
           "note": "vd_gemm_f16 at 8192^3 (random data) and a 256 MB device-to-device copy (read + write bytes), outside the timed region"}
    ratios = {k: round(out[k] / v, 4) for k, v in CAL_REF.items() if v}
    if ratios:
        out["ratio_to_r06_evidence_box"] = ratios
    return out


def cpu_baseline_leg(net, device):
    """CPU fp32 oracle on a bounded sample: one CFG-batch-2 UNet forward (64x64 latent, L=77) and one 32x32-latent
    VAE decode (scaled x4 to 64x64 by area); extrapolated to images/sec at 50 steps.  Threads are pinned (VD_CPU_THREADS,
    default 16 = the fastest setting measured on the GPU boxes' 256-thread hosts: 8 / 16 / 32 / 64 / 128 threads take 5.1 /
    4.2 / 4.6 / 6.3 / 11.2 s for this forward) and the count actually used is reported as `cores`."""
    from oracle import vd_oracle as O
    sd = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    cores = max(1, min(int(os.environ.get("VD_CPU_THREADS", "16")), os.cpu_count() or 1))
    prev = torch.get_num_threads()
    torch.set_num_threads(cores)
    g = torch.Generator().manual_seed(0)
    x = torch.randn((2, 4, 64, 64), generator=g)
    c = torch.randn((2, 77, 768), generator=g) * 0.5
    t = torch.tensor([501, 501])
    plan = O.unet_plan()
    with torch.no_grad():
        O.apply_model(sd, plan, x[:, :, :16, :16].contiguous(), t, c, c_type="text", global_ptr="image")  # warm the allocator
        t0 = time.time()
        O.apply_model(sd, plan, x, t, c, c_type="text", global_ptr="image")
        t_fwd = time.time() - t0
        z = torch.randn((1, 4, 32, 32), generator=g)
        t0 = time.time()
        O.vae_decode(sd, "vae.image", z)
        t_dec = (time.time() - t0) * 4.0
    torch.set_num_threads(prev)
    per_image = 50 * t_fwd + t_dec
    return {"value": round(1.0 / per_image, 5), "unit": "images/s", "cores": cores, "kind": "port",
            "kind_note": "CPU fp32 restatement of the reference's path (oracle/, pinned to the reference by fixtures and live "
                         "differentials); the reference tree itself is absent on the GPU box",
            "sample": "oracle fp32 on %d pinned threads: 1 UNet forward (CFG batch 2, 64x64x4 latent, L=77) = %.2f s; 1 VAE "
                      "decode 32x32 latent x4 area = %.2f s; extrapolated 50*forward + decode per image" % (cores, t_fwd, t_dec)}


def self_launch(n):
    """`python bench.py --gpus N` outside torchrun: re-run this command as N ranks under torch.distributed.run."""
    import socket
    import subprocess
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < n:
        raise SystemExit("bench.py --gpus %d: this node has %d visible GPU(s); refusing to report a %d-GPU number from fewer "
                         "devices" % (n, have, n))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd))


def timed_batches(net, sampler, wl, ctxs, n_global, ddim_steps, images, warmup, steps, barrier):
    """`warmup` untimed + `steps` timed batches of one workload; returns (seconds, last images)."""
    img = None
    for i in range(warmup):
        img = one_batch(net, sampler, wl, ctxs, n_global, ddim_steps, i, images)
    barrier()
    t0 = time.perf_counter()
    for i in range(steps):
        img = one_batch(net, sampler, wl, ctxs, n_global, ddim_steps, 10 + i, images)
    barrier()
    return time.perf_counter() - t0, img


def workload_inputs(wl, per_gpu, world, rank, device):
    n_global = per_gpu * world
    ctxs = make_contexts(wl, n_global, device, 1000)   # same seed on every rank: the full batch, sliced per rank
    images = None
    if wl["vae_enc"]:
        lo = per_gpu * rank
        gi = torch.Generator(device=device).manual_seed(2000)
        images = torch.rand((n_global, 3, 8 * wl["side"], 8 * wl["side"]), generator=gi, device=device).half()[lo:lo + per_gpu]
    return n_global, ctxs, images


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, img):
    """The decoded images of the last timed step as float32 [B, 3, H, W].  Larger than DUMP_LIMIT_BYTES (a global batch
    beyond the 1-GPU defaults): the first images of the batch that fit."""
    os.makedirs(out_dir, exist_ok=True)
    per_image = img[0].numel() * 4
    keep = max(1, min(img.shape[0], DUMP_LIMIT_BYTES // per_image))
    np.save(os.path.join(out_dir, "images.npy"), img[:keep].float().cpu().numpy())


def default_per_gpu(wl):
    # t2i / i2v: BASELINE quotes a per-GPU batch.  dual / triple: BASELINE quotes the GLOBAL batch of the 8-GPU job (16 / 32);
    # a rank always runs its share of that job (2 / 4 images), so on N GPUs the job is N/8 of the 8-GPU one: per-GPU work is
    # fixed as N grows = weak scaling for every workload
    return max(1, wl["batch"] // 8) if wl["global_fixed"] else wl["batch"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3, help="timed batches (each = 50 DDIM steps + decode)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="t2i",
                    help="t2i = BASELINE configs[1] (default, the config the metric is quoted on); i2v / dual / triple = configs[2..4]")
    ap.add_argument("--batch", type=int, default=None, help="images per GPU per step (default: the workload's)")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="skip the other_workloads block (configs[2..4], 2 timed batches each) of the default t2i line")
    ap.add_argument("--cpu-baseline-only", action="store_true",
                    help="run only the cpu_baseline leg (VD_CPU_THREADS selects the pinned thread count) and print it")
    ap.add_argument("--dump-kernel-table", default=None, help="write the per-kernel table of the roofline leg here (--full)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the decoded images of the last timed step to DIR/images.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="also measure metric (ii), the roofline, the CPU baseline, the box calibration and the other workloads")
    args = ap.parse_args()
    wl = WORKLOADS[args.workload]

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch with --nproc-per-node == --gpus)" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if distributed:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=device)

    # per-GPU batch fixed for every workload (see default_per_gpu): N GPUs sample N x per_gpu images per step
    per_gpu = args.batch if args.batch is not None else default_per_gpu(wl)
    scaling = "weak"

    from lib.model_zoo.ddim import DDIMSampler
    net = build_model(device)
    if args.cpu_baseline_only:
        print(json.dumps({"cpu_baseline": cpu_baseline_leg(net, device)}))
        return
    sampler = DDIMSampler(net)
    n_global, ctxs, images = workload_inputs(wl, per_gpu, world, rank, device)

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    elapsed, img = timed_batches(net, sampler, wl, ctxs, n_global, args.ddim_steps, images, args.warmup, args.steps, barrier)
    if distributed:
        tt = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    px = 8 * wl["side"]
    assert img.shape == (n_global, 3, px, px) and bool(torch.isfinite(img).all())

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, img)

    ms_per_step = 1e3 * elapsed / args.steps
    value = n_global * args.steps / elapsed
    n_unet_steps = int(args.ddim_steps * (1 - FIDELITY)) if wl["vae_enc"] else args.ddim_steps
    out = {
        "metric": "%dx%d images/sec (50-step DDIM)" % (px, px), "value": round(value, 4), "unit": "images/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 2),
        "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": "f16", "data": "synthetic",
        "config": {"workload": "BASELINE configs[%d]: %s; %d DDIM steps, CFG 7.5, bs=%d per GPU, fp16 (vd_four_flow_v1-0 UNet "
                               "859.5M + context blocks of the 0-D net) + kl-f8 decode; CLIP context encoding outside the "
                               "timed region" % (wl["cfg"], wl["desc"], args.ddim_steps, per_gpu),
                   "name": args.workload, "global_batch": n_global, "ddim_steps": args.ddim_steps,
                   "parallelism": "batch-shard x%d (latent drawn once and sliced, one all_gather of decoded images)" % world,
                   "weights": "random-init (fan-in scaled normal), no checkpoints offline",
                   "exact_reuse": "context K/V projections computed once per sample() (inside the timed region); data blocks "
                                  "in front of the first context block shared by the two CFG replicas; throughput is counted "
                                  "on the reference's algorithmic FLOPs"},
    }
    if rank == 0:
        try:   # which build of the HIP library produced this line (no build_mode record in the tree)
            from vd_hip.loader import lib_digest, lib_path
            stamp = lib_path() + ".stamp"
            out["library"] = {"path": os.path.relpath(lib_path(), ROOT), "digest": lib_digest(),
                              "source_stamp": (open(stamp).read().strip()[:16] if os.path.exists(stamp) else None),
                              "mtime": int(os.path.getmtime(lib_path())),
                              "note": "digest = SHA-256 prefix of libvd_hip.so; source_stamp = hash of csrc/*.hip + headers + build.py "
                                      "the library was built from (build.py rebuilds when it differs from the sources)"}
        except Exception as e:
            out["library"] = {"error": str(e)}
        alg_tf = per_gpu * (2 * n_unet_steps * wl["gf_fwd"] + wl["vae_dec"] + wl["vae_enc"]) / 1e3
        out["algorithmic_tflop_per_step"] = round(alg_tf, 1)
        out["whole_path_tflops_per_gpu"] = round(alg_tf / (ms_per_step / 1e3), 1)
        out["whole_path_frac_of_mfma_peak"] = round(alg_tf / (ms_per_step / 1e3) / MFMA_FP16_PEAK_TFLOPS, 4)
        if args.full and not args.no_roofline:
            # BASELINE metric (ii): device time of one guided DDIM step (UNet forward at CFG batch 2B + update) replayed
            # from the sampler's HIP graph; 40 % of the MFMA peak <=> 2 * B * gf_fwd / 1 PFLOP/s
            ms = graph_step_ms(net, sampler, wl, per_gpu, args.ddim_steps, device)
            if ms is not None:
                out["unet_forward_ms_per_ddim_step_bs%d" % per_gpu] = round(ms, 3)
                out["unet_forward_frac_of_mfma_peak"] = round(2 * per_gpu * wl["gf_fwd"] / ms / MFMA_FP16_PEAK_TFLOPS, 4)
                out["library_calls_per_ddim_step"] = getattr(graph_step_ms, "lib_calls", None)
            roof, table = roofline_leg(net, wl, per_gpu, device)
            out["roofline"] = roof
            if args.dump_kernel_table:
                with open(args.dump_kernel_table, "w") as f:
                    json.dump(table, f, indent=1, sort_keys=True)
        if args.full and not args.no_cpu_baseline and world == 1:   # reported baseline: rank 0 at N = 1 only
            out["cpu_baseline"] = cpu_baseline_leg(net, device)
        if args.full:
            try:
                out["box_calibration"] = box_calibration(device)
                cal = out["box_calibration"]
                if "unet_forward_ms_per_ddim_step_bs%d" % per_gpu in out and cal.get("ratio_to_r06_evidence_box", {}).get("gemm_8192_tflops"):
                    # the forward is MFMA-side work: its time on the evidence box's clock
                    out["unet_forward_ms_normalised_to_r06_box"] = round(
                        out["unet_forward_ms_per_ddim_step_bs%d" % per_gpu] * cal["ratio_to_r06_evidence_box"]["gemm_8192_tflops"], 3)
            except Exception as e:   # never lose the line over the calibration leg
                out["box_calibration"] = {"error": str(e)}
    if args.full and world == 1 and args.workload == "t2i" and args.batch is None and not args.no_other_workloads:
        # BASELINE configs[2..4] on this GPU, after (and outside) the headline's timed region: a --full run gives those
        # configurations a number from the same command as well
        others = {}
        del ctxs, images, img
        for name in ("i2v", "dual", "triple"):
            w2 = WORKLOADS[name]
            sampler.release_graphs()
            torch.cuda.empty_cache()
            pg = default_per_gpu(w2)
            ng, c2, im2 = workload_inputs(w2, pg, world, rank, device)
            sec, im = timed_batches(net, sampler, w2, c2, ng, args.ddim_steps, im2, 1, 2, barrier)
            px2 = 8 * w2["side"]
            assert im.shape == (ng, 3, px2, px2) and bool(torch.isfinite(im).all())
            nst = int(args.ddim_steps * (1 - FIDELITY)) if w2["vae_enc"] else args.ddim_steps
            tf = pg * (2 * nst * w2["gf_fwd"] + w2["vae_dec"] + w2["vae_enc"]) / 1e3
            others[name] = {"config": "BASELINE configs[%d]: %s" % (w2["cfg"], w2["desc"]), "value": round(ng * 2 / sec, 4),
                            "unit": "images/s", "metric": "%dx%d images/sec (50-step DDIM)" % (px2, px2), "n_gpus": world,
                            "bs_per_gpu": pg, "steps": 2, "warmup": 1, "ms_per_step": round(1e3 * sec / 2, 2), "scaling": "weak",
                            "whole_path_frac_of_mfma_peak": round(tf / (sec / 2) / MFMA_FP16_PEAK_TFLOPS, 4)}
            if not args.no_roofline:   # one guided DDIM step of this workload replayed from a HIP graph (as the headline's metric ii)
                ms2 = graph_step_ms(net, sampler, w2, pg, args.ddim_steps, device, reps=10)
                if ms2 is not None:
                    others[name]["unet_forward_ms_per_ddim_step"] = round(ms2, 3)
                    others[name]["unet_forward_frac_of_mfma_peak"] = round(2 * pg * w2["gf_fwd"] / ms2 / MFMA_FP16_PEAK_TFLOPS, 4)
                    others[name]["library_calls_per_ddim_step"] = getattr(graph_step_ms, "lib_calls", None)
            del c2, im2, im
        out["other_workloads"] = others
    if rank == 0:
        print(json.dumps(out))
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
