"""End-to-end parity of the HIP path (through the C ABI) against (1) the golden fixtures the reference produced
and (2) the CPU fp32 oracle on full-width models.

Tolerance: the path computes in fp16 with fp32 accumulation/statistics; BASELINE.json's north star bounds the
final latents at <= 1e-2 relative L2 vs the fp32 reference.  Single forwards are held to 5e-3.
"""
import threading

import numpy as np
import pytest
import torch

from vdtest_util import (clear_pack_caches, delayed_pack_builds, full_vd_cfg, load_gold, meta, rel_l2, synth_into, tiny_vd_cfg,
                         unet_middle)

pytestmark = pytest.mark.gpu

FWD_TOL = 5e-3
LATENT_TOL = 1e-2


def T(a, dev, dtype=torch.float16):
    return torch.from_numpy(np.asarray(a)).to(dev).to(dtype)


@pytest.fixture(scope="module")
def tiny(dev):
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    synth_into(net, m["seed"])
    net = net.half()
    net.to(dev)
    return net


def test_tiny_unet_vs_golden(tiny, dev):
    g = load_gold("unet_tiny.npz")
    x, t = T(g["x"], dev), torch.from_numpy(g["t"]).to(dev)
    e = tiny.apply_model({"type": "image", "x": x}, t, {"type": "text", "c": T(g["c_text"], dev)})
    assert e.shape == x.shape and e.dtype == torch.float16
    assert rel_l2(e, g["eps_text"]) < FWD_TOL
    e = tiny.apply_model({"type": "image", "x": x}, t, {"type": "image", "c": T(g["c_img"], dev)})
    assert rel_l2(e, g["eps_image"]) < FWD_TOL
    e = tiny.apply_model_multicontext({"type": "image", "x": x}, t, [
        {"type": "text", "c": T(g["c_text"], dev), "ratio": 0.4}, {"type": "image", "c": T(g["c_img"], dev), "ratio": 0.6}])
    assert rel_l2(e, g["eps_mix"]) < FWD_TOL
    # fp32 callers get fp32 back (compute stays fp16)
    e32 = tiny.apply_model({"type": "image", "x": x.float()}, t, {"type": "text", "c": T(g["c_text"], dev, torch.float32)})
    assert e32.dtype == torch.float32 and rel_l2(e32, g["eps_text"]) < FWD_TOL


def test_tiny_text_latent_flow_vs_golden(tiny, dev):
    """0-D (text-latent) data flow, SURVEY 8f-4: data blocks of diffuser['text'], context blocks of the context's type."""
    g = load_gold("unet0d_tiny.npz")
    x, t = T(g["x"], dev), torch.from_numpy(g["t"]).to(dev)
    e = tiny.apply_model({"type": "text", "x": x}, t, {"type": "image", "c": T(g["c_img"], dev)})
    assert e.shape == x.shape and e.dtype == torch.float16
    assert rel_l2(e, g["eps_image"]) < FWD_TOL
    e = tiny.apply_model({"type": "text", "x": x}, t, {"type": "text", "c": T(g["c_text"], dev)})
    assert rel_l2(e, g["eps_text"]) < FWD_TOL


def test_tiny_text_latent_ddim_vs_oracle(tiny, dev):
    """DDIM loop over the 768-d style text latent ([B, D] instead of [B, 4, h, w]) with CFG, image context."""
    from lib.model_zoo.ddim import DDIMSampler
    from oracle import synth, vd_oracle as O
    m = meta()
    g = load_gold("unet0d_tiny.npz")
    sd = synth.synth_state_dict(synth.shapes_of(tiny), m["seed"])
    sd.update(O.register_schedule())
    xT = torch.randn((2, 128), generator=torch.Generator().manual_seed(31))
    c, u = torch.from_numpy(g["c_img"]), torch.zeros_like(torch.from_numpy(g["c_img"]))
    with torch.no_grad():
        zr, _ = O.ddim_sample(sd, O.unet0d_plan(**m["unet0d"]), sd["alphas_cumprod"], xT,
                              [{"type": "image", "conditioning": c, "unconditional_conditioning": u}], 5, 4.0,
                              x_type="text", global_ptr="image")
    z, _ = DDIMSampler(tiny).sample(steps=5, shape=[2, 128], x_info={"type": "text", "xt": xT.half().to(dev)},
                                    c_info={"type": "image", "conditioning": c.half().to(dev),
                                            "unconditional_conditioning": u.half().to(dev),
                                            "unconditional_guidance_scale": 4.0}, eta=0., verbose=False)
    assert z.shape == (2, 128)
    assert rel_l2(z, zr) < LATENT_TOL


def test_guidance_replica_sharing_matches_explicit_batch(tiny, dev):
    """apply_model*(x, repeat=2) == apply_model*([x; x]): the data blocks in front of the first context block run once per
    sample instead of once per CFG replica; everything downstream sees the same tensors."""
    g = load_gold("unet_tiny.npz")
    x = T(g["x"], dev)[:1].repeat(2, 1, 1, 1)[:1]          # one sample
    c2 = torch.cat([T(g["c_text"], dev)[:1] * 0.0, T(g["c_text"], dev)[:1]])   # [uncond; cond] contexts
    t2 = torch.full((2,), 501, device=dev, dtype=torch.long)
    ref = tiny.apply_model({"type": "image", "x": torch.cat([x, x])}, t2, {"type": "text", "c": c2})
    out = tiny.apply_model({"type": "image", "x": x, "repeat": 2}, t2, {"type": "text", "c": c2})
    assert out.shape == ref.shape == (2, 4, 16, 16)
    assert rel_l2(out, ref) < 1e-3   # same kernels on the same values; GroupNorm's LDS atomics may reorder sums
    ci = T(g["c_img"], dev)[:1]
    specs = lambda: [{"type": "text", "c": c2, "ratio": 0.4}, {"type": "image", "c": torch.cat([ci * 0, ci]), "ratio": 0.6}]
    ref = tiny.apply_model_multicontext({"type": "image", "x": torch.cat([x, x])}, t2, specs())
    out = tiny.apply_model_multicontext({"type": "image", "x": x, "repeat": 2}, t2, specs())
    assert rel_l2(out, ref) < 1e-3


def test_tiny_ddim_vs_golden(tiny, dev, monkeypatch):
    from lib.model_zoo.ddim import DDIMSampler
    g = load_gold("ddim_tiny.npz")
    sampler = DDIMSampler(tiny)
    xT = T(g["xT"], dev)
    monkeypatch.setattr(torch, "randn", lambda *a, **k: xT.clone())
    ct = {"type": "text", "conditioning": T(g["c_text"], dev), "unconditional_conditioning": T(g["u_text"], dev),
          "unconditional_guidance_scale": 7.5}
    z, inter = sampler.sample(steps=5, shape=[2, 4, 16, 16], x_info={"type": "image"}, c_info=ct, eta=0., verbose=False)
    assert rel_l2(z, g["z_t2i"]) < LATENT_TOL
    assert rel_l2(inter["pred_x0"][-1], g["pred_x0_t2i"]) < LATENT_TOL
    ci = {"type": "image", "conditioning": T(g["c_img"], dev), "unconditional_conditioning": T(g["u_img"], dev)}
    zm, _ = sampler.sample_multicontext(steps=4, shape=[2, 4, 16, 16], x_info={"type": "image"}, c_info_list=[
        dict(ct, unconditional_guidance_scale=5.0, ratio=0.4), dict(ci, unconditional_guidance_scale=5.0, ratio=0.6)],
        eta=0., verbose=False)
    assert rel_l2(zm, g["z_mc"]) < LATENT_TOL
    monkeypatch.undo()
    zi, _ = sampler.sample(steps=5, shape=[2, 4, 16, 16],
                           x_info={"type": "image", "x0": T(g["x0"], dev), "x0_forward_timesteps": 3,
                                   "x0_noise": T(g["q_noise"], dev)},
                           c_info=dict(ci, unconditional_guidance_scale=1.0), eta=0., verbose=False)
    assert rel_l2(zi, g["z_i2i"]) < LATENT_TOL


def test_graph_reuse_across_sample_calls(tiny, dev, monkeypatch):
    """A sampler keeps the captured DDIM step across sample() calls of the same geometry (static latent / context / K-V
    buffers refreshed in place).  Calls 2 and 3 -- new context, new start latent, another guidance scale and step count --
    must give what a fresh sampler (fresh capture) gives (to run-to-run rounding: GroupNorm folds its partial sums with
    LDS float atomics, so two runs differ in the last bit; a stale context or latent would be an O(1) error); the fixture
    result must still come out of call 1; a weight update must invalidate the kept graph."""
    from lib.model_zoo.ddim import DDIMSampler
    g = load_gold("ddim_tiny.npz")
    shared = DDIMSampler(tiny)
    gen = torch.Generator().manual_seed(77)

    def case(k):
        if k == 0:
            return T(g["xT"], dev), T(g["c_text"], dev), T(g["u_text"], dev), 7.5, 5
        xT = torch.randn((2, 4, 16, 16), generator=gen).half().to(dev)
        c = (torch.randn(tuple(g["c_text"].shape), generator=gen) * 0.5).half().to(dev)
        u = (torch.randn(tuple(g["u_text"].shape), generator=gen) * 0.5).half().to(dev)
        return xT, c, u, (3.0, 9.0)[k % 2], (4, 6)[k % 2]

    def run(sampler, xT, c, u, scale, steps):
        monkeypatch.setattr(torch, "randn", lambda *a, **k: xT.clone())
        z, _ = sampler.sample(steps=steps, shape=[2, 4, 16, 16], x_info={"type": "image"}, eta=0., verbose=False,
                              c_info={"type": "text", "conditioning": c, "unconditional_conditioning": u,
                                      "unconditional_guidance_scale": scale})
        monkeypatch.undo()
        return z

    outs = []
    for k in range(3):
        args = case(k)
        z = run(shared, *args)
        outs.append(z.clone())
        assert rel_l2(z, run(DDIMSampler(tiny), *args)) < 5e-3, k
        if k == 0:
            assert rel_l2(z, g["z_t2i"]) < LATENT_TOL
    assert len(shared._static) == 1 and next(iter(shared._static.values()))["graph"] is not None
    assert rel_l2(outs[0], run(shared, *case(0))) < 5e-3        # earlier results were not overwritten, same input -> same output
    assert rel_l2(outs[1], outs[0]) > 0.1 and rel_l2(outs[2], outs[1]) > 0.1   # the three cases really differ
    # in-place weight change: the kept graph must not be replayed against stale packed weights -> new state, new capture
    keys_before = set(shared._static)
    w = tiny.diffuser["image"].data_blocks[1][0].in_layers[2].weight
    w0 = w.detach().clone()
    with torch.no_grad():
        w.mul_(1.5)
    try:
        args = case(0)
        z_new = run(shared, *args)
        assert set(shared._static) != keys_before
        assert rel_l2(z_new, run(DDIMSampler(tiny), *args)) < 5e-3
    finally:
        with torch.no_grad():
            w.copy_(w0)


def test_tiny_vae_vs_golden(tiny, dev):
    g = load_gold("vae_tiny.npz")
    img = T(g["img"], dev)
    post = tiny.vae["image"].encode(img, out_posterior=True)
    assert rel_l2(post.parameters, g["moments"]) < FWD_TOL
    z = tiny.vae["image"].encode_scaled(img, 0.18215, noise=torch.from_numpy(g["post_noise"]))
    assert rel_l2(z, g["z"]) < FWD_TOL
    dec = tiny.vae_decode(T(g["z"], dev), which="image")
    assert dec.shape == (2, 3, 32, 32) and float(dec.min()) >= 0 and float(dec.max()) <= 1
    assert rel_l2(dec, g["dec"]) < FWD_TOL
    assert rel_l2(tiny.vae_decode(T(g["zlat"], dev), which="image"), g["dec2"]) < FWD_TOL


def test_tiny_clip_vs_golden(dev):
    from lib.model_zoo.clip import CLIPImageContextEncoder, CLIPTextContextEncoder
    from oracle import synth
    m = meta()
    g = load_gold("clip_tiny.npz")
    tc, vc = m["clip"]["text_config"], m["clip"]["vision_config"]
    cfg = dict(text={k: tc[k] for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers",
                                        "num_attention_heads", "max_position_embeddings")},
               vision={k: vc[k] for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                                          "image_size", "patch_size")}, projection_dim=m["clip"]["projection_dim"])
    tenc = CLIPTextContextEncoder(config=cfg, fp16=True, max_length=24)
    sd = synth.synth_state_dict({"ctx.text.model." + k: v for k, v in synth.shapes_of(tenc.model).items()}, m["seed"])
    tenc.model.load_state_dict({k[len("ctx.text.model."):]: v for k, v in sd.items()}, strict=True)
    tenc = tenc.half().to(dev)
    z = tenc.encode(torch.from_numpy(g["input_ids"]))
    assert rel_l2(z, g["z_text"]) < FWD_TOL
    ienc = CLIPImageContextEncoder(config=cfg, fp16=True)
    ienc.model.load_state_dict(tenc.model.state_dict())
    ienc = ienc.half().to(dev)
    px = torch.randn((3, 3, 224, 224), generator=torch.Generator().manual_seed(int(g["px_seed"])))
    assert rel_l2(ienc.encode_pixels(px), g["z_img"]) < FWD_TOL
    ts = ienc.vtoken_mask(torch.from_numpy(g["masks"]).to(dev))
    assert ts is not None
    assert rel_l2(ienc.encode_pixels(px, ts), g["z_img_masked"]) < FWD_TOL


@pytest.fixture(scope="module")
def full(dev):
    from lib.model_zoo import get_model
    net = get_model()(full_vd_cfg(with_vae=True), verbose=False)
    sd = synth_into(net, 7)
    net = net.half()
    net.to(dev)
    return net, sd


def test_full_unet_forward_vs_oracle(full, dev):
    """Full-width openai_unet_2d_v1 (859.5 M params) + text context blocks of the 0D net, 32x32 latent, CFG batch 2."""
    from oracle import vd_oracle as O
    net, sd = full
    assert sum(p.numel() for p in net.diffuser["image"].parameters()) == 859520964
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 4, 32, 32), generator=g)
    c = torch.randn((2, 77, 768), generator=g) * 0.5
    t = torch.tensor([741, 741])
    with torch.no_grad():
        ref = O.apply_model(sd, O.unet_plan(), x, t, c, c_type="text", global_ptr="image")
    e = net.apply_model({"type": "image", "x": x.half().to(dev)}, t.to(dev), {"type": "text", "c": c.half().to(dev)})
    assert rel_l2(e, ref) < FWD_TOL
    c2 = torch.randn((2, 257, 768), generator=g) * 0.5
    with torch.no_grad():
        ref2 = O.apply_model_multicontext(sd, O.unet_plan(), x, t, [("text", c, 0.5), ("image", c2, 0.5)])
    e2 = net.apply_model_multicontext({"type": "image", "x": x.half().to(dev)}, t.to(dev), [
        {"type": "text", "c": c.half().to(dev), "ratio": 0.5}, {"type": "image", "c": c2.half().to(dev), "ratio": 0.5}])
    assert rel_l2(e2, ref2) < FWD_TOL


def test_half_batch_branches_match_the_unforked_forward(full, dev, monkeypatch):
    """vd.BATCH_FORK: the 16x16 / 8x8 levels as two forked half-batch branches (default for batches of >= 16 samples with one
    context type) against the same forward without the fork -- same kernels on the same values per sample, other split-K
    factors and statistics partials for the smaller batch, so agreement to the fp16 noise of a forward (the oracle tests put that
    at FWD_TOL), eager and inside a captured graph; a multi-context forward is not forked (its context types are)."""
    from lib.model_zoo import vd
    net, _ = full
    g = torch.Generator().manual_seed(21)
    x = (torch.randn((4, 4, 64, 64), generator=g)).half().to(dev)   # (64x64: the geometry whose forward is bit-reproducible run to run)
    c = (torch.randn((4, 77, 768), generator=g) * 0.5).half().to(dev)
    t = torch.tensor([741, 741, 301, 301], device=dev)
    fwd = lambda: net.apply_model({"type": "image", "x": x}, t, {"type": "text", "c": c})
    monkeypatch.setattr(vd, "BATCH_FORK", "0")
    ref = fwd().float()
    monkeypatch.setattr(vd, "BATCH_FORK", "1")
    out = fwd().float()
    assert rel_l2(out, ref) < FWD_TOL and not torch.equal(out, ref)   # (the fork did run: other split factors -> other roundings)
    again = fwd().float()
    assert torch.equal(out, again)                                    # run-to-run identical
    # captured and replayed (the sampler's step graph): the side branch must join the capture
    fwd(); torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        cap = fwd()
    gr.replay(); torch.cuda.synchronize()
    assert rel_l2(cap.float(), ref) < FWD_TOL
    c2 = (torch.randn((4, 257, 768), generator=g) * 0.5).half().to(dev)
    multi = lambda: net.apply_model_multicontext({"type": "image", "x": x}, t, [
        {"type": "text", "c": c, "ratio": 0.5}, {"type": "image", "c": c2, "ratio": 0.5}]).float()
    m1 = multi()
    monkeypatch.setattr(vd, "BATCH_FORK", "0")
    assert torch.equal(m1, multi())


def test_half_batch_branches_after_an_in_place_weight_edit(full, dev, monkeypatch):
    """The geometry above after an in-place edit of one 8x8-level convolution and the FeedForward output projection of the
    middle block (their weight-stream packs): the main branch rebuilds the packs on its stream, and the side branch must
    read the rebuilt ones (tests/test_streams_gpu.py has the tiny-model cases; weights restored afterwards)."""
    from lib.model_zoo import vd
    net, _ = full
    g = torch.Generator().manual_seed(21)
    x = (torch.randn((4, 4, 64, 64), generator=g)).half().to(dev)
    c = (torch.randn((4, 77, 768), generator=g) * 0.5).half().to(dev)
    t = torch.tensor([741, 741, 301, 301], device=dev)
    fwd = lambda: net.apply_model({"type": "image", "x": x}, t, {"type": "text", "c": c}).float()
    monkeypatch.setattr(vd, "BATCH_FORK", "0")
    r0 = fwd()
    assert torch.equal(r0, fwd()), "geometry not bit-reproducible run to run"
    monkeypatch.setattr(vd, "BATCH_FORK", "1")
    fwd()
    rb, st = unet_middle(net.diffuser["image"])
    ws = [rb.in_layers[2].weight, st.transformer_blocks[0].ff.net[2].weight]
    saved = [w.detach().clone() for w in ws]
    try:
        with torch.no_grad():
            ws[0].mul_(0.75)
            ws[1].mul_(1.25)
        with delayed_pack_builds() as amp:
            first = fwd()
        assert amp.builds > 0
        second = fwd()
        assert torch.equal(first, second)
        clear_pack_caches(net)          # every pack rebuilt from the edited weights, unforked: the fresh-net reference
        monkeypatch.setattr(vd, "BATCH_FORK", "0")
        ref = fwd()
        assert not torch.equal(ref, r0)
        assert rel_l2(second, ref) < FWD_TOL
    finally:
        with torch.no_grad():
            for w, s0 in zip(ws, saved):
                w.copy_(s0)


def test_two_threads_fork_onto_their_own_side_streams(full, dev, monkeypatch):
    """Two threads, each running dual-context forwards (context types forked onto side streams) on a stream of its own once
    the weights have been used: every output equals the same call run alone.  At this geometry the side branch's long-K
    projections take split-K launches whose slabs live in a per-stream workspace, so threads that shared a side stream would
    interleave slab writes and reduces."""
    from lib.model_zoo import vd
    from vd_hip import ops
    net, _ = full
    g = torch.Generator().manual_seed(23)
    t = torch.tensor([741, 301], device=dev)
    inputs = [[(torch.randn((2, 4, 32, 32), generator=g).half().to(dev), (torch.randn((2, 77, 768), generator=g) * 0.5).half().to(dev),
                (torch.randn((2, 257, 768), generator=g) * 0.5).half().to(dev)) for _ in range(4)] for _ in range(2)]
    fwd = lambda x, ct, ci: net.apply_model_multicontext({"type": "image", "x": x}, t, [
        {"type": "text", "c": ct, "ratio": 0.5}, {"type": "image", "c": ci, "ratio": 0.5}]).float()
    alone = [[fwd(*inp) for inp in per] for per in inputs]
    assert torch.equal(alone[0][0], fwd(*inputs[0][0])), "geometry not bit-reproducible run to run"
    torch.cuda.synchronize()
    slabs = []
    real_ws = ops.workspace

    def workspace(nbytes, device, tag="ws"):
        if tag == "gemm":   # split-K slabs (the reduce reads them back)
            slabs.append((threading.get_ident(), torch.cuda.current_stream().cuda_stream))
        return real_ws(nbytes, device, tag)
    monkeypatch.setattr(ops, "workspace", workspace)
    outs, sides, mains, idents, errors = [None, None], [None, None], [None, None], [None, None], []
    start = threading.Barrier(2)

    def worker(k):
        try:
            s = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(s):
                idents[k], mains[k] = threading.get_ident(), s.cuda_stream
                sides[k] = {st.cuda_stream for st in vd._side_streams(dev, 1)}
                start.wait(timeout=60)
                outs[k] = [fwd(*inp) for inp in inputs[k]]
            s.synchronize()
        except BaseException as e:   # re-raised in the test thread
            errors.append(e)
    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
    assert not any(th.is_alive() for th in threads)
    if errors:
        raise errors[0]
    differ = [(k, j) for k in range(2) for j in range(4) if not torch.equal(outs[k][j], alone[k][j])]
    assert not sides[0] & sides[1], "both threads fork onto side stream(s) %s (outputs that differ from the lone run: %s)" % (
        sides[0] & sides[1], differ)
    assert not (sides[0] | sides[1]) & {mains[0], mains[1]}
    for k in range(2):
        assert any(tid == idents[k] and sid in sides[k] for tid, sid in slabs), "no split-K launch on thread %d's side stream" % k
    assert not differ, differ


def test_bench_shape_forward_vs_oracle(full, dev):
    """The exact shape bench.py times (BASELINE configs[1]): CFG batch 8, 64x64 latent, L = 77 -- so the tile / split
    choices, the 128x320 tile of the 64x64 level and the attention kernel at N = 4096 are checked at full width."""
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(11)
    x = torch.randn((8, 4, 64, 64), generator=g)
    c = torch.randn((8, 77, 768), generator=g) * 0.5
    t = torch.tensor([981, 981, 501, 501, 21, 21, 1, 1])
    with torch.no_grad():
        ref = O.apply_model(sd, O.unet_plan(), x, t, c, c_type="text", global_ptr="image")
    e = net.apply_model({"type": "image", "x": x.half().to(dev)}, t.to(dev), {"type": "text", "c": c.half().to(dev)})
    assert rel_l2(e, ref) < FWD_TOL


def test_c5_shape_dual_context_vs_oracle(full, dev):
    """BASELINE configs[4] geometry: 96x96 latent (768x768 image, N = 9216 tokens), text (L = 77, ratio 0.4) + two
    masked-image contexts concatenated (L = 514, ratio 0.6); ragged key tiles (514 = 8*64 + 2) and M = 9216 GEMMs."""
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(12)
    x = torch.randn((1, 4, 96, 96), generator=g)
    ct = torch.randn((1, 77, 768), generator=g) * 0.5
    ci = torch.randn((1, 514, 768), generator=g) * 0.5
    t = torch.tensor([641])
    with torch.no_grad():
        ref = O.apply_model_multicontext(sd, O.unet_plan(), x, t, [("text", ct, 0.4), ("image", ci, 0.6)])
    e = net.apply_model_multicontext({"type": "image", "x": x.half().to(dev)}, t.to(dev), [
        {"type": "text", "c": ct.half().to(dev), "ratio": 0.4}, {"type": "image", "c": ci.half().to(dev), "ratio": 0.6}])
    assert e.shape == (1, 4, 96, 96)
    assert rel_l2(e, ref) < FWD_TOL


def test_full_vae_vs_oracle(full, dev):
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(5)
    z = torch.randn((1, 4, 32, 32), generator=g)
    with torch.no_grad():
        ref = O.vae_decode(sd, "vae.image", z / 0.18215)
    dec = net.vae_decode(z.half().to(dev), which="image")
    assert dec.shape == (1, 3, 256, 256)
    assert rel_l2(dec, ref) < FWD_TOL
    img = torch.rand((1, 3, 256, 256), generator=g)
    nz = torch.randn((1, 4, 32, 32), generator=g)
    with torch.no_grad():
        zref = O.diag_gaussian_sample(O.vae_encode_moments(sd, "vae.image", img), nz) * 0.18215
    zz = net.vae["image"].encode_scaled(img.half().to(dev), 0.18215, noise=nz)
    assert rel_l2(zz, zref) < FWD_TOL


def test_ddim_full_latent_parity(full, dev, monkeypatch):
    """North-star bound: final latents after a guided DDIM loop within 1e-2 rel-L2 of the fp32 reference path
    (full-width UNet, 16x16 latent to keep the CPU oracle in seconds, 6 steps, CFG 7.5)."""
    from lib.model_zoo.ddim import DDIMSampler
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(11)
    xT = torch.randn((1, 4, 16, 16), generator=g)
    c = torch.randn((1, 77, 768), generator=g) * 0.5
    u = torch.randn((1, 77, 768), generator=g) * 0.5
    steps = 5
    with torch.no_grad():
        zref, _ = O.ddim_sample(sd, O.unet_plan(), sd["alphas_cumprod"], xT,
                                [{"type": "text", "conditioning": c, "unconditional_conditioning": u}], steps, 7.5,
                                global_ptr="image")
    monkeypatch.setattr(torch, "randn", lambda *a, **k: xT.half().to(dev))
    z, _ = DDIMSampler(net).sample(steps=steps, shape=[1, 4, 16, 16], x_info={"type": "image"},
                                   c_info={"type": "text", "conditioning": c.half().to(dev),
                                           "unconditional_conditioning": u.half().to(dev),
                                           "unconditional_guidance_scale": 7.5}, eta=0., verbose=False)
    assert rel_l2(z, zref) < LATENT_TOL


def test_c1_geometry_ddim_parity(full, dev, monkeypatch):
    """BASELINE configs[0] geometry (the reference's own CPU-runnable case): 1 prompt, 64x64x4 latent, L = 77, 10 guided
    DDIM steps, full-width model -- final latent within the north-star bound of the fp32 path."""
    from lib.model_zoo.ddim import DDIMSampler
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(21)
    xT = torch.randn((1, 4, 64, 64), generator=g)
    c = torch.randn((1, 77, 768), generator=g) * 0.5
    u = torch.randn((1, 77, 768), generator=g) * 0.5
    with torch.no_grad():
        zref, _ = O.ddim_sample(sd, O.unet_plan(), sd["alphas_cumprod"], xT,
                                [{"type": "text", "conditioning": c, "unconditional_conditioning": u}], 10, 7.5,
                                global_ptr="image")
    monkeypatch.setattr(torch, "randn", lambda *a, **k: xT.half().to(dev))
    z, _ = DDIMSampler(net).sample(steps=10, shape=[1, 4, 64, 64], x_info={"type": "image"},
                                   c_info={"type": "text", "conditioning": c.half().to(dev),
                                           "unconditional_conditioning": u.half().to(dev),
                                           "unconditional_guidance_scale": 7.5}, eta=0., verbose=False)
    assert rel_l2(z, zref) < LATENT_TOL


def test_full_clip_vs_oracle(dev):
    """CLIP ViT-L/14 towers at full size (427.6 M parameters per encoder object) against the CPU oracle."""
    from lib.model_zoo.clip import CLIPImageContextEncoder, CLIPTextContextEncoder
    from oracle import synth, vd_oracle as O
    tenc = CLIPTextContextEncoder(fp16=True)
    assert sum(p.numel() for p in tenc.model.parameters()) == 427616513
    shapes = {"ctx.text.model." + k: v for k, v in synth.shapes_of(tenc.model).items()}
    sd = synth.synth_state_dict(shapes, 21)
    tenc.model.load_state_dict({k[len("ctx.text.model."):]: v for k, v in sd.items()}, strict=True)
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(1000, 49000, (2, 77), generator=g)
    for b, e in enumerate((9, 76)):
        ids[b, e] = 49407
        ids[b, e + 1:] = 0
    with torch.no_grad():
        zt_ref = O.clip_text_context(sd, "ctx.text.model", ids, 12, 12)
    tenc = tenc.half().to(dev)
    zt = tenc.encode(ids)
    assert zt.shape == (2, 77, 768)
    assert rel_l2(zt, zt_ref) < FWD_TOL
    ienc = CLIPImageContextEncoder(fp16=True)
    ienc.model.load_state_dict(tenc.model.state_dict())
    ienc = ienc.half().to(dev)
    del tenc
    px = torch.randn((2, 3, 224, 224), generator=g)
    masks = (torch.rand((2, 1, 96, 96), generator=g) > 0.5).float()
    with torch.no_grad():
        zi_ref = O.clip_image_context(sd, "ctx.text.model", px, 16, 24)
        vt, _ = O.clip_vtoken_mask(masks)
        zm_ref = O.clip_image_context(sd, "ctx.text.model", px, 16, 24, vtoken_mask=vt)
    zi = ienc.encode_pixels(px)
    assert zi.shape == (2, 257, 768)
    assert rel_l2(zi, zi_ref) < FWD_TOL
    zm = ienc.encode_pixels(px, ienc.vtoken_mask(masks.to(dev)))
    assert rel_l2(zm, zm_ref) < FWD_TOL
    # the reference-style entry point with raw images runs end to end (pre-processing on the device)
    img = torch.rand((2, 3, 512, 512), generator=g)
    z = ienc.encode(img.half().to(dev))
    assert z.shape == (2, 257, 768) and bool(torch.isfinite(z).all())


def test_image_variation_and_multicontext_flows(full, dev):
    """BASELINE configs 3-5 in miniature on the full-width model, as PARITY tests against the oracle's DDIM loop:
    image-variation (VAE encode -> q_sample with injected noise -> partial DDIM under an image context) and triple-context
    sampling (text + 2 concatenated image contexts, 514 tokens) at a 96x96 latent (768x768), 2 guided steps (the fp32 oracle needs
    ~12 s per guided step at this geometry; the multi-step multi-context loop is test_dual_context_guided_10_step_graph_loop_batch2_
    vs_oracle), graph replay and eager."""
    from lib.model_zoo.ddim import DDIMSampler
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(17)
    sampler = DDIMSampler(net)
    # C3: image variation with fidelity: encode (posterior sample with injected noise) -> 4 of 10 steps from q_sample(x0)
    img = torch.rand((2, 3, 256, 256), generator=g)
    nz_post = torch.randn((2, 4, 32, 32), generator=g)
    nz_q = torch.randn((2, 4, 32, 32), generator=g)
    ci = torch.randn((2, 257, 768), generator=g) * 0.5
    ui = torch.zeros_like(ci)
    steps, k = 10, 4
    with torch.no_grad():
        x0_ref = O.diag_gaussian_sample(O.vae_encode_moments(sd, "vae.image", img), nz_post) * 0.18215
        sched = O.ddim_schedule(sd["alphas_cumprod"], steps, 0.0)
        ts = torch.full((2,), int(sched["timesteps"][k]), dtype=torch.long)
        zref, _ = O.ddim_sample(sd, O.unet_plan(), sd["alphas_cumprod"], O.q_sample(sd, x0_ref, ts, nz_q),
                                [{"type": "image", "conditioning": ci, "unconditional_conditioning": ui}], steps, 7.5,
                                global_ptr="image", forward_steps=k)
        out_ref = O.vae_decode(sd, "vae.image", zref / 0.18215)
    x0 = net.vae["image"].encode_scaled(img.half().to(dev), 0.18215, noise=nz_post)
    assert x0.shape == (2, 4, 32, 32) and rel_l2(x0, x0_ref) < FWD_TOL
    z, _ = sampler.sample(steps=steps, shape=[2, 4, 32, 32],
                          x_info={"type": "image", "x0": x0, "x0_forward_timesteps": k, "x0_noise": nz_q.half().to(dev)},
                          c_info={"type": "image", "conditioning": ci.half().to(dev), "unconditional_conditioning": ui.half().to(dev),
                                  "unconditional_guidance_scale": 7.5}, eta=0., verbose=False)
    assert z.shape == (2, 4, 32, 32) and rel_l2(z, zref) < LATENT_TOL
    out = net.vae_decode(z, which="image")
    assert out.shape == (2, 3, 256, 256) and rel_l2(out, out_ref) < 2 * LATENT_TOL
    # C4 / C5: text + (2 masked images -> 514 tokens) at 96x96 latent, 2 guided steps
    ct = torch.randn((1, 77, 768), generator=g) * 0.5
    ut = torch.randn((1, 77, 768), generator=g) * 0.5
    c2 = torch.randn((1, 514, 768), generator=g) * 0.5
    xT = torch.randn((1, 4, 96, 96), generator=g)
    with torch.no_grad():
        zr, _ = O.ddim_sample(sd, O.unet_plan(), sd["alphas_cumprod"], xT,
                              [{"type": "text", "conditioning": ct, "unconditional_conditioning": ut, "ratio": 0.4},
                               {"type": "image", "conditioning": c2, "unconditional_conditioning": torch.zeros_like(c2), "ratio": 0.6}],
                              2, 7.5, global_ptr="image")
    h = lambda t: t.half().to(dev)
    cl = lambda: [{"type": "text", "conditioning": h(ct), "unconditional_conditioning": h(ut), "unconditional_guidance_scale": 7.5, "ratio": 0.4},
                  {"type": "image", "conditioning": h(c2), "unconditional_conditioning": torch.zeros_like(h(c2)), "unconditional_guidance_scale": 7.5, "ratio": 0.6}]
    zg, _ = sampler.sample_multicontext(steps=2, shape=[1, 4, 96, 96], x_info={"type": "image", "xt": h(xT).clone()},
                                        c_info_list=cl(), eta=0., verbose=False)
    sampler.use_graph = False
    ze, _ = sampler.sample_multicontext(steps=2, shape=[1, 4, 96, 96], x_info={"type": "image", "xt": h(xT).clone()},
                                        c_info_list=cl(), eta=0., verbose=False)
    assert zg.shape == (1, 4, 96, 96) and rel_l2(zg, zr) < LATENT_TOL and rel_l2(ze, zr) < LATENT_TOL
    # same kernels either way; GroupNorm's LDS float atomics make the last bit order-dependent, so compare to rounding
    assert rel_l2(zg, ze) < 2e-3, "HIP-graph replay and eager launches must agree"


def _replicated(t, times):
    return t.repeat(times, *([1] * (t.dim() - 1)))


def test_c4_per_gpu_shape_forward_vs_oracle(full, dev):
    """BASELINE configs[3] as one rank sees it: 16 samples over 8 GPUs = 2 samples, CFG batch 4, 64x64 latent, text (L = 77,
    ratio 0.5) + image (L = 257, ratio 0.5) contexts mixed.  The launch planner decides on (M, N, K), so the GPU runs the
    real CFG batch of 4; the oracle computes the two distinct samples once (the batch repeats them) -- every replica must
    match, whichever tiles / K slices it lands in."""
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(41)
    x = torch.randn((2, 4, 64, 64), generator=g)
    ct = torch.randn((2, 77, 768), generator=g) * 0.5
    ci = torch.randn((2, 257, 768), generator=g) * 0.5
    t = torch.tensor([801, 301])
    with torch.no_grad():
        ref = O.apply_model_multicontext(sd, O.unet_plan(), x, t, [("text", ct, 0.5), ("image", ci, 0.5)])
    r = 2
    e = net.apply_model_multicontext({"type": "image", "x": _replicated(x, r).half().to(dev)}, _replicated(t, r).to(dev), [
        {"type": "text", "c": _replicated(ct, r).half().to(dev), "ratio": 0.5},
        {"type": "image", "c": _replicated(ci, r).half().to(dev), "ratio": 0.5}])
    assert e.shape == (4, 4, 64, 64)
    assert rel_l2(e, _replicated(ref, r)) < FWD_TOL
    for k in range(r):
        assert rel_l2(e[2 * k:2 * k + 2], ref) < FWD_TOL, k


def test_c5_per_gpu_shape_forward_vs_oracle(full, dev):
    """BASELINE configs[4] as one rank sees it: 32 samples over 8 GPUs = 4 samples, CFG batch 8, 96x96 latent (768x768), text
    (L = 77, ratio 0.4) + two masked-image contexts (L = 514, ratio 0.6).  Two distinct samples repeated four times (see
    test_c4_per_gpu_shape_forward_vs_oracle): M = 73728-row GEMMs, 9216-token self-attention at batch 8, ragged key tiles."""
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(42)
    x = torch.randn((2, 4, 96, 96), generator=g)
    ct = torch.randn((2, 77, 768), generator=g) * 0.5
    ci = torch.randn((2, 514, 768), generator=g) * 0.5
    t = torch.tensor([641, 101])
    with torch.no_grad():
        ref = O.apply_model_multicontext(sd, O.unet_plan(), x, t, [("text", ct, 0.4), ("image", ci, 0.6)])
    r = 4
    e = net.apply_model_multicontext({"type": "image", "x": _replicated(x, r).half().to(dev)}, _replicated(t, r).to(dev), [
        {"type": "text", "c": _replicated(ct, r).half().to(dev), "ratio": 0.4},
        {"type": "image", "c": _replicated(ci, r).half().to(dev), "ratio": 0.6}])
    assert e.shape == (8, 4, 96, 96)
    for k in range(r):
        assert rel_l2(e[2 * k:2 * k + 2], ref) < FWD_TOL, k


@pytest.mark.parametrize("B,side", [(4, 64), (1, 96)])
def test_vae_decode_bench_shapes_vs_oracle(full, dev, B, side):
    """AutoencoderKL.decode at the shapes bench.py times: [4, 4, 64, 64] -> 512x512 (configs[1..3]) and [1, 4, 96, 96] ->
    768x768 (configs[4]): the mid-block attention over 4096 / 9216 tokens and the 3x3 convs at 512x512 / 768x768 x 128
    channels.  The oracle decodes ONE distinct latent (the 512x512 batch repeats it)."""
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(50 + side)
    z = torch.randn((1, 4, side, side), generator=g)
    with torch.no_grad():
        ref = O.vae_decode(sd, "vae.image", z / 0.18215)
    dec = net.vae_decode(_replicated(z, B).half().to(dev), which="image")
    assert dec.shape == (B, 3, 8 * side, 8 * side)
    for k in range(B):
        assert rel_l2(dec[k:k + 1], ref) < FWD_TOL, k


@pytest.mark.parametrize("B,H,W,L", [(1, 8, 8, 1), (3, 12, 20, 77), (2, 24, 8, 5)])
def test_tiny_unet_ragged_shapes_vs_oracle(tiny, dev, B, H, W, L):
    """Edge shapes the kernels must mask correctly: batch 1 / odd batch, non-square latents whose pixel count is not a
    multiple of any tile size, context lengths 1 and 5 (single ragged key tile)."""
    from oracle import synth, vd_oracle as O
    m = meta()
    sd = synth.synth_state_dict(synth.shapes_of(tiny), m["seed"])
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn((B, 4, H, W), generator=g)
    c = torch.randn((B, L, 128), generator=g) * 0.5
    t = torch.randint(1, 999, (B,), generator=g)
    with torch.no_grad():
        ref = O.apply_model(sd, O.unet_plan(**m["unet2d"]), x, t, c, c_type="text", global_ptr="image")
    e = tiny.apply_model({"type": "image", "x": x.half().to(dev)}, t.to(dev), {"type": "text", "c": c.half().to(dev)})
    assert e.shape == (B, 4, H, W)
    assert rel_l2(e, ref) < FWD_TOL


def test_sampler_eta_and_unguided_paths(tiny, dev):
    """eta > 0 (stochastic DDIM, eager steps) and guidance scale 1 (no CFG batch): finite, right shapes, seeded."""
    from lib.model_zoo.ddim import DDIMSampler
    g = load_gold("ddim_tiny.npz")
    sampler = DDIMSampler(tiny)
    ct = {"type": "text", "conditioning": T(g["c_text"], dev), "unconditional_conditioning": T(g["u_text"], dev)}
    outs = []
    for _ in range(2):
        torch.manual_seed(123)
        z, inter = sampler.sample(steps=5, shape=[2, 4, 16, 16], x_info={"type": "image"},
                                  c_info=dict(ct, unconditional_guidance_scale=3.0), eta=0.6, verbose=False, log_every_t=2)
        assert z.shape == (2, 4, 16, 16) and bool(torch.isfinite(z).all())
        assert len(inter["pred_x0"]) == 3  # indices 4, 2, 0
        outs.append(z)
    assert rel_l2(outs[0], outs[1]) < 2e-3  # same seed -> same trajectory (up to atomics order)
    z1, _ = sampler.sample(steps=4, shape=[2, 4, 16, 16], x_info={"type": "image", "xt": T(g["xT"], dev)},
                           c_info=dict(ct, unconditional_guidance_scale=1.0), eta=0., verbose=False)
    from oracle import synth, vd_oracle as O
    m = meta()
    sd = synth.synth_state_dict(synth.shapes_of(tiny), m["seed"])
    sd.update(O.register_schedule())
    with torch.no_grad():
        zr, _ = O.ddim_sample(sd, O.unet_plan(**m["unet2d"]), sd["alphas_cumprod"], torch.from_numpy(g["xT"]),
                              [{"type": "text", "conditioning": torch.from_numpy(g["c_text"])}], 4, 1.0, global_ptr="image")
    assert rel_l2(z1, zr) < LATENT_TOL


def test_checkpoint_ingestion(tmp_path, dev):
    """cfg.pth / load_state_dict path (reference get_model.py:75-79, app.py:267-277): an fp16 checkpoint written with the
    reference key layout loads with strict=True into the VAE and strict=False into VD, and changes the outputs."""
    from lib.cfg_helper import CfgDict
    from lib.model_zoo import get_model
    from oracle import synth
    m = meta()
    vae_cfg = CfgDict(type="autoencoderkl", args=m["vae"])
    ref_net = get_model()(vae_cfg, verbose=False)
    sd = {k: v.half() for k, v in synth.synth_state_dict(synth.shapes_of(ref_net), 99).items()}
    path = str(tmp_path / "kl-tiny.pth")
    torch.save(sd, path)
    net = get_model()(CfgDict(type="autoencoderkl", args=m["vae"], pth=path), verbose=False).half().to(dev)
    z = torch.randn((1, 4, 8, 8), generator=torch.Generator().manual_seed(1)).half().to(dev)
    out1 = net.decode(z)
    ref_net = ref_net.half().to(dev)
    out0 = ref_net.decode(z)           # un-loaded (random init) weights give a different image
    assert rel_l2(out1, out0) > 1e-2
    ref_net.load_state_dict(sd, strict=True)   # in-place reload must invalidate the packed-weight cache
    assert rel_l2(ref_net.decode(z), out1) < 1e-3


def test_full_text_latent_flow_vs_oracle(dev):
    """Full-width openai_unet_0d_v1_dc (1.44 B data + 0.27 B context parameters): one forward of the text-latent flow with
    an image context, CFG batch 2, against the CPU oracle."""
    from lib.cfg_helper import CfgDict, model_cfg_bank
    from lib.model_zoo import get_model
    from oracle import vd_oracle as O
    bank = model_cfg_bank()
    cfg = CfgDict(type="vd_v2_0", args=CfgDict(
        vae_cfg_list=[], ctx_cfg_list=[["image", "ctx-image-placeholder"], ["text", "ctx-text-placeholder"]],
        diffuser_cfg_list=[["image", bank("openai_unet_2d_v1")], ["text", bank("openai_unet_0d_v1_dc")]],
        global_layer_ptr="image", latent_scale_factor={"image": 0.18215}, beta_linear_start=0.00085,
        beta_linear_end=0.012, timesteps=1000, use_ema=False))
    net = get_model()(cfg, verbose=False)
    assert sum(p.numel() for p in net.diffuser["text"].parameters()) == 1706797888
    sd = synth_into(net, 13)
    net = net.half()
    net.to(dev)
    g = torch.Generator().manual_seed(14)
    x = torch.randn((2, 768), generator=g)
    c = torch.randn((2, 257, 768), generator=g) * 0.5
    t = torch.tensor([801, 801])
    with torch.no_grad():
        plan = O.unet0d_plan(**dict(bank("openai_unet_0d_v1_dc").args))
        ref = O.apply_model(sd, plan, x, t, c, x_type="text", c_type="image", global_ptr="image")
    e = net.apply_model({"type": "text", "x": x.half().to(dev)}, t.to(dev), {"type": "image", "c": c.half().to(dev)})
    assert e.shape == (2, 768)
    assert rel_l2(e, ref) < FWD_TOL


# ---- round 2: coverage gaps named by the round-1 review ------------------------------------------------------------

def test_full_schedule_50_step_ddim_parity(full, dev, monkeypatch):
    """The north-star bound over the FULL schedule the bench runs: 50 guided DDIM steps (CFG 7.5) replayed from the HIP
    graph, full-width model, 32x32 latent, B = 1 -- final latent within 1e-2 rel-L2 of the fp32 CPU path, so the error
    growth over 50 replays is measured, not extrapolated from the 5 / 10 step tests."""
    from lib.model_zoo.ddim import DDIMSampler
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(31)
    xT = torch.randn((1, 4, 32, 32), generator=g)
    c = torch.randn((1, 77, 768), generator=g) * 0.5
    u = torch.randn((1, 77, 768), generator=g) * 0.5
    with torch.no_grad():
        zref, _ = O.ddim_sample(sd, O.unet_plan(), sd["alphas_cumprod"], xT,
                                [{"type": "text", "conditioning": c, "unconditional_conditioning": u}], 50, 7.5,
                                global_ptr="image")
    monkeypatch.setattr(torch, "randn", lambda *a, **k: xT.half().to(dev))
    z, _ = DDIMSampler(net).sample(steps=50, shape=[1, 4, 32, 32], x_info={"type": "image"},
                                   c_info={"type": "text", "conditioning": c.half().to(dev),
                                           "unconditional_conditioning": u.half().to(dev),
                                           "unconditional_guidance_scale": 7.5}, eta=0., verbose=False)
    err = rel_l2(z, zref)
    print("50-step DDIM rel-L2 vs fp32 oracle: %.3e" % err)
    assert err < LATENT_TOL


def test_c3_shape_forward_vs_oracle(full, dev):
    """BASELINE configs[2] geometry (image variation, bs = 8): CFG batch 16, 64x64 latent, image context L = 257 with the
    all-zero unconditional half (app.py:345) -- full-width forward against the oracle."""
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(32)
    x = torch.randn((16, 4, 64, 64), generator=g)
    c = torch.randn((16, 257, 768), generator=g) * 0.5
    c[:8] = 0
    t = torch.tensor([981] * 4 + [601] * 4 + [201] * 4 + [1] * 4)
    with torch.no_grad():
        ref = O.apply_model(sd, O.unet_plan(), x, t, c, c_type="image", global_ptr="image")
    e = net.apply_model({"type": "image", "x": x.half().to(dev)}, t.to(dev), {"type": "image", "c": c.half().to(dev)})
    assert e.shape == (16, 4, 64, 64)
    assert rel_l2(e, ref) < FWD_TOL


def test_i2i_partial_schedule_vs_oracle(full, dev):
    """Image variation with fidelity (app.py:355-371, ddim.py:97-103): x0 -> q_sample(ts[k]) -> the first k of 10 DDIM
    steps, guided by an image context, full-width model -- against O.q_sample + O.ddim_sample(forward_steps=k)."""
    from lib.model_zoo.ddim import DDIMSampler
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(33)
    x0 = torch.randn((1, 4, 32, 32), generator=g) * 0.8
    nz = torch.randn((1, 4, 32, 32), generator=g)
    c = torch.randn((1, 257, 768), generator=g) * 0.5
    u = torch.zeros_like(c)
    steps, k = 10, 4
    sched = O.ddim_schedule(sd["alphas_cumprod"], steps, 0.0)
    ts = torch.full((1,), int(sched["timesteps"][k]), dtype=torch.long)
    with torch.no_grad():
        xk = O.q_sample(sd, x0, ts, nz)
        zref, _ = O.ddim_sample(sd, O.unet_plan(), sd["alphas_cumprod"], xk,
                                [{"type": "image", "conditioning": c, "unconditional_conditioning": u}], steps, 7.5,
                                global_ptr="image", forward_steps=k)
    z, _ = DDIMSampler(net).sample(steps=steps, shape=[1, 4, 32, 32],
                                   x_info={"type": "image", "x0": x0.half().to(dev), "x0_forward_timesteps": k,
                                           "x0_noise": nz.half().to(dev)},
                                   c_info={"type": "image", "conditioning": c.half().to(dev),
                                           "unconditional_conditioning": u.half().to(dev),
                                           "unconditional_guidance_scale": 7.5}, eta=0., verbose=False)
    assert rel_l2(z, zref) < LATENT_TOL


def test_stochastic_ddim_with_injected_noise_vs_oracle(tiny, dev, monkeypatch):
    """eta = 0.6: the per-step noise the sampler draws (torch.randn_like on the latent, like the reference's noise_like)
    is injected, and the same tensors drive O.p_sample_ddim(noise=...) -- values, not just finiteness."""
    from lib.model_zoo.ddim import DDIMSampler
    from oracle import synth, vd_oracle as O
    m = meta()
    gold = load_gold("ddim_tiny.npz")
    sd = synth.synth_state_dict(synth.shapes_of(tiny), m["seed"])
    sd.update(O.register_schedule())
    steps, eta, scale = 5, 0.6, 3.0
    g = torch.Generator().manual_seed(34)
    noises = [torch.randn((2, 4, 16, 16), generator=g) for _ in range(steps)]
    xT, c, u = torch.from_numpy(gold["xT"]), torch.from_numpy(gold["c_text"]), torch.from_numpy(gold["u_text"])
    plan = O.unet_plan(**m["unet2d"])
    sched = O.ddim_schedule(sd["alphas_cumprod"], steps, eta)
    x = xT
    with torch.no_grad():
        for i, step in enumerate(np.flip(sched["timesteps"])):
            index = steps - i - 1
            x, _ = O.p_sample_ddim(sd, plan, sched, x, [{"type": "text", "conditioning": c, "unconditional_conditioning": u}],
                                   index, step, scale, global_ptr="image", noise=noises[i].half().float())
    it = iter(noises)
    monkeypatch.setattr(torch, "randn_like", lambda t, **k: next(it).to(device=t.device, dtype=t.dtype))
    z, _ = DDIMSampler(tiny).sample(steps=steps, shape=[2, 4, 16, 16], x_info={"type": "image", "xt": T(gold["xT"], dev)},
                                    c_info={"type": "text", "conditioning": T(gold["c_text"], dev),
                                            "unconditional_conditioning": T(gold["u_text"], dev),
                                            "unconditional_guidance_scale": scale}, eta=eta, verbose=False)
    assert rel_l2(z, x) < LATENT_TOL


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_sampler_rng_consumption_matches_reference(tiny, dev, eta):
    """RNG contract (reference ddim.py:105 and :167): one latent-shaped torch.randn for x_T, then one
    noise_like(x) = torch.randn_like(x) per step EVEN at sigma = 0.  After sample() the device generator must be where
    the reference leaves it, so callers that keep drawing from it stay on the reference's stream."""
    from lib.model_zoo.ddim import DDIMSampler
    gold = load_gold("ddim_tiny.npz")
    steps, shape = 6, [2, 4, 16, 16]
    ct = {"type": "text", "conditioning": T(gold["c_text"], dev), "unconditional_conditioning": T(gold["u_text"], dev),
          "unconditional_guidance_scale": 7.5}
    torch.manual_seed(77)
    sampler = DDIMSampler(tiny)
    sampler.sample(steps=steps, shape=shape, x_info={"type": "image"}, c_info=dict(ct), eta=eta, verbose=False)
    after = torch.randn(8, device=dev)
    n_steps = len(sampler.ddim_timesteps)      # 7 for steps = 6: arange(0, 1000, 1000 // 6) has 7 entries, all are run
    assert n_steps == 7
    torch.manual_seed(77)
    x = torch.randn(shape, device=dev, dtype=torch.float16)     # ddim.py:105: randn(shape, device, dtype of the context)
    for _ in range(n_steps):
        torch.randn_like(x)                                       # ddim.py:167
    expect = torch.randn(8, device=dev)
    assert torch.equal(after, expect)


# ---- round 4: parity debts named by the round-3 review --------------------------------------------------------------

def test_noise_dropout_with_injected_mask_vs_oracle(tiny, dev, monkeypatch):
    """noise_dropout > 0 (reference ddim.py:167-169): F.dropout on the step noise.  The noise draws and the dropout masks
    are injected (torch.randn_like / torch.nn.functional.dropout patched), and the oracle's p_sample_ddim gets the very
    noise * mask / (1 - p) tensors the reference would add -- values, eta = 0.7, guided."""
    from lib.model_zoo.ddim import DDIMSampler
    from oracle import synth, vd_oracle as O
    m = meta()
    gold = load_gold("ddim_tiny.npz")
    sd = synth.synth_state_dict(synth.shapes_of(tiny), m["seed"])
    sd.update(O.register_schedule())
    steps, eta, scale, p = 5, 0.7, 3.0, 0.3
    g = torch.Generator().manual_seed(35)
    noises = [torch.randn((2, 4, 16, 16), generator=g) for _ in range(steps)]
    masks = [(torch.rand((2, 4, 16, 16), generator=g) >= p).float() / (1.0 - p) for _ in range(steps)]
    xT, c, u = torch.from_numpy(gold["xT"]), torch.from_numpy(gold["c_text"]), torch.from_numpy(gold["u_text"])
    plan = O.unet_plan(**m["unet2d"])
    sched = O.ddim_schedule(sd["alphas_cumprod"], steps, eta)
    x = xT
    with torch.no_grad():
        for i, step in enumerate(np.flip(sched["timesteps"])):
            index = steps - i - 1
            x, _ = O.p_sample_ddim(sd, plan, sched, x, [{"type": "text", "conditioning": c, "unconditional_conditioning": u}],
                                   index, step, scale, global_ptr="image", noise=(noises[i] * masks[i]).half().float())
    it, im = iter(noises), iter(masks)
    calls = {"dropout": 0}

    def fake_dropout(t, p=0.5, training=True, inplace=False):
        calls["dropout"] += 1
        assert abs(p - 0.3) < 1e-12 and training
        return (t.float() * next(im).to(t.device)).to(t.dtype)

    monkeypatch.setattr(torch, "randn_like", lambda t, **k: next(it).to(device=t.device, dtype=t.dtype))
    monkeypatch.setattr(torch.nn.functional, "dropout", fake_dropout)
    z, _ = DDIMSampler(tiny).sample(steps=steps, shape=[2, 4, 16, 16], x_info={"type": "image", "xt": T(gold["xT"], dev)},
                                    c_info={"type": "text", "conditioning": T(gold["c_text"], dev),
                                            "unconditional_conditioning": T(gold["u_text"], dev),
                                            "unconditional_guidance_scale": scale}, eta=eta, noise_dropout=p, verbose=False)
    assert calls["dropout"] == steps
    assert rel_l2(z, x) < LATENT_TOL


def test_noise_dropout_rng_order_matches_reference(tiny, dev):
    """Generator consumption with noise_dropout > 0 at eta = 0: per step one randn_like and one dropout mask draw, in
    that order, after the x_T draw (reference ddim.py:105,167-169); the latents equal the plain eta = 0 run (sigma = 0)."""
    from lib.model_zoo.ddim import DDIMSampler
    gold = load_gold("ddim_tiny.npz")
    steps, shape = 4, [2, 4, 16, 16]
    ct = {"type": "text", "conditioning": T(gold["c_text"], dev), "unconditional_conditioning": T(gold["u_text"], dev),
          "unconditional_guidance_scale": 7.5}
    torch.manual_seed(78)
    sampler = DDIMSampler(tiny)
    z, _ = sampler.sample(steps=steps, shape=shape, x_info={"type": "image"}, c_info=dict(ct), eta=0., noise_dropout=0.25,
                          verbose=False)
    after = torch.randn(8, device=dev)
    torch.manual_seed(78)
    x = torch.randn(shape, device=dev, dtype=torch.float16)
    for _ in range(len(sampler.ddim_timesteps)):
        torch.nn.functional.dropout(torch.randn_like(x), p=0.25)
    assert torch.equal(after, torch.randn(8, device=dev))
    torch.manual_seed(78)
    z0, _ = DDIMSampler(tiny).sample(steps=steps, shape=shape, x_info={"type": "image"}, c_info=dict(ct), eta=0., verbose=False)
    assert rel_l2(z, z0) < 2e-3   # eager loop vs graph-replayed loop of the same kernels


def test_sharded_device_generator_reproduces_unsharded_sampler(tiny, dev):
    """vd_sample_sharded(device_generator=True) on one rank starts from the x_T the reference's unsharded call draws
    (torch.manual_seed(seed + 100) -> torch.randn(shape, device, fp16), app.py:309 / ddim.py:105): identical images; the
    default host-generator draw gives a different (world-size invariant) x_T."""
    from lib.model_zoo import sharded
    from lib.model_zoo.ddim import DDIMSampler
    gold = load_gold("ddim_tiny.npz")
    ct = {"type": "text", "conditioning": T(gold["c_text"], dev), "unconditional_conditioning": T(gold["u_text"], dev)}
    seed, steps, shape = 5, 4, [2, 4, 16, 16]
    img = sharded.vd_sample_sharded(tiny, DDIMSampler(tiny), steps, shape, [dict(ct)], seed, device_generator=True)
    torch.manual_seed(seed + 100)
    z, _ = DDIMSampler(tiny).sample(steps=steps, shape=shape, x_info={"type": "image"},
                                    c_info=dict(ct, unconditional_guidance_scale=7.5), eta=0., verbose=False)
    ref = tiny.vae_decode(z, which="image")
    # same x_T, same kernels; not bit-equal from run to run (GroupNorm partial sums meet through LDS float atomics)
    assert rel_l2(img, ref) < 2e-3
    img_host = sharded.vd_sample_sharded(tiny, DDIMSampler(tiny), steps, shape, [dict(ct)], seed)
    assert rel_l2(img_host, ref) > 5e-2   # another x_T altogether


def test_c2_shape_guided_10_step_loop_batch2_vs_oracle(full, dev, monkeypatch):
    """BASELINE configs[1] geometry at a batch > 1: B = 2 (CFG batch 4), 64x64x4 latent, L = 77, 10 guided DDIM steps with
    the graph-replayed loop, full-width model, vs the fp32 CPU oracle -- the captured step at a full-width 64x64 geometry
    with more than one sample (per-sample GroupNorm statistics, per-image patches, batch-strided attention)."""
    from lib.model_zoo.ddim import DDIMSampler
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(41)
    xT = torch.randn((2, 4, 64, 64), generator=g)
    c = torch.randn((2, 77, 768), generator=g) * 0.5
    u = (torch.randn((1, 77, 768), generator=g) * 0.5).repeat(2, 1, 1)
    with torch.no_grad():
        zref, _ = O.ddim_sample(sd, O.unet_plan(), sd["alphas_cumprod"], xT,
                                [{"type": "text", "conditioning": c, "unconditional_conditioning": u}], 10, 7.5,
                                global_ptr="image")
    monkeypatch.setattr(torch, "randn", lambda *a, **k: xT.half().to(dev))
    z, _ = DDIMSampler(net).sample(steps=10, shape=[2, 4, 64, 64], x_info={"type": "image"},
                                   c_info={"type": "text", "conditioning": c.half().to(dev),
                                           "unconditional_conditioning": u.half().to(dev),
                                           "unconditional_guidance_scale": 7.5}, eta=0., verbose=False)
    err = rel_l2(z, zref)
    per_sample = [rel_l2(z[i], zref[i]) for i in range(2)]
    print("C2-shape 10-step B=2 rel-L2 vs fp32 oracle: %.3e (per sample %s)" % (err, per_sample))
    assert err < LATENT_TOL and max(per_sample) < LATENT_TOL


def test_dual_context_guided_10_step_graph_loop_batch2_vs_oracle(full, dev, monkeypatch):
    """BASELINE configs[3] (dual-guided: text L = 77 + image L = 257, attention mixing 0.5 / 0.5) through a 10-step guided,
    graph-replayed MULTICONTEXT loop at B = 2 (CFG batch 4) on the full-width model vs the fp32 CPU oracle (32x32 latent so
    the oracle finishes in about a minute): the captured step with two context block sets chained through the proj_out
    epilogues (alpha / residual), the hoisted time-embedding table and producer row statistics, per sample."""
    from lib.model_zoo.ddim import DDIMSampler
    from oracle import vd_oracle as O
    net, sd = full
    g = torch.Generator().manual_seed(77)
    xT = torch.randn((2, 4, 32, 32), generator=g)
    ct = torch.randn((2, 77, 768), generator=g) * 0.5
    ut = (torch.randn((1, 77, 768), generator=g) * 0.5).repeat(2, 1, 1)
    ci = torch.randn((2, 257, 768), generator=g) * 0.5
    ui = torch.zeros_like(ci)
    with torch.no_grad():
        zref, _ = O.ddim_sample(sd, O.unet_plan(), sd["alphas_cumprod"], xT,
                                [{"type": "text", "conditioning": ct, "unconditional_conditioning": ut, "ratio": 0.5},
                                 {"type": "image", "conditioning": ci, "unconditional_conditioning": ui, "ratio": 0.5}],
                                10, 7.5, global_ptr="image")
    h = lambda t: t.half().to(dev)
    cl = lambda: [{"type": "text", "conditioning": h(ct), "unconditional_conditioning": h(ut), "unconditional_guidance_scale": 7.5, "ratio": 0.5},
                  {"type": "image", "conditioning": h(ci), "unconditional_conditioning": h(ui), "unconditional_guidance_scale": 7.5, "ratio": 0.5}]
    sampler = DDIMSampler(net)
    assert sampler.use_graph
    z, _ = sampler.sample_multicontext(steps=10, shape=[2, 4, 32, 32], x_info={"type": "image", "xt": h(xT).clone()},
                                       c_info_list=cl(), eta=0., verbose=False)
    err = rel_l2(z, zref)
    per_sample = [rel_l2(z[i], zref[i]) for i in range(2)]
    print("dual-context 10-step B=2 graph loop rel-L2 vs fp32 oracle: %.3e (per sample %s)" % (err, per_sample))
    assert err < LATENT_TOL and max(per_sample) < LATENT_TOL
    # a second call re-uses the kept step graph (new latent, same geometry) and stays on the oracle's trajectory
    z2, _ = sampler.sample_multicontext(steps=10, shape=[2, 4, 32, 32], x_info={"type": "image", "xt": h(xT).clone()},
                                        c_info_list=cl(), eta=0., verbose=False)
    # step 0 of the first call ran eagerly, here it is replayed: the same kernels (the 4x4 level measures its GroupNorms through
    # LDS float atomics, so the last bit is order-dependent)
    assert rel_l2(z2, z) < 2e-3


def test_hoisted_time_embedding_matches_in_step_embedding(tiny, dev, monkeypatch):
    """DDIMSampler computes the t-only part of the UNet (time-embedding MLP + every ResBlock's emb_layers projection, reference
    vd.py:339-349 / openaimodel.py:2627-2633, :263) for all steps once per sample() and hands the step graph one row of that
    table (VD_v2_0.precompute_step_emb); with emb_hoist off every step recomputes it like the reference.  Same latents either
    way, single- and multi-context, and apply_model with the extension key equals apply_model without it."""
    from lib.model_zoo.ddim import DDIMSampler
    gd = load_gold("ddim_tiny.npz")
    xT = torch.from_numpy(gd["xT"]).half().to(dev)
    ct, ut = torch.from_numpy(gd["c_text"]).half().to(dev), torch.from_numpy(gd["u_text"]).half().to(dev)
    ci = {"type": "text", "conditioning": ct, "unconditional_conditioning": ut, "unconditional_guidance_scale": 7.5}
    outs = []
    for hoist in (True, False):
        s = DDIMSampler(tiny)
        s.emb_hoist = hoist
        z, _ = s.sample(steps=6, shape=list(xT.shape), x_info={"type": "image", "xt": xT.clone()}, c_info=dict(ci), eta=0., verbose=False)
        outs.append(z)
    assert rel_l2(outs[0], outs[1]) < 2e-3
    # one forward: the extension key against the in-forward embedding
    t = torch.full((xT.shape[0],), 601, device=dev, dtype=torch.long)
    pre = tiny.precompute_step_emb("image", t[:1])
    assert pre is not None
    row = pre[0][0]
    rows = {di: row[o:o + c] for di, (o, c) in pre[1].items()}
    e0 = tiny.apply_model({"type": "image", "x": xT}, t, {"type": "text", "c": ct})
    e1 = tiny.apply_model({"type": "image", "x": xT, "emb_rows": rows}, t, {"type": "text", "c": ct})
    assert rel_l2(e1, e0) < 2e-3
    assert tiny.precompute_step_emb("text", t[:1]) is None   # the 0-D text-latent flow keeps its in-forward embedding
