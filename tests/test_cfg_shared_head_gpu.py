"""The first context block under classifier-free guidance: its entry and self-attention run once per sample, and the launches
that first meet per-replica data read the shared activation through a batch period (sample b of the output reads sample b % P).

Kernel level: the period changes addresses only, so the periodic entry on the un-replicated operand and the plain entry on
ops.repeat_batch(operand) -- same grid, same tiles, same summation order -- must agree BIT FOR BIT (xattn, ff_chain, and the
tail of a transformer block whose self-attention output is pinned).  Model level: with the switch on, the block's head runs at
half the rows, where the GEMM planner may pick another tile or split, so on / off / the explicit [x; x] batch agree to 1e-3
relative L2 (the bound of the half-batch fork, which differs from its reference for the same reason); each setting is
bit-identical run to run, and a guided sampler gives the same latents eager and captured.  The model of those tests is the
fixture configuration at width 320 with heads of 40, the one width that has both periodic consumers; every test counts the
periodic launches, so it cannot pass without the sharing having run.  Other widths (the tiny fixture model) do not share:
run_unet replicates in front of the block, and asking a block of such a width for repeat > 1 is an error."""
import copy

import numpy as np
import pytest
import torch

from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

PLAN_TOL = 1e-3


@pytest.fixture(scope="module")
def ops():
    from vd_hip import ops as o
    return o


def rnd(shape, dev, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half().to(dev)


def per_sample(t):
    """t [P, ...] with a distinct offset per sample: a wrong sample mapping cannot cancel."""
    off = torch.arange(t.shape[0], device=t.device, dtype=torch.float32).view(-1, *([1] * (t.dim() - 1)))
    return (t.float() + 0.75 * (off + 1.0)).half()


# ---- xattn ---------------------------------------------------------------------------------------------------------------

def _xattn_operands(ops, dev, C, D, Nq, P, repeat, Nk=77):
    from lib.model_zoo.hip_layers import fold_layernorm
    H, B = C // D, P * repeat
    assert ops.xattn_supported(H, D)
    x = per_sample(rnd((P, Nq, C), dev, 1.1, 700))
    wq = rnd((C, C), dev, C ** -0.5, 701)
    kv = rnd((B, Nk, 2 * C), dev, 1.0, 702)
    ln = torch.nn.LayerNorm(C, eps=1e-5).to(dev)
    g = torch.Generator().manual_seed(703)
    with torch.no_grad():
        ln.weight.copy_((1.0 + 0.2 * torch.randn(C, generator=g)).to(dev))
        ln.bias.copy_((0.1 * torch.randn(C, generator=g)).to(dev))
    w, b, cs = fold_layernorm(wq, None, ln)
    return H, B, x, w, b, cs, kv


# (B * nqb) % 8: 2, 0 (4 samples x 2 query blocks, the second one ragged), 3, 2 -- both block maps of the kernel run
@pytest.mark.parametrize("C,D,Nq,P,repeat", [(320, 40, 128, 1, 2), (320, 40, 192, 2, 2), (320, 40, 128, 1, 3), (640, 80, 128, 1, 2),
                                            (1280, 160, 128, 1, 2)])
def test_xattn_period_is_bitwise_the_replicated_operand(ops, dev, C, D, Nq, P, repeat):
    H, B, x, w, b, cs, kv = _xattn_operands(ops, dev, C, D, Nq, P, repeat)
    k, v = kv[..., :C], kv[..., C:]
    ref = ops.xattn(ops.repeat_batch(x, repeat), w, b, cs, 1e-5, k, v, H)
    out = ops.xattn(x, w, b, cs, 1e-5, k, v, H, repeat=repeat)
    assert out.shape == ref.shape == (B, Nq, C) and bool(torch.isfinite(out).all())
    assert torch.equal(out, ref)
    # the replicas really differ (other K / V per replica): a kernel that ignored the replica index would not pass
    assert not torch.equal(out[:P], out[P:2 * P])


@pytest.mark.parametrize("Nq,B", [(128, 3), (192, 4)])
def test_xattn_period_equal_to_the_batch_is_the_plain_entry(ops, dev, Nq, B):
    """vd_xattn_rep_f16 with x_samples == B is vd_xattn_f16."""
    from vd_hip.loader import lib
    C, D = 320, 40
    H, _, x, w, b, cs, kv = _xattn_operands(ops, dev, C, D, Nq, B, 1)
    k, v = kv[..., :C], kv[..., C:]
    ref = ops.xattn(x, w, b, cs, 1e-5, k, v, H)
    out = torch.empty_like(ref)
    rc = lib().vd_xattn_rep_f16(x.data_ptr(), w.data_ptr(), b.data_ptr(), cs.data_ptr(), 1e-5, k.data_ptr(), v.data_ptr(), out.data_ptr(),
                                B, B, H, Nq, 77, D, k.stride(1), v.stride(1), k.stride(0), v.stride(0), D ** -0.5,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(out, ref)


def test_xattn_period_must_divide_the_batch(ops, dev):
    """B = 3 samples of K / V over x_samples = 2: refused by the launcher, nothing runs."""
    from vd_hip.loader import lib
    C, D = 320, 40
    H, _, x, w, b, cs, kv = _xattn_operands(ops, dev, C, D, 128, 2, 1)
    kv3 = torch.cat([kv, kv[:1]])
    k, v = kv3[..., :C], kv3[..., C:]
    out = torch.empty((3, 128, C), dtype=torch.float16, device=dev)
    args = lambda B, P: (x.data_ptr(), w.data_ptr(), b.data_ptr(), cs.data_ptr(), 1e-5, k.data_ptr(), v.data_ptr(), out.data_ptr(), B, P, H,
                         128, 77, D, k.stride(1), v.stride(1), k.stride(0), v.stride(0), D ** -0.5, torch.cuda.current_stream().cuda_stream)
    assert lib().vd_xattn_rep_f16(*args(3, 2)) != 0
    assert lib().vd_xattn_rep_f16(*args(2, 3)) != 0 and lib().vd_xattn_rep_f16(*args(2, 0)) != 0


# ---- ff_chain ------------------------------------------------------------------------------------------------------------

def _ff_operands(dev, HW, P, repeat):
    from lib.model_zoo.hip_layers import fold_layernorm
    from vd_hip.pack import pack_geglu
    C, M = 320, P * repeat * HW
    x0 = per_sample(rnd((P, HW, C), dev, 1.2, 900))
    r = per_sample(rnd((P, HW, C), dev, 1.0, 910)) * -1.0
    a = rnd((M // HW, HW, C), dev, 1.0, 901)
    wo, bo = rnd((C, C), dev, 0.05, 902), rnd((C,), dev, 0.2, 903)
    w1, b1 = rnd((8 * C, C), dev, 0.05, 904), rnd((8 * C,), dev, 0.2, 905)
    w2, b2 = rnd((C, 4 * C), dev, 0.03, 906), rnd((C,), dev, 0.2, 907)
    wp, bp = rnd((C, C), dev, 0.05, 908), rnd((C,), dev, 0.2, 909)
    ln = torch.nn.LayerNorm(C, eps=1e-5).to(dev)
    g = torch.Generator().manual_seed(911)
    with torch.no_grad():
        ln.weight.copy_((1.0 + 0.2 * torch.randn(C, generator=g)).to(dev))
        ln.bias.copy_((0.1 * torch.randn(C, generator=g)).to(dev))
    wf, bf, _ = fold_layernorm(w1, b1, ln)
    w1p, b1p = pack_geglu(wf, bf)
    return dict(x0=x0, r=r, a=a, wo=wo, bo=bo, w1p=w1p, b1p=b1p, w2=w2, b2=b2, wp=wp, bp=bp)


@pytest.mark.parametrize("pre,post", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("HW,P,repeat", [(128, 1, 2), (128, 2, 2), (256, 1, 2), (256, 2, 2), (128, 1, 3)])
def test_ff_chain_period_is_bitwise_the_replicated_operands(ops, dev, HW, P, repeat, pre, post):
    """Both residuals (x0 behind attn2.to_out, r behind proj_out) differ per sample and from each other."""
    o = _ff_operands(dev, HW, P, repeat)
    rep = lambda t: ops.repeat_batch(t, repeat)
    # without the first projection x is the feed-forward's own input: per replica, never shared
    x_full = rep(o["x0"]) if pre else per_sample(rnd((P * repeat, HW, 320), dev, 1.2, 920))
    kw_ref, kw_new = {}, {}
    if pre:
        kw_ref.update(a=o["a"], wo=o["wo"], bo=o["bo"])
        kw_new.update(kw_ref)
    if post:
        kw_ref.update(wp=o["wp"], bp=o["bp"], alpha=0.4, res=rep(o["r"]), want_stats=True, stat_img_rows=HW)
        kw_new.update(kw_ref, res=o["r"])
    kw_new.update(repeat=repeat, stat_img_rows=HW)
    ref = ops.ff_chain(x_full, o["w1p"], o["b1p"], o["w2"], o["b2"], 1e-5, **kw_ref)
    out = ops.ff_chain(o["x0"] if pre else x_full, o["w1p"], o["b1p"], o["w2"], o["b2"], 1e-5, **kw_new)
    assert out.shape == ref.shape == (P * repeat, HW, 320) and bool(torch.isfinite(out).all())
    assert torch.equal(out, ref)
    if post:
        s_new, s_ref = ops.stats_of(out), ops.stats_of(ref)
        assert s_new is not None and s_ref is not None and torch.equal(s_new.buf, s_ref.buf)
    if P > 1:   # the samples of the shared operands are not interchangeable
        swapped = dict(kw_new)
        x_sw = o["x0"].flip(0) if pre else x_full
        if post:
            swapped["res"] = o["r"].flip(0)
        assert not torch.equal(ops.ff_chain(x_sw, o["w1p"], o["b1p"], o["w2"], o["b2"], 1e-5, **swapped), ref)


def test_ff_chain_refuses_a_tile_that_straddles_two_samples(ops, dev):
    """HW = 192: the second 128-row tile holds rows of two samples -- the launcher refuses the period, at P = 1 and at P = 2."""
    from vd_hip.loader import VdHipError
    for P in (1, 2):
        o = _ff_operands(dev, 192, P, 2)
        assert not ops.ff_chain_period_ok(192)
        with pytest.raises(VdHipError, match="period_rows"):
            ops.ff_chain(o["x0"], o["w1p"], o["b1p"], o["w2"], o["b2"], 1e-5, a=o["a"], wo=o["wo"], bo=o["bo"], wp=o["wp"], bp=o["bp"],
                         alpha=0.4, res=o["r"], repeat=2, stat_img_rows=192)


# ---- the transformer block -------------------------------------------------------------------------------------------------

def _st320(dev, seed=5):
    """One width-320 SpatialTransformer (8 heads of 40, context width 768) with seeded weights; proj_out is not left at zero."""
    from lib.model_zoo.attention import SpatialTransformer
    st = SpatialTransformer(320, 8, 40, context_dim=768)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in st.named_parameters():
            if p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * (p[0].numel() ** -0.5))
            elif n.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return st.half().to(dev)


@pytest.mark.parametrize("HW,with_post", [(256, True), (256, False), (192, False), (192, True)])
def test_block_tail_is_bitwise_given_the_same_self_attention_output(ops, dev, HW, with_post, monkeypatch):
    """BasicTransformerBlock with attn1 pinned to one tensor: behind it the shared run (repeat=2: periodic xattn and ff_chain, or at
    HW = 192 the fallback that replicates behind attn1) and the run on the replicated input launch the same kernels with the same
    plan on the same values -- the cases in which both settings must agree bit for bit."""
    st = _st320(dev)
    blk = st.transformer_blocks[0]
    P, rep_n, C = 2, 2, 320
    h = per_sample(rnd((P, HW, C), dev, 1.0, 40))
    h1 = per_sample(rnd((P, HW, C), dev, 1.0, 41))        # what attn1 "returns" for the P samples
    pres = per_sample(rnd((P, HW, C), dev, 1.0, 42))
    ctx = rnd((P * rep_n, 77, 768), dev, 0.5, 43)
    monkeypatch.setattr(blk.attn1, "forward", lambda x, **kw: h1 if x.shape[0] == P else ops.repeat_batch(h1, rep_n))
    post = lambda r: (tuple(st.proj_out._w()) + (0.7, r, HW)) if with_post else None
    shared = blk(h, context=ctx, repeat=rep_n, post=post(pres))
    ref = blk(ops.repeat_batch(h, rep_n), context=ctx, post=post(ops.repeat_batch(pres, rep_n)))
    if with_post:
        assert isinstance(shared, tuple) and isinstance(ref, tuple)
        shared, ref = shared[0], ref[0]
    assert shared.shape == ref.shape and shared.shape[0] == P * rep_n
    assert torch.equal(shared, ref)


@pytest.mark.parametrize("P,HW", [(2, (16, 16)), (2, (16, 12)), (4, (64, 64))])
def test_spatial_transformer_320_shared_head_vs_replicated_input(ops, dev, P, HW):
    """A width-320 SpatialTransformer at 16x16 (B = 2 -> 4: the three-launch entry and the chained tail at the smallest HW
    vd_ff_chain_f16 takes with a period), at 16x12 (HW = 192: the launcher would refuse, the host replicates behind attn1) and at
    64x64 with B = 4 -> 8 (the benchmark's combination: the one-launch entry vd_gemm_row320_chain_f16 on the P samples, then the
    chained tail with proj_out folded in, both residuals periodic).  The head runs on half the rows, where the planner may
    choose differently: 1e-3 relative L2; each form is bit-identical run to run."""
    st = _st320(dev)
    H, W = HW
    assert st.shares_cfg_head()
    assert ops.st_chain_supported(P, H * W, 320, 320) == (H * W == 4096)   # which entry the shared run takes
    x = per_sample(rnd((P, H, W, 320), dev, 1.0, 50))
    if H * W == 4096:
        # the one-launch entry takes GroupNorm's statistics from the tensor's producer, as every input of this block in run_unet
        # carries them (ops.repeat_batch replicates them along).  Without them it measures x with gn_partial_kernel, whose LDS float
        # atomics make the sums -- and with them the last bit of the output -- differ from run to run, shared or not.
        x._vd_stats = ops.chan_stats(x, 256)   # what a producer attaches
    ctx = rnd((2 * P, 77, 768), dev, 0.5, 51)
    ref = st(ops.repeat_batch(x, 2), ctx)
    out = st(x, ctx, repeat=2)
    assert out.shape == ref.shape == (2 * P, H, W, 320) and bool(torch.isfinite(out).all())
    e = rel_l2(out, ref)
    print("SpatialTransformer 320 %dx%d shared vs replicated: rel-L2 %.3e, bitwise %s" % (H, W, e, torch.equal(out, ref)))
    assert e < PLAN_TOL
    assert torch.equal(out, st(x, ctx, repeat=2)) and torch.equal(ref, st(ops.repeat_batch(x, 2), ctx))
    assert rel_l2(out[:P], out[P:]) > 1e-3   # the replicas did meet their own contexts
    s_out, s_ref = ops.stats_of(out), ops.stats_of(ref)
    assert (s_out is None) == (s_ref is None)
    if s_out is not None:
        assert s_out.buf.shape == s_ref.buf.shape and s_out.T == s_ref.T and s_out.HW == s_ref.HW


# ---- a small width-320 model ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide(dev):
    """The tiny fixture configuration with ONE level of width 320 and heads of 40 in both diffusers (24 M + 43 M parameters):
    every context block has the periodic consumers, so guided forwards share the head of the first one."""
    from lib.model_zoo import get_model
    m = copy.deepcopy(meta())
    m["unet2d"].update(model_channels=320, num_head_channels=40, channel_mult=[1], num_res_blocks=[1], attention_resolutions=[1])
    m["unet0d"].update(model_channels=320, num_head_channels=40, channel_mult=[1], num_noattn_blocks=[1], second_dim=[4], with_attn=[True])
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    synth_into(net, 11)
    net = net.half()
    net.to(dev)
    assert all(blk[0].shares_cfg_head() for d in net.diffuser.values() for blk in d.context_blocks)
    return net


@pytest.fixture(scope="module")
def tiny(dev):
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    synth_into(net, m["seed"])
    net = net.half()
    net.to(dev)
    return net


def T(a, dev, dtype=torch.float16):
    return torch.from_numpy(np.asarray(a)).to(dev).to(dtype)


def _count_periodic(ops, monkeypatch):
    """[launches of vd_xattn_rep_f16 with a period, launches of vd_ff_chain_f16 with a period] from here on."""
    n = [0, 0]
    real_x, real_f = ops.xattn, ops.ff_chain

    def xattn(*a, **k):
        n[0] += k.get("repeat", 1) > 1
        return real_x(*a, **k)

    def ff_chain(*a, **k):
        n[1] += k.get("repeat", 1) > 1
        return real_f(*a, **k)
    monkeypatch.setattr(ops, "xattn", xattn)
    monkeypatch.setattr(ops, "ff_chain", ff_chain)
    return n


@pytest.mark.parametrize("B,side", [(2, 16), (4, 64)])
def test_wide_unet_shared_head_on_off_and_explicit_batch(wide, ops, dev, B, side, monkeypatch):
    """run_unet(repeat=2) on the width-320 model with VD_CFG_HEAD_SHARE on and off, and the repeat=1 forward on the materialised
    [x; x] batch (the reference's definition): 16x16 with B = 2 (three-launch entry) and 64x64 with B = 4 (the benchmark's
    geometry: one-launch entry, proj_out folded into the chained tail).  On shares -- one periodic xattn and one periodic ff_chain
    launch per forward, none with the switch off."""
    from lib.model_zoo import vd
    g = torch.Generator().manual_seed(7 + side)
    x = torch.randn((B, 4, side, side), generator=g).half().to(dev)
    c = (torch.randn((B, 77, 128), generator=g) * 0.5).half().to(dev)
    c2 = torch.cat([c * 0.0, c])
    t2 = torch.full((2 * B,), 501, device=dev, dtype=torch.long)
    fwd = lambda: wide.apply_model({"type": "image", "x": x, "repeat": 2}, t2, {"type": "text", "c": c2}).float()
    n = _count_periodic(ops, monkeypatch)
    assert vd.CFG_HEAD_SHARE   # the default
    on = fwd()
    assert n == [1, 1], n
    on2 = fwd()
    monkeypatch.setattr(vd, "CFG_HEAD_SHARE", False)
    off = fwd()
    off2 = fwd()
    explicit = wide.apply_model({"type": "image", "x": torch.cat([x, x])}, t2, {"type": "text", "c": c2}).float()
    assert n == [2, 2], n   # nothing periodic with the switch off or on the explicit batch
    print("wide UNet B=%d %dx%d: on vs off %.3e, on vs explicit %.3e, off vs explicit %.3e; run to run on %s off %s" % (
        B, side, side, rel_l2(on, off), rel_l2(on, explicit), rel_l2(off, explicit), torch.equal(on, on2), torch.equal(off, off2)))
    assert on.shape == explicit.shape == (2 * B, 4, side, side) and bool(torch.isfinite(on).all())
    assert rel_l2(on[:B], on[B:]) > 1e-3   # the replicas met their own contexts
    assert rel_l2(on, off) < PLAN_TOL and rel_l2(on, explicit) < PLAN_TOL and rel_l2(off, explicit) < PLAN_TOL
    assert torch.equal(on, on2) and torch.equal(off, off2)


def test_other_widths_do_not_share(tiny, ops, dev, monkeypatch):
    """The tiny fixture model (widths 64 / 128) has no periodic consumers: run_unet replicates in front of the block whatever the
    switch says, and a block of such a width refuses repeat > 1 instead of taking a path nothing else runs."""
    g = load_gold("unet_tiny.npz")
    x, c = T(g["x"], dev), T(g["c_text"], dev)
    c2 = torch.cat([c * 0.0, c])
    t2 = torch.full((2 * x.shape[0],), 501, device=dev, dtype=torch.long)
    n = _count_periodic(ops, monkeypatch)
    out = tiny.apply_model({"type": "image", "x": x, "repeat": 2}, t2, {"type": "text", "c": c2}).float()
    explicit = tiny.apply_model({"type": "image", "x": torch.cat([x, x])}, t2, {"type": "text", "c": c2}).float()
    assert n == [0, 0] and rel_l2(out, explicit) < PLAN_TOL
    st = tiny.diffuser["image"].context_blocks[0][0]
    assert not st.shares_cfg_head()
    xs = rnd((2, 16, 16, st.in_channels), dev, 1.0, 3)
    with pytest.raises(ops.VdHipError, match="batch period"):
        st(xs, rnd((4, 77, 128), dev, 0.5, 4), repeat=2)


@pytest.mark.parametrize("name", ["ddim", "dpmpp"])
def test_guided_sampling_eager_vs_captured(wide, ops, dev, name, monkeypatch):
    """Four guided steps on the width-320 model with the shared head (the default; counted): the captured step graph gives the eager
    latents.  (Four, not three: a three-step uniform grid over 1000 training steps ends at index 1000 and raises IndexError, as
    the reference's make_ddim_sampling_parameters does; four is the shortest guided loop above three that the schedule accepts.)"""
    from lib.model_zoo import vd
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    assert vd.CFG_HEAD_SHARE
    cls = DDIMSampler if name == "ddim" else DPMSolverSampler
    g = torch.Generator().manual_seed(5)
    xT = torch.randn((2, 4, 16, 16), generator=g).half().to(dev)
    c = (torch.randn((2, 77, 128), generator=g) * 0.5).half().to(dev)
    u = (torch.randn((2, 77, 128), generator=g) * 0.5).half().to(dev)

    def run(sampler):
        kw = {"eta": 0.0} if name == "ddim" else {}
        z, _ = sampler.sample(steps=4, shape=[2, 4, 16, 16], x_info={"type": "image", "xt": xT.clone()}, verbose=False,
                              c_info={"type": "text", "conditioning": c, "unconditional_conditioning": u,
                                      "unconditional_guidance_scale": 7.5}, **kw)
        return z.float()

    n = _count_periodic(ops, monkeypatch)
    captured = cls(wide)
    assert captured.use_graph
    z_graph = run(captured)
    assert n[0] >= 1 and n[0] == n[1], n   # the forwards that were launched from Python (warm-up, capture) shared the head
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = cls(wide)
    assert not eager.use_graph
    n[0] = n[1] = 0
    z_eager = run(eager)
    assert n == [4, 4], n   # one shared head per eager step
    print("%s eager vs captured: rel-L2 %.3e" % (name, rel_l2(z_graph, z_eager)))
    assert bool(torch.isfinite(z_graph).all())
    assert torch.equal(z_graph, z_eager)
