"""FreeU on the GPU: the kernel (vd_freeu_f16 through ops.freeu) bit for bit on exact inputs and per element on random ones, its
independence of batch and run, the forward with x_info['freeu'] against the oracle walk of tests/freeu_cases.py, the four samplers'
loops against the oracle loop, graph replay against eager steps, the graph key, and the combinations with DeepCache, windows,
inpainting and the guidance rescale."""
import numpy as np
import pytest
import torch

import deepcache_cases as dc
import freeu_cases as fc
import window_cases as wc
from freeu_cases import FWD_TOL, LATENT_TOL, SETTING
from vdtest_util import assert_exact, load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

SHAPE = [2, 4, 16, 16]


@pytest.fixture(scope="module")
def tiny(dev):
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    sd = synth_into(net, m["seed"])
    net = net.half()
    net.to(dev)
    return net, sd


@pytest.fixture(scope="module")
def plan():
    from oracle import vd_oracle as O
    return O.unet_plan(**meta()["unet2d"])


@pytest.fixture(scope="module")
def gold():
    return load_gold("ddim_tiny.npz")


def nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def nchw(t):
    return t.permute(0, 3, 1, 2).cpu()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", fc.EXACT_PLANES)
def test_exact_inputs_give_the_float64_reference_rounded_once(dev, H, W):
    """Integers in [-8, 8] on planes whose every table entry is 0 or +-1: the seven sums, the bracket and g times it are exact in
    fp32, so the output is the float64 definition rounded once to fp16, bit for bit."""
    from vd_hip import ops
    assert all(set(np.unique(t)) <= {-1.0, 0.0, 1.0} for t in ops.freeu_tables_host(H, W))
    B, C = 3, 64
    h = fc.exact_ints((B, C, H, W), 7 * H + W)
    x = fc.exact_ints((B, C, H, W), 70 * H + W)
    for s in fc.EXACT_S:
        ref = fc.fourier_filter(x.double(), 1, s)
        near = ref.half().double()
        assert (ref - near).abs().max().item() <= 1e-9                 # every reference value is an fp16 value
        assert (ref != x.double()).double().mean().item() > 0.5        # ... and the filter moves most of them
        for b in fc.EXACT_B:
            h2, x2 = ops.freeu(nhwc(h, dev), nhwc(x, dev), b, s)
            assert h2.dtype == x2.dtype == torch.float16 and tuple(h2.shape) == tuple(x2.shape) == (B, H, W, C)
            # (value for value: where the definition gives a zero, torch.fft leaves it either sign)
            assert_exact(nchw(x2), near, ("sample", "channel", "y", "x"), "%d x %d, s %g, b %g" % (H, W, s, b))
            want = h.clone()
            want[:, :C // 2] = (h[:, :C // 2].float() * np.float32(b)).half()
            assert torch.equal(bits(nchw(h2)), bits(want)), (H, W, s, b)


@pytest.mark.parametrize("H,W,C0,C1,B", fc.BOUNDED)
def test_random_inputs_stay_inside_the_per_element_bound(dev, H, W, C0, C1, B):
    from vd_hip import ops
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + C1 + B)
    h = torch.randn((B, C0, H, W), generator=g).half()
    x = (torch.randn((B, C1, H, W), generator=g) * 1.5 + 0.25).half()
    for b, s in ((SETTING[0], SETTING[2]), (SETTING[1], SETTING[3])):
        h2, x2 = ops.freeu(nhwc(h, dev), nhwc(x, dev), b, s)
        ref = fc.fourier_filter(x.double(), 1, float(np.float32(s)))
        bound = fc.skip_bound(x, ref, float(np.float32(s)))
        err = (nchw(x2).double() - ref).abs().numpy()
        worst = float((err / bound).max())
        print("%dx%d C0 %d C1 %d B %d s %.1f: max |out - ref| / bound %.3f, max abs err %.3e" % (H, W, C0, C1, B, s, worst, err.max()))
        assert (err <= bound).all()
        got = nchw(h2)
        assert torch.equal(bits(got[:, C0 // 2:]), bits(h[:, C0 // 2:]))                                   # the copied half
        assert torch.equal(bits(got[:, :C0 // 2]), bits((h[:, :C0 // 2].float() * np.float32(b)).half()))  # the scaled half


def test_a_sample_has_the_same_bits_in_any_batch_slice_and_run(dev):
    from vd_hip import ops
    g = torch.Generator().manual_seed(5)
    for H, W, C0, C1 in [(8, 8, 128, 128), (32, 32, 64, 320), (6, 10, 64, 32)]:
        h = nhwc(torch.randn((4, C0, H, W), generator=g).half(), dev)
        x = nhwc(torch.randn((4, C1, H, W), generator=g).half(), dev)
        h3, x3 = ops.freeu(h[:3], x[:3], 1.2, 0.2)
        again = ops.freeu(h[:3], x[:3], 1.2, 0.2)
        assert torch.equal(again[0], h3) and torch.equal(again[1], x3)
        for i in range(3):
            hi, xi = ops.freeu(h[i:i + 1].clone(), x[i:i + 1].clone(), 1.2, 0.2)
            assert torch.equal(hi[0], h3[i]) and torch.equal(xi[0], x3[i]), (H, W, i)
        hv, xv = ops.freeu(h[2:4], x[2:4], 1.2, 0.2)              # the second half of a batch of four, as the fork walks it
        assert h[2:4].data_ptr() != h.data_ptr() and torch.equal(hv[0], h3[2]) and torch.equal(xv[0], x3[2])
        # inputs untouched, ones are the identity on h and (s = 1: g = 0) on the skip
        h1, x1 = ops.freeu(h, x, 1.0, 1.0)
        assert torch.equal(h1, h) and torch.equal(x1, x) and h1.data_ptr() != h.data_ptr() and x1.data_ptr() != x.data_ptr()


def test_op_refuses_bad_arguments(dev):
    from vd_hip import ops
    t = lambda *s: torch.zeros(s, dtype=torch.float16, device=dev)
    for h, x in [(t(1, 4, 4, 12), t(1, 4, 4, 8)), (t(1, 4, 4, 8), t(1, 4, 4, 4)), (t(1, 1, 4, 8), t(1, 1, 4, 8)), (t(1, 4, 1, 8), t(1, 4, 1, 8)),
                 (t(1, 4, 4, 8), t(2, 4, 4, 8)), (t(1, 4, 4, 8), t(1, 4, 2, 8)), (t(4, 4, 8), t(4, 4, 8))]:
        with pytest.raises(ValueError, match="freeu"):
            ops.freeu(h, x, 1.2, 0.9)
    for b, s in [(True, 0.9), (1.2, None), (float("nan"), 0.9), (1.2, float("inf")), ("1.2", 0.9)]:
        with pytest.raises(ValueError, match="freeu"):
            ops.freeu(t(1, 4, 4, 8), t(1, 4, 4, 8), b, s)
    cy = ops.freeu_tables(4, 6, dev)
    assert [tuple(v.shape) for v in cy] == [(4,), (4,), (6,), (6,), (24,), (24,)] and ops.freeu_tables(4, 6, dev) is cy
    assert all(torch.equal(v.cpu(), torch.from_numpy(w)) for v, w in zip(cy, ops.freeu_tables_host(4, 6)))


# ---- 2. the forward --------------------------------------------------------------------------------------------------------

def _inputs(seed, B, dual, guided, H=16, W=16):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, H, W), generator=g).half().float()
    rows = (2 if guided else 1) * B
    ctx = [("text", (torch.randn((rows, 77, 128), generator=g) * 0.5).half().float(), 0.4 if dual else 1.0)]
    if dual:
        ctx.append(("image", (torch.randn((rows, 50, 128), generator=g) * 0.5).half().float(), 0.6))
    return x, ctx


def _fwd(net, dev, x, t, ctx, guided, **keys):
    rows = (2 if guided else 1) * x.shape[0]
    x_info = dict({"type": "image", "x": x.half().to(dev), "repeat": 2 if guided else 1}, **keys)
    ts = torch.full((rows,), t, dtype=torch.long, device=dev)
    if len(ctx) == 1:
        return net.apply_model(x_info, ts, {"type": ctx[0][0], "c": ctx[0][1].half().to(dev)})
    return net.apply_model_multicontext(x_info, ts, [{"type": ct, "c": c.half().to(dev), "ratio": r} for ct, c, r in ctx])


def _oracle(sd, plan, x, t, ctx, guided, setting, **kw):
    xin = torch.cat([x, x]) if guided else x
    return fc.walk(sd, plan, xin, torch.full((xin.shape[0],), t, dtype=torch.long), ctx, setting, **kw)


@pytest.mark.parametrize("dual", [False, True])
def test_guided_forward_vs_the_oracle_walk(tiny, plan, dev, dual):
    net, sd = tiny
    x, ctx = _inputs(31 + dual, 2, dual, True)
    ref = _oracle(sd, plan, x, 500, ctx, True, SETTING)
    off = _oracle(sd, plan, x, 500, ctx, True, None)
    assert rel_l2(ref, off) >= 10 * FWD_TOL          # precondition, on the oracle alone: the bound tells FreeU on from off
    e = _fwd(net, dev, x, 500, ctx, True, freeu=SETTING)
    plain = _fwd(net, dev, x, 500, ctx, True)
    err, gap = rel_l2(e, ref), rel_l2(ref, off)
    print("dual %d: forward with FreeU vs the oracle walk %.3e; oracle on vs off %.3e; plain forward vs oracle off %.3e"
          % (dual, err, gap, rel_l2(plain, off)))
    assert e.dtype == torch.float16 and tuple(e.shape) == (4, 4, 16, 16)
    assert err < FWD_TOL
    assert rel_l2(plain, off) < FWD_TOL and rel_l2(e, off) > 5 * FWD_TOL
    as_dict = _fwd(net, dev, x, 500, ctx, True, freeu=dict(zip(("b1", "b2", "s1", "s2"), SETTING)))
    assert torch.equal(as_dict, e)
    # absent = None = all ones = today's forward
    for off_key in ({"freeu": None}, {"freeu": (1, 1, 1, 1)}, {"freeu": {"b1": 1.0, "b2": 1.0, "s1": 1.0, "s2": 1.0}}):
        assert torch.equal(_fwd(net, dev, x, 500, ctx, True, **off_key), plain)


@pytest.mark.parametrize("setting", [(1.2, 1.0, 0.9, 1.0), (1.0, 1.4, 1.0, 0.2), (1.0, 1.0, 0.5, 1.0)])
def test_a_stage_of_ones_launches_nothing(tiny, plan, dev, monkeypatch, setting):
    """One active stage: three launches (stage 1: output blocks 0 .. 2) or one (stage 2: block 3), and the oracle's values."""
    from vd_hip import ops
    net, sd = tiny
    x, ctx = _inputs(41, 2, False, False)
    calls, real = [], ops.freeu

    def counted(h, skip, b, s):
        calls.append((h.shape[-1], b, s))
        return real(h, skip, b, s)

    monkeypatch.setattr(ops, "freeu", counted)
    e = _fwd(net, dev, x, 500, ctx, False, freeu=setting)
    b1, b2, s1, s2 = setting
    assert calls == ([(128, b1, s1)] * 3 if (b1, s1) != (1.0, 1.0) else []) + ([(64, b2, s2)] if (b2, s2) != (1.0, 1.0) else [])
    assert rel_l2(e, _oracle(sd, plan, x, 500, ctx, False, setting)) < FWD_TOL
    calls.clear()
    _fwd(net, dev, x, 500, ctx, False, freeu=(1, 1, 1, 1))
    _fwd(net, dev, x, 500, ctx, False)
    assert calls == []


def test_forward_inside_the_half_batch_fork(tiny, plan, dev, monkeypatch):
    """VD_BATCH_FORK=1 semantics: the 8 x 8 level (output blocks 0 and 1, stage 1) runs as two half-batch branches on slices."""
    from lib.model_zoo import vd
    net, sd = tiny
    x, ctx = _inputs(51, 4, False, False)
    monkeypatch.setattr(vd, "BATCH_FORK", "1")
    e = _fwd(net, dev, x, 500, ctx, False, freeu=SETTING)
    assert torch.equal(_fwd(net, dev, x, 500, ctx, False, freeu=SETTING), e)
    assert rel_l2(e, _oracle(sd, plan, x, 500, ctx, False, SETTING)) < FWD_TOL
    monkeypatch.setattr(vd, "BATCH_FORK", "0")
    assert rel_l2(_fwd(net, dev, x, 500, ctx, False, freeu=SETTING), e) < 1e-3


# ---- 3. loops --------------------------------------------------------------------------------------------------------------

def _ci(c, u, scale, ctype="text", **kw):
    return dict({"type": ctype, "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale}, **kw)


def _on_dev(c, dev):
    return dict(c, conditioning=c["conditioning"].half().to(dev), unconditional_conditioning=c["unconditional_conditioning"].half().to(dev))


def _make(kind, net, **kw):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    from lib.model_zoo.unipc import UniPCSampler
    return {"ddim": DDIMSampler, "2m": DPMSolverSampler, "unipc": UniPCSampler, "sde": DPMSolverSDESampler}[kind](net, **kw)


def _gold_case(gold):
    xT = torch.from_numpy(gold["xT"]).float()
    return xT, [_ci(torch.from_numpy(gold["c_text"]), torch.from_numpy(gold["u_text"]), 7.5)]


def _sample(sampler, dev, xT, cs, steps=5, c_keys=None, call=None, **keys):
    x_info = dict({"type": "image", "xt": xT.half().to(dev)}, **keys)
    c = dict(_on_dev(cs[0], dev), **(c_keys or {}))
    return sampler.sample(steps=steps, shape=list(xT.shape), x_info=x_info, c_info=c, verbose=False, **(call or {}))


@pytest.mark.parametrize("kind", ["ddim", "2m", "unipc", "sde0", "sde1"])
def test_five_step_loops_vs_the_oracle_loop(tiny, plan, dev, gold, kind):
    from test_philox_cpu import normals_ref_batch
    net, sd = tiny
    xT, cs = _gold_case(gold)
    seeds = [41, 2 ** 33 + 9]
    base = kind[:3] if kind.startswith("sde") else kind
    sampler = _make(base, net)
    keys, call, noise = {}, {}, None
    if kind == "sde0":
        call = {"eta": 0.0}
    elif kind == "sde1":
        keys = {"seeds": seeds}
        per = int(np.prod(SHAPE[1:]))
        noise = lambda draw: torch.from_numpy(normals_ref_batch(seeds, per, draw, 2))
    z, _ = _sample(sampler, dev, xT, cs, call=call, freeu=SETTING, **keys)
    assert len(sampler.ddim_timesteps) == 5
    ref = fc.oracle_loop(sd, plan, sampler, base, xT, cs, 7.5, SETTING, noise=noise)
    off = fc.oracle_loop(sd, plan, sampler, base, xT, cs, 7.5, None, noise=noise)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("%s: final latent vs the oracle loop with FreeU %.3e; oracle loop on vs off %.3e" % (kind, err, gap))
    assert err < LATENT_TOL
    # (oracle alone: on and off end 1.3e-2 .. 1.5e-2 apart on these weights) the bound tells the loop with FreeU from the loop
    # without, and the product's latent is nearer to the former
    assert gap > LATENT_TOL and err < rel_l2(z, off)


@pytest.mark.parametrize("kind", ["ddim", "2m", "unipc", "sde"])
def test_graph_replay_eager_steps_and_a_fresh_sampler_agree_bitwise(tiny, dev, gold, monkeypatch, kind):
    net, _ = tiny
    xT, cs = _gold_case(gold)
    keys = {"seeds": [5, 6]} if kind == "sde" else {}
    shared = _make(kind, net)
    z_off0, _ = _sample(shared, dev, xT, cs, **keys)                          # before any call with the key
    z_on, _ = _sample(shared, dev, xT, cs, freeu=SETTING, **keys)
    z_off, _ = _sample(shared, dev, xT, cs, **keys)                           # an off-call behind an on-call: its own bits
    assert torch.equal(z_off, z_off0) and not torch.equal(z_on, z_off)
    assert len(shared._static) == 2 and all(st["graph"] is not None for st in shared._static.values())
    assert torch.equal(_sample(shared, dev, xT, cs, freeu=SETTING, **keys)[0], z_on)                 # on the kept graph
    assert torch.equal(_sample(shared, dev, xT, cs, freeu=(1, 1, 1, 1), **keys)[0], z_off)
    assert len(shared._static) == 2
    assert torch.equal(_sample(_make(kind, net), dev, xT, cs, freeu=SETTING, **keys)[0], z_on)       # a fresh sampler
    other, _ = _sample(shared, dev, xT, cs, freeu=(1.2, 1.4, 0.9, 0.5), **keys)                      # another setting: another graph
    assert not torch.equal(other, z_on)
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = _make(kind, net)
    assert not eager.use_graph
    assert torch.equal(_sample(eager, dev, xT, cs, freeu=SETTING, **keys)[0], z_on)
    assert torch.equal(_sample(eager, dev, xT, cs, **keys)[0], z_off)


def test_eager_ddim_loop_and_single_steps_honour_the_key(tiny, dev, gold):
    from lib.model_zoo.ddim import DDIMSampler
    net, _ = tiny
    xT, cs = _gold_case(gold)
    outs = []
    for keys in ({"freeu": SETTING}, {"freeu": SETTING}, {}):
        torch.manual_seed(3)
        outs.append(_sample(DDIMSampler(net), dev, xT, cs, call={"eta": 0.5}, **keys)[0])
    assert torch.equal(outs[0], outs[1]) and rel_l2(outs[0], outs[2]) > 1e-3
    s = DDIMSampler(net)
    s.make_schedule(5, verbose=False)
    c = _on_dev(cs[0], dev)
    t = torch.full((2,), int(s.ddim_timesteps[4]), dtype=torch.long, device=dev)
    x = xT.half().to(dev)
    torch.manual_seed(1)
    on = s.p_sample_ddim({"type": "image", "x": x, "freeu": SETTING}, c, t, 4)[0]
    torch.manual_seed(1)
    off = s.p_sample_ddim({"type": "image", "x": x}, c, t, 4)[0]
    torch.manual_seed(1)
    ones = s.p_sample_ddim({"type": "image", "x": x, "freeu": (1, 1, 1, 1)}, c, t, 4)[0]
    assert torch.equal(ones, off) and rel_l2(on, off) > 1e-4


def test_multicontext_loop_vs_the_oracle_loop(tiny, plan, dev, gold):
    net, sd = tiny
    xT, cs = _gold_case(gold)
    cs = [dict(cs[0], ratio=0.4), _ci(torch.from_numpy(gold["c_img"]), torch.from_numpy(gold["u_img"]), 7.5, "image", ratio=0.6)]
    sampler = _make("2m", net)
    z, _ = sampler.sample_multicontext(steps=5, shape=SHAPE, x_info={"type": "image", "xt": xT.half().to(dev), "freeu": SETTING},
                                       c_info_list=[_on_dev(c, dev) for c in cs], verbose=False)
    ref = fc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, SETTING)
    print("dual 2m: final latent vs the oracle loop with FreeU %.3e" % rel_l2(z, ref))
    assert rel_l2(z, ref) < LATENT_TOL


# ---- 4. combinations -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,depth", [("ddim", 1), ("unipc", 3)])
def test_with_deepcache_vs_the_cached_oracle_loop(tiny, plan, dev, gold, kind, depth):
    """Depth 1 cuts in front of the last load (stage 2, 16 x 16), depth 3 in front of output block 1 (stage 1, 8 x 8): the kept
    feature is the tensor in front of that load, and every walk that consumes it applies the stage to a copy."""
    net, sd = tiny
    xT, cs = _gold_case(gold)
    sampler = _make(kind, net)
    z, inter = _sample(sampler, dev, xT, cs, freeu=SETTING, cache_interval=2, cache_depth=depth)
    assert inter["cache_full_steps"] == [0, 2, 4]
    st = [s for s in sampler._static.values() if "deep" in s][0]
    kept = st["deep"].buf.clone()
    ref = fc.oracle_loop(sd, plan, sampler, kind, xT, cs, 7.5, SETTING, interval=2, depth=depth)
    off = fc.oracle_loop(sd, plan, sampler, kind, xT, cs, 7.5, None, interval=2, depth=depth)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("%s depth %d: cached loop with FreeU vs the cached oracle loop %.3e; oracle on vs off %.3e" % (kind, depth, err, gap))
    assert err < LATENT_TOL and gap > LATENT_TOL and err < rel_l2(z, off)
    z2, _ = _sample(sampler, dev, xT, cs, freeu=SETTING, cache_interval=2, cache_depth=depth)
    assert torch.equal(z2, z) and torch.equal(st["deep"].buf, kept)          # on the kept graphs; the last store is the same


def test_with_windows_vs_per_window_oracle_forwards_merged(tiny, plan, dev):
    net, sd = tiny
    g = torch.Generator().manual_seed(61)
    shape = (1, 4, 16, 32)
    xT = torch.randn(shape, generator=g).half().float()
    cs = [_ci((torch.randn((1, 77, 128), generator=g) * 0.5).half().float(), (torch.randn((1, 77, 128), generator=g) * 0.5).half().float(), 7.5)]
    sampler = _make("2m", net)
    z, _ = _sample(sampler, dev, xT, cs, freeu=SETTING, window=16)
    geo = wc.geometry(16, 32, 16, 8)
    assert len(geo["offs"]) == 3
    ref = fc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, SETTING, geo=geo)
    off = wc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, geo)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("windowed 2m: loop with FreeU vs the windowed oracle loop %.3e; windowed oracle on vs off %.3e" % (err, gap))
    assert err < LATENT_TOL and gap > LATENT_TOL and err < rel_l2(z, off)


def test_with_inpainting_the_known_region_comes_back_bitwise(tiny, dev, gold):
    net, _ = tiny
    xT, cs = _gold_case(gold)
    x0 = (torch.randn(SHAPE, generator=torch.Generator().manual_seed(4)) * 0.5).half().to(dev)
    mask = torch.ones((2, 1, 16, 16))
    mask[..., :6, :] = 0
    mask = mask.half().to(dev)
    run = lambda **kw: _make("unipc", net).sample(steps=5, shape=SHAPE, x_info=dict({"type": "image", "x0": x0, "xt": xT.half().to(dev),
                                                                                       "inpaint_mask": mask}, **kw),
                                                  c_info=_on_dev(cs[0], dev), verbose=False)[0]
    z, z_off = run(freeu=SETTING), run()
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(z[keep], x0[keep]) and bool(torch.isfinite(z).all())
    assert rel_l2(z[~keep], z_off[~keep]) > LATENT_TOL


def test_with_guidance_rescale_vs_the_oracle_loop(tiny, plan, dev, gold):
    net, sd = tiny
    xT, cs = _gold_case(gold)
    sampler = _make("ddim", net)
    z, inter = _sample(sampler, dev, xT, cs, c_keys={"guidance_rescale": 0.7}, freeu=SETTING)
    assert len(inter["guidance_rescale"]) >= 1
    ref = fc.oracle_loop(sd, plan, sampler, "ddim", xT, cs, 7.5, SETTING, phi=0.7)
    off = fc.oracle_loop(sd, plan, sampler, "ddim", xT, cs, 7.5, None, phi=0.7)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("rescaled ddim: loop with FreeU vs the oracle loop %.3e; oracle on vs off %.3e" % (err, gap))
    assert err < LATENT_TOL and gap > LATENT_TOL and err < rel_l2(z, off)


def test_sharded_world1_matches_direct_sample(tiny, dev, gold):
    from lib.model_zoo import sharded
    net, _ = tiny
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dev).half()
    ct = _ci(T(gold["c_text"]), T(gold["u_text"]), 7.5)
    imgs = sharded.vd_sample_sharded(net, _make("2m", net), 5, SHAPE, [dict(ct)], 3, guidance_scale=7.5, device_generator=True,
                                     freeu=SETTING)
    torch.manual_seed(103)
    z, _ = _make("2m", net).sample(steps=5, shape=SHAPE, x_info={"type": "image", "freeu": SETTING}, c_info=dict(ct), verbose=False)
    assert torch.equal(imgs, net.vae_decode(z, which="image"))
