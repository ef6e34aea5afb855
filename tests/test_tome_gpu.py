"""Token merging on the GPU: the four entries (vd_tome_match_f16, vd_tome_plan, vd_tome_merge_f16, vd_tome_unmerge_f16 through
vd_hip.ops) against the float64 / int64 restatement of tests/tome_cases.py, one SpatialTransformer at the full widths, the tiny
model's forward and the four samplers' loops against the oracle walk replaying the device's plans, and the bit identities of the
sampler keys (off = today's bits; graph replay = eager steps = a fresh sampler)."""
import numpy as np
import pytest
import torch

import tome_cases as tc
from tome_cases import FWD_TOL, LATENT_TOL
from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

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


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _match(dev, h, H, W):
    from vd_hip import ops
    idx, mx = ops.tome_match(h.to(dev), H, W)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), mx.cpu().numpy()


# ---- 1. match --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,C,B", tc.GRIDS)
def test_match_random_inputs_stay_inside_the_fp32_bound(dev, H, W, C, B):
    h = tc.random_metric(H, W, C, B, 100 + H)
    s = tc.scores64(h, H, W)
    best = s.max(-1)
    tol = tc.match_tol(C)
    idx, mx = _match(dev, h, H, W)
    assert idx.dtype == np.int32 and idx.shape == best.shape and idx.min() >= 0 and idx.max() < s.shape[-1]
    got = np.take_along_axis(s, idx[..., None].astype(np.int64), -1)[..., 0]
    print("grid %dx%d C %d B %d: worst chosen-score deficit %.3e, worst |node_max - max| %.3e, tol %.3e, rows off the float64 argmax %d"
          % (H, W, C, B, (best - got).max(), np.abs(mx - best).max(), tol, int((idx != s.argmax(-1)).sum())))
    assert (got >= best - tol).all()
    assert (np.abs(mx.astype(np.float64) - best) <= tol).all()
    # the same rows as a column slice of a wider tensor (ldh > C) and as a batch-slice view
    wide = torch.zeros((B + 1, H * W, C + 8), dtype=torch.float16)
    wide[1:, :, :C] = h
    idx2, mx2 = _match(dev, wide.to(dev)[1:, :, :C], H, W)
    assert np.array_equal(idx2, idx) and np.array_equal(mx2.view(np.int32), mx.view(np.int32))


@pytest.mark.parametrize("H,W,C,B", tc.GRIDS)
def test_match_planted_inputs_give_the_float64_argmax_everywhere(dev, H, W, C, B):
    h, chosen = tc.planted_metric(H, W, C, B, 200 + W)
    idx, mx = _match(dev, h, H, W)
    assert np.array_equal(idx, chosen)
    assert (np.abs(mx - tc.match_ref(h, H, W)[1]) <= tc.match_tol(C)).all()


@pytest.mark.parametrize("H,W,C,B", [tc.GRIDS[1], tc.GRIDS[4]])
def test_match_exact_ties_zero_rows_and_two_runs(dev, H, W, C, B):
    src, dst = tc.sets(H, W)
    Nd = len(dst)
    h = tc.random_metric(H, W, C, B, 300)
    pairs = [(1, 2), (0, Nd - 1), (3, Nd // 2 + 1)]          # duplicates inside one tile of 32 destinations and across tiles
    for lo, hi in pairs:
        h[:, dst[hi]] = h[:, dst[lo]]
    for k, (lo, hi) in enumerate(pairs):                      # sources that ARE the duplicated row (scaled: the cosine is 1 for both)
        h[:, src[5 + k]] = h[:, dst[lo]] * 0.5
        h[:, src[40 + k]] = h[:, dst[hi]] * 2.0
    h[:, src[20]] = 0                                         # an all-zero source
    h[0, dst[5]] = 0                                          # and an all-zero destination
    idx, mx = _match(dev, h, H, W)
    assert np.isfinite(mx).all()
    for k, (lo, hi) in enumerate(pairs):
        assert (idx[:, 5 + k] == lo).all() and (idx[:, 40 + k] == lo).all()
        assert (idx != hi).all()                              # the higher duplicate never wins: its twin has the same fp32 score
    assert (idx[:, 20] == 0).all() and (mx[:, 20] == 0).all()
    s = tc.scores64(h, H, W)
    assert (np.take_along_axis(s, idx[..., None].astype(np.int64), -1)[..., 0] >= s.max(-1) - tc.match_tol(C)).all()
    idx2, mx2 = _match(dev, h, H, W)
    assert np.array_equal(idx, idx2) and np.array_equal(mx.view(np.int32), mx2.view(np.int32))


# ---- 2. plan ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,B", [(g[0], g[1], g[3]) for g in tc.GRIDS] + [(64, 64, 1)])      # 64 x 64: more than one staged tile
def test_plan_is_the_restatement_int_for_int(dev, H, W, B):
    from vd_hip import ops
    rng = np.random.default_rng(H * 100 + W)
    Nd = H * W // 4
    Ns = H * W - Nd
    mx = rng.standard_normal((B, Ns)).astype(np.float32)
    mx[:, rng.integers(0, Ns, Ns // 3)] = np.float32(0.25)                  # many duplicates
    mx[:, rng.integers(0, Ns, max(Ns // 8, 1))] = np.float32(-0.5)          # negative duplicates
    mx[:, 0], mx[:, Ns - 1] = mx.max() + 1, mx.max() + 1                    # a tie for the first rank, at both ends
    idx = rng.integers(0, Nd, (B, Ns)).astype(np.int32)
    for r in (0, 1, Ns // 2, Ns):
        row_of = ops.tome_plan(torch.from_numpy(idx).to(dev), torch.from_numpy(mx).to(dev), H, W, r)
        assert row_of.dtype == torch.int32 and np.array_equal(row_of.cpu().numpy(), tc.plan_ref(idx, mx, H, W, r)), (H, W, r)


# ---- 3. merge / unmerge ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,C,B", tc.GRIDS)
def test_merge_and_unmerge_equal_the_restatement_per_element(dev, H, W, C, B):
    from vd_hip import ops
    rng = np.random.default_rng(H + 7 * W)
    Nd = H * W // 4
    Ns = H * W - Nd
    g = torch.Generator().manual_seed(H * W)
    qkv = (torch.randn((B + 1, H * W, 3 * C), generator=g) * 3).half()
    qkv[:, :, ::7] *= 2.0 ** -12                             # subnormal results among the means
    mx = rng.standard_normal((B, Ns)).astype(np.float32)
    idx = rng.integers(0, Nd, (B, Ns)).astype(np.int32)
    one = np.full((B, Ns), Nd - 1, dtype=np.int32)           # one destination receives every merged source
    qd = qkv.to(dev)
    for r, ix in [(0, idx), (1, idx), (Ns // 2, idx), (Ns, idx), (Ns, one), (Ns // 2, one)]:
        row_of = tc.plan_ref(ix, mx, H, W, r)
        rd = torch.from_numpy(row_of).to(dev)
        x = qd[1:]                                            # a batch-slice view of the fused [B + 1, N, 3 C]
        m = ops.tome_merge(x, rd, H, W, r)
        assert tuple(m.shape) == (B, H * W - r, 3 * C)
        assert torch.equal(m.cpu(), torch.from_numpy(tc.merge_ref(qkv[1:], row_of, r))), (r,)
        mk = ops.tome_merge(x[..., C:2 * C], rd, H, W, r)    # a column slice: ld = 3 C
        assert torch.equal(mk, m[..., C:2 * C])
        u = ops.tome_unmerge(m[..., 2 * C:], rd, H, W, r)    # the gather through ld = 3 C too
        assert torch.equal(u.cpu(), torch.from_numpy(tc.unmerge_ref(m[..., 2 * C:].cpu(), row_of)))
    row_of = tc.plan_ref(idx, mx, H, W, 0)
    back = ops.tome_unmerge(ops.tome_merge(qd[1:], torch.from_numpy(row_of).to(dev), H, W, 0), torch.from_numpy(row_of).to(dev), H, W, 0)
    assert torch.equal(back, qd[1:])                          # r = 0: merge then unmerge is the identity


def test_merge_rounds_the_crafted_mean_once(dev):
    from vd_hip import ops
    vals, direct = tc.double_rounding_rows()
    src, dst = tc.sets(4, 4)
    x = np.zeros((1, 16, 8), dtype=np.float16)
    x[0, dst[0]], x[0, src[0]], x[0, src[1]] = vals[0], vals[1], vals[2]
    x[0, dst[0], 1], x[0, src[0], 1], x[0, src[1], 1] = -vals[0], -vals[1], -vals[2]
    idx = np.zeros((1, 12), dtype=np.int32)
    mx = np.linspace(1.0, 0.0, 12, dtype=np.float32)[None]
    row_of = tc.plan_ref(idx, mx, 4, 4, 2)
    ref = tc.merge_ref(x, row_of, 2)
    assert ref[0, 10, 0] == direct and ref[0, 10, 1] == -direct
    m = ops.tome_merge(torch.from_numpy(x).to(dev), torch.from_numpy(row_of).to(dev), 4, 4, 2)
    assert torch.equal(m.cpu(), torch.from_numpy(ref))
    assert float(m[0, 10, 0]) == 1.0 + 2.0 ** -10             # not 1.0, what double -> float -> half gives


def test_entries_refuse_bad_arguments(dev):
    from vd_hip import ops
    h = torch.zeros((1, 16, 64), dtype=torch.float16, device=dev)
    with pytest.raises(ops.VdHipError, match="vd_tome_match_f16.*even"):
        ops.tome_match(torch.zeros((1, 15, 64), dtype=torch.float16, device=dev), 3, 5)
    with pytest.raises(ops.VdHipError, match="vd_tome_match_f16.*unsupported"):
        ops.tome_match(torch.zeros((1, 16, 48), dtype=torch.float16, device=dev), 4, 4)
    with pytest.raises(ops.VdHipError, match="vd_tome_match_f16"):
        ops.tome_match(torch.zeros((1, 16, 72), dtype=torch.float16, device=dev)[..., 4:68], 4, 4)      # misaligned rows
    with pytest.raises(ops.VdHipError, match="tome_match"):
        ops.tome_match(h, 4, 5)
    idx = torch.zeros((1, 12), dtype=torch.int32, device=dev)
    mx = torch.zeros((1, 12), dtype=torch.float32, device=dev)
    for r in (-1, 13):
        with pytest.raises(ops.VdHipError, match="vd_tome_plan.*outside"):
            ops.tome_plan(idx, mx, 4, 4, r)
    row_of = ops.tome_plan(idx, mx, 4, 4, 4)
    with pytest.raises(ops.VdHipError, match="vd_tome_merge_f16.*multiple of 8"):
        ops.tome_merge(torch.zeros((1, 16, 12), dtype=torch.float16, device=dev), row_of, 4, 4, 4)
    with pytest.raises(ops.VdHipError, match="tome_unmerge"):
        ops.tome_unmerge(torch.zeros((1, 11, 8), dtype=torch.float16, device=dev), row_of, 4, 4, 4)


# ---- 4. one block at the full widths -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,side,repeat", [(320, 16, 2), (640, 8, 1)])
def test_one_block_at_the_full_widths_vs_the_oracle_block(dev, C, side, repeat):
    """One SpatialTransformer at each full width that merges -- 320: q | k | v and the metric h arrive from the chained entry kernel
    and the block runs its self-attention once per guidance pair (repeat = 2, the shared CFG head); 640: the block's own fused
    projection -- with seeded weights (proj_out not left at zero) at ratio 0.5, against the oracle block of tests/tome_cases.py on the
    device's plan.  Compared on what the block adds to its input (out - x), sample by sample, with the project's forward bound."""
    from lib.model_zoo.attention import SpatialTransformer
    heads = 8
    st = SpatialTransformer(C, heads, C // heads, context_dim=768)
    g = torch.Generator().manual_seed(C)
    with torch.no_grad():
        for n, p in st.named_parameters():
            if p.dim() >= 2:
                v = torch.randn(p.shape, generator=g) * (p[0].numel() ** -0.5)
            elif n.endswith("weight"):
                v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
            else:
                v = 0.1 * torch.randn(p.shape, generator=g)
            p.copy_(v.half().float())
    sd = {"b." + k: v.detach().clone().float() for k, v in st.state_dict().items()}
    B = 2
    x = torch.randn((B, C, side, side), generator=g).half().float()
    ctx = (torch.randn((repeat * B, 77, 768), generator=g) * 0.5).half().float()
    r = tc.r_of(side, side, 0.5)
    st = st.half().to(dev)
    if repeat > 1:
        assert st.shares_cfg_head()
    xd = x.permute(0, 2, 3, 1).contiguous().half().to(dev)
    rec = []
    kw = {"repeat": repeat} if repeat > 1 else {}
    out = st(xd, ctx.half().to(dev), tome=(r, lambda row_of: rec.append(row_of.clone())), **kw)
    assert len(rec) == 1 and tuple(rec[0].shape) == (B, side * side) and tuple(out.shape) == (repeat * B, side, side, C)
    ro = np.concatenate([rec[0].cpu().numpy()] * repeat)
    xr = torch.cat([x] * repeat)
    with torch.no_grad():
        ref = tc.spatial_transformer(sd, "b", xr, ctx, heads, r, ro)[0] - xr
        from oracle import vd_oracle as O
        off = O.spatial_transformer(sd, "b", xr, ctx, heads) - xr
    delta = (out.float() - torch.cat([xd] * repeat).float()).permute(0, 3, 1, 2).cpu()
    errs = [rel_l2(delta[b], ref[b]) for b in range(repeat * B)]
    plain = (st(xd, ctx.half().to(dev), **kw).float() - torch.cat([xd] * repeat).float()).permute(0, 3, 1, 2).cpu()
    print("width %d: block delta vs the oracle block on the device's plan per sample %s; plain block vs the oracle without merging %.3e; "
          "merged vs unmerged on the device %.3e" % (C, ["%.3e" % e for e in errs], rel_l2(plain, off), rel_l2(delta, plain)))
    assert all(e < FWD_TOL for e in errs)
    assert rel_l2(plain, off) < FWD_TOL and rel_l2(delta, plain) > FWD_TOL
    assert torch.equal(st(xd, ctx.half().to(dev), tome=(r, None), **kw), out)         # the same call twice: the same bits


# ---- 5. the tiny model's forward ---------------------------------------------------------------------------------------------------

def _inputs(seed, B, dual, guided):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, 16, 16), generator=g).half().float()
    rows = lambda L: (torch.randn(((2 if guided else 1) * B, L, 128), generator=g) * 0.5).half().float()
    ctx = [("text", rows(77), 0.4 if dual else 1.0)]
    if dual:
        ctx.append(("image", rows(50), 0.6))
    return x, ctx


def _fwd(net, dev, x, t, ctx, reps, **keys):
    x_info = dict({"type": "image", "x": x.half().to(dev), "repeat": reps}, **keys)
    ts = torch.full((reps * x.shape[0],), t, dtype=torch.long, device=dev)
    if len(ctx) == 1:
        return net.apply_model(x_info, ts, {"type": ctx[0][0], "c": ctx[0][1].half().to(dev)})
    return net.apply_model_multicontext(x_info, ts, [{"type": ct, "c": c.half().to(dev), "ratio": r} for ct, c, r in ctx])


@pytest.mark.parametrize("dual,guided,md", [(False, True, 2), (True, True, 1), (False, False, 2)])
def test_forward_vs_the_oracle_walk_on_the_devices_plans(tiny, plan, dev, dual, guided, md):
    from lib.model_zoo.vd import TokenMerge
    net, sd = tiny
    B, reps = 2, 2 if guided else 1
    x, ctx = _inputs(31 + dual + 2 * guided, B, dual, guided)
    tm = TokenMerge(0.5, md)
    tm.record = []
    e = _fwd(net, dev, x, 500, ctx, reps, tome=tm)
    n_blocks = {1: 3, 2: 7}[md] * len(ctx)
    assert len(tm.record) == n_blocks and all(ro.dtype == torch.int32 for _, ro in tm.record)
    xin = torch.cat([x] * reps)
    t = torch.full((xin.shape[0],), 500, dtype=torch.long)
    tokens = []
    it = iter(tm.record)
    ref = tc.walk(sd, plan, xin, t, ctx, 0.5, md, it, tokens=tokens)
    assert next(it, None) is None and tokens[0] == (256, 128)
    plain = _fwd(net, dev, x, 500, ctx, reps)
    err, moved = rel_l2(e, ref), rel_l2(e, plain)
    print("dual %d guided %d max_downsample %d: forward vs the oracle walk on the device's plans %.3e; merged vs unmerged forward %.3e"
          % (dual, guided, md, err, moved))
    assert err < FWD_TOL and moved > FWD_TOL
    # off: absent, None and ratio 0 are today's forward, bit for bit
    assert torch.equal(_fwd(net, dev, x, 500, ctx, reps, tome=None), plain)
    assert torch.equal(_fwd(net, dev, x, 500, ctx, reps, tome=TokenMerge(0.0, md)), plain)
    tm.record = None
    assert torch.equal(_fwd(net, dev, x, 500, ctx, reps, tome=tm), e)


# ---- 6. loops ----------------------------------------------------------------------------------------------------------------------

def _ci(c, u, scale, ctype="text", **kw):
    return dict({"type": ctype, "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale}, **kw)


def _on_dev(c, dev):
    return dict(c, conditioning=c["conditioning"].half().to(dev), unconditional_conditioning=c["unconditional_conditioning"].half().to(dev))


def _make(kind, net, **kw):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    from lib.model_zoo.unipc import UniPCSampler
    return {"ddim": DDIMSampler, "2m": DPMSolverSampler, "unipc": UniPCSampler, "sde": DPMSolverSDESampler}[kind](net, **kw)


def _gold_case(gold, scale=7.5):
    xT = torch.from_numpy(gold["xT"]).float()
    return xT, [_ci(torch.from_numpy(gold["c_text"]), torch.from_numpy(gold["u_text"]), scale)]


def _sample(sampler, dev, xT, cs, steps=6, c_keys=None, call=None, **keys):
    """steps = 6: the uniform schedule's spacing 1000 // 6 = 166 gives the SEVEN timesteps 1, 167, ..., 997."""
    x_info = dict({"type": "image", "xt": xT.half().to(dev)}, **keys)
    c = dict(_on_dev(cs[0], dev), **(c_keys or {}))
    return sampler.sample(steps=steps, shape=list(xT.shape), x_info=x_info, c_info=c, verbose=False, **(call or {}))


@pytest.mark.parametrize("kind,scale,md", [("ddim", 7.5, 1), ("2m", 7.5, 2), ("unipc", 7.5, 1), ("sde", 7.5, 1), ("2m", 1.0, 1)])
def test_seven_step_loops_vs_the_oracle_loop_on_the_devices_plans(tiny, plan, dev, gold, kind, scale, md):
    from lib.model_zoo.vd import TokenMerge
    net, sd = tiny
    xT, cs = _gold_case(gold, scale)
    sampler = _make(kind, net)
    sampler.use_graph = False                                 # eager steps: the record hook does not live in a graph
    tm = TokenMerge(0.5, md)
    tm.record = []
    call = {"eta": 0.0} if kind == "sde" else {}
    z, inter = _sample(sampler, dev, xT, cs, call=call, tome=tm)
    blocks = {1: 3, 2: 7}[md]
    assert len(sampler.ddim_timesteps) == 7 and len(tm.record) == 7 * blocks
    assert inter["tome_tokens"] == ([(256, 128)] * 3 if md == 1 else [(256, 128), (64, 32), (64, 32), (64, 32), (64, 32), (256, 128), (256, 128)])
    ref = tc.oracle_loop(sd, plan, sampler, kind, xT, cs, scale, 0.5, md, plans=tm.record)
    z_off, i_off = _sample(sampler, dev, xT, cs, call=call)
    err, moved = rel_l2(z, ref), rel_l2(z, z_off)
    print("%s s %.1f max_downsample %d: final latent vs the oracle loop on the device's plans %.3e; merged vs unmerged latent %.3e"
          % (kind, scale, md, err, moved))
    assert "tome_tokens" not in i_off
    # the merged loop sits closer to the oracle loop on its own plans than to the unmerged loop: the bound resolves the feature
    assert err < LATENT_TOL and err < moved
    # the keys give the same loop as the ready object
    assert torch.equal(_sample(sampler, dev, xT, cs, call=call, tome_ratio=0.5, tome_max_downsample=md)[0], z)


@pytest.mark.parametrize("kind", ["ddim", "2m", "unipc", "sde"])
def test_graph_replay_eager_steps_and_a_fresh_sampler_agree_bitwise(tiny, dev, gold, monkeypatch, kind):
    net, _ = tiny
    xT, cs = _gold_case(gold)
    keys = {"seeds": [5, 6]} if kind == "sde" else {}
    shared = _make(kind, net)
    z_off0, i_off = _sample(shared, dev, xT, cs, **keys)                      # before any call with the key
    z_on, i_on = _sample(shared, dev, xT, cs, tome_ratio=0.5, **keys)
    z_off, _ = _sample(shared, dev, xT, cs, **keys)                           # an off-call behind an on-call: its own earlier bits
    assert torch.equal(z_off, z_off0) and not torch.equal(z_on, z_off) and "tome_tokens" not in i_off
    assert i_on["tome_tokens"] == [(256, 128)] * 3
    assert len(shared._static) == 2 and all(st["graph"] is not None for st in shared._static.values())
    assert torch.equal(_sample(shared, dev, xT, cs, tome_ratio=0.5, **keys)[0], z_on)          # the same call twice, on the kept graph
    for off_keys in (dict(tome_ratio=0), dict(tome_ratio=None, tome_max_downsample=2), dict(tome_ratio=0.0)):
        assert torch.equal(_sample(shared, dev, xT, cs, **dict(keys, **off_keys))[0], z_off)
    assert len(shared._static) == 2
    z_two, _ = _sample(shared, dev, xT, cs, tome_ratio=0.5, tome_max_downsample=2, **keys)     # another setting: another graph
    assert not torch.equal(z_two, z_on) and not torch.equal(z_two, z_off)
    assert torch.equal(_sample(_make(kind, net), dev, xT, cs, tome_ratio=0.5, **keys)[0], z_on)       # a fresh sampler
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = _make(kind, net)
    assert not eager.use_graph
    assert torch.equal(_sample(eager, dev, xT, cs, tome_ratio=0.5, **keys)[0], z_on)
    assert torch.equal(_sample(eager, dev, xT, cs, tome_ratio=0.5, tome_max_downsample=2, **keys)[0], z_two)
    assert torch.equal(_sample(eager, dev, xT, cs, **keys)[0], z_off)


def test_multicontext_eager_ddim_and_single_steps_honour_the_keys(tiny, dev, gold):
    from lib.model_zoo.ddim import DDIMSampler
    net, _ = tiny
    xT, cs = _gold_case(gold)
    g = torch.Generator().manual_seed(9)
    img = _ci((torch.randn((2, 50, 128), generator=g) * 0.5), (torch.randn((2, 50, 128), generator=g) * 0.5), 7.5, "image", ratio=0.6)
    s = _make("2m", net)
    multi = lambda **kw: s.sample_multicontext(steps=5, shape=SHAPE, x_info=dict({"type": "image", "xt": xT.half().to(dev)}, **kw),
                                               c_info_list=[dict(_on_dev(cs[0], dev), ratio=0.4), _on_dev(img, dev)], verbose=False)
    z_on, inter = multi(tome_ratio=0.5)
    z_off, _ = multi()
    assert inter["tome_tokens"] == [(256, 128)] * 3 and rel_l2(z_on, z_off) > 1e-3 and torch.equal(multi(tome_ratio=0.5)[0], z_on)
    outs = []
    for keys in ({"tome_ratio": 0.5}, {"tome_ratio": 0.5, "tome_max_downsample": 1}, {}, {"tome_ratio": 0}):
        torch.manual_seed(3)
        outs.append(_sample(DDIMSampler(net), dev, xT, cs, steps=5, call={"eta": 0.5}, **keys)[0])     # the eager loop (eta > 0)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3]) and rel_l2(outs[0], outs[2]) > 1e-3
    s = DDIMSampler(net)
    s.make_schedule(5, verbose=False)
    t = torch.full((2,), int(s.ddim_timesteps[4]), dtype=torch.long, device=dev)
    x = xT.half().to(dev)
    c = _on_dev(cs[0], dev)
    step = lambda **kw: s.p_sample_ddim(dict({"type": "image", "x": x}, **kw), c, t, 4)[0]
    assert torch.equal(step(tome_ratio=0), step()) and rel_l2(step(tome_ratio=0.5), step()) > 1e-3


def test_with_windows_deepcache_freeu_rescale_and_inpainting(tiny, dev, gold):
    """The combinations none of which touch attn1: each runs on its kept graph, differs from its unmerged twin and repeats its bits."""
    net, _ = tiny
    xT, cs = _gold_case(gold)
    g = torch.Generator().manual_seed(4)
    wide = torch.randn((2, 4, 16, 24), generator=g)
    mask = torch.zeros((2, 1, 16, 16))
    mask[:, :, :, :8] = 1
    cases = [
        (dict(window=16), wide, {}),
        (dict(cache_interval=2, cache_depth=1), xT, {}),
        (dict(freeu=(1.1, 1.2, 0.9, 0.8)), xT, {}),
        (dict(), xT, {"guidance_rescale": 0.7}),
        (dict(inpaint_mask=mask.half().to(dev), x0=xT.half().to(dev)), xT, {}),
    ]
    for keys, x0, c_keys in cases:
        s = _make("2m", net)
        z_on, inter = _sample(s, dev, x0, cs, steps=5, c_keys=c_keys, tome_ratio=0.5, **keys)
        z_off, _ = _sample(s, dev, x0, cs, steps=5, c_keys=c_keys, **keys)
        assert inter["tome_tokens"] == [(256, 128)] * 3, keys       # with a window: the window's grid, not the canvas'
        assert rel_l2(z_on, z_off) > 1e-3, keys
        assert torch.equal(_sample(s, dev, x0, cs, steps=5, c_keys=c_keys, tome_ratio=0.5, **keys)[0], z_on), keys


def test_value_errors_on_the_device_path(tiny, dev, gold):
    from lib.model_zoo.vd import TokenMerge
    net, _ = tiny
    xT, cs = _gold_case(gold)
    s = _make("ddim", net)
    tm = TokenMerge(0.5)
    tm.record = []
    with pytest.raises(ValueError, match="tome.*record"):
        _sample(s, dev, xT, cs, tome=tm)                      # the static loop captures its steps
    assert tm.record == []
    with pytest.raises(ValueError, match="tome.*pag"):
        _sample(s, dev, xT, cs, tome_ratio=0.5, pag_scale=3.0)
    with pytest.raises(ValueError, match="tome.*odd"):
        _sample(s, dev, torch.zeros(2, 4, 16, 18), cs, tome_ratio=0.5, tome_max_downsample=2)
    x, ctx = _inputs(5, 2, False, True)
    with pytest.raises(ValueError, match="tome.*pag"):
        _fwd(net, dev, x, 500, ctx, 3, tome=TokenMerge(0.5), pag=("mid", 4))
    with pytest.raises(ValueError, match="tome"):
        _fwd(net, dev, x, 500, ctx, 2, tome=0.5)
