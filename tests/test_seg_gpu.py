"""Smoothed energy guidance on the GPU: the query-blur entry (vd_attention_qblur_f16 through ops.attention(blur_from=..., blur=...))
bit for bit on exact operands and per element on random ones, the forward with x_info['seg'] against the oracle walk of
tests/seg_cases.py, the four samplers' loops against the oracle loop, graph replay against eager steps, the kept graph across scales
and sigmas, the launch counts, and the combinations with the guidance rescale, inpainting, FreeU, windows, the multi-context entry
and the sharded helper."""
import numpy as np
import pytest
import torch

import seg_cases as sc
import window_cases as wc
from seg_cases import FWD_TOL, INF, LATENT_TOL, LOOP_LAYERS, SEG_SCALE
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


# ---- 1. the entry ------------------------------------------------------------------------------------------------------------------

def _operands(host_q, dev, g, fused):
    """q | k | v on the device for the fp16 host queries [B, N, C]: three contiguous tensors, or the column blocks of one fused
    [B, N, 3 C] projection (ld = 3 C); k and v are random."""
    B, N, C = host_q.shape
    k, v = torch.randn((B, N, C), generator=g).half(), torch.randn((B, N, C), generator=g).half()
    if fused:
        buf = torch.cat([host_q, k, v], -1).to(dev)
        return buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:]
    return host_q.to(dev), k.to(dev), v.to(dev)


def _check_call(ops, q, k, v, heads, bf, taps, R, gh, gw, want_qb=None):
    """One call of the entry with a workspace of its own: the leading samples are the plain call on them alone, the blurred samples
    the plain call on the workspace, both bit for bit; returns the workspace rows it wrote.  want_qb: their expected bits."""
    B, N, C = q.shape
    qb = torch.full(((B - bf) * N * C + 8,), 7.0, dtype=torch.float16, device=q.device)
    out = ops.attention(q, k, v, heads, blur_from=bf, blur=(taps, R, gh, gw), qb=qb)
    assert out.dtype == torch.float16 and tuple(out.shape) == (B, N, C) and out.is_contiguous()
    assert bool((qb[(B - bf) * N * C:] == 7.0).all())                         # nothing behind the blurred samples' rows is written
    got = qb[:(B - bf) * N * C].view(B - bf, N, C)
    if bf > 0:
        assert torch.equal(bits(out[:bf]), bits(ops.attention(q[:bf], k[:bf], v[:bf], heads))), (bf, "a call on those samples alone")
    if bf < B:
        if want_qb is not None:
            assert torch.equal(bits(got), bits(want_qb[bf:])), (bf, "the blurred queries")
        assert torch.equal(bits(out[bf:]), bits(ops.attention(got, k[bf:], v[bf:], heads))), (bf, "the plain call on the workspace")
    return got


@pytest.mark.parametrize("H,D", sc.HEAD_DIMS)
@pytest.mark.parametrize("grid,R", sc.EXACT_GRIDS)
def test_exact_operands_give_the_float64_formula_bit_for_bit(dev, grid, R, H, D):
    from vd_hip import ops
    (gh, gw), C, B = grid, H * D, 3
    g = torch.Generator().manual_seed(1000 * gh + 10 * gw + R + D)
    host = torch.randint(-8, 9, (B, gh * gw, C), generator=g).half()
    w = sc.DYADIC[R]
    ref = sc.blur64(host, gh, gw, w, R)
    taps = torch.tensor(w, dtype=torch.float32, device=dev)
    for fused in (False, True):
        q, k, v = _operands(host, dev, g, fused)
        for bf in (0, 1, B):
            _check_call(ops, q, k, v, H, bf, taps, R, gh, gw, ref.half())
        assert torch.equal(q.cpu(), host)                                        # the queries themselves are untouched
    if (gh * gw) & (gh * gw - 1) == 0:                                           # mean mode with N a power of two
        mref = sc.blur64(host, gh, gw, None, -1)
        q, k, v = _operands(host, dev, g, True)
        for bf in (0, 1):
            _check_call(ops, q, k, v, H, bf, None, -1, gh, gw, mref.half())


@pytest.mark.parametrize("grid,H,D,sigma", sc.RANDOM_CASES)
def test_random_operands_stay_inside_the_per_element_bound(dev, grid, H, D, sigma):
    from lib.model_zoo.vd import seg_taps
    from vd_hip import ops
    (gh, gw), C, B = grid, H * D, 2
    g = torch.Generator().manual_seed(int(100 * sigma) + gh + gw)
    host = (torch.randn((B, gh * gw, C), generator=g) * 1.5 + 0.1).half()
    R, w = seg_taps(sigma)
    taps = torch.from_numpy(w).to(dev)
    ref, bound = sc.blur_bound(host, gh, gw, w, R)
    for fused, bf in ((True, 0), (False, 1)):
        q, k, v = _operands(host, dev, g, fused)
        got = _check_call(ops, q, k, v, H, bf, taps, R, gh, gw)
        err = (got.double().cpu() - ref[bf:]).abs().numpy()
        print("grid %r H D %d x %d sigma %.1f (R %d) blur_from %d: max |qb - ref64| / bound %.3f" % (grid, H, D, sigma, R, bf, float((err / bound[bf:]).max())))
        assert (err <= bound[bf:]).all()
        assert torch.equal(bits(_check_call(ops, q, k, v, H, bf, taps, R, gh, gw)), bits(got))           # a second run: the same bits


@pytest.mark.parametrize("grid", sc.MEAN_GRIDS)
def test_mean_mode_stays_inside_its_bound_and_repeats_its_bits(dev, grid):
    from vd_hip import ops
    (gh, gw), H, D, B = grid, 2, 40, 3
    g = torch.Generator().manual_seed(gh * 100 + gw)
    host = (torch.randn((B, gh * gw, H * D), generator=g) * 1.5 + 0.1).half()
    ref, bound = sc.mean_bound(host)
    q, k, v = _operands(host, dev, g, True)
    got = _check_call(ops, q, k, v, H, 1, None, -1, gh, gw)
    err = (got.double().cpu() - ref[1:]).abs().numpy()
    print("grid %r mean mode: max |qb - ref64| / bound %.3f" % (grid, float((err / bound[1:]).max())))
    assert (err <= bound[1:]).all()
    assert torch.equal(bits(_check_call(ops, q, k, v, H, 1, None, -1, gh, gw)), bits(got))
    alone = _check_call(ops, q[2:], k[2:], v[2:], H, 0, None, -1, gh, gw)         # a sample's mean does not see its batch
    assert torch.equal(bits(alone[0]), bits(got[1]))


def test_the_largest_layer_one_blurred_sample(dev):
    """64 x 64 tokens, H D = 320, R = 3 (sigma 1), one blurred sample behind one plain one: finite mode and the mean."""
    from lib.model_zoo.vd import seg_taps
    from vd_hip import ops
    gh = gw = 64
    H, D = 8, 40
    g = torch.Generator().manual_seed(64)
    host = (torch.randn((2, gh * gw, H * D), generator=g) * 1.5 + 0.1).half()
    R, w = seg_taps(1.0)
    assert R == 3
    q, k, v = _operands(host, dev, g, True)
    got = _check_call(ops, q, k, v, H, 1, torch.from_numpy(w).to(dev), R, gh, gw)
    ref, bound = sc.blur_bound(host[1:], gh, gw, w, R)
    err = (got.double().cpu() - ref).abs().numpy()
    print("64 x 64 x 320, R 3: max |qb - ref64| / bound %.3f" % float((err / bound).max()))
    assert (err <= bound).all()
    mgot = _check_call(ops, q, k, v, H, 1, None, -1, gh, gw)
    mref, mbound = sc.mean_bound(host[1:])
    assert ((mgot.double().cpu() - mref).abs().numpy() <= mbound).all()


def test_entry_refuses_bad_arguments(dev):
    from vd_hip import ops
    t = lambda *s: torch.zeros(s, dtype=torch.float16, device=dev)
    q = t(3, 64, 80)
    taps = torch.tensor([0.25, 0.5, 0.25], dtype=torch.float32, device=dev)
    ok = dict(k=q, v=q, blur_from=1, blur=(taps, 1, 8, 8))
    assert tuple(ops.attention(q, q, q, 2, blur_from=1, blur=(taps, 1, 8, 8)).shape) == (3, 64, 80)
    bad = [dict(k=t(3, 96, 80), v=t(3, 96, 80)),                                  # Nq != Nk
           dict(causal=True), dict(blur_from=-1), dict(blur_from=4), dict(blur=(taps, 1, 8, 9)), dict(blur=(taps, 1, 4, 8)),
           dict(blur=(taps, -2, 8, 8)), dict(blur=(None, -3, 8, 8))]
    for kw in bad:
        a = dict(ok, **kw)
        with pytest.raises(ops.VdHipError, match="vd_attention_qblur_f16"):
            ops.attention(q, a.pop("k"), a.pop("v"), 2, **a)
    odd = t(3, 64, 3 * 80 + 4)                                                  # ld = 244: rows lose their 16-byte alignment
    with pytest.raises(ops.VdHipError, match="vd_attention_qblur_f16"):
        ops.attention(odd[..., :80], odd[..., 80:160], odd[..., 160:240], 2, blur_from=1, blur=(taps, 1, 8, 8))
    shifted = t(3, 64, 3 * 80 + 8)                                              # column offset 4: q is not 16-byte aligned
    with pytest.raises(ops.VdHipError, match="vd_attention_qblur_f16"):
        ops.attention(shifted[..., 4:84], shifted[..., 84:164], shifted[..., 164:244], 2, blur_from=1, blur=(taps, 1, 8, 8))
    with pytest.raises(ops.VdHipError, match="vd_attention_qblur_f16"):        # a workspace that is not 16-byte aligned
        ops.attention(q, q, q, 2, blur_from=1, blur=(taps, 1, 8, 8), qb=t(2 * 64 * 80 + 8)[4:])
    with pytest.raises(ops.VdHipError, match="vd_attention_qblur_f16.*head dim"):
        ops.attention(t(2, 64, 48), t(2, 64, 48), t(2, 64, 48), 1, blur_from=1, blur=(taps, 1, 8, 8))      # what the plain entry refuses
    for kw in (dict(blur_from=1), dict(blur=(taps, 1, 8, 8)), dict(blur_from=1.0, blur=(taps, 1, 8, 8)), dict(blur_from=1, blur=(taps, 1, 8)),
               dict(blur_from=1, blur=(None, 1, 8, 8)), dict(blur_from=1, blur=(taps, 2, 8, 8)), dict(blur_from=1, blur=(taps, 1, 8, 8), ident_from=1),
               dict(blur_from=1, blur=(taps, 1, 8, 8), qb=t(16))):
        with pytest.raises(ops.VdHipError, match="blur|taps|qb"):
            ops.attention(q, q, q, 2, **kw)


# ---- 2. the forward --------------------------------------------------------------------------------------------------------------

def _inputs(seed, B, dual, reps, guided):
    """x [B, 4, 16, 16] and the contexts of `reps` replicas: the perturbed one (the last, when reps counts one) repeats the
    conditional rows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, 16, 16), generator=g).half().float()
    seg = reps > (2 if guided else 1)

    def rows(L):
        base = (torch.randn(((2 if guided else 1) * B, L, 128), generator=g) * 0.5).half().float()
        return torch.cat([base, base[-B:]]) if seg else base

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


def _oracle(sd, plan, x, t, ctx, reps, layers=(), row0=None, sigma=INF):
    xin = torch.cat([x] * reps)
    mask = torch.zeros((xin.shape[0],), dtype=torch.bool)
    if row0 is not None:
        mask[row0:] = True
    return sc.walk(sd, plan, xin, torch.full((xin.shape[0],), t, dtype=torch.long), ctx, sc.layers_of(plan, layers) if row0 is not None else (),
                   mask, sigma)


@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("layers,dual", [(sc.LAYER_CASES[0], False), (sc.LAYER_CASES[1], False), (sc.LAYER_CASES[1], True)])
def test_forward_vs_the_oracle_walk_replica_by_replica(tiny, plan, dev, layers, dual, guided, sigma):
    net, sd = tiny
    B, reps = 2, 3 if guided else 2
    x, ctx = _inputs(71 + dual + 2 * guided, B, dual, reps, guided)
    row0 = (reps - 1) * B
    ref = _oracle(sd, plan, x, 500, ctx, reps, layers, row0, sigma)
    gap = rel_l2(ref[row0:], ref[row0 - B:row0])
    assert gap >= 10 * FWD_TOL                      # precondition, on the oracle alone: the bound tells perturbed from conditional
    e = _fwd(net, dev, x, 500, ctx, reps, seg=(layers, row0, sigma))
    assert e.dtype == torch.float16 and tuple(e.shape) == (reps * B, 4, 16, 16)
    errs = [rel_l2(e[r * B:(r + 1) * B], ref[r * B:(r + 1) * B]) for r in range(reps)]
    plain = _fwd(net, dev, x, 500, [(ct, c[:row0], r) for ct, c, r in ctx], reps - 1)      # today's forward on the leading replicas
    lead = rel_l2(e[:row0], plain)
    print("layers %r dual %d guided %d sigma %r: replicas vs the oracle walk %s; e_p vs e_c on the oracle %.3f; leading replicas vs the "
          "plain forward %.3e" % (layers, dual, guided, sigma, ["%.3e" % v for v in errs], gap, lead))
    assert all(v < FWD_TOL for v in errs)
    assert lead < FWD_TOL and rel_l2(e[row0:], plain[-B:]) > 5 * FWD_TOL
    assert torch.equal(_fwd(net, dev, x, 500, ctx, reps, seg=(list(reversed(layers)), row0, sigma)), e)      # the normalised tuple


def test_forward_without_the_key_is_todays_forward(tiny, dev):
    net, _ = tiny
    for guided in (True, False):
        reps = 2 if guided else 1
        x, ctx = _inputs(81, 2, False, reps, guided)
        plain = _fwd(net, dev, x, 500, ctx, reps)
        assert torch.equal(_fwd(net, dev, x, 500, ctx, reps, seg=None), plain)
        assert torch.equal(_fwd(net, dev, x, 500, ctx, reps), plain)
    # no row perturbed (row0 = all rows): the softmax path of every sample, through the replicated (unshared) entry
    x, ctx = _inputs(82, 2, False, 2, True)
    e = _fwd(net, dev, x, 500, ctx, 2, seg=((0, 2), 4, 1.0))
    assert rel_l2(e, _fwd(net, dev, x, 500, ctx, 2)) < 1e-3


def test_forward_inside_the_half_batch_fork_where_the_boundary_cuts_the_replicas(tiny, plan, dev, monkeypatch):
    """VD_BATCH_FORK=1 semantics at B = 4, three replicas: the 8 x 8 level and the middle block run as two branches of rows [0, 6)
    and [6, 12) while the perturbed rows are [8, 12): the second branch gets blur_from = 2, the first 6 (nothing blurred).  (The
    threshold is lowered to 64 rows per sample, which puts the fork where a 32 x 32 latent has it.)  With a workspace (a captured
    step's) the two branches write disjoint rows of it."""
    from lib.model_zoo import vd
    from vd_hip import ops
    net, sd = tiny
    x, ctx = _inputs(91, 4, False, 3, True)
    seen, real = [], ops.attention

    def counted(q, k, v, heads, **kw):
        if kw.get("blur_from") is not None:
            seen.append((q.shape[0], kw["blur_from"], None if kw.get("qb") is None else kw["qb"].numel()))
        return real(q, k, v, heads, **kw)

    monkeypatch.setattr(ops, "attention", counted)
    monkeypatch.setattr(vd, "BATCH_FORK", "1")
    monkeypatch.setattr(vd, "BATCH_FORK_HW", 64)
    key = ((1, 2, 3), 8, 1.0)
    e = _fwd(net, dev, x, 500, ctx, 3, seg=key)
    assert sorted(seen) == [(6, 2, None)] * 3 + [(6, 6, None)] * 3            # one blur-path call per (layer, branch)
    assert torch.equal(_fwd(net, dev, x, 500, ctx, 3, seg=key), e)
    ref = _oracle(sd, plan, x, 500, ctx, 3, (1, 2, 3), 8, 1.0)
    assert all(rel_l2(e[r * 4:(r + 1) * 4], ref[r * 4:(r + 1) * 4]) < FWD_TOL for r in range(3))
    seen.clear()
    elems = vd.seg_workspace_elems(net, ["text"], 16, 16, (1, 2, 3))
    assert elems == 8 * 8 * 128
    bufs = (torch.from_numpy(vd.seg_taps(1.0)[1]).to(dev), torch.zeros((1, 4, elems), dtype=torch.float16, device=dev))
    assert torch.equal(_fwd(net, dev, x, 500, ctx, 3, seg=key, seg_buffers=bufs), e)
    assert sorted(seen) == [(6, 2, 4 * elems)] * 3 + [(6, 6, None)] * 3       # the branch with four blurred rows: four rows of it
    assert bool((bufs[1] != 0).any())
    seen.clear()
    monkeypatch.setattr(vd, "BATCH_FORK", "0")
    assert rel_l2(_fwd(net, dev, x, 500, ctx, 3, seg=key), e) < 1e-3 and seen == [(12, 8, None)] * 3


@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("C,side", [(320, 16), (640, 8), (1280, 8)])
def test_one_block_at_the_full_widths_vs_the_oracle_block(dev, C, side, sigma):
    """The tiny net has widths 64 and 128 only.  One SpatialTransformer at each full width -- 320: q | k | v arrive from the chained
    entry kernel and the tail is the one-launch chain; 640 / 1280: the block's own fused projection -- with seeded weights (proj_out
    not left at zero), B = 3, blur_from = 1, against the oracle block of tests/seg_cases.py on the same fp16-rounded weights.
    Compared on what the block adds to its input (out - x), sample by sample, with the project's forward bound."""
    from lib.model_zoo.attention import SpatialTransformer
    from lib.model_zoo.vd import seg_taps
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
    x = torch.randn((3, C, side, side), generator=g).half().float()
    ctx = (torch.randn((3, 77, 768), generator=g) * 0.5).half().float()
    mask = torch.tensor([False, True, True])
    with torch.no_grad():
        ref = sc.spatial_transformer(sd, "b", x, ctx, heads, mask, sigma) - x
        off = sc.spatial_transformer(sd, "b", x, ctx, heads, torch.zeros(3, dtype=torch.bool), sigma) - x
    gap = rel_l2(ref[1:], off[1:])
    assert gap >= 10 * FWD_TOL and rel_l2(ref[:1], off[:1]) < 1e-6       # precondition, on the oracle alone
    st = st.half().to(dev)
    xd = x.permute(0, 2, 3, 1).contiguous().half().to(dev)
    R, w = seg_taps(sigma)
    out = st(xd, ctx.half().to(dev), blur_from=1, blur=(None if w is None else torch.from_numpy(w).to(dev), R))
    delta = (out.float() - xd.float()).permute(0, 3, 1, 2).cpu()
    errs = [rel_l2(delta[b], ref[b]) for b in range(3)]
    plain = (st(xd, ctx.half().to(dev)).float() - xd.float()).permute(0, 3, 1, 2).cpu()
    print("width %d sigma %r: block delta vs the oracle block per sample %s; plain block vs the oracle without SEG %.3e; oracle perturbed "
          "vs not %.3f" % (C, sigma, ["%.3e" % e for e in errs], rel_l2(plain, off), gap))
    assert all(e < FWD_TOL for e in errs)
    assert rel_l2(plain, off) < FWD_TOL and rel_l2(delta[1:], off[1:]) > 5 * FWD_TOL


# ---- 3. loops --------------------------------------------------------------------------------------------------------------------

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


def _seg(sigma=INF, scale=SEG_SCALE, layers=LOOP_LAYERS):
    return {"seg_scale": scale, "seg_blur_sigma": sigma, "seg_layers": layers}


def _sample(sampler, dev, xT, cs, steps=5, c_keys=None, call=None, **keys):
    x_info = dict({"type": "image", "xt": xT.half().to(dev)}, **keys)
    c = dict(_on_dev(cs[0], dev), **(c_keys or {}))
    return sampler.sample(steps=steps, shape=list(xT.shape), x_info=x_info, c_info=c, verbose=False, **(call or {}))


_OFF = {}


def _off_loop(sd, plan, sampler, base, kind, xT, cs, scale, noise=None, **kw):
    """The oracle loop without SEG, computed once per (kind, scale, extras) and shared."""
    key = (kind, scale, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _OFF:
        _OFF[key] = sc.oracle_loop(sd, plan, sampler, base, xT, cs, scale, 0.0, noise=noise, **kw)
    return _OFF[key]


@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("kind,scale", [("ddim", 7.5), ("2m", 7.5), ("unipc", 7.5), ("sde0", 7.5), ("sde1", 7.5), ("ddim", 1.0), ("2m", 1.0),
                                        ("unipc", 1.0), ("sde0", 1.0), ("sde1", 1.0)])
def test_five_step_loops_vs_the_oracle_loop(tiny, plan, dev, gold, kind, scale, sigma):
    from test_philox_cpu import normals_ref_batch
    net, sd = tiny
    xT, cs = _gold_case(gold, scale)
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
    z, inter = _sample(sampler, dev, xT, cs, call=call, **dict(keys, **_seg(sigma)))
    assert len(sampler.ddim_timesteps) == 5 and inter["seg_layers"] == LOOP_LAYERS and "pag_layers" not in inter
    ref = sc.oracle_loop(sd, plan, sampler, base, xT, cs, scale, SEG_SCALE, LOOP_LAYERS, sigma, noise=noise)
    off = _off_loop(sd, plan, sampler, base, kind, xT, cs, scale, noise=noise)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("%s s %.1f sigma %r: final latent vs the oracle loop with SEG %.3e; oracle loop on vs off %.3e; latent vs the oracle loop off %.3e"
          % (kind, scale, sigma, err, gap, rel_l2(z, off)))
    assert gap > LATENT_TOL                  # precondition, on the oracle alone
    assert err < LATENT_TOL and err < rel_l2(z, off)


@pytest.mark.parametrize("kind", ["ddim", "2m", "unipc", "sde"])
def test_graph_replay_eager_steps_and_a_fresh_sampler_agree_bitwise(tiny, dev, gold, monkeypatch, kind):
    net, _ = tiny
    xT, cs = _gold_case(gold)
    keys = {"seeds": [5, 6]} if kind == "sde" else {}
    run = lambda s, **kw: _sample(s, dev, xT, cs, **dict(keys, **kw))
    shared = _make(kind, net)
    z_off0, i_off = run(shared)                                                # before any call with the key
    k_off = list(shared._static)
    z_on, _ = run(shared, **_seg(1.0))
    z_off, _ = run(shared)                                                     # an off-call behind an on-call: its own earlier bits
    assert torch.equal(z_off, z_off0) and not torch.equal(z_on, z_off) and "seg_layers" not in i_off
    assert len(shared._static) == 2 and all(st["graph"] is not None for st in shared._static.values())
    assert k_off[0] in shared._static                                          # today's graph key, unchanged
    on_state = [st for st in shared._static.values() if "seg_qb" in st]
    assert len(on_state) == 1 and "pag_w" in on_state[0] and tuple(on_state[0]["seg_taps"].shape) == (7,)
    graph = on_state[0]["graph"]
    assert torch.equal(run(shared, **_seg(1.0))[0], z_on)                      # on the kept graph
    for off_keys in (dict(seg_scale=0), dict(seg_scale=None, seg_layers=[1], seg_blur_sigma=1.0), dict(seg_scale=0.0, seg_blur_sigma=-3)):
        assert torch.equal(run(shared, **off_keys)[0], z_off)
    # a second scale and a second sigma of the same R = 3 replay the same kept graph with another weight and other taps
    z_two, _ = run(shared, **_seg(1.0, scale=1.5))
    z_sig, _ = run(shared, **_seg(1.15))
    mine = lambda: [st for st in shared._static.values() if "seg_qb" in st]
    assert len(shared._static) == 2 and len(mine()) == 1 and mine()[0] is on_state[0] and on_state[0]["graph"] is graph
    assert len({bits(z).numpy().tobytes() for z in (z_on, z_two, z_sig, z_off)}) == 4
    assert torch.equal(run(_make(kind, net), **_seg(1.0))[0], z_on)            # a fresh sampler
    assert torch.equal(run(_make(kind, net), **_seg(1.0, scale=1.5))[0], z_two)
    assert torch.equal(run(_make(kind, net), **_seg(1.15))[0], z_sig)
    # another R (sigma 0.5: R = 1; infinity: the mean query) captures again
    z_r1, _ = run(shared, **_seg(0.5))
    r1_state = [st for st in mine() if st is not on_state[0]]
    assert len(r1_state) == 1 and r1_state[0]["graph"] is not None and r1_state[0]["graph"] is not graph
    assert tuple(r1_state[0]["seg_taps"].shape) == (3,) and not torch.equal(z_r1, z_on)
    z_inf, _ = run(shared, **_seg(INF))
    inf_state = [st for st in mine() if st["seg_taps"] is None]
    assert len(inf_state) == 1 and inf_state[0]["graph"] is not None and not torch.equal(z_inf, z_on)
    assert torch.equal(run(shared, **_seg(1e4))[0], z_inf) and len([st for st in mine() if st["seg_taps"] is None]) == 1   # every sigma of the mean mode
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = _make(kind, net)
    assert not eager.use_graph
    assert torch.equal(run(eager, **_seg(1.0))[0], z_on)
    assert torch.equal(run(eager, **_seg(INF))[0], z_inf)
    assert torch.equal(run(eager)[0], z_off)


def test_unguided_graph_serves_every_scale_and_off_keeps_its_bits(tiny, dev, gold):
    net, _ = tiny
    xT, cs = _gold_case(gold, 1.0)
    s = _make("2m", net)
    z_off = _sample(s, dev, xT, cs)[0]
    z_a = _sample(s, dev, xT, cs, **_seg())[0]
    z_b = _sample(s, dev, xT, cs, **_seg(scale=0.5))[0]
    assert len(s._static) == 2 and not torch.equal(z_a, z_b) and not torch.equal(z_a, z_off)
    assert torch.equal(_sample(s, dev, xT, cs)[0], z_off) and torch.equal(_sample(s, dev, xT, cs, **_seg())[0], z_a)


def test_eager_ddim_loop_and_single_steps_honour_the_keys(tiny, dev, gold):
    from lib.model_zoo.ddim import DDIMSampler
    net, _ = tiny
    xT, cs = _gold_case(gold)
    outs = []
    for keys in (_seg(), dict(_seg(), seg_blur_sigma=None), {}, {"seg_scale": 0}):
        torch.manual_seed(3)
        z, inter = _sample(DDIMSampler(net), dev, xT, cs, call={"eta": 0.5}, **keys)
        assert ("seg_layers" in inter) == bool(keys.get("seg_scale"))
        outs.append(z)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3]) and rel_l2(outs[0], outs[2]) > 1e-3
    s = DDIMSampler(net)
    s.make_schedule(5, verbose=False)
    t = torch.full((2,), int(s.ddim_timesteps[4]), dtype=torch.long, device=dev)
    x = xT.half().to(dev)
    for scale in (7.5, 1.0):
        c = _on_dev(_gold_case(gold, scale)[1][0], dev)
        step = lambda **kw: (torch.manual_seed(1), s.p_sample_ddim(dict({"type": "image", "x": x}, **kw), c, t, 4)[0])[1]
        on, off, zero = step(**_seg(1.0)), step(), step(seg_scale=0, seg_layers=[9])
        assert torch.equal(zero, off) and rel_l2(on, off) > 1e-4 and torch.equal(step(**_seg(1.0, layers=[3, 2, 1, 0])), on)
        assert not torch.equal(step(**_seg(INF)), on) and not torch.equal(step(**_seg(1.0, layers=[0])), on)


def test_multicontext_loop_vs_the_oracle_loop(tiny, plan, dev, gold):
    net, sd = tiny
    xT, cs = _gold_case(gold)
    cs = [dict(cs[0], ratio=0.4), _ci(torch.from_numpy(gold["c_img"]), torch.from_numpy(gold["u_img"]), 7.5, "image", ratio=0.6)]
    sampler = _make("2m", net)
    z, _ = sampler.sample_multicontext(steps=5, shape=SHAPE, x_info=dict({"type": "image", "xt": xT.half().to(dev)}, **_seg(1.0)),
                                       c_info_list=[_on_dev(c, dev) for c in cs], verbose=False)
    ref = sc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, SEG_SCALE, LOOP_LAYERS, 1.0)
    off = sc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, 0.0)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("dual 2m: final latent vs the oracle loop with SEG %.3e; oracle on vs off %.3e" % (err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, off)


# ---- 4. combinations ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma", sc.SIGMAS)
def test_with_guidance_rescale_vs_the_oracle_loop(tiny, plan, dev, gold, sigma):
    """The rescale targets the standard deviation of the unperturbed e_c, as with pag."""
    net, sd = tiny
    xT, cs = _gold_case(gold)
    sampler = _make("ddim", net)
    z, inter = _sample(sampler, dev, xT, cs, c_keys={"guidance_rescale": 0.7}, **_seg(sigma))
    assert len(inter["guidance_rescale"]) >= 1
    ref = sc.oracle_loop(sd, plan, sampler, "ddim", xT, cs, 7.5, SEG_SCALE, LOOP_LAYERS, sigma, phi=0.7)
    off = _off_loop(sd, plan, sampler, "ddim", "ddim", xT, cs, 7.5, phi=0.7)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("rescaled ddim sigma %r: loop with SEG vs the oracle loop %.3e; oracle on vs off %.3e" % (sigma, err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, off)


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
    z, z_off = run(**_seg(1.0)), run()
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(z[keep], x0[keep]) and bool(torch.isfinite(z).all())
    assert rel_l2(z[~keep], z_off[~keep]) > LATENT_TOL


@pytest.mark.parametrize("sigma", sc.SIGMAS)
def test_with_freeu_on_top_vs_the_oracle_with_both(tiny, plan, dev, gold, sigma):
    from freeu_cases import SETTING
    net, sd = tiny
    xT, cs = _gold_case(gold)
    sampler = _make("2m", net)
    z, _ = _sample(sampler, dev, xT, cs, freeu=SETTING, **_seg(sigma))
    ref = sc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, SEG_SCALE, LOOP_LAYERS, sigma, setting=SETTING)
    only_freeu = _off_loop(sd, plan, sampler, "2m", "2m", xT, cs, 7.5, setting=SETTING)
    err, gap = rel_l2(z, ref), rel_l2(ref, only_freeu)
    print("2m with FreeU and SEG sigma %r vs the oracle with both %.3e; oracle both vs FreeU alone %.3e" % (sigma, err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, only_freeu)


@pytest.mark.parametrize("sigma", sc.SIGMAS)
def test_with_windows_vs_per_window_oracle_forwards_merged(tiny, plan, dev, sigma):
    """Each window is a sample with a token grid of its own: the blur runs over the window's grid, not the canvas's."""
    net, sd = tiny
    g = torch.Generator().manual_seed(61)
    shape = (1, 4, 16, 32)
    xT = torch.randn(shape, generator=g).half().float()
    cs = [_ci((torch.randn((1, 77, 128), generator=g) * 0.5).half().float(), (torch.randn((1, 77, 128), generator=g) * 0.5).half().float(), 7.5)]
    sampler = _make("2m", net)
    z, _ = _sample(sampler, dev, xT, cs, window=16, **_seg(sigma))
    geo = wc.geometry(16, 32, 16, 8)
    assert len(geo["offs"]) == 3
    ref = sc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, SEG_SCALE, LOOP_LAYERS, sigma, geo=geo)
    off = wc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, geo)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("windowed 2m sigma %r: loop with SEG vs the windowed oracle loop %.3e; windowed oracle on vs off %.3e" % (sigma, err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, off)
    assert torch.equal(_sample(sampler, dev, xT, cs, window=16, **_seg(sigma))[0], z)          # on the kept graph


def test_hypertile_combines_while_no_chosen_layer_is_tiled(tiny, dev, gold):
    net, _ = tiny
    xT, cs = _gold_case(gold)
    s = _make("2m", net)
    z = _sample(s, dev, xT, cs, hypertile=8, **_seg(1.0, layers=(1, 2, 3)))[0]       # tiles of 8 cut block 0 (16 x 16), not the 8 x 8 blocks
    assert bool(torch.isfinite(z).all()) and not torch.equal(z, _sample(s, dev, xT, cs, **_seg(1.0, layers=(1, 2, 3)))[0])
    with pytest.raises(ValueError, match="seg.*HyperTile"):
        _sample(s, dev, xT, cs, hypertile=8, **_seg(1.0))


def test_sharded_world1_matches_direct_sample(tiny, dev, gold):
    from lib.model_zoo import sharded
    net, _ = tiny
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dev).half()
    ct = _ci(T(gold["c_text"]), T(gold["u_text"]), 7.5)
    imgs = sharded.vd_sample_sharded(net, _make("2m", net), 5, SHAPE, [dict(ct)], 3, guidance_scale=7.5, device_generator=True,
                                     seg_scale=SEG_SCALE, seg_blur_sigma=1.0, seg_layers=(1, 2))
    torch.manual_seed(103)
    z, _ = _make("2m", net).sample(steps=5, shape=SHAPE, x_info={"type": "image", "seg_scale": SEG_SCALE, "seg_blur_sigma": 1.0, "seg_layers": (1, 2)},
                                   c_info=dict(ct), verbose=False)
    assert torch.equal(imgs, net.vae_decode(z, which="image"))


def test_launch_counts_one_fold_per_step_and_one_blur_call_per_layer_and_type(tiny, dev, gold, monkeypatch):
    from vd_hip import ops
    net, _ = tiny
    xT, cs = _gold_case(gold)
    dual = [dict(cs[0], ratio=0.4), _ci(torch.from_numpy(gold["c_img"]), torch.from_numpy(gold["u_img"]), 7.5, "image", ratio=0.6)]
    folds, blurs, plains, real_fold, real_attn = [], [], [], ops.pag_fold, ops.attention

    def fold(eps, reps, w):
        folds.append((eps.shape[0], reps))
        return real_fold(eps, reps, w)

    def attn(q, k, v, heads, **kw):
        if kw.get("blur_from") is not None:
            blurs.append((q.shape[0], kw["blur_from"], kw["blur"][1]))
        else:
            plains.append(q.shape[0])
        return real_attn(q, k, v, heads, **kw)

    monkeypatch.setattr(ops, "pag_fold", fold)
    monkeypatch.setattr(ops, "attention", attn)
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")                       # eager steps: every launch of every step passes the wrappers
    s = _make("2m", net)
    _sample(s, dev, xT, cs)
    base = len(plains)
    plains.clear()
    _sample(s, dev, xT, cs, seg_scale=0, seg_blur_sigma=1.0)
    assert folds == [] and blurs == [] and len(plains) == base      # off: the launches of a call without the keys
    _sample(s, dev, xT, cs, **_seg(1.0, layers="mid"))
    assert folds == [(6, 3)] * 5 and blurs == [(6, 4, 3)] * 5      # one layer, one type, one branch
    folds.clear(), blurs.clear()
    _sample(s, dev, xT, _gold_case(gold, 1.0)[1], **_seg(INF, layers=(0, 2, 6)))
    assert folds == [(4, 2)] * 5 and blurs == [(4, 2, -1)] * 15
    folds.clear(), blurs.clear()
    s.sample_multicontext(steps=5, shape=SHAPE, x_info=dict({"type": "image", "xt": xT.half().to(dev)}, **_seg(0.5, layers=(1, 2))),
                          c_info_list=[_on_dev(c, dev) for c in dual], verbose=False)
    assert folds == [(6, 3)] * 5 and blurs == [(6, 4, 1)] * (5 * 2 * 2)      # every context type's block at a layer's index
