"""Perturbed-attention guidance on the GPU: the identity entry (vd_attention_ident_f16 through ops.attention(ident_from=...)) and the
fold (vd_pag_fold_f16 through ops.pag_fold) bit for bit and per element, the forward with x_info['pag'] against the oracle walk of
tests/pag_cases.py, the four samplers' loops against the oracle loop, graph replay against eager steps, the kept graph across
scales, and the combinations with the guidance rescale, inpainting, FreeU, windows and the sharded helper."""
import numpy as np
import pytest
import torch

import pag_cases as pc
import window_cases as wc
from pag_cases import FWD_TOL, LATENT_TOL, PAG_SCALE
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


# ---- 1. the identity entry ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", pc.IDENT_ROWS)
@pytest.mark.parametrize("heads", pc.IDENT_HEADS)
@pytest.mark.parametrize("D", pc.IDENT_DIMS)
def test_identity_rows_copy_v_and_the_others_are_the_plain_call(dev, D, heads, N):
    from vd_hip import ops
    C, B = heads * D, 3
    g = torch.Generator().manual_seed(D * 1000 + heads * 100 + N)
    fused = torch.randn((B + 1, N, 3 * C), generator=g).half().to(dev)          # q | k | v of one fused projection, ld = 3 C
    kept = fused.clone()
    for base in (fused[:B], fused[1:]):                                         # the batch, and a batch-slice view of it
        q, k, v = base[..., :C], base[..., C:2 * C], base[..., 2 * C:]
        plain = ops.attention(q, k, v, heads)
        for i in range(B + 1):
            out = ops.attention(q, k, v, heads, ident_from=i)
            assert out.dtype == torch.float16 and tuple(out.shape) == (B, N, C) and out.is_contiguous()
            assert torch.equal(bits(out[i:]), bits(v[i:])), (i, "identity rows are v")
            if i > 0:
                assert torch.equal(bits(out[:i]), bits(ops.attention(q[:i], k[:i], v[:i], heads))), (i, "a call on those samples alone")
                assert torch.equal(bits(out[:i]), bits(plain[:i])), i
        assert not torch.equal(plain, v)
    # into a caller's buffer with a wider row (ldo > H D) and a scale of its own; the second half of a batch of four
    half = fused[2:4]
    q, k, v = half[..., :C], half[..., C:2 * C], half[..., 2 * C:]
    wide = torch.full((2, N, C + 8), 7.0, dtype=torch.float16, device=dev)
    out = ops.attention(q, k, v, heads, scale=0.1, out=wide[..., :C], ident_from=1)
    assert torch.equal(bits(out[1]), bits(v[1])) and torch.equal(bits(out[0]), bits(ops.attention(q[:1], k[:1], v[:1], heads, scale=0.1)[0]))
    assert bool((wide[..., C:] == 7.0).all())
    assert torch.equal(fused, kept)                                             # the inputs are untouched


def test_identity_entry_refuses_bad_arguments(dev):
    from vd_hip import ops
    t = lambda *s: torch.zeros(s, dtype=torch.float16, device=dev)
    q = t(3, 64, 80)
    bad = [dict(k=t(3, 96, 80), v=t(3, 96, 80)),                                  # Nq != Nk
           dict(causal=True), dict(ident_from=-1), dict(ident_from=4)]
    for kw in bad:
        a = dict(dict(k=q, v=q, ident_from=1), **kw)
        with pytest.raises(ops.VdHipError, match="vd_attention_ident_f16"):
            ops.attention(q, a.pop("k"), a.pop("v"), 2, **a)
    odd = t(3, 64, 3 * 80 + 4)                                                  # ld = 244: rows lose their 16-byte alignment
    with pytest.raises(ops.VdHipError, match="vd_attention_ident_f16"):
        ops.attention(odd[..., :80], odd[..., 80:160], odd[..., 160:240], 2, ident_from=1)
    shifted = t(3, 64, 3 * 80 + 8)                                              # column offset 4: v is not 16-byte aligned
    with pytest.raises(ops.VdHipError, match="vd_attention_ident_f16"):
        ops.attention(shifted[..., 4:84], shifted[..., 84:164], shifted[..., 164:244], 2, ident_from=1)
    with pytest.raises(ops.VdHipError, match="vd_attention_ident_f16.*head dim"):
        ops.attention(t(2, 64, 48), t(2, 64, 48), t(2, 64, 48), 1, ident_from=1)      # what the plain entry refuses, under this name
    with pytest.raises(ops.VdHipError, match="ident_from"):
        ops.attention(q, q, q, 2, ident_from=1.0)


# ---- 2. the fold ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reps", [2, 3])
def test_fold_exact_operands_give_the_float64_formula_bit_for_bit(dev, reps):
    from vd_hip import ops
    g = torch.Generator().manual_seed(17 + reps)
    for n in pc.FOLD_SIZES:
        host = torch.randint(-8, 9, (reps, n), generator=g).half()
        for j, w in enumerate(pc.FOLD_WEIGHTS if n < (1 << 20) else pc.FOLD_WEIGHTS[:1]):
            ref = pc.fold_ref64(host, reps, w)
            assert torch.equal(ref.half().double(), ref)                                    # an fp16 value
            # aligned, and (odd j) starting one element into a buffer: no replica is 16-byte aligned, n % 8 or not
            buf = torch.zeros((reps * n + 1,), dtype=torch.float16, device=dev)
            eps = buf[j % 2:j % 2 + reps * n].view(reps, n)
            eps.copy_(host)
            wd = torch.full((1,), w, dtype=torch.float32, device=dev)
            view = ops.pag_fold(eps, reps, wd)
            assert view.data_ptr() == eps.data_ptr() and tuple(view.shape) == (reps - 1, n)
            assert torch.equal(bits(eps[0]), bits(ref.half())), (n, w)
            assert torch.equal(bits(eps[1:]), bits(host[1:])), (n, w, "the other replicas are untouched")
            assert float(wd.item()) == w and float(buf[-1 if j % 2 == 0 else 0].item()) == 0.0


@pytest.mark.parametrize("reps", [2, 3])
def test_fold_random_operands_stay_inside_the_per_element_bound(dev, reps):
    from vd_hip import ops
    from lib.model_zoo.ddim import pag_weight
    g = torch.Generator().manual_seed(23 + reps)
    for n in (4099, 2 * 4 * 16 * 16, 3 * 8192 + 3):
        host = (torch.randn((reps, n), generator=g) * 1.5 + 0.1).half()
        for w in (float(pag_weight(7.5, 3.0, True)), 3.0, float(pag_weight(1.5, 5.0, True)), 0.1):
            eps = host.to(dev)
            ops.pag_fold(eps, reps, torch.full((1,), w, dtype=torch.float32, device=dev))
            err = (eps[0].double().cpu() - pc.fold_ref64(host, reps, w)).abs().numpy()
            bound = pc.fold_bound(host, reps, w)
            print("reps %d n %d w %+.4f: max |out - ref64| / bound %.3f" % (reps, n, w, float((err / bound).max())))
            assert (err <= bound).all()
            assert torch.equal(bits(eps[1:]), bits(host[1:]))


def test_fold_weight_zero_keeps_the_bits_and_a_sample_does_not_see_its_batch(dev):
    from vd_hip import ops
    g = torch.Generator().manual_seed(29)
    wd = lambda w: torch.full((1,), w, dtype=torch.float32, device=dev)
    for reps in (2, 3):
        host = torch.randn((reps, 3, 4, 16, 16), generator=g).half()
        host[0, 0, 0, 0, :4] = torch.tensor([-0.0, 0.0, 65504.0, -6e-8]).half()
        eps = host.to(dev)
        ops.pag_fold(eps, reps, wd(0.0))
        assert torch.equal(bits(eps), bits(host))
        ops.pag_fold(eps, reps, wd(-0.4615))
        assert not torch.equal(bits(eps[0]), bits(host[0])) and torch.equal(bits(eps[1:]), bits(host[1:]))
        for b in range(3):                                    # sample b alone, and in a batch of two
            one = host[:, b:b + 1].contiguous().to(dev)
            ops.pag_fold(one, reps, wd(-0.4615))
            assert torch.equal(bits(one[0, 0]), bits(eps[0, b])), (reps, b)
        pair = host[:, 1:].contiguous().to(dev)
        view = ops.pag_fold(pair.view((reps * 2,) + tuple(host.shape[2:])), reps, wd(-0.4615))
        assert tuple(view.shape) == ((reps - 1) * 2, 4, 16, 16) and torch.equal(bits(view[:2]), bits(eps[0, 1:]))
    for bad in (dict(reps=1), dict(reps=4), dict(reps=True)):
        with pytest.raises(ops.VdHipError, match="pag_fold"):
            ops.pag_fold(torch.zeros((6, 8), dtype=torch.float16, device=dev), bad["reps"], wd(1.0))
    with pytest.raises(ops.VdHipError, match="pag_fold"):
        ops.pag_fold(torch.zeros((4, 8), dtype=torch.float16, device=dev), 3, wd(1.0))


# ---- 3. the forward ------------------------------------------------------------------------------------------------------------

def _inputs(seed, B, dual, reps, guided):
    """x [B, 4, 16, 16] and the contexts of `reps` replicas: the perturbed one (the last, when reps counts one) repeats the
    conditional rows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, 16, 16), generator=g).half().float()
    pag = reps > (2 if guided else 1)

    def rows(L):
        base = (torch.randn(((2 if guided else 1) * B, L, 128), generator=g) * 0.5).half().float()
        return torch.cat([base, base[-B:]]) if pag else base

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


def _oracle(sd, plan, x, t, ctx, reps, layers=(), row0=None):
    xin = torch.cat([x] * reps)
    mask = torch.zeros((xin.shape[0],), dtype=torch.bool)
    if row0 is not None:
        mask[row0:] = True
    return pc.walk(sd, plan, xin, torch.full((xin.shape[0],), t, dtype=torch.long), ctx, pc.layers_of(plan, layers) if row0 is not None else (),
                   mask)


@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("layers,dual", [("mid", False), ("mid", True), ((1, 2, 3), False), ((0,), False)])
def test_forward_vs_the_oracle_walk_replica_by_replica(tiny, plan, dev, layers, dual, guided):
    net, sd = tiny
    B, reps = 2, 3 if guided else 2
    x, ctx = _inputs(71 + dual + 2 * guided, B, dual, reps, guided)
    row0 = (reps - 1) * B
    ref = _oracle(sd, plan, x, 500, ctx, reps, layers, row0)
    gap = rel_l2(ref[row0:], ref[row0 - B:row0])
    assert gap >= 10 * FWD_TOL                      # precondition, on the oracle alone: the bound tells perturbed from conditional
    e = _fwd(net, dev, x, 500, ctx, reps, pag=(layers, row0))
    assert e.dtype == torch.float16 and tuple(e.shape) == (reps * B, 4, 16, 16)
    errs = [rel_l2(e[r * B:(r + 1) * B], ref[r * B:(r + 1) * B]) for r in range(reps)]
    plain = _fwd(net, dev, x, 500, [(ct, c[:row0], r) for ct, c, r in ctx], reps - 1)      # today's forward on the leading replicas
    lead = rel_l2(e[:row0], plain)
    print("layers %r dual %d guided %d: replicas vs the oracle walk %s; e_p vs e_c on the oracle %.3f; leading replicas vs the plain "
          "forward %.3e" % (layers, dual, guided, ["%.3e" % v for v in errs], gap, lead))
    assert all(v < FWD_TOL for v in errs)
    assert lead < FWD_TOL and rel_l2(e[row0:], plain[-B:]) > 5 * FWD_TOL
    if isinstance(layers, tuple):                   # the normalised tuple, a list in another order: the same forward
        assert torch.equal(_fwd(net, dev, x, 500, ctx, reps, pag=(list(reversed(layers)), row0)), e)


def test_forward_without_the_key_is_todays_forward(tiny, dev):
    net, _ = tiny
    for guided in (True, False):
        reps = 2 if guided else 1
        x, ctx = _inputs(81, 2, False, reps, guided)
        plain = _fwd(net, dev, x, 500, ctx, reps)
        assert torch.equal(_fwd(net, dev, x, 500, ctx, reps, pag=None), plain)
        assert torch.equal(_fwd(net, dev, x, 500, ctx, reps), plain)
    # no row perturbed (row0 = all rows): the softmax path of every sample, through the replicated (unshared) entry
    x, ctx = _inputs(82, 2, False, 2, True)
    e = _fwd(net, dev, x, 500, ctx, 2, pag=((0, 2), 4))
    assert rel_l2(e, _fwd(net, dev, x, 500, ctx, 2)) < 1e-3


def test_forward_inside_the_half_batch_fork_where_the_boundary_cuts_the_replicas(tiny, plan, dev, monkeypatch):
    """VD_BATCH_FORK=1 semantics at B = 4, three replicas: the 8 x 8 level and the middle block run as two branches of rows [0, 6)
    and [6, 12) while the perturbed rows are [8, 12): the second branch gets ident_from = 2, the first 6 (nothing perturbed).
    (At a 16 x 16 latent the whole net is below the default threshold of 256 rows per sample and no level would fork: the threshold
    is lowered to 64 rows, which puts the fork where a 32 x 32 latent has it.)"""
    from lib.model_zoo import vd
    from vd_hip import ops
    net, sd = tiny
    x, ctx = _inputs(91, 4, False, 3, True)
    seen, real = [], ops.attention

    def counted(q, k, v, heads, **kw):
        if kw.get("ident_from") is not None:
            seen.append((q.shape[0], kw["ident_from"]))
        return real(q, k, v, heads, **kw)

    monkeypatch.setattr(ops, "attention", counted)
    monkeypatch.setattr(vd, "BATCH_FORK", "1")
    monkeypatch.setattr(vd, "BATCH_FORK_HW", 64)
    e = _fwd(net, dev, x, 500, ctx, 3, pag=((1, 2, 3), 8))
    assert sorted(seen) == [(6, 2)] * 3 + [(6, 6)] * 3            # one identity-path call per (layer, branch)
    assert torch.equal(_fwd(net, dev, x, 500, ctx, 3, pag=((1, 2, 3), 8)), e)
    ref = _oracle(sd, plan, x, 500, ctx, 3, (1, 2, 3), 8)
    assert all(rel_l2(e[r * 4:(r + 1) * 4], ref[r * 4:(r + 1) * 4]) < FWD_TOL for r in range(3))
    seen.clear()
    monkeypatch.setattr(vd, "BATCH_FORK", "0")
    assert rel_l2(_fwd(net, dev, x, 500, ctx, 3, pag=((1, 2, 3), 8)), e) < 1e-3 and seen == [(12, 8)] * 3


@pytest.mark.parametrize("C,side", [(320, 16), (640, 8), (1280, 8)])
def test_one_block_at_the_full_widths_vs_the_oracle_block(dev, C, side):
    """The tiny net has widths 64 and 128 only.  One SpatialTransformer at each full width -- 320: q | k | v arrive from the chained
    entry kernel and the tail is the one-launch chain; 640 / 1280: the block's own fused projection -- with seeded weights (proj_out
    not left at zero), B = 3, ident_from = 1, against the oracle block of tests/pag_cases.py on the same fp16-rounded weights.
    Compared on what the block adds to its input (out - x), sample by sample, with the project's forward bound."""
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
    x = torch.randn((3, C, side, side), generator=g).half().float()
    ctx = (torch.randn((3, 77, 768), generator=g) * 0.5).half().float()
    mask = torch.tensor([False, True, True])
    with torch.no_grad():
        ref = pc.spatial_transformer(sd, "b", x, ctx, heads, mask) - x
        off = pc.spatial_transformer(sd, "b", x, ctx, heads, torch.zeros(3, dtype=torch.bool)) - x
    gap = rel_l2(ref[1:], off[1:])
    assert gap >= 10 * FWD_TOL and rel_l2(ref[:1], off[:1]) < 1e-6       # precondition, on the oracle alone
    st = st.half().to(dev)
    xd = x.permute(0, 2, 3, 1).contiguous().half().to(dev)
    out = st(xd, ctx.half().to(dev), ident_from=1)
    delta = (out.float() - xd.float()).permute(0, 3, 1, 2).cpu()
    errs = [rel_l2(delta[b], ref[b]) for b in range(3)]
    plain = (st(xd, ctx.half().to(dev)).float() - xd.float()).permute(0, 3, 1, 2).cpu()
    print("width %d: block delta vs the oracle block per sample %s; plain block vs the oracle without PAG %.3e; oracle perturbed vs not %.3f"
          % (C, ["%.3e" % e for e in errs], rel_l2(plain, off), gap))
    assert all(e < FWD_TOL for e in errs)
    assert rel_l2(plain, off) < FWD_TOL and rel_l2(delta[1:], off[1:]) > 5 * FWD_TOL


# ---- 4. loops --------------------------------------------------------------------------------------------------------------------

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


def _sample(sampler, dev, xT, cs, steps=5, c_keys=None, call=None, **keys):
    x_info = dict({"type": "image", "xt": xT.half().to(dev)}, **keys)
    c = dict(_on_dev(cs[0], dev), **(c_keys or {}))
    return sampler.sample(steps=steps, shape=list(xT.shape), x_info=x_info, c_info=c, verbose=False, **(call or {}))


_OFF = {}


def _off_loop(sd, plan, sampler, base, kind, xT, cs, scale, noise=None, **kw):
    """The oracle loop without PAG, computed once per (kind, scale, extras) and shared."""
    key = (kind, scale, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _OFF:
        _OFF[key] = pc.oracle_loop(sd, plan, sampler, base, xT, cs, scale, 0.0, noise=noise, **kw)
    return _OFF[key]


@pytest.mark.parametrize("kind,scale", [("ddim", 7.5), ("2m", 7.5), ("unipc", 7.5), ("sde0", 7.5), ("sde1", 7.5), ("ddim", 1.0), ("2m", 1.0)])
def test_five_step_loops_vs_the_oracle_loop(tiny, plan, dev, gold, kind, scale):
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
    z, inter = _sample(sampler, dev, xT, cs, call=call, pag_scale=PAG_SCALE, **keys)
    assert len(sampler.ddim_timesteps) == 5 and inter["pag_layers"] == (pc.TINY_MID,)
    ref = pc.oracle_loop(sd, plan, sampler, base, xT, cs, scale, PAG_SCALE, "mid", noise=noise)
    off = _off_loop(sd, plan, sampler, base, kind, xT, cs, scale, noise=noise)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("%s s %.1f: final latent vs the oracle loop with PAG %.3e; oracle loop on vs off %.3e; latent vs the oracle loop off %.3e"
          % (kind, scale, err, gap, rel_l2(z, off)))
    assert gap > LATENT_TOL                  # precondition, on the oracle alone
    assert err < LATENT_TOL and err < rel_l2(z, off)


@pytest.mark.parametrize("scale,layers", [(7.5, (1, 2, 3)), (1.0, (0, 6))])
def test_other_layers_vs_the_oracle_loop(tiny, plan, dev, gold, scale, layers):
    net, sd = tiny
    xT, cs = _gold_case(gold, scale)
    sampler = _make("ddim", net)
    z, inter = _sample(sampler, dev, xT, cs, pag_scale=PAG_SCALE, pag_layers=list(reversed(layers)))
    assert inter["pag_layers"] == layers
    ref = pc.oracle_loop(sd, plan, sampler, "ddim", xT, cs, scale, PAG_SCALE, layers)
    off = _off_loop(sd, plan, sampler, "ddim", "ddim", xT, cs, scale)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("ddim s %.1f layers %r: final latent vs the oracle loop %.3e; oracle on vs off %.3e" % (scale, layers, err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, off)


@pytest.mark.parametrize("kind", ["ddim", "2m", "unipc", "sde"])
def test_graph_replay_eager_steps_and_a_fresh_sampler_agree_bitwise(tiny, dev, gold, monkeypatch, kind):
    net, _ = tiny
    xT, cs = _gold_case(gold)
    keys = {"seeds": [5, 6]} if kind == "sde" else {}
    shared = _make(kind, net)
    z_off0, i_off = _sample(shared, dev, xT, cs, **keys)                      # before any call with the key
    z_on, _ = _sample(shared, dev, xT, cs, pag_scale=PAG_SCALE, **keys)
    z_off, _ = _sample(shared, dev, xT, cs, **keys)                           # an off-call behind an on-call: its own earlier bits
    assert torch.equal(z_off, z_off0) and not torch.equal(z_on, z_off) and "pag_layers" not in i_off
    assert len(shared._static) == 2 and all(st["graph"] is not None for st in shared._static.values())
    on_state = [st for st in shared._static.values() if "pag_w" in st]
    assert len(on_state) == 1
    graph = on_state[0]["graph"]
    assert torch.equal(_sample(shared, dev, xT, cs, pag_scale=PAG_SCALE, **keys)[0], z_on)          # on the kept graph
    for off_keys in (dict(pag_scale=0), dict(pag_scale=None, pag_layers=[1]), dict(pag_scale=0.0, pag_layers="mid")):
        assert torch.equal(_sample(shared, dev, xT, cs, **dict(keys, **off_keys))[0], z_off)
    # a second scale replays the same kept graph with another weight
    z_two, _ = _sample(shared, dev, xT, cs, pag_scale=1.5, **keys)
    assert len(shared._static) == 2 and on_state[0]["graph"] is graph and [st for st in shared._static.values() if "pag_w" in st][0] is on_state[0]
    assert not torch.equal(z_two, z_on) and not torch.equal(z_two, z_off)
    assert torch.equal(_sample(_make(kind, net), dev, xT, cs, pag_scale=PAG_SCALE, **keys)[0], z_on)       # a fresh sampler
    assert torch.equal(_sample(_make(kind, net), dev, xT, cs, pag_scale=1.5, **keys)[0], z_two)
    # other layers: another key, another graph
    z_lay, _ = _sample(shared, dev, xT, cs, pag_scale=PAG_SCALE, pag_layers=(1, 2, 3), **keys)
    lay_state = [st for st in shared._static.values() if "pag_w" in st and st is not on_state[0]]
    assert not torch.equal(z_lay, z_on) and len(lay_state) == 1 and lay_state[0]["graph"] is not None and lay_state[0]["graph"] is not graph
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = _make(kind, net)
    assert not eager.use_graph
    assert torch.equal(_sample(eager, dev, xT, cs, pag_scale=PAG_SCALE, **keys)[0], z_on)
    assert torch.equal(_sample(eager, dev, xT, cs, pag_scale=PAG_SCALE, pag_layers=[3, 2, 1], **keys)[0], z_lay)
    assert torch.equal(_sample(eager, dev, xT, cs, **keys)[0], z_off)


def test_unguided_graph_serves_every_scale_and_off_keeps_its_bits(tiny, dev, gold):
    net, _ = tiny
    xT, cs = _gold_case(gold, 1.0)
    s = _make("2m", net)
    z_off = _sample(s, dev, xT, cs)[0]
    z_a = _sample(s, dev, xT, cs, pag_scale=PAG_SCALE)[0]
    z_b = _sample(s, dev, xT, cs, pag_scale=0.5)[0]
    assert len(s._static) == 2 and not torch.equal(z_a, z_b) and not torch.equal(z_a, z_off)
    assert torch.equal(_sample(s, dev, xT, cs)[0], z_off) and torch.equal(_sample(s, dev, xT, cs, pag_scale=PAG_SCALE)[0], z_a)


def test_eager_ddim_loop_and_single_steps_honour_the_keys(tiny, dev, gold):
    from lib.model_zoo.ddim import DDIMSampler
    net, _ = tiny
    xT, cs = _gold_case(gold)
    outs = []
    for keys in ({"pag_scale": PAG_SCALE}, {"pag_scale": PAG_SCALE, "pag_layers": "mid"}, {}, {"pag_scale": 0}):
        torch.manual_seed(3)
        z, inter = _sample(DDIMSampler(net), dev, xT, cs, call={"eta": 0.5}, **keys)
        assert ("pag_layers" in inter) == bool(keys.get("pag_scale"))
        outs.append(z)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3]) and rel_l2(outs[0], outs[2]) > 1e-3
    s = DDIMSampler(net)
    s.make_schedule(5, verbose=False)
    t = torch.full((2,), int(s.ddim_timesteps[4]), dtype=torch.long, device=dev)
    x = xT.half().to(dev)
    for scale in (7.5, 1.0):
        c = _on_dev(_gold_case(gold, scale)[1][0], dev)
        step = lambda **kw: (torch.manual_seed(1), s.p_sample_ddim(dict({"type": "image", "x": x}, **kw), c, t, 4)[0])[1]
        on, off, zero = step(pag_scale=PAG_SCALE), step(), step(pag_scale=0, pag_layers=[9])
        assert torch.equal(zero, off) and rel_l2(on, off) > 1e-4 and torch.equal(step(pag_scale=PAG_SCALE, pag_layers=[2]), on)
        assert not torch.equal(step(pag_scale=PAG_SCALE, pag_layers=[0]), on)


def test_multicontext_loop_vs_the_oracle_loop(tiny, plan, dev, gold):
    net, sd = tiny
    xT, cs = _gold_case(gold)
    cs = [dict(cs[0], ratio=0.4), _ci(torch.from_numpy(gold["c_img"]), torch.from_numpy(gold["u_img"]), 7.5, "image", ratio=0.6)]
    sampler = _make("2m", net)
    z, _ = sampler.sample_multicontext(steps=5, shape=SHAPE, x_info={"type": "image", "xt": xT.half().to(dev), "pag_scale": PAG_SCALE},
                                       c_info_list=[_on_dev(c, dev) for c in cs], verbose=False)
    ref = pc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, PAG_SCALE, "mid")
    off = pc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, 0.0)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("dual 2m: final latent vs the oracle loop with PAG %.3e; oracle on vs off %.3e" % (err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, off)


# ---- 5. combinations ---------------------------------------------------------------------------------------------------------------

def test_with_guidance_rescale_vs_the_oracle_loop(tiny, plan, dev, gold):
    """The rescale targets the standard deviation of the unperturbed e_c (diffusers' rescale_noise_cfg(noise_pred, noise_pred_text))."""
    net, sd = tiny
    xT, cs = _gold_case(gold)
    sampler = _make("ddim", net)
    z, inter = _sample(sampler, dev, xT, cs, c_keys={"guidance_rescale": 0.7}, pag_scale=PAG_SCALE)
    assert len(inter["guidance_rescale"]) >= 1
    ref = pc.oracle_loop(sd, plan, sampler, "ddim", xT, cs, 7.5, PAG_SCALE, "mid", phi=0.7)
    off = _off_loop(sd, plan, sampler, "ddim", "ddim", xT, cs, 7.5, phi=0.7)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("rescaled ddim: loop with PAG vs the oracle loop %.3e; oracle on vs off %.3e" % (err, gap))
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
    z, z_off = run(pag_scale=PAG_SCALE), run()
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(z[keep], x0[keep]) and bool(torch.isfinite(z).all())
    assert rel_l2(z[~keep], z_off[~keep]) > LATENT_TOL


def test_with_freeu_on_top_vs_the_oracle_with_both(tiny, plan, dev, gold):
    from freeu_cases import SETTING
    net, sd = tiny
    xT, cs = _gold_case(gold)
    sampler = _make("2m", net)
    z, _ = _sample(sampler, dev, xT, cs, pag_scale=PAG_SCALE, freeu=SETTING)
    ref = pc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, PAG_SCALE, "mid", setting=SETTING)
    only_freeu = _off_loop(sd, plan, sampler, "2m", "2m", xT, cs, 7.5, setting=SETTING)
    err, gap = rel_l2(z, ref), rel_l2(ref, only_freeu)
    print("2m with FreeU and PAG vs the oracle with both %.3e; oracle both vs FreeU alone %.3e" % (err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, only_freeu)


def test_with_windows_vs_per_window_oracle_forwards_merged(tiny, plan, dev):
    net, sd = tiny
    g = torch.Generator().manual_seed(61)
    shape = (1, 4, 16, 32)
    xT = torch.randn(shape, generator=g).half().float()
    cs = [_ci((torch.randn((1, 77, 128), generator=g) * 0.5).half().float(), (torch.randn((1, 77, 128), generator=g) * 0.5).half().float(), 7.5)]
    sampler = _make("2m", net)
    z, _ = _sample(sampler, dev, xT, cs, pag_scale=PAG_SCALE, window=16)
    geo = wc.geometry(16, 32, 16, 8)
    assert len(geo["offs"]) == 3
    ref = pc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, PAG_SCALE, "mid", geo=geo)
    off = wc.oracle_loop(sd, plan, sampler, "2m", xT, cs, 7.5, geo)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("windowed 2m: loop with PAG vs the windowed oracle loop %.3e; windowed oracle on vs off %.3e" % (err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, off)
    assert torch.equal(_sample(sampler, dev, xT, cs, pag_scale=PAG_SCALE, window=16)[0], z)          # on the kept graph


def test_sharded_world1_matches_direct_sample(tiny, dev, gold):
    from lib.model_zoo import sharded
    net, _ = tiny
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dev).half()
    ct = _ci(T(gold["c_text"]), T(gold["u_text"]), 7.5)
    imgs = sharded.vd_sample_sharded(net, _make("2m", net), 5, SHAPE, [dict(ct)], 3, guidance_scale=7.5, device_generator=True,
                                     pag_scale=PAG_SCALE, pag_layers=(1, 2))
    torch.manual_seed(103)
    z, _ = _make("2m", net).sample(steps=5, shape=SHAPE, x_info={"type": "image", "pag_scale": PAG_SCALE, "pag_layers": (1, 2)},
                                   c_info=dict(ct), verbose=False)
    assert torch.equal(imgs, net.vae_decode(z, which="image"))


def test_launch_counts_one_fold_per_step_and_one_identity_call_per_layer_and_type(tiny, dev, gold, monkeypatch):
    from vd_hip import ops
    net, _ = tiny
    xT, cs = _gold_case(gold)
    dual = [dict(cs[0], ratio=0.4), _ci(torch.from_numpy(gold["c_img"]), torch.from_numpy(gold["u_img"]), 7.5, "image", ratio=0.6)]
    folds, idents, real_fold, real_attn = [], [], ops.pag_fold, ops.attention

    def fold(eps, reps, w):
        folds.append((eps.shape[0], reps))
        return real_fold(eps, reps, w)

    def attn(q, k, v, heads, **kw):
        if kw.get("ident_from") is not None:
            idents.append((q.shape[0], kw["ident_from"]))
        return real_attn(q, k, v, heads, **kw)

    monkeypatch.setattr(ops, "pag_fold", fold)
    monkeypatch.setattr(ops, "attention", attn)
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")                       # eager steps: every launch of every step passes the wrappers
    s = _make("2m", net)
    _sample(s, dev, xT, cs)
    _sample(s, dev, xT, cs, pag_scale=0)
    assert folds == [] and idents == []
    _sample(s, dev, xT, cs, pag_scale=PAG_SCALE)
    assert folds == [(6, 3)] * 5 and idents == [(6, 4)] * 5        # one layer, one type, one branch
    folds.clear(), idents.clear()
    _sample(s, dev, xT, _gold_case(gold, 1.0)[1], pag_scale=PAG_SCALE, pag_layers=(0, 2, 6))
    assert folds == [(4, 2)] * 5 and idents == [(4, 2)] * 15
    folds.clear(), idents.clear()
    s.sample_multicontext(steps=5, shape=SHAPE, x_info={"type": "image", "xt": xT.half().to(dev), "pag_scale": PAG_SCALE, "pag_layers": (1, 2)},
                          c_info_list=[_on_dev(c, dev) for c in dual], verbose=False)
    assert folds == [(6, 3)] * 5 and idents == [(6, 4)] * (5 * 2 * 2)      # every context type's block at a layer's index
