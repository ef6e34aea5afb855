"""Adaptive projected guidance on the GPU: the fold (vd_apg_fold_f16 through ops.apg_fold) against the float64 statement formed from
the same fp32-rounded operands -- its per-sample figures, replica 0 and the running direction per element with bounds counted from
the contract's roundings, the bytes it must not touch, a sample's bits wherever it runs, the two-step recursion, the unread state,
degenerate samples, the argument checks -- and the four samplers' loops against the oracle loop of tests/apg_cases.py, graph replay
against eager steps, the kept graph across settings, off-calls, and the combinations with the guidance rescale, perturbed-attention
guidance, inpainting, windows, the eager DDIM loop and the sharded helper."""
import numpy as np
import pytest
import torch

import apg_cases as ac
import window_cases as wc
from apg_cases import CTX_AMP, LATENT_TOL, SCALE, SETTING, SHAPE, STEPS
from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu


def _view(dev, host, offset):
    """`host` on the device as a view `offset` elements into a larger allocation (offset = 1: misaligned)."""
    base = torch.empty((host.numel() + offset,), device=dev, dtype=host.dtype)
    out = base[offset:]
    out.copy_(host.reshape(-1))
    return out


def _fold(dev, x, eps, v_prev, row, offset=0, tail=None):
    """One launch on views `offset` elements into larger allocations.  eps is followed by `tail` (a third replica) when given.
    Returns (replica 0, everything behind it, v, fac) on the host."""
    from vd_hip import ops
    B, per = x.shape
    full = eps.reshape(-1) if tail is None else torch.cat([eps.reshape(-1), tail.reshape(-1)])
    xd, ed, vd = _view(dev, x, offset), _view(dev, full, offset), _view(dev, v_prev, offset)
    coef = torch.from_numpy(np.ascontiguousarray(row, dtype=np.float32)).to(dev)
    out, fac = ops.apg_fold(xd, ed, vd, coef, per)
    torch.cuda.synchronize()
    assert out.data_ptr() == ed.data_ptr() and fac.shape == (B, 4) and fac.dtype == torch.float32
    e = ed.cpu()
    return e[:B * per].view(B, per), e[B * per:], vd.cpu().view(B, per), fac.cpu()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _ulps(a, b):
    """distance in fp32 units in the last place between fp32 values of one sign (a: fp32 tensor, b: float64 array)"""
    bb = torch.from_numpy(np.asarray(b, dtype=np.float64).astype(np.float32))
    return (a.float().view(torch.int32).long() - bb.view(torch.int32).long()).abs()


def _check(x, eps, v_prev, row, got, tail):
    """Everything one launch wrote, against the float64 statement formed from the same fp32-rounded D and v."""
    B, per = x.shape
    out0, rest, v_k, fac_k = got
    D, v = ac.element_stage(x, eps, v_prev, row)
    fac, slack = ac.fac_ref(D, v, row)
    # the running direction: -g32 (e_c - e_u) + beta v_prev in float64 with two fp32 roundings (the product, the fma); the
    # difference of two fp16 values is exact in fp32 unless their exponents lie more than 13 apart (then one more)
    eu, ec = ac.f32(eps[:B]).astype(np.float64), ac.f32(eps[B:]).astype(np.float64)
    g32 = float(np.float32(row[0] * row[1]))
    dD = -g32 * (ec - eu)
    v64 = dD + float(row[3]) * v_prev.double().numpy() if row[3] != 0 else dD
    assert np.all(np.abs(v_k.double().numpy() - v64) <= 2.0 ** -24 * (2 * np.abs(dD) + np.abs(v64)) + 1e-45)
    assert np.array_equal(v_k.numpy(), v) or float(np.mean(v_k.numpy() != v)) < 1e-6     # the emulator's fma ties (double rounding) only
    # fac: norms and k within 1 fp32 ulp, p within half an ulp plus the cancellation term
    fk = fac_k.double().numpy()
    assert int(_ulps(fac_k[:, 0], fac[:, 0]).max()) <= 1 and int(_ulps(fac_k[:, 3], fac[:, 3]).max()) <= 1
    assert int(_ulps(fac_k[:, 1], fac[:, 1]).max()) <= 1
    assert np.all(np.abs(fk[:, 2] - fac[:, 2]) <= 0.5 * ac.ulp32(fac[:, 2]) + slack), (fk[:, 2], fac[:, 2], slack)
    # replica 0 per element from the kernel's own fac
    ref, bound = ac.fold_ref_and_bound(D, v_k.numpy(), ac.f32(eps[B:]), fac_k.numpy(), row)
    err = np.abs(out0.double().numpy() - ref)
    assert np.all(err <= bound), float((err / bound).max())
    # replica 1 and whatever follows keep their bytes
    keep = eps[B:].reshape(-1) if tail is None else torch.cat([eps[B:].reshape(-1), tail.reshape(-1)])
    assert torch.equal(_bits(rest), _bits(keep))
    return fac


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,per,offset", ac.KERNEL_CASES)
def test_fold_vs_fp64_statement(dev, B, per, offset):
    x, eps, v_prev = ac.kernel_inputs(B, per, 100 + per + offset)
    tail = torch.randn((B, per), generator=torch.Generator().manual_seed(per)).half()
    for beta in ac.BETAS:
        th = ac.thresholds(x, eps, v_prev, beta)
        for r in th:
            for eta in ac.ETAS:
                row = ac.coef_row(eta, r, beta)
                fac = _check(x, eps, v_prev, row, _fold(dev, x, eps, v_prev, row, offset, tail), tail)
                if r == th[1]:
                    assert np.all(fac[:, 1] < 1)
                else:
                    assert np.all(fac[:, 1] == 1)
                if per > 1:
                    assert np.all(np.abs(fac[:, 2]) > 0.1 * fac[:, 1]) and np.all(np.abs(fac[:, 2]) < 1.5)     # eta matters


@pytest.mark.parametrize("B,per,offset", ac.KERNEL_CASES)
def test_a_sample_has_the_same_bits_wherever_it_runs(dev, B, per, offset):
    x, eps, v_prev = ac.kernel_inputs(B, per, 200 + per + offset)
    row = ac.coef_row(0.5, ac.thresholds(x, eps, v_prev, -0.5)[1], -0.5)
    whole = _fold(dev, x, eps, v_prev, row, offset)
    again = _fold(dev, x, eps, v_prev, row, offset)
    same = lambda a, b: torch.equal(_bits(a), _bits(b))
    assert all(same(a, b) for a, b in zip(whole, again))                            # twice in a row
    fx, fe, fv = ac.kernel_inputs(4, per, 300 + per)
    for b in range(B):
        one = (x[b:b + 1], torch.cat([eps[b:b + 1], eps[B + b:B + b + 1]]), v_prev[b:b + 1])
        alone = _fold(dev, *one, row, offset)
        other = _fold(dev, *one, row, 1 - offset)                                   # the other alignment
        first = _fold(dev, torch.cat([one[0], fx]), torch.cat([eps[b:b + 1], fe[:4], eps[B + b:B + b + 1], fe[4:]]),
                      torch.cat([one[2], fv]), row, offset)
        last = _fold(dev, torch.cat([fx, one[0]]), torch.cat([fe[:4], eps[b:b + 1], fe[4:], eps[B + b:B + b + 1]]),
                     torch.cat([fv, one[2]]), row, offset)
        for got, i in ((alone, 0), (other, 0), (first, 0), (last, 4)):
            assert same(got[0][i], whole[0][b]) and same(got[2][i], whole[2][b]) and same(got[3][i], whole[3][b]), (b, i)
        assert same(first[0][1:], last[0][:4]) and same(first[3][1:], last[3][:4])    # and so have the fillers


@pytest.mark.parametrize("B,per,offset", [(3, 4099, 1), (2, 768, 0)])
def test_two_successive_calls_follow_the_recursion_and_the_first_does_not_read_the_state(dev, B, per, offset):
    from lib.model_zoo.ddim import apg_guided_eps
    x1, eps1, _ = ac.kernel_inputs(B, per, 400 + per)
    x2, eps2, _ = ac.kernel_inputs(B, per, 500 + per)
    nan = torch.full((B, per), float("nan"))
    r = ac.thresholds(x1, eps1, nan, 0.0)[1]
    row1, row2 = ac.coef_row(0.0, r, 0.0), ac.coef_row(0.0, r, -0.5)
    got1 = _fold(dev, x1, eps1, nan, row1, offset)
    assert all(bool(torch.isfinite(t).all()) for t in (got1[0], got1[2], got1[3]))           # beta_eff = 0: the NaN state is not read
    _check(x1, eps1, torch.zeros((B, per)), row1, got1, None)
    got2 = _fold(dev, x2, eps2, got1[2], row2, offset)
    _check(x2, eps2, got1[2], row2, got2, None)
    # and the float64 statement's own two-step recursion, to fp32 accuracy
    s1 = apg_guided_eps(x1, eps1, None, row1.astype(np.float64))
    s2 = apg_guided_eps(x2, eps2, s1[1], row2.astype(np.float64))
    assert np.allclose(got2[3].double().numpy(), s2[2].numpy(), rtol=1e-5, atol=1e-6)
    assert rel_l2(got2[2].double(), s2[1]) < 1e-6 and rel_l2(got2[0].double(), s2[0]) < 1e-3


def test_degenerate_samples(dev):
    for B, per in ((2, 768), (3, 4099)):
        g = torch.Generator().manual_seed(per)
        zero = torch.zeros((B, per), dtype=torch.float16)
        e_u = torch.randn((B, per), generator=g).half()
        for r in (0.0, 2.5):
            # all-zero x and e_c: D_c = 0
            out, _, v, fac = _fold(dev, zero, torch.cat([e_u, zero]), torch.zeros((B, per)), ac.coef_row(0.0, r, 0.0))
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(fac).all()) and bool(torch.isfinite(v).all())
            assert bool((fac[:, 2] == 0).all()) and bool((fac[:, 3] == 0).all())
            assert bool((fac[:, 1] == 1).all()) if r == 0.0 else bool((fac[:, 1] <= 1).all())
            # e_u == e_c: no direction
            x = torch.randn((B, per), generator=g).half()
            out, _, v, fac = _fold(dev, x, torch.cat([e_u, e_u]), torch.zeros((B, per)), ac.coef_row(0.0, r, 0.0))
            assert bool((fac[:, 0] == 0).all()) and bool((fac[:, 1] == 1).all()) and bool((fac[:, 2] == 0).all()) and bool((v == 0).all())
            assert torch.equal(_bits(out), _bits(e_u))


def test_argument_checks(dev):
    from vd_hip import ops
    from vd_hip.loader import VdHipError, lib
    f16 = dict(device=dev, dtype=torch.float16)
    f32 = dict(device=dev, dtype=torch.float32)
    x, eps, v = torch.zeros((2, 16), **f16), torch.zeros((4, 16), **f16), torch.zeros((2, 16), **f32)
    coef, fac = torch.from_numpy(ac.coef_row(0.5, 0.0, 0.0)).to(dev), torch.zeros((2, 4), **f32)
    assert ops.apg_fold(x, eps, v, coef, 16)[1].shape == (2, 4)
    assert ops.apg_fold(x, eps, v, coef, 16, out_fac=fac)[1] is fac
    for bad in (lambda: ops.apg_fold(x, eps, v, coef, 0), lambda: ops.apg_fold(x, eps, v, coef, 5), lambda: ops.apg_fold(x, eps[:3], v, coef, 16),
                lambda: ops.apg_fold(x.float(), eps, v, coef, 16), lambda: ops.apg_fold(x, eps, v.half(), coef, 16),
                lambda: ops.apg_fold(x, eps, v[:1], coef, 16), lambda: ops.apg_fold(x, eps, v, coef[:6], 16),
                lambda: ops.apg_fold(x, eps, v, coef.half(), 16), lambda: ops.apg_fold(x, eps, v, coef, 16, out_fac=fac[:1]),
                lambda: ops.apg_fold(x.cpu(), eps, v, coef, 16)):
        with pytest.raises(VdHipError):
            bad()
    h, p = lib(), lambda t: t.data_ptr()
    ok = dict(x=p(x), eps=p(eps), v=p(v), coef=p(coef), fac=p(fac), n=32, per=16)
    call = lambda **kw: (lambda a: h.vd_apg_fold_f16(a["x"], a["eps"], a["v"], a["coef"], a["fac"], a["n"], a["per"], None))(dict(ok, **kw))
    for kw in (dict(x=None), dict(eps=None), dict(v=None), dict(coef=None), dict(fac=None), dict(n=0), dict(per=0), dict(n=-32), dict(per=5),
               dict(v=p(v) + 2), dict(coef=p(coef) + 1), dict(fac=p(fac) + 2)):
        assert call(**kw) < 0 and h.vd_last_error().decode().startswith("vd_apg_fold_f16"), kw
    assert call() == 0
    torch.cuda.synchronize()


# ---- 2. the samplers against the oracle ------------------------------------------------------------------------------------------

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


APG = dict(apg_eta=SETTING[0], apg_norm_threshold=SETTING[1], apg_momentum=SETTING[2])
SEEDS = [41, 2 ** 33 + 9]


def _ci(c, u, scale=SCALE, ctype="text", **kw):
    return dict({"type": ctype, "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale}, **kw)


def _on_dev(c, dev):
    return dict(c, conditioning=c["conditioning"].half().to(dev), unconditional_conditioning=c["unconditional_conditioning"].half().to(dev))


def _make(kind, net, **kw):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    from lib.model_zoo.unipc import UniPCSampler
    return {"ddim": DDIMSampler, "2m": DPMSolverSampler, "unipc": UniPCSampler, "sde": DPMSolverSDESampler}[kind](net, **kw)


def _gold_case(gold, scale=SCALE):
    xT = torch.from_numpy(gold["xT"]).float()
    return xT, [_ci(torch.from_numpy(gold["c_text"]) * CTX_AMP, torch.from_numpy(gold["u_text"]), scale)]


def _sample(sampler, dev, xT, cs, steps=STEPS, c_keys=None, call=None, **keys):
    x_info = dict({"type": "image", "xt": xT.half().to(dev)}, **keys)
    c = dict(_on_dev(cs[0], dev), **(c_keys or {}))
    return sampler.sample(steps=steps, shape=list(xT.shape), x_info=x_info, c_info=c, verbose=False, **(call or {}))


def _keys(kind):
    return {"seeds": SEEDS} if kind == "sde" else {}


def _noise(kind):
    from test_philox_cpu import normals_ref_batch
    if kind != "sde":
        return None
    return lambda draw: torch.from_numpy(normals_ref_batch(SEEDS, int(np.prod(SHAPE[1:])), draw, 2))


def _first_step_fac(logged, first):
    """The first step sees the same x_T as the oracle's, fp16 forward against fp32 forward: the bound test_cfg_rescale_gpu uses for
    its first-step factors, 1e-2 -- absolute for k and p (like the rescale factors, of order 1 or below), relative for the norms."""
    got = logged.double().cpu()
    assert got.shape == (SHAPE[0], 4)
    print("first step fac", got.tolist(), "oracle", {k: v.tolist() for k, v in first.items()})
    assert float(((got[:, 0] - first["v_norm"]) / first["v_norm"]).abs().max()) < 1e-2
    assert float(((got[:, 3] - first["d_norm"]) / first["d_norm"]).abs().max()) < 1e-2
    assert float((got[:, 1] - first["k"]).abs().max()) < 1e-2 and float((got[:, 2] - first["p"]).abs().max()) < 1e-2


@pytest.mark.parametrize("kind", ["ddim", "2m", "sde", "unipc"])
def test_ten_step_loops_vs_the_oracle_loop(tiny, plan, dev, gold, kind):
    net, sd = tiny
    xT, cs = _gold_case(gold)
    sampler = _make(kind, net)
    z, inter = _sample(sampler, dev, xT, cs, **dict(_keys(kind), **APG))
    z_plain, inter_plain = _sample(_make(kind, net), dev, xT, cs, **_keys(kind))
    first = {}
    ref = ac.oracle_loop(sd, plan, sampler, kind, xT, cs, SCALE, SETTING, noise=_noise(kind), first=first)
    err, diff = rel_l2(z, ref), rel_l2(z, z_plain)
    print("%s: final latent vs the oracle loop with APG %.3e; vs the plain-guidance run %.3e" % (kind, err, diff))
    assert err < LATENT_TOL
    assert diff > 10 * LATENT_TOL                   # the fold really ran: this fails without the feature
    assert "apg" not in inter_plain and len(inter["apg"]) == len(inter["pred_x0"]) == 2     # log_every_t = 100: the first and the last step
    for fac in inter["apg"]:
        assert fac.shape == (2, 4) and fac.dtype == torch.float32 and bool(torch.isfinite(fac).all())
    assert bool((inter["apg"][0][:, 1] < 0.5).all()) and bool((inter["apg"][1][:, 1] == 1).all())   # r = 2.5 clips early, not late
    _first_step_fac(inter["apg"][0], first)


# ---- 3. graphs -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ddim", "2m", "sde", "unipc"])
def test_graph_replay_kept_graph_and_off_calls(tiny, dev, gold, monkeypatch, kind):
    from vd_hip import ops
    net, _ = tiny
    xT, cs = _gold_case(gold)
    keys = _keys(kind)
    neutral = dict(apg_eta=1.0, apg_norm_threshold=0.0, apg_momentum=0)
    other = dict(apg_eta=0.5, apg_norm_threshold=4.0, apg_momentum=0.25)
    shared = _make(kind, net)
    z_off0, i_off = _sample(shared, dev, xT, cs, steps=6, **keys)                       # before any call with the keys
    assert len(shared._static) == 1 and "apg" not in i_off
    z_on, _ = _sample(shared, dev, xT, cs, steps=6, **dict(keys, **APG))
    assert len(shared._static) == 2
    on_state = [st for st in shared._static.values() if "apg_v" in st]
    assert len(on_state) == 1 and on_state[0]["graph"] is not None
    graph = on_state[0]["graph"]
    # off-calls behind an on-call keep the bits they had before it, on the state they had: no new key, no fold
    for off_keys in ({}, neutral, dict(apg_eta=None), dict(apg_eta=1)):
        assert torch.equal(_sample(shared, dev, xT, cs, steps=6, **dict(keys, **off_keys))[0], z_off0)
    assert len(shared._static) == 2 and not torch.equal(z_on, z_off0)
    # another setting replays the same kept graph: no new capture, another result
    z_two, _ = _sample(shared, dev, xT, cs, steps=6, **dict(keys, **other))
    assert len(shared._static) == 2 and on_state[0]["graph"] is graph
    assert [st for st in shared._static.values() if "apg_v" in st][0] is on_state[0]
    assert not torch.equal(z_two, z_on) and not torch.equal(z_two, z_off0)
    assert torch.equal(_sample(shared, dev, xT, cs, steps=6, **dict(keys, **APG))[0], z_on)           # and back, on the kept graph
    assert torch.equal(_sample(_make(kind, net), dev, xT, cs, steps=6, **dict(keys, **other))[0], z_two)      # a fresh sampler
    # graph replay equals eager steps bit for bit; eager steps launch one fold per step, and none when off
    folds, real = [], ops.apg_fold

    def counted(x, eps, v, coef, per_sample, out_fac=None):
        folds.append((tuple(x.shape), eps.shape[0], per_sample))
        return real(x, eps, v, coef, per_sample, out_fac=out_fac)

    monkeypatch.setattr(ops, "apg_fold", counted)
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = _make(kind, net)
    assert not eager.use_graph
    assert torch.equal(_sample(eager, dev, xT, cs, steps=6, **dict(keys, **APG))[0], z_on)
    assert folds == [(tuple(SHAPE), 4, 1024)] * len(eager.ddim_timesteps)       # one launch per step (1000 // 6 strides: 7 steps)
    folds.clear()
    assert torch.equal(_sample(eager, dev, xT, cs, steps=6, **keys)[0], z_off0)
    assert torch.equal(_sample(eager, dev, xT, cs, steps=6, **dict(keys, **neutral))[0], z_off0)
    # an unguided call ignores the keys
    one = _gold_case(gold, 1.0)[1]
    z_u0, _ = _sample(eager, dev, xT, one, steps=6, **keys)
    z_u1, i_u1 = _sample(eager, dev, xT, one, steps=6, **dict(keys, **APG))
    assert torch.equal(z_u0, z_u1) and "apg" not in i_u1 and folds == []


# ---- 4. combinations -------------------------------------------------------------------------------------------------------------

def test_with_guidance_rescale_vs_the_oracle_loop(tiny, plan, dev, gold):
    """The rescale keeps targeting the standard deviation of e_c and sees the folded pair."""
    net, sd = tiny
    xT, cs = _gold_case(gold)
    sampler = _make("2m", net)
    z, inter = _sample(sampler, dev, xT, cs, c_keys={"guidance_rescale": 0.7}, **APG)
    assert len(inter["guidance_rescale"]) == 2 and len(inter["apg"]) == 2
    ref = ac.oracle_loop(sd, plan, sampler, "2m", xT, cs, SCALE, SETTING, phi=0.7)
    off = ac.oracle_loop(sd, plan, sampler, "2m", xT, cs, SCALE, None, phi=0.7)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("rescaled 2m: loop with APG vs the oracle loop %.3e; oracle on vs off %.3e" % (err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, off)


def test_with_pag_vs_the_oracle_loop(tiny, plan, dev, gold):
    """PAG's fold runs after APG's and adds to replica 0: the two compose additively."""
    net, sd = tiny
    xT, cs = _gold_case(gold)
    sampler = _make("ddim", net)
    z, inter = _sample(sampler, dev, xT, cs, pag_scale=3.0, **APG)
    assert "pag_layers" in inter and len(inter["apg"]) == 2
    ref = ac.oracle_loop(sd, plan, sampler, "ddim", xT, cs, SCALE, SETTING, pag_scale=3.0)
    off = ac.oracle_loop(sd, plan, sampler, "ddim", xT, cs, SCALE, None, pag_scale=3.0)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("ddim with PAG: loop with APG vs the oracle loop %.3e; oracle on vs off %.3e" % (err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, off)


def test_with_inpainting_vs_the_oracle_loop_and_the_known_region_returns(tiny, plan, dev, gold):
    from lib.model_zoo.ddim import inpaint_blend_table
    net, sd = tiny
    xT, cs = _gold_case(gold)
    x0 = (torch.randn(SHAPE, generator=torch.Generator().manual_seed(4)) * 0.5).half()
    mask = torch.ones((2, 1, 16, 16))
    mask[..., :6, :] = 0                         # keep the top rows
    sampler = _make("ddim", net)
    z, _ = _sample(sampler, dev, xT, cs, x0=x0.to(dev), inpaint_mask=mask.half().to(dev), **APG)
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(z.cpu()[keep], x0[keep]) and bool(torch.isfinite(z).all())
    tab = inpaint_blend_table(sampler.alphas_cumprod, sampler.ddim_timesteps).astype(np.float64)
    noise = xT.half().float()                    # a call that starts from xt blends with xt itself
    blend = lambda i, x: mask * x + (1 - mask) * (tab[i][0] * x0.float() + tab[i][1] * noise)
    ref = ac.oracle_loop(sd, plan, sampler, "ddim", xT, cs, SCALE, SETTING, blend=blend)
    off = ac.oracle_loop(sd, plan, sampler, "ddim", xT, cs, SCALE, None, blend=blend)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("inpainting ddim: loop with APG vs the oracle loop %.3e; oracle on vs off %.3e" % (err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, off)


def test_with_windows_vs_the_windowed_oracle_loop(tiny, plan, dev):
    """The fold sees the canvas prediction: one launch on the [1, 4, 16, 32] canvas, whatever the windows."""
    net, sd = tiny
    g = torch.Generator().manual_seed(61)
    shape = (1, 4, 16, 32)
    xT = torch.randn(shape, generator=g).half().float()
    cs = [_ci((torch.randn((1, 77, 128), generator=g) * 0.5 * CTX_AMP).half().float(), (torch.randn((1, 77, 128), generator=g) * 0.5).half().float())]
    sampler = _make("2m", net)
    z, inter = _sample(sampler, dev, xT, cs, window=16, **APG)
    assert inter["apg"][0].shape == (1, 4)
    geo = wc.geometry(16, 32, 16, 8)
    ref = ac.oracle_loop(sd, plan, sampler, "2m", xT, cs, SCALE, SETTING, geo=geo)
    off = ac.oracle_loop(sd, plan, sampler, "2m", xT, cs, SCALE, None, geo=geo)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("windowed 2m: loop with APG vs the windowed oracle loop %.3e; windowed oracle on vs off %.3e" % (err, gap))
    assert gap > LATENT_TOL and err < LATENT_TOL and err < rel_l2(z, off)


def test_eager_ddim_with_eta_applies_apg_and_draws_what_the_plain_call_draws(tiny, dev, gold):
    from lib.model_zoo.ddim import DDIMSampler
    net, _ = tiny
    xT, cs = _gold_case(gold)
    runs = {}
    for on in (False, True):
        torch.manual_seed(21)
        z, inter = _sample(DDIMSampler(net), dev, xT, cs, steps=6, call={"eta": 1.0}, **(APG if on else {}))
        runs[on] = (z, inter, torch.cuda.get_rng_state(dev))
    z, inter, state = runs[True]
    assert bool(torch.isfinite(z).all()) and torch.equal(state, runs[False][2])
    assert rel_l2(z, runs[False][0]) > 2e-2 and "apg" not in runs[False][1]
    assert len(inter["apg"]) == 2 and all(f.shape == (2, 4) and bool(torch.isfinite(f).all()) for f in inter["apg"])
    assert bool((inter["apg"][0][:, 1] < 0.5).all())
    # its first step sees what the static loop's first step sees: the same latent, the same fold
    first = _sample(DDIMSampler(net), dev, xT, cs, steps=6, **APG)[1]["apg"][0]
    assert rel_l2(inter["apg"][0], first) < 1e-2


def test_sharded_world1_matches_the_direct_call_bitwise(tiny, dev, gold):
    from lib.model_zoo import sharded
    net, _ = tiny
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dev).half()
    ct = _ci(T(gold["c_text"] * CTX_AMP), T(gold["u_text"]))
    seed, steps = 3, 6
    imgs = sharded.vd_sample_sharded(net, _make("2m", net), steps, SHAPE, [dict(ct)], seed, guidance_scale=SCALE, **APG)
    plain = sharded.vd_sample_sharded(net, _make("2m", net), steps, SHAPE, [dict(ct)], seed, guidance_scale=SCALE)
    xT = sharded.draw_initial_latent(SHAPE, seed).to(dev)
    z, _ = _make("2m", net).sample(steps=steps, shape=SHAPE, x_info=dict({"type": "image", "xt": xT}, **APG), c_info=dict(ct), verbose=False)
    assert torch.equal(imgs, net.vae_decode(z, which="image"))
    assert rel_l2(imgs, plain) > 2e-2


def test_sag_with_apg_raises(tiny, dev, gold):
    net, _ = tiny
    xT, cs = _gold_case(gold)
    for kind in ("ddim", "2m", "sde", "unipc"):
        s = _make(kind, net)
        with pytest.raises(ValueError, match="apg.*sag_scale.*out of scope"):
            _sample(s, dev, xT, cs, sag_scale=1.0, **dict(_keys(kind), **APG))
        assert len(s._static) == 0                  # nothing was set up
