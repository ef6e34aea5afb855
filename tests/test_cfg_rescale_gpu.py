"""Guidance rescale on the GPU: the factor kernel (vd_cfg_rescale_factor_f16) against the float64 statement
ddim.cfg_rescale_factors, the rescaled fused updates (the _rs entry points) against their siblings (all factors 1: the same
bytes) and against an fp64 formula with per-sample factors, and the three samplers with c_info['guidance_rescale'] against
the fp32 CPU oracle loop with the rescale inserted; graph replay and kept graphs, inpainting, the sharded helper, the eager
DDIM loop (eta = 1) and the single step."""
import numpy as np
import pytest
import torch

from test_philox_cpu import normals_ref_batch
from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

LATENT_TOL = 1e-2            # the bound of test_dpm_solver_gpu.test_order2_tiny_vs_oracle (same value)
NOISE_ATOL = 2e-5            # of the generated normals (tests/test_philox_gpu.py)
RTOL, ATOL = 2 ** -10, 2e-4  # of test_dpm_solver_gpu.test_kernel_vs_fp64_formula
SCALE, PHI = 7.5, 0.7
# The sampler tests multiply the conditional contexts of the fixtures by CTX_AMP.  The synthetic tiny UNet barely responds to
# the fixtures' contexts as they are (e_c - e_u is 4 % of e_c on the fp32 oracle), so guidance at 7.5 inflates the std of the
# prediction by 2 %, the factors are 0.98 - 0.99 and a rescaled 10-step run differs from the unrescaled one by 1.3e-3 rel-L2:
# nothing to tell apart.  Trained models are used where guidance inflates the std well beyond that of e_c; a conditional
# context 8 times as large (exact in fp16) puts the tiny model there: factors 0.5 - 0.8 and 0.13 rel-L2 between the rescaled and
# the unrescaled loop on the fp32 oracle.  Not larger: the attention logits grow with it, and at 16 the fp16 forward itself is
# 1.1e-2 from the fp32 oracle over ten steps, with or without the rescale.
CTX_AMP = 8.0
SHAPE = [2, 4, 16, 16]
SEEDS = [11, 2 ** 35 + 5, 2 ** 63 - 1, 7, 2 ** 40 + 3, 99, 2 ** 62, 12345]
FACTOR_CASES = [(1, 1, 0), (3, 4099, 0), (3, 4099, 1), (2, 768, 0), (4, 16384, 0), (2, 36864, 0)]
# (B, per_sample, element offset) of the update tests.  The solver kernel takes its 16-byte loop only when every stream is
# 16-byte aligned, the conditional half eps + n included, so n % 8 == 0 at offset 0.  n = 3 * 4099 is odd: both 4099 cases of
# the issue run the scalar loop (one of them misaligned on top).  The three cases after them are aligned with
# per_sample % 8 != 0, so lanes of the 16-byte loop straddle two samples and look their factors up per element: 8 * 4099 (a
# boundary at every odd offset within a lane), 2 * 4100 (4 elements each side) and 2 * 252 (the [4, 9, 7] latent).
UPDATE_CASES = [(3, 4099, 0), (3, 4099, 1), (4, 16384, 0), (8, 4099, 0), (2, 4100, 0), (2, 252, 0)]
STRADDLING = [(8, 4099, 0), (2, 4100, 0), (2, 252, 0)]
KINDS = ["ddim_host", "ddim_host_noise", "ddim_dev", "ddim_dev_noise", "2m", "sde0", "sde"]


def T(a, dev, dtype=torch.float16):
    return torch.from_numpy(np.asarray(a)).to(dev).to(dtype)


def _view(dev, host, offset):
    """`host` on the device as a view `offset` elements into a larger allocation (offset = 1: misaligned)."""
    base = torch.empty((host.numel() + offset,), device=dev, dtype=host.dtype)
    out = base[offset:]
    out.copy_(host.reshape(-1))
    return out


def _ulps(a, b):
    """distance in fp32 units in the last place between two positive fp32 tensors"""
    return (a.float().cpu().view(torch.int32).long() - b.float().cpu().view(torch.int32).long()).abs()


# ---- 1. the factor kernel -----------------------------------------------------------------------------------------------

def _factors(dev, eps_h, per, phi, offset=0, scale=SCALE):
    from vd_hip import ops
    coef = torch.tensor([scale, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=dev)
    k = ops.cfg_rescale_factor(_view(dev, eps_h, offset), coef, torch.tensor([phi], dtype=torch.float32, device=dev), per)
    torch.cuda.synchronize()
    return k.cpu()


def _eps_case(B, per, seed):
    return torch.randn(2 * B * per, generator=torch.Generator().manual_seed(seed)).half()


@pytest.mark.parametrize("B,per,offset", FACTOR_CASES)
@pytest.mark.parametrize("phi", [0., 0.7, 1.])
def test_factor_kernel_vs_fp64_statement(dev, B, per, offset, phi):
    from lib.model_zoo.ddim import cfg_rescale_factors
    eps = _eps_case(B, per, 100 + per + offset)
    k = _factors(dev, eps, per, phi, offset)
    ref = cfg_rescale_factors(eps.view(2 * B, per), SCALE, phi)
    assert k.dtype == torch.float32 and k.shape == (B,)
    print("factors", k.tolist(), "reference", ref.tolist())
    if phi == 0. or per == 1:
        assert bool((k == 1.0).all())
    else:
        assert bool((k > 0).all()) and bool((k < 1).all())
    # fp64 accumulation of exact squares leaves a relative error near per * 2^-53, far below half an fp32 ulp: 1 ulp only
    # admits a rounding-boundary case
    assert int(_ulps(k, ref).max()) <= 1


@pytest.mark.parametrize("B,per,offset", FACTOR_CASES)
def test_a_factor_has_the_same_bits_wherever_its_sample_runs(dev, B, per, offset):
    eps = _eps_case(B, per, 200 + per + offset)
    eu, ec = eps[:B * per].view(B, per), eps[B * per:].view(B, per)
    whole = _factors(dev, eps, per, PHI, offset)
    assert torch.equal(whole, _factors(dev, eps, per, PHI, offset))                 # twice in a row
    fill = _eps_case(4, per, 300 + per)
    fu, fc = fill[:4 * per].view(4, per), fill[4 * per:].view(4, per)
    for b in range(B):
        alone = _factors(dev, torch.cat([eu[b], ec[b]]), per, PHI, offset)
        first = _factors(dev, torch.cat([eu[b:b + 1], fu, ec[b:b + 1], fc]).reshape(-1), per, PHI, offset)
        last = _factors(dev, torch.cat([fu, eu[b:b + 1], fc, ec[b:b + 1]]).reshape(-1), per, PHI, offset)
        other = _factors(dev, torch.cat([eu[b], ec[b]]), per, PHI, 1 - offset)      # the other alignment
        assert alone.shape == (1,) and first.shape == (5,)
        for got in (alone[0], first[0], last[4], other[0]):
            assert got.view(torch.int32).item() == whole[b].view(torch.int32).item(), b
        assert torch.equal(first[1:], last[:4])                                     # and so have the fillers


def test_factor_of_degenerate_predictions(dev):
    for B, per in ((2, 768), (3, 4099)):
        zero = torch.zeros(2 * B * per, dtype=torch.float16)
        for phi in (0.7, 1.0):
            assert bool((_factors(dev, zero, per, phi) == 1.0).all())
        assert bool((_factors(dev, _eps_case(B, per, 5), per, 0.) == 1.0).all())
    const = torch.cat([torch.full((2 * 768,), 0.25), torch.full((2 * 768,), -1.5)]).half()
    assert bool((_factors(dev, const, 768, 0.7) == 1.0).all())
    assert bool((_factors(dev, _eps_case(5, 1, 6), 1, 1.0) == 1.0).all())           # per_sample = 1


@pytest.mark.parametrize("per,offset", [(4099, 0), (4099, 1), (16384, 0)])
def test_factor_variance_is_formed_in_fp64(dev, per, offset):
    """e_c with mean 3 and std 0.01: in fp32 sums the one-pass variance loses every digit (sum v^2 = 9 m against V = 1e-4 m);
    fp64 sums keep the factor within 4 fp32 ulp of the reference."""
    from lib.model_zoo.ddim import cfg_rescale_factors
    B = 3
    g = torch.Generator().manual_seed(per + offset)
    eu = torch.randn(B * per, generator=g)
    ec = 3.0 + 0.01 * torch.randn(B * per, generator=g)
    eps = torch.cat([eu, ec]).half()
    assert abs(float(eps[B * per:].float().std()) - 0.01) < 2e-3
    for phi in (0.7, 1.0):
        k = _factors(dev, eps, per, phi, offset)
        ref = cfg_rescale_factors(eps.view(2 * B, per), SCALE, phi)
        print("factors", k.tolist(), "reference", ref.tolist())
        assert int(_ulps(k, ref).max()) <= 4


def test_factor_and_update_argument_checks(dev):
    from vd_hip import ops
    from vd_hip.loader import VdHipError, lib
    f16 = dict(device=dev, dtype=torch.float16)
    f32 = dict(device=dev, dtype=torch.float32)
    x, eps = torch.zeros((2, 16), **f16), torch.zeros((4, 16), **f16)
    coef, phi, kfac = torch.zeros(8, **f32), torch.zeros(1, **f32), torch.ones(2, **f32)
    hist = torch.zeros((2, 16), **f32)
    seeds = torch.zeros(2, dtype=torch.int64, device=dev)
    rng = torch.zeros(2, dtype=torch.int32, device=dev)
    assert ops.cfg_rescale_factor(eps, coef, phi, 16).shape == (2,)
    for bad in (lambda: ops.cfg_rescale_factor(eps, coef, phi, 0), lambda: ops.cfg_rescale_factor(eps, coef, phi, 5),
                lambda: ops.cfg_rescale_factor(eps.float(), coef, phi, 16),
                lambda: ops.cfg_rescale_factor(eps, coef, phi.half(), 16),
                lambda: ops.cfg_rescale_factor(eps, coef, phi, 16, out=torch.zeros(3, **f32)),
                lambda: ops.cfg_ddim_step_dev_rs(x, eps, coef, kfac, guided=False, x_prev=x),
                lambda: ops.cfg_ddim_step_dev_rs(x, eps, coef, kfac[:1], guided=True, x_prev=x),
                lambda: ops.cfg_ddim_step_rs(x, eps[:2], kfac, guided=False, guidance_scale=1., a_t=.5, a_prev=.6, sigma=0.,
                                             sqrt_one_minus_at=.7),
                lambda: ops.cfg_dpmpp_step_dev_rs(x, eps, coef, hist, kfac.half(), guided=True, x_next=x),
                lambda: ops.cfg_dpmpp_step_dev_rs(x, eps[:2], coef, hist, kfac, guided=False, x_next=x),
                lambda: ops.cfg_dpmpp_sde_step_dev_rs(x, eps, coef, hist, seeds, rng, kfac[:1], guided=True, x_next=x),
                lambda: ops.cfg_dpmpp_sde_step_dev_rs(x, eps[:2], coef, hist, seeds, rng, kfac, guided=False, x_next=x)):
        with pytest.raises(VdHipError):
            bad()
    # the C ABI itself: < 0 with a message, nothing launched
    h, p = lib(), lambda t: t.data_ptr()
    assert h.vd_cfg_rescale_factor_f16(None, 32, 16, p(coef), p(phi), p(kfac), None) < 0
    assert h.vd_cfg_rescale_factor_f16(p(eps), 0, 16, p(coef), p(phi), p(kfac), None) < 0
    assert h.vd_cfg_rescale_factor_f16(p(eps), 32, 0, p(coef), p(phi), p(kfac), None) < 0
    assert h.vd_cfg_rescale_factor_f16(p(eps), 32, 5, p(coef), p(phi), p(kfac), None) < 0
    assert b"per_sample" in h.vd_last_error()
    for guided, per, kf in ((0, 16, p(kfac)), (1, 5, p(kfac)), (1, 0, p(kfac)), (1, 16, None)):
        assert h.vd_cfg_ddim_step_dev_rs_f16(p(x), p(eps), None, p(x), None, 32, per, guided, p(coef), kf, None) < 0
        assert h.vd_cfg_ddim_step_rs_f16(p(x), p(eps), None, p(x), None, 32, per, guided, 7.5, .5, .6, 0., .7, kf, None) < 0
        assert h.vd_cfg_dpmpp_step_dev_rs_f16(p(x), p(eps), p(hist), p(x), None, 32, per, guided, p(coef), kf, None) < 0
        assert h.vd_cfg_dpmpp_sde_step_dev_rs_f16(p(x), p(eps), p(hist), p(x), None, 32, per, guided, p(coef), p(seeds),
                                                  p(rng), kf, None) < 0
    torch.cuda.synchronize()


# ---- 2. / 3. the rescaled updates ---------------------------------------------------------------------------------------

DDIM_STEP = dict(a_t=0.5, a_prev=0.62, sqrt_one_minus_at=float(np.sqrt(np.float32(1.) - np.float32(0.5))))
DDIM_SIGMA = 0.3


def _tables():
    from lib.model_zoo.diffusion_utils import make_ddim_timesteps
    from lib.model_zoo.dpm_solver import dpmpp_coef_table, dpmpp_sde_coef_table
    from oracle import vd_oracle as O
    ac = O.register_schedule()["alphas_cumprod"].numpy()
    ts = make_ddim_timesteps("uniform", 10, 1000, verbose=False)
    return {"2m": dpmpp_coef_table(ac, ts, scale=SCALE), "sde0": dpmpp_sde_coef_table(ac, ts, eta=0., scale=SCALE),
            "sde": dpmpp_sde_coef_table(ac, ts, eta=1., scale=SCALE)}


def _ddim_row(sigma):
    a_t, a_prev = DDIM_STEP["a_t"], DDIM_STEP["a_prev"]
    return np.array([SCALE, 1.0 / np.sqrt(np.float32(a_t)), np.sqrt(np.float32(a_prev)),
                     np.sqrt(np.float32(max(np.float32(1.) - np.float32(a_prev) - np.float32(sigma) * np.float32(sigma), 0.))),
                     sigma, DDIM_STEP["sqrt_one_minus_at"]], dtype=np.float32)


def _update_inputs(B, per, seed):
    g = torch.Generator().manual_seed(seed)
    n = B * per
    return torch.randn(n, generator=g).half(), torch.randn(2 * n, generator=g).half(), torch.randn(n, generator=g).half()


def _run_update(dev, kind, inputs, B, per, offset, alias, kfac_h):
    """Two consecutive steps of one fused update (solvers: a first-order row, NaN history unread, then a second-order row on
    it; DDIM: the same row twice) on views `offset` elements into larger allocations; kfac_h None runs the sibling entry point.
    Returns per step (x_next, pred_x0, hist or None, the history the step started from or None, the row) on the host."""
    from vd_hip import ops
    x_h, eps_h, noise_h = inputs
    n = B * per
    x = _view(dev, x_h, offset).view(B, per)
    eps = _view(dev, eps_h, offset)
    kfac = None if kfac_h is None else kfac_h.to(dev)
    new = lambda: _view(dev, torch.empty(n, dtype=torch.float16), offset).view(B, per)
    out = []
    if kind.startswith("ddim"):
        noise = _view(dev, noise_h, offset).view(B, per) if kind.endswith("noise") else None
        sigma = DDIM_SIGMA if noise is not None else 0.
        row = _ddim_row(sigma)
        for _ in range(2):
            if "host" in kind:
                kw = dict(guided=True, guidance_scale=SCALE, sigma=sigma, noise=noise, **DDIM_STEP)
                xn, p0 = ops.cfg_ddim_step(x, eps, **kw) if kfac is None else ops.cfg_ddim_step_rs(x, eps, kfac, **kw)
            else:
                xn, p0, coef = (x if alias else new()), new(), torch.from_numpy(row).to(dev)
                if kfac is None:
                    ops.cfg_ddim_step_dev(x, eps, coef, guided=True, x_prev=xn, pred_x0=p0, noise=noise)
                else:
                    ops.cfg_ddim_step_dev_rs(x, eps, coef, kfac, guided=True, x_prev=xn, pred_x0=p0, noise=noise)
            torch.cuda.synchronize()
            out.append((xn.cpu().clone().reshape(-1), p0.cpu().clone().reshape(-1), None, None, row))
            x = xn
        return out
    tab = _tables()[kind]
    rows = (tab[-1], tab[5])
    assert rows[0][6] == 0 and rows[1][6] != 0 and (rows[0][7] > 0) == (kind == "sde")
    hist = _view(dev, torch.full((n,), float("nan")), offset).view(B, per)          # the first step must not read it
    p0 = new()
    sd = torch.tensor(SEEDS[:B], dtype=torch.int64, device=dev)
    for draw, row in enumerate(rows):
        prev = hist.cpu().clone().reshape(-1)
        coef = torch.from_numpy(np.ascontiguousarray(row)).to(dev)
        xn = x if alias else new()
        rng = torch.tensor([draw, 2], dtype=torch.int32, device=dev)
        if kind == "2m":
            if kfac is None:
                ops.cfg_dpmpp_step_dev(x, eps, coef, hist, guided=True, x_next=xn, pred_x0=p0)
            else:
                ops.cfg_dpmpp_step_dev_rs(x, eps, coef, hist, kfac, guided=True, x_next=xn, pred_x0=p0)
        elif kfac is None:
            ops.cfg_dpmpp_sde_step_dev(x, eps, coef, hist, sd, rng, guided=True, x_next=xn, pred_x0=p0)
        else:
            ops.cfg_dpmpp_sde_step_dev_rs(x, eps, coef, hist, sd, rng, kfac, guided=True, x_next=xn, pred_x0=p0)
        torch.cuda.synchronize()
        out.append((xn.cpu().clone().reshape(-1), p0.cpu().clone().reshape(-1), hist.cpu().clone().reshape(-1), prev, row))
        x = xn
    return out


@pytest.mark.parametrize("B,per,offset", UPDATE_CASES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alias", [False, True])
def test_unit_factors_give_the_sibling_entry_points_bytes(dev, kind, B, per, offset, alias):
    inputs = _update_inputs(B, per, 400 + per + offset)
    sib = _run_update(dev, kind, inputs, B, per, offset, alias, None)
    rs = _run_update(dev, kind, inputs, B, per, offset, alias, torch.ones(B))
    for a, b in zip(sib, rs):
        assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
        assert torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))
        if a[2] is not None:
            assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


@pytest.mark.parametrize("B,per,offset", UPDATE_CASES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alias", [False, True])
def test_rescaled_updates_vs_fp64_formula(dev, kind, B, per, offset, alias):
    """Per element with that element's own sample factor.  In the STRADDLING cases the 2M kernel and the SDE kernel without
    noise (sde0; with noise and per_sample % 8 != 0 the SDE kernel walks its scalar loop) move lanes of 8 elements that lie in
    two samples; a lane that applied one factor to all 8, or its neighbour's (factors differ by up to 4x), would be off by far
    more than the tolerance.  The other cases run the scalar loop (4099 x 3) or lanes within one sample (16384)."""
    assert all(B * per % 8 == 0 and per % 8 != 0 and off == 0 for B, per, off in STRADDLING)
    inputs = _update_inputs(B, per, 500 + per + offset)
    kfac = (0.3 + 0.9 * torch.rand(B, generator=torch.Generator().manual_seed(per + offset))).float()
    steps = _run_update(dev, kind, inputs, B, per, offset, alias, kfac)
    n = B * per
    xd, ed, nd = inputs[0].double(), inputs[1].double(), inputs[2].double()
    kd = kfac.double().repeat_interleave(per)
    for draw, (x_next, p0, hist, prev, row) in enumerate(steps):
        r = [float(v) for v in row.astype(np.float64)]
        e = kd * (ed[:n] + r[0] * (ed[n:] - ed[:n]))
        atol = ATOL
        if kind.startswith("ddim"):
            x0 = (xd - r[5] * e) * r[1]
            xn = r[2] * x0 + r[3] * e + (r[4] * nd if kind.endswith("noise") else 0.0)
        else:
            x0 = (xd - r[2] * e) * r[1]
            d = r[5] * x0 + (r[6] * prev.double() if r[6] != 0 else 0.0)
            xn = r[3] * xd + r[4] * d
            if kind == "sde":
                xn = xn + r[7] * torch.from_numpy(normals_ref_batch(SEEDS[:B], per, draw, 2)).reshape(-1)
                atol = ATOL + r[7] * NOISE_ATOL
            assert bool(torch.isfinite(hist).all()) and rel_l2(hist, x0) < 1e-6
        assert bool(torch.isfinite(x_next).all())
        torch.testing.assert_close(x_next.double(), xn, rtol=RTOL, atol=atol)
        torch.testing.assert_close(p0.double(), x0, rtol=RTOL, atol=ATOL)
        xd = x_next.double()


@pytest.mark.parametrize("B,per,offset", UPDATE_CASES)
def test_rescaled_sde_update_keeps_its_noise(dev, B, per, offset):
    """x_next minus the noise-free x_next (the same rows with coef[7] = 0, the same factors) is coef[7] * z.  Each of the two
    fp16 outputs is within rtol |v| + atol of its exact value, so their difference is within the sum of the two bounds."""
    from vd_hip import ops
    inputs = _update_inputs(B, per, 600 + per + offset)
    kfac = (0.3 + 0.9 * torch.rand(B, generator=torch.Generator().manual_seed(per))).float().to(dev)
    n = B * per
    row = _tables()["sde"][5].copy()
    assert row[6] != 0 and row[7] > 0
    sd = torch.tensor(SEEDS[:B], dtype=torch.int64, device=dev)
    rng = torch.tensor([3, 2], dtype=torch.int32, device=dev)
    outs = []
    for c_z in (row[7], 0.):
        coef = torch.from_numpy(np.concatenate([row[:7], [c_z]]).astype(np.float32)).to(dev)
        x = _view(dev, inputs[0], offset).view(B, per)
        hist = _view(dev, inputs[2].float(), offset).view(B, per)
        xn = _view(dev, torch.empty(n, dtype=torch.float16), offset).view(B, per)
        ops.cfg_dpmpp_sde_step_dev_rs(x, _view(dev, inputs[1], offset), coef, hist, sd, rng, kfac, guided=True, x_next=xn)
        torch.cuda.synchronize()
        outs.append(xn.cpu().double().reshape(-1))
    z = torch.from_numpy(normals_ref_batch(SEEDS[:B], per, 3, 2)).reshape(-1)
    bound = RTOL * (outs[0].abs() + outs[1].abs()) + 2 * ATOL + float(row[7]) * NOISE_ATOL
    err = (outs[0] - outs[1] - float(row[7]) * z).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    assert rel_l2(outs[0] - outs[1], float(row[7]) * z) < 1e-2


# ---- 4. the samplers against the oracle ---------------------------------------------------------------------------------

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
def gold():
    return load_gold("ddim_tiny.npz")


def _ci(c, u, scale=SCALE, ctype="text", **kw):
    return dict({"type": ctype, "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale},
                **kw)


def _on_dev(c, dev):
    return dict(c, conditioning=c["conditioning"].half().to(dev),
                unconditional_conditioning=c["unconditional_conditioning"].half().to(dev))


def _sampler(name, net):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    return {"ddim": lambda: DDIMSampler(net), "dpm": lambda: DPMSolverSampler(net),
            "sde0": lambda: DPMSolverSDESampler(net, eta=0.), "sde1": lambda: DPMSolverSDESampler(net, eta=1.)}[name]()


def _contexts(gold, mix):
    ct = _ci(torch.from_numpy(gold["c_text"]) * CTX_AMP, torch.from_numpy(gold["u_text"]))
    ci = _ci(torch.from_numpy(gold["c_img"]) * CTX_AMP, torch.from_numpy(gold["u_img"]), ctype="image")
    return [dict(ct, ratio=0.4), dict(ci, ratio=0.6)] if mix else [ct]


def _oracle_loop(sd, family, sampler, xT, contexts, phi):
    """The existing tests' fp32 loops over the CPU oracle (DDIM with eta = 0: test_inpaint_gpu._oracle without the blend;
    DPM-Solver++(2M): test_dpm_solver_gpu._oracle_dpm) with the rescale of ddim.cfg_rescale_factors inserted after the
    guidance combine; also returns the factors of every step."""
    from lib.model_zoo.ddim import cfg_rescale_factors
    from lib.model_zoo.diffusion_utils import make_ddim_sampling_parameters
    from lib.model_zoo.dpm_solver import dpmpp_coef_table
    from oracle import vd_oracle as O
    plan = O.unet_plan(**meta()["unet2d"])
    ts = sampler.ddim_timesteps
    if family == "dpm":
        tab = torch.from_numpy(dpmpp_coef_table(sampler.alphas_cumprod, ts, order=2, lower_order_final=True, scale=SCALE))
    else:
        _, a_t, a_prev = make_ddim_sampling_parameters(sampler.alphas_cumprod, ts, 0.0, verbose=False)
    x, hist, factors = xT.float(), None, []
    cs = [(c["type"], torch.cat([c["unconditional_conditioning"], c["conditioning"]]).float(), c.get("ratio", 1.0))
          for c in contexts]
    for i in reversed(range(len(ts))):
        t = torch.full((2 * x.shape[0],), int(ts[i]), dtype=torch.long)
        with torch.no_grad():
            eps = O.apply_model_multicontext(sd, plan, torch.cat([x, x]), t, cs, "image", "image")
        e_u, e_c = eps.chunk(2)
        e = e_u + SCALE * (e_c - e_u)
        if phi > 0:
            k = cfg_rescale_factors(eps, SCALE, phi).float()
            factors.append(k)
            e = k.view(-1, 1, 1, 1) * e
        if family == "dpm":
            row = [float(v) for v in tab[i]]
            x0 = (x - row[2] * e) * row[1]
            d = row[5] * x0 + (row[6] * hist if row[6] != 0 else 0.0)
            x, hist = row[3] * x + row[4] * d, x0
        else:
            p0 = (x - np.sqrt(1 - a_t[i]) * e) / np.sqrt(a_t[i])
            x = (np.sqrt(a_prev[i]) * p0 + np.sqrt(1 - a_prev[i]) * e).float()
    return x, factors


_ORACLE = {}


def _oracle_cached(sd, family, sampler, xT, gold, mix):
    """computed once per (solver family, context mix) and shared: the 2M sampler and the SDE sampler at eta = 0 walk one table"""
    if (family, mix) not in _ORACLE:
        _ORACLE[(family, mix)] = _oracle_loop(sd, family, sampler, xT, _contexts(gold, mix), PHI)
    return _ORACLE[(family, mix)]


def _sample(sampler, dev, xT, contexts, phi=None, steps=10, **x_extra):
    cs = [_on_dev(c, dev) for c in contexts]
    if phi is not None:
        cs = [dict(c, guidance_rescale=phi) for c in cs]
    x_info = dict({"type": "image", "xt": xT.half().to(dev)}, **x_extra)
    if len(cs) == 1:
        return sampler.sample(steps=steps, shape=list(xT.shape), x_info=x_info, c_info=cs[0], verbose=False)
    return sampler.sample_multicontext(steps=steps, shape=list(xT.shape), x_info=x_info, c_info_list=cs, verbose=False)


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("name", ["ddim", "dpm", "sde0"])
def test_rescaled_samplers_tiny_vs_oracle(tiny, dev, gold, name, mix):
    net, sd = tiny
    xT = torch.from_numpy(gold["xT"]).float()
    sampler = _sampler(name, net)
    z, inter = _sample(sampler, dev, xT, _contexts(gold, mix), PHI)
    ref, factors = _oracle_cached(sd, "ddim" if name == "ddim" else "dpm", sampler, xT, gold, mix)
    err = rel_l2(z, ref)
    z_plain, inter_plain = _sample(_sampler(name, net), dev, xT, _contexts(gold, mix), 0.)
    diff = rel_l2(z, z_plain)
    print("%s mix=%s: rel-L2 vs the rescaled oracle loop %.3e, vs the phi = 0 run %.3e" % (name, mix, err, diff))
    assert err < LATENT_TOL
    assert diff > 10 * LATENT_TOL                   # the rescale really ran: this fails without the feature
    assert "guidance_rescale" not in inter_plain
    logged = inter["guidance_rescale"]
    assert len(logged) == len(inter["pred_x0"]) == 2            # 10 steps, log_every_t = 100: the first and the last step
    for k in logged:
        assert k.shape == (2,) and k.dtype == torch.float32
        assert bool((k > 0).all()) and bool((k <= 1).all())
    # the first step's factors see the same x_T as the oracle's: fp16 forward against fp32 forward
    assert float((logged[0].cpu() - factors[0]).abs().max()) < 1e-2


# ---- 5. graphs ----------------------------------------------------------------------------------------------------------

def _case(dev, seed, shape=tuple(SHAPE)):
    g = torch.Generator().manual_seed(seed)
    xT = torch.randn(shape, generator=g)
    c = torch.randn((shape[0], 77, 128), generator=g) * 0.5 * CTX_AMP
    u = torch.randn((shape[0], 77, 128), generator=g) * 0.5
    return xT, [_ci(c, u)]


def _extra(name):
    return {"seeds": [3, 4]} if name == "sde1" else {}


@pytest.mark.parametrize("name", ["ddim", "dpm", "sde1"])
def test_rescaled_graph_replay_matches_eager(tiny, dev, monkeypatch, name):
    net, _ = tiny
    xT, ctx = _case(dev, 5)
    z_graph, i_graph = _sample(_sampler(name, net), dev, xT, ctx, PHI, steps=8, **_extra(name))
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = _sampler(name, net)
    assert not eager.use_graph
    z_eager, i_eager = _sample(eager, dev, xT, ctx, PHI, steps=8, **_extra(name))
    assert rel_l2(z_graph, z_eager) < 2e-3
    assert rel_l2(i_graph["guidance_rescale"][-1], i_eager["guidance_rescale"][-1]) < 2e-3


@pytest.mark.parametrize("name", ["ddim", "dpm", "sde1"])
def test_one_kept_graph_serves_every_positive_weight(tiny, dev, name):
    net, _ = tiny
    shared = _sampler(name, net)
    xT, ctx = _case(dev, 6)
    z_a, _ = _sample(shared, dev, xT, ctx, 0.3, steps=6, **_extra(name))
    assert len(shared._static) == 1
    st = next(iter(shared._static.values()))
    graph = st["graph"]
    assert graph is not None and st["phi"].item() == np.float32(0.3) and st["kfac"].shape == (2,)
    z_b, _ = _sample(shared, dev, xT, ctx, 0.9, steps=6, **_extra(name))
    assert len(shared._static) == 1 and st["graph"] is graph and st["phi"].item() == np.float32(0.9)
    fresh_a, _ = _sample(_sampler(name, net), dev, xT, ctx, 0.3, steps=6, **_extra(name))
    fresh_b, _ = _sample(_sampler(name, net), dev, xT, ctx, 0.9, steps=6, **_extra(name))
    print("%s: phi 0.3 vs 0.9 rel-L2 %.3e" % (name, rel_l2(z_a, z_b)))
    assert torch.equal(z_a, fresh_a) and torch.equal(z_b, fresh_b)          # each weight its own result
    assert not torch.equal(z_a, z_b) and rel_l2(z_a, z_b) > 10 * 2e-3       # ten times the graph-vs-eager bound apart


@pytest.mark.parametrize("name", ["ddim", "dpm", "sde1"])
def test_unrescaled_calls_keep_their_bits_around_rescaled_ones(tiny, dev, name):
    net, _ = tiny
    xT, ctx = _case(dev, 7)
    z_nokey, i_nokey = _sample(_sampler(name, net), dev, xT, ctx, None, steps=6, **_extra(name))
    shared = _sampler(name, net)
    z_before, _ = _sample(shared, dev, xT, ctx, 0., steps=6, **_extra(name))
    z_rs, _ = _sample(shared, dev, xT, ctx, PHI, steps=6, **_extra(name))
    z_after, i_after = _sample(shared, dev, xT, ctx, 0., steps=6, **_extra(name))
    assert len(shared._static) == 2                                         # one state with the rescale, one without
    assert torch.equal(z_before, z_nokey) and torch.equal(z_after, z_nokey)
    assert "guidance_rescale" not in i_nokey and "guidance_rescale" not in i_after
    assert not torch.equal(z_rs, z_nokey)
    # an unguided call ignores the key
    one = [dict(c, unconditional_guidance_scale=1.0) for c in ctx]
    z_u0, _ = _sample(_sampler(name, net), dev, xT, one, None, steps=6, **_extra(name))
    z_u1, i_u1 = _sample(_sampler(name, net), dev, xT, one, PHI, steps=6, **_extra(name))
    assert torch.equal(z_u0, z_u1) and "guidance_rescale" not in i_u1


# ---- 6. other paths -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ddim", "dpm", "sde1"])
def test_inpainting_with_rescale_returns_the_known_region(tiny, dev, name):
    net, _ = tiny
    xT, ctx = _case(dev, 9)
    x0 = (torch.randn(SHAPE, generator=torch.Generator().manual_seed(4)) * 0.5).half().to(dev)
    mask = torch.ones((2, 1, 16, 16))
    mask[..., :6, :] = 0                         # keep the top rows
    mask = mask.half().to(dev)
    extra = dict(_extra(name), x0=x0, inpaint_mask=mask)
    z, inter = _sample(_sampler(name, net), dev, xT, ctx, PHI, steps=6, **extra)
    z_plain, _ = _sample(_sampler(name, net), dev, xT, ctx, 0., steps=6, **extra)
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(z[keep], x0[keep])
    assert rel_l2(z[~keep], x0[~keep]) > 0.1 and bool(torch.isfinite(z).all())
    assert rel_l2(z[~keep], z_plain[~keep]) > 2e-2 and len(inter["guidance_rescale"]) == 2


def test_sharded_world1_matches_the_direct_call_bitwise(tiny, dev, gold):
    from lib.model_zoo import sharded
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    net, _ = tiny
    ct = _ci(T(gold["c_text"] * CTX_AMP, dev), T(gold["u_text"], dev))
    seed, steps = 3, 6
    imgs = sharded.vd_sample_sharded(net, DPMSolverSampler(net), steps, SHAPE, [dict(ct)], seed, guidance_scale=SCALE,
                                     guidance_rescale=PHI)
    plain = sharded.vd_sample_sharded(net, DPMSolverSampler(net), steps, SHAPE, [dict(ct)], seed, guidance_scale=SCALE)
    xT = sharded.draw_initial_latent(SHAPE, seed).to(dev)
    z, _ = DPMSolverSampler(net).sample(steps=steps, shape=SHAPE, x_info={"type": "image", "xt": xT},
                                        c_info=dict(ct, guidance_rescale=PHI), verbose=False)
    assert torch.equal(imgs, net.vae_decode(z, which="image"))
    assert rel_l2(imgs, plain) > 2e-2


def test_eager_ddim_with_eta_rescales_and_draws_what_the_unrescaled_call_draws(tiny, dev):
    from lib.model_zoo.ddim import DDIMSampler
    net, _ = tiny
    xT, ctx = _case(dev, 12)
    cs = [_on_dev(c, dev) for c in ctx]
    runs = {}
    for phi in (0., PHI):
        torch.manual_seed(21)
        z, inter = DDIMSampler(net).sample(steps=6, shape=SHAPE, x_info={"type": "image", "xt": xT.half().to(dev)},
                                           c_info=dict(cs[0], guidance_rescale=phi), eta=1., verbose=False)
        runs[phi] = (z, inter, torch.cuda.get_rng_state(dev))
    z, inter, state = runs[PHI]
    assert bool(torch.isfinite(z).all()) and torch.equal(state, runs[0.][2])
    assert rel_l2(z, runs[0.][0]) > 2e-2 and "guidance_rescale" not in runs[0.][1]
    assert len(inter["guidance_rescale"]) == 2
    for k in inter["guidance_rescale"]:
        assert k.shape == (2,) and bool((k > 0).all()) and bool((k <= 1).all())


def test_single_step_rescales(tiny, dev):
    """p_sample_ddim with the key: x - sqrt(a_t) pred_x0 = sqrt(1 - a_t) e, so the rescaled step's is k_b times the plain
    step's, with the factor the sampler logs for its first step from the same latent."""
    from lib.model_zoo.ddim import DDIMSampler
    net, _ = tiny
    xT, ctx = _case(dev, 14)
    c = _on_dev(ctx[0], dev)
    s = DDIMSampler(net)
    _, inter = s.sample(steps=6, shape=SHAPE, x_info={"type": "image", "xt": xT.half().to(dev)},
                        c_info=dict(c, guidance_rescale=PHI), verbose=False)
    k = inter["guidance_rescale"][0].double().cpu()
    index = len(s.ddim_timesteps) - 1
    t = torch.full((2,), int(s.ddim_timesteps[index]), device=dev, dtype=torch.long)
    x = xT.half().to(dev)
    outs = {}
    for phi in (0., PHI):
        outs[phi] = s.p_sample_ddim({"type": "image", "x": x}, dict(c, guidance_rescale=phi), t, index)
    a_t = float(s.ddim_alphas[index])
    d = {phi: (x.double() - np.sqrt(a_t) * outs[phi][1].double()).cpu().flatten(1) for phi in outs}
    k_est = (d[PHI] * d[0.]).sum(1) / (d[0.] * d[0.]).sum(1)
    print("single step: factors", k.tolist(), "estimated from pred_x0", k_est.tolist())
    assert rel_l2(d[PHI], k_est[:, None] * d[0.]) < 1e-2
    assert float((k_est - k).abs().max()) < 1e-2
    assert not torch.equal(outs[PHI][0], outs[0.][0])
