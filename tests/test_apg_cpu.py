"""Adaptive projected guidance on the host: ddim.apg_guided_eps against an independent transcription of the paper's Algorithm 1 in the
space of data predictions, the coefficient table, the validation of x_info['apg_eta'] / ['apg_norm_threshold'] / ['apg_momentum']
(nothing is drawn and no device is touched before a raise), the step graph's key, the sharding helper's forwarding, the C ABI listing
with the entry's refusals, the reference arithmetic of tests/apg_cases.py, and the oracle preconditions: that the project's bound
tells APG on from off in every sampler's loop.  No GPU."""
import numpy as np
import pytest
import torch

import apg_cases as ac
from apg_cases import LATENT_TOL
from test_pag_cpu import _NoDevice, _samplers
from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg


@pytest.fixture(scope="module")
def tiny_cpu():
    """The tiny product model on the CPU (never run) and its fp32 weights."""
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    return net, synth_into(net, m["seed"])


@pytest.fixture(scope="module")
def plan():
    from oracle import vd_oracle as O
    return O.unet_plan(**meta()["unet2d"])


@pytest.fixture(scope="module")
def gold():
    return load_gold("ddim_tiny.npz")


C_INFO = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_conditioning": torch.zeros(1, 7, 128),
          "unconditional_guidance_scale": 7.5}
BAD_ETAS = [-0.1, 1.0001, float("nan"), float("inf"), "0.5", True, False, (0.5,), [0.5], 1j]
BAD_THRESHOLDS = [-1.0, -1e-9, float("nan"), float("inf"), "2.5", True, (2.5,), 1j]
BAD_MOMENTA = [1.0, -1.0, 1.5, -7, float("nan"), float("inf"), float("-inf"), "-0.5", True, False, [0.5], 1j]


# ---- 1. the float64 statement ----------------------------------------------------------------------------------------------------

def _row64(a_t, eta, r, beta):
    s1, isa = np.sqrt(1.0 - a_t), 1.0 / np.sqrt(a_t)
    return np.array([s1, isa, 1.0 / (s1 * isa), beta, r, 1.0 - eta, 0.0, 0.0])


@pytest.mark.parametrize("eta,r,beta", [(0.0, 2.5, -0.5), (0.5, 0.0, 0.0), (1.0, 40.0, 0.7), (0.3, 1e9, -0.9), (0.0, 0.0, 0.0), (1.0, 3.0, 0.0)])
def test_statement_against_algorithm_1_in_x0_space(eta, r, beta):
    """Three steps with the running average carried along.  Both sides are float64 formulas of the same quantity: 1e-12 relative."""
    from lib.model_zoo.ddim import apg_guided_eps
    g = torch.Generator().manual_seed(17)
    s, shape = 7.5, (3, 4, 9, 7)
    v = avg = None
    clipped = []
    for step, a_t in enumerate((0.05, 0.4, 0.93)):
        x = torch.randn(shape, generator=g, dtype=torch.float64)
        e_c = torch.randn(shape, generator=g, dtype=torch.float64)
        e_u = e_c - 0.3 * (x - np.sqrt(1 - a_t) * e_c) / np.sqrt(a_t) + 0.4 * torch.randn(shape, generator=g, dtype=torch.float64)
        row = _row64(a_t, eta, r, 0.0 if step == 0 else beta)
        eu2, v, fac = apg_guided_eps(x, torch.cat([e_u, e_c]), v, row)
        mine = eu2 + s * (e_c - eu2)                                   # what the unchanged update forms
        ref, avg = ac.guided_eps(x, e_u, e_c, avg, a_t, s, (eta, r, beta))
        assert float((mine - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
        assert float((v - avg).abs().max()) <= 1e-12 * float(avg.abs().max())
        assert fac.shape == (3, 4) and fac.dtype == torch.float64
        assert float((fac[:, 0] - v.flatten(1).norm(dim=1)).abs().max()) <= 1e-12 * float(fac[:, 0].max())
        clipped.append(bool((fac[:, 1] < 1).all()))
        assert bool((fac[:, 2].abs() > 0.02 * fac[:, 1]).all())        # the inputs are correlated: there is a parallel part
    if r in (2.5, 3.0):
        assert clipped[0]                                              # g = 4.4 at a_t = 0.05: the direction is long there
    if r in (0.0, 1e9):
        assert not any(clipped)


def test_neutral_triple_gives_e_u_back_and_eta_removes_the_parallel_part():
    from lib.model_zoo.ddim import apg_guided_eps
    g = torch.Generator().manual_seed(2)
    x, e_u, e_c = [torch.randn((2, 4, 8, 8), generator=g, dtype=torch.float64) for _ in range(3)]
    eu2, v, fac = apg_guided_eps(x, torch.cat([e_u, e_c]), None, _row64(0.3, 1.0, 0.0, 0.0))
    assert float((eu2 - e_u).abs().max()) <= 1e-12 * float(e_u.abs().max()) and bool((fac[:, 1] == 1).all())
    # v_prev is not read when beta_eff == 0
    nan = torch.full_like(x, float("nan"))
    assert torch.equal(apg_guided_eps(x, torch.cat([e_u, e_c]), nan, _row64(0.3, 1.0, 0.0, 0.0))[0], eu2)
    # eta = 0: the guided data prediction minus D_c is orthogonal to D_c
    row = _row64(0.3, 0.0, 0.0, 0.0)
    eu0 = apg_guided_eps(x, torch.cat([e_u, e_c]), None, row)[0]
    d_c = (x - row[0] * e_c) * row[1]
    n = (eu0 - e_c) * (row[0] * row[1])
    assert float((n * d_c).flatten(1).sum(1).abs().max()) <= 1e-12 * float((n.flatten(1).norm(dim=1) * d_c.flatten(1).norm(dim=1)).max())
    # degenerate samples: no NaN, p = 0, k = 1
    zero = torch.zeros_like(x)
    out, v, fac = apg_guided_eps(zero, torch.cat([e_u, zero]), None, _row64(0.3, 0.0, 0.0, 0.0))
    assert bool((fac[:, 2] == 0).all()) and bool((fac[:, 3] == 0).all()) and bool((fac[:, 1] == 1).all())
    out, v, fac = apg_guided_eps(x, torch.cat([e_c, e_c]), None, _row64(0.3, 0.0, 2.5, 0.0))
    assert bool((fac[:, 0] == 0).all()) and bool((fac[:, 1] == 1).all()) and bool((fac[:, 2] == 0).all()) and torch.equal(out, e_c)


def test_coefficient_table_rows_and_the_first_step_of_a_call():
    from lib.model_zoo.ddim import apg_coef_table
    from lib.model_zoo.diffusion_utils import make_ddim_timesteps
    from oracle import vd_oracle as O
    alphas = O.register_schedule()["alphas_cumprod"].numpy()
    ts = make_ddim_timesteps("uniform", 10, 1000, verbose=False)
    tab = apg_coef_table(alphas, ts, 0.25, 2.5, -0.5)
    assert tab.shape == (10, 8) and tab.dtype == np.float32
    a = alphas.astype(np.float64)[ts]
    assert np.array_equal(tab[:, 0], np.sqrt(1 - a).astype(np.float32)) and np.array_equal(tab[:, 1], (1 / np.sqrt(a)).astype(np.float32))
    assert np.array_equal(tab[:, 2], (1.0 / (np.sqrt(1 - a) / np.sqrt(a))).astype(np.float32))
    assert np.all(tab[:, 4] == np.float32(2.5)) and np.all(tab[:, 5] == np.float32(0.75)) and np.all(tab[:, 6:] == 0)
    # the loops walk the indices downwards: the first step a call runs reads the last row, and only that one starts the direction
    assert tab[-1, 3] == 0 and np.all(tab[:-1, 3] == np.float32(-0.5))
    # a call that starts from x0 diffused to step k of the schedule runs timesteps[:k] (DDIMSampler._start_latent)
    for k in (7, 1):
        part = apg_coef_table(alphas, ts[:k], 0.25, 2.5, -0.5)
        assert part.shape == (k, 8) and part[-1, 3] == 0 and np.all(part[:-1, 3] == np.float32(-0.5))
        assert np.array_equal(part[:, :3], tab[:k, :3])
    assert apg_coef_table(alphas, ts[:0], 0.25, 2.5, -0.5).shape == (0, 8)


def test_start_latent_truncates_the_schedule_the_table_is_built_from(tiny_cpu, monkeypatch):
    from lib.model_zoo.ddim import DDIMSampler, apg_coef_table
    net = tiny_cpu[0]
    monkeypatch.setattr(net, "q_sample", lambda x0, ts, noise=None: x0)       # the forward process itself is a device op
    s = DDIMSampler(net)
    s.make_schedule(10, verbose=False)
    x0 = torch.zeros(1, 4, 16, 16)
    _, timesteps, _ = s._start_latent([1, 4, 16, 16], {"x0": x0, "x0_forward_timesteps": 6, "x0_noise": x0}, False, "cpu", torch.float32)
    assert len(timesteps) == 6
    tab = apg_coef_table(s.alphas_cumprod, timesteps, *ac.SETTING)
    assert tab.shape == (6, 8) and tab[5, 3] == 0 and np.all(tab[:5, 3] == np.float32(-0.5))


# ---- 2. the keys -----------------------------------------------------------------------------------------------------------------

def test_keys_are_validated_and_normalised():
    from lib.model_zoo.vd import _apg_arg
    arg = lambda **kw: _apg_arg(dict({"type": "image"}, **kw))
    assert arg() is None and arg(apg_eta=None, apg_norm_threshold=None, apg_momentum=None) is None
    for neutral in (dict(apg_eta=1), dict(apg_eta=1.0, apg_norm_threshold=0, apg_momentum=0.0), dict(apg_norm_threshold=0.0),
                    dict(apg_momentum=-0.0), dict(apg_eta=np.float32(1.0), apg_momentum=np.int64(0))):
        assert arg(**neutral) is None
        assert arg(sag_scale=1.0, **neutral) is None                     # off: the combination is not looked at
    assert arg(apg_eta=0) == (0.0, 0.0, 0.0) and arg(apg_norm_threshold=2.5) == (1.0, 2.5, 0.0) and arg(apg_momentum=-0.5) == (1.0, 0.0, -0.5)
    assert arg(apg_eta=np.float32(0.5), apg_norm_threshold=np.int32(3), apg_momentum=0.25) == (0.5, 3.0, 0.25)
    assert arg(apg_eta=0.0, apg_norm_threshold=2.5, apg_momentum=-0.5, pag_scale=3.0, window=16, cache_interval=2) == ac.SETTING
    for bad in BAD_ETAS:
        with pytest.raises(ValueError, match="apg"):
            arg(apg_eta=bad)
    for bad in BAD_THRESHOLDS:
        with pytest.raises(ValueError, match="apg"):
            arg(apg_norm_threshold=bad)
    for bad in BAD_MOMENTA:
        with pytest.raises(ValueError, match="apg"):
            arg(apg_momentum=bad)
    with pytest.raises(ValueError, match="apg.*sag_scale.*out of scope on purpose"):
        arg(apg_eta=0.0, sag_scale=1.0)
    assert arg(apg_eta=0.0, sag_scale=0) == (0.0, 0.0, 0.0) and arg(apg_eta=0.0, sag_scale=None) == (0.0, 0.0, 0.0)


def test_samplers_raise_before_anything_is_drawn(tiny_cpu):
    model = _NoDevice(tiny_cpu[0])
    state = torch.get_rng_state()
    for s in _samplers(model):
        run = lambda scale=7.5, **keys: s.sample(steps=5, shape=[1, 4, 16, 16], x_info=dict({"type": "image"}, **keys),
                                                 c_info=dict(C_INFO, unconditional_guidance_scale=scale), verbose=False)
        multi = lambda **keys: s.sample_multicontext(steps=5, shape=[1, 4, 16, 16], x_info=dict({"type": "image"}, **keys),
                                                     c_info_list=[dict(C_INFO)], verbose=False)
        for key, values in (("apg_eta", BAD_ETAS), ("apg_norm_threshold", BAD_THRESHOLDS), ("apg_momentum", BAD_MOMENTA)):
            for bad in values:
                with pytest.raises(ValueError, match="apg"):
                    run(**{key: bad})
                with pytest.raises(ValueError, match="apg"):
                    multi(**{key: bad})
                with pytest.raises(ValueError, match="apg"):
                    run(scale=1.0, **{key: bad})                         # a bad value raises in an unguided call too
        with pytest.raises(ValueError, match="apg.*sag_scale"):
            run(apg_eta=0.0, sag_scale=1.0)
        with pytest.raises(ValueError, match="apg.*sag_scale"):
            multi(apg_norm_threshold=2.5, apg_momentum=-0.5, sag_scale=0.5)
        for good in (dict(), dict(apg_eta=1.0, apg_norm_threshold=0.0, apg_momentum=0.0), dict(apg_eta=0.0),
                     dict(apg_eta=0.0, apg_norm_threshold=2.5, apg_momentum=-0.5), dict(apg_momentum=0.9, window=8),
                     dict(apg_eta=0.5, pag_scale=3.0)):
            with pytest.raises(AssertionError, match="touched the device"):
                run(**good)
            with pytest.raises(AssertionError, match="touched the device"):
                run(scale=1.0, **good)
    assert torch.equal(torch.get_rng_state(), state)        # nothing was drawn from the (host) generator on the way


def test_p_sample_ddim_validates_the_keys_and_refuses_a_guided_step(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(_NoDevice(tiny_cpu[0]))
    c_info = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_guidance_scale": 1.0}
    for keys in (dict(apg_eta=-1), dict(apg_momentum=1.0), dict(apg_norm_threshold="2")):
        x_info = dict({"type": "image", "x": torch.zeros(1, 4, 16, 16)}, **keys)
        with pytest.raises(ValueError, match="apg"):
            s.p_sample_ddim(x_info, c_info, torch.tensor([1]), 0)
    net = tiny_cpu[0]
    net.device = "cpu"
    guided = dict(c_info, unconditional_conditioning=torch.zeros(1, 7, 128), unconditional_guidance_scale=7.5)
    with pytest.raises(ValueError, match="apg.*whole sample"):
        DDIMSampler(net).p_sample_ddim({"type": "image", "x": torch.zeros(1, 4, 16, 16), "apg_eta": 0.0}, guided, torch.tensor([1]), 0)


def test_graph_key_has_one_bit_for_on_and_off_and_none_for_the_setting(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(tiny_cpu[0])
    x = torch.zeros(1, 4, 16, 16)
    cis = [{"type": "text", "c": torch.zeros(2, 7, 128)}]
    key = lambda guided=True, **kw: s._static_key(x, dict({"type": "image"}, **kw), cis, guided, True)
    off = key()
    for neutral in (dict(apg_eta=1.0), dict(apg_eta=1, apg_norm_threshold=0, apg_momentum=0), dict(apg_eta=None, apg_momentum=None)):
        assert key(**neutral) == off                                  # absent or neutral: the key it always had
    on = key(apg_eta=0.0, apg_norm_threshold=2.5, apg_momentum=-0.5)
    assert on == off + (("apg",),)
    assert key(apg_eta=0.5) == on and key(apg_norm_threshold=9.0) == on and key(apg_momentum=0.3) == on     # one graph, every setting
    assert key(False) == key(False, apg_eta=0.0, apg_norm_threshold=2.5, apg_momentum=-0.5)                # unguided: off
    both = key(apg_eta=0.0, pag_scale=3.0, hypertile=8)
    assert both[-1] == ("apg",) and both[:-1] == key(pag_scale=3.0, hypertile=8)


def test_sharding_helper_forwards_the_keys():
    from lib.model_zoo import sharded
    seen = []

    class Net(object):
        device = "cpu"

        def vae_decode(self, z, which):
            return z

    class Sampler(object):
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=False):
            seen.append(tuple(x_info.get(k, "absent") for k in ("apg_eta", "apg_norm_threshold", "apg_momentum")))
            return x_info["xt"], {}

    ctx = lambda: {"type": "text", "conditioning": torch.zeros(2, 7, 16), "unconditional_conditioning": torch.zeros(2, 7, 16)}
    sharded.vd_sample_sharded(Net(), Sampler(), 6, [2, 4, 8, 8], [ctx()], seed=3)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, [2, 4, 8, 8], [ctx()], seed=3, apg_eta=0.0)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, [2, 4, 8, 8], [ctx()], seed=3, apg_eta=0.5, apg_norm_threshold=2.5, apg_momentum=-0.5)
    assert seen == [("absent",) * 3, (0.0, "absent", "absent"), (0.5, 2.5, -0.5)]


def test_entry_is_declared_and_refuses_bad_arguments_without_a_device():
    import ctypes
    import os
    import re
    from vd_hip import ops
    from vd_hip.loader import PROTOTYPES, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "vd_hip.h")).read()
    assert re.search(r"\bint vd_apg_fold_f16\(", hdr) and len(PROTOTYPES["vd_apg_fold_f16"][1]) == 8
    assert '"apg.hip"' in open(os.path.join(root, "versatile-diffusion_amd", "build.py")).read()
    assert callable(ops.apg_fold)
    L = lib()
    assert L.vd_abi_version() == 8                  # the entry is additive
    P = ctypes.c_void_p
    ok = dict(x=P(4096), eps=P(8192), v=P(16384), coef=P(32768), fac=P(65536), n=24, per=12)
    fold = lambda **kw: (lambda a: L.vd_apg_fold_f16(a["x"], a["eps"], a["v"], a["coef"], a["fac"], a["n"], a["per"], None))(dict(ok, **kw))
    for kw in (dict(x=None), dict(eps=None), dict(v=None), dict(coef=None), dict(fac=None), dict(n=0), dict(n=-24), dict(per=0), dict(per=-1),
               dict(per=5), dict(per=48), dict(v=P(16386)), dict(coef=P(32769)), dict(fac=P(65538)), dict(x=P(4097)), dict(eps=P(8193))):
        assert fold(**kw) < 0 and L.vd_last_error().decode().startswith("vd_apg_fold_f16"), kw


# ---- 3. the reference arithmetic of the kernel tests -------------------------------------------------------------------------------

def test_reference_stage_and_bounds_hold_for_fp32_arithmetic_done_in_numpy():
    """The contract's operations carried out in numpy fp32 (fma through float64) sit within the per-element bound of the float64
    reference; the inputs give |p| between 0.1 and 1; the thresholds clip every sample / none."""
    from lib.model_zoo.ddim import apg_guided_eps
    for (B, per, _), beta in zip(ac.KERNEL_CASES[1:5], (0.0, -0.5, -0.5, 0.0)):
        x, eps, v_prev = ac.kernel_inputs(B, per, 7 + per)
        th = ac.thresholds(x, eps, v_prev, beta)
        for eta, r in ((0.0, th[1]), (0.5, th[2]), (1.0, 0.0)):
            row = ac.coef_row(eta, r, beta)
            D, v = ac.element_stage(x, eps, v_prev, row)
            fac, slack = ac.fac_ref(D, v, row)
            assert np.all(np.abs(fac[:, 2]) > 0.1 * fac[:, 1]) and np.all(np.abs(fac[:, 2]) < 1.5)
            assert np.all(fac[:, 1] < 1) if r == th[1] else np.all(fac[:, 1] == 1)
            assert np.all(slack < 2.0 ** -30)
            # the float64 statement agrees with the fp32-staged reference to fp32 accuracy
            st = apg_guided_eps(x, eps, v_prev, row.astype(np.float64))
            assert np.allclose(st[2].numpy(), fac, rtol=1e-5, atol=1e-6)
            fac32 = fac.astype(np.float32)
            q = np.float32(np.float64(row[5]) * np.float64(fac32[:, 2]))[:, None]
            kv = (fac32[:, 1:2] * v).astype(np.float32)
            nn = ac.fma32(-q * np.ones_like(D), D, kv)
            ec = ac.f32(eps[B:])
            out = ac.fma32(nn, np.full_like(nn, row[2]), ec).astype(np.float16).astype(np.float64)
            ref, bound = ac.fold_ref_and_bound(D, v, ec, fac32, row)
            assert np.all(np.abs(out - ref) <= bound)
            assert np.all(bound <= 2.0 ** -9 * (np.abs(ref) + 1.0))          # and the bound is an fp16 rounding, not a tolerance


# ---- 4. the oracle's preconditions: the project's bound tells APG on from off ---------------------------------------------------------

def _contexts(gold, scale=ac.SCALE):
    return [{"type": "text", "conditioning": torch.from_numpy(gold["c_text"]) * ac.CTX_AMP,
             "unconditional_conditioning": torch.from_numpy(gold["u_text"]), "unconditional_guidance_scale": scale}]


def _cpu_sampler(kind, net):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    from lib.model_zoo.unipc import UniPCSampler
    s = {"ddim": DDIMSampler, "2m": DPMSolverSampler, "unipc": UniPCSampler, "sde": DPMSolverSDESampler}[kind](net)
    s.make_schedule(ac.STEPS, ddim_eta=1.0 if kind == "sde" else 0.0, verbose=False)
    return s


@pytest.mark.parametrize("kind", ["ddim", "2m", "sde", "unipc"])
def test_loop_precondition_ten_steps_on_vs_plain_guidance(tiny_cpu, plan, gold, kind):
    """Setting (eta 0, r 2.5, beta -0.5) at s = 7.5 with the conditional context x 8, ten steps, on the fp32 oracle: the final latent
    is at least 10 x LATENT_TOL from plain guidance in every sampler; the identity setting is plain guidance up to fp32 rounding."""
    from test_philox_cpu import normals_ref_batch
    net, sd = tiny_cpu
    xT = torch.from_numpy(gold["xT"]).float()
    s = _cpu_sampler(kind, net)
    seeds = [41, 2 ** 33 + 9]
    noise = (lambda draw: torch.from_numpy(normals_ref_batch(seeds, int(np.prod(ac.SHAPE[1:])), draw, 2))) if kind == "sde" else None
    first = {}
    on = ac.oracle_loop(sd, plan, s, kind, xT, _contexts(gold), ac.SCALE, ac.SETTING, noise=noise, first=first)
    off = ac.oracle_loop(sd, plan, s, kind, xT, _contexts(gold), ac.SCALE, None, noise=noise)
    assert rel_l2(off, ac.pc.oracle_loop(sd, plan, s, kind, xT, _contexts(gold), ac.SCALE, noise=noise)) < 1e-6      # off is the plain oracle loop
    gap = rel_l2(on, off)
    print("%s: ten steps with APG %r vs plain guidance %.3e rel-L2; first step ||v|| %s k %s p %s" %
          (kind, ac.SETTING, gap, first["v_norm"].tolist(), first["k"].tolist(), first["p"].tolist()))
    assert gap >= 10 * LATENT_TOL and bool(torch.isfinite(on).all())
    assert bool((first["k"] < 0.5).all())                           # r = 2.5 clips the first step
    if kind == "ddim":
        ident = ac.oracle_loop(sd, plan, s, kind, xT, _contexts(gold), ac.SCALE, (1.0, 0.0, 0.0))
        print("ddim: the identity setting vs plain guidance %.3e" % rel_l2(ident, off))
        assert rel_l2(ident, off) < 1e-4
