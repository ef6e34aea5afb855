"""Guidance rescale on the host: the samplers' 'guidance_rescale' key (validation, the unguided call, the kept-graph key),
the float64 statement of the factor (ddim.cfg_rescale_factors), the C ABI listings and the sharded helper's argument."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["vd_cfg_rescale_factor_f16", "vd_cfg_ddim_step_rs_f16", "vd_cfg_ddim_step_dev_rs_f16",
                    "vd_cfg_dpmpp_step_dev_rs_f16", "vd_cfg_dpmpp_sde_step_dev_rs_f16"]


class Net(torch.nn.Module):
    num_timesteps = 1000
    device = torch.device("cpu")

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 4)
        self.register_buffer("alphas_cumprod", torch.linspace(0.999, 0.005, 1000))


def _ci(scale, **kw):
    c = torch.zeros((2, 7, 16))
    return dict({"type": "text", "conditioning": c, "unconditional_conditioning": c.clone(),
                 "unconditional_guidance_scale": scale}, **kw)


def _samplers():
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    return [DDIMSampler, DPMSolverSampler, DPMSolverSDESampler]


# ---- the key ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), "0.7", None, True])
def test_cfg_contexts_rejects_values_outside_the_unit_interval(bad):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(Net())
    with pytest.raises(ValueError):
        s._cfg_contexts([_ci(7.5, guidance_rescale=bad)])
    with pytest.raises(ValueError):
        s._cfg_contexts([_ci(7.5, guidance_rescale=0.5), _ci(7.5, guidance_rescale=bad)])


def test_cfg_contexts_returns_the_weight_and_ignores_it_unguided():
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(Net())
    copies, guided, scale, phi = s._cfg_contexts([_ci(7.5)])
    assert guided and scale == 7.5 and phi == 0. and copies[0]["c"].shape == (4, 7, 16)
    for value in (0, 0.7, 1, np.float32(0.25)):
        assert s._cfg_contexts([_ci(7.5, guidance_rescale=value)])[3] == float(value)
    assert s._cfg_contexts([_ci(7.5, guidance_rescale=0.3, ratio=0.4), _ci(7.5, guidance_rescale=0.3, ratio=0.6)])[3] == 0.3
    with pytest.raises(ValueError):       # contexts of one call that disagree (a missing key is 0)
        s._cfg_contexts([_ci(7.5, guidance_rescale=0.3), _ci(7.5, guidance_rescale=0.4)])
    with pytest.raises(ValueError):
        s._cfg_contexts([_ci(7.5, guidance_rescale=0.3), _ci(7.5)])
    copies, guided, _, phi = s._cfg_contexts([_ci(1.0, guidance_rescale=0.7)])      # unguided: ignored
    assert not guided and phi == 0. and copies[0]["c"].shape == (2, 7, 16)


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), "0.7"])
def test_sampler_entry_points_raise_before_drawing(bad):
    """sample*, ddim_sampling* and p_sample_ddim* of every sampler: ValueError, and the generator has not been used."""
    shape = [2, 4, 8, 8]
    for cls in _samplers():
        s = cls(Net())
        x_info = {"type": "image", "seeds": [1, 2]}
        state = torch.get_rng_state()
        with pytest.raises(ValueError, match="guidance_rescale"):
            s.sample(steps=4, shape=shape, x_info=dict(x_info), c_info=_ci(7.5, guidance_rescale=bad), verbose=False)
        with pytest.raises(ValueError, match="guidance_rescale"):
            s.sample_multicontext(steps=4, shape=shape, x_info=dict(x_info), verbose=False,
                                  c_info_list=[_ci(7.5, guidance_rescale=0.5), _ci(7.5, guidance_rescale=bad)])
        with pytest.raises(ValueError, match="guidance_rescale"):
            s.sample_multicontext(steps=4, shape=shape, x_info=dict(x_info), verbose=False,
                                  c_info_list=[_ci(7.5, guidance_rescale=0.5), _ci(7.5, guidance_rescale=0.6)])
        with pytest.raises(ValueError, match="guidance_rescale"):
            s.ddim_sampling(shape, dict(x_info), _ci(7.5, guidance_rescale=bad))
        assert torch.equal(torch.get_rng_state(), state)
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(Net())
    s.make_schedule(4, verbose=False)
    x_info = {"type": "image", "x": torch.zeros(shape)}
    with pytest.raises(ValueError, match="guidance_rescale"):
        s.p_sample_ddim(x_info, _ci(7.5, guidance_rescale=bad), torch.tensor([981, 981]), 3)
    with pytest.raises(ValueError, match="guidance_rescale"):
        s.p_sample_ddim_multicontext(x_info, [_ci(7.5), _ci(7.5, guidance_rescale=bad)], torch.tensor([981, 981]), 3)


def test_kept_graph_key_separates_rescaled_from_unrescaled_calls():
    """A graph captured without the rescale is never handed to a rescaled call and the other way round; every positive weight
    shares one state, whose "phi" buffer the call loads."""
    for cls in _samplers():
        s = cls(Net())
        x = torch.zeros(2, 4, 8, 8, dtype=torch.float16)
        ctx = [{"type": "text", "c": torch.zeros(4, 77, 768), "ratio": 1.0}]
        args = (x, {"type": "image"}, ctx, True, True, None)
        off = s._static_state(*args)
        assert "phi" not in off and "kfac" not in off
        on = s._static_state(*args, 0.3)
        assert on is not off and len(s._static) == 2
        assert on["phi"].shape == (1,) and on["phi"].dtype == torch.float32
        assert on["kfac"].shape == (2,) and on["kfac"].dtype == torch.float32
        assert s._static_state(*args, 0.9) is on and s._static_state(*args, rescale=1.0) is on
        assert s._static_state(*args, 0.) is off and s._static_state(*args) is off
        assert len(s._static) == 2
        for ci in ctx:
            ci["c"] = torch.zeros(4, 77, 768)
        s._seeds = None
        s._load_state(on, x, [dict(ci) for ci in ctx], None, 0.9)
        assert on["phi"].item() == np.float32(0.9)


# ---- the float64 statement ----------------------------------------------------------------------------------------------

def _eps(B, shape, seed, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((2 * B,) + tuple(shape), generator=g).to(dtype)


def test_factors_phi_zero_is_exactly_one():
    from lib.model_zoo.ddim import cfg_rescale_factors
    k = cfg_rescale_factors(_eps(3, (4, 9, 7), 1), 7.5, 0.)
    assert k.dtype == torch.float64 and k.shape == (3,) and bool((k == 1.0).all())


@pytest.mark.parametrize("shape", [(4, 16, 16), (768,), (4, 9, 7)])
def test_factors_phi_one_restores_the_conditional_std(shape):
    from lib.model_zoo.ddim import cfg_guided_eps, cfg_rescale_factors
    eps = _eps(3, shape, 2)
    k = cfg_rescale_factors(eps, 7.5, 1.)
    eg = cfg_guided_eps(eps, 7.5).flatten(1)
    ec = eps[3:].double().flatten(1)
    for ddof in (0, 1):        # the ratio does not depend on the estimator
        got, want = (k[:, None] * eg).std(1, correction=ddof), ec.std(1, correction=ddof)
        assert float(((got - want).abs() / want).max()) < 1e-12
    assert bool((k > 0).all()) and bool((k < 1).all())          # guidance at 7.5 inflates the std
    # the guided prediction is the fp32 value the kernels form
    assert torch.equal(eg, eg.float().double())
    assert float((eg - (eps[:3].double() + 7.5 * (eps[3:].double() - eps[:3].double())).flatten(1)).abs().max()) < 1e-5
    # in between: the blend
    half = cfg_rescale_factors(eps, 7.5, 0.5)
    assert float((half - (0.5 * k + 0.5)).abs().max()) < 1e-15


def test_factors_of_degenerate_predictions_are_one():
    from lib.model_zoo.ddim import cfg_rescale_factors
    zero = torch.zeros((4, 4, 8, 8), dtype=torch.float16)
    assert bool((cfg_rescale_factors(zero, 7.5, 0.7) == 1.0).all())
    const = torch.cat([torch.full((2, 300), 0.25), torch.full((2, 300), -1.5)]).half()
    assert bool((cfg_rescale_factors(const, 7.5, 0.7) == 1.0).all())
    one = _eps(5, (1,), 3)                                      # a single element has no variance
    assert bool((cfg_rescale_factors(one, 7.5, 1.0) == 1.0).all())
    flat_c = _eps(2, (64,), 4)                                  # a constant conditional prediction: r = 0
    flat_c[2:] = 0.5
    assert torch.equal(cfg_rescale_factors(flat_c, 7.5, 1.0), torch.zeros(2, dtype=torch.float64))
    assert float((cfg_rescale_factors(flat_c, 7.5, 0.25) - 0.75).abs().max()) == 0.


def test_a_factor_does_not_depend_on_the_batch_around_its_sample():
    from lib.model_zoo.ddim import cfg_rescale_factors
    eps = _eps(5, (4, 9, 7), 5)
    whole = cfg_rescale_factors(eps, 7.5, 0.7)
    for b in range(5):
        alone = cfg_rescale_factors(torch.stack([eps[b], eps[5 + b]]), 7.5, 0.7)
        assert torch.equal(alone, whole[b:b + 1])
    perm = [3, 0, 4, 1, 2]
    moved = cfg_rescale_factors(torch.cat([eps[:5][perm], eps[5:][perm]]), 7.5, 0.7)
    assert torch.equal(moved, whole[perm])


def test_the_weight_is_taken_in_fp32_as_the_device_buffer_holds_it():
    from lib.model_zoo.ddim import cfg_rescale_factors
    eps = _eps(2, (64,), 6)
    assert torch.equal(cfg_rescale_factors(eps, 7.5, 0.7), cfg_rescale_factors(eps, 7.5, float(np.float32(0.7))))


# ---- listings -----------------------------------------------------------------------------------------------------------

def test_header_loader_and_integration_name_every_new_entry_point():
    from vd_hip.loader import PROTOTYPES
    hdr = open(os.path.join(ROOT, "include", "vd_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in PROTOTYPES, name
        assert "`%s`" % name in doc, name
    # a rescaled update takes its sibling's arguments plus per_sample (where the sibling has none) and kfac
    import ctypes
    for name in NEW_ENTRY_POINTS[1:]:
        sib = PROTOTYPES[name.replace("_rs_f16", "_f16")][1]
        extra = 1 if ctypes.c_int64 in sib[6:7] else 2
        assert len(PROTOTYPES[name][1]) == len(sib) + extra, name
        assert PROTOTYPES[name][1][-2:] == [ctypes.c_void_p, ctypes.c_void_p]       # kfac, stream
    assert re.search(r"#define VD_HIP_ABI_VERSION 8\b", hdr)


# ---- the sharded helper -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("contexts", [1, 2])
def test_vd_sample_sharded_passes_the_key_on(contexts):
    from lib.model_zoo import sharded
    seen = []

    class Sampler:
        def sample(self, steps, shape, x_info, c_info, eta, verbose):
            seen.append([c_info])
            return x_info["xt"], {}

        def sample_multicontext(self, steps, shape, x_info, c_info_list, eta, verbose):
            seen.append(c_info_list)
            return x_info["xt"], {}

    class Model:
        device = torch.device("cpu")

        def vae_decode(self, z, which):
            return z

    ctx = [dict(_ci(1.0), ratio=1.0 / contexts) for _ in range(contexts)]
    sharded.vd_sample_sharded(Model(), Sampler(), 4, [2, 4, 8, 8], ctx, 3, guidance_scale=7.5, guidance_rescale=0.7)
    sharded.vd_sample_sharded(Model(), Sampler(), 4, [2, 4, 8, 8], ctx, 3, guidance_scale=7.5)
    assert [len(s) for s in seen] == [contexts, contexts]
    assert all(ci["guidance_rescale"] == 0.7 and ci["unconditional_guidance_scale"] == 7.5 for ci in seen[0])
    assert all(ci["guidance_rescale"] == 0. for ci in seen[1])
    assert all("guidance_rescale" not in ci for ci in ctx)          # the caller's dicts are left alone
