"""Inpainting (blended latent diffusion) on the host: the blend table against its formula, the pixel -> latent mask
helper against a numpy restatement, the C ABI's argument checks without a device and the samplers' validation of the
inpainting keys.  No GPU needed."""
import numpy as np
import pytest
import torch


def _ac():
    from oracle import vd_oracle as O
    return O.register_schedule()["alphas_cumprod"].numpy()


def _timesteps(steps):
    from lib.model_zoo.diffusion_utils import make_ddim_timesteps
    return make_ddim_timesteps("uniform", steps, 1000, verbose=False)


@pytest.mark.parametrize("steps,k", [(5, None), (10, None), (50, None), (10, 3), (50, 17)])
def test_blend_table_matches_formula(steps, k):
    from lib.model_zoo.ddim import inpaint_blend_table
    ac, ts = _ac(), _timesteps(steps)
    if k is not None:
        ts = ts[:k]                      # the x0 + x0_forward_timesteps schedule
    tab = inpaint_blend_table(ac, ts)
    assert tab.dtype == np.float32 and tab.shape == (len(ts), 2)
    a_prev = [float(np.float32(ac[0]))] + [float(np.float32(ac[t])) for t in ts[:-1]]
    for i in range(len(ts)):
        want = (1.0, 0.0) if i == 0 else (np.sqrt(a_prev[i]), np.sqrt(1.0 - a_prev[i]))
        np.testing.assert_allclose(tab[i].astype(np.float64), want, rtol=1e-7, atol=0)
    assert tab[0, 0] == 1.0 and tab[0, 1] == 0.0


def _pool_np(m, f, mode):
    b, _, H, W = m.shape
    blocks = m.reshape(b, 1, H // f, f, W // f, f).astype(np.float64)
    return blocks.max(axis=(3, 5)) if mode == "max" else blocks.mean(axis=(3, 5))


@pytest.mark.parametrize("mode", ["max", "area"])
@pytest.mark.parametrize("batch", [1, 3])
def test_latent_mask_matches_numpy(mode, batch):
    from lib.app_ops import latent_mask
    g = torch.Generator().manual_seed(5 + batch)
    hard = torch.rand((batch, 1, 64, 48), generator=g) > 0.9
    soft = torch.rand((batch, 1, 64, 48), generator=g)
    for m in (hard, soft):
        out = latent_mask(m, mode=mode)
        assert out.shape == (batch, 1, 8, 6) and out.dtype == torch.float32
        np.testing.assert_allclose(out.numpy(), _pool_np(m.float().numpy(), 8, mode), rtol=1e-6, atol=1e-7)
    out = latent_mask(soft, mode=mode, factor=2)
    assert out.shape == (batch, 1, 32, 24)
    np.testing.assert_allclose(out.numpy(), _pool_np(soft.numpy(), 2, mode), rtol=1e-6, atol=1e-7)
    # a single masked pixel: "max" regenerates its whole latent pixel, "area" gives it 1/64
    one = torch.zeros((1, 1, 16, 16))
    one[0, 0, 9, 3] = 1
    lm = latent_mask(one, mode=mode)
    assert lm[0, 0, 1, 0] == (1.0 if mode == "max" else 1.0 / 64) and float(lm.sum()) == float(lm[0, 0, 1, 0])


def test_latent_mask_rejects_bad_shapes():
    from lib.app_ops import latent_mask
    for shape in [(1, 1, 60, 64), (1, 1, 64, 20), (1, 2, 64, 64), (1, 64, 64)]:
        with pytest.raises(ValueError):
            latent_mask(torch.ones(shape))
    with pytest.raises(ValueError):
        latent_mask(torch.ones((1, 1, 64, 64)), mode="min")


def test_masked_blend_rejects_bad_arguments_without_a_device():
    import ctypes
    from vd_hip.loader import lib
    h = lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(x=p, x0=p, noise=p, mask=p, out=p, B=2, C=4, HW=8, Bm=2, coef=p)

    def call(**kw):
        a = dict(ok, **kw)
        return h.vd_masked_blend_f16(a["x"], a["x0"], a["noise"], a["mask"], a["out"], a["B"], a["C"], a["HW"], a["Bm"],
                                     a["coef"], None)
    for k in ("x", "x0", "noise", "mask", "out", "coef"):
        assert call(**{k: None}) < 0 and b"vd_masked_blend_f16" in h.vd_last_error(), k
    for k in ("B", "C", "HW"):
        assert call(**{k: 0}) < 0, k
        assert call(**{k: -1}) < 0, k
    for bm in (0, 3, -1):
        assert call(Bm=bm) < 0 and b"mask batch" in h.vd_last_error(), bm


class _Stub:
    num_timesteps = 1000
    alphas_cumprod = torch.from_numpy(_ac())


@pytest.mark.parametrize("sampler_name", ["ddim", "dpm"])
def test_sampler_rejects_bad_inpainting_arguments(sampler_name):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    s = (DDIMSampler if sampler_name == "ddim" else DPMSolverSampler)(_Stub())
    shape = [2, 4, 8, 8]
    x0, m = torch.zeros(shape), torch.ones((2, 1, 8, 8))
    bad = [
        dict(type="text", x0=torch.zeros((2, 128)), inpaint_mask=torch.ones((2, 1, 1, 1))),    # a text latent
        dict(type="image", inpaint_mask=m),                                                     # no x0
        dict(type="image", x0=x0, inpaint_mask=torch.ones((2, 1, 8, 4))),                       # wrong mask shape
        dict(type="image", x0=x0, inpaint_mask=torch.ones((2, 8, 8))),                          # mask without channel
        dict(type="image", x0=x0, inpaint_mask=torch.ones((2, 4, 8, 8))),                       # per-channel mask
        dict(type="image", x0=x0, inpaint_mask=torch.ones((3, 1, 8, 8))),                       # wrong mask batch
        dict(type="image", x0=torch.zeros((2, 4, 8, 4)), inpaint_mask=m),                       # x0 is not the latent
    ]
    for x_info in bad:
        with pytest.raises(ValueError):
            s.sample(steps=5, shape=shape, x_info=dict(x_info), c_info={}, verbose=False)
        with pytest.raises(ValueError):
            s.sample_multicontext(steps=5, shape=shape, x_info=dict(x_info), c_info_list=[{}], verbose=False)


def test_single_step_api_rejects_a_mask():
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(_Stub())
    x_info = {"type": "image", "x": torch.zeros((1, 4, 8, 8)), "x0": torch.zeros((1, 4, 8, 8)),
              "inpaint_mask": torch.ones((1, 1, 8, 8))}
    t = torch.tensor([981])
    with pytest.raises(ValueError):
        s.p_sample_ddim(x_info, {}, t, 0)
    with pytest.raises(ValueError):
        s.p_sample_ddim_multicontext(x_info, [{}], t, 0)


def test_sharded_mask_needs_images():
    from lib.model_zoo import sharded
    with pytest.raises(ValueError):
        sharded.vd_sample_sharded(None, None, 5, [1, 4, 8, 8], [], 0, mask=torch.ones((1, 1, 64, 64)))
