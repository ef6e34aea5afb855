"""The SDE variant of DPM-Solver++(2M) on the host: its coefficient table (dpm_solver.dpmpp_sde_coef_table) against the 2M
table (eta = 0, bitwise) and against float64 closed forms (eta = 1), the per-sample seeds of sharded batches, and the
argument validation of DPMSolverSDESampler, which runs before any device work.  No GPU, no library needed."""
import numpy as np
import pytest
import torch


def _ac():
    from oracle import vd_oracle as O
    return O.register_schedule()["alphas_cumprod"].numpy()


def _timesteps(method, steps):
    from lib.model_zoo.diffusion_utils import make_ddim_timesteps
    return make_ddim_timesteps(method, steps, 1000, verbose=False)


CASES = [("uniform", 1), ("uniform", 5), ("uniform", 14), ("uniform", 15), ("uniform", 50), ("quad", 20)]


@pytest.mark.parametrize("method,steps", CASES)
@pytest.mark.parametrize("order", [1, 2])
def test_eta0_is_the_2m_table_bitwise(method, steps, order):
    from lib.model_zoo.dpm_solver import dpmpp_coef_table, dpmpp_sde_coef_table
    ac, ts = _ac(), _timesteps(method, steps)
    for lof in (True, False):
        sde = dpmpp_sde_coef_table(ac, ts, eta=0.0, s_noise=1.3, order=order, lower_order_final=lof, scale=3.5)
        ref = dpmpp_coef_table(ac, ts, order=order, lower_order_final=lof, scale=3.5)
        assert sde.dtype == np.float32 and sde.shape == (len(ts), 8)
        assert sde.tobytes() == ref.tobytes()


@pytest.mark.parametrize("method,steps", CASES)
@pytest.mark.parametrize("eta,s_noise", [(1.0, 1.0), (1.0, 0.8), (0.5, 1.0)])
def test_rows_match_closed_forms(method, steps, eta, s_noise):
    """x_next = (sg_n/sg_t) e^{-eta h} x + al_n (1 - e^{-(1+eta) h}) D + s_noise sg_n sqrt(1 - e^{-2 eta h}) z, written
    with exp instead of expm1, in float64, to fp32 rounding; the other columns are the 2M table's."""
    from lib.model_zoo.dpm_solver import dpmpp_coef_table, dpmpp_sde_coef_table
    ac, ts = _ac(), _timesteps(method, steps)
    tab = dpmpp_sde_coef_table(ac, ts, eta=eta, s_noise=s_noise, scale=2.0)
    base = dpmpp_coef_table(ac, ts, scale=2.0)
    assert tab.dtype == np.float32 and tab.shape == (len(ts), 8)
    for col in (0, 1, 2, 5, 6):
        assert np.array_equal(tab[:, col], base[:, col]), col
    a = np.array([float(np.float32(ac[t])) for t in ts])
    a_n = np.concatenate([[float(np.float32(ac[0]))], a[:-1]])
    lam = lambda v: 0.5 * np.log(v / (1.0 - v))
    h = lam(a_n) - lam(a)
    ref3 = np.sqrt((1.0 - a_n) / (1.0 - a)) * np.exp(-eta * h)
    ref4 = np.sqrt(a_n) * (1.0 - np.exp(-(1.0 + eta) * h))
    ref7 = s_noise * np.sqrt(1.0 - a_n) * np.sqrt(1.0 - np.exp(-2.0 * eta * h))
    np.testing.assert_allclose(tab[:, 3].astype(np.float64), ref3, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(tab[:, 4].astype(np.float64), ref4, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(tab[:, 7].astype(np.float64), ref7, rtol=2e-6, atol=1e-7)
    assert (tab[:, 7] > 0).all()


def test_eta1_preserves_the_marginal_variance():
    """With a perfect data prediction D = x0 and x = al_t x0 + sg_t e, the first-order eta = 1 step lands on
    al_n x0 + (sg_n e^{-h}) e + noise with total variance sg_n^2: (sg_n e^{-h})^2 + c_7^2 = sg_n^2, and the x0
    coefficient al_t ratio + c_d equals al_n."""
    from lib.model_zoo.dpm_solver import dpmpp_sde_coef_table
    ac, ts = _ac(), _timesteps("uniform", 20)
    tab = dpmpp_sde_coef_table(ac, ts, eta=1.0, order=1).astype(np.float64)
    a = np.array([float(np.float32(ac[t])) for t in ts])
    a_n = np.concatenate([[float(np.float32(ac[0]))], a[:-1]])
    np.testing.assert_allclose(np.sqrt(a) * tab[:, 3] + tab[:, 4], np.sqrt(a_n), rtol=1e-6)
    np.testing.assert_allclose((np.sqrt(1 - a) * tab[:, 3]) ** 2 + tab[:, 7] ** 2, 1 - a_n, rtol=1e-5, atol=1e-9)


def test_repeated_timestep_and_bad_arguments_raise():
    from lib.model_zoo.dpm_solver import dpmpp_sde_coef_table
    with pytest.raises(ValueError, match="index"):
        dpmpp_sde_coef_table(_ac(), _timesteps("quad", 50))
    with pytest.raises(ValueError):
        dpmpp_sde_coef_table(_ac(), _timesteps("uniform", 10), order=3)
    with pytest.raises(ValueError):
        dpmpp_sde_coef_table(_ac(), _timesteps("uniform", 10), eta=-0.5)


def test_sample_seeds_are_disjoint_and_stable_across_splits():
    from lib.model_zoo.sharded import sample_seeds, shard_bounds
    B, seed = 11, 1234
    whole = sample_seeds(seed, 0, B)
    assert whole == [seed * 2 ** 32 + i for i in range(B)] and len(set(whole)) == B
    assert all(0 <= s < 2 ** 63 for s in whole)
    for world in (1, 2, 3, 4, 11):
        parts = [sample_seeds(seed, *shard_bounds(B, world, r)) for r in range(world)]
        assert sum(parts, []) == whole, world
    assert not set(whole) & set(sample_seeds(seed + 1, 0, B))
    assert max(sample_seeds(2 ** 31 - 1, 0, 4)) < 2 ** 63
    for bad in (-1, 2 ** 31):
        with pytest.raises(ValueError):
            sample_seeds(bad, 0, 2)


class _Stub:
    """A model without a device: whatever gets past the validation fails on `.device` with AttributeError."""
    num_timesteps = 1000

    def __init__(self):
        self.alphas_cumprod = torch.from_numpy(_ac())


def _call(sampler, x_info, **kw):
    return sampler.sample(steps=5, shape=[2, 4, 8, 8], x_info=x_info, c_info={}, verbose=False, **kw)


def test_sampler_validates_before_any_device_work():
    from lib.model_zoo.dpm_solver import DPMSolverSDESampler
    with pytest.raises(ValueError):
        DPMSolverSDESampler(_Stub(), order=3)
    with pytest.raises(ValueError):
        DPMSolverSDESampler(_Stub(), eta=-1.0)
    s = DPMSolverSDESampler(_Stub())
    assert s.eta == 1.0
    with pytest.raises(ValueError, match="seeds"):
        _call(s, {"type": "image"})                                     # missing
    with pytest.raises(ValueError, match="seeds"):
        _call(s, {"type": "image", "seeds": [1]})                       # short
    with pytest.raises(ValueError, match="seeds"):
        _call(s, {"type": "image", "seeds": [1, -2]})                   # negative
    with pytest.raises(ValueError, match="seeds"):
        _call(s, {"type": "image", "seeds": [1, 2 ** 63]})              # out of range
    with pytest.raises(ValueError, match="seeds"):
        _call(s, {"type": "image", "seeds": torch.tensor([1, 2, 3])})   # long, as a tensor
    with pytest.raises(ValueError, match="seeds"):
        _call(s, {"type": "image", "seeds": [1.5, 2.0]})
    with pytest.raises(ValueError, match="noise_dropout"):
        _call(s, {"type": "image", "seeds": [1, 2]}, noise_dropout=0.1)
    with pytest.raises(ValueError):
        _call(s, {"type": "image", "seeds": [1, 2]}, eta=-0.5)
    # x_info["type"] is not restricted; valid arguments get past the validation (and then need a real model)
    for x_info, kw in (({"type": "text", "seeds": [1, 2]}, {}), ({"type": "image"}, {"eta": 0.0}),
                       ({"type": "image", "seeds": torch.tensor([3, 2 ** 63 - 1])}, {})):
        with pytest.raises(AttributeError):
            _call(s, x_info, **kw)
    with pytest.raises(NotImplementedError):
        s._step()


def test_2m_sampler_still_rejects_stochastic_arguments():
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    s = DPMSolverSampler(_Stub())
    with pytest.raises(ValueError):
        _call(s, {"type": "image"}, eta=0.5)
    with pytest.raises(ValueError):
        _call(s, {"type": "image"}, noise_dropout=0.1)
    with pytest.raises(ValueError):
        _call(s, {"type": "image", "seeds": [1, 2]}, eta=1.0)
