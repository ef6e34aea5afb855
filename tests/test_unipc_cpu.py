"""UniPC coefficient table (lib/model_zoo/unipc.unipc_coef_table) on the host: whole loops driven by its collapsed rows
against an independent float64 restatement of the method in difference form, its identities with DDIM and DPM-Solver++(2M),
its formal orders on an analytic problem, its convergence on the tiny fp32 oracle model, and the sampler's argument
validation.  No GPU, no library needed."""
import json
import math

import numpy as np
import pytest
import torch

from vdtest_util import load_gold, meta, rel_l2


def _ac():
    from oracle import vd_oracle as O
    return O.register_schedule()["alphas_cumprod"].numpy()


def _timesteps(method, steps):
    from lib.model_zoo.diffusion_utils import make_ddim_timesteps
    return make_ddim_timesteps(method, steps, 1000, verbose=False)


def run_rows(tab, x, model):
    """A whole loop from the collapsed rows; model(x, i) is the (guided) noise prediction at DDIM index i.  Returns the final
    latent and the final state (x_last, m_1, m_2, m_3).  An operand whose coefficient is 0 is not touched (it may be None)."""
    tab = np.asarray(tab, dtype=np.float64)
    xl = m1 = m2 = m3 = None
    for i in reversed(range(tab.shape[0])):
        r = tab[i]
        mt = (x - r[2] * model(x, i)) * r[1]
        if r[3] != 0:
            xc = r[4] * xl + r[8] * mt
            for c, m in ((r[5], m1), (r[6], m2), (r[7], m3)):
                if c != 0:
                    xc = xc + c * m
        else:
            xc = x
        xn = r[9] * xc + r[10] * mt
        for c, m in ((r[11], m1), (r[12], m2)):
            if c != 0:
                xn = xn + c * m
        xl, m1, m2, m3, x = xc, mt, m1, m2, xn
    return x, (xl, m1, m2, m3)


def _rho_restated(P, rks, hh, corrector):
    """The weights of an update of order P (bh2: B = expm1(hh)), from the linear system R rho = b of the paper."""
    r = list(rks) + [1.0]
    phi1 = math.expm1(hh)
    g = [phi1 / hh - 1.0]
    for i in range(1, P):
        g.append(g[-1] / hh - 1.0 / math.factorial(i + 1))
    R = np.array([[rj ** i for rj in r] for i in range(P)])
    b = np.array([g[i] * math.factorial(i + 1) / phi1 for i in range(P)])
    if corrector:
        return [0.5] if P == 1 else list(np.linalg.solve(R, b))
    if P <= 2:
        return [0.5][:P - 1]
    return list(np.linalg.solve(R[:P - 1, :P - 1], b[:P - 1]))


def run_restated(ac, ts, order, corrector, lower_order_final, x, model):
    """UniPC (bh2, data prediction) in difference form, float64: sampling step k works on DDIM index S-1-k and goes from
    a_t = ac[ts[i]] to DDIM's previous alpha (ac[ts[i-1]], ac[0] for i = 0)."""
    S = len(ts)
    a = [float(np.float32(ac[t])) for t in ts]
    a_n = [float(np.float32(ac[0]))] + a[:-1]
    lam = lambda v: 0.5 * math.log(v / (1.0 - v))
    hist = []                  # (lam, sg, m) of the previous steps, the most recent first
    x_last, p_prev = None, None
    for k in range(S):
        i = S - 1 - k
        al_t, sg_t, lam_t = math.sqrt(a[i]), math.sqrt(1.0 - a[i]), lam(a[i])
        al_n, sg_n, lam_n = math.sqrt(a_n[i]), math.sqrt(1.0 - a_n[i]), lam(a_n[i])
        m_t = (x - sg_t * model(x, i)) / al_t
        x_c = x
        if corrector and k >= 1:
            q = p_prev
            lam_1, sg_1, m_1 = hist[0]
            h = lam_t - lam_1
            rks = [(hist[j][0] - lam_1) / h for j in range(1, q)]
            D = [(hist[j][2] - m_1) / rks[j - 1] for j in range(1, q)]
            rho = _rho_restated(q, rks, -h, True)
            phi1 = math.expm1(-h)
            res = rho[-1] * (m_t - m_1)
            for rj, Dj in zip(rho[:-1], D):
                res = res + rj * Dj
            x_c = sg_t / sg_1 * x_last - al_t * phi1 * m_1 - al_t * phi1 * res
        p = min(order, k + 1, S - k) if lower_order_final else min(order, k + 1)
        h = lam_n - lam_t
        rks = [(hist[j - 1][0] - lam_t) / h for j in range(1, p)]
        D = [(hist[j - 1][2] - m_t) / rks[j - 1] for j in range(1, p)]
        rho = _rho_restated(p, rks, -h, False)
        phi1 = math.expm1(-h)
        x_next = sg_n / sg_t * x_c - al_n * phi1 * m_t
        for rj, Dj in zip(rho, D):
            x_next = x_next - al_n * phi1 * rj * Dj
        hist.insert(0, (lam_t, sg_t, m_t))
        x_last, p_prev, x = x_c, p, x_next
    ms = [hist[j][2] if j < len(hist) else None for j in range(3)]
    return x, (x_last, ms[0], ms[1], ms[2])


def _random_model(seed, n=64):
    """A fixed smooth 'network': eps(x, i) = tanh(A x) + b_i, the same function for every solver that is handed it."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    b = 0.3 * rng.standard_normal((1024, n))
    return (lambda x, i: np.tanh(A @ x) + b[i]), rng.standard_normal(n)


CASES = [(m, s) for m in ("uniform", "quad") for s in (1, 2, 3, 5, 10, 20, 50) if not (m == "quad" and s > 25)]


@pytest.mark.parametrize("method,steps", CASES)
@pytest.mark.parametrize("order", [1, 2, 3])
def test_table_loops_match_the_restated_method(method, steps, order):
    from lib.model_zoo import unipc
    ac, ts = _ac(), _timesteps(method, steps)
    if (method, steps) == ("uniform", 3):
        # no such schedule: the uniform grid of 3 steps over 1000 holds timestep 1000 and DDIM's own parameters raise, as the
        # reference's do (test_host_cpu pins that for the sampler); the table hands the error on
        with pytest.raises(IndexError):
            unipc.unipc_coef_table(ac, ts, order=order)
        return
    S = len(ts)
    model, x0 = _random_model(steps + 7 * order)
    for corrector in (True, False):
        for lof in (True, False):
            tab = unipc.unipc_coef_table(ac, ts, order=order, corrector=corrector, lower_order_final=lof, scale=3.5)
            assert tab.dtype == np.float32 and tab.shape == (S, 16) and tab.shape[1] % 4 == 0
            assert (tab[:, unipc.SCALE] == 3.5).all() and (tab[:, 14:] == 0).all()
            # the first step of a call has no corrector; an entry of the history that does not exist yet has coefficient 0
            assert tab[S - 1, unipc.CORR] == 0
            for k in range(S):
                row = tab[S - 1 - k]
                assert row[unipc.HIST] == min(k, 3)
                assert row[unipc.CORR] == (1.0 if corrector and k >= 1 else 0.0)
                if row[unipc.CORR] == 0:
                    assert (row[unipc.C_X:unipc.C_T + 1] == 0).all()
                for j in range(1, 4):
                    if j > k:
                        assert row[unipc.C_1 + j - 1] == 0, (k, j)
                        assert j > 2 or row[unipc.P_1 + j - 1] == 0, (k, j)
            got, got_state = run_rows(tab, x0.copy(), model)
            ref, ref_state = run_restated(ac, ts, order, corrector, lof, x0.copy(), model)
            what = (corrector, lof)
            assert rel_l2(got, ref) < 1e-6, what
            assert rel_l2(got_state[0], ref_state[0]) < 1e-6, what
            for g, r in zip(got_state[1:], ref_state[1:]):
                assert (g is None) == (r is None), what
                if r is not None:
                    assert rel_l2(g, r) < 1e-6, what


def test_repeated_timestep_and_bad_order_raise():
    from lib.model_zoo.unipc import unipc_coef_table
    with pytest.raises(ValueError, match="index"):
        unipc_coef_table(_ac(), _timesteps("quad", 50))
    for order in (0, 4, 2.5):
        with pytest.raises(ValueError, match="order"):
            unipc_coef_table(_ac(), _timesteps("uniform", 10), order=order)


@pytest.mark.parametrize("method,steps", [("uniform", 5), ("uniform", 50), ("quad", 20)])
def test_order1_without_corrector_is_ddim(method, steps):
    """order=1, corrector=False: x_next = p_x x + p_t m_t == sqrt(a_prev) x0 + sqrt(1 - a_prev) e (DDIM, eta = 0)."""
    from lib.model_zoo import unipc
    from lib.model_zoo.diffusion_utils import make_ddim_sampling_parameters
    ac, ts = _ac(), _timesteps(method, steps)
    tab = unipc.unipc_coef_table(ac, ts, order=1, corrector=False).astype(np.float64)
    assert not tab[:, unipc.CORR].any() and not tab[:, unipc.P_1:unipc.P_2 + 1].any()
    _, alphas, alphas_prev = make_ddim_sampling_parameters(ac, ts, 0.0, verbose=False)
    rng = np.random.default_rng(3)
    for i in range(len(ts)):
        x, e = rng.standard_normal(4096), rng.standard_normal(4096)
        m_t = (x - tab[i, unipc.SQRT_1MAT] * e) * tab[i, unipc.RSQRT_AT]
        ours = tab[i, unipc.P_X] * x + tab[i, unipc.P_T] * m_t
        x0_ref = (x - np.sqrt(1 - alphas[i]) * e) / np.sqrt(alphas[i])
        ddim = np.sqrt(alphas_prev[i]) * x0_ref + np.sqrt(1 - alphas_prev[i]) * e
        assert np.linalg.norm(ours - ddim) / np.linalg.norm(ddim) < 1e-6, i


@pytest.mark.parametrize("method,steps", [("uniform", 2), ("uniform", 5), ("uniform", 10), ("uniform", 13), ("quad", 5),
                                          ("quad", 10)])
def test_order2_without_corrector_is_dpmpp_2m(method, steps):
    """Below 15 steps both tables end on a first-order step: the predictor alone with rho = 1/2 is DPM-Solver++(2M)."""
    from lib.model_zoo.dpm_solver import dpmpp_coef_table
    from lib.model_zoo.unipc import unipc_coef_table
    ac, ts = _ac(), _timesteps(method, steps)
    assert len(ts) < 15            # (the uniform grid of 13 steps has 14 timesteps)
    model, x0 = _random_model(steps)
    got, _ = run_rows(unipc_coef_table(ac, ts, order=2, corrector=False), x0.copy(), model)
    tab = dpmpp_coef_table(ac, ts, order=2).astype(np.float64)
    x, hist = x0.copy(), None
    for i in reversed(range(len(ts))):
        m = (x - tab[i, 2] * model(x, i)) * tab[i, 1]
        d = tab[i, 5] * m + (tab[i, 6] * hist if tab[i, 6] != 0 else 0.0)
        x, hist = tab[i, 3] * x + tab[i, 4] * d, m
    assert rel_l2(got, x) < 1e-6


def test_formal_orders_on_gaussian_data():
    """The analytic problem of test_dpm_solver_cpu.test_formal_orders_on_gaussian_data (data ~ N(0, diag(s2)), exact eps and
    exact solution), quad grid, error ratios from 10 to 20 steps.  Measured: order 1 with the corrector 4.2 (second order),
    order 2 with it 11.0 (third order), and UniPC-2 at 20 steps has 0.092 of 2M's error.  A wrong r_j, a reversed history
    or a corrector fed the wrong order loses these."""
    from lib.model_zoo.dpm_solver import dpmpp_coef_table
    from lib.model_zoo.unipc import unipc_coef_table
    ac = _ac().astype(np.float64)
    s2 = np.array([0.01, 0.3, 1.0, 4.0])
    xT = np.array([1.0, -0.7, 0.5, 2.0])

    def eps_at(ts):
        def eps(x, i):
            a = float(np.float32(ac[ts[i]]))
            x0 = np.sqrt(a) * s2 / (a * s2 + 1 - a) * x
            return (x - np.sqrt(a) * x0) / np.sqrt(1 - a)
        return eps

    def exact(ts):
        a_T, a_0 = float(np.float32(ac[ts[-1]])), float(np.float32(ac[0]))
        return np.sqrt(a_0 * s2 + 1 - a_0) * xT / np.sqrt(a_T * s2 + 1 - a_T)

    def err(ts, order):
        x, _ = run_rows(unipc_coef_table(ac, ts, order=order), xT.copy(), eps_at(ts))
        return np.linalg.norm(x - exact(ts)) / np.linalg.norm(exact(ts))

    def err_2m(ts):
        tab, eps = dpmpp_coef_table(ac, ts, order=2).astype(np.float64), eps_at(ts)
        x, hist = xT.copy(), None
        for i in reversed(range(len(ts))):
            x0 = (x - tab[i, 2] * eps(x, i)) * tab[i, 1]
            d = tab[i, 5] * x0 + (tab[i, 6] * hist if tab[i, 6] != 0 else 0.0)
            x, hist = tab[i, 3] * x + tab[i, 4] * d, x0
        return np.linalg.norm(x - exact(ts)) / np.linalg.norm(exact(ts))

    e = {(n, o): err(_timesteps("quad", n), o) for n in (10, 20) for o in (1, 2)}
    e2m = err_2m(_timesteps("quad", 20))
    print("UniPC errors:", e, "2M at 20 steps:", e2m)
    assert e[10, 1] / e[20, 1] > 3.2, e
    assert e[10, 2] / e[20, 2] > 6, e
    assert e[20, 2] < 0.15 * e2m, (e, e2m)


def test_convergence_on_tiny_oracle():
    """The set-up of test_dpm_solver_cpu.test_convergence_on_tiny_oracle (CFG 3.0, B = 2, 16x16, quad grids from t = 801) and
    its reference, the 201-step 2M solution.  UniPC-2 at 201 steps must land on it within 7e-5, the distance the 2M test
    states between that reference and a 401-step one (measured: 1.2e-5).  At 10 and 20 steps UniPC-2's error is below 0.92 of
    2M's (measured 0.80 and 0.84: eps of the synthetic weights is rough in t, so no solver reaches its formal order)."""
    from lib.model_zoo.dpm_solver import dpmpp_coef_table
    from lib.model_zoo.unipc import unipc_coef_table
    from oracle import synth, vd_oracle as O
    m = meta()
    g = load_gold("unet_tiny.npz")
    shapes = {str(k): tuple(json.loads(str(s))) for k, s in zip(g["state_keys"], g["state_shapes"])}
    sd = synth.synth_state_dict(shapes, m["seed"])
    plan = O.unet_plan(**m["unet2d"])
    ac = _ac()
    gen = torch.Generator().manual_seed(11)
    B, scale = 2, 3.0
    c = torch.randn((B, 77, 128), generator=gen) * 0.5
    u = torch.randn((1, 77, 128), generator=gen).repeat(B, 1, 1) * 0.5
    xT = torch.randn((B, 4, 16, 16), generator=gen).double().numpy()

    def eps_at(ts):
        def eps(x, i):
            xin = torch.from_numpy(x).float().repeat(2, 1, 1, 1)
            with torch.no_grad():
                e = O.apply_model_multicontext(sd, plan, xin, torch.full((2 * B,), int(ts[i]), dtype=torch.long),
                                               [("text", torch.cat([u, c]), 1.0)], "image", global_ptr="image")
            e_u, e_c = e.double().numpy()[:B], e.double().numpy()[B:]
            return e_u + scale * (e_c - e_u)
        return eps

    def dpm(ts):
        tab, eps = dpmpp_coef_table(ac, ts, order=2, scale=scale).astype(np.float64), eps_at(ts)
        x, hist = xT.copy(), None
        for i in reversed(range(len(ts))):
            x0 = (x - tab[i, 2] * eps(x, i)) * tab[i, 1]
            d = tab[i, 5] * x0 + (tab[i, 6] * hist if tab[i, 6] != 0 else 0.0)
            x, hist = tab[i, 3] * x + tab[i, 4] * d, x0
        return x

    def unipc(ts):
        return run_rows(unipc_coef_table(ac, ts, order=2, scale=scale), xT.copy(), eps_at(ts))[0]

    fine = np.arange(1, 802, 4)
    ref = dpm(fine)
    far = rel_l2(unipc(fine), ref)
    errs = {}
    for n in (10, 20):
        ts = _timesteps("quad", n)
        assert ts[0] == 1 and ts[-1] == 801
        errs[n] = (rel_l2(unipc(ts), ref), rel_l2(dpm(ts), ref))
    print("UniPC-2 at 201 steps vs the 201-step 2M reference: %.3e; rel-L2 vs it (UniPC-2, 2M): %r" % (far, errs))
    assert far < 7e-5
    assert errs[10][0] < 0.92 * errs[10][1], errs
    assert errs[20][0] < 0.92 * errs[20][1], errs


def test_sampler_validates_before_device_work():
    from lib.model_zoo.unipc import UniPCSampler

    class _Stub:
        num_timesteps = 1000
        alphas_cumprod = torch.from_numpy(_ac())

        @property
        def device(self):
            raise AssertionError("the sampler touched the device before validating its arguments")

    for order in (0, 4):
        with pytest.raises(ValueError, match="order"):
            UniPCSampler(_Stub(), order=order)
    s = UniPCSampler(_Stub(), order=3)
    assert s.order == 3 and s.corrector and s.lower_order_final and not s.draws_step_noise and s.coef_width == 16
    args = dict(steps=5, shape=[1, 4, 8, 8], x_info={"type": "image"}, c_info={}, verbose=False)
    with pytest.raises(ValueError, match="eta"):
        s.sample(eta=0.5, **args)
    with pytest.raises(ValueError, match="noise_dropout"):
        s.sample(noise_dropout=0.1, **args)
    with pytest.raises(ValueError, match="noise_dropout"):
        s.sample_multicontext(steps=5, shape=[1, 4, 8, 8], x_info={"type": "image"}, c_info_list=[{}], noise_dropout=0.1,
                              verbose=False)
    # a repeated timestep: the table of the quad grid at 50 steps
    s.make_schedule(50, ddim_discretize="quad", verbose=False)
    with pytest.raises(ValueError, match="index"):
        s._coef_table(len(s.ddim_timesteps), 7.5, torch.device("cpu"))
    # no single-step API
    class _OnCpu(_Stub):
        device = torch.device("cpu")

    x_info = {"type": "image", "x": torch.zeros(1, 4, 8, 8)}
    c_info = {"type": "text", "conditioning": torch.zeros(1, 7, 16), "unconditional_guidance_scale": 1.0}
    with pytest.raises(NotImplementedError, match="single-step"):
        UniPCSampler(_OnCpu()).p_sample_ddim(x_info, c_info, torch.tensor([1]), 0)
