"""UniPC sampler (Zhao et al., "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models", 2023;
variant bh2 with data prediction, what diffusers' UniPCMultistepScheduler(solver_type="bh2", predict_x0=True) computes) with
classifier-free guidance, on DDIMSampler's static step loop.

`UniPCSampler(model).sample(steps, shape, x_info, c_info)` has DDIMSampler's arguments, dict protocol and return values and
runs every flow it runs.  It walks the same DDIM timestep grid as DPMSolverSampler.  Its corrector reuses the model output the
next predictor needs anyway, so it raises the order by one at no extra UNet evaluation: the step stays UNet forward + ONE fused
kernel (ops.cfg_unipc_step_dev: CFG combine, corrector, predictor and the shift of the history), captured once into a HIP
graph and replayed.  The solver's state is four fp32 buffers (the corrected latent the previous predictor started from and
the data predictions of the last three steps); the per-step scalars are a row of the fp32 [S, 16] table of unipc_coef_table,
copied into a device buffer between replays.
"""
import math

import numpy as np
import torch

from vd_hip import ops

from .ddim import DDIMSampler
from .diffusion_utils import make_ddim_sampling_parameters

COEF_WIDTH = 16
# columns of a row (the layout vd_cfg_unipc_step_dev_f16 reads)
SCALE, RSQRT_AT, SQRT_1MAT, CORR, C_X, C_1, C_2, C_3, C_T, P_X, P_T, P_1, P_2, HIST = range(14)


def _solve(R, b):
    """The solution of the 1x1 .. 3x3 system R x = b: Gaussian elimination with partial pivoting on Python floats (a table
    holds two such systems per step; a LAPACK call per system would cost more than the rest of the table)."""
    n = len(b)
    A = [list(R[i]) + [b[i]] for i in range(n)]
    for c in range(n):
        piv = max(range(c, n), key=lambda i: abs(A[i][c]))
        A[c], A[piv] = A[piv], A[c]
        for i in range(c + 1, n):
            f = A[i][c] / A[c][c]
            for j in range(c, n + 1):
                A[i][j] -= f * A[c][j]
    x = [0.0] * n
    for i in reversed(range(n)):
        x[i] = (A[i][n] - sum(A[i][j] * x[j] for j in range(i + 1, n))) / A[i][i]
    return x


def _rho(P, rks, hh, corrector):
    """(rho, phi1, B) of a UniPC update of order P over a step of log-SNR length h = -hh, variant bh2 (B = phi1):
    R[i][j] = r_j^i with r_P = 1 and b_i = g_i (i+1)! / B, g_0 = phi1/hh - 1, g_{i+1} = g_i/hh - 1/(i+2)!.  The predictor
    takes P - 1 weights: none for P = 1, the paper's 1/2 for P = 2, the leading (P-1)x(P-1) system otherwise; the corrector
    takes P: 1/2 for P = 1, else the full system."""
    phi1 = math.expm1(hh)
    B = phi1
    r = list(rks) + [1.0]
    R = [[rj ** i for rj in r] for i in range(P)]
    b, g, fact = [], phi1 / hh - 1.0, 1.0
    for i in range(P):
        b.append(g * fact / B)
        fact *= i + 2
        g = g / hh - 1.0 / fact
    if corrector:
        rho = [0.5] if P == 1 else _solve(R, b)
    elif P <= 2:
        rho = [0.5] * (P - 1)
    else:
        rho = _solve([row[:P - 1] for row in R[:P - 1]], b[:P - 1])
    return rho, phi1, B


def unipc_coef_table(alphas_cumprod, timesteps, order=2, corrector=True, lower_order_final=True, scale=1.0):
    """fp32 [S, 16] rows per DDIM index, computed in float64 (the layout the kernel reads, see vd_cfg_unipc_step_dev_f16):

        {scale, 1/al_t, sg_t, corrector on, c_x, c_1, c_2, c_3, c_t, p_x, p_t, p_1, p_2, hist, 0, 0}

    in the notation of dpmpp_coef_table: a_t, a_n are DDIM's arrays, al = sqrt(a), sg = sqrt(1 - a), lam = log(al / sg);
    sampling step k = 0 .. S-1 works on index i = S-1-k.  With m_t the data prediction of this step, x_last the corrected
    latent the previous predictor started from and m_1, m_2, m_3 the data predictions of the previous steps (m_1 the most
    recent, at lam_1 = lam_t[i+1] and so on), the step is

        x_c    = c_x x_last + c_1 m_1 + c_2 m_2 + c_3 m_3 + c_t m_t        (corrector on; else x_c = x)
        x_next = p_x x_c + p_t m_t + p_1 m_1 + p_2 m_2

    the collapsed form of the paper's updates, which are linear in their operands:

        corrector, h = lam_t - lam_1, r_j = (lam_{j+1} - lam_1)/h, D_j = (m_{j+1} - m_1)/r_j, order q:
            x_c = (sg_t/sg_1) x_last - al_t phi1 m_1 - al_t B (sum_{j<q} rho_j D_j + rho_q (m_t - m_1))
        predictor, h = lam_n - lam_t, r_j = (lam_j - lam_t)/h, D_j = (m_j - m_t)/r_j, order p:
            x_next = (sg_n/sg_t) x_c - al_n phi1 m_t - al_n B sum_{j<p} rho_j D_j

    with phi1 = B = expm1(-h) and the weights rho of _rho.  The predictor order of step k is p_k = min(order, k + 1), also
    capped by S - k when lower_order_final is set; the corrector of step k >= 1 has the order q = p_{k-1} and step 0 has none
    (nor has any step when corrector is False).  hist = min(k, 3) tells the kernel how much history exists; the coefficient
    of an entry that does not exist yet is exactly 0.  order 1 without the corrector is DDIM at eta = 0, order 2 without it
    is DPM-Solver++(2M).  A repeated timestep (h <= 0) raises ValueError as in dpmpp_coef_table.

    Rounding to fp32: the history coefficients (c_1..c_3, p_1, p_2) are rounded as they are; c_t and p_t are then chosen so
    that the fp32 coefficients of the data predictions add up to the float64 sum.  The m_j of neighbouring steps are close,
    so what matters is that sum and the weights of their differences: rounded like this the collapsed row is as accurate as
    the difference form with fp32 weights.  It matters where the weights are large and cancel -- up to 16 in magnitude on a
    last step of order 3 without lower_order_final (|coef| <= 2.8 with it), where plain rounding costs 1.4e-6 rel-L2 over a
    20-step loop and this 7e-7."""
    tab = _rows_f64(alphas_cumprod, timesteps, order, corrector, lower_order_final, scale)
    out = tab.astype(np.float32)
    for hist_cols, cur in (((C_1, C_2, C_3), C_T), ((P_1, P_2), P_T)):
        total = tab[:, list(hist_cols) + [cur]].sum(axis=1)
        out[:, cur] = (total - out[:, list(hist_cols)].astype(np.float64).sum(axis=1)).astype(np.float32)
    return out


def _rows_f64(alphas_cumprod, timesteps, order, corrector, lower_order_final, scale):
    """unipc_coef_table before its rounding to fp32."""
    if order not in (1, 2, 3):
        raise ValueError("UniPC order must be 1, 2 or 3, got %r" % (order,))
    ts = np.asarray(timesteps)
    S = ts.shape[0]
    _, a_t, a_next = make_ddim_sampling_parameters(alphas_cumprod, ts, 0.0, verbose=False)
    a_t, a_next = np.asarray(a_t, np.float64), np.asarray(a_next, np.float64)
    al_t, sg_t = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    al_n, sg_n = np.sqrt(a_next), np.sqrt(1.0 - a_next)
    lam_t, lam_n = np.log(al_t) - np.log(sg_t), np.log(al_n) - np.log(sg_n)
    for i in range(S):
        if not lam_n[i] - lam_t[i] > 0.0:
            raise ValueError("UniPC: DDIM index %d (timestep %d) does not advance the log-SNR (h = %r); the timestep grid "
                             "repeats a step" % (i, int(ts[i]), float(lam_n[i] - lam_t[i])))
    orders = [min(order, k + 1, S - k) if lower_order_final else min(order, k + 1) for k in range(S)]
    # the step loop on Python floats (numpy scalars would cost several times the arithmetic)
    al_t, sg_t, al_n, sg_n, lam_t, lam_n = (v.tolist() for v in (al_t, sg_t, al_n, sg_n, lam_t, lam_n))
    tab = [[0.0] * COEF_WIDTH for _ in range(S)]
    for k in range(S):
        i = S - 1 - k
        tab[i][SCALE], tab[i][RSQRT_AT], tab[i][SQRT_1MAT], tab[i][HIST] = float(scale), 1.0 / al_t[i], sg_t[i], min(k, 3)
        if corrector and k >= 1:
            q = orders[k - 1]
            h = lam_t[i] - lam_t[i + 1]
            rks = [(lam_t[i + 1 + j] - lam_t[i + 1]) / h for j in range(1, q)]
            rho, phi1, B = _rho(q, rks, -h, True)
            tab[i][CORR] = 1.0
            tab[i][C_X] = sg_t[i] / sg_t[i + 1]
            tab[i][C_T] = -al_t[i] * B * rho[q - 1]
            tab[i][C_1] = -al_t[i] * phi1 + al_t[i] * B * (sum(rho[j - 1] / rks[j - 1] for j in range(1, q)) + rho[q - 1])
            for j in range(1, q):
                tab[i][C_1 + j] = -al_t[i] * B * rho[j - 1] / rks[j - 1]
        p = orders[k]
        h = lam_n[i] - lam_t[i]
        rks = [(lam_t[i + j] - lam_t[i]) / h for j in range(1, p)]
        rho, phi1, B = _rho(p, rks, -h, False)
        tab[i][P_X] = sg_n[i] / sg_t[i]
        tab[i][P_T] = -al_n[i] * phi1 + al_n[i] * B * sum(rho[j - 1] / rks[j - 1] for j in range(1, p))
        for j in range(1, p):
            tab[i][P_T + j] = -al_n[i] * B * rho[j - 1] / rks[j - 1]
    return np.array(tab, dtype=np.float64)


class UniPCSampler(DDIMSampler):
    """UniPC (bh2, data prediction) with classifier-free guidance; deterministic (eta = 0 only).  order: the predictor's, 1 to
    3 (the corrector adds one); corrector=False leaves the predictor alone (order 1: DDIM, order 2: DPM-Solver++(2M)).

    RNG contract: DPMSolverSampler's -- the device generator is used only for x_T (or q_sample's forward noise), nothing per
    step.  When inpainting, only the latent is blended: the solver's state keeps the raw values, as 2M's history does."""
    coef_width = COEF_WIDTH
    draws_step_noise = False
    _state_names = ("x_last", "m1", "m2", "m3")

    def __init__(self, model, schedule="linear", order=2, corrector=True, lower_order_final=True, **kwargs):
        if order not in (1, 2, 3):
            raise ValueError("UniPCSampler: order must be 1, 2 or 3, got %r" % (order,))
        super().__init__(model, schedule=schedule, **kwargs)
        self.order = order
        self.corrector = bool(corrector)
        self.lower_order_final = bool(lower_order_final)
        self._table = (None, None)          # (key, rows) of the last call: see _coef_table

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0.:
            raise ValueError("UniPCSampler is deterministic: eta must be 0, got %r" % (ddim_eta,))
        super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=ddim_eta, verbose=verbose)

    def _ddim_sampling_multicontext(self, shape, x_info, c_info_list, noise_dropout, temperature, log_every_t, _single):
        if noise_dropout > 0.:
            raise ValueError("UniPCSampler is deterministic: noise_dropout must be 0, got %r" % (noise_dropout,))
        return super()._ddim_sampling_multicontext(shape, x_info, c_info_list, noise_dropout, temperature, log_every_t,
                                                   _single)

    def _coef_table(self, total_steps, scale, device):
        # the rows cost about half a millisecond of host arithmetic per call (two small linear systems per step): a call that
        # repeats the previous call's grid, schedule and scale -- a server's usual case -- takes them from the last call
        ts = np.ascontiguousarray(self.ddim_timesteps[:total_steps])
        key = (ts.tobytes(), np.asarray(self.alphas_cumprod).tobytes(), self.order, self.corrector, self.lower_order_final,
               float(scale))
        if self._table[0] != key:
            self._table = (key, unipc_coef_table(self.alphas_cumprod, ts, order=self.order, corrector=self.corrector,
                                                 lower_order_final=self.lower_order_final, scale=scale))
        return torch.from_numpy(self._table[1]).to(device)

    def _extra_static(self, x):
        # not read on the first step of a call (rows with hist = 0), so they need no initial value
        return {k: torch.empty(x.shape, device=x.device, dtype=torch.float32) for k in self._state_names}

    def _update_static(self, bufs, eps, guided):
        state = tuple(bufs[k] for k in self._state_names)
        if "kfac" in bufs:      # guidance rescale: the factor kernel, then the update that multiplies by its factors
            self._rescale_static(bufs, eps)
            ops.cfg_unipc_step_dev_rs(bufs["xs"], eps, bufs["coef"], state, bufs["kfac"], guided=guided, x_next=bufs["xs"],
                                      pred_x0=bufs["p0"])
        else:
            ops.cfg_unipc_step_dev(bufs["xs"], eps, bufs["coef"], state, guided=guided, x_next=bufs["xs"],
                                   pred_x0=bufs["p0"])
        if "mask" in bufs:      # inpainting: the state keeps the raw values, only the latent is blended
            self._blend_static(bufs, bufs["xs"])

    def _step(self, *args, **kwargs):
        # the multistep update needs the history of the loop: there is no stand-alone single step (p_sample_ddim*)
        raise NotImplementedError("%s runs whole sample() loops on the GPU; it has no single-step API" % type(self).__name__)
