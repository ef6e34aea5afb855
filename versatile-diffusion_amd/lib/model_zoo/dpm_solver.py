"""DPM-Solver++(2M) sampler (Lu et al., "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic
Models", 2022, Algorithm 2) with classifier-free guidance, on DDIMSampler's static step loop.

`DPMSolverSampler(model).sample(steps, shape, x_info, c_info)` has DDIMSampler's arguments, dict protocol and return
values and runs every flow it runs (xt / x0 + x0_forward_timesteps / random x_T, the 0-D text latent, multi-context).  It
walks the same DDIM timestep grid; at 15-25 steps the multistep update gets close to what DDIM gives at 50.

The whole step -- UNet forward + ONE fused kernel for the CFG combine and the multistep update
(ops.cfg_dpmpp_step_dev) -- is captured once into a HIP graph and replayed, exactly like DDIM: the solver's only state is
an fp32 buffer holding the previous step's data prediction x0, and the per-step scalars are a row of the fp32[S, 8]
table of dpmpp_coef_table, copied into a device buffer between replays.
"""
import numpy as np
import torch

from vd_hip import ops

from .ddim import DDIMSampler
from .diffusion_utils import make_ddim_sampling_parameters


def dpmpp_coef_table(alphas_cumprod, timesteps, order=2, lower_order_final=True, scale=1.0):
    """fp32 [S, 8] rows {scale, 1/sqrt(a_t), sqrt(1-a_t), sigma_next/sigma_t, c_d, w_cur, w_prev, 0} per DDIM index,
    computed in float64 (the layout the kernel reads, see vd_cfg_dpmpp_step_dev_f16).

    a_t = ac[timesteps[i]] and a_next = alphas_prev[i] are DDIM's own arrays (make_ddim_sampling_parameters), so the last
    step goes to ac[0] as DDIM's does.  With alpha = sqrt(a), sigma = sqrt(1-a), lambda = log(alpha / sigma) and
    h = lambda_next - lambda_t:  x_next = (sigma_next/sigma_t) x - alpha_next expm1(-h) D, where D = x0 on first-order
    rows and D = (1 + 1/(2r)) x0 - 1/(2r) x0_prev with r = h_prev / h on second-order rows (h_prev: the h of the step
    that produced x0_prev, i.e. row i + 1 -- sampling runs from index S-1 down to 0).

    First-order rows: the first step of a call (index S-1), every row when order == 1, and the final step (index 0) when
    lower_order_final is set and there are fewer than 15 steps.  A first-order row is DDIM with eta = 0:
    x_next = alpha_next x0 + sigma_next e.  A repeated timestep (h = 0, e.g. the "quad" grid at >= 50 steps) raises
    ValueError."""
    if order not in (1, 2):
        raise ValueError("DPM-Solver++ order must be 1 or 2, got %r" % (order,))
    ts = np.asarray(timesteps)
    S = ts.shape[0]
    _, a_t, a_next = make_ddim_sampling_parameters(alphas_cumprod, ts, 0.0, verbose=False)
    a_t, a_next = np.asarray(a_t, np.float64), np.asarray(a_next, np.float64)
    al_t, sg_t = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    al_n, sg_n = np.sqrt(a_next), np.sqrt(1.0 - a_next)
    h = (np.log(al_n) - np.log(sg_n)) - (np.log(al_t) - np.log(sg_t))
    for i in range(S):
        if not h[i] > 0.0:
            raise ValueError("DPM-Solver++: DDIM index %d (timestep %d) does not advance the log-SNR (h = %r); the "
                             "timestep grid repeats a step" % (i, int(ts[i]), float(h[i])))
    tab = np.zeros((S, 8), dtype=np.float64)
    tab[:, 0] = float(scale)
    tab[:, 1] = 1.0 / al_t
    tab[:, 2] = sg_t
    tab[:, 3] = sg_n / sg_t
    tab[:, 4] = -al_n * np.expm1(-h)
    for i in range(S):
        first = order == 1 or i == S - 1 or (i == 0 and lower_order_final and S < 15)
        if first:
            tab[i, 5], tab[i, 6] = 1.0, 0.0
        else:
            r = h[i + 1] / h[i]
            tab[i, 5], tab[i, 6] = 1.0 + 0.5 / r, -0.5 / r
    return tab.astype(np.float32)


class DPMSolverSampler(DDIMSampler):
    """DPM-Solver++(2M) with classifier-free guidance; deterministic (eta = 0 only).

    RNG contract: the sampler draws from the device generator only for x_T (one latent-sized torch.randn, when neither
    x_info["xt"] nor x_info["x0"] is given; with "x0" and no "x0_noise", q_sample draws the forward noise instead) and
    nothing per step.  This differs from DDIMSampler, which also consumes one latent-sized draw per step as the reference
    does.  Graph capture / replay bookkeeping never leaks into the generator state."""
    coef_width = 8
    draws_step_noise = False

    def __init__(self, model, schedule="linear", order=2, lower_order_final=True, **kwargs):
        if order not in (1, 2):
            raise ValueError("DPMSolverSampler: order must be 1 or 2, got %r" % (order,))
        super().__init__(model, schedule=schedule, **kwargs)
        self.order = order
        self.lower_order_final = bool(lower_order_final)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0.:
            raise ValueError("DPMSolverSampler is deterministic: eta must be 0, got %r" % (ddim_eta,))
        super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=ddim_eta, verbose=verbose)

    def _ddim_sampling_multicontext(self, shape, x_info, c_info_list, noise_dropout, temperature, log_every_t, _single):
        if noise_dropout > 0.:
            raise ValueError("DPMSolverSampler is deterministic: noise_dropout must be 0, got %r" % (noise_dropout,))
        return super()._ddim_sampling_multicontext(shape, x_info, c_info_list, noise_dropout, temperature, log_every_t,
                                                   _single)

    def _coef_table(self, total_steps, scale, device):
        tab = dpmpp_coef_table(self.alphas_cumprod, self.ddim_timesteps[:total_steps], order=self.order,
                               lower_order_final=self.lower_order_final, scale=scale)
        return torch.from_numpy(tab).to(device)

    def _extra_static(self, x):
        return {"x0_hist": torch.empty(x.shape, device=x.device, dtype=torch.float32)}

    def _update_static(self, bufs, eps, guided):
        ops.cfg_dpmpp_step_dev(bufs["xs"], eps, bufs["coef"], bufs["x0_hist"], guided=guided, x_next=bufs["xs"],
                               pred_x0=bufs["p0"])
        if "mask" in bufs:      # inpainting: the history keeps the raw data prediction, only the latent is blended
            self._blend_static(bufs, bufs["xs"])

    def _step(self, *args, **kwargs):
        # the multistep update needs the history of the loop: there is no stand-alone single step (p_sample_ddim*)
        raise NotImplementedError("DPMSolverSampler runs whole sample() loops on the GPU; it has no single-step API")
