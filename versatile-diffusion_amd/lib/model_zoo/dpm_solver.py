"""DPM-Solver++(2M) sampler (Lu et al., "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic
Models", 2022, Algorithm 2) with classifier-free guidance, on DDIMSampler's static step loop.

`DPMSolverSampler(model).sample(steps, shape, x_info, c_info)` has DDIMSampler's arguments, dict protocol and return
values and runs every flow it runs (xt / x0 + x0_forward_timesteps / random x_T, the 0-D text latent, multi-context).  It
walks the same DDIM timestep grid; at 15-25 steps the multistep update gets close to what DDIM gives at 50.

The whole step -- UNet forward + ONE fused kernel for the CFG combine and the multistep update
(ops.cfg_dpmpp_step_dev) -- is captured once into a HIP graph and replayed, exactly like DDIM: the solver's only state is
an fp32 buffer holding the previous step's data prediction x0, and the per-step scalars are a row of the fp32[S, 8]
table of dpmpp_coef_table, copied into a device buffer between replays.

`DPMSolverSDESampler` is the stochastic variant (SDE-DPM-Solver++(2M) of the same paper; k-diffusion's dpmpp_2m_sde,
midpoint type, in the VP parameterisation) on the same graph: its noise is generated inside the update kernel
(ops.cfg_dpmpp_sde_step_dev) by a counter-based generator keyed by a per-sample seed (x_info["seeds"]), so the step stays
one fused launch, nothing is drawn from torch's generator, and a sample's noise does not depend on the batch it runs in.
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


def dpmpp_sde_coef_table(alphas_cumprod, timesteps, eta=1.0, s_noise=1.0, order=2, lower_order_final=True, scale=1.0):
    """fp32 [S, 8] rows {scale, 1/sqrt(a_t), sqrt(1-a_t), (sg_n/sg_t) exp(-eta h), -al_n expm1(-(1+eta) h), w_cur, w_prev,
    s_noise sg_n sqrt(-expm1(-2 eta h))} per DDIM index, computed in float64 (the layout vd_cfg_dpmpp_sde_step_dev_f16
    reads), in the notation of dpmpp_coef_table (al / sg of a_t and a_next, h, r; the same first- and second-order rows,
    the same ValueError for h <= 0):

        x_next = (sg_n/sg_t) exp(-eta h) x + al_n (1 - exp(-(1+eta) h)) D + s_noise sg_n sqrt(1 - exp(-2 eta h)) z

    with D = w_cur x0 + w_prev x0_prev as in 2M and z ~ N(0, I).  eta = 1 is SDE-DPM-Solver++(2M) (Lu et al. 2022;
    k-diffusion's dpmpp_2m_sde, midpoint type, carried to the VP parameterisation); eta = 0 is dpmpp_coef_table bit for
    bit (exp(-0 h) = 1 and (1 + 0) h = h are exact)."""
    eta, s_noise = float(eta), float(s_noise)
    if not eta >= 0.0:
        raise ValueError("DPM-Solver++ SDE: eta must be >= 0, got %r" % (eta,))
    tab = dpmpp_coef_table(alphas_cumprod, timesteps, order=order, lower_order_final=lower_order_final,
                           scale=scale).astype(np.float64)
    ts = np.asarray(timesteps)
    _, a_t, a_next = make_ddim_sampling_parameters(alphas_cumprod, ts, 0.0, verbose=False)
    a_t, a_next = np.asarray(a_t, np.float64), np.asarray(a_next, np.float64)
    al_t, sg_t = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    al_n, sg_n = np.sqrt(a_next), np.sqrt(1.0 - a_next)
    h = (np.log(al_n) - np.log(sg_n)) - (np.log(al_t) - np.log(sg_t))
    tab[:, 3] = (sg_n / sg_t) * np.exp(-eta * h)
    tab[:, 4] = -al_n * np.expm1(-(1.0 + eta) * h)
    tab[:, 7] = s_noise * sg_n * np.sqrt(np.abs(np.expm1(-2.0 * eta * h)))   # expm1 <= 0; abs also turns -0.0 into 0.0
    return tab.astype(np.float32)


def _check_seeds(seeds, batch):
    """x_info["seeds"] as a host int64 tensor [batch], validated: one seed per sample, each in [0, 2^63)."""
    if isinstance(seeds, torch.Tensor):
        if seeds.dtype != torch.int64 or seeds.dim() != 1:
            raise ValueError("x_info['seeds'] must be an int64 tensor of shape [B], got %s %s" % (seeds.dtype, tuple(seeds.shape)))
        vals = seeds.detach().cpu().tolist()
    else:
        vals = list(seeds)
    if len(vals) != batch:
        raise ValueError("x_info['seeds'] has %d entries, expected one per sample (%d)" % (len(vals), batch))
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("x_info['seeds'] must hold integers, got %r" % (v,))
        if not 0 <= int(v) < 2 ** 63:
            raise ValueError("x_info['seeds'] must lie in [0, 2^63), got %r" % (v,))
    return torch.tensor([int(v) for v in vals], dtype=torch.int64)


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

    def _solver_update(self, bufs, eps, guided):
        if "kfac" in bufs:      # guidance rescale: the factor kernel, then the update that multiplies by its factors
            self._rescale_static(bufs, eps)
            ops.cfg_dpmpp_step_dev_rs(bufs["xs"], eps, bufs["coef"], bufs["x0_hist"], bufs["kfac"], guided=guided,
                                      x_next=bufs["xs"], pred_x0=bufs["p0"])
        else:
            ops.cfg_dpmpp_step_dev(bufs["xs"], eps, bufs["coef"], bufs["x0_hist"], guided=guided, x_next=bufs["xs"],
                                   pred_x0=bufs["p0"])

    def _update_static(self, bufs, eps, guided):
        self._solver_update(bufs, eps, guided)
        if "mask" in bufs:      # inpainting: the history keeps the raw data prediction, only the latent is blended
            self._blend_static(bufs, bufs["xs"])

    def _step(self, *args, **kwargs):
        # the multistep update needs the history of the loop: there is no stand-alone single step (p_sample_ddim*)
        raise NotImplementedError("%s runs whole sample() loops on the GPU; it has no single-step API" % type(self).__name__)


class DPMSolverSDESampler(DPMSolverSampler):
    """SDE-DPM-Solver++(2M) with classifier-free guidance: DPMSolverSampler plus eta (1 = the SDE solver, 0 = 2M itself)
    and `temperature` as the noise scale s_noise; noise_dropout still raises.

    Noise contract: x_info["seeds"] (a sequence or int64 tensor, one seed in [0, 2^63) per sample; required when eta > 0)
    keys a counter-based generator (ops.philox_normal; layout in include/vd_hip.h).  Step noise is generated inside the
    update kernel (stream 2, draw = step number in sampling order), and with seeds present x_T (stream 0; when neither
    "xt" nor "x0" is given) and the forward-process noise (stream 1; "x0" without "x0_noise") come from the same
    generator.  The sampler then draws nothing from the device generator, and the noise a sample sees is bit-identical
    whatever batch, batch position, graph or rank it runs in."""

    def __init__(self, model, schedule="linear", order=2, lower_order_final=True, eta=1.0, **kwargs):
        if not float(eta) >= 0.:
            raise ValueError("DPMSolverSDESampler: eta must be >= 0, got %r" % (eta,))
        super().__init__(model, schedule=schedule, order=order, lower_order_final=lower_order_final, **kwargs)
        self.eta = float(eta)
        self._eta, self._s_noise, self._seeds = self.eta, 1.0, None

    @torch.no_grad()
    def sample(self, steps, shape, x_info, c_info, eta=None, temperature=1., noise_dropout=0., verbose=True,
               log_every_t=100):
        return super().sample(steps, shape, x_info, c_info, eta=self.eta if eta is None else eta, temperature=temperature,
                              noise_dropout=noise_dropout, verbose=verbose, log_every_t=log_every_t)

    @torch.no_grad()
    def sample_multicontext(self, steps, shape, x_info, c_info_list, eta=None, temperature=1., noise_dropout=0.,
                            verbose=True, log_every_t=100):
        return super().sample_multicontext(steps, shape, x_info, c_info_list, eta=self.eta if eta is None else eta,
                                           temperature=temperature, noise_dropout=noise_dropout, verbose=verbose,
                                           log_every_t=log_every_t)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if not float(ddim_eta) >= 0.:
            raise ValueError("DPMSolverSDESampler: eta must be >= 0, got %r" % (ddim_eta,))
        # eta belongs to the solver's own table; DDIM's sigmas stay 0, so the loop is the static one
        self._eta = float(ddim_eta)
        super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=0., verbose=verbose)

    def _ddim_sampling_multicontext(self, shape, x_info, c_info_list, noise_dropout, temperature, log_every_t, _single):
        # validated before anything touches the device
        if noise_dropout > 0.:
            raise ValueError("DPMSolverSDESampler has no noise dropout: noise_dropout must be 0, got %r" % (noise_dropout,))
        seeds = x_info.get("seeds")
        if seeds is None and self._eta > 0.:
            raise ValueError("DPMSolverSDESampler: eta = %r needs x_info['seeds'], one seed per sample" % (self._eta,))
        self._seeds = None if seeds is None else _check_seeds(seeds, int(shape[0]))
        self._s_noise = float(temperature)
        return super()._ddim_sampling_multicontext(shape, x_info, c_info_list, noise_dropout, temperature, log_every_t,
                                                   _single)

    def _start_latent(self, shape, x_info, masked, device, dtype):
        if self._seeds is None:
            return super()._start_latent(shape, x_info, masked, device, dtype)
        # what the base class would draw from the device generator comes from the seeded one instead
        xi, seeds = dict(x_info), self._seeds.to(device)
        if xi.get("xt") is None:
            if xi.get("x0") is not None and (not masked or xi.get("x0_forward_timesteps") is not None):
                if xi.get("x0_noise") is None:
                    xi["x0_noise"] = ops.philox_normal(seeds, shape, stream=1).to(dtype)
            else:
                xi["xt"] = ops.philox_normal(seeds, shape, stream=0).to(dtype)
        return super()._start_latent(shape, xi, masked, device, dtype)

    def _coef_table(self, total_steps, scale, device):
        tab = dpmpp_sde_coef_table(self.alphas_cumprod, self.ddim_timesteps[:total_steps], eta=self._eta,
                                   s_noise=self._s_noise, order=self.order, lower_order_final=self.lower_order_final,
                                   scale=scale)
        return torch.from_numpy(tab).to(device)

    def _rng_table(self, total_steps, device):
        # {draw, stream} per step in sampling order: the step noise is stream 2
        draws = np.stack([np.arange(total_steps), np.full((total_steps,), 2)], axis=1).astype(np.int32)
        return torch.from_numpy(draws).to(device)

    def _extra_static(self, x):
        return dict(super()._extra_static(x), seeds=torch.zeros((x.shape[0],), device=x.device, dtype=torch.int64),
                    rng=torch.zeros((2,), device=x.device, dtype=torch.int32))

    def _load_state(self, st, x, c_info_list, inpaint, phi=0., window=None, pag_w=None, sag=None, seg=None):
        if self._seeds is None:
            st["seeds"].zero_()          # eta = 0 without seeds: the noise coefficient is 0 and the seeds are not read
        else:
            st["seeds"].copy_(self._seeds)
        return super()._load_state(st, x, c_info_list, inpaint, phi, window, pag_w, sag, seg)

    def _solver_update(self, bufs, eps, guided):
        if "kfac" in bufs:
            self._rescale_static(bufs, eps)
            ops.cfg_dpmpp_sde_step_dev_rs(bufs["xs"], eps, bufs["coef"], bufs["x0_hist"], bufs["seeds"], bufs["rng"],
                                          bufs["kfac"], guided=guided, x_next=bufs["xs"], pred_x0=bufs["p0"])
        else:
            ops.cfg_dpmpp_sde_step_dev(bufs["xs"], eps, bufs["coef"], bufs["x0_hist"], bufs["seeds"], bufs["rng"],
                                       guided=guided, x_next=bufs["xs"], pred_x0=bufs["p0"])
