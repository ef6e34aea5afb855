"""DDIM sampler with the reference's API (lib/model_zoo/ddim.py:10-298 there): `DDIMSampler(model).sample(...)`
and `.sample_multicontext(...)` with the same arguments, dict protocol and return values.

What changed underneath: the CFG combine and the DDIM update are ONE elementwise kernel (the reference issues ~10
tiny kernels and three device->host syncs per step), the CFG-doubled context batch is assembled once instead of every
step, the step-invariant context K/V projections of all 16 cross-attention layers are computed once per sample() call,
and -- because every launch goes to torch's current stream with static shapes -- the whole step (UNet forward + update,
~450 kernel launches) is captured once into a HIP graph and replayed for the remaining steps; between replays the host
only refreshes a 6-float coefficient vector and the timestep tensor.  Set VD_DDIM_GRAPH=0 to run every step eagerly.
"""
import contextlib
import gc
import numbers
import os
import threading

import numpy as np
import torch

from vd_hip import ops

from . import windows
from .diffusion_utils import make_ddim_sampling_parameters, make_ddim_timesteps
from .vd import (DeepCache, _apg_arg, _freeu_arg, _hypertile_arg, _pag_arg, _sag_arg, _seg_arg, _tome_arg, capture_stream, deep_cut, kv_mark_stale, kv_refresh, kv_refreshable,
                 kv_rows, hypertile_blocks, sag_map_size, sag_taps, seg_taps, seg_workspace_elems, tome_blocks)


def inpaint_blend_table(alphas_cumprod, timesteps):
    """fp32 [S, 2] rows {ca, cn} of the inpainting blend (ops.masked_blend) per DDIM index i, computed in float64: after
    the step of index i lands on a_prev[i] (DDIM's alphas_prev, the DPM solver's a_next), the known region is reset to
    ca x0 + cn noise with (ca, cn) = (sqrt(a_prev[i]), sqrt(1 - a_prev[i])) for i > 0 and (1, 0) for i = 0, so the last
    step returns the known region as x0 itself."""
    _, _, a_prev = make_ddim_sampling_parameters(alphas_cumprod, np.asarray(timesteps), 0.0, verbose=False)
    a_prev = np.asarray(a_prev, dtype=np.float64)
    tab = np.stack([np.sqrt(a_prev), np.sqrt(1.0 - a_prev)], axis=1)
    tab[0] = (1.0, 0.0)
    return tab.astype(np.float32)


def _inpaint_args(x_info, shape):
    """Whether x_info asks for inpainting, after validating its extension keys (inpaint_mask, x0) against the latent shape.
    Runs before anything touches the device."""
    mask = x_info.get("inpaint_mask")
    if mask is None:
        return False
    if x_info.get("type") != "image":
        raise ValueError("inpaint_mask applies to x_info['type'] == 'image' only, got %r" % (x_info.get("type"),))
    x0 = x_info.get("x0")
    if x0 is None:
        raise ValueError("inpaint_mask needs x_info['x0'], the encoded image")
    shape = tuple(int(s) for s in shape)
    if len(shape) != 4 or tuple(x0.shape) != shape:
        raise ValueError("inpainting: x0 has shape %s, expected the latent shape %s" % (tuple(x0.shape), shape))
    if mask.dim() != 4 or mask.shape[1] != 1 or tuple(mask.shape[2:]) != shape[2:]:
        raise ValueError("inpaint_mask has shape %s, expected [B or 1, 1, %d, %d]" % ((tuple(mask.shape),) + shape[2:]))
    if mask.shape[0] not in (1, shape[0]):
        raise ValueError("inpaint_mask has batch %d, expected 1 or %d" % (mask.shape[0], shape[0]))
    return True


def _cache_args(x_info, model):
    """(interval N, depth k) of DeepCache sampling from x_info's extension keys cache_interval (an int >= 1, default 1 = off) and
    cache_depth (an int in [1, n - 1] for the n skips of the data net, default 1; vd.deep_cut), validated: ValueError for
    anything else, and for N > 1 on a flow other than the 2-D image flow.  Step i of a call (sampling order, 0 = the first step
    the call runs) is a full forward that stores the deep feature iff i % N == 0; the others reuse it.  Touches no device."""
    N, k = x_info.get("cache_interval", 1), x_info.get("cache_depth", 1)
    for name, v in (("cache_interval", N), ("cache_depth", k)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("x_info[%r] must be an int >= 1, got %r" % (name, v))
    N, k = int(N), int(k)
    if N > 1 and x_info.get("type") != "image":
        raise ValueError("cache_interval > 1 applies to x_info['type'] == 'image' only, got %r" % (x_info.get("type"),))
    if x_info.get("type") == "image" and (N > 1 or k > 1):
        deep_cut(model.diffuser[x_info["type"]], k)        # raises for a depth out of range
    return N, k


def _window_args(x_info, shape, model):
    """The plan of a windowed (MultiDiffusion) call from x_info's extension keys, or None: `window` (an int or (h, w) in latent
    pixels; absent = off), `window_stride` (an int or a pair, default half the window per axis), `window_wrap` (bool, default
    False: the x axis wraps around, a 360-degree panorama), `window_weight` ('uniform', the default, 'gaussian' or 'tent') and
    `window_batch` (an int >= 1, default 8: the most windows per sample in one UNet forward).  Validated with the tables of
    lib/model_zoo/windows.py: ValueError for a bad value of any key and for a flow other than the 2-D image flow.  None also
    when the plan has a single window (window == canvas): that call is the plain call and gives its bits.  The plan: the
    geometry "key" (h, w, sy, sx, wrap, weight, nc, m), "n" windows run as "nc" forwards of "m" slots per sample, "offsets"
    int32 [nc, m, 2] (the unused slots of the last forward repeat the last window), "wgt" fp32 [h, w] and "inv_den" fp32
    [H, W].
    `region_masks` (regional prompts; real or bool [R, H, W] or [R, 1, H, W] on the canvas latent grid, values in [0, 1], shared
    by the samples; windows.region_masks_arg) needs `window` and the image flow.  The plan is then built also for a single window
    and holds "regions" R, "masks" fp32 [R, H, W] and as "inv_den" windows.region_inv_den; its key carries R as a ninth entry.
    Touches no device (but reads masks given as a device tensor)."""
    window, masks = x_info.get("window"), x_info.get("region_masks")
    if masks is not None and x_info.get("type") != "image":
        raise ValueError("region_masks applies to x_info['type'] == 'image' only, got %r" % (x_info.get("type"),))
    if masks is not None and window is None:
        raise ValueError("region_masks needs x_info['window'] (pass the canvas size for a plain image)")
    if window is None:
        return None
    if x_info.get("type") != "image":
        raise ValueError("window applies to x_info['type'] == 'image' only, got %r" % (x_info.get("type"),))
    shape = tuple(int(s) for s in shape)
    if len(shape) != 4:
        raise ValueError("window: the latent shape must be [B, C, H, W], got %s" % (shape,))
    H, W = shape[2:]
    h, w = windows.int_pair("window", window)
    stride = x_info.get("window_stride")
    sy, sx = (max(h // 2, 1), max(w // 2, 1)) if stride is None else windows.int_pair("window_stride", stride)
    wrap, weight = x_info.get("window_wrap", False), x_info.get("window_weight", "uniform")
    from .openaimodel import Downsample
    factor = 2 ** sum(isinstance(mod, Downsample) for mod in model.diffuser[x_info["type"]].modules())
    offsets = windows.window_offsets(H, W, (h, w), (sy, sx), wrap, multiple=factor)
    wgt = windows.window_weights(h, w, weight)
    n = offsets.shape[0]
    nc, m = windows.window_chunks(n, x_info.get("window_batch", 8))
    if masks is not None:
        if torch.is_tensor(masks):
            masks = masks.detach().cpu()
            masks = (masks if masks.dtype == torch.bool else masks.float()).numpy()
        masks = windows.region_masks_arg(masks, H, W)
    elif n == 1:
        return None
    padded = np.concatenate([offsets, np.repeat(offsets[-1:], nc * m - n, axis=0)]).reshape(nc, m, 2)
    plan = {"key": (h, w, sy, sx, bool(wrap), weight, nc, m), "n": n, "nc": nc, "m": m, "offsets": np.ascontiguousarray(padded),
            "wgt": wgt}
    if masks is None:
        plan["inv_den"] = windows.window_inv_den(H, W, offsets, wgt, bool(wrap))
    else:
        plan.update(key=plan["key"] + (masks.shape[0],), regions=masks.shape[0], masks=masks,
                    inv_den=windows.region_inv_den(H, W, offsets, wgt, masks, bool(wrap)))
    return plan


def _region_contexts(c_info_list, window, batch):
    """The context list a regional-prompt call works on: region-major, R x len(c_info_list) shallow copies whose 'conditioning'
    is region r's tensor -- entry r of a list or tuple of R tensors [B, L, D], or the context's plain tensor, shared by all
    regions (each context decides for itself).  Without region masks (the plan has no "regions") the list comes back as it is,
    and a conditioning list raises.  ValueError for a list of another length than R, entries whose shapes differ and a batch
    other than `batch`.  Touches no device."""
    R = None if window is None else window.get("regions")
    for ci in c_info_list:
        cond = ci.get("conditioning")
        if not isinstance(cond, (list, tuple)):
            continue
        if R is None:
            raise ValueError("a list of conditionings (one per region) needs x_info['region_masks']")
        if len(cond) != R:
            raise ValueError("the conditioning list has %d entries for %d region_masks" % (len(cond), R))
        shapes = [tuple(c.shape) for c in cond]
        if any(sh != shapes[0] for sh in shapes):
            raise ValueError("the regions' conditionings differ in shape: %r" % (shapes,))
        if len(shapes[0]) != 3 or shapes[0][0] != int(batch):
            raise ValueError("a region's conditioning has shape %s, expected [%d, L, D]" % (shapes[0], int(batch)))
    if R is None:
        return c_info_list
    return [dict(ci, conditioning=ci["conditioning"][r] if isinstance(ci["conditioning"], (list, tuple)) else ci["conditioning"])
            for r in range(R) for ci in c_info_list]


def cfg_guided_eps(eps, scale):
    """float64 [B, ...]: the guided prediction eg = fmaf(s, ec - eu, eu) of eps = [e_uncond ; e_cond] ([2B, ...]) as the fused
    updates form it in fp32 -- the difference rounded to fp32, the guidance scale rounded to fp32, the product-sum rounded to
    fp32 once (formed in float64, where the product of two fp32 values is exact)."""
    eu, ec = eps.detach().float().chunk(2)
    s = float(np.float32(scale))
    return (s * (ec - eu).double() + eu.double()).float().double()


def cfg_rescale_factors(eps, scale, phi):
    """float64 [B]: the guidance-rescale factors of eps = [e_uncond ; e_cond] ([2B, ...]) before their rounding to fp32, a plain
    torch statement of the contract in include/vd_hip.h (Lin et al. 2023, section 3.4; diffusers' guidance_rescale):

        eg = cfg_guided_eps(eps, scale);  V(v) = sum v^2 - (sum v)^2 / m  over the sample's m elements, in float64
        r = sqrt(max(V(ec), 0) / V(eg)), or 1 if V(eg) <= 0, m == 1 or r is not finite;  k = phi r + (1 - phi)

    with phi rounded to fp32 first (the samplers keep it in an fp32 device buffer).  The kernel's factor
    (ops.cfg_rescale_factor, intermediates['guidance_rescale']) is k.float(); the update then uses e' = k eg in place of eg."""
    ec = eps.detach().float().chunk(2)[1].double().flatten(1)
    eg = cfg_guided_eps(eps, scale).flatten(1)
    m = ec.shape[1]
    var = lambda v: (v * v).sum(1) - v.sum(1) ** 2 / m
    vc, vg = var(ec), var(eg)
    ok = vg > 0 if m > 1 else torch.zeros_like(vg, dtype=torch.bool)
    r = torch.sqrt(vc.clamp(min=0) / torch.where(ok, vg, torch.ones_like(vg)))
    r = torch.where(ok & torch.isfinite(r), r, torch.ones_like(r))
    p = float(np.float32(phi))
    return p * r + (1.0 - p)


def _rescale_arg(c_info_list):
    """The contexts' 'guidance_rescale' (extension key, default 0 = off) as a float, validated: ValueError unless it is a real
    number in [0, 1] that all contexts of the call agree on.  Touches no device."""
    phis = []
    for ci in c_info_list:
        value = ci.get("guidance_rescale", 0.)
        if isinstance(value, bool) or not isinstance(value, numbers.Real) or not 0. <= float(value) <= 1.:
            raise ValueError("c_info['guidance_rescale'] must be a real number in [0, 1], got %r" % (value,))
        phis.append(float(value))
    if any(p != phis[0] for p in phis):
        raise ValueError("A different guidance_rescale between different context is not allowed, got %r" % (phis,))
    return phis[0]


def replica_count(guided, pag):
    """How many replicas of the latent batch the UNet sees in a step: 1 unguided, 2 under classifier-free guidance ([uncond ;
    cond]) or unguided with perturbed-attention guidance ([cond ; perturbed]), 3 with both ([uncond ; cond ; perturbed])."""
    return (2 if guided else 1) + (1 if pag else 0)


def pag_weight(scale, pag_scale, guided):
    """The fp32 weight ops.pag_fold reads (vd_pag_fold_f16, include/vd_hip.h), formed in float64 and rounded once.  Guided: the
    fold rewrites e_u to a' = e_u + w (e_c - e_p) with w = -s_pag / (s - 1), so the update's a' + s (e_c - a') is
    e_u + s (e_c - e_u) + s_pag (e_c - e_p).  Unguided: e_c + s_pag (e_c - e_p), w = s_pag."""
    if guided:
        return np.float32(-np.float64(pag_scale) / (np.float64(scale) - 1.0))
    return np.float32(np.float64(pag_scale))


def sag_weight(scale, sag_scale, guided):
    """The fp32 weight ops.sag_fold reads (vd_sag_fold_f16, include/vd_hip.h), formed in float64 and rounded once.  Guided: the fold
    rewrites e_u to a' = e_u + w (e_u - e_d) with w = -s_sag / (s - 1), so the update's a' + s (e_c - a') is
    e_u + s (e_c - e_u) + s_sag (e_u - e_d).  Unguided: e_c + s_sag (e_c - e_d), w = s_sag."""
    if guided:
        return np.float32(-np.float64(sag_scale) / (np.float64(scale) - 1.0))
    return np.float32(np.float64(sag_scale))


def sag_coef_table(alphas_cumprod, timesteps):
    """fp32 [S, 3] rows {sqrt(a_t), sqrt(1 - a_t), 1 / sqrt(a_t)} of ops.sag_degrade per DDIM index i, a_t = alphas_cumprod[timesteps[i]],
    computed in float64: the data prediction and the re-noising of a self-attention-guidance step (diffusers' pred_x0 / add_noise)."""
    a = np.asarray(alphas_cumprod, dtype=np.float64)[np.asarray(timesteps, dtype=np.int64)]
    return np.stack([np.sqrt(a), np.sqrt(1.0 - a), 1.0 / np.sqrt(a)], axis=1).astype(np.float32)


def sag_ratios(c_info_list):
    """fp32 [T]: the normalised ratios vd.run_unet mixes the context types with (float64 r / sum r, rounded once)."""
    r = np.array([float(ci.get("ratio", 1.0)) for ci in c_info_list], dtype=np.float64)
    return (r / r.sum()).astype(np.float32)


def apg_coef_table(alphas_cumprod, timesteps, eta, r, beta):
    """fp32 [S, 8] rows {s1, isa, 1 / g, beta_eff, r, 1 - eta, 0, 0} of ops.apg_fold per DDIM index i (the row the loops copy next
    to their coefficient row), a_t = alphas_cumprod[timesteps[i]], s1 = sqrt(1 - a_t), isa = 1 / sqrt(a_t), g = s1 isa, every entry
    formed in float64 and rounded once.  `timesteps` are the steps THIS call runs (a start from x_info['xt'] or
    ['x0_forward_timesteps'] runs the leading ones only): the loops walk the indices downwards, so the row of the first step a call
    runs is the LAST one, and it has beta_eff = 0 -- the running direction starts there and the state is not read; every other
    row has beta_eff = beta."""
    a = np.asarray(alphas_cumprod, dtype=np.float64)[np.asarray(timesteps, dtype=np.int64)]
    s1, isa = np.sqrt(1.0 - a), 1.0 / np.sqrt(a)
    tab = np.zeros((a.shape[0], 8), dtype=np.float64)
    tab[:, 0], tab[:, 1], tab[:, 2] = s1, isa, 1.0 / (s1 * isa)
    tab[:, 3], tab[:, 4], tab[:, 5] = float(beta), float(r), 1.0 - float(eta)
    if a.shape[0]:
        tab[-1, 3] = 0.0
    return tab.astype(np.float32)


def apg_guided_eps(x, eps, v_prev, row):
    """The float64 statement of adaptive projected guidance (Sadat et al. 2024, Algorithm 1, written for an epsilon model; the
    contract of vd_apg_fold_f16 in include/vd_hip.h without its roundings).  x [B, ...] the latent, eps = [e_uncond ; e_cond]
    ([2B, ...]), v_prev [B, ...] the running direction of the step before (None, or anything when row[3] == 0: not read), row the
    step's {s1, isa, 1 / g, beta_eff, r, 1 - eta, ...} (apg_coef_table).  Per sample, with g = s1 isa and sums over its elements:

        D_c = (x - s1 e_c) isa;  dD = -g (e_c - e_u);  v = dD + beta_eff v_prev
        k = min(1, r / ||v||), 1 if r == 0 or ||v|| == 0;  p = k <v, D_c> / <D_c, D_c>, 0 if <D_c, D_c> == 0;  q = (1 - eta) p
        n = k v - q D_c;  e_u' = e_c + n row[2]

    Returns (e_u' [B, ...], v [B, ...], fac [B, 4] = {||v||, k, p, ||D_c||}), all float64.  The update's e_u' + s (e_c - e_u') is
    e_c - (s - 1) n / g, the epsilon form of D_c + (s - 1) n; (eta, r, beta) = (1, 0, 0) returns e_u."""
    s1, isa, ig, beta, r, ome = [float(v) for v in list(row)[:6]]
    eu, ec = eps.detach().double().chunk(2)
    x = x.detach().double()
    g = s1 * isa
    D = (x - s1 * ec) * isa
    v = -g * (ec - eu)
    if beta != 0.:
        v = v + beta * v_prev.detach().double()
    dot = lambda a, b: (a * b).flatten(1).sum(1)
    svv, svd, sdd = dot(v, v), dot(v, D), dot(D, D)
    nv, one = torch.sqrt(svv), torch.ones_like(svv)
    k = torch.where(nv > 0, (r / torch.where(nv > 0, nv, one)).clamp(max=1.0), one) if r != 0. else one
    p = torch.where(sdd > 0, k * svd / torch.where(sdd > 0, sdd, one), torch.zeros_like(sdd))
    col = lambda t: t.view(-1, *([1] * (x.dim() - 1)))
    n = col(k) * v - col(ome * p) * D
    return ec + n * ig, v, torch.stack([nv, k, p, torch.sqrt(sdd)], dim=1)


_gc_lock = threading.Lock()
_gc_holds = [0, False]      # captures in progress in this process; whether the collector was on when the first began


@contextlib.contextmanager
def _no_gc():
    """Python's cyclic collector stays off while a step is being captured, in any thread: a collection that frees a dropped
    sampler's kept graph runs torch's graph destructor, which synchronises the device -- not allowed while a stream is
    capturing, and an error thrown from a destructor ends the process.  The collector's setting is process-wide, so captures
    are counted: the first switches it off, the last restores it.  Garbage made meanwhile waits for the next collection."""
    with _gc_lock:
        if _gc_holds[0] == 0:
            _gc_holds[1] = gc.isenabled()
            gc.disable()
        _gc_holds[0] += 1
    try:
        yield
    finally:
        with _gc_lock:
            _gc_holds[0] -= 1
            if _gc_holds[0] == 0 and _gc_holds[1]:
                gc.enable()


class DDIMSampler(object):
    # hooks of the static step loop (_loop_static) for samplers that share it (dpm_solver.DPMSolverSampler): the width of
    # the per-step device coefficient row, and whether every step draws its reference noise_like(x) from the generator
    coef_width = 6
    draws_step_noise = True

    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.use_graph = os.environ.get("VD_DDIM_GRAPH", "1") != "0"
        self.graph_cache = os.environ.get("VD_DDIM_GRAPH_CACHE", "1") != "0"   # keep captured steps across sample() calls
        self.replay_first = os.environ.get("VD_DDIM_REPLAY_FIRST", "1") != "0"   # with a kept graph step 0 is replayed too
        # the t-only part of the UNet (time-embedding MLP + every ResBlock's emb_layers projection) for all steps at once,
        # outside the step graph (VD_v2_0.precompute_step_emb); 0 = recompute it inside every step like the reference
        self.emb_hoist = os.environ.get("VD_EMB_HOIST", "1") != "0"
        self._static = {}
        # one request at a time per sampler: the kept step graphs read and write static buffers (the reference's sampler is
        # not re-entrant either, but it has no captured state to corrupt; app.py runs Gradio workers unlocked)
        self._lock = threading.RLock()

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def release_graphs(self):
        """Drop the kept step graphs with their static latent / context / K-V buffers (and the kept deep feature of DeepCache
        sampling, the tables and buffers of windowed sampling) and private memory pools (up to two
        geometries are kept alive per sampler; at 768x768, batch 32 that is a sizeable HBM reservation).  The next
        sample() call captures again.  Serialised with running sample() calls by the sampler's lock."""
        with self._lock:
            self._static.clear()

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize,
                                                  num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps, verbose=verbose)
        if hasattr(self.model, "host_schedule"):
            alphas_cumprod = self.model.host_schedule("alphas_cumprod")
        else:
            alphas_cumprod = self.model.alphas_cumprod.detach().float().cpu().numpy()
        assert alphas_cumprod.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        self.alphas_cumprod = alphas_cumprod
        sigmas, alphas, alphas_prev = make_ddim_sampling_parameters(
            alphacums=alphas_cumprod, ddim_timesteps=self.ddim_timesteps, eta=ddim_eta, verbose=verbose)
        self.ddim_sigmas = np.asarray(sigmas, dtype=np.float32)
        self.ddim_alphas = np.asarray(alphas, dtype=np.float32)
        self.ddim_alphas_prev = np.asarray(alphas_prev, dtype=np.float64)
        self.ddim_sqrt_one_minus_alphas = np.sqrt(np.float32(1.) - self.ddim_alphas)

    # ---- entry points (single context = a list of one, `single` picks apply_model) ---------------------
    @torch.no_grad()
    def sample(self, steps, shape, x_info, c_info, eta=0., temperature=1., noise_dropout=0., verbose=True,
               log_every_t=100):
        return self._run(shape, x_info, [c_info], noise_dropout, temperature, log_every_t, True, (steps, eta, verbose))

    @torch.no_grad()
    def ddim_sampling(self, shape, x_info, c_info, noise_dropout=0., temperature=1., log_every_t=100):
        return self._run(shape, x_info, [c_info], noise_dropout, temperature, log_every_t, True)

    @torch.no_grad()
    def sample_multicontext(self, steps, shape, x_info, c_info_list, eta=0., temperature=1., noise_dropout=0.,
                            verbose=True, log_every_t=100):
        return self._run(shape, x_info, c_info_list, noise_dropout, temperature, log_every_t, False, (steps, eta, verbose))

    @torch.no_grad()
    def ddim_sampling_multicontext(self, shape, x_info, c_info_list, noise_dropout=0., temperature=1.,
                                   log_every_t=100, _single=False):
        return self._run(shape, x_info, c_info_list, noise_dropout, temperature, log_every_t, _single)

    def _run(self, shape, x_info, c_info_list, noise_dropout, temperature, log_every_t, single, schedule=None):
        """The body of the four entry points; schedule = (steps, eta, verbose) of sample*(), which set the schedule first."""
        with self._lock:   # the schedule attributes and the kept step graphs are per-sampler state
            if schedule is not None:
                steps, eta, verbose = schedule
                self.make_schedule(ddim_num_steps=steps, ddim_eta=eta, verbose=verbose)
                if verbose:
                    print("Data shape for DDIM sampling is {}, eta {}".format(shape, eta))
            return self._ddim_sampling_multicontext(shape, x_info, c_info_list, noise_dropout, temperature, log_every_t, single)

    def _ddim_sampling_multicontext(self, shape, x_info, c_info_list, noise_dropout, temperature, log_every_t, _single):
        _freeu_arg(x_info)      # x_info['freeu'] (extension key, vd.freeu_setting): a bad value raises before anything is drawn
        masked = _inpaint_args(x_info, shape)
        interval, depth = _cache_args(x_info, self.model)
        window = _window_args(x_info, shape, self.model)
        if window is not None and interval > 1:
            raise ValueError("cache_interval > 1 does not combine with window: DeepCache would keep one feature per chunk of windows")
        # x_info['pag_scale'] / ['pag_layers'] (extension keys, vd._pag_arg): None, or (s_pag, layers); raises like the others
        pag = _pag_arg(x_info, self.model)
        # x_info['seg_scale'] / ['seg_blur_sigma'] / ['seg_layers'] (extension keys, vd._seg_arg): None, or (s_seg, layers, sigma);
        # raises like the others.  Smoothed energy guidance IS the perturbed replica of pag with another perturbation (and never in
        # the same call), so from here on `pag` is whichever is on: (scale, layers) or (scale, layers, sigma)
        seg = _seg_arg(x_info, self.model, shape)
        if seg is not None:
            pag = seg
        # x_info['tome_ratio'] / ['tome_max_downsample'] (extension keys, vd._tome_arg): None, or the TokenMerge; raises like the
        # others.  The setting travels with every forward (_eps), like FreeU's
        tome = _tome_arg(x_info, self.model, shape)
        # x_info['hypertile'] / ['hypertile_max_downsample'] (extension keys, vd._hypertile_arg): None, or the HyperTile; raises like
        # the others.  It travels with every forward too (_eps)
        hypertile = _hypertile_arg(x_info, self.model, shape)
        # x_info['sag_scale'] / ['sag_blur_sigma'] (extension keys, vd._sag_arg): None, or (s_sag, sigma); raises like the others
        sag = _sag_arg(x_info, self.model, shape)
        # x_info['apg_eta'] / ['apg_norm_threshold'] / ['apg_momentum'] (extension keys, vd._apg_arg): None, or (eta, r, beta);
        # raises like the others
        apg = _apg_arg(x_info)
        # regional prompts: from here on the contexts are the flat region-major list, one conditioning tensor each
        c_info_list = _region_contexts(c_info_list, window, shape[0])
        # CFG batch [uncond ; cond] assembled ONCE; K/V projections of it cached for the whole loop.  First, so that a bad
        # guidance_rescale raises like a bad mask: before anything is drawn
        device = self.model.device
        c_info_list, guided, scale, phi = self._cfg_contexts(c_info_list, 1 if window is None else window["m"], pag is not None)
        if not guided:
            apg = None      # there is no guidance direction to project: an unguided call ignores the keys, like the rescale
        dtype = c_info_list[0]["conditioning"].dtype
        x_info["x"], timesteps, blend_noise = self._start_latent(shape, x_info, masked, device, dtype)
        inpaint = None
        if masked:
            # blended latent diffusion: one fixed noise for the whole call (x0_noise, else the start q_sample's, else x_T)
            f16 = dict(device=device, dtype=torch.float16)
            inpaint = {"x0": x_info["x0"].to(**f16).contiguous(), "mask": x_info["inpaint_mask"].to(**f16).contiguous(),
                       "noise": blend_noise.to(**f16).contiguous(),
                       "table": torch.from_numpy(inpaint_blend_table(self.alphas_cumprod, timesteps)).to(device)}

        total_steps = timesteps.shape[0]
        x = x_info["x"].to(torch.float16).contiguous()
        eta_zero = bool(np.all(self.ddim_sigmas[:total_steps] == 0.))
        # noise_dropout > 0 (reference ddim.py:167-169 / :294-296: F.dropout on the step noise) draws a mask from the device
        # generator on every step, between the noise draws: that order only exists in the eager loop
        if x.is_cuda and eta_zero and total_steps > 0 and not noise_dropout > 0.:
            x, intermediates = self._loop_static(x, x_info, c_info_list, timesteps, guided, scale, _single, log_every_t, dtype,
                                                 inpaint, phi, interval, depth, window, pag, sag, apg)
        else:
            intermediates = {"pred_xt": [], "pred_x0": []}
            apg_step = None
            if apg is not None:     # per-call buffers; row `index` of the table is the step's coefficient row
                apg_step = {"v": torch.empty(x.shape, device=x.device, dtype=torch.float32),
                            "tab": torch.from_numpy(apg_coef_table(self.alphas_cumprod, timesteps, *apg)).to(x.device),
                            "fac": torch.empty((x.shape[0], 4), device=x.device, dtype=torch.float32)}
                intermediates["apg"] = []
            deep = DeepCache(depth) if interval > 1 else None
            wstate = None if window is None else self._window_state(window, x, guided, pag is not None)      # once per call
            pag_step = None if pag is None else (self._pert_fwd(pag, x.device),
                                                 torch.full((1,), float(pag_weight(scale, pag[0], guided)),
                                                            device=x.device, dtype=torch.float32))
            sag_step = None if sag is None else self._sag_eager(sag, scale, guided, c_info_list, x)
            if phi > 0.:
                intermediates["guidance_rescale"] = []
            for ci in c_info_list:
                ci["kv_cache"] = {}
            rescale = self._rescale_scalars(scale, phi, x.device)         # once per call, not per step
            for i, step in enumerate(np.flip(timesteps)):
                index = total_steps - i - 1
                x, pred_x0, kfac = self._step(x, x_info, c_info_list, int(step), index, guided, scale, temperature, _single,
                                              noise_dropout=noise_dropout, rescale=rescale,
                                              deep=None if deep is None else (deep, "store" if i % interval == 0 else "reuse"),
                                              window=wstate, pag=pag_step, sag=sag_step,
                                              apg=None if apg_step is None else (apg_step["v"], apg_step["tab"][index], apg_step["fac"]))
                if inpaint is not None:
                    ops.masked_blend(x, inpaint["x0"], inpaint["noise"], inpaint["mask"], inpaint["table"][index], out=x)
                if index % log_every_t == 0 or index == total_steps - 1:
                    intermediates["pred_xt"].append(x.to(dtype))
                    intermediates["pred_x0"].append(pred_x0.to(dtype))
                    if kfac is not None:
                        intermediates["guidance_rescale"].append(kfac)
                    if apg_step is not None:
                        intermediates["apg"].append(apg_step["fac"].clone())
        if interval > 1:
            intermediates["cache_full_steps"] = list(range(0, total_steps, interval))
        if pag is not None:
            intermediates["pag_layers" if seg is None else "seg_layers"] = pag[1]
        if sag is not None:
            intermediates["sag_map"] = sag_map_size(self.model.diffuser[x_info["type"]], x.shape[2], x.shape[3])
        if tome is not None:
            th, tw = (x.shape[2], x.shape[3]) if window is None else window["key"][:2]
            intermediates["tome_tokens"] = [(H * W, H * W - r) for _, H, W, r in
                                            tome_blocks(self.model.diffuser[x_info["type"]], th, tw, tome)]
        if hypertile is not None:
            th, tw = (x.shape[2], x.shape[3]) if window is None else window["key"][:2]
            intermediates["hypertile_tiles"] = [(H * W, nty * ntx) for _, H, W, nty, ntx in
                                                hypertile_blocks(self.model.diffuser[x_info["type"]], th, tw, hypertile)]
        x_info["x"] = x.to(dtype)
        return x_info["x"], intermediates

    def _start_latent(self, shape, x_info, masked, device, dtype):
        """(x, timesteps, blend_noise) of a call: the latent the loop starts from -- x_info["xt"], else x_info["x0"] diffused to
        step x0_forward_timesteps of the schedule (which then ends there), else random x_T -- and the fixed noise an inpainting
        call blends with.  A masked call draws from the generator exactly what the unmasked call draws."""
        timesteps = self.ddim_timesteps
        noise = x_info.get("x0_noise")   # extension: inject the forward-process noise instead of drawing it, for reproducible runs
        if x_info.get("xt") is not None:
            x = x_info["xt"].to(device=device, dtype=dtype)
        elif x_info.get("x0") is not None and (not masked or x_info.get("x0_forward_timesteps") is not None):
            x0 = x_info["x0"].to(device=device, dtype=dtype)
            k = x_info["x0_forward_timesteps"]
            ts = torch.full((shape[0],), int(timesteps[k]), device=device, dtype=torch.long)
            timesteps = timesteps[:k]
            if masked and noise is None:
                # the draw q_sample would make (same generator use as the unmasked call); the blend reuses it
                noise = torch.randn_like(x0)
            x = self.model.q_sample(x0, ts, noise=noise)
        else:
            x = torch.randn(shape, device=device, dtype=dtype)
        return x, timesteps, x if noise is None else noise

    def _cfg_contexts(self, c_info_list, slots=1, pag=False):
        """(copies, guided, scale, phi): shallow copies of the contexts with 'c', the batch the UNet sees ([uncond ; cond] under
        guidance), on the model's device.  The samplers work on the copies: 'c' (possibly a static buffer the captured graph
        reads) and 'kv_cache' never appear in the caller's dicts.  phi = c_info['guidance_rescale'] (extension key, default
        0 = off; cfg_rescale_factors): ValueError unless it is a real number in [0, 1] that all contexts agree on; an unguided
        call (scale == 1) ignores it, phi = 0.  slots > 1 (windowed sampling, the plan's m): the UNet's batch order is
        (replica, sample, window slot), so every row is repeated `slots` times in place.
        pag (perturbed-attention guidance): one more replica at the end, [uncond ; cond ; perturbed] or [cond ; perturbed]; the
        perturbed replica carries the conditional context, which therefore appears twice."""
        scale = c_info_list[0]["unconditional_guidance_scale"]
        for ci in c_info_list:
            assert ci["unconditional_guidance_scale"] == scale, \
                "A different unconditional guidance scale between different context is not allowed!"
        phi = _rescale_arg(c_info_list)
        guided = scale != 1.
        if not guided:
            phi = 0.
        copies = [dict(ci) for ci in c_info_list]
        for ci in copies:
            parts = [ci["unconditional_conditioning"], ci["conditioning"]] if guided else [ci["conditioning"]]
            if pag:
                parts.append(ci["conditioning"])
            if slots > 1:
                parts = [p.repeat_interleave(slots, 0) for p in parts]
            c = torch.cat(parts) if len(parts) > 1 else parts[0]
            ci["c"] = c.to(self.model.device)
        return copies, guided, scale, phi

    @staticmethod
    def _window_state(plan, x, guided, pag=False):
        """The device side of a windowed call's plan (_window_args) for the canvas latent x [B, C, H, W]: the tables "offs"
        (int32 [nc, m, 2]), "wgt", "inv_den", and the buffers "win" (fp16 [B, m, C, h, w], the UNet's input), "acc" (fp32
        canvas, only with several forwards per step) and "eps" (fp16 [R B, C, H, W], what _eps returns; R = replica_count(guided,
        pag), so with perturbed-attention guidance the canvas prediction has a perturbed replica too).  With regions also
        "rmask" (fp32 [R, H, W]); "rmask" and "inv_den" are then buffers that _load_state refills per call.  Lives in the static
        state entry, or for one call of the eager loop."""
        h, w = plan["key"][:2]
        B, C, H, W = x.shape
        rb = replica_count(guided, pag) * B
        dev = dict(device=x.device)
        ws = {"plan": plan, "offs": torch.from_numpy(plan["offsets"]).to(**dev), "wgt": torch.from_numpy(plan["wgt"]).to(**dev),
              "inv_den": torch.from_numpy(plan["inv_den"]).to(**dev),
              "win": torch.empty((B, plan["m"], C, h, w), dtype=torch.float16, **dev),
              "acc": torch.empty((rb, C, H, W), dtype=torch.float32, **dev) if plan["nc"] * plan.get("regions", 1) > 1 else None,
              "eps": torch.empty((rb, C, H, W), dtype=torch.float16, **dev)}
        if "regions" in plan:
            ws["rmask"] = torch.from_numpy(plan["masks"]).to(**dev)
        return ws

    def _eps_windowed(self, x_info, x, t, c_info_list, guided, single, emb_rows, ws, pag=None):
        """The canvas prediction [R B, C, H, W] of a windowed step: per chunk of the plan, in order, ops.window_gather of the
        latent's windows, the UNet on them as a batch of B m samples (t and the contexts carry R B m rows, order (r, b, k)),
        and ops.window_merge of what it predicts -- a sum in ascending window order, so the chunking does not decide a bit.
        With regions (regional prompts) c_info_list is the region-major list of _region_contexts: the chunks run once per region
        with that region's slice of the contexts, and ops.window_merge_masked fuses them with the region's mask, region-major."""
        plan = ws["plan"]
        (h, w, _, _, wrap), nc, m = plan["key"][:5], plan["nc"], plan["m"]
        x = x.to(torch.float16).contiguous()
        B, C, H, W = x.shape
        R = plan.get("regions")
        if R is not None:
            per = len(c_info_list) // R
            assert per * R == len(c_info_list), "the context list is not region-major"
            for r in range(R):
                for k in range(nc):
                    ops.window_gather(x, ws["offs"][k], h, w, wrap, out=ws["win"])
                    e = self._eps(x_info, ws["win"].view(B * m, C, h, w), t, c_info_list[r * per:(r + 1) * per], guided, single,
                                  emb_rows, pag=pag)
                    ops.window_merge_masked(e.to(torch.float16).contiguous().view(-1, m, C, h, w), ws["offs"][k], ws["wgt"],
                                            ws["rmask"][r], ws["inv_den"], H, W, min(m, plan["n"] - k * m), wrap,
                                            r == 0 and k == 0, r == R - 1 and k == nc - 1, acc=ws["acc"], out=ws["eps"])
            return ws["eps"]
        for k in range(nc):
            ops.window_gather(x, ws["offs"][k], h, w, wrap, out=ws["win"])
            e = self._eps(x_info, ws["win"].view(B * m, C, h, w), t, c_info_list, guided, single, emb_rows, pag=pag)
            ops.window_merge(e.to(torch.float16).contiguous().view(-1, m, C, h, w), ws["offs"][k], ws["wgt"], ws["inv_den"], H, W,
                             min(m, plan["n"] - k * m), wrap, k == 0, k == nc - 1, acc=ws["acc"], out=ws["eps"])
        return ws["eps"]

    def _eps(self, x_info, x, t, c_info_list, guided, single, emb_rows=None, deep=None, window=None, pag=None, sag=None):
        """The UNet on latent x at timesteps t.  guided: the batch is [x; x] (ddim.py:144-149); it is handed over as (x, repeat=2)
        so the data blocks in front of the first context block run once (extension key of this package's apply_model*).
        deep: (DeepCache, "store" | "reuse") of a cached call's full / shallow step (apply_model*'s 'deep_cache').
        window: the _window_state of a windowed call -- x is the canvas, and so is what comes back (_eps_windowed).
        x_info['freeu'] (FreeU, vd.freeu_setting) travels with every forward, so with windows it acts inside each window's.
        pag: None, or the layers of perturbed-attention guidance: one more replica, the last, runs those context blocks with
        identity self-attention (apply_model*'s 'pag' = (layers, first perturbed row)); with windows, in each window's forward.
        Or the dict of _pert_fwd (smoothed energy guidance): the same replica blurs its queries in those blocks instead
        (apply_model*'s 'seg' = (layers, first perturbed row, sigma) and 'seg_buffers' = (taps, workspace)).
        x_info['tome_ratio'] / ['tome_max_downsample'] (token merging, vd._tome_arg) travel with every forward as apply_model*'s
        'tome', so with windows the merge acts on each window's token grid.
        x_info['hypertile'] / ['hypertile_max_downsample'] (HyperTile, vd._hypertile_arg) travel the same way, as apply_model*'s
        'hypertile': with windows the tiles are cut on each window's token grid.
        sag: None, or the fp32 [T, B, Nm] mass buffer of self-attention guidance (apply_model*'s 'sag'): the forward also writes the
        column mass of the middle block's self-attention map of replica 0 into it."""
        if window is not None:
            assert deep is None and sag is None, "DeepCache and sag do not combine with windows"
            return self._eps_windowed(x_info, x, t, c_info_list, guided, single, emb_rows, window, pag)
        reps = replica_count(guided, pag is not None)
        xi = {"type": x_info["type"], "x": x, "repeat": reps}
        if pag is not None:
            assert deep is None, "DeepCache does not combine with pag"
            if isinstance(pag, dict):
                xi["seg"] = (pag["layers"], (reps - 1) * x.shape[0], pag["sigma"])
                xi["seg_buffers"] = (pag["taps"], pag["qb"])
            else:
                xi["pag"] = (pag, (reps - 1) * x.shape[0])
        if sag is not None:
            assert deep is None, "DeepCache does not combine with sag"
            xi["sag"] = sag
        if emb_rows is not None:
            xi["emb_rows"] = emb_rows
        if deep is not None:
            xi["deep_cache"] = deep
        if x_info.get("freeu") is not None:
            xi["freeu"] = x_info["freeu"]
        tome = _tome_arg(x_info, self.model)
        if tome is not None:
            xi["tome"] = tome
        hypertile = _hypertile_arg(x_info, self.model)
        if hypertile is not None:
            xi["hypertile"] = hypertile
        if single:
            return self.model.apply_model(xi, t, c_info_list[0])
        return self.model.apply_model_multicontext(xi, t, c_info_list)

    @staticmethod
    def _pert_fwd(pag, device, st=None):
        """What _eps takes as `pag`: the layers of perturbed-attention guidance (pag = (s_pag, layers)), or for smoothed energy
        guidance (pag = (s_seg, layers, sigma)) the dict {"layers", "sigma", "taps", "qb"} -- taps and workspace from the static
        state `st` (a captured step uploads and allocates nothing), else the taps uploaded here and no workspace (every launch
        allocates its own)."""
        if len(pag) == 2:
            return pag[1]
        if st is not None:
            return {"layers": pag[1], "sigma": pag[2], "taps": st["seg_taps"], "qb": st["seg_qb"]}
        taps = seg_taps(pag[2])[1]
        return {"layers": pag[1], "sigma": pag[2], "taps": None if taps is None else torch.from_numpy(taps).to(device), "qb": None}

    def _seg_state_arg(self, pag, x, c_info_list, window):
        """_new_state's `pag` of a call: False, True (perturbed-attention guidance), or for smoothed energy guidance the dict
        {"R", "rows", "elems", "types"}: the tap radius (-1: mean mode), the rows of the perturbed replica in a forward, the fp16
        elements one of them needs at most (vd.seg_workspace_elems on the latent or the window) and the number of context types."""
        if pag is None or len(pag) == 2:
            return pag is not None
        H, W = (x.shape[2], x.shape[3]) if window is None else window["key"][:2]
        return {"R": seg_taps(pag[2])[0], "rows": x.shape[0] * (1 if window is None else window["m"]),
                "elems": seg_workspace_elems(self.model, [ci["type"] for ci in c_info_list], H, W, pag[1]), "types": len(c_info_list)}

    def _sag_eager(self, sag, scale, guided, c_info_list, x):
        """The device state of self-attention guidance for one call of the eager loop (or one p_sample_ddim*): what _new_state keeps
        and _load_state loads on the static loop, plus "alphas", the float64 host schedule "coef" is refreshed from per step."""
        st = self._sag_buffers(x, len(c_info_list))
        self._sag_load(st, sag, scale, guided, c_info_list)
        st["alphas"] = np.asarray(self.alphas_cumprod, dtype=np.float64)
        return st

    def _sag_buffers(self, x, T):
        """The buffers of a self-attention-guidance step on the latent x [B, C, H, W] with T context types: "mass" fp32 [T, B, Nm]
        (written by the first forward), "xd" (the degraded latent, the second forward's input), "coef" fp32 [3] = {sa, s1, isa}
        (per step), and per call "w" fp32 [1] (sag_weight), "taps" fp32 [9] (vd.sag_taps) and "ratio" fp32 [T] (sag_ratios)."""
        Hm, Wm = sag_map_size(self.model.diffuser["image"], x.shape[2], x.shape[3])
        f32 = dict(device=x.device, dtype=torch.float32)
        return {"map": (Hm, Wm), "mass": torch.zeros((T, x.shape[0], Hm * Wm), **f32), "xd": torch.empty_like(x),
                "coef": torch.empty((3,), **f32), "w": torch.empty((1,), **f32), "taps": torch.empty((9,), **f32),
                "ratio": torch.empty((T,), **f32)}

    @staticmethod
    def _sag_load(sg, sag, scale, guided, c_info_list):
        """This call's fold weight, blur taps and context ratios into the buffers of _sag_buffers; sag = (s_sag, sigma)."""
        dev = sg["w"].device
        sg["w"].fill_(float(sag_weight(scale, sag[0], guided)))
        sg["taps"].copy_(torch.from_numpy(sag_taps(sag[1]).astype(np.float32)).to(dev))
        sg["ratio"].copy_(torch.from_numpy(sag_ratios(c_info_list)).to(dev))

    def _sag_fold(self, sg, x_info, x, t, eps, c_info_list, single, emb_rows=None):
        """The second half of a self-attention-guidance step, behind the first forward (which wrote sg["mass"]): ops.sag_degrade of
        the latent x with replica 0 of eps into sg["xd"], the second forward on it -- one replica, with the replica-0 rows of the
        contexts and of their cached K/V (vd.kv_rows: nothing is projected again), the same FreeU setting and time-embedding rows --
        and ops.sag_fold of its prediction into replica 0 of eps (contiguous fp16 [R B, C, H, W]), in place.  t: the B timesteps."""
        B = x.shape[0]
        ops.sag_degrade(x, eps[:B], sg["mass"], sg["ratio"], sg["taps"], sg["coef"], sg["map"][0], sg["map"][1], out=sg["xd"])
        c0 = [dict(ci, c=ci["c"][:B], kv_cache=kv_rows(ci.get("kv_cache"), B)) for ci in c_info_list]
        e_d = self._eps(x_info, sg["xd"], t, c0, False, single, emb_rows)
        return ops.sag_fold(eps, e_d.to(torch.float16).contiguous(), sg["w"])

    def _coef_table(self, total_steps, scale, device):
        """[S, 6] fp32 device table of {scale, 1/sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sigma, sqrt(1-a_t)}; row i is
        copied into the static coef buffer before step i (a sampler on this loop returns its own [S, coef_width] table)."""
        a_t = self.ddim_alphas[:total_steps].astype(np.float64)
        a_prev = self.ddim_alphas_prev[:total_steps].astype(np.float64)
        sig = self.ddim_sigmas[:total_steps].astype(np.float64)
        tab = np.stack([np.full_like(a_t, float(scale)), 1.0 / np.sqrt(a_t), np.sqrt(a_prev),
                        np.sqrt(np.maximum(1.0 - a_prev - sig ** 2, 0.0)), sig,
                        self.ddim_sqrt_one_minus_alphas[:total_steps].astype(np.float64)], axis=1)
        return torch.from_numpy(tab.astype(np.float32)).to(device)

    # ---- the static step loop ----------------------------------------------------------------------------
    def _new_state(self, x, c_info_list, guided, inpaint, rescale=0., cache_depth=0, window=None, pag=False, sag=False, apg=False):
        """Everything a captured step dereferences: latent buffers, step scalars, the CFG context batches and their K/V
        projections, the sampler's own buffers (_extra_static), when inpainting x0 / noise / mask / blend, and with the guidance
        rescale its weight "phi" (fp32 [1], loaded per call: one graph serves every positive weight) and the factors "kfac"
        (fp32 [B], written by every step); and the graph.  cache_depth > 0 (DeepCache sampling): "graph" is the full step that
        stores the deep feature, "graph_shallow" the step that reuses it, and "deep" holds the one kept buffer both read.
        window (the plan of _window_args): "window" holds its tables and buffers (_window_state), and "ts" has a row per
        window slot like the context batches.  pag (perturbed-attention guidance on): "ts" and the window buffers have the rows
        of replica_count(guided, pag) replicas, and "pag_w" is the fold's weight (fp32 [1], loaded per call: one graph serves
        every positive pag_scale and every guidance scale); a dict (_seg_state_arg: smoothed energy guidance, the same replica and
        fold) adds "seg_taps" (fp32 [2 R + 1], loaded per call: one graph serves every sigma of the same R; None in mean mode) and
        "seg_qb" (fp16 [context types, perturbed rows, elements]: the workspace of the blurred queries).  sag (self-attention guidance on): "sag" holds the buffers of
        _sag_buffers; its weight, taps and ratios are loaded per call, its coefficients per step: one graph serves every sag_scale,
        sigma and guidance scale.  apg (adaptive projected guidance on): "apg_v" is the running direction (fp32, like the latent),
        "apg_coef" the fold's row (fp32 [8], loaded per step) and "apg_fac" its per-sample figures (fp32 [B, 4], written by every
        step): one graph serves every eta, threshold, momentum and guidance scale."""
        nb = replica_count(guided, pag) * x.shape[0] * (1 if window is None else window["m"])
        st = {"xs": torch.empty_like(x), "x_next": torch.empty_like(x), "p0": torch.empty_like(x),
              "ts": torch.empty((nb,), device=x.device, dtype=torch.long),
              "coef": torch.empty((self.coef_width,), device=x.device, dtype=torch.float32),
              "c": [torch.empty(ci["c"].shape, device=x.device, dtype=torch.float16) for ci in c_info_list],
              "kv": [dict() for _ in c_info_list], "graph": None}
        st.update(self._extra_static(x))
        if cache_depth > 0:
            st.update(graph_shallow=None, deep=DeepCache(cache_depth))
        if window is not None:
            st["window"] = self._window_state(window, x, guided, pag)
        if pag:
            st["pag_w"] = torch.empty((1,), device=x.device, dtype=torch.float32)
        if isinstance(pag, dict):
            st["seg_taps"] = None if pag["R"] < 0 else torch.empty((2 * pag["R"] + 1,), device=x.device, dtype=torch.float32)
            st["seg_qb"] = torch.empty((pag["types"], pag["rows"], pag["elems"]), device=x.device, dtype=torch.float16)
        if sag:
            st["sag"] = self._sag_buffers(x, len(c_info_list))
        if apg:
            st.update(apg_v=torch.empty(x.shape, device=x.device, dtype=torch.float32),
                      apg_coef=torch.empty((8,), device=x.device, dtype=torch.float32),
                      apg_fac=torch.empty((x.shape[0], 4), device=x.device, dtype=torch.float32))
        if rescale > 0.:
            st.update(phi=torch.empty((1,), device=x.device, dtype=torch.float32),
                      kfac=torch.empty((x.shape[0],), device=x.device, dtype=torch.float32))
        if inpaint is not None:
            st.update({k: torch.empty_like(inpaint[k]) for k in ("x0", "noise", "mask")},
                      blend=torch.empty((2,), device=x.device, dtype=torch.float32))
        return st

    def _static_key(self, x, x_info, c_info_list, guided, single, inpaint=None, rescale=0., cache_depth=0, window=None):
        """What a kept step graph is good for: a call with another key never replays it (_static_state)."""
        # in-place updates / load_state_dict bump a parameter's version, .half() / .to() move its storage: the key hashes the
        # ORDERED (storage, version) pairs of every parameter and buffer (an additive checksum would let two parameters
        # that swap storages collide)
        wv = hash(tuple((t.data_ptr(), t._version) for t in list(self.model.parameters()) + list(self.model.buffers())))
        # (emb_hoist is part of the key: a step graph captured with the hoisted time embedding reads st["embrow"], one captured
        # without it computes the embedding inside the step -- replaying either under the other setting would be silently wrong;
        # so is inpainting with its mask batch: a graph captured with the blend reads the static x0 / noise / mask buffers;
        # and the guidance rescale (`rescale`: its weight), on or off whatever the positive weight: a graph captured with it
        # launches the factor kernel and the rescaled update, one captured without it must keep giving the unrescaled bits;
        # and DeepCache sampling with its depth (0: off), not its interval: one pair of graphs serves every interval >= 2, and
        # an uncached call never replays a graph that stores;
        # and windowed sampling with its whole geometry (h, w, sy, sx, wrap, weight, nc, m), None when off: the graph holds the
        # gather / forward / merge chain of that plan and reads its tables; with regional prompts the number of regions follows
        # (the chain runs once per region), the masks do not: they are loaded per call;
        # and FreeU with its four values (b1, b2, s1, s2), None when off or all ones: the scalars are arguments of the captured
        # ops.freeu launches, and which stages launch at all depends on them -- one graph per setting;
        # and perturbed-attention guidance, (on?, layers): a graph captured with it runs one more replica, the identity attention of
        # those context blocks and the fold; its scale is not in the key -- the fold's weight is loaded per call;
        # and token merging, (ratio, max_downsample) or None, in front of those two: r is an argument of the captured launches and
        # decides the shapes behind them -- one graph per setting;
        # and self-attention guidance: a further entry ("sag",) at the END when it is on, nothing when it is off (the key of a call
        # without it is the key it always had): a graph captured with it runs the mass, the degrade, a second forward and the fold;
        # its scale and sigma are not in the key -- weight and taps are loaded per call;
        # and HyperTile, likewise: a further entry ("hypertile", tile, max_downsample) in front of sag's when it is on, nothing when it
        # is off: the tile side is an argument of the captured tile / untile launches and decides the attention's shapes;
        # and adaptive projected guidance, likewise: a further entry ("apg",) at the very end when it is on (a guided call whose
        # triple is not the neutral one), nothing when it is off: a graph captured with it launches the fold; eta, threshold and
        # momentum are not in the key -- the fold's row is loaded per step;
        # and smoothed energy guidance, likewise: a further entry ("seg", layers, R) when it is on, R = -1 for the mean query: a graph
        # captured with it runs pag's extra replica with the query blur of those blocks at that tap radius and the fold; its scale
        # and its taps are not in the key -- both are loaded per call, so one graph serves every sigma of the same R)
        pag = _pag_arg(x_info, self.model)
        tome = _tome_arg(x_info, self.model)
        mask_batch = 0 if inpaint is None else inpaint["mask"].shape[0]
        key = (id(self.model), wv, str(x.device), tuple(x.shape), x_info["type"], bool(guided), bool(single), bool(self.emb_hoist),
               tuple((ci["type"], tuple(ci["c"].shape), float(ci.get("ratio", 1.0))) for ci in c_info_list),
               inpaint is not None, mask_batch, rescale > 0., cache_depth, None if window is None else window["key"],
               None if tome is None else tome.key(), (pag is not None, None if pag is None else pag[1]), _freeu_arg(x_info))
        hypertile = _hypertile_arg(x_info, self.model)
        if hypertile is not None:
            key = key + (("hypertile",) + hypertile.key(),)
        if _sag_arg(x_info, self.model) is not None:
            key = key + (("sag",),)
        if guided and _apg_arg(x_info) is not None:
            key = key + (("apg",),)
        seg = _seg_arg(x_info, self.model)
        if seg is not None:
            key = key + (("seg", seg[1], seg_taps(seg[2])[0]),)
        return key

    def _static_state(self, x, x_info, c_info_list, guided, single, inpaint=None, rescale=0., cache_depth=0, window=None, pag=False,
                      sag=False, apg=False):
        """The state (_new_state) kept ACROSS sample() calls per (model weights, shapes, flow): a second call with the same
        geometry re-uses the instantiated HIP graph instead of capturing again (capture = one host-bound pass over ~400
        launches with the GPU idle + instantiation: 10-15 ms per batch of 680).  None when graphs are not kept."""
        if not self.graph_cache:
            return None
        key = self._static_key(x, x_info, c_info_list, guided, single, inpaint, rescale, cache_depth, window)
        st = self._static.pop(key, None)
        if st is None:
            while len(self._static) >= 2:                      # shapes seen long ago: let their graphs go
                self._static.pop(next(iter(self._static)))
            st = self._new_state(x, c_info_list, guided, inpaint, rescale, cache_depth, window, pag, sag, apg)
        self._static[key] = st                                 # most recently used last
        return st

    def _load_state(self, st, x, c_info_list, inpaint, phi=0., window=None, pag_w=None, sag=None, seg=None):
        """seg: None, or the fp32 taps of this call's smoothed energy guidance (vd.seg_taps), copied into "seg_taps".  Copy this call's latent, contexts, inpainting tensors, region masks (with their inv_den; `window` is the call's
        plan), the weight of the perturbed-attention fold (pag_w, pag_weight) and the weight, taps and ratios of self-attention
        guidance (sag = (s_sag, sigma, guidance scale, guided); _sag_load) into the state and hand its context buffers and
        K/V caches to c_info_list.  Returns whether step 0 may be replayed (else it runs eagerly and refreshes the K/V on its way)."""
        st["xs"].copy_(x)
        if window is not None and "regions" in window:      # one kept graph serves every mask of the same R and geometry
            st["window"]["rmask"].copy_(torch.from_numpy(window["masks"]))
            st["window"]["inv_den"].copy_(torch.from_numpy(window["inv_den"]))
        if "phi" in st:
            st["phi"].fill_(phi)
        if "pag_w" in st:
            st["pag_w"].fill_(float(pag_w))
        if st.get("seg_taps") is not None:
            st["seg_taps"].copy_(torch.from_numpy(seg))
        if "sag" in st:
            self._sag_load(st["sag"], sag[:2], sag[2], sag[3], c_info_list)
        if inpaint is not None:
            for k in ("x0", "noise", "mask"):
                st[k].copy_(inpaint[k])
        for ci, cbuf, kv in zip(c_info_list, st["c"], st["kv"]):
            cbuf.copy_(ci["c"])
            ci["c"] = cbuf
            kv_mark_stale(kv)   # K/V of the previous call's context: recomputed in place
            ci["kv_cache"] = kv
        if not (st["graph"] is not None and self.use_graph and self.replay_first and all(kv_refreshable(kv) for kv in st["kv"])):
            return False
        # a kept graph: the context K/V projections of this call are refreshed in place right here (16 small GEMMs per
        # context), so step 0 is replayed like every other step instead of running its ~370 launches eagerly
        for ci, kv in zip(c_info_list, st["kv"]):
            kv_refresh(kv, self.model._prep(ci["c"]))
        return True

    def _step_emb(self, st, x_info, steps_dev, single):
        """(table [S, total], {data block index: view of st["embrow"]}) of the hoisted time embedding, or (None, None): every
        sample of the batch is at the same timestep in every step, and all steps are known now, so the t-only part of the forward
        (reference vd.py:339-349 -> openaimodel.py:2627-2633, :263) is computed here for all of them (M = steps instead of `steps`
        times M = batch) and the step reads row i from the static buffer st["embrow"]."""
        pre = None
        if self.emb_hoist and hasattr(self.model, "precompute_step_emb"):
            pre = self.model.precompute_step_emb(x_info["type"], steps_dev, multicontext=not single)
        if st.get("graph_embrow", pre is not None) != (pre is not None):
            # the kept graph was captured with / without the hoisted embedding row and this call has it the other way round
            # (precompute_step_emb started / stopped returning a table): capture again instead of replaying stale conditioning
            st["graph"] = None
            if "graph_shallow" in st:
                st["graph_shallow"] = None
        if pre is None:
            return None, None
        emb_tab, layout = pre
        if "embrow" not in st or st["embrow"].numel() != emb_tab.shape[1]:
            assert st["graph"] is None and st.get("graph_shallow") is None, "the kept step graph reads another time-embedding buffer"
            st["embrow"] = torch.empty((emb_tab.shape[1],), device=emb_tab.device, dtype=torch.float16)
        return emb_tab, {di: st["embrow"][o:o + c] for di, (o, c) in layout.items()}

    def _loop_static(self, x, x_info, c_info_list, timesteps, guided, scale, single, log_every_t, dtype, inpaint=None,
                     phi=0., interval=1, depth=1, window=None, pag=None, sag=None, apg=None):
        """eta = 0 loop on static buffers: step 0 runs eagerly (fills weight-pack and K/V caches), is then captured
        into a HIP graph, and the graph is replayed for the remaining steps -- and, through _static_state, by later
        sample() calls of the same geometry.  Returns (final fp16 latent, intermediates).
        interval > 1 (DeepCache sampling, _cache_args): step i is full iff i % interval == 0 and runs the graph st["graph"]
        (forward that stores the deep feature + update), every other step runs st["graph_shallow"] (forward that reuses it +
        update); each is captured the first time its kind of step is met behind step 0, which is full and, when eager, fills
        every cache either walk needs (the shallow walk runs a subset of the full walk's blocks at the same shapes).
        window (the plan of _window_args): the step's prediction is the fusion of the windows' (_eps_windowed); the update, the
        rescale factors, the blend, the seeded noise and the solver histories see the canvas and nothing else.
        pag (None, or (s_pag, layers) of vd._pag_arg, or (s_seg, layers, sigma) of vd._seg_arg -- smoothed energy guidance, the same
        replica with blurred queries instead of the identity map): the forward runs one more replica, perturbed, and ops.pag_fold folds its
        prediction into replica 0 between the forward and the update; the update, the rescale factors, the blend, the noise and the
        histories see the folded pair (or single) and nothing else, so every sampler on this loop gets it.
        sag (None, or (s_sag, sigma) of vd._sag_arg): the step runs TWO forwards in sequence in the one captured graph -- the first,
        today's, also writes the column mass of the middle block's self-attention map; ops.sag_degrade blurs and re-noises the latent
        with it; the second forward predicts from that on one replica; ops.sag_fold folds its prediction into replica 0 (_sag_fold) --
        and then the unchanged update, like pag's.
        apg (None, or (eta, r, beta) of vd._apg_arg; guided calls only): ops.apg_fold rewrites replica 0 right behind the forward,
        in front of pag's fold, from the latent, the pair and the running direction kept in the state (apg_guided_eps); the row of
        apg_coef_table is copied next to the coefficient row, so one kept graph serves every setting; the update, the rescale
        factors, the blend, the noise and the histories see the folded pair, so every sampler on this loop gets it."""
        tome = _tome_arg(x_info, self.model)
        if tome is not None and tome.record is not None and self.use_graph:
            raise ValueError("tome: TokenMerge.record is an eager-only hook; this loop captures its steps into a graph (use_graph)")
        total_steps = timesteps.shape[0]
        rescale = phi if guided else 0.          # the guidance-rescale weight of this call; 0: off
        cache_depth = depth if interval > 1 else 0
        pstate = self._seg_state_arg(pag, x, c_info_list, window)     # False, True, or the sizes of smoothed energy guidance
        st = (self._static_state(x, x_info, c_info_list, guided, single, inpaint, rescale, cache_depth, window, pstate,
                                 sag is not None, apg is not None)
              or self._new_state(x, c_info_list, guided, inpaint, rescale, cache_depth, window, pstate, sag is not None,
                                 apg is not None))
        replay_first = self._load_state(st, x, c_info_list, inpaint, rescale, window,
                                        None if pag is None else pag_weight(scale, pag[0], guided),
                                        None if sag is None else (sag[0], sag[1], scale, guided),
                                        seg_taps(pag[2])[1] if isinstance(pstate, dict) else None)
        pfwd = None if pag is None else self._pert_fwd(pag, x.device, st)
        sag_tab = None if sag is None else torch.from_numpy(sag_coef_table(self.alphas_cumprod, timesteps[:total_steps])).to(x.device)
        apg_tab = None if apg is None else torch.from_numpy(apg_coef_table(self.alphas_cumprod, timesteps[:total_steps], *apg)).to(x.device)
        per_sample = x.numel() // x.shape[0]
        reps = replica_count(guided, pag is not None)
        table = self._coef_table(total_steps, scale, x.device)
        rng_tab = self._rng_table(total_steps, x.device)
        steps_dev = torch.from_numpy(np.ascontiguousarray(np.flip(timesteps)).astype(np.int64)).to(x.device)
        emb_tab, emb_rows = self._step_emb(st, x_info, steps_dev, single)

        def body(mode=None):
            eps = self._eps(x_info, st["xs"], st["ts"], c_info_list, guided, single, emb_rows,
                            None if mode is None else (st["deep"], mode), st.get("window"), pfwd,
                            None if sag is None else st["sag"]["mass"])
            eps = eps.contiguous()
            if apg is not None:     # replica 0 rewritten from the latent, the pair and the running direction
                ops.apg_fold(st["xs"], eps, st["apg_v"], st["apg_coef"], per_sample, out_fac=st["apg_fac"])
            if pag is not None:
                eps = ops.pag_fold(eps, reps, st["pag_w"])      # the folded pair (single): what every update below reads
            if sag is not None:     # degrade, second forward, fold into replica 0: what every update below reads
                eps = self._sag_fold(st["sag"], x_info, st["xs"], st["ts"][:st["xs"].shape[0]], eps, c_info_list, single, emb_rows)
            self._update_static(st, eps, guided)

        bodies = {"graph": body if interval == 1 else (lambda: body("store")), "graph_shallow": lambda: body("reuse")}

        # RNG contract: the reference draws noise_like(x) = torch.randn_like(x) on every step even when sigma = 0
        # (ddim.py:167 / :294 there), so the device generator ends a sample() call advanced by one latent-sized draw per
        # step.  The draws are consumed here, up front, and the generator state is pinned to that point after the loop
        # (graph capture / replay bookkeeping must not leak into it), so code that keeps drawing from the default
        # generator after sample() sees the reference's stream.
        for _ in range(total_steps if self.draws_step_noise else 0):
            torch.randn_like(st["xs"])
        rng_after = torch.cuda.get_rng_state(x.device)
        intermediates = {"pred_xt": [], "pred_x0": []}
        if rescale > 0.:
            intermediates["guidance_rescale"] = []
        if apg is not None:
            intermediates["apg"] = []
        for i in range(total_steps):
            index = total_steps - i - 1
            st["ts"].copy_(steps_dev[i].expand(st["ts"].shape[0]))       # device-side refresh, no host sync
            st["coef"].copy_(table[index])
            if sag_tab is not None:
                st["sag"]["coef"].copy_(sag_tab[index])
            if apg_tab is not None:
                st["apg_coef"].copy_(apg_tab[index])
            if rng_tab is not None:
                st["rng"].copy_(rng_tab[i])
            if inpaint is not None:
                st["blend"].copy_(inpaint["table"][index])
            if emb_tab is not None:
                st["embrow"].copy_(emb_tab[i])
            kind = "graph" if i % interval == 0 else "graph_shallow"
            if (i == 0 and not replay_first) or not self.use_graph:
                bodies[kind]()
            else:
                if st[kind] is None:
                    st[kind] = self._capture(bodies[kind])
                    st["graph_embrow"] = emb_tab is not None
                if st[kind] is None:
                    bodies[kind]()
                else:
                    st[kind].replay()
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates["pred_xt"].append(st["xs"].to(dtype).clone())
                intermediates["pred_x0"].append(st["p0"].to(dtype).clone())
                if rescale > 0.:
                    intermediates["guidance_rescale"].append(st["kfac"].clone())
                if apg is not None:
                    intermediates["apg"].append(st["apg_fac"].clone())
        torch.cuda.set_rng_state(rng_after, x.device)
        return st["xs"].clone(), intermediates

    def _rng_table(self, total_steps, device):
        """int32 [S, 2] device table whose row i (sampling order) is copied into the sampler's static "rng" buffer
        (_extra_static) before step i, next to the coefficient row; None: the sampler has no such buffer."""
        return None

    def _extra_static(self, x):
        """Further step-loop buffers (name -> tensor) of a sampler built on this loop, kept with the step graph."""
        return {}

    def _update_static(self, bufs, eps, guided):
        """The update at the end of a static step: reads bufs["xs"] (latent), eps and bufs["coef"], leaves the next latent in
        bufs["xs"] and the data prediction in bufs["p0"].  Captured into the step graph with the UNet forward.  When inpainting
        (bufs has "mask"), the latent that lands in bufs["xs"] is blended with the known region (_blend_static).  With the
        guidance rescale (bufs has "kfac") the factor kernel runs first and the update multiplies by its factors."""
        if "kfac" in bufs:
            self._rescale_static(bufs, eps)
            ops.cfg_ddim_step_dev_rs(bufs["xs"], eps, bufs["coef"], bufs["kfac"], guided=guided, x_prev=bufs["x_next"],
                                     pred_x0=bufs["p0"])
        else:
            ops.cfg_ddim_step_dev(bufs["xs"], eps, bufs["coef"], guided=guided, x_prev=bufs["x_next"], pred_x0=bufs["p0"])
        if "mask" in bufs:
            self._blend_static(bufs, bufs["x_next"])          # in place of the copy: no extra launch
        else:
            bufs["xs"].copy_(bufs["x_next"])

    @staticmethod
    def _rescale_static(bufs, eps):
        """bufs["kfac"] = the guidance-rescale factors of eps for the scale in bufs["coef"][0] and the weight bufs["phi"]."""
        ops.cfg_rescale_factor(eps, bufs["coef"], bufs["phi"], bufs["xs"].numel() // bufs["xs"].shape[0], out=bufs["kfac"])

    @staticmethod
    def _blend_static(bufs, x):
        """bufs["xs"] = mask x + (1 - mask) (blend[0] x0 + blend[1] noise) on the static inpainting buffers."""
        ops.masked_blend(x, bufs["x0"], bufs["noise"], bufs["mask"], bufs["blend"], out=bufs["xs"])

    def _capture(self, body):
        with _no_gc():
            return self._capture_step(body)

    def _capture_step(self, body):
        try:
            g = torch.cuda.CUDAGraph()
            s = capture_stream()   # (never a side stream of the forked UNet branches)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    body()
            torch.cuda.current_stream().wait_stream(s)
            ops.drop_workspaces(s.cuda_stream)
            return g
        except Exception as e:  # stay on the (same) HIP kernels, just launched eagerly
            print("[DDIMSampler] HIP graph capture unavailable (%s); running steps eagerly" % e)
            self.use_graph = False
            return None

    def _step(self, x, x_info, c_info_list, step, index, guided, scale, temperature, single, noise_dropout=0., rescale=None,
              deep=None, window=None, pag=None, sag=None, apg=None):
        """One p_sample_ddim (reference ddim.py:129-171 / 244-298) on the fp16 device latent `x` [B,C,H,W]: (x_prev, pred_x0,
        the guidance-rescale factors [B] or None).  rescale: None, or the device scalars of _rescale_scalars.  deep, window: _eps's.
        pag: None, or (layers, the fold's weight as a device fp32 [1]) of perturbed-attention guidance.
        sag: None, or the state of _sag_eager: the step of self-attention guidance (_sag_fold) between the forward and the update.
        apg: None, or (running direction fp32 like x, the step's device row of apg_coef_table, fac fp32 [B, 4] to write) of adaptive
        projected guidance: ops.apg_fold right behind the forward, as in the static loop."""
        reps = replica_count(guided, pag is not None)
        rows = reps * x.shape[0] * (1 if window is None else window["plan"]["m"])
        t_in = torch.full((rows,), step, device=x.device, dtype=torch.long)
        eps = self._eps(x_info, x, t_in, c_info_list, guided, single, deep=deep, window=window, pag=None if pag is None else pag[0],
                        sag=None if sag is None else sag["mass"])
        sigma = float(self.ddim_sigmas[index])
        # drawn on every step like the reference's noise_like(x) (ddim.py:167 there): same generator consumption, and for
        # eta > 0 the same noise values as a reference running in fp16 on this device
        noise = torch.randn_like(x)
        if noise_dropout > 0.:
            # reference: noise = dropout(sigma_t * noise_like(x) * temperature, p) -- the mask (and its 1 / (1 - p) scale)
            # commutes with the scalar factors, so it is applied to the unit noise; drawn even at sigma = 0, like there
            noise = torch.nn.functional.dropout(noise, p=noise_dropout)
        if sigma != 0.:
            noise = noise if temperature == 1. else (noise.float() * temperature).to(torch.float16)
        else:
            noise = None
        scalars = dict(guided=guided, guidance_scale=float(scale), a_t=float(self.ddim_alphas[index]),
                       a_prev=float(self.ddim_alphas_prev[index]), sigma=sigma,
                       sqrt_one_minus_at=float(self.ddim_sqrt_one_minus_alphas[index]), noise=noise)
        eps = eps.contiguous()
        if apg is not None:
            ops.apg_fold(x, eps, apg[0], apg[1], x.numel() // x.shape[0], out_fac=apg[2])
        if pag is not None:
            eps = ops.pag_fold(eps, reps, pag[1])
        if sag is not None:
            a = sag["alphas"][step]
            sag["coef"].copy_(torch.tensor([np.sqrt(a), np.sqrt(1.0 - a), 1.0 / np.sqrt(a)], dtype=torch.float32))
            eps = self._sag_fold(sag, x_info, x, t_in[:x.shape[0]], eps.to(torch.float16), c_info_list, single)
        if rescale is None:
            return ops.cfg_ddim_step(x, eps, **scalars) + (None,)
        kfac = ops.cfg_rescale_factor(eps, rescale[0], rescale[1], x.numel() // x.shape[0])
        return ops.cfg_ddim_step_rs(x, eps, kfac, **scalars) + (kfac,)

    @staticmethod
    def _rescale_scalars(scale, phi, device):
        """(guidance scale, weight) as fp32 [1] device tensors for the eager steps' factor kernel; None when the rescale is off
        (phi == 0, which _cfg_contexts also returns for an unguided call)."""
        if not phi > 0.:
            return None
        f32 = dict(device=device, dtype=torch.float32)
        return torch.full((1,), float(scale), **f32), torch.full((1,), float(phi), **f32)

    @torch.no_grad()
    def p_sample_ddim(self, x_info, c_info, t, index, repeat_noise=False, use_original_steps=False,
                      noise_dropout=0., temperature=1.):
        """Reference-compatible single step: returns (x_prev, pred_x0)."""
        return self._p_sample(x_info, [c_info], t, index, repeat_noise, use_original_steps, noise_dropout, temperature, True)

    @torch.no_grad()
    def p_sample_ddim_multicontext(self, x_info, c_info_list, t, index, repeat_noise=False, use_original_steps=False,
                                   noise_dropout=0., temperature=1.):
        return self._p_sample(x_info, c_info_list, t, index, repeat_noise, use_original_steps, noise_dropout, temperature, False)

    def _p_sample(self, x_info, c_info_list, t, index, repeat_noise, use_original_steps, noise_dropout, temperature, single):
        if x_info.get("inpaint_mask") is not None:
            raise ValueError("inpaint_mask: masked sampling runs whole sample() loops; p_sample_ddim* does not blend")
        if _cache_args(x_info, self.model)[0] > 1:
            raise ValueError("cache_interval > 1: DeepCache sampling runs whole sample() loops; p_sample_ddim* keeps no feature")
        if x_info.get("window") is not None or x_info.get("region_masks") is not None:
            raise ValueError("window: windowed sampling runs whole sample() loops; p_sample_ddim* fuses no windows (or regions)")
        _freeu_arg(x_info)      # FreeU is stateless: the step's forward applies it (_eps)
        pag = _pag_arg(x_info, self.model)      # so is perturbed-attention guidance: one more replica and the fold
        seg = _seg_arg(x_info, self.model, x_info["x"].shape)   # and smoothed energy guidance: the same replica, blurred queries
        if seg is not None:
            pag = seg
        _tome_arg(x_info, self.model, x_info["x"].shape)    # and token merging: the step's forward applies it (_eps)
        _hypertile_arg(x_info, self.model, x_info["x"].shape)   # and HyperTile: the step's forward applies it (_eps)
        sag = _sag_arg(x_info, self.model, x_info["x"].shape)   # and self-attention guidance: the step runs its second forward
        assert not use_original_steps and not repeat_noise
        apg = _apg_arg(x_info)      # adaptive projected guidance keeps a running direction between the steps of a loop
        cis, guided, scale, phi = self._cfg_contexts(c_info_list, pag=pag is not None)
        if apg is not None and guided:
            raise ValueError("apg: adaptive projected guidance runs whole sample() loops; p_sample_ddim* keeps no direction between steps")
        x = x_info["x"]
        if pag is not None:
            pag = (self._pert_fwd(pag, x.device),
                   torch.full((1,), float(pag_weight(scale, pag[0], guided)), device=x.device, dtype=torch.float32))
        x16 = x.to(torch.float16).contiguous()
        xp, p0, _ = self._step(x16, x_info, cis, int(t[0]), index, guided, scale,
                               temperature, single, noise_dropout=noise_dropout,
                               rescale=self._rescale_scalars(scale, phi, x.device), pag=pag,
                               sag=None if sag is None else self._sag_eager(sag, scale, guided, cis, x16))
        return xp.to(x.dtype), p0.to(x.dtype)
