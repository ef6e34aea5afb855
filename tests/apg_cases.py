"""Adaptive projected guidance (Sadat, Hilliges, Weber 2024; diffusers' AdaptiveProjectedGuidance) restated for the tests: Algorithm 1
of the paper in the space of data predictions, transcribed in plain float64 torch and independent of ddim.apg_guided_eps; the DDIM /
DPM-Solver++(2M) / SDE / UniPC loops on the fp32 CPU oracle with it in place of the plain guidance combine (built on pag_cases.walk /
replicas and deepcache_cases.cfg_contexts, driven by the sampler's own coefficient table), with the guidance rescale, perturbed-
attention guidance, a window geometry and the inpainting blend as optional pieces; the kernel's cases, correlated inputs and bounds.
Shared by the CPU and the GPU tests."""
import numpy as np
import torch

import deepcache_cases as dc
import pag_cases as pc
from deepcache_cases import LATENT_TOL  # noqa: F401  (the project's bound, re-exported for the tests)

SCALE = 7.5
CTX_AMP = 8.0                     # test_cfg_rescale_gpu.CTX_AMP: the conditional context at which guidance moves the tiny model
SETTING = (0.0, 2.5, -0.5)        # (eta, norm threshold, momentum) of the sampler cases
STEPS = 10
SHAPE = [2, 4, 16, 16]
# (B, per_sample, element offset) of the kernel cases: the rescale tests' plus the [4, 9, 7] latent (252: 16-byte aligned samples
# with a partial last group at an even sample, misaligned samples at odd ones)
KERNEL_CASES = [(1, 1, 0), (3, 4099, 0), (3, 4099, 1), (2, 768, 0), (2, 252, 0), (4, 16384, 0), (2, 36864, 0)]
ETAS = [0.0, 0.5, 1.0]
BETAS = [0.0, -0.5]
A_T = 0.35                        # the alpha-bar of the kernel cases' step: s1 = 0.806, isa = 1.69, g = 1.36


def project(v0, v1):
    """diffusers' project(): (the part of v0 parallel to v1, the part orthogonal to it), per sample, in float64."""
    dims = list(range(1, v0.dim()))
    v1 = torch.nn.functional.normalize(v1.double(), dim=dims)
    par = (v0.double() * v1).sum(dim=dims, keepdim=True) * v1
    return par, v0.double() - par


def algorithm1(d_c, d_u, avg, s, eta, r, beta):
    """Algorithm 1 of the paper on data predictions d_c, d_u [B, ...] (float64): returns (the guided data prediction, the new running
    average).  avg: the running average of the step before, None on the first step."""
    diff = d_c.double() - d_u.double()
    if avg is not None:
        diff = diff + beta * avg                                    # momentum: the running average replaces the difference
    new_avg = diff
    if r > 0:
        norm = diff.flatten(1).norm(dim=1).view(-1, *([1] * (diff.dim() - 1)))
        diff = diff * torch.minimum(torch.ones_like(norm), r / norm)
    par, orth = project(diff, d_c)
    return d_c.double() + (s - 1.0) * (orth + eta * par), new_avg


def guided_eps(x, e_u, e_c, avg, a_t, s, setting):
    """float64: the guided epsilon of an APG step -- both predictions turned into data predictions at alpha-bar a_t, algorithm1, and
    the result turned back -- and the new running average."""
    sa, s1 = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    to_d = lambda e: (x.double() - s1 * e.double()) / sa
    d, avg = algorithm1(to_d(e_c), to_d(e_u), avg, s, *setting)
    return (x.double() - sa * d) / s1, avg


def rescale(e, e_c, phi):
    """diffusers' rescale_noise_cfg(e, e_c, phi), the standard deviations per sample in float64."""
    sd_ = lambda v: v.double().flatten(1).std(1, unbiased=False)
    k = float(np.float32(phi)) * (sd_(e_c) / sd_(e)) + (1.0 - float(np.float32(phi)))
    return e * k.view(-1, *([1] * (e.dim() - 1)))


def oracle_loop(sd, plan, sampler, kind, xT, contexts, scale, setting=None, phi=0.0, pag_scale=0.0, geo=None, blend=None, noise=None,
                first=None):
    """The loop `sampler` ran last ("ddim", "2m", "sde" or "unipc") in fp32 on the oracle with adaptive projected guidance of
    `setting` = (eta, r, beta) (None: plain guidance) in place of e_u + s (e_c - e_u), driven by the sampler's own coefficient table
    (pag_cases.oracle_loop's update formulas, restated).  phi: the guidance-rescale weight; pag_scale: perturbed-attention guidance
    in the middle block, added to the guided prediction; geo: a window geometry (window_cases.geometry); blend(index, x) -> x: the
    inpainting blend behind every step; noise(draw) -> the step noise of kind "sde"; first: a dict that receives the first step's
    "v_norm", "k", "p", "d_norm" per sample."""
    ts = sampler.ddim_timesteps
    S = len(ts)
    tab = sampler._coef_table(S, scale, torch.device("cpu")).double().numpy()
    ac = np.asarray(sampler.alphas_cumprod, dtype=np.float64)
    assert scale != 1.0
    pag = pag_scale > 0
    lay = pc.layers_of(plan, "mid") if pag else ()
    cs0 = dc.cfg_contexts(contexts, True)
    x = xT.float().cpu()
    hist = xl = m1 = m2 = m3 = avg = None
    for k, i in enumerate(reversed(range(S))):
        r = [float(v) for v in tab[i]]
        xin, cs, mask = pc.replicas(x, cs0, True, pag)
        t = torch.full((xin.shape[0],), int(ts[i]), dtype=torch.long)
        eps = pc.windowed_eps(sd, plan, xin, t, cs, geo, lay, mask) if geo is not None else pc.walk(sd, plan, xin, t, cs, lay, mask)
        parts = eps.chunk(3 if pag else 2)
        e_u, e_c = parts[0], parts[1]
        if setting is None:
            e = (e_u + r[0] * (e_c - e_u)).double()
        else:
            if first is not None and k == 0:
                a = float(ac[ts[i]])
                d_c = (x.double() - np.sqrt(1 - a) * e_c.double()) / np.sqrt(a)
                v = (-np.sqrt(1 - a) / np.sqrt(a)) * (e_c.double() - e_u.double())
                vn, dn = v.flatten(1).norm(dim=1), d_c.flatten(1).norm(dim=1)
                kk = torch.minimum(torch.ones_like(vn), setting[1] / vn) if setting[1] > 0 else torch.ones_like(vn)
                first.update(v_norm=vn, k=kk, p=kk * (v * d_c).flatten(1).sum(1) / dn ** 2, d_norm=dn)
            e, avg = guided_eps(x, e_u, e_c, avg, float(ac[ts[i]]), r[0], setting)
        if pag:
            e = e + pag_scale * (e_c - parts[2]).double()
        if phi > 0:
            e = rescale(e, e_c, phi)
        e = e.float()
        if kind == "ddim":      # {scale, 1/sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev - sigma^2), sigma, sqrt(1 - a_t)}
            p0 = (x - r[5] * e) * r[1]
            x = r[2] * p0 + r[3] * e
        elif kind in ("2m", "sde"):   # {scale, 1/sqrt(a_t), sqrt(1 - a_t), sigma_next/sigma_t, c_d, w_cur, w_prev, noise coefficient}
            p0 = (x - r[2] * e) * r[1]
            d = r[5] * p0 + (r[6] * hist if r[6] != 0 else 0.0)
            xn = r[3] * x + r[4] * d
            if kind == "sde" and r[7] != 0:
                xn = xn + r[7] * noise(k).reshape(x.shape).float()
            x, hist = xn, p0
        else:                   # the row layout of unipc.unipc_coef_table
            assert kind == "unipc"
            mt = (x - r[2] * e) * r[1]
            xc = x
            if r[3] != 0:
                xc = r[4] * xl + r[8] * mt
                for c, m in ((r[5], m1), (r[6], m2), (r[7], m3)):
                    if c != 0:
                        xc = xc + c * m
            xn = r[9] * xc + r[10] * mt
            for c, m in ((r[11], m1), (r[12], m2)):
                if c != 0:
                    xn = xn + c * m
            xl, m1, m2, m3, x = xc, mt, m1, m2, xn
        if blend is not None:
            x = blend(i, x).float()
    return x


# ---- the kernel's cases --------------------------------------------------------------------------------------------------------

def coef_row(eta, r, beta, a_t=A_T):
    """The fp32 row the fold reads, formed like ddim.apg_coef_table's: every entry in float64, rounded once."""
    s1, isa = np.sqrt(1.0 - a_t), 1.0 / np.sqrt(a_t)
    return np.array([s1, isa, 1.0 / (s1 * isa), beta, r, 1.0 - eta, 0.0, 0.0], dtype=np.float64).astype(np.float32)


def kernel_inputs(B, per, seed):
    """(x [B, per], eps [2B, per], v_prev [B, per]): fp16, fp16, fp32.  Correlated on purpose: e_u = e_c - 0.3 (a D-like term), so
    the direction has a parallel part with |p| of order 0.1 to 1 and eta matters."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, per), generator=g)
    e_c = torch.randn((B, per), generator=g)
    d_like = (x - np.sqrt(1.0 - A_T) * e_c) / np.sqrt(A_T) + 0.5 * torch.randn((B, per), generator=g)
    e_u = e_c - 0.3 * d_like
    v_prev = torch.randn((B, per), generator=g) * 0.5
    return x.half(), torch.cat([e_u, e_c]).half(), v_prev.float()


def thresholds(x, eps, v_prev, beta):
    """(0, a threshold that clips every sample, one that clips none) for these inputs: 0.4 and 2.5 times the mean norm of v."""
    from lib.model_zoo.ddim import apg_guided_eps
    nv = apg_guided_eps(x, eps, v_prev, coef_row(1.0, 0.0, beta).astype(np.float64))[2][:, 0]
    return [0.0, float(0.4 * nv.min()), float(2.5 * nv.max())]


def f32(t):
    return t.double().numpy().astype(np.float32)


def fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in float64 and the sum is rounded to float64 first; the double
    rounding differs from fmaf only when that sum sits within 2^-53 of an fp32 tie (tests/test_exact_norm_cpu.py's emulator)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def element_stage(x, eps, v_prev, row):
    """(D, v) as fp32 arrays [B, per] with the contract's roundings: D = fmaf(-s1, e_c, x) * isa; dD = (-g32) (e_c - e_u);
    v = fmaf(beta, v_prev, dD) or dD."""
    B = x.shape[0]
    xf, eu, ec = f32(x), f32(eps[:B]), f32(eps[B:])
    s1, isa, beta = row[0], row[1], row[3]
    D = fma32(-s1 * np.ones_like(ec), ec, xf) * isa
    g32 = np.float32(s1 * isa)
    dD = (-g32) * (ec - eu)
    v = fma32(np.full_like(dD, beta), f32(v_prev), dD) if beta != 0 else dD
    return D.astype(np.float32), v.astype(np.float32)


def fac_ref(D, v, row):
    """float64 [B, 4] = {||v||, k, p, ||D||} from the fp32-rounded D and v, exact sums (math.fsum), and the cancellation term of p:
    k per 2^-52 sum |v D| / sum D^2."""
    import math
    out, slack = [], []
    r, per = float(row[4]), D.shape[1]
    for b in range(D.shape[0]):
        d, w = D[b].astype(np.float64), v[b].astype(np.float64)
        svv, svd, sdd = math.fsum(w * w), math.fsum(w * d), math.fsum(d * d)
        nv = math.sqrt(svv)
        k = min(1.0, r / nv) if r != 0 and nv != 0 else 1.0
        out.append([nv, k, k * svd / sdd if sdd != 0 else 0.0, math.sqrt(sdd)])
        slack.append(k * per * 2.0 ** -52 * math.fsum(np.abs(w * d)) / sdd if sdd != 0 else 0.0)
    return np.array(out), np.array(slack)


def ulp32(a):
    """The spacing of fp32 at |a| (float64 array)."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    return np.where(a > 0, 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -126))) - 23), 2.0 ** -149)


def ulp16(a):
    """The spacing of fp16 at |a| (float64 array); subnormals: 2^-24."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    return 2.0 ** (np.maximum(np.floor(np.log2(np.maximum(a, 2.0 ** -14))), -14) - 10)


def fold_ref_and_bound(D, v, ec, fac, row):
    """(float64 reference, bound) per element of replica 0 from the fp32-rounded D and v, e_c and the KERNEL'S OWN fac (k and p as it
    wrote them): ref = e_c + ig (k v - q D) with q = fp32((1 - eta) p).  The bound counts the contract's roundings:
      k * v            one fp32 rounding:  2^-24 |k v|
      fmaf(-q, D, kv)  one:                2^-24 |nn|
      q itself is formed in fp64 from the unrounded p and rounded once; the reference rounds p first and then the product, so q can
                       differ by one fp32 ulp:  ulp32(q) |D|
      fmaf(nn, ig, e_c) one:               2^-24 |ref|         (the error of nn is carried through ig)
      fp16(...)        a rounding of its own:  ulp16(|ref| + e32) / 2"""
    k = fac[:, 1].astype(np.float64)[:, None]
    q32 = (np.float32(row[5]).astype(np.float64) * fac[:, 2].astype(np.float64)).astype(np.float32).astype(np.float64)[:, None]
    ig = float(row[2])
    D64, v64, ec64 = D.astype(np.float64), v.astype(np.float64), ec.astype(np.float64)
    kv = k * v64
    nn = kv - q32 * D64
    ref = ec64 + ig * nn
    e_nn = 2.0 ** -24 * (np.abs(kv) + np.abs(nn)) + ulp32(q32) * np.abs(D64)
    e32 = abs(ig) * e_nn + 2.0 ** -24 * np.abs(ref)
    return ref, e32 + 0.5 * ulp16(np.abs(ref) + e32)
