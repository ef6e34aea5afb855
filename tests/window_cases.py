"""Windowed (MultiDiffusion) sampling restated in torch on the CPU: the merge kernel's chain with its roundings written out, the
exact (float64) merge, the windowed prediction on the fp32 oracle (deepcache_cases.walk on the windows, merged), and DDIM /
DPM-Solver++(2M) / UniPC loops on it driven by a sampler's own coefficient table.  Shared by the CPU and the GPU tests."""
import numpy as np
import torch

import deepcache_cases as dc
from deepcache_cases import FWD_TOL, LATENT_TOL  # noqa: F401  (the project's bounds, re-exported for the tests)

from lib.model_zoo import windows


def geometry(H, W, window, stride, wrap=False, weight="uniform"):
    """The tables of lib/model_zoo/windows.py for one geometry: offsets int32 [Wn, 2], wgt fp32 [h, w], inv_den fp32 [H, W]."""
    offs = windows.window_offsets(H, W, window, stride, wrap)
    h, w = windows.int_pair("window", window)
    wgt = windows.window_weights(h, w, weight)
    return {"H": H, "W": W, "h": h, "w": w, "wrap": bool(wrap), "offs": offs, "wgt": wgt,
            "inv_den": windows.window_inv_den(H, W, offs, wgt, bool(wrap))}


def cols(ox, w, W, wrap):
    c = torch.arange(w) + int(ox)
    return c % W if wrap else c


def gather_ref(x, offs, h, w, wrap):
    """[B, Wn, C, h, w]: the windows of x [B, C, H, W] by torch indexing."""
    W = x.shape[-1]
    return torch.stack([x[:, :, int(oy):int(oy) + h][..., cols(ox, w, W, wrap)] for oy, ox in np.asarray(offs)], dim=1)


def merge_restated(eps_win, offs, wgt, inv_den, H, W, wrap):
    """fp16 [RB, C, H, W]: the contract of vd_window_merge_f16 on eps_win fp16 [RB, Wn, C, h, w] -- per canvas element the chain
    a = fmaf(wgt, eps, a) over the covering windows in ascending order (the product formed in float64, where fp32 x fp16 is
    exact; the sum rounded to fp32), then a * inv_den rounded to fp32, then to fp16."""
    RB, Wn, C, h, w = eps_win.shape
    wgt64 = torch.as_tensor(wgt).double()
    a = torch.zeros((RB, C, H, W), dtype=torch.float32)
    for k, (oy, ox) in enumerate(np.asarray(offs)):
        ys, xs = slice(int(oy), int(oy) + h), cols(ox, w, W, wrap)
        a[:, :, ys, xs] = (wgt64 * eps_win[:, k].double() + a[:, :, ys, xs].double()).float()
    return (a * torch.as_tensor(inv_den).float()).half()


def merge_ref64(eps_win, offs, wgt, inv_den, H, W, wrap):
    """float64 [RB, C, H, W]: (the sum of wgt x eps over the covering windows) x inv_den, every operation in float64."""
    RB, Wn, C, h, w = eps_win.shape
    wgt64 = torch.as_tensor(wgt).double()
    a = torch.zeros((RB, C, H, W), dtype=torch.float64)
    for k, (oy, ox) in enumerate(np.asarray(offs)):
        ys, xs = slice(int(oy), int(oy) + h), cols(ox, w, W, wrap)
        a[:, :, ys, xs] += wgt64 * eps_win[:, k].double()
    return a * torch.as_tensor(inv_den).double()


def windowed_eps(sd, plan, x, t, ctx, geo):
    """fp32 [rows, C, H, W]: the windowed prediction on the oracle.  x [rows, C, H, W] is the batch the UNet would see on the
    canvas ([x ; x] under guidance), t its timesteps, ctx [(type, c [rows, L, D], ratio)].  Every window of geo (geometry())
    goes through deepcache_cases.walk with its rows' contexts -- all windows in one batch, window-major -- and the predictions
    are merged in float64.  With one window this is the walk on x itself, bit for bit (1.0 e, times 1 / 1.0)."""
    rows = x.shape[0]
    wins = gather_ref(x, geo["offs"], geo["h"], geo["w"], geo["wrap"])                     # [rows, Wn, C, h, w]
    Wn = wins.shape[1]
    xb = wins.transpose(0, 1).reshape((Wn * rows,) + tuple(wins.shape[2:]))
    e = dc.walk(sd, plan, xb, t.repeat(Wn), [(ct, c.repeat(Wn, 1, 1), r) for ct, c, r in ctx])
    e = e.reshape((Wn, rows) + tuple(e.shape[1:])).transpose(0, 1)
    return merge_ref64(e, geo["offs"], geo["wgt"], geo["inv_den"], geo["H"], geo["W"], geo["wrap"]).float()


def oracle_loop(sd, plan, sampler, kind, xT, contexts, scale, geo):
    """The windowed loop `sampler` ran last ("ddim", "2m" or "unipc") in fp32 on the oracle, driven by the sampler's own
    coefficient table: deepcache_cases.oracle_loop's update formulas, restated, on the fused prediction of the canvas."""
    ts = sampler.ddim_timesteps
    S = len(ts)
    tab = sampler._coef_table(S, scale, torch.device("cpu")).double().numpy()
    guided = scale != 1.0
    cs = dc.cfg_contexts(contexts, guided)
    x = xT.float().cpu()
    hist = xl = m1 = m2 = m3 = None
    for i in reversed(range(S)):
        r = [float(v) for v in tab[i]]
        xin = torch.cat([x, x]) if guided else x
        eps = windowed_eps(sd, plan, xin, torch.full((xin.shape[0],), int(ts[i]), dtype=torch.long), cs, geo)
        if guided:
            e_u, e_c = eps.chunk(2)
            e = e_u + r[0] * (e_c - e_u)
        else:
            e = eps
        if kind == "ddim":      # {scale, 1/sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev - sigma^2), sigma, sqrt(1 - a_t)}
            p0 = (x - r[5] * e) * r[1]
            x = r[2] * p0 + r[3] * e
        elif kind == "2m":      # {scale, 1/sqrt(a_t), sqrt(1 - a_t), sigma_next/sigma_t, c_d, w_cur, w_prev, 0}
            p0 = (x - r[2] * e) * r[1]
            d = r[5] * p0 + (r[6] * hist if r[6] != 0 else 0.0)
            x, hist = r[3] * x + r[4] * d, p0
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
    return x
