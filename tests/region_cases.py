"""Regional prompts on the windowed path restated in torch on the CPU: the masked merge kernel's chain with its roundings
written out, the exact (float64) regional merge, the regional prediction on the fp32 oracle (deepcache_cases.walk per (region,
window), merged in float64) and the oracle loops of tests/window_cases.py driven by it.  Shared by the CPU and the GPU tests."""
from unittest import mock

import numpy as np
import torch

import deepcache_cases as dc
import window_cases as wc
from window_cases import FWD_TOL, LATENT_TOL  # noqa: F401  (the project's bounds, re-exported for the tests)

from lib.model_zoo import windows


def half_masks(H, W, split=None):
    """fp32 [2, H, W]: region 0 owns the columns left of `split` (default W // 2), region 1 the rest; hard and complementary."""
    split = W // 2 if split is None else split
    m = np.zeros((2, H, W), dtype=np.float32)
    m[0, :, :split] = 1.0
    m[1, :, split:] = 1.0
    return m


def geometry(H, W, window, stride, masks, wrap=False, weight="uniform"):
    """window_cases.geometry plus "masks" fp32 [R, H, W] (windows.region_masks_arg) and, as "inv_den", windows.region_inv_den."""
    geo = wc.geometry(H, W, window, stride, wrap, weight)
    masks = windows.region_masks_arg(masks, H, W)
    return dict(geo, masks=masks, inv_den=windows.region_inv_den(H, W, geo["offs"], geo["wgt"], masks, bool(wrap)))


def _terms(eps_wins, offs, wgt, masks, W, wrap):
    """(r, k, ys, xs, wm fp32 [h, w], on bool [h, w], eps_wins[r][:, k]) in the kernel's order: region-major, windows ascending."""
    wgt32 = torch.as_tensor(wgt).float()
    h, w = wgt32.shape
    for r, e in enumerate(eps_wins):
        mask = torch.as_tensor(masks[r]).float()
        for k, (oy, ox) in enumerate(np.asarray(offs)):
            ys, xs = slice(int(oy), int(oy) + h), wc.cols(ox, w, W, wrap)
            mv = mask[ys][:, xs]
            yield r, k, ys, xs, wgt32 * mv, mv != 0, e[:, k]                    # wm: one fp32 multiply, rounded once


def merge_masked_restated(eps_wins, offs, wgt, masks, inv_den, H, W, wrap):
    """fp16 [RB, C, H, W]: the contract of vd_window_merge_masked_f16 over all launches of a step on eps_wins, R tensors fp16
    [RB, Wn, C, h, w] -- per canvas element a = fmaf(wm, eps, a) with wm = fp32(wgt x mask_r), region-major and inside a region
    in ascending window order, skipped where mask_r is 0 (the product formed in float64, where fp32 x fp16 is exact; the sum
    rounded to fp32), then a * inv_den rounded to fp32, then to fp16."""
    RB, _, C = eps_wins[0].shape[:3]
    a = torch.zeros((RB, C, H, W), dtype=torch.float32)
    for _, _, ys, xs, wm, on, e in _terms(eps_wins, offs, wgt, masks, W, wrap):
        old = a[:, :, ys, xs]
        a[:, :, ys, xs] = torch.where(on, (wm.double() * e.double() + old.double()).float(), old)
    return (a * torch.as_tensor(inv_den).float()).half()


def merge_masked_ref64(eps_wins, offs, wgt, masks, inv_den, H, W, wrap):
    """float64 [RB, C, H, W]: (the sum over regions and covering windows of wm x eps, where mask_r is not 0) x inv_den, every
    operation after wm = fp32(wgt x mask_r) in float64."""
    RB, _, C = eps_wins[0].shape[:3]
    a = torch.zeros((RB, C, H, W), dtype=torch.float64)
    for _, _, ys, xs, wm, on, e in _terms(eps_wins, offs, wgt, masks, W, wrap):
        a[:, :, ys, xs] += torch.where(on, wm.double() * e.double(), torch.zeros((), dtype=torch.float64))
    return a * torch.as_tensor(inv_den).double()


def window_preds(sd, plan, x, t, ctx, geo):
    """fp32 [rows, Wn, C, h, w]: the oracle's prediction on every window of x [rows, C, H, W] with the rows' contexts ctx
    [(type, c [rows, L, D], ratio)] -- window_cases.windowed_eps before its merge."""
    rows = x.shape[0]
    wins = wc.gather_ref(x, geo["offs"], geo["h"], geo["w"], geo["wrap"])
    Wn = wins.shape[1]
    xb = wins.transpose(0, 1).reshape((Wn * rows,) + tuple(wins.shape[2:]))
    e = dc.walk(sd, plan, xb, t.repeat(Wn), [(ct, c.repeat(Wn, 1, 1), r) for ct, c, r in ctx])
    return e.reshape((Wn, rows) + tuple(e.shape[1:])).transpose(0, 1)


def regional_eps(sd, plan, x, t, region_ctx, geo):
    """fp32 [rows, C, H, W]: the regional prediction on the oracle: region_ctx[r] is region r's [(type, c, ratio)] for the rows
    of x; every (region, window) goes through the oracle and the predictions are merged in float64 with geo["masks"]."""
    e = [window_preds(sd, plan, x, t, ctx, geo) for ctx in region_ctx]
    return merge_masked_ref64(e, geo["offs"], geo["wgt"], geo["masks"], geo["inv_den"], geo["H"], geo["W"], geo["wrap"]).float()


def oracle_loop(sd, plan, sampler, kind, xT, region_contexts, scale, geo):
    """window_cases.oracle_loop on the regional prediction: region_contexts[r] is the list of sampler-style context dicts of
    region r (the guidance scale is one for all).  The loop's update formulas are window_cases' own; only the prediction it
    calls is replaced for the duration of the loop."""
    guided = scale != 1.0
    region_ctx = [dc.cfg_contexts(cs, guided) for cs in region_contexts]
    eps = lambda sd_, plan_, xin, t, cs, geo_: regional_eps(sd, plan, xin, t, region_ctx, geo)
    with mock.patch.object(wc, "windowed_eps", eps):
        return wc.oracle_loop(sd, plan, sampler, kind, xT, region_contexts[0], scale, geo)
