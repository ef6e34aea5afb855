"""FreeU restated in fp64 / fp32 on the CPU: the skip filter by torch.fft with the shifted mask (as diffusers writes it), the
seven-sum formula of include/vd_hip.h, the backbone scale, an oracle walk that applies FreeU in front of
torch.cat([h, hs.pop()], 1) by the width rule (with DeepCache's cut), the windowed prediction on it, and DDIM / DPM-Solver++(2M) /
SDE / UniPC loops driven by a sampler's own coefficient table.  Shared by the CPU and the GPU tests."""
import numpy as np
import torch

import deepcache_cases as dc
import window_cases as wc
from deepcache_cases import FWD_TOL, LATENT_TOL  # noqa: F401  (the project's bounds, re-exported for the tests)

from oracle import vd_oracle as O

SETTING = (1.2, 1.4, 0.9, 0.2)       # (b1, b2, s1, s2): the values the paper gives for SD 1.4
FULL_STAGES = (1280, 640, [0, 1, 2, 3, 4, 5, 6], [7, 8, 9])
TINY_STAGES = (128, 64, [0, 1, 2], [3])


def fourier_filter(x, threshold, scale):
    """diffusers' fourier_filter (utils/torch_utils.py) in the dtype of x [B, C, H, W]: fftn, fftshift, the mask with `scale` on
    [crow - threshold, crow + threshold) x [ccol - threshold, ccol + threshold), ifftshift, ifftn, the real part."""
    x_freq = torch.fft.fftn(x, dim=(-2, -1))
    x_freq = torch.fft.fftshift(x_freq, dim=(-2, -1))
    B, C, H, W = x_freq.shape
    mask = torch.ones((B, C, H, W), dtype=x.dtype)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    x_freq = x_freq * mask
    x_freq = torch.fft.ifftshift(x_freq, dim=(-2, -1))
    return torch.fft.ifftn(x_freq, dim=(-2, -1)).real


def seven_sums(x, s):
    """The written-out form of the contract on x [..., H, W] in float64, with float64 trig of the unreduced angles."""
    x = x.double()
    H, W = x.shape[-2:]
    th = (2.0 * np.pi * torch.arange(H, dtype=torch.float64) / H)[:, None]
    ph = (2.0 * np.pi * torch.arange(W, dtype=torch.float64) / W)[None, :]
    sm = lambda t: (x * t).sum((-2, -1), keepdim=True)
    one = torch.ones((H, W), dtype=torch.float64)
    g = (float(s) - 1.0) / (H * W)
    acc = sm(one) * one
    for t in (torch.cos(th) * one, torch.sin(th) * one, torch.cos(ph) * one, torch.sin(ph) * one, torch.cos(th + ph), torch.sin(th + ph)):
        acc = acc + sm(t) * t
    return x + g * acc


def backbone(h, b):
    """h [B, C, H, W] with its first C // 2 channels scaled by b (out of place, any dtype)."""
    out = h.clone()
    out[:, :h.shape[1] // 2] = out[:, :h.shape[1] // 2] * b
    return out


def apply(h, skip, b, s):
    """One stage on NCHW tensors in their own dtype (the oracle's fp32, or float64)."""
    return backbone(h, b), fourier_filter(skip, 1, s)


def entering_widths(plan):
    """The width of the h in front of every load of the plan's walk, in order: the output width of the data block before it."""
    ch, di, widths = None, 0, []
    for s in dc.flat_order(plan):
        if s == "d":
            ch = plan["data"][di][2]
            di += 1
        elif s == "load_hidden_feature":
            widths.append(ch)
    return widths


def stage_blocks(plan):
    """(W1, W2, output blocks of stage 1, of stage 2) by the width rule."""
    widths = entering_widths(plan)
    W1 = max(widths)
    return W1, W1 // 2, [i for i, w in enumerate(widths) if w == W1], [i for i, w in enumerate(widths) if w == W1 // 2]


def stage_map(plan, setting):
    """{width of the entering h: (b, s)} by the width rule, from the plan's own blocks: W1 = the widest h entering an output block."""
    if setting is None:
        return {}
    W1 = max(entering_widths(plan))
    b1, b2, s1, s2 = [float(v) for v in setting]
    return {W1: (b1, s1), W1 // 2: (b2, s2)}


def walk(sd, plan, x, t, contexts, setting=None, depth=None, cache=None, mode="full", x_type="image", record=None):
    """deepcache_cases.walk with FreeU in front of every concat: h, skip = apply(h, hs.pop(), b, s) where the entering width is a
    stage's.  In a cached walk the kept feature is the tensor in front of the load, un-scaled.  record: a list that receives the
    output-block index and stage (1, 2 or 0) of every load."""
    order = dc.flat_order(plan)
    emb = O.time_embed(sd, "diffuser.%s.time_embed" % x_type, O.timestep_embedding(t, plan["model_channels"]))
    ratios = np.array([float(r) for _, _, r in contexts])
    ratios = ratios / ratios.sum()
    stages = stage_map(plan, setting)
    widths = sorted(stages, reverse=True)
    kinds, di, ci = [], 0, 0
    for s in order:
        if s == "d":
            kinds.append(("d", di))
            di += 1
        elif s == "c":
            kinds.append(("c", ci))
            ci += 1
        else:
            kinds.append((s, None))
    first_load = [i for i, k in enumerate(kinds) if k[0] == "load_hidden_feature"][0]
    hs = []

    def run(lo, hi, h):
        for pos, (s, j) in list(enumerate(kinds))[lo:hi]:
            if s == "d":
                h = O._data_block(sd, "diffuser.%s.data_blocks.%d" % (x_type, j), plan["data"][j][0], h, emb)
            elif s == "c":
                out = None
                for (ct, c, _), r in zip(contexts, ratios):
                    hi_ = O.spatial_transformer(sd, "diffuser.%s.context_blocks.%d.0" % (ct, j), h, c, plan["ctx"][j][1])
                    if len(contexts) > 1:
                        hi_ = hi_ * float(r)
                    out = hi_ if out is None else out + hi_
                h = out
            elif s == "save_hidden_feature":
                hs.append(h)
            else:
                skip = hs.pop()
                bs = stages.get(h.shape[1])
                if record is not None:
                    k = sum(1 for q in kinds[first_load:pos] if q[0] == "load_hidden_feature")
                    record.append((k, 0 if bs is None else 1 + widths.index(h.shape[1])))
                if bs is not None:
                    h, skip = apply(h, skip, *bs)
                h = torch.cat([h, skip], 1)
        return h

    with torch.no_grad():
        if depth is None:
            return run(0, len(kinds), x)
        a, b = dc.cut(order, depth)
        if mode == "full":
            h = run(0, b, x)
            cache["f"] = h.clone()
            return run(b, len(kinds), h)
        assert mode == "shallow"
        run(0, a, x)
        return run(b, len(kinds), cache["f"])


def windowed_eps(sd, plan, x, t, ctx, geo, setting):
    """window_cases.windowed_eps with FreeU inside each window's forward."""
    rows = x.shape[0]
    wins = wc.gather_ref(x, geo["offs"], geo["h"], geo["w"], geo["wrap"])
    Wn = wins.shape[1]
    xb = wins.transpose(0, 1).reshape((Wn * rows,) + tuple(wins.shape[2:]))
    e = walk(sd, plan, xb, t.repeat(Wn), [(ct, c.repeat(Wn, 1, 1), r) for ct, c, r in ctx], setting)
    e = e.reshape((Wn, rows) + tuple(e.shape[1:])).transpose(0, 1)
    return wc.merge_ref64(e, geo["offs"], geo["wgt"], geo["inv_den"], geo["H"], geo["W"], geo["wrap"]).float()


def oracle_loop(sd, plan, sampler, kind, xT, contexts, scale, setting=None, interval=1, depth=1, geo=None, phi=0.0, noise=None):
    """The loop `sampler` ran last ("ddim", "2m", "sde" or "unipc") in fp32 on the oracle with FreeU in every forward, driven by
    the sampler's own coefficient table (deepcache_cases.oracle_loop's update formulas, restated).  interval / depth: DeepCache's
    schedule; geo: a window geometry (window_cases.geometry); phi: the guidance-rescale weight (ddim.cfg_rescale_factors);
    noise(draw) -> the step noise of kind "sde" (its table's column 7 is the noise coefficient)."""
    from lib.model_zoo.ddim import cfg_rescale_factors
    ts = sampler.ddim_timesteps
    S = len(ts)
    tab = sampler._coef_table(S, scale, torch.device("cpu")).double().numpy()
    guided = scale != 1.0
    cs = dc.cfg_contexts(contexts, guided)
    x = xT.float().cpu()
    cache = {}
    hist = xl = m1 = m2 = m3 = None
    for k, i in enumerate(reversed(range(S))):
        r = [float(v) for v in tab[i]]
        xin = torch.cat([x, x]) if guided else x
        t = torch.full((xin.shape[0],), int(ts[i]), dtype=torch.long)
        if geo is not None:
            eps = windowed_eps(sd, plan, xin, t, cs, geo, setting)
        elif interval == 1:
            eps = walk(sd, plan, xin, t, cs, setting)
        else:
            eps = walk(sd, plan, xin, t, cs, setting, depth=depth, cache=cache, mode="full" if k % interval == 0 else "shallow")
        if guided:
            e_u, e_c = eps.chunk(2)
            e = e_u + r[0] * (e_c - e_u)
            if phi > 0:
                kf = cfg_rescale_factors(eps, r[0], phi).float()
                e = e * kf.view(-1, *([1] * (e.dim() - 1)))
        else:
            e = eps
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
    return x


# ---- the op's cases ------------------------------------------------------------------------------------------------------------
EXACT_PLANES = [(2, 2), (4, 4), (2, 4)]
EXACT_S = [0.5, 0.0, 2.0]
EXACT_B = [1.5, 0.75]
# (H, W, C0, C1, B): every plane at C1 = 64 with C0 different and equal, every width once more on the smallest planes, both batches
BOUNDED = [(8, 8, 64, 64, 3), (16, 16, 128, 64, 1), (32, 32, 64, 64, 1), (8, 24, 24, 64, 3), (6, 10, 64, 64, 1),
           (8, 8, 64, 32, 3), (6, 10, 32, 32, 1), (16, 16, 320, 320, 1), (8, 8, 640, 320, 3), (8, 8, 1280, 1280, 3),
           (16, 16, 640, 1280, 1), (32, 32, 1280, 320, 1), (8, 24, 320, 320, 1), (6, 10, 1280, 1280, 1),
           # planes of more pixels than four rounds of a block's threads, odd and even
           (32, 33, 32, 32, 1), (32, 64, 64, 32, 3), (33, 63, 32, 32, 1), (64, 64, 32, 64, 1)]


def exact_ints(shape, seed):
    """fp16 integers in [-8, 8], seeded on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-8, 9, tuple(shape), generator=g).half()


def ulp16(v):
    """The fp16 spacing at magnitude v (float64 array): 2^(e - 10) with e = max(floor(log2 v), -14)."""
    v = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(v)) - 10)


def skip_bound(x_nchw, ref, s):
    """Per element of ref [B, C, H, W] (float64): e32 + ulp16(|ref| + e32) / 2 with e32 = 7 (H W + 16) 2^-23 |g| sum |x| over the
    element's plane -- fp32 summation of H W terms and the once-rounded tables, seven sums, one final rounding to fp16."""
    H, W = x_nchw.shape[-2:]
    g = abs(float(s) - 1.0) / (H * W)
    e32 = 7.0 * (H * W + 16) * 2.0 ** -23 * g * x_nchw.double().abs().sum((-2, -1), keepdim=True).numpy()
    e32 = np.broadcast_to(e32, ref.shape)
    return e32 + 0.5 * ulp16(np.abs(ref.numpy()) + e32)
