"""Perturbed-attention guidance (Ahn et al. 2024; diffusers' pag_scale / pag_applied_layers) restated in fp32 on the CPU oracle: a
walk built from oracle.vd_oracle's blocks in which the chosen context blocks replace the self-attention map of the perturbed rows by
the identity, attn1 = to_out(to_v(norm1(h))), the windowed prediction on it, the fold's formula in float64 with its per-element
bound, and DDIM / DPM-Solver++(2M) / SDE / UniPC loops driven by a sampler's own coefficient table that form
e_u + s (e_c - e_u) + s_pag (e_c - e_p) (or e_c + s_pag (e_c - e_p)) in fp32.  Shared by the CPU and the GPU tests."""
import numpy as np
import torch
import torch.nn.functional as F

import deepcache_cases as dc
import freeu_cases as fc
import window_cases as wc
from deepcache_cases import FWD_TOL, LATENT_TOL  # noqa: F401  (the project's bounds, re-exported for the tests)

from oracle import vd_oracle as O

PAG_SCALE = 3.0           # diffusers' documented default for pag_scale
TINY_BLOCKS, TINY_MID = 7, 2
FULL_BLOCKS, FULL_MID = 16, 6
LAYER_CASES = ["mid", (1, 2, 3), (0,)]


def layers_of(plan, layers):
    """The normalised tuple of a pag_layers value on the plan's walk: "mid" is the middle stage's context block."""
    if layers == "mid":
        return (sum(s == "c" for s in plan["i_order"]),)
    return tuple(sorted(int(v) for v in layers))


def spatial_transformer(sd, p, x, context, heads, perturbed):
    """oracle.vd_oracle.spatial_transformer with the rows of the bool vector `perturbed` taking the identity attention map in the
    block's self-attention: attn1 = to_out(to_v(norm1(h))); the other rows take the softmax path."""
    b, c, hh, ww = x.shape
    h = O._conv(sd, p + ".proj_in", O._gn(sd, p + ".norm", x, 1e-6)).flatten(2).transpose(1, 2)
    q = p + ".transformer_blocks.0"
    w = h.shape[-1]
    ln = lambda name, t: F.layer_norm(t, (w,), sd[q + "." + name + ".weight"], sd[q + "." + name + ".bias"], 1e-5)
    n1 = ln("norm1", h)
    a1 = torch.empty_like(h)
    keep = ~perturbed
    if bool(keep.any()):
        a1[keep] = O.cross_attention(sd, q + ".attn1", n1[keep], None, heads)
    if bool(perturbed.any()):
        a1[perturbed] = O._lin(sd, q + ".attn1.to_out.0", F.linear(n1[perturbed], sd[q + ".attn1.to_v.weight"]))
    h = a1 + h
    h = O.cross_attention(sd, q + ".attn2", ln("norm2", h), context, heads) + h
    v, gate = O._lin(sd, q + ".ff.net.0.proj", ln("norm3", h)).chunk(2, dim=-1)
    h = O._lin(sd, q + ".ff.net.2", v * F.gelu(gate)) + h
    return O._conv(sd, p + ".proj_out", h.transpose(1, 2).reshape(b, c, hh, ww)) + x


def walk(sd, plan, x, t, contexts, layers=(), perturbed=None, setting=None, x_type="image", record=None):
    """The UNet on x [rows, C, H, W] at timesteps t with contexts [(type, c, ratio), ...]: deepcache_cases.walk (with FreeU in front
    of every concat when `setting` is given, freeu_cases' rule) in which a context block whose walk index is in `layers` runs the
    rows of the bool vector `perturbed` with identity self-attention -- every context type's block at that index.  record: a list
    that receives the walk index of every context block that perturbed some row."""
    order = dc.flat_order(plan)
    emb = O.time_embed(sd, "diffuser.%s.time_embed" % x_type, O.timestep_embedding(t, plan["model_channels"]))
    ratios = np.array([float(r) for _, _, r in contexts])
    ratios = ratios / ratios.sum()
    stages = fc.stage_map(plan, setting)
    if perturbed is None:
        perturbed = torch.zeros((x.shape[0],), dtype=torch.bool)
    h, hs, di, ci = x, [], 0, 0
    with torch.no_grad():
        for s in order:
            if s == "d":
                h = O._data_block(sd, "diffuser.%s.data_blocks.%d" % (x_type, di), plan["data"][di][0], h, emb)
                di += 1
            elif s == "c":
                on = ci in layers and bool(perturbed.any())
                if on and record is not None:
                    record.append(ci)
                out = None
                for (ct, c, _), r in zip(contexts, ratios):
                    p = "diffuser.%s.context_blocks.%d.0" % (ct, ci)
                    hi = spatial_transformer(sd, p, h, c, plan["ctx"][ci][1], perturbed) if on else \
                        O.spatial_transformer(sd, p, h, c, plan["ctx"][ci][1])
                    if len(contexts) > 1:
                        hi = hi * float(r)
                    out = hi if out is None else out + hi
                h = out
                ci += 1
            elif s == "save_hidden_feature":
                hs.append(h)
            else:
                skip = hs.pop()
                bs = stages.get(h.shape[1])
                if bs is not None:
                    h, skip = fc.apply(h, skip, *bs)
                h = torch.cat([h, skip], 1)
    return h


def windowed_eps(sd, plan, x, t, ctx, geo, layers, perturbed, setting=None):
    """window_cases.windowed_eps on the walk above: every window of a perturbed row is perturbed."""
    rows = x.shape[0]
    wins = wc.gather_ref(x, geo["offs"], geo["h"], geo["w"], geo["wrap"])
    Wn = wins.shape[1]
    xb = wins.transpose(0, 1).reshape((Wn * rows,) + tuple(wins.shape[2:]))
    e = walk(sd, plan, xb, t.repeat(Wn), [(ct, c.repeat(Wn, 1, 1), r) for ct, c, r in ctx], layers, perturbed.repeat(Wn), setting)
    e = e.reshape((Wn, rows) + tuple(e.shape[1:])).transpose(0, 1)
    return wc.merge_ref64(e, geo["offs"], geo["wgt"], geo["inv_den"], geo["H"], geo["W"], geo["wrap"]).float()


def replicas(x, ctx, guided, pag):
    """(the batch the UNet sees, its contexts, the bool vector of its perturbed rows) for the latent x [B, ...] and the contexts
    [(type, c, ratio)] of deepcache_cases.cfg_contexts ([uncond ; cond] rows when guided): with pag one more replica at the end
    that carries the conditional context."""
    B = x.shape[0]
    reps = (2 if guided else 1) + (1 if pag else 0)
    cs = [(ct, torch.cat([c, c[-B:]]) if pag else c, r) for ct, c, r in ctx]
    mask = torch.zeros((reps * B,), dtype=torch.bool)
    if pag:
        mask[-B:] = True
    return torch.cat([x] * reps), cs, mask


def combine(eps, scale, pag_scale, guided, pag, phi=0.0):
    """fp32 [B, ...]: e_u + s (e_c - e_u) + s_pag (e_c - e_p) of eps = [e_u ; e_c ; e_p] (the guided term dropped when unguided,
    the pag term when off), and with phi > 0 diffusers' rescale_noise_cfg(e, e_c, phi): e (phi std(e_c) / std(e) + 1 - phi), the
    standard deviations per sample in float64."""
    parts = list(eps.chunk((2 if guided else 1) + (1 if pag else 0)))
    e_p = parts.pop() if pag else None
    e_c = parts[-1]
    e = e_c if not guided else parts[0] + scale * (e_c - parts[0])
    if pag:
        e = e + pag_scale * (e_c - e_p)
    if phi > 0 and guided:
        sd_ = lambda v: v.double().flatten(1).std(1, unbiased=False)
        k = float(np.float32(phi)) * (sd_(e_c) / sd_(e)) + (1.0 - float(np.float32(phi)))
        e = e * k.float().view(-1, *([1] * (e.dim() - 1)))
    return e


def oracle_loop(sd, plan, sampler, kind, xT, contexts, scale, pag_scale=0.0, layers="mid", setting=None, geo=None, phi=0.0,
                noise=None):
    """The loop `sampler` ran last ("ddim", "2m", "sde" or "unipc") in fp32 on the oracle with perturbed-attention guidance of
    weight pag_scale (0: off, two or one replicas) in the context blocks `layers`, driven by the sampler's own coefficient table
    (deepcache_cases.oracle_loop's update formulas, restated).  setting: FreeU in every forward; geo: a window geometry
    (window_cases.geometry); phi: the guidance-rescale weight; noise(draw) -> the step noise of kind "sde"."""
    ts = sampler.ddim_timesteps
    S = len(ts)
    tab = sampler._coef_table(S, scale, torch.device("cpu")).double().numpy()
    guided, pag = scale != 1.0, pag_scale > 0
    lay = layers_of(plan, layers) if pag else ()
    cs0 = dc.cfg_contexts(contexts, guided)
    x = xT.float().cpu()
    hist = xl = m1 = m2 = m3 = None
    for k, i in enumerate(reversed(range(S))):
        r = [float(v) for v in tab[i]]
        xin, cs, mask = replicas(x, cs0, guided, pag)
        t = torch.full((xin.shape[0],), int(ts[i]), dtype=torch.long)
        if geo is not None:
            eps = windowed_eps(sd, plan, xin, t, cs, geo, lay, mask, setting)
        else:
            eps = walk(sd, plan, xin, t, cs, lay, mask, setting)
        e = combine(eps, r[0], float(pag_scale), guided, pag, phi)
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


# ---- the two entries' cases ----------------------------------------------------------------------------------------------------
IDENT_DIMS = [40, 64, 80, 160]
IDENT_HEADS = [1, 2]
IDENT_ROWS = [64, 96, 256]
FOLD_WEIGHTS = [-0.5, 0.25, 2.0, -1.0]
# per-replica element counts: below one vector, odd, a multiple of 8 below and above a block's 2048, not a multiple of 8, > 2^20
FOLD_SIZES = [5, 8, 1000, 2048 + 8, 4099, 3 * 8192 + 3, (1 << 20) + 24]


def fold_ref64(eps, reps, w):
    """float64 [n]: fp32(a) + w (c - p) of eps [reps, n] (fp16) with w rounded to fp32 -- the exact value the fold approximates."""
    e = eps.double()
    return e[0] + float(np.float32(w)) * (e[reps - 2] - e[reps - 1])


def fold_bound(eps, reps, w):
    """Per element: e32 + ulp16(|ref| + e32) / 2 with e32 = 2^-23 (|a| + 2 |w d|) -- the fp32 subtraction (exact for fp16 operands
    within 2^24 of each other's scale, else one rounding of d), the fma's one rounding, and the rounding to fp16 of its own."""
    e = eps.double()
    wd = np.abs(float(np.float32(w)) * (e[reps - 2] - e[reps - 1]).numpy())
    e32 = 2.0 ** -23 * (np.abs(e[0].numpy()) + 2.0 * wd)
    return e32 + 0.5 * fc.ulp16(np.abs(fold_ref64(eps, reps, w).numpy()) + e32)
