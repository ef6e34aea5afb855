"""Self-attention guidance (Hong et al., ICCV 2023; diffusers' StableDiffusionSAGPipeline) restated on the CPU oracle: the column
mass of a self-attention map, the mask, the reflected 9-tap blur, the re-noising and the fold in float64 with their per-element
bounds, a walk built from oracle.vd_oracle's blocks whose middle context block also returns the attn1 probabilities' column mass,
and DDIM / DPM-Solver++(2M) / SDE / UniPC loops driven by a sampler's own coefficient table that run the two forwards of a step and
form e_u + s (e_c - e_u) + s_sag (e0 - e_d) in fp32.  Shared by the CPU and the GPU tests."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import attn_cases as ac
import deepcache_cases as dc
import freeu_cases as fc
import pag_cases as pc
from deepcache_cases import FWD_TOL, LATENT_TOL  # noqa: F401  (the project's bounds, re-exported for the tests)

from oracle import vd_oracle as O

SAG_SCALE = 0.75          # diffusers' documented default for sag_scale
SIGMA = 1.0               # ... and the sigma of its gaussian_blur_2d(kernel_size=9, sigma=1.0)
# The issue asks for 3 steps; the samplers' uniform schedule only takes step counts that divide the 1000 training steps (1000 // 3
# = 333 puts its last timestep at index 1000), so the loops run the next count that can be scheduled.
STEPS = 4
SHAPE = [2, 4, 16, 16]    # the forward tests
TINY_MAP = (8, 8)         # the middle block's token grid of the tiny net on a 16 x 16 latent
# The loop tests: one sample on an 8 x 8 latent, 16 middle tokens -- the fewest masses that can come near the threshold.
LOOP_SHAPE = [1, 4, 8, 8]
LOOP_KINDS = ("ddim", "2m", "sde", "unipc")
LOOP_SCALES = (7.5, 1.0)
LOOP_SEEDS = [41]         # the SDE sampler's noise seeds
# The input seed of every loop case: the first seed from 0 on at which no combined column mass of the oracle loop comes within 1.5
# MASS_MARGIN of the threshold (searched on the CPU oracle alone; test_sag_cpu.py asserts MASS_MARGIN itself for each).
LOOP_SEED = {("ddim", 7.5): 53, ("ddim", 1.0): 23, ("2m", 7.5): 32, ("2m", 1.0): 23, ("sde", 7.5): 5, ("sde", 1.0): 1, ("unipc", 7.5): 32,
             ("unipc", 1.0): 23, "rescale": 1, "inpaint": 18, "freeu": 32}
# The tests scale the middle attn1.to_q.weight of every context type by this factor, for the device net and the oracle alike
# (sharpen): 1.0 leaves the synthetic weights as they are.
SHARPEN = 1.0
# Largest |device mass - oracle mass| over the forward tests (fp16 weights and activations against the fp32 oracle), measured:
# 2.53e-3 (test_sag_gpu.test_forward_keeps_its_bits_and_writes_the_mass_of_the_middle_attn1: dual context, unguided, the image
# type's block; 2.05e-3 single context), rounded up.  The margin the loop tests ask for around the threshold is four times that.
MASS_DIFF_MEASURED = 2.6e-3
MASS_MARGIN = 4 * MASS_DIFF_MEASURED


def loop_inputs(case):
    """(xT [1, 4, 8, 8], c, u [1, 77, 128]) of the loop case `case` (a key of LOOP_SEED), fp16-representable fp32, seeded."""
    g = torch.Generator().manual_seed(LOOP_SEED[case])
    return (torch.randn(LOOP_SHAPE, generator=g).half().float(), (torch.randn((1, 77, 128), generator=g) * 0.5).half().float(),
            (torch.randn((1, 77, 128), generator=g) * 0.5).half().float())


def loop_context(case, scale, **kw):
    _, c, u = loop_inputs(case)
    return dict({"type": "text", "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale}, **kw)


def loop_inpaint():
    """(x0, mask [1, 1, 8, 8] with the upper three rows known) of the inpainting loop case; the blend noise is xT."""
    x0 = (torch.randn(LOOP_SHAPE, generator=torch.Generator().manual_seed(4)) * 0.5).half().float()
    mask = torch.ones((1, 1, 8, 8))
    mask[..., :3, :] = 0
    return x0, mask


def sde_noise():
    from test_philox_cpu import normals_ref_batch
    per = int(np.prod(LOOP_SHAPE[1:]))
    return lambda draw: torch.from_numpy(normals_ref_batch(LOOP_SEEDS, per, draw, 2))


# ---- the definition, in float64 ------------------------------------------------------------------------------------------------
def taps(sigma=SIGMA):
    """float64 [9]: g[k] = exp(-((k - 4) / sigma)^2 / 2) / sum."""
    g = np.exp(-0.5 * ((np.arange(9, dtype=np.float64) - 4.0) / float(sigma)) ** 2)
    return g / g.sum()


def refl(i, n):
    """torch's 'reflect' padding index, no edge repeat: -1 -> 1, n -> n - 2."""
    i = np.asarray(i)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def nearest(H, W, Hm, Wm):
    """int64 [H, W]: the token ((y Hm) // H) Wm + (x Wm) // W under every latent pixel."""
    y, x = np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64)
    return ((y * Hm) // H)[:, None] * Wm + ((x * Wm) // W)[None, :]


def coef_of(a):
    """{sa, s1, isa} in float64 for alphas_cumprod[t] = a."""
    a = float(a)
    return np.sqrt(a), np.sqrt(1.0 - a), 1.0 / np.sqrt(a)


def mass_ref64(q, k, H, scale=None):
    """float64 [B, N]: (1 / H) sum_h sum_i softmax_j(scale q_i . k_j) of q, k [B, N, H D] -- the sum over queries, per key."""
    B, N, C = q.shape
    D = C // H
    scale = D ** -0.5 if scale is None else scale
    qd = q.double().reshape(B, N, H, D).permute(0, 2, 1, 3)
    kd = k.double().reshape(B, N, H, D).permute(0, 2, 1, 3)
    P = torch.softmax(qd @ kd.transpose(-1, -2) * scale, -1)
    return P.sum(2).mean(1)


def mass_bound(ref):
    """|got - ref| <= 2^-16 max(1, ref): the fp32 score error is <= 8 * 2^-23, exp adds a few ulp (< 2^-19 relative per term), the
    sums are of non-negative terms; eightfold margin, and a structural error is >= 1 / H."""
    return 2.0 ** -16 * np.maximum(1.0, np.asarray(ref, dtype=np.float64))


def combined_mass(mass, ratio):
    """fp32 [B, Nm]: m = fma(r_t, mass_t, m) for t ascending from 0 on fp32 operands (the products are exact in float64; the test
    masses keep the sums exact too)."""
    m = np.zeros(mass.shape[1:], dtype=np.float32)
    for t in range(mass.shape[0]):
        m = (np.float64(np.float32(ratio[t])) * mass[t].astype(np.float32).astype(np.float64) + m.astype(np.float64)).astype(np.float32)
    return m


def blur64(p0, g):
    """float64: sum_i sum_j g[i] g[j] p0[refl(y + i - 4), refl(x + j - 4)] on [..., H, W]."""
    H, W = p0.shape[-2:]
    iy = refl(np.arange(H)[:, None] + np.arange(9)[None, :] - 4, H)       # [H, 9]
    ix = refl(np.arange(W)[:, None] + np.arange(9)[None, :] - 4, W)
    row = (p0[..., :, ix] * g).sum(-1)                                    # [..., H, W]
    return (row[..., iy, :] * g[:, None]).sum(-2)


def degrade_ref64(x, eps, mass, ratio, sigma, a, Hm, Wm):
    """(xd, A, mask) in float64 for fp16 x, eps [B, C, H, W], fp32 mass [T, B, Hm Wm], ratio [T]: the degraded latent before its
    rounding to fp16, the absolute sum A = sa sum g g |p0| + s1 |e| its fp32 evaluation is bounded with, and the pixel mask."""
    sa, s1, isa = (float(np.float32(v)) for v in coef_of(a))
    g = np.float32(taps(sigma)).astype(np.float64)
    xd_, ed = x.double().numpy(), eps.double().numpy()
    B, C, H, W = xd_.shape
    M = combined_mass(np.asarray(mass), np.asarray(ratio)) > np.float32(1.0)            # [B, Nm]
    Mpx = M[:, nearest(H, W, Hm, Wm)]                                                   # [B, H, W]
    p0 = (xd_ - s1 * ed) * isa
    d = np.where(Mpx[:, None], blur64(p0, g), p0)
    absd = np.where(Mpx[:, None], blur64(np.abs(p0), g), np.abs(p0))
    return sa * d + s1 * ed, sa * absd + s1 * np.abs(ed), Mpx


def degrade_bound(ref, A):
    """Per element: 2^-11 |ref| + 2^-24 (the rounding to fp16) + 2^-17 A (about 25 fp32 operations on the absolute sum, 4x margin)."""
    return 2.0 ** -11 * np.abs(ref) + 2.0 ** -24 + 2.0 ** -17 * A


def fold_ref64(a, d, w):
    """float64: a + w (a - d) with w rounded to fp32 -- for integer-valued fp16 operands and the test weights an fp16 value."""
    return a.double() + float(np.float32(w)) * (a.double() - d.double())


# ---- the cases of the three entries ----------------------------------------------------------------------------------------------
MASS_SHAPES = [(2, 3, 64, 64), (1, 2, 70, 40), (2, 8, 144, 160), (1, 2, 257, 80), (2, 2, 1024, 40)]      # (B, H, N, D)
MASS_KINDS = ("uniform", "selector", "random")
DEGRADE_SHAPES = [(2, 4, 8, 8, 2, 2), (1, 4, 16, 24, 2, 3), (1, 4, 20, 20, 3, 3), (1, 4, 64, 96, 8, 12), (1, 3, 5, 5, 1, 1)]
DEGRADE_REFUSED = (1, 4, 4, 8, 1, 1)
DEGRADE_RATIOS = [(1.0,), (0.5, 0.5), (0.25, 0.75)]
DEGRADE_MASSES = np.array([0.0, 0.5, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), 2.0], dtype=np.float32)
DEGRADE_ALPHA = 0.3


@functools.lru_cache(maxsize=None)
def mass_case(shape, kind):
    """(q, k fp16 [B, N, H D], float64 reference [B, N], selector counts or None) of one operand family, seeded."""
    B, H, N, D = shape
    rng = np.random.default_rng(900 + 7 * MASS_SHAPES.index(shape) + MASS_KINDS.index(kind))
    counts = None
    if kind == "uniform":
        q = np.zeros((B, N, H, D), np.float32)
        k = rng.standard_normal((B, N, H, D)).astype(np.float32)
        counts = None
    elif kind == "selector":
        book = ac.codebook(N, D, D // 4)
        g = ac.gain(D)
        q, k = np.empty((B, N, H, D), np.float32), np.empty((B, N, H, D), np.float32)
        counts = np.zeros((B, H, N), np.int64)
        for b in range(B):
            for h in range(H):
                codes = book[rng.permutation(N)][:, rng.permutation(D)]
                pi = rng.integers(0, max(N // 2, 1), N)            # some keys several times, the upper half never ...
                pi[::7] = N - 1 - (np.arange(len(pi[::7])) % 3)    # ... except the last three, in other tiles than their queries
                k[b, :, h] = codes
                q[b, :, h] = g * codes[pi]
                counts[b, h] = np.bincount(pi, minlength=N)
    else:
        q = rng.standard_normal((B, N, H, D)).astype(np.float32)
        k = rng.standard_normal((B, N, H, D)).astype(np.float32)
    q = torch.from_numpy(q.reshape(B, N, H * D)).half()
    k = torch.from_numpy(k.reshape(B, N, H * D)).half()
    if kind == "random":      # |scale q . k| <= 8: shrink q by a power of two where a logit is larger
        qd = q.double().reshape(B, N, H, D).permute(0, 2, 1, 3)
        kd = k.double().reshape(B, N, H, D).permute(0, 2, 1, 3)
        top = float((qd @ kd.transpose(-1, -2)).abs().max()) * D ** -0.5
        while top > 8.0:
            q, top = q * 0.5, top * 0.5
    return q, k, mass_ref64(q, k, H), counts


@functools.lru_cache(maxsize=None)
def degrade_case(shape, T, sigma, fill=None):
    """(x, eps fp16, mass fp32 [T, B, Nm]) of one degrade case, seeded; fill: None (masses drawn from DEGRADE_MASSES),
    0.0 (an all-zero mask) or 2.0 (an all-one mask)."""
    B, C, H, W, Hm, Wm = shape
    g = torch.Generator().manual_seed(500 + 11 * DEGRADE_SHAPES.index(shape) + T + int(sigma * 2))
    x = torch.randn((B, C, H, W), generator=g).half()
    eps = torch.randn((B, C, H, W), generator=g).half()
    rng = np.random.default_rng(int(g.initial_seed()))
    if fill is None:
        mass = DEGRADE_MASSES[rng.integers(0, len(DEGRADE_MASSES), (T, B, Hm * Wm))]
        if Hm * Wm > 1:       # at least one masked and one unmasked cell per sample, whatever was drawn
            mass[:, :, 0], mass[:, :, -1] = 2.0, 0.0
    else:
        mass = np.full((T, B, Hm * Wm), fill, np.float32)
    return x, eps, mass


# ---- the walk with the middle block's column mass --------------------------------------------------------------------------------
def sharpen(sd, plan, factor=SHARPEN, types=("text", "image")):
    """A copy of the state dict with the middle context block's attn1.to_q.weight of every context type scaled by `factor`."""
    mid = sum(s == "c" for s in plan["i_order"])
    out = dict(sd)
    for ct in types:
        key = "diffuser.%s.context_blocks.%d.0.transformer_blocks.0.attn1.to_q.weight" % (ct, mid)
        if key in out:
            out[key] = out[key] * float(factor)
    return out


def spatial_transformer(sd, p, x, context, heads):
    """oracle.vd_oracle.spatial_transformer, restated, that also returns the column mass [B, N] of its attn1 probabilities (the sum
    over queries, per key, the mean over heads), in float64 from the fp32 q and k."""
    b, c, hh, ww = x.shape
    h = O._conv(sd, p + ".proj_in", O._gn(sd, p + ".norm", x, 1e-6)).flatten(2).transpose(1, 2)
    q = p + ".transformer_blocks.0"
    w = h.shape[-1]
    ln = lambda name, t: F.layer_norm(t, (w,), sd[q + "." + name + ".weight"], sd[q + "." + name + ".bias"], 1e-5)
    n1 = ln("norm1", h)
    mass = mass_ref64(F.linear(n1, sd[q + ".attn1.to_q.weight"]), F.linear(n1, sd[q + ".attn1.to_k.weight"]), heads)
    h = O.cross_attention(sd, q + ".attn1", n1, None, heads) + h
    h = O.cross_attention(sd, q + ".attn2", ln("norm2", h), context, heads) + h
    v, gate = O._lin(sd, q + ".ff.net.0.proj", ln("norm3", h)).chunk(2, dim=-1)
    h = O._lin(sd, q + ".ff.net.2", v * F.gelu(gate)) + h
    return O._conv(sd, p + ".proj_out", h.transpose(1, 2).reshape(b, c, hh, ww)) + x, mass


def walk(sd, plan, x, t, contexts, setting=None, x_type="image"):
    """(eps, masses): pag_cases.walk without perturbed rows whose middle context block also returns, per context type, the column
    mass float64 [rows, Nm] of its attn1 (masses is a list with one entry per type) and the block's token grid."""
    order = dc.flat_order(plan)
    mid = sum(s == "c" for s in plan["i_order"])
    emb = O.time_embed(sd, "diffuser.%s.time_embed" % x_type, O.timestep_embedding(t, plan["model_channels"]))
    ratios = np.array([float(r) for _, _, r in contexts])
    ratios = ratios / ratios.sum()
    stages = fc.stage_map(plan, setting)
    h, hs, di, ci, masses, grid = x, [], 0, 0, None, None
    with torch.no_grad():
        for s in order:
            if s == "d":
                h = O._data_block(sd, "diffuser.%s.data_blocks.%d" % (x_type, di), plan["data"][di][0], h, emb)
                di += 1
            elif s == "c":
                out = None
                if ci == mid:
                    masses, grid = [], tuple(h.shape[2:])
                for (ct, c, _), r in zip(contexts, ratios):
                    p = "diffuser.%s.context_blocks.%d.0" % (ct, ci)
                    if ci == mid:
                        hi, m = spatial_transformer(sd, p, h, c, plan["ctx"][ci][1])
                        masses.append(m)
                    else:
                        hi = O.spatial_transformer(sd, p, h, c, plan["ctx"][ci][1])
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
    return h, masses, grid


def blur32(p0, sigma):
    """fp32 torch: F.pad(mode='reflect') and the two 1-D convolutions of diffusers' gaussian_blur_2d at kernel size 9."""
    g = torch.from_numpy(taps(sigma)).float()
    C = p0.shape[1]
    xp = F.pad(p0, (4, 4, 4, 4), mode="reflect")
    xp = F.conv2d(xp, g.view(1, 1, 1, 9).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(xp, g.view(1, 1, 9, 1).repeat(C, 1, 1, 1), groups=C)


def sag_eps(sd, plan, x, t, cs0, guided, scale, sag_scale, sigma, a, setting=None, margin=None):
    """fp32 [B, ...]: the guided prediction of one self-attention-guidance step on the latent x [B, C, H, W] at timestep t (an int)
    with the contexts cs0 of deepcache_cases.cfg_contexts ([uncond ; cond] rows when guided) -- and e_c, for the rescale.
    margin: a list that receives min |m - 1| over the combined column masses of the step."""
    B = x.shape[0]
    reps = 2 if guided else 1
    tt = torch.full((reps * B,), int(t), dtype=torch.long)
    eps, masses, (Hm, Wm) = walk(sd, plan, torch.cat([x] * reps), tt, cs0, setting)
    e0, e_c = eps[:B], eps[-B:]
    ratios = np.array([float(r) for _, _, r in cs0])
    ratios = ratios / ratios.sum()
    m = sum(float(r) * mt[:B] for r, mt in zip(ratios, masses))                 # float64 [B, Nm]
    if margin is not None:
        margin.append(float((m - 1.0).abs().min()))
    H, W = x.shape[2:]
    Mpx = (m > 1.0)[:, torch.from_numpy(nearest(H, W, Hm, Wm))]                 # [B, H, W]
    sa, s1, isa = (float(v) for v in coef_of(a))
    p0 = (x - s1 * e0) * isa
    d = torch.where(Mpx[:, None], blur32(p0, sigma), p0)
    xd = (sa * d + s1 * e0).half().float()                                      # stored as fp16
    e_d = walk(sd, plan, xd, tt[:B], [(ct, c[:B], r) for ct, c, r in cs0], setting)[0]
    e = e_c if not guided else eps[:B] + scale * (e_c - eps[:B])
    return e + sag_scale * (e0 - e_d), e_c


def oracle_loop(sd, plan, sampler, kind, xT, contexts, scale, sag_scale=0.0, sigma=SIGMA, setting=None, phi=0.0, noise=None,
                inpaint=None, margin=None):
    """The loop `sampler` ran last ("ddim", "2m", "sde" or "unipc") in fp32 on the oracle with self-attention guidance of weight
    sag_scale (0: off, today's loop), driven by the sampler's own coefficient table (pag_cases.oracle_loop's update formulas,
    restated).  setting: FreeU in every forward; phi: the guidance-rescale weight (diffusers' rescale_noise_cfg on the final
    prediction against e_c); inpaint = (x0, mask, noise): the blend of ddim.inpaint_blend_table behind every update;
    noise(draw) -> the step noise of kind "sde"; margin: a list that receives min |m - 1| of every step."""
    from lib.model_zoo.ddim import inpaint_blend_table
    ts = sampler.ddim_timesteps
    S = len(ts)
    tab = sampler._coef_table(S, scale, torch.device("cpu")).double().numpy()
    alphas = np.asarray(sampler.alphas_cumprod, dtype=np.float64)
    blend = None if inpaint is None else inpaint_blend_table(sampler.alphas_cumprod, ts)
    guided = scale != 1.0
    cs0 = dc.cfg_contexts(contexts, guided)
    x = xT.float().cpu()
    hist = xl = m1 = m2 = m3 = None
    for k, i in enumerate(reversed(range(S))):
        r = [float(v) for v in tab[i]]
        if sag_scale > 0:
            e, e_c = sag_eps(sd, plan, x, int(ts[i]), cs0, guided, r[0], float(sag_scale), sigma, alphas[int(ts[i])], setting, margin)
        else:
            reps = 2 if guided else 1
            eps = pc.walk(sd, plan, torch.cat([x] * reps), torch.full((reps * x.shape[0],), int(ts[i]), dtype=torch.long), cs0,
                          setting=setting)
            e_c = eps[-x.shape[0]:]
            e = e_c if not guided else eps[:x.shape[0]] + r[0] * (e_c - eps[:x.shape[0]])
        if phi > 0 and guided:
            sd_ = lambda v: v.double().flatten(1).std(1, unbiased=False)
            kf = float(np.float32(phi)) * (sd_(e_c) / sd_(e)) + (1.0 - float(np.float32(phi)))
            e = e * kf.float().view(-1, 1, 1, 1)
        if kind == "ddim":
            p0 = (x - r[5] * e) * r[1]
            x = r[2] * p0 + r[3] * e
        elif kind in ("2m", "sde"):
            p0 = (x - r[2] * e) * r[1]
            d = r[5] * p0 + (r[6] * hist if r[6] != 0 else 0.0)
            xn = r[3] * x + r[4] * d
            if kind == "sde" and r[7] != 0:
                xn = xn + r[7] * noise(k).reshape(x.shape).float()
            x, hist = xn, p0
        else:
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
        if inpaint is not None:
            x0, mask, nz = (v.float().cpu() for v in inpaint)
            x = mask * x + (1.0 - mask) * (float(blend[i][0]) * x0 + float(blend[i][1]) * nz)
    return x
