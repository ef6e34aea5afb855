"""Smoothed energy guidance (Hong 2024; ComfyUI's SEG node, diffusers' SmoothedEnergyGuidance) restated on the CPU oracle: the tap
rule and the folded reflection written out independently of the package, the separable query blur in float64 as an index walk, the
walk of tests/pag_cases.py in which the chosen context blocks blur the perturbed rows' n1 @ to_q over the token grid in front of
cross_attention's softmax (sigma = infinity: the mean query), and pag_cases' replicas / combine / oracle_loop on that walk -- SEG is
PAG's perturbed replica with another perturbation, so the combination e_u + s (e_c - e_u) + s_seg (e_c - e_p) and the loops are
the same statements.  Shared by the CPU and the GPU tests."""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

import freeu_cases as fc
import pag_cases as pc
from pag_cases import FWD_TOL, LATENT_TOL, combine, layers_of, replicas  # noqa: F401  (the project's bounds and PAG's statements)

from oracle import vd_oracle as O

SEG_SCALE = 3.0             # the upstream default of seg_scale (ComfyUI's SEG node, diffusers' SmoothedEnergyGuidance)
INF = math.inf              # the upstream default of seg_blur_sigma
MEAN_SIGMA = 9999.0         # from here on the official implementation takes the mean query
# on a 16 x 16 latent the tiny model's blocks 1 - 4 (the middle one, 2, among them) have an 8 x 8 token grid at width 128, the blocks
# 0, 5 and 6 a 16 x 16 one at width 64.  The mean query in the middle block alone moves the tiny model's prediction by 0.025 (rel-L2
# at t = 500) and in (1, 2, 3) at sigma 1 by 0.046, less than ten times the forward bound; the first block does (0.060 - 0.067),
# and so do the first four (0.074 - 0.084), which also span both grids and both widths
LAYER_CASES = [(0,), (0, 1, 2, 3)]
LOOP_LAYERS = (0, 1, 2, 3)
SIGMAS = [INF, 1.0]


def refl(i, n):
    """Reflection without repeating the edge as a brute-force walk: |i| steps from 0, turning at 0 and n - 1; 0 for n == 1 (and an
    index inside the grid is itself: the walk would arrive there without turning)."""
    if n == 1:
        return 0
    if 0 <= i < n:
        return i
    pos, d = 0, (1 if i >= 0 else -1)
    for _ in range(abs(i)):
        if pos + d < 0 or pos + d > n - 1:
            d = -d
        pos += d
    return pos


def taps_of(sigma):
    """(R, float64 taps): ks = ceil(6 sigma), plus 1 if even; R = (ks - 1) / 2; w[d] = exp(-0.5 (d / sigma)^2) / sum.  (-1, None) in
    mean mode (sigma >= 9999 or infinite)."""
    if math.isinf(sigma) or sigma >= MEAN_SIGMA:
        return -1, None
    ks = int(math.ceil(6.0 * sigma))
    if ks % 2 == 0:
        ks += 1
    R = (ks - 1) // 2
    w = np.array([math.exp(-0.5 * (d / sigma) ** 2) for d in range(-R, R + 1)], dtype=np.float64)
    return R, w / w.sum()


def blur64(q, gh, gw, taps, R):
    """float64 [B, gh gw, C]: qb[y, x] = sum_dy w[dy] (sum_dx w[dx] q[refl(y + dy, gh), refl(x + dx, gw)]) of q [B, gh gw, C], the
    taps as they are given (length 2 R + 1); R == -1: every row is the sample's mean row."""
    B, N, C = q.shape
    q = q.double().reshape(B, gh, gw, C)
    if R < 0:
        return q.reshape(B, N, C).mean(1, keepdim=True).expand(B, N, C).contiguous()
    w = [float(v) for v in taps]
    ix = [[refl(x + d, gw) for x in range(gw)] for d in range(-R, R + 1)]
    iy = [[refl(y + d, gh) for y in range(gh)] for d in range(-R, R + 1)]
    h = sum(w[j] * q[:, :, ix[j], :] for j in range(2 * R + 1))
    return sum(w[j] * h[:, iy[j], :, :] for j in range(2 * R + 1)).reshape(B, N, C)


def blur_conv(q, gh, gw, taps, R):
    """The same blur as torch states it for R < min(gh, gw): F.pad(mode="reflect") and a depthwise conv2d, in float64."""
    B, N, C = q.shape
    img = q.double().reshape(B, gh, gw, C).permute(0, 3, 1, 2)
    w = torch.as_tensor(np.asarray(taps, dtype=np.float64))
    k2 = (w[:, None] * w[None, :]).expand(C, 1, 2 * R + 1, 2 * R + 1).contiguous()
    out = F.conv2d(F.pad(img, (R, R, R, R), mode="reflect"), k2, groups=C)
    return out.permute(0, 2, 3, 1).reshape(B, N, C)


def blurred_self_attention(sd, p, x, heads, gh, gw, sigma):
    """oracle.vd_oracle.cross_attention(sd, p, x, None, heads) with q = to_q(x) blurred over the gh x gw grid (per channel, all
    heads alike) before the softmax scale; k and v are untouched."""
    R, taps = taps_of(sigma)
    q = blur64(F.linear(x, sd[p + ".to_q.weight"]), gh, gw, taps, R).to(x.dtype)
    k = F.linear(x, sd[p + ".to_k.weight"])
    v = F.linear(x, sd[p + ".to_v.weight"])
    b, n, c = q.shape
    d = c // heads
    sp = lambda t: t.view(b, t.shape[1], heads, d).transpose(1, 2)
    sim = sp(q) @ sp(k).transpose(-1, -2) * (d ** -0.5)
    out = (sim.softmax(dim=-1) @ sp(v)).transpose(1, 2).reshape(b, n, c)
    return O._lin(sd, p + ".to_out.0", out)


def spatial_transformer(sd, p, x, context, heads, perturbed, sigma=INF):
    """pag_cases.spatial_transformer with the perturbation of SEG: the rows of the bool vector `perturbed` run the block's
    self-attention with blurred queries; the other rows take the plain path."""
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
        a1[perturbed] = blurred_self_attention(sd, q + ".attn1", n1[perturbed], heads, hh, ww, sigma)
    h = a1 + h
    h = O.cross_attention(sd, q + ".attn2", ln("norm2", h), context, heads) + h
    v, gate = O._lin(sd, q + ".ff.net.0.proj", ln("norm3", h)).chunk(2, dim=-1)
    h = O._lin(sd, q + ".ff.net.2", v * F.gelu(gate)) + h
    return O._conv(sd, p + ".proj_out", h.transpose(1, 2).reshape(b, c, hh, ww)) + x


@contextlib.contextmanager
def _perturbation(sigma):
    """pag_cases' walk, windowed prediction and loop look their perturbed block up in their module: for the duration they find SEG's."""
    real = pc.spatial_transformer
    pc.spatial_transformer = lambda sd, p, x, context, heads, perturbed: spatial_transformer(sd, p, x, context, heads, perturbed, sigma)
    try:
        yield
    finally:
        pc.spatial_transformer = real


def walk(sd, plan, x, t, contexts, layers=(), perturbed=None, sigma=INF, setting=None, record=None):
    """pag_cases.walk with the perturbed rows' queries blurred at `sigma` in the context blocks `layers`."""
    with _perturbation(sigma):
        return pc.walk(sd, plan, x, t, contexts, layers, perturbed, setting, record=record)


def oracle_loop(sd, plan, sampler, kind, xT, contexts, scale, seg_scale=0.0, layers=LOOP_LAYERS, sigma=INF, **kw):
    """pag_cases.oracle_loop with SEG's perturbed replica: weight seg_scale (0: off), blur sigma, context blocks `layers`."""
    with _perturbation(sigma):
        return pc.oracle_loop(sd, plan, sampler, kind, xT, contexts, scale, seg_scale, layers, **kw)


# ---- the entry's cases ---------------------------------------------------------------------------------------------------------
EXACT_GRIDS = [((2, 2), 1), ((4, 6), 7), ((5, 7), 3), ((8, 8), 1), ((8, 8), 3), ((16, 16), 3), ((1, 1), 1)]
HEAD_DIMS = [(1, 64), (2, 40), (8, 40)]
# dyadic taps that sum to 1: with small-integer q every fp32 partial sum of both passes is exact (multiples of 2^-8 below 2^4), so
# the entry's result is the float64 formula rounded once to fp16
DYADIC = {1: [0.25, 0.5, 0.25], 3: [v / 16.0 for v in (1, 2, 3, 4, 3, 2, 1)], 7: [v / 16.0 for v in (1,) * 7 + (2,) + (1,) * 7]}
# random operands: (grid, H, D, sigma); the last two leave the LDS path (a hull of 48 rows x 48 tokens; a 1600-token row)
RANDOM_CASES = [((8, 8), 8, 160, 1.0), ((5, 7), 2, 40, 2.5), ((16, 16), 8, 80, 0.5), ((4, 6), 1, 64, 2.5), ((48, 48), 1, 64, 8.0),
                ((1, 1600), 1, 64, 0.5)]
MEAN_GRIDS = [(1, 1), (2, 2), (5, 7), (8, 8), (16, 16), (32, 32)]


def blur_bound(q, gh, gw, taps, R):
    """Per element of the finite-mode blur: 0.5 ulp_fp16(ref) + (4 R + 4) 2^-24 sum |w| |q| -- 2 (2 R + 1) fused multiply-adds,
    each one rounding of a partial sum that the absolute sum bounds, and the rounding to fp16 of its own."""
    ref = blur64(q, gh, gw, taps, R)
    mag = blur64(q.double().abs(), gh, gw, np.abs(np.asarray(taps, dtype=np.float64)), R)
    return ref, 0.5 * fc.ulp16(np.abs(ref.numpy())) + (4 * R + 4) * 2.0 ** -24 * mag.numpy()


def mean_bound(q):
    """Per element of the mean query: 0.5 ulp_fp16(ref) + N 2^-24 mean |q| -- N - 1 additions and the division, each one rounding."""
    N = q.shape[1]
    ref = blur64(q, 1, N, None, -1)
    mag = q.double().abs().mean(1, keepdim=True).expand_as(ref)
    return ref, 0.5 * fc.ulp16(np.abs(ref.numpy())) + N * 2.0 ** -24 * mag.numpy()
