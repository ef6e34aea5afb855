"""HyperTile (tfernd 2023, with scale_depth and a fixed divisor) restated on the CPU: the index map of include/vd_hip.h (tiled row ->
token) and its inverse, the reshape / permute form of the two copies, which levels of a walk tile, an oracle walk built on
deepcache_cases.walk's structure and oracle.vd_oracle's blocks in which a tiled block's attn1 is
untile(attention(tile(q | k | v))) in fp32, and the solver loops of tome_cases on that walk.  Shared by the CPU and the GPU tests."""
import numpy as np
import torch
import torch.nn.functional as F

import deepcache_cases as dc
from deepcache_cases import FWD_TOL, LATENT_TOL  # noqa: F401  (the project's bounds, re-exported for the tests)

from oracle import vd_oracle as O

# (B, H, W, th, tw, cols): the kernel cases -- square and not, th != tw, a width that is no power of two, more than one block of 256
# chunks, and one tile (the identity)
KERNEL_CASES = [(2, 8, 8, 4, 4, 24), (1, 8, 16, 4, 8, 8), (3, 4, 12, 2, 3, 960), (2, 16, 16, 16, 16, 40)]
MAP_CASES = [(8, 8, 4, 4), (8, 16, 4, 8), (4, 12, 2, 3), (6, 10, 3, 5), (16, 16, 16, 16), (12, 4, 1, 4), (2, 2, 1, 1)]


# ---- the definition --------------------------------------------------------------------------------------------------------------
def index_map(H, W, th, tw):
    """int64 [H W]: perm[g] = the token n = y W + x that row g of a sample's tiled rows holds -- g = (ty ntx + tx) th tw + i tw + j,
    n = (ty th + i) W + tx tw + j."""
    assert H % th == 0 and W % tw == 0
    ntx = W // tw
    g = np.arange(H * W)
    tile, within = np.divmod(g, th * tw)
    ty, tx = np.divmod(tile, ntx)
    i, j = np.divmod(within, tw)
    return (ty * th + i) * W + tx * tw + j


def inverse_map(H, W, th, tw):
    """int64 [H W]: inv[n] = the tiled row of token n."""
    perm = index_map(H, W, th, tw)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return inv


def tile_ref(x, H, W, th, tw):
    """[B, H W, c] -> [B nty ntx, th tw, c] by reshape / permute (any dtype; no arithmetic)."""
    B, N, c = x.shape
    assert N == H * W
    return x.reshape(B, H // th, th, W // tw, tw, c).permute(0, 1, 3, 2, 4, 5).reshape(B * (H // th) * (W // tw), th * tw, c)


def untile_ref(a, B, H, W, th, tw):
    c = a.shape[-1]
    return a.reshape(B, H // th, W // tw, th, tw, c).permute(0, 1, 3, 2, 4, 5).reshape(B, H * W, c)


def kernel_input(B, H, W, cols, seed):
    """fp16 [B, H W, cols] whose every 16-byte chunk is distinct (a counter in the first element of each chunk under random
    values): a row or chunk that landed in the wrong place cannot equal the right one."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H * W, cols), generator=g).half()
    cnt = torch.arange(B * H * W * (cols // 8), dtype=torch.int32).view(B, H * W, cols // 8)
    x[..., ::8] = (cnt % 2048).half()
    x[..., 1::8] = (cnt // 2048).half()
    return x


# ---- which blocks tile -----------------------------------------------------------------------------------------------------------
def tiles_of(h_hw, x_hw, tile, max_downsample):
    """(nty, ntx) of a context block whose grid is h_hw on a latent of x_hw, or None where it runs untiled."""
    for f in (1, 2, 4):
        if f <= max_downsample and (-(-x_hw[0] // f), -(-x_hw[1] // f)) == tuple(h_hw):
            if h_hw[0] <= tile and h_hw[1] <= tile:
                return None
            assert h_hw[0] % tile == 0 and h_hw[1] % tile == 0
            return h_hw[0] // tile, h_hw[1] // tile
    return None


# ---- the oracle walk ---------------------------------------------------------------------------------------------------------------
def tiled_attention(q, k, v, heads, H, W, th, tw):
    """softmax(q k^T d^-1/2) v per th x tw tile of the H x W token grid, fp32: [B, H W, w] -> [B, H W, w]."""
    b, n, w = q.shape
    d = w // heads
    tq, tk, tv = (tile_ref(t, H, W, th, tw) for t in (q, k, v))
    sp = lambda t: t.reshape(t.shape[0], th * tw, heads, d).transpose(1, 2)
    a = ((sp(tq) @ sp(tk).transpose(-1, -2) * (d ** -0.5)).softmax(-1) @ sp(tv)).transpose(1, 2).reshape(-1, th * tw, w)
    return untile_ref(a, b, H, W, th, tw)


def spatial_transformer(sd, p, x, context, heads, th, tw, perturbed=None):
    """oracle.vd_oracle.spatial_transformer whose self-attention runs inside th x tw tiles.  perturbed: None, or a bool [rows]: those
    rows take the identity attention map (attn1 = to_out(v)), tiled or not."""
    b, c, hh, ww = x.shape
    h = O._conv(sd, p + ".proj_in", O._gn(sd, p + ".norm", x, 1e-6)).flatten(2).transpose(1, 2)
    q = p + ".transformer_blocks.0"
    w = h.shape[-1]
    ln = lambda name, t: F.layer_norm(t, (w,), sd[q + "." + name + ".weight"], sd[q + "." + name + ".bias"], 1e-5)
    n1 = ln("norm1", h)
    aq, ak, av = (F.linear(n1, sd[q + ".attn1.to_%s.weight" % k]) for k in "qkv")
    a = tiled_attention(aq, ak, av, heads, hh, ww, th, tw)
    if perturbed is not None:
        a = torch.where(torch.as_tensor(perturbed)[:, None, None], av, a)
    h = O._lin(sd, q + ".attn1.to_out.0", a) + h
    h = O.cross_attention(sd, q + ".attn2", ln("norm2", h), context, heads) + h
    v, gate = O._lin(sd, q + ".ff.net.0.proj", ln("norm3", h)).chunk(2, dim=-1)
    h = O._lin(sd, q + ".ff.net.2", v * F.gelu(gate)) + h
    return O._conv(sd, p + ".proj_out", h.transpose(1, 2).reshape(b, c, hh, ww)) + x


def walk(sd, plan, x, t, contexts, tile=0, max_downsample=1, x_type="image", tiles=None):
    """The UNet on x [rows, C, H, W] at timesteps t with contexts [(type, c, ratio), ...]: deepcache_cases.walk's plain walk in which
    the context blocks of tiles_of run their self-attention inside tile x tile tiles -- every context type's block at that index.
    tile 0: the plain walk.  tiles: a list that receives (N, nty ntx) per tiled block."""
    order = dc.flat_order(plan)
    emb = O.time_embed(sd, "diffuser.%s.time_embed" % x_type, O.timestep_embedding(t, plan["model_channels"]))
    ratios = np.array([float(r) for _, _, r in contexts])
    ratios = ratios / ratios.sum()
    h, hs, di, ci = x, [], 0, 0
    with torch.no_grad():
        for s in order:
            if s == "d":
                h = O._data_block(sd, "diffuser.%s.data_blocks.%d" % (x_type, di), plan["data"][di][0], h, emb)
                di += 1
            elif s == "c":
                hh, ww = h.shape[-2:]
                nt = tiles_of((hh, ww), tuple(x.shape[-2:]), tile, max_downsample) if tile else None
                if nt is not None and tiles is not None:
                    tiles.append((hh * ww, nt[0] * nt[1]))
                out = None
                for (ct, c, _), rr in zip(contexts, ratios):
                    p = "diffuser.%s.context_blocks.%d.0" % (ct, ci)
                    if nt is not None:
                        hi = spatial_transformer(sd, p, h, c, plan["ctx"][ci][1], tile, tile)
                    else:
                        hi = O.spatial_transformer(sd, p, h, c, plan["ctx"][ci][1])
                    if len(contexts) > 1:
                        hi = hi * float(rr)
                    out = hi if out is None else out + hi
                h = out
                ci += 1
            elif s == "save_hidden_feature":
                hs.append(h)
            else:
                h = torch.cat([h, hs.pop()], 1)
    return h


def oracle_loop(sd, plan, sampler, kind, xT, contexts, scale, tile=0, max_downsample=1):
    """The loop `sampler` ran last ("ddim", "2m", "sde" at eta 0 or "unipc") in fp32 on the oracle with HyperTile, driven by the
    sampler's own coefficient table (tome_cases.oracle_loop's update formulas, restated)."""
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
        t = torch.full((xin.shape[0],), int(ts[i]), dtype=torch.long)
        eps = walk(sd, plan, xin, t, cs, tile, max_downsample)
        if guided:
            e_u, e_c = eps.chunk(2)
            e = e_u + r[0] * (e_c - e_u)
        else:
            e = eps
        if kind == "ddim":      # {scale, 1/sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev - sigma^2), sigma, sqrt(1 - a_t)}
            p0 = (x - r[5] * e) * r[1]
            x = r[2] * p0 + r[3] * e
        elif kind in ("2m", "sde"):   # {scale, 1/sqrt(a_t), sqrt(1 - a_t), sigma_next/sigma_t, c_d, w_cur, w_prev, noise coefficient}
            assert r[7] == 0
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
