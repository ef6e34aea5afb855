"""Token merging (Bolya & Hoffman 2023; tomesd with sx = sy = 2, use_rand = False) restated on the CPU: the definition of
include/vd_hip.h in numpy float64 / int64 (sets, match, plan, merge with exact sums, unmerge), a literal transcription of the tomesd
algorithm to hold it against, an oracle walk built on deepcache_cases.walk's structure and oracle.vd_oracle's blocks in which a merging
block's attn1 is unmerge(attention(merge(q | k | v))) in fp32 -- on its own plan or on plans recorded from the device -- and the solver
loops of pag_cases on that walk.  Shared by the CPU and the GPU tests."""
import numpy as np
import torch
import torch.nn.functional as F

import deepcache_cases as dc
from deepcache_cases import FWD_TOL, LATENT_TOL  # noqa: F401  (the project's bounds, re-exported for the tests)

from oracle import vd_oracle as O

GRIDS = [(4, 4, 64, 1), (8, 8, 320, 3), (6, 10, 64, 2), (16, 8, 640, 1), (32, 32, 320, 2)]      # (H, W, C, B)


def match_tol(C):
    """2 (C + 8) 2^-24: the fp32 dot-product bound in cosine units plus the norm roundings."""
    return 2.0 * (C + 8) * 2.0 ** -24


# ---- the definition --------------------------------------------------------------------------------------------------------------
def sets(H, W):
    """(src, dst): the token indices n = y W + x of the sources (ascending n) and of the destinations (y, x both even; ordinal
    order) of an H x W grid."""
    assert H % 2 == 0 and W % 2 == 0
    y, x = np.divmod(np.arange(H * W), W)
    is_dst = (y % 2 == 0) & (x % 2 == 0)
    return np.nonzero(~is_dst)[0], np.nonzero(is_dst)[0]


def r_of(H, W, ratio):
    N = H * W
    return min(int(N * ratio), N - N // 4)


def scores64(h, H, W):
    """float64 [B, Ns, Nd]: the cosine of every (source, destination) pair of the metric h [B, N, C] (fp16 values); an all-zero
    row scores 0."""
    h = np.asarray(h.detach().cpu().numpy() if torch.is_tensor(h) else h).astype(np.float64)
    src, dst = sets(H, W)
    ss = (h * h).sum(-1)
    inv = np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0)
    return np.einsum("bic,bdc->bid", h[:, src], h[:, dst]) * inv[:, src, None] * inv[:, None, dst]


def match_ref(h, H, W):
    """(node_idx int32 [B, Ns], node_max float64 [B, Ns]) in float64; among equal scores the lowest d (np.argmax's rule)."""
    s = scores64(h, H, W)
    idx = s.argmax(-1)
    return idx.astype(np.int32), np.take_along_axis(s, idx[..., None], -1)[..., 0]


def plan_ref(node_idx, node_max, H, W, r):
    """row_of int32 [B, N] from node_idx [B, Ns] and the fp32 node_max [B, Ns]: a descending, stable rank, the first r merged."""
    node_idx = np.asarray(node_idx)
    node_max = np.asarray(node_max, dtype=np.float32)
    src, dst = sets(H, W)
    B, Ns = node_max.shape
    assert 0 <= r <= Ns
    row_of = np.empty((B, H * W), dtype=np.int32)
    for b in range(B):
        order = np.argsort(-node_max[b].astype(np.float64), kind="stable")
        rank = np.empty(Ns, dtype=np.int64)
        rank[order] = np.arange(Ns)
        row_of[b, dst] = Ns - r + np.arange(len(dst))
        row_of[b, src] = np.where(rank >= r, rank - r, Ns - r + node_idx[b])
    return row_of


def merge_ref(x, row_of, r):
    """fp16 [B, N - r, cols] of the fp16 x [B, N, cols]: every row the mean of the tokens that map to it -- the sum exact in int64
    units of 2^-24, the quotient double(sum) / count rounded once to fp16 (numpy converts float64 to float16 directly)."""
    x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    assert x.dtype == np.float16
    row_of = np.asarray(row_of)
    B, N, cols = x.shape
    fx = np.round(x.astype(np.float64) * 2.0 ** 24).astype(np.int64)
    assert np.array_equal(fx.astype(np.float64) * 2.0 ** -24, x.astype(np.float64))
    out = np.empty((B, N - r, cols), dtype=np.float16)
    for b in range(B):
        acc = np.zeros((N - r, cols), dtype=np.int64)
        np.add.at(acc, row_of[b], fx[b])
        cnt = np.bincount(row_of[b], minlength=N - r).astype(np.float64)
        assert cnt.min() >= 1
        out[b] = ((acc.astype(np.float64) * 2.0 ** -24) / cnt[:, None]).astype(np.float16)
    return out


def unmerge_ref(a, row_of):
    a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return np.stack([a[b][np.asarray(row_of)[b]] for b in range(a.shape[0])])


# ---- tomesd, transcribed (tomesd/merge.py: bipartite_soft_matching_random2d with no_rand = True, then merge / unmerge) ------------
def tomesd_ref(metric, x, H, W, r):
    """(merged, unmerged-of-merged) of x [B, N, c] under the matching of metric [B, N, C], both float64 torch tensors, as the
    package computes them: argsort / gather / scatter_reduce('mean')."""
    B, N, _ = metric.shape
    sy = sx = 2
    hsy, wsx = H // sy, W // sx
    rand_idx = torch.zeros(hsy, wsx, 1, dtype=torch.int64)
    idx_buffer_view = torch.zeros(hsy, wsx, sy * sx, dtype=torch.int64)
    idx_buffer_view.scatter_(dim=2, index=rand_idx, src=-torch.ones_like(rand_idx, dtype=rand_idx.dtype))
    idx_buffer_view = idx_buffer_view.view(hsy, wsx, sy, sx).transpose(1, 2).reshape(hsy * sy, wsx * sx)
    idx_buffer = idx_buffer_view
    rand_idx = idx_buffer.reshape(1, -1, 1).argsort(dim=1, stable=True)
    num_dst = hsy * wsx
    a_idx = rand_idx[:, num_dst:, :]
    b_idx = rand_idx[:, :num_dst, :]

    def split(t):
        C = t.shape[-1]
        src = torch.gather(t, dim=1, index=a_idx.expand(B, N - num_dst, C))
        dst = torch.gather(t, dim=1, index=b_idx.expand(B, num_dst, C))
        return src, dst

    metric = metric / metric.norm(dim=-1, keepdim=True)
    a, b = split(metric)
    scores = a @ b.transpose(-1, -2)
    r = min(a.shape[1], r)
    node_max, node_idx = scores.max(dim=-1)
    edge_idx = node_max.argsort(dim=-1, descending=True)[..., None]
    unm_idx = edge_idx[..., r:, :]
    src_idx = edge_idx[..., :r, :]
    dst_idx = torch.gather(node_idx[..., None], dim=-2, index=src_idx)

    src, dst = split(x)
    n, t1, c = src.shape
    unm = torch.gather(src, dim=-2, index=unm_idx.expand(n, t1 - r, c))
    src = torch.gather(src, dim=-2, index=src_idx.expand(n, r, c))
    dst = dst.scatter_reduce(-2, dst_idx.expand(n, r, c), src, reduce="mean")
    merged = torch.cat([unm, dst], dim=1)

    unm_len = unm_idx.shape[1]
    unm, dst = merged[..., :unm_len, :], merged[..., unm_len:, :]
    src = torch.gather(dst, dim=-2, index=dst_idx.expand(B, r, c))
    out = torch.zeros(B, N, c, dtype=merged.dtype)
    out.scatter_(dim=-2, index=b_idx.expand(B, num_dst, c), src=dst)
    out.scatter_(dim=-2, index=torch.gather(a_idx.expand(B, a_idx.shape[1], 1), dim=1, index=unm_idx).expand(B, unm_len, c), src=unm)
    out.scatter_(dim=-2, index=torch.gather(a_idx.expand(B, a_idx.shape[1], 1), dim=1, index=src_idx).expand(B, r, c), src=src)
    return merged, out


# ---- inputs of the kernel tests ---------------------------------------------------------------------------------------------------
def random_metric(H, W, C, B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, H * W, C), generator=g).half()


def planted_metric(H, W, C, B, seed):
    """(h fp16 [B, N, C], chosen int [B, Ns]): every source is a chosen destination plus small noise; asserts that every float64
    top-2 margin of the scores exceeds 4 match_tol(C), so the argmax is decided far outside the kernel's rounding."""
    g = torch.Generator().manual_seed(seed)
    src, dst = sets(H, W)
    h = torch.randn((B, H * W, C), generator=g)
    chosen = torch.randint(0, len(dst), (B, len(src)), generator=g)
    for b in range(B):
        h[b, src] = h[b, dst][chosen[b]] * (0.5 + torch.rand((len(src), 1), generator=g)) + 0.05 * torch.randn((len(src), C), generator=g)
    h = h.half()
    s = scores64(h, H, W)
    if len(dst) > 1:
        top = np.sort(s, -1)
        assert (top[..., -1] - top[..., -2]).min() > 4 * match_tol(C), (top[..., -1] - top[..., -2]).min()
    assert np.array_equal(s.argmax(-1), chosen.numpy())
    return h, chosen.numpy()


def double_rounding_rows():
    """Three fp16 values whose exact mean rounds to another fp16 directly than through float32: 3 + 3 * 2^-11 + 2^-24 over 3 is
    1 + 2^-11 + 2^-24 / 3, just above the midpoint of 1 and 1 + 2^-10; float32 drops the excess and the tie then goes to even."""
    vals = np.array([3.0, 3.0 * 2.0 ** -11, 2.0 ** -24], dtype=np.float64)
    assert np.array_equal(vals.astype(np.float16).astype(np.float64), vals)
    q = vals.sum() / 3.0
    direct, via32 = np.float16(q), np.float16(np.float32(q))
    assert direct != via32 and float(direct) == 1.0 + 2.0 ** -10 and float(via32) == 1.0
    return vals.astype(np.float16), direct


# ---- the oracle walk ---------------------------------------------------------------------------------------------------------------
def merges(h_hw, x_hw, max_downsample):
    return any(h_hw[0] * f == x_hw[0] and h_hw[1] * f == x_hw[1] for f in range(1, max_downsample + 1))


def spatial_transformer(sd, p, x, context, heads, r, row_of=None):
    """oracle.vd_oracle.spatial_transformer whose self-attention merges r tokens: q | k | v of norm1(h), each row of the merged
    tensor the fp32 mean of the tokens that map to it, softmax attention on the N - r rows, a row gather back, to_out.  row_of
    [B, N] given: that plan; else the definition's own from the metric h in float64.  Returns (out, row_of)."""
    b, c, hh, ww = x.shape
    h = O._conv(sd, p + ".proj_in", O._gn(sd, p + ".norm", x, 1e-6)).flatten(2).transpose(1, 2)
    q = p + ".transformer_blocks.0"
    w = h.shape[-1]
    ln = lambda name, t: F.layer_norm(t, (w,), sd[q + "." + name + ".weight"], sd[q + "." + name + ".bias"], 1e-5)
    if row_of is None:
        idx, mx = match_ref(h.double(), hh, ww)
        row_of = plan_ref(idx, mx.astype(np.float32), hh, ww, r)
    ro = torch.as_tensor(np.asarray(row_of), dtype=torch.int64)
    n1 = ln("norm1", h)
    qkv = torch.cat([F.linear(n1, sd[q + ".attn1.to_%s.weight" % k]) for k in "qkv"], -1)
    Nm = hh * ww - r
    merged = torch.zeros((b, Nm, qkv.shape[-1]), dtype=qkv.dtype).index_put_(
        (torch.arange(b)[:, None].expand_as(ro), ro), qkv, accumulate=True)
    cnt = torch.zeros((b, Nm), dtype=qkv.dtype).index_put_((torch.arange(b)[:, None].expand_as(ro), ro), torch.ones_like(ro, dtype=qkv.dtype),
                                                          accumulate=True)
    merged = merged / cnt[..., None]
    mq, mk, mv = merged.chunk(3, -1)
    d = w // heads
    sp = lambda t: t.view(b, Nm, heads, d).transpose(1, 2)
    a = ((sp(mq) @ sp(mk).transpose(-1, -2) * (d ** -0.5)).softmax(-1) @ sp(mv)).transpose(1, 2).reshape(b, Nm, w)
    a = torch.gather(a, 1, ro[..., None].expand(b, hh * ww, w))
    h = O._lin(sd, q + ".attn1.to_out.0", a) + h
    h = O.cross_attention(sd, q + ".attn2", ln("norm2", h), context, heads) + h
    v, gate = O._lin(sd, q + ".ff.net.0.proj", ln("norm3", h)).chunk(2, dim=-1)
    h = O._lin(sd, q + ".ff.net.2", v * F.gelu(gate)) + h
    return O._conv(sd, p + ".proj_out", h.transpose(1, 2).reshape(b, c, hh, ww)) + x, row_of


def walk(sd, plan, x, t, contexts, ratio=0.0, max_downsample=1, plans=None, x_type="image", tokens=None):
    """The UNet on x [rows, C, H, W] at timesteps t with contexts [(type, c, ratio), ...]: deepcache_cases.walk's plain walk in which
    the context blocks whose token grid is the latent grid (or, max_downsample 2, half of it per side) merge r = r_of(grid, ratio)
    tokens in their self-attention -- every context type's block at that index.  plans: None (the definition's own plan per block
    and type), or an iterator over the row_of arrays [rows, N] recorded from the device, consumed in walk order.  tokens: a list
    that receives (N, N - r) per merging block."""
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
                r = r_of(hh, ww, ratio) if ratio > 0 and merges((hh, ww), x.shape[-2:], max_downsample) else 0
                if r > 0 and tokens is not None:
                    tokens.append((hh * ww, hh * ww - r))
                out = None
                for (ct, c, _), rr in zip(contexts, ratios):
                    p = "diffuser.%s.context_blocks.%d.0" % (ct, ci)
                    if r > 0:
                        ro = None
                        if plans is not None:
                            wi, ro = next(plans)
                            assert wi == ci, (wi, ci)
                            ro = ro.cpu().numpy()
                            if ro.shape[0] != h.shape[0]:       # attn1 ran once per guidance pair: both replicas took that plan
                                assert h.shape[0] % ro.shape[0] == 0
                                ro = np.concatenate([ro] * (h.shape[0] // ro.shape[0]))
                        hi = spatial_transformer(sd, p, h, c, plan["ctx"][ci][1], r, ro)[0]
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


def oracle_loop(sd, plan, sampler, kind, xT, contexts, scale, ratio=0.0, max_downsample=1, plans=None):
    """The loop `sampler` ran last ("ddim", "2m", "sde" at eta 0 or "unipc") in fp32 on the oracle with token merging, driven by the
    sampler's own coefficient table (pag_cases.oracle_loop's update formulas, restated).  plans: the list a TokenMerge.record
    collected over the whole device loop, replayed in order."""
    ts = sampler.ddim_timesteps
    S = len(ts)
    tab = sampler._coef_table(S, scale, torch.device("cpu")).double().numpy()
    guided = scale != 1.0
    cs = dc.cfg_contexts(contexts, guided)
    x = xT.float().cpu()
    it = None if plans is None else iter(plans)
    hist = xl = m1 = m2 = m3 = None
    for k, i in enumerate(reversed(range(S))):
        r = [float(v) for v in tab[i]]
        xin = torch.cat([x, x]) if guided else x
        t = torch.full((xin.shape[0],), int(ts[i]), dtype=torch.long)
        eps = walk(sd, plan, xin, t, cs, ratio, max_downsample, it)
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
    if it is not None:
        assert next(it, None) is None, "the device recorded more plans than the oracle walk consumed"
    return x
