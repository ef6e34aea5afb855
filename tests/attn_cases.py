"""Case table of the exact (per-element) tests of the attention kernels.

Every attention kernel of the library shares one arithmetic skeleton: fp32 scores, a subtracted running maximum, P = exp2(S')
rounded to fp16, O += V^T P^T in fp32, a row sum l, out = O * (1 / l).  The operands below leave that skeleton no rounding freedom:
every probability a correct kernel forms is exactly 0 or one constant per row, v holds small non-zero integers, so O is a sum of
exactly representable fp32 values, l an integer multiple of the constant, and the output the float64 softmax result correctly
rounded to fp16 (vdtest_util.attn_mismatch is the acceptance rule).  Three operand families, seeded on the CPU and drawn per
(batch, head), so that exchanging two heads or two samples changes the answer:

  uniform   q = 0: every logit is 0, every visible key has P = 1, the output is the mean of v over exactly the visible keys (the
            prefix mean under `causal`).  v = +-(1 .. vmax), one sign per (batch, head, channel), so no mean is near zero.
  selector  the key rows of one (batch, head) are pairwise distinct balanced +-1 codes of length D with a minimum Hamming distance
            d; q[i] = g * code[pi(i)].  The winner leads every other key by >= 2 g d D^-0.5 natural units; v holds non-zero integers
            of magnitude <= 255; the output is v[pi(i)]: attention as a gather.
  group     the selector with every code shared by three keys placed by a seeded permutation (different tiles wherever the shape
            has them): the three score identically and the output is the mean of three v rows, accumulated across tiles with
            rescales in between.  v has one sign per (batch, head, channel): what the losers leave in an accumulator before the
            winner arrives (below 2^-40 of it) can cost the last bit of a partial sum, which stays 2^-23 of the result only if the
            three terms do not cancel.

pi forces winners into the first tile, the tile seam (keys 63 / 64), the middle, one 32-key step before the end, the first key of
the last tile and the last key; under `causal` pi(i) <= i and every fifth row selects its own diagonal key.  The other rows draw pi
at random, so a winner comes both before and after keys with a higher running loser maximum (immediate and deferred rescale).
g = floor(80 / sqrt(D)), d = D / 4: the largest logit is below 80 natural units, the lead at least 32.

tests/test_exact_attention_cpu.py checks every precondition without a GPU; tests/test_exact_attention_gpu.py runs the kernels.
build(name) draws the operands and computes the float64 reference once per process.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

KINDS = ("uniform", "selector", "group")
SHAPES = {}
LN_EPS = 1e-5


def _shape(name, family, B, H, D, Nq, Nk, causal=False, kinds=KINDS, **kw):
    assert name not in SHAPES, name
    SHAPES[name] = dict(shape=name, family=family, B=B, H=H, D=D, Nq=Nq, Nk=Nk, causal=causal, kinds=kinds, **kw)


# ---- attn_fwd_kernel<D, 4>: 128 queries per block (wave w owns rows 32 w ..), 64 keys per tile -----------------------------------
# launch_attn<40>; Nk > 128 so no ctx_map; BH = 8: the "XCD owns consecutive pairs" mapping.  Second query block of two rows, three
# tiles, the last of one key: the smallest shape with a ragged block, a ragged tile and a full tile between them.
_shape("fwd40_ragged", "fwd4", 1, 8, 40, 130, 129)
# Nk <= 128 and B * nqb = 2 * 4 = 8: ctx_map (the heads of one (batch, query block) back to back on one XCD)
_shape("fwd40_ctx_map", "fwd4", 2, 8, 40, 512, 77)
# B * nqb = 2 is no multiple of 8: launch_attn refuses ctx_map, BH = 8 takes the pairs mapping with a short context
_shape("fwd40_ctx_refused", "fwd4", 1, 8, 40, 200, 77)
# BH = 3: plain fallback mapping.  Causal: tiles cross the diagonal, the tile count is clipped per block (block 0 of the second
# shape sees one of its three tiles), and rows 70 .. 129 of the first have more queries than keys.
_shape("fwd64_causal_tall", "fwd4", 1, 3, 64, 130, 70, causal=True)
_shape("fwd64_causal_wide", "fwd4", 1, 3, 64, 70, 130, causal=True)
# the text encoders' shape; BH = 36: fallback mapping
_shape("fwd64_clip", "fwd4", 3, 12, 64, 77, 77, causal=True)
# double-buffered (2 * TILE_BYTES <= 60 KiB), five tiles, the last of one key; BH = 16: pairs mapping, two pairs per XCD
_shape("fwd80_five_tiles", "fwd4", 2, 8, 80, 96, 257)
# 2 * TILE_BYTES > 60 KiB: the single-buffer path (barrier, refill, barrier); nine tiles, the last of two keys
_shape("fwd160_single_buffer", "fwd4", 2, 8, 160, 100, 514)
# q, k, v column slices of one fused [B, N, 3C] projection, out= a guarded column slice (ldo = C + 8, spare rows after Nq)
_shape("fwd40_views", "fwd4", 2, 8, 40, 130, 130, views=True)
_shape("fwd160_views", "fwd4", 1, 3, 160, 70, 70, views=True)

# ---- attn_pipe_kernel<40> (Nq >= 2048, Nk >= 1024): 512 queries per block (wave w owns rows 64 w ..), 32-key steps -----------------
# The running max is the fp16 value (rounded up) in Q's spare k-slot, so the shared probability of a row is exp2(s - fp16(m)) <= 1
# instead of 1: still ONE constant per row -- the column of ones sums the same fp16 P that multiplies v -- which is all the
# derivation needs.  The same two shapes run on attn_fwd_kernel<40, 8> (256 queries per block) in a child with VD_ATTN_PIPE=0.
# BH = 2: fallback mapping; five blocks, rows 2088 .. 2559 of the last empty (whole row blocks of waves 0 / 1, whole waves
# after them); 17 tiles, the last of one key
_shape("pipe_ragged", "pipe", 1, 2, 40, 2088, 1025, vmax=6)
# BH = 8: pairs mapping; the last tile holds six keys; pi forces key 0, key Nk - 1 and key Nk - 33
_shape("pipe_pairs", "pipe", 1, 8, 40, 2048, 1030, vmax=6)

# ---- attn_wide_kernel<D>: one head, 32 queries per block, 32 keys per tile, wave w owns channels w D/4 .. of Q.K^T and of O --------
# The codes span all of D and come with decoys that differ in ONE wave's quarter (codebook): every wave's partial score is needed to
# find the winner.
_shape("wide128", "wide", 3, 1, 128, 64, 64)        # two full tiles, two blocks per sample
_shape("wide256", "wide", 2, 1, 256, 333, 333)      # eleven tiles, the last of 13 keys; last query block of 13 rows
_shape("wide512", "wide", 1, 1, 512, 100, 100)      # three tiles plus four keys, last query block of four rows; 160 KiB of LDS

# ---- xattn_kernel<D> through ops.xattn with the LayerNorm fold: 128 queries per block x one head ------------------------------------
# uniform: wq = 0 and no bias, x random with a common offset (q is exactly 0 whatever x and its statistics are);
# selector: wq = g I, gamma = 1, beta = 0, x[i] = a_i * (per-head codes) + o_i with a_i in {0.5, 1, 2} and o_i in {-0.25, 0, 0.5}:
# the codes are balanced, so the row mean is o_i exactly and LayerNorm returns the codes times (1 + eps / a^2)^-0.5, which the fp16
# rounding of q turns into exactly g * code.
_XK = ("uniform", "selector")
_shape("xattn40_plain", "xattn", 1, 8, 40, 130, 77, kinds=_XK)      # B * nqb = 2: plain block order; ragged second block
_shape("xattn40_xcd_map", "xattn", 2, 8, 40, 512, 77, kinds=_XK)    # B * nqb = 8: xcd_map
_shape("xattn80", "xattn", 2, 8, 80, 96, 257, kinds=_XK)            # five tiles: the two-buffer ring wraps, last tile of one key
_shape("xattn160", "xattn", 2, 8, 160, 64, 514, kinds=_XK)          # 4-stage projection pipeline, VALU row sums, nine tiles

CASES = {}
for _n, _s in SHAPES.items():
    for _k in _s["kinds"]:
        CASES["%s-%s" % (_n, _k)] = dict(_s, name="%s-%s" % (_n, _k), kind=_k)

FAMILIES = ("fwd4", "pipe", "wide", "xattn")


def names(family=None, kind=None):
    return [n for n, c in CASES.items() if (family is None or c["family"] == family) and (kind is None or c["kind"] == kind)]


def gain(D):
    return int(80.0 / D ** 0.5)


def _seed(name):
    return 7000 + 10 * list(CASES).index(name)


@functools.lru_cache(maxsize=None)
def codebook(n, D, d, slices=1):
    """n pairwise distinct balanced +-1 codes of length D with pairwise Hamming distance >= d: greedy choice among seeded random
    candidates.  slices = 4 (the wide kernel, whose waves own a quarter of the head dim each): every quarter is balanced by itself
    and a candidate enters as a family of five -- the code and its four decoys with one quarter negated, at distance D / 4 from
    it -- so a partial score that is lost, or taken from another wave's quarter, makes a decoy tie with or beat the winner."""
    rng = np.random.default_rng(1000 * D + d + slices)
    w = D // slices
    base = np.tile(np.where(np.arange(w) < w // 2, 1, -1).astype(np.int32), slices)
    chosen = np.empty((n + 4, D), np.int32)
    m = 0
    for _ in range(8):
        cand = np.concatenate([rng.permuted(np.tile(base[:w], (4096, 1)), axis=1) for _ in range(slices)], 1)
        for c in cand:
            fam = c[None, :]
            if slices > 1:
                fam = np.tile(c, (slices + 1, 1))
                for j in range(slices):
                    fam[j + 1, j * w:(j + 1) * w] *= -1
            if m == 0 or (chosen[:m] @ fam.T).max() <= D - 2 * d:     # dot = D - 2 * distance
                chosen[m:m + len(fam)] = fam
                m += len(fam)
                if m >= n:
                    return chosen[:n]
    raise AssertionError("codebook(%d, %d, %d): %d codes found" % (n, D, d, m))


def _forced_keys(Nk):
    f = [0, Nk - 1, max(Nk - 33, 0), (Nk - 1) // 64 * 64, Nk // 2, min(63, Nk - 1), min(64, Nk - 1)]
    return np.array(f, np.int64)


def _draw(c, s):
    """Per (batch, head): codes [B, H, Nk, D] (+-1), code id of every key cid [B, H, Nk], winner key pi [B, H, Nq], v [B, Nk, H, D]."""
    B, H, D, Nq, Nk, kind = c["B"], c["H"], c["D"], c["Nq"], c["Nk"], c["kind"]
    rng = np.random.default_rng(s)
    slices = 4 if c["family"] == "wide" else 1
    book = codebook(Nk, D, D // 4, slices)
    w = D // slices
    codes = np.empty((B, H, Nk, D), np.int32)
    cid = np.empty((B, H, Nk), np.int64)
    pi = np.empty((B, H, Nq), np.int64)
    rows = np.arange(Nq)
    forced = _forced_keys(Nk)
    for b in range(B):
        for h in range(H):
            if kind == "group":
                ng, perm = Nk // 3, rng.permutation(Nk)
                cid[b, h, perm] = np.where(np.arange(Nk) < 3 * ng, np.arange(Nk) // 3, ng + np.arange(Nk) - 3 * ng)
            else:
                cid[b, h] = np.arange(Nk)
            cols = np.concatenate([j * w + rng.permutation(w) for j in range(slices)])     # (columns stay inside their quarter)
            codes[b, h] = book[rng.permutation(Nk)][:, cols][cid[b, h]]
            p = rng.integers(0, Nk, Nq)
            p[rows % 3 == 0] = forced[(rows[rows % 3 == 0] // 3) % len(forced)]
            if c["causal"]:
                p = np.minimum(p, rows)
                p[rows % 5 == 0] = np.minimum(rows[rows % 5 == 0], Nk - 1)
            pi[b, h] = p
    if kind == "uniform":
        vmax = c.get("vmax", 16)
        v = rng.integers(1, vmax + 1, (B, Nk, H, D)) * np.where(rng.integers(0, 2, (B, 1, H, D)) > 0, 1, -1)
    else:   # group: one sign per (batch, head, channel) again -- the three rows of a group must not cancel, see the module docstring
        v = rng.integers(1, 256, (B, Nk, H, D)) * np.where(rng.integers(0, 2, (B, Nk if kind == "selector" else 1, H, D)) > 0, 1, -1)
    return rng, codes, cid, pi, v


def layernorm_fold_q(x, wq, gamma, beta, H, D):
    """float64 LayerNorm -> projection with the folded fp16 weight (gamma folded into wq, beta into a bias: what
    hip_layers.fold_layernorm hands the kernel) -> q rounded to fp16, as the kernel rounds it.  Returns (q fp16, folded weight fp16)."""
    w_fold = (wq.float() * gamma.float()[None, :]).half()
    bias = (wq.float() @ beta.float()).half()
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    xn = (xd - mean) / torch.sqrt(var + LN_EPS)
    qd = xn @ w_fold.double().t() + bias.double()
    return torch.from_numpy(qd.numpy().astype(np.float16)), w_fold


def visible(Nq, Nk, causal):
    """[Nq, Nk] bool: key j is visible to query i (causal: j <= i)."""
    if not causal:
        return np.ones((Nq, Nk), bool)
    return np.arange(Nk)[None, :] <= np.arange(Nq)[:, None]


def softmax_attention(q, k, v, H, causal, scale=None):
    """float64 softmax(q k^T scale) v on [B, N, H * D] operands -> (out [B, Nq, H, D], P [B, H, Nq, Nk], logits [B, H, Nq, Nk])."""
    B, Nq, C = q.shape
    Nk, D = k.shape[1], C // H
    scale = D ** -0.5 if scale is None else scale
    qd = q.double().view(B, Nq, H, D).permute(0, 2, 1, 3)
    kd = k.double().view(B, Nk, H, D).permute(0, 2, 1, 3)
    vd = v.double().view(B, Nk, H, D).permute(0, 2, 1, 3)
    logits = qd @ kd.transpose(-1, -2) * scale
    s = logits.masked_fill(~torch.from_numpy(visible(Nq, Nk, causal)), float("-inf"))
    P = torch.softmax(s, -1)
    return (P @ vd).permute(0, 2, 1, 3).contiguous(), P, logits


@functools.lru_cache(maxsize=None)
def build(name):
    """Operands (CPU fp16) and the float64 reference `ref` [B, Nq, H, D] of a case, with what the precondition tests read: the
    largest |logit|, the largest probability mass outside the winning keys, the value the winners select (`selected`), the
    winning key of every row (`pi` [B, H, Nq]) and the code ids (`cid`).  Computed once per process and shared -- do not modify."""
    c = CASES[name]
    B, H, D, Nq, Nk, kind = c["B"], c["H"], c["D"], c["Nq"], c["Nk"], c["kind"]
    C = H * D
    rng, codes, cid, pi, v = _draw(c, _seed(name))
    t = SimpleNamespace(case=c, codes=codes, cid=cid, pi=pi, g=gain(D))
    t.k = torch.from_numpy(codes.transpose(0, 2, 1, 3).reshape(B, Nk, C).astype(np.float32)).half()
    t.v = torch.from_numpy(v.reshape(B, Nk, C).astype(np.float32)).half()
    qcodes = np.take_along_axis(codes, pi[..., None], 2).transpose(0, 2, 1, 3).reshape(B, Nq, C)     # code[pi(i)] per head
    if c["family"] == "xattn":
        if kind == "uniform":
            t.wq = torch.zeros(C, C).half()
            x = rng.standard_normal((B, Nq, C)) * 1.1 + rng.choice([-1.5, 0.0, 0.3, 2.0], (B, Nq, 1))
        else:
            t.wq = (torch.eye(C) * t.g).half()
            x = qcodes * rng.choice([0.5, 1.0, 2.0], (B, Nq, 1)) + rng.choice([-0.25, 0.0, 0.5], (B, Nq, 1))
        t.x = torch.from_numpy(x.astype(np.float32)).half()
        t.gamma, t.beta = torch.ones(C), torch.zeros(C)
        t.q, t.w_fold = layernorm_fold_q(t.x, t.wq, t.gamma, t.beta, H, D)
    elif kind == "uniform":
        t.q = torch.zeros(B, Nq, C).half()
    else:
        t.q = torch.from_numpy((qcodes * t.g).astype(np.float32)).half()
    t.ref, P, logits = softmax_attention(t.q, t.k, t.v, H, c["causal"])
    vis = torch.from_numpy(visible(Nq, Nk, c["causal"]))
    if kind == "uniform":
        win = vis[None, None].expand(B, H, Nq, Nk)
    else:
        cidt, pit = torch.from_numpy(cid), torch.from_numpy(pi)
        win = (cidt[:, :, None, :] == torch.gather(cidt, 2, pit)[..., None]) & vis[None, None]
    t.win = win
    t.max_logit = logits.abs().max().item()
    t.off_mass = (P * (~win)).sum(-1).max().item()
    vd = t.v.double().view(B, Nk, H, D).permute(0, 2, 1, 3)
    wd = win.double()
    t.selected = ((wd @ vd) / wd.sum(-1, keepdim=True)).permute(0, 2, 1, 3).contiguous()
    t.cancels = not torch.equal((wd @ vd).abs(), wd @ vd.abs())      # some row adds v of both signs in one channel
    t.carried = (wd @ vd.abs()).max().item()      # largest sum of |v| over the keys that carry probability in one row
    return t
