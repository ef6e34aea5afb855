"""Transformer blocks of the VD UNet on the HIP kernel library, tokens-major (B*HW, C) end to end.

Same module tree / state-dict keys as the reference (lib/model_zoo/attention.py:37-64,152-266 there), different
execution: no NCHW<->(b, hw, c) transposes (the activation already is (B*HW, C)), q/k/v of the self-attention
in ONE GEMM, scores never materialised (vd_attention_f16), residual adds / GEGLU gating / bias fused into GEMM
epilogues, context K/V projections reusable across DDIM steps through an explicit cache.
"""
import torch
import torch.nn as nn

from vd_hip import ops, pack

from . import hip_layers
from .hip_layers import Conv2d, GroupNorm, LayerNorm, Linear, PackCache, _h, fold_layernorm


class GEGLU(nn.Module, PackCache):
    """proj: dim_in -> 2*dim_out, out = value * gelu(gate)  (reference attention.py:37-45), gating fused in the
    GEMM epilogue; the weight rows are re-interleaved once so value/gate tiles meet in one workgroup."""

    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = Linear(dim_in, dim_out * 2)

    def forward(self, x, ln=None, ln_sums=None):
        """ln: the nn.LayerNorm the reference applies in front (x is then the UN-normalised input; folded, see
        hip_layers.fold_layernorm).  ln_sums: (sum, sum of squares) per row of x from the launch that stored x."""
        if ln is None:
            wp, bp = self._packed("geglu", (self.proj.weight, self.proj.bias),
                                  lambda: pack.pack_geglu(_h(self.proj.weight), _h(self.proj.bias)))
            return ops.linear(x, wp, bp, act=ops.ACT_GEGLU)

        wp, bp, cs = self.folded(ln)
        kw = {}
        if hip_layers.wstream_epi_level("geglu", x.numel() // x.shape[-1], x.shape[-1]):
            kw["w_stream_epi"] = self.folded_stream(ln)
        return ops.linear(x, wp, bp, act=ops.ACT_GEGLU, colsum=cs, ln_eps=ln.eps, ln_sums=ln_sums, **kw)

    def folded_stream(self, ln):
        """The packed weight of folded() in MFMA-fragment order for vd_gemm_wstream_epi_f16 (a wave's two 32-row tiles are the value
        and the gate rows of its 32 outputs); keyed on the same parameters."""
        return self._packed("geglu_ln_stream", (self.proj.weight, self.proj.bias, ln.weight, ln.bias),
                            lambda: pack.pack_linear_weight_stream(self.folded(ln)[0]))

    def folded(self, ln):
        """(gamma-folded GEGLU-packed weight, beta-folded packed bias, fp32 row sums of the packed weight), cached."""
        def build():
            w, b, _ = fold_layernorm(_h(self.proj.weight), _h(self.proj.bias), ln)
            wp, bp = pack.pack_geglu(w, b)
            return wp, bp, wp.float().sum(1).contiguous()
        return self._packed("geglu_ln", (self.proj.weight, self.proj.bias, ln.weight, ln.bias), build)


class FeedForward(nn.Module):
    def __init__(self, dim, dim_out=None, mult=4, glu=True, dropout=0.0):
        super().__init__()
        assert glu, "only the gated (GEGLU) feed-forward is on the VD path"
        inner = int(dim * mult)
        dim_out = dim if dim_out is None else dim_out
        self.net = nn.Sequential(GEGLU(dim, inner), nn.Dropout(dropout), Linear(inner, dim_out))

    def chain_operands(self, ln):
        """(w1 packed, b1 packed, w2, b2) of the one-launch kernels, or None when this feed-forward does not fit them."""
        proj, out = self.net[0].proj, self.net[2]
        C = proj.in_features
        if out.bias is None or proj.bias is None or out.out_features != C or out.in_features != 4 * C:
            return None
        wp, bp, _ = self.net[0].folded(ln)
        w2, b2 = out._w()
        return wp, bp, w2, b2

    def forward(self, x, res=None, ln=None, ln_sums=None, post=None, sync=None):
        """ln: the LayerNorm in front (folded); ln_sums: row statistics of x from its producer (ops.gemm(row_sums=...)).  Where the library has the one-launch kernel for this width (C = 320: the
        64x64 level, whose [M, 4C] GEGLU intermediate is 84 MB) LayerNorm, both projections, the gating and the residual
        run in vd_ff_geglu_f16; elsewhere GEGLU GEMM -> output GEMM.
        post = (proj_out, alpha, pres [.., C], stat_img_rows): SpatialTransformer.proj_out (+ skip / context mixing) to be folded into
        the output GEMM -- one launch over [h | res] with the pre-multiplied weights (Linear._w_proj_fold) instead of two, the
        feed-forward's own output never stored.  Returns (proj_out's output, True) when it was, else the feed-forward's output
        as without post (the caller runs proj_out).  sync: called right before the folded launch (the one that reads pres)."""
        C = x.shape[-1]
        proj, out = self.net[0].proj, self.net[2]
        if (ln is not None and res is not None and out.bias is not None and proj.bias is not None and proj.in_features == C
                and out.out_features == C and out.in_features == 4 * C and ops.ff_geglu_supported(C)):
            wp, bp, _ = self.net[0].folded(ln)
            w2, b2 = out._w()
            return ops.ff_geglu(x, wp, bp, w2, b2, res, ln.eps)
        h = self.net[0](x, ln=ln, ln_sums=ln_sums)
        if (post is not None and res is not None and out.proj_fold_ok(post[0]) and res.shape[-1] == out.out_features
                and h.is_contiguous() and res.is_contiguous() and post[2].is_contiguous()):
            pconv, alpha, pres, hw = post
            w_cat, bm = out._w_proj_fold(pconv)
            m, n = h.numel() // h.shape[-1], out.out_features
            kw = {}
            # the same shapes Linear.forward hands to the weight-streaming kernel (16x16 / 8x8 levels), K now 5C
            if ops.GEMM_WSTREAM and out.in_features >= 2048 and n % 256 == 0 and m % 128 == 0 and m <= 4096:
                kw["w_stream_cat"] = out._w_proj_fold_stream(pconv)
            if sync is not None:
                sync()
            y = ops.gemm(h.view(m, -1), w_cat, a1=res.view(m, n), bias=bm, alpha=float(alpha), res=pres.view(m, n), want_stats=True,
                         stat_img_rows=int(hw), **kw)
            return y, True
        return out(h, res=res)


class CrossAttention(nn.Module, PackCache):
    """softmax(q k^T d^-1/2) v with q from x and k, v from the context (x itself when context is None)."""

    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.0):
        super().__init__()
        inner = dim_head * heads
        self.is_self = context_dim is None
        context_dim = query_dim if context_dim is None else context_dim
        self.scale = dim_head ** -0.5
        self.heads = heads
        self.inner = inner
        self.to_q = Linear(query_dim, inner, bias=False)
        self.to_k = Linear(context_dim, inner, bias=False)
        self.to_v = Linear(context_dim, inner, bias=False)
        self.to_out = nn.Sequential(Linear(inner, query_dim), nn.Dropout(dropout))

    def _w_qkv(self):
        return self._packed("qkv", (self.to_q.weight, self.to_k.weight, self.to_v.weight),
                            lambda: torch.cat([_h(self.to_q.weight), _h(self.to_k.weight), _h(self.to_v.weight)], 0))

    def _w_kv(self):
        return self._packed("kv", (self.to_k.weight, self.to_v.weight),
                            lambda: torch.cat([_h(self.to_k.weight), _h(self.to_v.weight)], 0))

    def project_context(self, context):
        """[B, L, Dc] -> fused [B, L, 2*inner] (k | v); step-invariant for a fixed context."""
        return ops.linear(context, self._w_kv())

    def _w_qkv_ln(self, ln):
        return self._packed("qkv_ln", (self.to_q.weight, self.to_k.weight, self.to_v.weight, ln.weight, ln.bias),
                            lambda: fold_layernorm(self._w_qkv(), None, ln))

    def _w_qkv_ln_stream(self, ln):
        """The weight of _w_qkv_ln in MFMA-fragment order for vd_gemm_wstream_epi_f16; keyed on the same parameters."""
        return self._packed("qkv_ln_stream", (self.to_q.weight, self.to_k.weight, self.to_v.weight, ln.weight, ln.bias),
                            lambda: pack.pack_linear_weight_stream(self._w_qkv_ln(ln)[0]))

    def _w_q_ln(self, ln):
        return self._packed("q_ln", (self.to_q.weight, ln.weight, ln.bias),
                            lambda: fold_layernorm(_h(self.to_q.weight), None, ln))

    def forward(self, x, context=None, res=None, kv=None, ln=None, qkv=None, ln_sums=None, out_sums=None, defer_out=False, repeat=1,
                ident_from=None, tome=None, sag=None, tile=None, blur_from=None, blur=None):
        """ln_sums: row statistics of x for `ln` (from x's producer); out_sums: zeroed fp32 [rows, 2] the output projection
        accumulates the row statistics of ITS output into (for the LayerNorm in front of the next block part).
        defer_out: return the attention output `a` WITHOUT the output projection (the caller folds to_out + res into its next
        launch: ops.ff_chain); only honoured on the one-launch cross-attention path, else the projected tensor comes back as usual.
        x [B, N, C] -> to_out(attn) (+ res fused).  ln: the LayerNorm in front of the block's q (and self k / v)
        projections, folded into them -- x is then the un-normalised input.  qkv: the fused self-attention projection when
        the caller has already computed it (SpatialTransformer's chained entry kernel).
        repeat > 1 (with a context; only with defer_out on the one-launch path, i.e. where vd_xattn_rep_f16 applies): x holds ONE
        replica of a classifier-free-guidance batch, context / kv all of them; the result has repeat times the samples of x.
        ident_from (self-attention only; perturbed-attention guidance): the samples from this index on take the identity attention
        map, i.e. to_out(to_v(ln(x))) (ops.attention(ident_from=...)), whoever computed qkv.
        tome (self-attention only; token merging, contract in include/vd_hip.h): None, or (H, W, r, metric[, sink]) with r > 0 --
        the tokens are an H x W grid, metric [B, N, C] is the block's un-normalised input, and the r most redundant source tokens
        are merged into their most similar destination: q | k | v as always -> ops.tome_match on the metric -> ops.tome_plan ->
        ops.tome_merge of the fused q | k | v -> ops.attention on N - r rows -> ops.tome_unmerge back to N rows -> to_out.
        sink, when given, is called with row_of (int32 [B, N]).  It does not combine with ident_from.
        sag (self-attention only; self-attention guidance): None, or a contiguous fp32 [n, N] view with n <= B: it receives the
        column mass of the attention map of the samples [0, n) (ops.sag_mass of their q | k), whoever computed qkv.  The attention
        itself is untouched: the output bits are those of the call without it.  It does not combine with tome.
        tile (self-attention only; HyperTile, contract in include/vd_hip.h): None, or (H, W, th, tw) -- the tokens are an H x W grid
        cut into th x tw tiles and every tile attends inside itself: q | k | v as always, whoever computed it -> ops.tile_tokens of
        the fused tensor -> ops.attention on its [B nt, th tw, *] slices (nt = (H / th) (W / tw)) -> ops.untile_tokens -> to_out.
        It does not combine with tome or sag.  With ident_from the identity rows are per token and commute with the permutation:
        the tiled batch takes ident_from * nt, so the perturbed samples are v, bit for bit, as without tiles.
        blur_from, blur (self-attention only; smoothed energy guidance, contract in include/vd_hip.h): None, or an index and
        (taps, R, gh, gw[, qb]) -- the samples from blur_from on attend with their projected queries blurred over the gh x gw token
        grid (ops.attention(blur_from=..., blur=..., qb=...)), whoever computed qkv; k and v are untouched.  It does not combine
        with ident_from, tome or tile."""
        c = self.inner
        if (blur_from is None) != (blur is None):
            raise ops.VdHipError("CrossAttention(blur_from=%r, blur=%r): the index and the blur setting go together" % (blur_from, blur))
        if blur_from is not None and not (context is None and kv is None):
            raise ops.VdHipError("CrossAttention(blur_from=%r): the query blur applies to self-attention only" % (blur_from,))
        if blur_from is not None and (ident_from is not None or tome is not None or tile is not None):
            raise ops.VdHipError("CrossAttention(blur_from=%r): the query blur does not combine with ident_from, tome or tile" % (blur_from,))
        if tile is not None and not (context is None and kv is None):
            raise ops.VdHipError("CrossAttention(tile=...): tiled attention applies to self-attention only")
        if tile is not None and (tome is not None or sag is not None):
            raise ops.VdHipError("CrossAttention(tile=...): tiled attention does not combine with tome or sag")
        if sag is not None and not (context is None and kv is None and tome is None):
            raise ops.VdHipError("CrossAttention(sag=...): the column mass is taken in an unmerged self-attention only")
        if tome is not None and not (context is None and kv is None):
            raise ops.VdHipError("CrossAttention(tome=...): token merging applies to self-attention only")
        if tome is not None and ident_from is not None:
            raise ops.VdHipError("CrossAttention(tome=..., ident_from=%r): token merging and the identity attention map do not combine" % (ident_from,))
        if ident_from is not None and not (context is None and kv is None):
            raise ops.VdHipError("CrossAttention(ident_from=%r): the identity attention map applies to self-attention only" % (ident_from,))
        if repeat > 1 and not (defer_out and (context is not None or kv is not None) and ln is not None and x.dim() == 3
                               and x.is_contiguous() and ops.xattn_supported(self.heads, c // self.heads)):
            raise ops.VdHipError("CrossAttention(repeat=%d): no cross-attention kernel with a batch period for this call "
                                 "(width %d, %d heads); replicate the input in front" % (repeat, c, self.heads))
        if context is None and kv is None:
            if qkv is not None:
                pass
            elif ln is None:
                qkv = ops.linear(x, self._w_qkv())
            else:
                w, b, cs = self._w_qkv_ln(ln)
                kw = {}
                if hip_layers.wstream_epi_level("qkv", x.numel() // x.shape[-1], x.shape[-1]):
                    kw["w_stream_epi"] = self._w_qkv_ln_stream(ln)
                qkv = ops.linear(x, w, b, colsum=cs, ln_eps=ln.eps, ln_sums=ln_sums, **kw)
            if sag is not None:
                n = sag.shape[0]
                if qkv.dim() != 3 or sag.dim() != 2 or not 0 < n <= qkv.shape[0] or sag.shape[1] != qkv.shape[1]:
                    raise ops.VdHipError("CrossAttention(sag=...): the mass buffer %s does not fit q|k|v %s" % (tuple(sag.shape), tuple(qkv.shape)))
                ops.sag_mass(qkv[:n, :, :c], qkv[:n, :, c:2 * c], self.heads, scale=self.scale, out=sag)
            if tile is not None:
                tH, tW, th, tw = (int(v) for v in tile)
                if qkv.dim() != 3 or tH * tW != qkv.shape[1] or th <= 0 or tw <= 0 or tH % th or tW % tw:
                    raise ops.VdHipError("CrossAttention(tile=%r): q|k|v %s is not [B, %d x %d, *] in whole tiles"
                                         % (tuple(tile), tuple(qkv.shape), tH, tW))
                nt = (tH // th) * (tW // tw)
                m = ops.tile_tokens(qkv, tH, tW, th, tw)
                ikw = {} if ident_from is None else {"ident_from": int(ident_from) * nt}
                a = ops.attention(m[..., :c], m[..., c:2 * c], m[..., 2 * c:], self.heads, scale=self.scale, **ikw)
                a = ops.untile_tokens(a, qkv.shape[0], tH, tW, th, tw)
            elif tome is not None:
                tH, tW, r, metric = tome[:4]
                if qkv.dim() != 3 or metric.dim() != 3 or metric.shape[:2] != qkv.shape[:2] or tH * tW != qkv.shape[1]:
                    raise ops.VdHipError("CrossAttention(tome=...): the metric %s / q|k|v %s are not [B, %d x %d, *]"
                                         % (tuple(metric.shape), tuple(qkv.shape), tH, tW))
                node_idx, node_max = ops.tome_match(metric, tH, tW)
                row_of = ops.tome_plan(node_idx, node_max, tH, tW, r)
                if len(tome) > 4 and tome[4] is not None:
                    tome[4](row_of)
                m = ops.tome_merge(qkv, row_of, tH, tW, r)
                a = ops.attention(m[..., :c], m[..., c:2 * c], m[..., 2 * c:], self.heads, scale=self.scale)
                a = ops.tome_unmerge(a, row_of, tH, tW, r)
            elif blur_from is not None:
                a = ops.attention(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], self.heads, scale=self.scale,
                                  blur_from=int(blur_from), blur=tuple(blur[:4]), qb=blur[4] if len(blur) > 4 else None)
            elif ident_from is None:
                a = ops.attention(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], self.heads, scale=self.scale)
            else:
                a = ops.attention(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], self.heads, scale=self.scale, ident_from=int(ident_from))
        else:
            if kv is None:
                kv = self.project_context(context)
            if ln is not None and x.dim() == 3 and x.is_contiguous() and ops.xattn_supported(self.heads, c // self.heads):
                # LayerNorm + to_q + attention over the (short) context in ONE launch: q never exists in memory
                w, b, cs = self._w_q_ln(ln)
                a = ops.xattn(x, w, b, cs, ln.eps, kv[..., :c], kv[..., c:], self.heads, scale=self.scale, repeat=repeat)
                if defer_out:
                    a._vd_deferred_out = True
                    return a
                return self.to_out[0](a, res=res, row_sums=out_sums)
            if ln is None:
                q = self.to_q(x)
            else:
                w, b, cs = self._w_q_ln(ln)
                q = ops.linear(x, w, b, colsum=cs, ln_eps=ln.eps)
            a = ops.attention(q, kv[..., :c], kv[..., c:], self.heads, scale=self.scale)
        return self.to_out[0](a, res=res, row_sums=out_sums)


def period_consumers(C, heads):
    """Whether a transformer block of width C can run its self-attention once per sample of a guided batch: behind attn1 the
    cross-attention (vd_xattn_rep_f16) and the chained tail with its first projection (vd_ff_chain_f16, VdFfChain.period_rows)
    must both be there to read the shared activation through the batch period."""
    return bool(hip_layers.LN_FOLD and heads > 0 and C % heads == 0 and ops.xattn_supported(heads, C // heads)
                and ops.ff_geglu_supported(C) and ops.ff_chain_supported(C, "pre"))


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, n_heads, d_head, dropout=0.0, context_dim=None, gated_ff=True, checkpoint=True,
                 disable_self_attn=False):
        super().__init__()
        assert not disable_self_attn
        self.attn1 = CrossAttention(query_dim=dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.ff = FeedForward(dim, dropout=dropout, glu=gated_ff)
        self.attn2 = CrossAttention(query_dim=dim, context_dim=context_dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.norm1 = LayerNorm(dim)
        self.norm2 = LayerNorm(dim)
        self.norm3 = LayerNorm(dim)
        self.checkpoint = checkpoint  # kept for config compatibility; inference never re-computes

    def forward(self, x, context=None, kv=None, qkv=None, ln1_sums=None, post=None, sync=None, repeat=1, ff_post=None, ident_from=None,
                tome=None, sag=None, tile=None, blur_from=None, blur=None):
        """post = (wp [C, C], bp, alpha, res [B, N, C], stat_img_rows): SpatialTransformer.proj_out (+ skip / context mixing) to be
        folded into the block's last launch.  Returns (tensor, True) when it was -- the tensor is then proj_out's output -- else
        the block output (the caller runs proj_out).  sync: called right before a launch that reads post's `res` (see
        SpatialTransformer.forward).
        ff_post = (proj_out, alpha, res, stat_img_rows): the same request where the feed-forward runs as separate GEMMs (widths 640 /
        1280): proj_out is folded into the feed-forward's output GEMM by pre-multiplied weights (FeedForward.forward(post=...)).
        repeat > 1: x (and post's res) hold ONE replica of a classifier-free-guidance batch, context / kv all of them.  Nothing
        reads the context before attn2, so attn1 runs on the one replica; the launches that first meet per-replica data -- the
        cross-attention and the chained tail -- read x / res through the batch period.  Only widths that have both kernels take
        repeat > 1 (period_consumers; C = 320): any other call is an error, the caller replicates in front of the block.  The result
        has repeat times the samples of x.
        ident_from: handed to attn1 (CrossAttention.forward); the replicas then differ from attn1 on, so it needs repeat == 1.
        tome: None, or (H, W, r, sink) of token merging: attn1 gets (H, W, r, x, sink) -- the metric is this block's un-normalised
        input.  With repeat > 1 the merge runs on the one replica attn1 sees.
        sag: handed to attn1 (CrossAttention.forward): the buffer that receives the column mass of its leading samples.
        tile: handed to attn1 (CrossAttention.forward): (H, W, th, tw) of HyperTile.  With repeat > 1 the tiled attention runs on
        the one replica attn1 sees.
        blur_from, blur: handed to attn1 (CrossAttention.forward); like ident_from they need repeat == 1."""
        if tome is not None:
            tome = (tome[0], tome[1], tome[2], x, tome[3] if len(tome) > 3 else None)
        if blur_from is not None and repeat > 1:
            raise ops.VdHipError("BasicTransformerBlock(repeat=%d, blur_from=%r): a perturbed replica cannot share attn1" % (repeat, blur_from))
        bkw = {} if blur_from is None else {"blur_from": blur_from, "blur": blur}
        if ident_from is not None and repeat > 1:
            raise ops.VdHipError("BasicTransformerBlock(repeat=%d, ident_from=%r): a perturbed replica cannot share attn1" % (repeat, ident_from))
        if repeat > 1 and not period_consumers(x.shape[-1], self.attn2.heads):
            raise ops.VdHipError("BasicTransformerBlock(repeat=%d): width %d has no consumers with a batch period" % (repeat, x.shape[-1]))
        if hip_layers.LN_FOLD:  # the three LayerNorms ride in the q/k/v, q and GEGLU projections (VD_EPI_LNFOLD)
            x = self.attn1(x, res=x, ln=self.norm1, qkv=qkv, ln_sums=ln1_sums, ident_from=ident_from, tome=tome, sag=sag, tile=tile, **bkw)
            C = x.shape[-1]
            fops = self.ff.chain_operands(self.norm3) if (x.is_contiguous() and ops.ff_geglu_supported(C)) else None
            if fops is not None and (ops.ff_chain_supported(C, "pre") or (post is not None and ops.ff_chain_supported(C, "post"))):
                # 64x64 level: attn2.to_out + x -> norm3 -> feed-forward -> + x [-> proj_out -> + x_in] in ONE launch
                w1p, b1p, w2, b2 = fops
                if repeat > 1 and not (x.dim() == 3 and ops.ff_chain_period_ok(x.shape[1])):
                    # (a 128-row tile of the chained tail would straddle two samples: replicate behind attn1)
                    if post is not None:
                        post = post[:3] + (ops.repeat_batch(post[3], repeat),) + post[4:]
                    x, repeat = ops.repeat_batch(x, repeat), 1
                kw = {}
                xin = x
                if ops.ff_chain_supported(C, "pre"):
                    a = self.attn2(x, context=context, res=x, kv=kv, ln=self.norm2, defer_out=True, repeat=repeat)
                    if getattr(a, "_vd_deferred_out", False):
                        wo, bo = self.attn2.to_out[0]._w()
                        kw.update(a=a, wo=wo, bo=bo)
                    else:
                        xin = a   # the projected tensor came back (the unfused cross-attention path)
                else:
                    xin = self.attn2(x, context=context, res=x, kv=kv, ln=self.norm2)
                folded = post is not None and ops.ff_chain_supported(C, "post")
                if folded:
                    wp, bp, alpha, pres, hw = post
                    kw.update(wp=wp, bp=bp, alpha=alpha, res=pres, want_stats=True, stat_img_rows=hw)
                if kw:
                    if folded and sync is not None:
                        sync()
                    if repeat > 1:   # x (with a) and pres stay un-replicated: the kernel reads them through the batch period
                        kw.update(repeat=repeat, stat_img_rows=x.shape[1])
                    out = ops.ff_chain(xin, w1p, b1p, w2, b2, self.norm3.eps, **kw)
                    return (out, True) if folded else out
                return self.ff(xin, res=xin, ln=self.norm3)
            # norm3's statistics: accumulated by attn2's output projection where the feed-forward runs as separate GEMMs (the
            # one-launch feed-forward of the 64x64 level normalises in registers)
            if repeat > 1:
                raise ops.VdHipError("BasicTransformerBlock(repeat=%d): the chained tail does not take this feed-forward" % repeat)
            C = x.shape[-1]
            s3 = None if ops.ff_geglu_supported(C) else ops.rowsum_take(x.numel() // C, x.device)
            x = self.attn2(x, context=context, res=x, kv=kv, ln=self.norm2, out_sums=s3)
            return self.ff(x, res=x, ln=self.norm3, ln_sums=getattr(x, "_vd_rowsums", None), post=ff_post, sync=sync)
        x = self.attn1(self.norm1(x), res=x, ident_from=ident_from, tome=tome, sag=sag, tile=tile, **bkw)
        x = self.attn2(self.norm2(x), context=context, res=x, kv=kv)
        x = self.ff(self.norm3(x), res=x)
        return x


class SpatialTransformer(nn.Module):
    """GroupNorm(eps 1e-6) -> 1x1 proj_in -> transformer block -> 1x1 proj_out -> + x_in, on [B, H, W, C]."""

    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0.0, context_dim=None, disable_self_attn=False):
        super().__init__()
        assert depth == 1
        self.in_channels = in_channels
        inner = n_heads * d_head
        self.norm = GroupNorm(32, in_channels, eps=1e-6, affine=True)
        self.proj_in = Conv2d(in_channels, inner, kernel_size=1, stride=1, padding=0)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(inner, n_heads, d_head, dropout=dropout, context_dim=context_dim,
                                   disable_self_attn=disable_self_attn) for _ in range(depth)])
        self.proj_out = Conv2d(inner, in_channels, kernel_size=1, stride=1, padding=0)
        with torch.no_grad():  # zero_module(proj_out), reference attention.py:249-253
            self.proj_out.weight.zero_()
            self.proj_out.bias.zero_()

    def project_context(self, context):
        return self.transformer_blocks[0].attn2.project_context(context)

    def shares_cfg_head(self):
        """True when forward(repeat > 1) reads the shared activation through the batch period of the one-launch cross-attention
        and of the chained tail (vd.run_unet hands a guided batch over un-replicated only then)."""
        return period_consumers(self.proj_in.out_channels, self.transformer_blocks[0].attn2.heads)

    def forward(self, x, context=None, kv=None, alpha=1.0, res=None, sync=None, repeat=1, ident_from=None, tome=None, sag=None, tile=None,
                blur_from=None, blur=None):
        """Returns alpha * (proj_out(...) + bias) + res, res defaulting to x (the block's own skip).
        alpha/res implement VD's context mixing sum_i r_i * ST_i(x) without extra passes.
        sync: callable invoked right before the ONE launch that reads `res` (the last of the block): the caller runs the blocks
        of several context types on forked streams and `res` is the previous type's output (vd.run_unet).
        repeat > 1: x holds ONE replica of a classifier-free-guidance batch (vd.run_unet(repeat=...)), context / kv all of them;
        the entry and the self-attention run once per sample and the output has repeat times the samples of x (the block's own
        skip only: res is None).
        ident_from (perturbed-attention guidance, needs repeat == 1): samples [ident_from, B) of x take the identity self-attention
        map in this block, whether q | k | v come from the chained entry kernel (width 320) or from the block's own projection.
        tome: None, or (r, sink) of token merging (r > 0): this block's self-attention merges r tokens of its H x W grid, the metric
        being the h that enters the transformer block (at width 320 the one the chained entry kernel returns).
        sag: None, or a contiguous fp32 [n, H W] view, n <= B: the block's self-attention writes the column mass of its attention map
        for the samples [0, n) into it (self-attention guidance); the block's output is untouched.
        tile: None, or (th, tw) of HyperTile: this block's self-attention runs inside th x tw tiles of its H x W grid
        (CrossAttention.forward(tile=(H, W, th, tw))), under repeat > 1 too: once per guidance pair.
        blur_from, blur = (taps, R[, qb]) (smoothed energy guidance, needs repeat == 1): samples [blur_from, B) of x attend in this
        block's self-attention with their queries blurred over its H x W grid (CrossAttention.forward(blur=(taps, R, H, W[, qb]))),
        whether q | k | v come from the chained entry kernel (width 320) or from the block's own projection."""
        assert repeat == 1 or blur_from is None, "a perturbed replica takes the replicated input"
        bkw = {}
        if blur_from is not None:
            bkw = {"blur_from": int(blur_from), "blur": (blur[0], int(blur[1]), x.shape[1], x.shape[2]) + tuple(blur[2:])}
        if tile is not None:
            tile = (x.shape[1], x.shape[2], int(tile[0]), int(tile[1]))
        if tome is not None:
            tome = (x.shape[1], x.shape[2], int(tome[0]), tome[1] if len(tome) > 1 else None)
        assert repeat == 1 or ident_from is None, "a perturbed replica takes the replicated input"
        assert repeat == 1 or res is None, "a shared input takes the block's own skip"
        if repeat > 1 and not self.shares_cfg_head():
            raise ops.VdHipError("SpatialTransformer(repeat=%d): width %d has no consumers with a batch period; replicate in front"
                                 % (repeat, self.proj_in.out_channels))
        B, H, W, C = x.shape
        blk = self.transformer_blocks[0]
        inner = self.proj_in.out_channels
        if hip_layers.LN_FOLD and x.is_contiguous() and ops.st_chain_supported(B, H * W, C, inner):
            # GroupNorm (as a per-sample affine map) -> proj_in -> h and LayerNorm(h) -> q | k | v in one launch
            g, b = self.norm._w()
            # (centred fp16 map: (x - fp16(mean)) * scale + shift', no |mean| / sigma amplification of the fp16 rounding)
            sc, sh, ct = ops.groupnorm_affine(x, g, b, groups=self.norm.num_groups, eps=self.norm.eps, centered=True)
            w1, b1 = self.proj_in._w()
            w2, b2, _ = blk.attn1._w_qkv_ln(blk.norm1)
            h, qkv = ops.row320_chain(x.view(B, H * W, C), sc, sh, H * W, w1, b1, w2, b2, blk.norm1.eps, center=ct)
            pres = x if res is None else res
            post = None
            if pres.is_contiguous() and self.proj_out.out_channels == inner and self.proj_out.bias is not None:
                wp, bp = self.proj_out._w()
                post = (wp, bp, float(alpha), pres.view(B, H * W, C), H * W)
            h = blk(h, context=context, kv=kv, qkv=qkv, post=post, sync=sync, repeat=repeat, ident_from=ident_from, tome=tome, sag=sag,
                    tile=tile, **bkw)
            if isinstance(h, tuple):   # proj_out (+ skip, alpha, statistics) ran inside the block's last launch
                out = h[0]
                st = ops.stats_of(out)
                out = out.view(repeat * B, H, W, C)
                if st is not None:
                    out._vd_stats = st
                return out
            if sync is not None:
                sync()
            if repeat > 1:
                pres = ops.repeat_batch(pres, repeat)
            return self.proj_out(h.view(repeat * B, H, W, -1), alpha=alpha, res=pres, want_stats=True)
        # norm1's row statistics ride on proj_in's epilogue (ops.gemm(row_sums=...)) instead of a vd_row_stats_f16 launch
        s1 = ops.rowsum_take(B * H * W, x.device) if hip_layers.LN_FOLD else None
        h = self.proj_in(self.norm(x, silu=False), row_sums=s1)
        ff_post = None
        if hip_layers.FF_PROJ_FOLD and hip_layers.LN_FOLD and repeat == 1 and self.proj_out.out_channels == inner:
            pres = x if res is None else res
            if pres.is_contiguous():   # proj_out rides in the feed-forward's output GEMM: that launch now is the one that reads res
                ff_post = (self.proj_out, float(alpha), pres, H * W)
        h = self.transformer_blocks[0](h.view(B, H * W, -1), context=context, kv=kv, ln1_sums=getattr(h, "_vd_rowsums", None),
                                       repeat=repeat, ff_post=ff_post, sync=sync if ff_post is not None else None, ident_from=ident_from,
                                       tome=tome, sag=sag, tile=tile, **bkw)
        if isinstance(h, tuple):   # proj_out (+ skip, alpha, statistics) ran inside the feed-forward's output GEMM
            out = h[0]
            st = ops.stats_of(out)
            out = out.view(B, H, W, C)
            if st is not None:
                out._vd_stats = st
            return out
        if sync is not None:
            sync()
        if repeat > 1:   # (proj_out's residual read has no batch period)
            res = ops.repeat_batch(x, repeat)
        return self.proj_out(h.view(repeat * B, H, W, -1), alpha=alpha, res=x if res is None else res, want_stats=True)
