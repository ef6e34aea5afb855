"""Device versions of the tensor work the reference does in app.py around the model calls:
the 'Simple' colour adjustment of image variation (app.py:373-379) and the `adjust_rank` focus control of the image
context (app.py:48-127).  Same call signatures as there; the arithmetic runs in hand-written HIP kernels (vd_hip).
`latent_mask` (not in the reference) turns a pixel inpainting mask into the latent mask of x_info["inpaint_mask"]."""
import numpy as np
import torch

from vd_hip import ops


def color_adjust_simple(imout, cx):
    """imout: [B,3,H,W] decoded images (or a list of [3,H,W]); cx: the input image [1,3,H,W] / [3,H,W].  Returns the
    adjusted images in the form they came in (reference app.py:373-379: per channel (x - mean) / std * std_cx + mean_cx,
    clamped to [0,1])."""
    as_list = isinstance(imout, (list, tuple))
    x = torch.stack(list(imout)) if as_list else imout
    dt = x.dtype
    out = ops.color_adjust(x.to(torch.float16).contiguous(), cx.to(device=x.device, dtype=torch.float16).contiguous()).to(dt)
    return list(out) if as_list else out


def latent_mask(mask, mode="max", factor=8):
    """Pixel inpainting mask [B or 1, 1, H, W] (1 = regenerate, 0 = keep; float or bool) -> fp32 latent mask
    [B or 1, 1, H / factor, W / factor] for x_info["inpaint_mask"] (factor: the VAE's downsampling, 8 for kl-f8).
    mode "max" regenerates every latent pixel that touches a masked pixel; "area" takes the masked fraction (a soft mask).
    Runs once per call, off the step path, so plain torch pooling does it."""
    if mode not in ("max", "area"):
        raise ValueError("latent_mask: mode must be 'max' or 'area', got %r" % (mode,))
    if mask.dim() != 4 or mask.shape[1] != 1 or mask.shape[2] % factor or mask.shape[3] % factor:
        raise ValueError("latent_mask: expected a [B or 1, 1, H, W] mask with H and W multiples of %d, got %s"
                         % (factor, tuple(mask.shape)))
    pool = torch.nn.functional.max_pool2d if mode == "max" else torch.nn.functional.avg_pool2d
    return pool(mask.float(), factor)


def region_masks(pixel_masks, mode="area", factor=8, background=True):
    """Pixel masks of the regions of a regional-prompt call [R, 1, Hp, Wp] (1 = the region owns the pixel; float or bool) ->
    (fp32 [R or R + 1, Hp / factor, Wp / factor] for x_info["region_masks"], whether a region was appended).  Every mask is
    pooled by latent_mask(mode, factor).  background=True appends clip(1 - sum_r m_r, 0, 1) as a last region when that is non-zero
    anywhere: the call then needs one more conditioning, the prompt of whatever the masks leave open."""
    if pixel_masks.dim() != 4 or pixel_masks.shape[0] < 1:
        raise ValueError("region_masks: expected [R, 1, H, W] pixel masks with R >= 1, got %s" % (tuple(pixel_masks.shape),))
    m = latent_mask(pixel_masks, mode=mode, factor=factor)[:, 0]
    if background:
        rest = (1.0 - m.sum(0)).clamp(0.0, 1.0)
        if bool((rest != 0).any()):
            return torch.cat([m, rest[None]]), True
    return m, False


class adjust_rank(object):
    """Focus control of the image context: rescale the leading singular components of the (row-centred) CLIP token matrix
    -- lvl < 0.5 suppresses the top `max_drop_rank[0] + 1` ("semantic") components, lvl > 0.5 suppresses components
    `max_drop_rank[1]` .. q-1 and everything beyond rank q ("style") -- then restore the tensor's std.  Same constructor,
    call signature and level -> scale curves as the reference class (app.py:56-127); the decomposition and the
    reconstruction run in vd_adjust_rank_f16 (fp32 subspace iteration on the device instead of torch.pca_lowrank)."""

    def __init__(self, max_drop_rank=[1, 5], q=20):
        self.max_semantic_drop_rank = max_drop_rank[0]
        self.max_style_drop_rank = max_drop_rank[1]
        self.q = q
        t0, y00 = np.exp((0 - 0.5) * 2), -self.max_semantic_drop_rank
        t1, y01 = np.exp((0.5 - 0.5) * 2), 1
        self.t2y0_semf = lambda t: (np.exp((t - 0.5) * 2) - t0) / (t1 - t0) * (y01 - y00) + y00
        sx1 = self.max_semantic_drop_rank + 1
        self.x2y_semf = lambda x, y0: (x - 0) / (sx1 - 0) * (1 - y0) + y0
        u0, z00 = np.exp((1 - 0.5) * 2), -(q - self.max_style_drop_rank)
        self.t2y0_styf = lambda t: (np.exp((t - 0.5) * 2) - u0) / (t1 - u0) * (1 - z00) + z00
        tx0, tx1 = q - 1, self.max_style_drop_rank - 1
        self.x2y_styf = lambda x, y0: (x - tx0) / (tx1 - tx0) * (1 - y0) + y0

    def scales(self, lvl):
        """(f [q] multipliers of the singular values, keep_remainder) for a focus level in [0, 1], lvl != 0.5."""
        f = np.ones(self.q, dtype=np.float64)
        if lvl < 0.5:
            assert lvl >= 0
            for xi in range(0, self.max_semantic_drop_rank + 1):
                f[xi] = max(self.x2y_semf(xi, self.t2y0_semf(lvl)), 0)
            return f, True
        assert lvl <= 1
        for xi in range(self.max_style_drop_rank, self.q):
            f[xi] = max(self.x2y_styf(xi, self.t2y0_styf(lvl)), 0)
        return f, False

    def __call__(self, x, lvl):
        if lvl == 0.5:
            return x
        f, keep = self.scales(lvl)
        dt = x.dtype
        x16 = x.to(torch.float16).contiguous()
        g = torch.from_numpy((f - (1.0 if keep else 0.0)).astype(np.float32)).to(x16.device)
        return ops.adjust_rank(x16, g, 1.0 if keep else 0.0).to(dt)
