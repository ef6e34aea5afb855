"""AutoencoderKL (KL-f8) inference path with the reference's surface (lib/model_zoo/autokl.py:14-49 there):
`encode(x)` -> sampled latent, `decode(z)` -> image in [0,1]; NCHW in / NCHW out, HIP kernels in between.
Training-only pieces of the reference (loss, discriminator, optimisers; autokl.py:57-140) are out of scope.

Not in the reference: the tiled path (`tile=`, `tile_stride=`, `tile_wrap=`, `tile_weight=`, `tile_batch=` on decode /
decode_scaled / encode / encode_scaled; lib/model_zoo/vae_tiles.py).  The canvas is cut into overlapping tiles, every tile goes
through the network as a sample of its own, and one kernel (ops.tile_blend) fuses the tiles' outputs.  The result is NOT the
whole-canvas result: every tile has its own GroupNorm statistics, its own mid-block attention and its own zero padding at tile
borders away from the wrap -- the geometry the autoencoder was trained at.  Without `tile` a call is the whole-canvas call."""
import torch
import torch.nn as nn

from vd_hip import ops

from . import vae_tiles
from .autokl_modules import Decoder, Encoder
from .common.get_model import register
from .distributions import DiagonalGaussianDistribution
from .hip_layers import Conv2d


def _img16(x):
    if not x.is_cuda:
        raise RuntimeError("AutoencoderKL needs GPU tensors: this package has no CPU path")
    return x.to(torch.float16).contiguous()


def _canvas_hw(x, what):
    if x.dim() != 4:
        raise ValueError("tile: %s must be [B, C, H, W], got shape %s" % (what, tuple(x.shape)))
    return int(x.shape[2]), int(x.shape[3])


_TILE_CACHE_SIZE = 8


@register("autoencoderkl")
class AutoencoderKL(nn.Module):
    def __init__(self, ddconfig, lossconfig, embed_dim):
        super().__init__()
        assert lossconfig is None, "the LPIPS/discriminator loss is training-only and not part of this package"
        self.encoder = Encoder(**ddconfig)
        self.decoder = Decoder(**ddconfig)
        assert ddconfig["double_z"]
        self.quant_conv = Conv2d(2 * ddconfig["z_channels"], 2 * embed_dim, 1)
        self.post_quant_conv = Conv2d(embed_dim, ddconfig["z_channels"], 1)
        self.embed_dim = embed_dim
        self.factor = vae_tiles.vae_factor(ddconfig.get("ch_mult", (1, 2, 4, 8)))
        self._tile_cache = {}       # device copies of a tiled geometry's tables

    # ---- the tiled path ------------------------------------------------------------------------------------------------------
    def _tile_tables(self, plan, which, device):
        """(gather int32 [nc, m, 2], blend int32 [nc, m, 2], wgt fp32, inv_den fp32) of `plan` on `device`, kept per geometry."""
        key = (which,) + plan["key"] + (str(device),)
        t = self._tile_cache.get(key)
        if t is None:
            while len(self._tile_cache) >= _TILE_CACHE_SIZE:
                self._tile_cache.pop(next(iter(self._tile_cache)))
            t = tuple(torch.from_numpy(a).to(device) for a in (plan["gather"], plan["blend"]) + vae_tiles.tile_tables(plan))
            self._tile_cache[key] = t
        return t

    def _tiled(self, x16, plan, which, run, **blend):
        """The chunks of `plan` in ascending order: cut the tiles of x16 [B, C, H, W] (ops.window_gather), `run` them as a batch
        [B m, C, h, w] -> channels-last [B m, oh, ow, Co], and sum them onto the canvas (ops.tile_blend)."""
        B, C = x16.shape[:2]
        gather, offs, wgt, inv_den = self._tile_tables(plan, which, x16.device)
        (gh, gw), (OH, OW), nc, m, wrap = plan["gather_hw"], plan["out_hw"], plan["nc"], plan["m"], plan["wrap"]
        acc = out = None
        for k in range(nc):
            win = ops.window_gather(x16, gather[k], gh, gw, wrap)
            y = run(win.view(B * m, C, gh, gw))
            y = y.reshape((B, m) + tuple(y.shape[1:]))
            if nc > 1 and acc is None:
                acc = torch.empty((B, y.shape[-1], OH, OW), device=x16.device, dtype=torch.float32)
            out = ops.tile_blend(y, offs[k], wgt, inv_den, OH, OW, plan["valid"][k], wrap, k == 0, k == nc - 1, acc=acc, **blend)
        return out

    def _tile_plan(self, x, tile_keys, encode):
        """vae_tiles.tile_plan of a call on x (the latent of a decode, the image of an encode), or None for the plain call.
        Validates the keys; touches no device."""
        if not tile_keys:
            return None
        H = W = 1                                                   # not looked at without `tile`
        if tile_keys.get("tile") is not None:
            H, W = _canvas_hw(x, "the image" if encode else "the latent")
            if encode:
                H, W = vae_tiles.encode_canvas(H, W, self.factor)
        return vae_tiles.tile_plan(tile_keys, H, W, self.factor, encode=encode)

    def _posterior(self, x, **tile_keys):
        plan = self._tile_plan(x, tile_keys, True)
        if plan is None:
            h = self.encoder(_img16(x), in_scale=2.0, in_shift=-1.0)  # x*2-1 folded into the first conv's gather
            return DiagonalGaussianDistribution(self.quant_conv(h))
        run = lambda t: self.quant_conv(self.encoder(t, in_scale=2.0, in_shift=-1.0))
        return DiagonalGaussianDistribution(self._tiled(_img16(x), plan, "encode", run, out_nhwc=True))

    @torch.no_grad()
    def encode(self, x, out_posterior=False, noise=None, **tile_keys):
        post = self._posterior(x, **tile_keys)
        return post if out_posterior else post.sample(noise).to(x.dtype)

    @torch.no_grad()
    def encode_scaled(self, x, scale, noise=None, **tile_keys):
        """scale * encode(x) with the latent scale folded into the sampling kernel (VD_v2_0.vae_encode)."""
        return self._posterior(x, **tile_keys).sample(noise, scale=scale).to(x.dtype)

    @torch.no_grad()
    def decode(self, z, **tile_keys):
        return self.decode_scaled(z, 1.0, **tile_keys)

    @torch.no_grad()
    def decode_scaled(self, z, inv_scale, **tile_keys):
        """decode(inv_scale * z); the scale rides in the first 1x1 conv's gather, clamp((x+1)/2) in the final
        NHWC->NCHW store (tiled: in the blend of the tiles)."""
        plan = self._tile_plan(z, tile_keys, False)
        if plan is None:
            h = self.post_quant_conv(_img16(z), in_layout="nchw", in_scale=float(inv_scale))
            dec = self.decoder(h)
            return ops.nhwc_to_nchw(dec, scale=0.5, shift=0.5, clamp01=True).to(z.dtype)
        run = lambda t: self.decoder(self.post_quant_conv(t, in_layout="nchw", in_scale=float(inv_scale)))
        return self._tiled(_img16(z), plan, "decode", run, scale=0.5, shift=0.5, clamp01=True).to(z.dtype)
