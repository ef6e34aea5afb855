"""The tiled VAE path restated on the CPU, in numpy and on the fp32 oracle only: the blend kernel's chain with its roundings written
out, the exact (float64) blend, and the tiled decode / encode on the oracle run per tile and blended.  Shared by the CPU and
the GPU tests."""
import numpy as np
import torch

from deepcache_cases import FWD_TOL  # noqa: F401  (the project's bound on one forward, re-exported for the tests)

from lib.model_zoo import windows


def geometry(H, W, tile, stride, wrap=False, weight="tent", f=1, encode=False):
    """The tables of one tiled geometry, built from lib/model_zoo/windows.py alone: H x W the canvas LATENT, tile / stride in
    latent pixels, f the autoencoder's factor.  "offs" int32 [n, 2] on the latent grid; "in_offs" / "in_hw" what the tiles are
    cut with (decode: latent, encode: pixels); "out_offs", "wgt", "inv_den", "PH", "PW" on the grid the blend writes (decode:
    pixels, encode: latent)."""
    h, w = windows.int_pair("tile", tile)
    offs = windows.window_offsets(H, W, (h, w), stride, wrap)
    fi, fo = (f, 1) if encode else (1, f)
    wgt = windows.window_weights(fo * h, fo * w, weight)
    return {"H": H, "W": W, "h": h, "w": w, "f": f, "wrap": bool(wrap), "offs": offs, "in_offs": offs * np.int32(fi),
            "in_hw": (fi * h, fi * w), "out_offs": offs * np.int32(fo), "wgt": wgt, "PH": fo * H, "PW": fo * W,
            "inv_den": windows.window_inv_den(fo * H, fo * W, offs * np.int32(fo), wgt, bool(wrap))}


def _cols(ox, pw, PW, wrap):
    c = np.arange(pw) + int(ox)
    return c % PW if wrap else c


def coverage(offs, ph, pw, PH, PW, wrap):
    """int [PH, PW]: how many tiles cover each canvas pixel."""
    n = np.zeros((PH, PW), dtype=np.int64)
    for oy, ox in np.asarray(offs).reshape(-1, 2):
        n[int(oy):int(oy) + ph, _cols(ox, pw, PW, wrap)] += 1
    return n


def blend_sum_restated(tiles, offs, wgt, PH, PW, wrap, acc=None):
    """np.float32 [RB, C, PH, PW]: the accumulator of vd_tile_blend_f16 after the tiles fp16 [RB, n, ph, pw, C] -- per canvas
    element the chain a = fmaf(wgt, tile, a) over the covering tiles in ascending order (the product formed in float64, where
    fp32 x fp16 is exact; the sum rounded to fp32), continued from `acc` when given."""
    tiles = np.asarray(tiles)
    RB, n, ph, pw, C = tiles.shape
    w64 = np.asarray(wgt, dtype=np.float32).astype(np.float64)
    a = np.zeros((RB, C, PH, PW), dtype=np.float32) if acc is None else np.array(acc, dtype=np.float32)
    for k, (oy, ox) in enumerate(np.asarray(offs).reshape(-1, 2)):
        ys, xs = slice(int(oy), int(oy) + ph), _cols(ox, pw, PW, wrap)
        t = tiles[:, k].astype(np.float64).transpose(0, 3, 1, 2)                          # [RB, C, ph, pw]
        a[:, :, ys, xs] = (w64 * t + a[:, :, ys, xs].astype(np.float64)).astype(np.float32)
    return a


def blend_finish_restated(a, inv_den, scale=1.0, shift=0.0, clamp01=False, out_nhwc=False):
    """np.float16: the last launch's tail on the fp32 sum a [RB, C, PH, PW] -- v = a * inv_den rounded to fp32, then
    fmaf(v, scale, shift) (formed in float64, rounded to fp32), then fminf(fmaxf(v, 0), 1) when clamp01, then one rounding to
    fp16; [RB, C, PH, PW], or [RB, PH, PW, C] with out_nhwc."""
    with np.errstate(invalid="ignore"):
        v = (np.asarray(a, dtype=np.float32) * np.asarray(inv_den, dtype=np.float32)).astype(np.float32)
        v = (v.astype(np.float64) * float(np.float32(scale)) + float(np.float32(shift))).astype(np.float32)
        if clamp01:
            v = np.fmin(np.fmax(v, np.float32(0)), np.float32(1))
        out = v.astype(np.float16)
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1)) if out_nhwc else out


def blend_restated(tiles, offs, wgt, inv_den, PH, PW, wrap, scale=1.0, shift=0.0, clamp01=False, out_nhwc=False):
    """np.float16: the contract of vd_tile_blend_f16 (include/vd_hip.h) step by step in np.float32 with one fp16 rounding."""
    a = blend_sum_restated(tiles, offs, wgt, PH, PW, wrap)
    return blend_finish_restated(a, inv_den, scale, shift, clamp01, out_nhwc)


def blend_ref64(tiles, offs, wgt, inv_den, PH, PW, wrap, scale=1.0, shift=0.0, clamp01=False, out_nhwc=False):
    """np.float64: the same value with every operation in float64 and no rounding."""
    tiles = np.asarray(tiles)
    RB, n, ph, pw, C = tiles.shape
    w64 = np.asarray(wgt).astype(np.float64)
    a = np.zeros((RB, C, PH, PW), dtype=np.float64)
    for k, (oy, ox) in enumerate(np.asarray(offs).reshape(-1, 2)):
        ys, xs = slice(int(oy), int(oy) + ph), _cols(ox, pw, PW, wrap)
        a[:, :, ys, xs] += w64 * tiles[:, k].astype(np.float64).transpose(0, 3, 1, 2)
    v = a * np.asarray(inv_den).astype(np.float64) * float(scale) + float(shift)
    if clamp01:
        v = np.clip(v, 0.0, 1.0)
    return np.ascontiguousarray(v.transpose(0, 2, 3, 1)) if out_nhwc else v


def cut_tiles(x, offs, th, tw, wrap):
    """[n] tensors [B, C, th, tw]: the tiles of x [B, C, H, W] by torch indexing, columns taken modulo W with `wrap`."""
    W = x.shape[-1]
    return [x[:, :, int(oy):int(oy) + th][..., torch.from_numpy(_cols(ox, tw, W, wrap))] for oy, ox in np.asarray(offs)]


def decode_raw(sd, p, z, ch_mult=(1, 2, 4, 4), num_res_blocks=2):
    """oracle.vd_oracle.vae_decode up to the decoder's raw output (before its clamp((h + 1) / 2, 0, 1)), from the oracle's own
    layers in the oracle's order; test_tile_vae_cpu pins clamp((decode_raw + 1) / 2) to O.vae_decode bit for bit."""
    import torch.nn.functional as F
    from oracle import vd_oracle as O
    nres = len(ch_mult)
    d = p + ".decoder"
    h = O._conv(sd, p + ".post_quant_conv", z)
    h = O._conv(sd, d + ".conv_in", h, padding=1)
    h = O._vae_resnet(sd, d + ".mid.block_1", h)
    h = O._vae_attn(sd, d + ".mid.attn_1", h)
    h = O._vae_resnet(sd, d + ".mid.block_2", h)
    for lvl in reversed(range(nres)):
        for blk in range(num_res_blocks + 1):
            h = O._vae_resnet(sd, d + ".up.%d.block.%d" % (lvl, blk), h)
        if lvl != 0:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = O._conv(sd, d + ".up.%d.upsample.conv" % lvl, h, padding=1)
    return O._conv(sd, d + ".conv_out", F.silu(O._gn(sd, d + ".norm_out", h, 1e-6)), padding=1)


def _blend_per_tile(outs, geo, **tail):
    """float64 blend of a list of per-tile oracle outputs [B, C, oh, ow] (fp32 torch)."""
    tiles = np.stack([o.double().numpy().transpose(0, 2, 3, 1) for o in outs], axis=1)    # [B, n, oh, ow, C]
    return blend_ref64(tiles, geo["out_offs"], geo["wgt"], geo["inv_den"], geo["PH"], geo["PW"], geo["wrap"], **tail)


def tiled_decode_ref(sd, z, geo, p="vae.image", **vae_kw):
    """float64 [B, 3, f H, f W]: the tiled decode of the latent z [B, zc, H, W] (what decode() is handed: already divided by
    the latent scale) on the fp32 oracle -- every tile of geo (geometry(..., f=f)) decoded on its own, tile after tile so
    that a tile's bits do not depend on its place in a batch, the raw outputs blended in float64, then clip(0.5 v + 0.5, 0, 1)."""
    with torch.no_grad():
        outs = [decode_raw(sd, p, t.float().contiguous(), **vae_kw)
                for t in cut_tiles(z, geo["in_offs"], geo["in_hw"][0], geo["in_hw"][1], geo["wrap"])]
    return _blend_per_tile(outs, geo, scale=0.5, shift=0.5, clamp01=True)


def tiled_moments_ref(sd, im, geo, p="vae.image", **vae_kw):
    """float64 [B, 2 zc, H, W]: the moments of a tiled encode of the image im [B, 3, f H, f W] in [0, 1] on the fp32 oracle --
    O.vae_encode_moments per tile of geo (geometry(..., f=f, encode=True)), blended in float64."""
    from oracle import vd_oracle as O
    with torch.no_grad():
        outs = [O.vae_encode_moments(sd, p, t.float().contiguous(), **vae_kw)
                for t in cut_tiles(im, geo["in_offs"], geo["in_hw"][0], geo["in_hw"][1], geo["wrap"])]
    return _blend_per_tile(outs, geo)
