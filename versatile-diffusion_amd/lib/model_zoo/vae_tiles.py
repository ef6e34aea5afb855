"""Host plan of the tiled path through the KL-f8 autoencoder (AutoencoderKL.decode / encode with `tile=`): which tiles of a
canvas run through the network, in which chunks, and the tables the blend kernel reads.  The geometry is that of windowed
sampling, so the offsets, the chunking, the weights and the denominator come from lib/model_zoo/windows.py as they are; this
module validates the keys and puts the tables on the right grid.  Pure numpy; touches no device.  The kernels that read the
tables: ops.window_gather and ops.tile_blend (contract in include/vd_hip.h).

The keys (keyword arguments of decode / decode_scaled / encode / encode_scaled, VD_v2_0.vae_decode / vae_encode pass them on):
  tile         an int or (h, w) in LATENT pixels, for decode and encode alike; a tile covers f h x f w image pixels with
               f = 2 ** (len(ch_mult) - 1).  Absent or None: tiling is off, the call is today's call.
  tile_stride  an int or a pair, 1 <= s <= tile; default three quarters of the tile per axis (at least 1)
  tile_wrap    bool, default False: the x axis wraps around (a 360-degree panorama decodes with no seam at x = 0)
  tile_weight  'tent' (default), 'uniform' or 'gaussian' (windows.window_weights)
  tile_batch   an int >= 1, default 8: the most tiles per sample in one pass through the network"""
import numpy as np

from . import windows

TILE_KEYS = ("tile", "tile_stride", "tile_wrap", "tile_weight", "tile_batch")


def vae_factor(ch_mult):
    """The autoencoder's total down-sampling factor: 8 for KL-f8's ch_mult (1, 2, 4, 4)."""
    return 2 ** (len(ch_mult) - 1)


def _as_tile_error(e):
    # windows.py words its errors for the samplers' window_* keys; the rules are the same, the key names are ours
    return ValueError(str(e).replace("window", "tile"))


def tile_plan(keys, H, W, factor, encode=False):
    """The plan of a tiled decode (encode=False) or encode (True) of an H x W canvas LATENT from the tile_* keys, or None when
    the call is the plain whole-canvas call: no `tile`, or a single tile without wrap.  ValueError, by the rules and in the
    wording of windows._axis and ddim._window_args, for a tile larger than the canvas, a tile side < 1, a stride < 1 or > the
    tile, a non-int or a bool where an int is wanted, a non-bool tile_wrap, an unknown tile_weight, tile_batch < 1, and any other
    tile_* key given without `tile`; TypeError for a key that is no tile key.  Every key is checked also when the plan has a
    single tile.
    The plan: the geometry "key" (H, W, h, w, sy, sx, wrap, weight, nc, m), "n" tiles run as "nc" passes of "m" slots per sample,
    "valid" [nc] slots that count in each pass (the unused slots of the last pass repeat the last tile), "gather" int32
    [nc, m, 2] and "gather_hw" -- the offsets and the tile size ops.window_gather cuts with, on the grid of the network's input
    (decode: latent; encode: image pixels) -- and "blend" int32 [nc, m, 2], "tile_hw" and "out_hw" on the grid of its output
    (decode: pixels, (f h, f w) and (f H, f W); encode: latent, (h, w) and (H, W)).  The plan is cheap (a call makes one every
    time); the two tables of the output grid, which are images, come from tile_tables(plan) and are kept by the caller."""
    unknown = sorted(k for k in keys if k not in TILE_KEYS)
    if unknown:
        raise TypeError("unexpected keyword argument(s) %s; the tiling keys are %s" % (", ".join(unknown), ", ".join(TILE_KEYS)))
    tile = keys.get("tile")
    if tile is None:
        given = [k for k in TILE_KEYS[1:] if k in keys]
        if given:
            raise ValueError("%s needs `tile` (pass the canvas size for a plain call)" % given[0])
        return None
    H, W, f = int(H), int(W), int(factor)
    try:
        h, w = windows.int_pair("tile", tile)
        stride = keys.get("tile_stride")
        sy, sx = (max(3 * h // 4, 1), max(3 * w // 4, 1)) if stride is None else windows.int_pair("tile_stride", stride)
        wrap, weight = keys.get("tile_wrap", False), keys.get("tile_weight", "tent")
        offsets = windows.window_offsets(H, W, (h, w), (sy, sx), wrap)
        wrap = bool(wrap)
        windows.window_weights(1, 1, weight)                                # the kind alone; the table is tile_tables' work
        n = offsets.shape[0]
        nc, m = windows.window_chunks(n, keys.get("tile_batch", 8))
    except ValueError as e:
        raise _as_tile_error(e) from None
    if n == 1 and not wrap:
        return None
    fo = 1 if encode else f
    padded = np.ascontiguousarray(np.concatenate([offsets, np.repeat(offsets[-1:], nc * m - n, axis=0)]).reshape(nc, m, 2))
    gather, blend = (padded * np.int32(f), padded) if encode else (padded, padded * np.int32(f))
    return {"key": (H, W, h, w, sy, sx, wrap, weight, nc, m), "n": n, "nc": nc, "m": m,
            "valid": [min(m, n - k * m) for k in range(nc)], "gather": np.ascontiguousarray(gather, dtype=np.int32),
            "gather_hw": (f * h, f * w) if encode else (h, w), "blend": np.ascontiguousarray(blend, dtype=np.int32),
            "tile_hw": (fo * h, fo * w), "out_hw": (fo * H, fo * W), "wrap": wrap, "weight": weight}


def tile_tables(plan):
    """(wgt fp32 [oh, ow], inv_den fp32 [OH, OW]) of a plan, on the grid the blend writes: windows.window_weights of the tile
    there and windows.window_inv_den of the plan's "n" tiles.  For a decode these are images (a 512 x 2048 canvas: 4 MB, and
    a float64 pass per tile to build it), so AutoencoderKL keeps them per geometry."""
    (oh, ow), (OH, OW) = plan["tile_hw"], plan["out_hw"]
    wgt = windows.window_weights(oh, ow, plan["weight"])
    offsets = plan["blend"].reshape(-1, 2)[:plan["n"]]
    return wgt, windows.window_inv_den(OH, OW, offsets, wgt, plan["wrap"])


def encode_canvas(Hp, Wp, factor):
    """(H, W): the canvas latent of an Hp x Wp image under a tiled encode.  ValueError for an image side that is not `factor`
    times an integer (the plain encode rounds such a side down inside the network; tiles could not be laid on it)."""
    Hp, Wp, f = int(Hp), int(Wp), int(factor)
    for name, L in (("y", Hp), ("x", Wp)):
        if L < f or L % f:
            raise ValueError("tile: the image's %s side %d is not the autoencoder's down-sampling factor %d times an integer"
                             % (name, L, f))
    return Hp // f, Wp // f
