"""Host tables of windowed (MultiDiffusion, Bar-Tal et al. 2023) sampling: where the windows lie on the canvas latent, the
weight a window gives each of its pixels, the reciprocal of the weights that land on a canvas pixel, and how the windows of a
step are split into UNet forwards of one shape; and for regional prompts (MultiDiffusion section 4.3: one context per masked
region) the region masks and the reciprocal of weight x mask summed over regions and windows.  Pure numpy; touches no device.
The kernels that read these tables: ops.window_gather / ops.window_merge / ops.window_merge_masked (contract in
include/vd_hip.h); the samplers' use of them: ddim._window_args."""
import numpy as np


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an int, got %r" % (name, v))
    return int(v)


def int_pair(name, v):
    """(y, x) of an int or a pair of ints."""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("%s must be an int or a pair (y, x), got %r" % (name, v))
        return _int(name, v[0]), _int(name, v[1])
    return (_int(name, v),) * 2


def _axis(name, L, l, s, wrap, multiple):
    if l < 1 or l > L:
        raise ValueError("window: the %s side %d must lie in [1, canvas %d]" % (name, l, L))
    if l % multiple:
        raise ValueError("window: the %s side %d is not a multiple of the data net's down-sampling factor %d" % (name, l, multiple))
    if s < 1:
        raise ValueError("window_stride: the %s stride must be >= 1, got %d" % (name, s))
    if s > l:
        raise ValueError("window_stride: the %s stride %d is larger than the window side %d and would leave holes" % (name, s, l))
    if wrap:
        return list(range(0, L, s))
    return list(range(0, L - l, s)) + [L - l]


def window_offsets(H, W, window, stride, wrap=False, multiple=1):
    """int32 [Wn, 2] rows (oy, ox) of the windows on an H x W canvas, row-major with y outer and x inner.  window, stride: an
    int or a pair (y, x).  Per axis of canvas length L, window l and stride s: range(0, L - l, s) and then L - l, so the last
    window lies flush against the edge and any canvas >= the window is covered (the overlap counts are then not uniform).  With
    `wrap` the x axis is range(0, W, s) and a window's columns are (ox + j) % W: a 360-degree panorama with no seam.
    ValueError for a window larger than the canvas, a stride < 1 or > the window (holes), non-ints and bools, and a window side
    that is not a multiple of `multiple` (the data net's total down-sampling factor, ddim._window_args passes it)."""
    H, W, multiple = _int("H", H), _int("W", W), _int("multiple", multiple)
    if not isinstance(wrap, (bool, np.bool_)):
        raise ValueError("window_wrap must be a bool, got %r" % (wrap,))
    if H < 1 or W < 1 or multiple < 1:
        raise ValueError("window_offsets: H, W and multiple must be >= 1, got %r" % ((H, W, multiple),))
    (h, w), (sy, sx) = int_pair("window", window), int_pair("window_stride", stride)
    ys = _axis("y", H, h, sy, False, multiple)
    xs = _axis("x", W, w, sx, bool(wrap), multiple)
    return np.array([(oy, ox) for oy in ys for ox in xs], dtype=np.int32).reshape(-1, 2)


def window_weights(h, w, kind):
    """fp32 [h, w]: the weight of each pixel of a window in the fusion.  'uniform': ones (MultiDiffusion).  'gaussian': the
    outer product of g(i) = exp(-((i - (n - 1) / 2) / n)^2 / (2 * 0.01)) per axis of length n (the Mixture-of-Diffusers weighting;
    its normalisation cancels against window_inv_den), computed in float64 and rounded once.  'tent': the outer product of
    t(i) = min(i + 1, n - i) per axis, small integers and so exact in fp32 (the tiled VAE's default, lib/model_zoo/vae_tiles.py):
    a tile's weight falls to its minimum at the tile's edge, so weight / denominator is continuous across tile edges where
    uniform averaging leaves a step."""
    h, w = _int("h", h), _int("w", w)
    if h < 1 or w < 1:
        raise ValueError("window_weights: h and w must be >= 1, got %r" % ((h, w),))
    if kind == "uniform":
        return np.ones((h, w), dtype=np.float32)
    if kind == "gaussian":
        g = lambda n: np.exp(-((np.arange(n, dtype=np.float64) - (n - 1) / 2.0) / n) ** 2 / (2 * 0.01))
        return np.outer(g(h), g(w)).astype(np.float32)
    if kind == "tent":
        t = lambda n: np.minimum(np.arange(n) + 1, n - np.arange(n)).astype(np.float64)
        return np.outer(t(h), t(w)).astype(np.float32)
    raise ValueError("window_weight must be 'uniform', 'gaussian' or 'tent', got %r" % (kind,))


def window_inv_den(H, W, offsets, weights, wrap):
    """fp32 [H, W]: 1 / (the sum of the weights that land on the pixel) -- float64 sum over the windows of `offsets`
    (window_offsets) of the fp32 `weights` (window_weights), float64 reciprocal, one rounding.  Every pixel is covered by the
    construction of the offsets, so every entry is finite; ValueError for a table that leaves a pixel bare."""
    weights = np.asarray(weights, dtype=np.float32)
    h, w = weights.shape
    den = np.zeros((H, W), dtype=np.float64)
    cols = np.arange(w)
    for oy, ox in np.asarray(offsets).reshape(-1, 2):
        xs = (int(ox) + cols) % W if wrap else int(ox) + cols
        den[int(oy):int(oy) + h, xs] += weights.astype(np.float64)
    if not np.all(den > 0):
        raise ValueError("window_inv_den: the windows leave %d canvas pixels uncovered" % int(np.sum(~(den > 0))))
    return (1.0 / den).astype(np.float32)


def window_chunks(Wn, window_batch):
    """(nc, m): the Wn windows of a step run as nc = ceil(Wn / window_batch) UNet forwards of m = ceil(Wn / nc) window slots per
    sample.  Every forward of a step has the same shape, so one K/V cache, one set of GEMM plans and one captured shape serve all
    of them; the nc * m - Wn unused slots of the last forward repeat the call's last window and the merge ignores them."""
    Wn, window_batch = _int("Wn", Wn), _int("window_batch", window_batch)
    if Wn < 1 or window_batch < 1:
        raise ValueError("window_batch must be an int >= 1 (and Wn >= 1), got %r" % ((Wn, window_batch),))
    nc = -(-Wn // window_batch)
    return nc, -(-Wn // nc)


def region_masks_arg(masks, H, W):
    """fp32 [R, H, W]: the region masks of a regional-prompt call (x_info['region_masks']) on the H x W canvas latent grid, from
    a real or bool array [R, H, W] or [R, 1, H, W].  ValueError for another rank or shape, R < 1, and values that are not
    finite or lie outside [0, 1]."""
    m = np.asarray(masks)
    if m.dtype == np.bool_:
        m = m.astype(np.float32)
    if m.dtype.kind not in "fiu":
        raise ValueError("region_masks must be real or bool, got dtype %s" % (m.dtype,))
    if m.ndim == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.ndim != 3 or tuple(m.shape[1:]) != (H, W):
        raise ValueError("region_masks has shape %s, expected [R, %d, %d] or [R, 1, %d, %d]" % (np.shape(masks), H, W, H, W))
    if m.shape[0] < 1:
        raise ValueError("region_masks needs at least one region, got shape %s" % (np.shape(masks),))
    m = np.ascontiguousarray(m, dtype=np.float32)
    if not np.all(np.isfinite(m)) or m.min() < 0 or m.max() > 1:
        raise ValueError("region_masks must hold finite values in [0, 1]")
    return m


def region_inv_den(H, W, offsets, weights, masks, wrap):
    """fp32 [H, W]: 1 / (the sum over the regions r and the windows k that cover the pixel of wm = fp32(wgt_k x mask_r), the
    products the merge kernel forms) -- float64 sum, float64 reciprocal, one rounding.  With one region whose mask is all ones
    this is window_inv_den, bit for bit.  ValueError for pixels no region owns (or no window covers)."""
    weights = np.asarray(weights, dtype=np.float32)
    masks = np.asarray(masks, dtype=np.float32)
    h, w = weights.shape
    den = np.zeros((H, W), dtype=np.float64)
    cols = np.arange(w)
    for mask in masks:
        for oy, ox in np.asarray(offsets).reshape(-1, 2):
            ys, xs = slice(int(oy), int(oy) + h), (int(ox) + cols) % W if wrap else int(ox) + cols
            den[ys, xs] += (weights * mask[ys, xs]).astype(np.float64)        # the fp32 product, rounded, then widened
    if not np.all(den > 0):
        raise ValueError("region_masks leave %d canvas pixels uncovered; add a background region" % int(np.sum(~(den > 0))))
    return (1.0 / den).astype(np.float32)
