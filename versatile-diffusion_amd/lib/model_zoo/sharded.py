"""Batch-axis sharding of the sampling path across the GPUs of a node: one process per GPU (torchrun), full weight
replica per rank, NO collective inside the DDIM loop, one all_gather of the decoded images at the end (RCCL over xGMI
when the backend is "nccl"; gloo in the CPU tests).

The reference has no inference-time multi-GPU path (app.py:279-283 uses one device); samples are independent
(GroupNorm / LayerNorm / attention are per sample), so the batch axis shards with the CFG pair of a sample kept on one
rank.  The full initial latent is drawn ONCE with the reference's seed rule (`torch.manual_seed(seed + 100)`,
app.py:309) and sliced, never re-seeded per rank, so 1-GPU and N-GPU runs produce the same images.
"""
import torch
import torch.distributed as dist

from ..app_ops import latent_mask


def shard_bounds(total, world_size, rank):
    """Contiguous, balanced [lo, hi) slice of `total` samples for `rank` (earlier ranks take the remainder)."""
    base, rem = divmod(total, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def draw_initial_latent(shape, seed, dtype=torch.float32, device_generator=False, device=None):
    """Full-batch x_T with the reference's seed convention (`seed + 100`, app.py:309).

    Default: from a HOST generator -- identical on every rank and for every world size, but NOT the numbers the
    reference's unsharded call draws (it seeds the global generator and draws `torch.randn(shape, device=cuda,
    dtype=fp16)` on the device, ddim.py:105).  device_generator=True reproduces exactly that draw (global
    `torch.manual_seed(seed + 100)`, then randn on `device` in `dtype`): a single-rank sharded run then starts from the
    same x_T as `DDIMSampler.sample(x_info={'type': 'image'})` after the app's seeding.  Device RNG streams depend on
    the tensor's shape, so this mode is only offered for the whole batch on one rank (world size 1)."""
    if device_generator:
        torch.manual_seed(int(seed) + 100)
        return torch.randn(tuple(shape), device=device, dtype=dtype)
    g = torch.Generator(device="cpu").manual_seed(int(seed) + 100)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float32).to(dtype)


def sample_seeds(seed, lo, hi):
    """Per-sample noise seeds of samples [lo, hi) of a batch seeded with `seed` (DPMSolverSDESampler's x_info["seeds"]):
    seed * 2^32 + global sample index, so a sample keeps its seed -- and with it its noise -- however the batch is split."""
    seed = int(seed)
    if not 0 <= seed < 2 ** 31:
        raise ValueError("sample_seeds: seed must lie in [0, 2^31), got %r" % (seed,))
    return [seed * 2 ** 32 + i for i in range(int(lo), int(hi))]


def _slice_ctx(c_info, lo, hi):
    """The context of samples [lo, hi).  A list or tuple conditioning holds one tensor per region (regional prompts): every
    entry is sliced along its batch -- slicing the list itself would cut regions, not samples."""
    out = dict(c_info)
    for k in ("conditioning", "unconditional_conditioning"):
        v = c_info[k]
        out[k] = type(v)(c[lo:hi] for c in v) if isinstance(v, (list, tuple)) else v[lo:hi]
    return out


def sample_sharded(sample_fn, decode_fn, shape, c_info_list, seed, device, group=None, gather=True, device_generator=False):
    """Run `sample_fn(x_T_local, c_info_list_local) -> latents` and `decode_fn(latents) -> images` on this rank's slice
    of the batch and all_gather the images.

    shape: full-batch latent shape [B, C, h, w]; c_info_list: reference-style context dicts holding the FULL batch.
    Returns [B, 3, H, W] images on every rank (or the local slice when gather=False)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    B = shape[0]
    if B < world:  # deterministic from the arguments: every rank raises, nobody is left waiting in the all_gather
        raise ValueError("sample_sharded: batch %d < world size %d (every rank needs at least one sample)" % (B, world))
    if torch.device(device).type == "cuda":
        torch.cuda.set_device(device)  # kernels and the RCCL communicator of this rank live on its own GPU
    lo, hi = shard_bounds(B, world, rank)
    if device_generator:
        if world != 1:
            raise ValueError("sample_sharded: device_generator=True reproduces the unsharded sampler's x_T and needs world size 1")
        x_T = draw_initial_latent(shape, seed, dtype=torch.float16, device_generator=True, device=device)
    else:
        x_T = draw_initial_latent(shape, seed)[lo:hi].to(device)
    local_ctx = [_slice_ctx(ci, lo, hi) for ci in c_info_list]
    images = decode_fn(sample_fn(x_T, local_ctx))
    if world == 1 or not gather:
        return images
    # ragged slices: pad to the largest slice so a single fixed-size all_gather does it
    max_n = shard_bounds(B, world, 0)[1]
    pad = images
    if images.shape[0] < max_n:
        pad = torch.cat([images, images.new_zeros((max_n - images.shape[0],) + tuple(images.shape[1:]))])
    bufs = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(bufs, pad.contiguous(), group=group)
    parts = []
    for r, b in enumerate(bufs):
        rlo, rhi = shard_bounds(B, world, r)
        parts.append(b[: rhi - rlo])
    return torch.cat(parts)


def vd_sample_sharded(net, sampler, steps, shape, c_info_list, seed, guidance_scale=7.5, eta=0., group=None,
                      images=None, fidelity=0., device_generator=False, mask=None, guidance_rescale=0.,
                      cache_interval=1, cache_depth=1, window=None, window_stride=None, window_wrap=False,
                      window_weight="uniform", window_batch=8, freeu=None, region_masks=None, pag_scale=None,
                      pag_layers=None, tome_ratio=None, tome_max_downsample=None, vae_tile=None, vae_tile_stride=None,
                      vae_tile_wrap=None, vae_tile_weight=None, vae_tile_batch=None, sag_scale=None, sag_blur_sigma=None,
                      hypertile=None, hypertile_max_downsample=None, apg_eta=None, apg_norm_threshold=None, apg_momentum=None,
                      seg_scale=None, seg_blur_sigma=None, seg_layers=None):
    """t2i / image-variation / multi-context sampling + kl-f8 decode of a full batch, sharded over the process group.

    images + fidelity > 0: image variation with fidelity (reference app.py:355-371) -- `images` is THIS RANK's slice of
    the input images [n_local, 3, H, W] in [0, 1]; x0 = vae_encode(images) and only the first int(steps * (1 - fidelity))
    DDIM steps run (ddim.py:97-103).  Posterior and forward-process noise are slices of seeded full-batch draws (see
    sample_fn), so the result does not depend on the world size.

    images + mask: inpainting (not in the reference) -- `mask` is the pixel mask of this rank's `images` [n_local, 1, H, W]
    or a broadcast [1, 1, H, W] (1 = regenerate, 0 = keep), turned into the latent mask by app_ops.latent_mask(mode="max").
    x0 is encoded as above also when fidelity == 0, and then the full schedule runs from x_T.

    guidance_rescale: the samplers' c_info['guidance_rescale'] (ddim.cfg_rescale_factors), set next to the scale; a sample's
    factors do not depend on the rank or the slice it runs in.

    cache_interval, cache_depth: the samplers' x_info['cache_interval'] / ['cache_depth'] (DeepCache sampling, ddim._cache_args;
    1 = off).  The full / shallow schedule depends on the step number alone, so it is the same on every rank.

    window, window_stride, window_wrap, window_weight, window_batch: the samplers' x_info keys of the same names (windowed /
    MultiDiffusion sampling, ddim._window_args; window=None = off, and then none of them is set).  `shape` is the canvas; the
    windows lie on the latent's H and W, so a rank's slice of the batch sees the same plan as the whole batch.

    freeu: the samplers' x_info['freeu'] (FreeU, vd.freeu_setting: (b1, b2, s1, s2) or a dict of them; None = off, and then the
    key is not set).  A sample's filtered skips do not depend on the batch it runs in, so neither on the rank.

    pag_scale, pag_layers: the samplers' x_info['pag_scale'] and x_info['pag_layers'] (perturbed-attention guidance, vd._pag_arg;
    None = the key is not set).  The perturbed replica is per sample, so a rank's slice sees what the whole batch would.

    sag_scale, sag_blur_sigma: the samplers' x_info['sag_scale'] and x_info['sag_blur_sigma'] (self-attention guidance, vd._sag_arg;
    None = the key is not set).  The attention map, the mask and the second forward are per sample, so a rank's slice sees what the
    whole batch would.

    tome_ratio, tome_max_downsample: the samplers' x_info['tome_ratio'] and x_info['tome_max_downsample'] (token merging,
    vd._tome_arg; None = the key is not set).  The merge is per sample, so a rank's slice sees what the whole batch would.

    hypertile, hypertile_max_downsample: the samplers' x_info['hypertile'] and x_info['hypertile_max_downsample'] (HyperTile,
    vd._hypertile_arg; None = the key is not set).  The tiles are cut per sample, so a rank's slice sees what the whole batch would.

    seg_scale, seg_blur_sigma, seg_layers: the samplers' x_info keys of the same names (smoothed energy guidance, vd._seg_arg; None =
    the key is not set).  The perturbed replica and its query blur are per sample, so a rank's slice sees what the whole batch would.

    apg_eta, apg_norm_threshold, apg_momentum: the samplers' x_info keys of the same names (adaptive projected guidance,
    vd._apg_arg; None = the key is not set).  The projection, the norm and the running direction are per sample, so a rank's slice
    sees what the whole batch would.

    region_masks: the samplers' x_info['region_masks'] (regional prompts on the windowed path, ddim._window_args; None = off, and
    then the key is not set; it needs `window`).  A context's 'conditioning' may then be a list of one [B, L, D] tensor per
    region, sliced per sample (_slice_ctx).  The masks are shared by the samples, so every rank sees the same ones.

    vae_tile, vae_tile_stride, vae_tile_wrap, vae_tile_weight, vae_tile_batch: the autoencoder's tile, tile_stride, tile_wrap,
    tile_weight and tile_batch (the tiled VAE path, lib/model_zoo/vae_tiles.py), passed to both net.vae_encode and
    net.vae_decode; None = the key is not passed, and with all five None the calls are the plain ones.  Tiles lie on a
    sample's H and W, so a rank's slice decodes to what the whole batch would."""
    if mask is not None and images is None:
        raise ValueError("vd_sample_sharded: mask needs images")
    vae_keys = {k: v for k, v in (("tile", vae_tile), ("tile_stride", vae_tile_stride), ("tile_wrap", vae_tile_wrap),
                                  ("tile_weight", vae_tile_weight), ("tile_batch", vae_tile_batch)) if v is not None}

    def sample_fn(x_T, ctxs):
        for ci in ctxs:
            ci["unconditional_guidance_scale"] = guidance_scale
            ci["guidance_rescale"] = guidance_rescale
        lshape = [x_T.shape[0]] + list(shape[1:])
        if images is not None and (fidelity > 0. or mask is not None):
            # every random number of this branch comes from a seeded FULL-batch draw sliced to this rank's samples, like
            # x_T: the forward-process noise of q_sample is the rank's slice of the x_T draw itself (the `x0_noise`
            # extension of DDIMSampler), the VAE posterior noise a second draw (seed + 1) -- never the rank's own device
            # generator, so a 1-GPU and an N-GPU run give the same images (and two ranks never repeat each other's noise)
            world = dist.get_world_size(group) if dist.is_initialized() else 1
            rank = dist.get_rank(group) if dist.is_initialized() else 0
            lo, hi = shard_bounds(shape[0], world, rank)
            post = draw_initial_latent(shape, int(seed) + 1)[lo:hi].to(x_T.device)
            x0 = net.vae_encode(images, which="image", noise=post, **vae_keys)
            x_info = {"type": "image", "x0": x0, "x0_noise": x_T}
            if fidelity > 0.:
                x_info["x0_forward_timesteps"] = int(steps * (1 - fidelity))
            else:
                x_info["xt"] = x_T
            if mask is not None:
                x_info["inpaint_mask"] = latent_mask(mask.to(x_T.device), mode="max",
                                                     factor=images.shape[-1] // shape[-1])
        else:
            x_info = {"type": "image", "xt": x_T}
        x_info["cache_interval"], x_info["cache_depth"] = cache_interval, cache_depth
        if window is not None:
            x_info.update(window=window, window_stride=window_stride, window_wrap=window_wrap, window_weight=window_weight,
                          window_batch=window_batch)
        if region_masks is not None:
            x_info["region_masks"] = region_masks
        if freeu is not None:
            x_info["freeu"] = freeu
        if pag_scale is not None:
            x_info["pag_scale"] = pag_scale
        if pag_layers is not None:
            x_info["pag_layers"] = pag_layers
        if sag_scale is not None:
            x_info["sag_scale"] = sag_scale
        if sag_blur_sigma is not None:
            x_info["sag_blur_sigma"] = sag_blur_sigma
        if tome_ratio is not None:
            x_info["tome_ratio"] = tome_ratio
        if tome_max_downsample is not None:
            x_info["tome_max_downsample"] = tome_max_downsample
        if hypertile is not None:
            x_info["hypertile"] = hypertile
        if hypertile_max_downsample is not None:
            x_info["hypertile_max_downsample"] = hypertile_max_downsample
        for key, value in (("apg_eta", apg_eta), ("apg_norm_threshold", apg_norm_threshold), ("apg_momentum", apg_momentum),
                           ("seg_scale", seg_scale), ("seg_blur_sigma", seg_blur_sigma), ("seg_layers", seg_layers)):
            if value is not None:
                x_info[key] = value
        from .dpm_solver import DPMSolverSDESampler
        if isinstance(sampler, DPMSolverSDESampler):
            world = dist.get_world_size(group) if dist.is_initialized() else 1
            rank = dist.get_rank(group) if dist.is_initialized() else 0
            x_info["seeds"] = sample_seeds(seed, *shard_bounds(shape[0], world, rank))
        if len(ctxs) == 1:
            z, _ = sampler.sample(steps=steps, shape=lshape, x_info=x_info, c_info=ctxs[0], eta=eta, verbose=False)
        else:
            z, _ = sampler.sample_multicontext(steps=steps, shape=lshape, x_info=x_info, c_info_list=ctxs, eta=eta,
                                               verbose=False)
        return z

    return sample_sharded(sample_fn, lambda z: net.vae_decode(z, which="image", **vae_keys), shape, c_info_list, seed, net.device,
                          group=group, device_generator=device_generator)
