"""VD_v2_0: the multi-flow container (VAEs, context encoders, diffusers + DDPM schedule) behind the reference's
model contract (lib/model_zoo/vd.py:41-455 there): `ctx_encode`, `vae_encode`, `vae_decode`, `apply_model`,
`apply_model_multicontext`, `q_sample`, the 12 schedule buffers, `.to()` semantics and the state-dict layout.

Execution differs from the reference: `apply_model*` converts nothing to NCHW in between -- the latent enters the
first conv straight from NCHW, every block runs channels-last fp16 on HIP kernels, skip connections are read in
place (no torch.cat), context mixing is folded into the proj_out epilogues, and the step-invariant context K/V
projections can be cached across DDIM steps (`c_info['kv_cache']`, set up by DDIMSampler).
"""
from functools import partial

import os
import threading

import numpy as np
import numpy.random as npr
import torch
import torch.nn as nn

from vd_hip import ops

from ..log_service import print_log
from .common.get_model import get_model, register
from .diffusion_utils import extract_into_tensor, make_beta_schedule, timestep_embedding
from .hip_layers import PackCache

symbol = "vd"


class String_Reg_Buffer(nn.Module):
    """A config entry given as a plain string is kept as a byte buffer (reference vd.py:28-39)."""

    def __init__(self, output_string):
        super().__init__()
        self.register_buffer("output_string", torch.tensor(list(bytes(output_string, "utf8")), dtype=torch.uint8))

    @torch.no_grad()
    def forward(self, *args, **kwargs):
        return bytes(self.output_string.tolist()).decode()


CTX_FORK = os.environ.get("VD_CTX_FORK", "1") != "0"   # development switch: 0 = the context types of a block one after the other
# run_unet(repeat > 1): the first context block of a step with ONE context type takes the un-replicated activation and runs its entry
# and self-attention once per sample (SpatialTransformer.forward(repeat=...)); 0 = replicate in front of the block
CFG_HEAD_SHARE = os.environ.get("VD_CFG_HEAD_SHARE", "1") != "0"
# Round 6: the low-resolution levels of the UNet (rows per sample <= VD_BATCH_FORK_HW, default 256 = the 16x16 and 8x8 levels and the
# middle block) as TWO forked branches of half the batch each.  Measured (profiles/HISTORY.md R6.8): image variation at CFG batch 16
# +1.6 .. +2.5 % images/s (each half is the CFG-batch-8 problem the planner's rules were measured on, and the halves' latency-bound
# launches fill each other's gaps); text-to-image at CFG batch 8 -4 % (halves of 4 samples: split-K convolutions that each fill
# the chip cannot run side by side).  So: "auto" = batches of >= VD_BATCH_FORK_MIN (16) samples with ONE context type (the context
# types of a multi-context stage are forked already); 0 = never, 1 = every even batch with one context type.
BATCH_FORK = os.environ.get("VD_BATCH_FORK", "auto")
BATCH_FORK_HW = int(os.environ.get("VD_BATCH_FORK_HW", "256"))
BATCH_FORK_MIN = int(os.environ.get("VD_BATCH_FORK_MIN", "16"))
_SIDE = {}
_SIDE_LOCK = threading.Lock()


def _side_streams(device, n, kind="ctx"):
    """Side streams of the forked branches, one set per (thread, device): the sampler's eager warm-up step and its captured
    step run on one thread and use the same streams, so the per-stream workspaces of vd_hip.ops (keyed by stream) are
    allocated once, outside any capture; two threads never put their branches -- and split-K slabs -- on one stream.
    torch hands out streams round-robin from a fixed pool of 32 per device, so a new torch.cuda.Stream() can BE a stream this
    process already uses: one another live thread forks onto, one of this thread's own side streams, or the stream the fork
    starts from (the capture stream of torch.cuda.graph, or a sampler's).  A branch "forked" onto the caller's own stream waits for
    and is joined through events of that same stream, which ends a stream capture in a crash of the runtime -- which streams meet
    depends on how many streams the process has created before.  So the n streams handed out are distinct from each other, from
    this thread's streams of the other kinds and from the CURRENT stream; a kept stream that is the current one is passed over
    for this call (capture_stream() gives a sampler a stream that is none of them, so that does not happen to its captures).
    Cost of passing over, accepted: the thread's list can grow by one stream per distinct current stream that was a kept one (at
    most the 32 handles of the pool), and the replacement can be first used -- and its ops workspaces first allocated -- inside a
    capture of a caller that captures on a stream of its own choosing; those workspaces then live in that graph's pool, as the
    capture stream's own do."""
    me = threading.get_ident()
    main = torch.cuda.current_stream(device).cuda_stream
    with _SIDE_LOCK:
        lst = _SIDE.setdefault((kind, device.index, me), [])
        pick = [s for s in lst if s.cuda_stream != main][:n]
        if len(pick) < n:
            alive = {t.ident for t in threading.enumerate()} | {me}
            for k in [k for k in _SIDE if k[2] not in alive]:
                del _SIDE[k]
            _SIDE[(kind, device.index, me)] = lst
            taken = {s.cuda_stream for k, l in _SIDE.items() if k[1] == device.index for s in l}   # other threads', and this thread's own
            taken.add(main)
            for _ in range(64):
                if len(pick) >= n:
                    break
                s = torch.cuda.Stream(device=device)
                if s.cuda_stream not in taken:
                    taken.add(s.cuda_stream)
                    lst.append(s)
                    pick.append(s)
            if len(pick) < n:
                raise RuntimeError("run_unet: no side stream left that neither this thread nor another one already uses")
        return pick


def side_stream_handles(device=None):
    """Raw handles of every side stream kept for forked branches (all threads): a stream a caller creates to capture forwards on
    should be none of them, so that the captured step forks onto the streams its eager warm-up step used."""
    idx = None if device is None else torch.device(device).index
    with _SIDE_LOCK:
        return {s.cuda_stream for k, l in _SIDE.items() if idx is None or k[1] == idx for s in l}


def capture_stream(device=None):
    """A stream to capture forwards on that is no kept side stream (torch's pool hands the same 32 streams out again and again): the
    captured step then forks onto the very streams its eager warm-up step used."""
    busy = side_stream_handles(device)
    s = None
    for _ in range(64):
        s = torch.cuda.Stream(device=device)
        if s.cuda_stream not in busy:
            break
    return s


class _BranchOrder(object):
    """Start order of forked branches (the context types of a block, the half-batch branches).  A later branch starts behind
    the fork event, recorded on the caller's stream behind everything the branches read -- unless an earlier branch BUILT
    weight packs (PackCache.builds moved during its host walk): their writes are on that branch's stream, and the other branch
    may read them, so the later branches start behind an event recorded after that branch.  Forwards that build nothing
    (every forward once the weights have been used, and any captured step) keep fully parallel branches."""

    def __init__(self, main):
        self.gate = torch.cuda.Event()
        self.gate.record(main)

    def enter(self, stream, first=False):
        """In front of a branch's launches on `stream` (first: the branch on the fork's own stream); returns a token."""
        if not first:
            stream.wait_event(self.gate)
        return PackCache.builds

    def leave(self, stream, token):
        """Behind the branch's launches."""
        if PackCache.builds != token:
            self.gate = torch.cuda.Event()
            self.gate.record(stream)


# ---- the context K/V cache (c_info['kv_cache']) ---------------------------------------------------------------------
# A plain dict that callers start as {} and share between forwards on one context: id(context module) -> its projected K/V,
# next to two entries under string keys -- the modules by the same ids (so that entries can be refreshed without a forward)
# and the ids whose tensor still holds the projection of an earlier context.  Only the four functions below know this layout.
_KV_MODULES, _KV_STALE = "_modules", "_stale"


def kv_lookup(cache, module, c):
    """K/V of context `c` [B, L, Dc] for the context block `module`: projected on first use and kept in `cache`; an entry marked
    stale is refilled in its own storage (a captured graph reads that buffer: new context, same storage).  None without a cache."""
    if cache is None:
        return None
    mid = id(module)
    kv = cache.get(mid)
    if kv is None:
        kv = cache[mid] = module[0].project_context(c)
        cache.setdefault(_KV_MODULES, {})[mid] = module
    elif mid in cache.get(_KV_STALE, ()):
        kv.copy_(module[0].project_context(c))
        cache[_KV_STALE].discard(mid)
    return kv


def kv_mark_stale(cache):
    """The forwards that share `cache` get a new context: every entry is recomputed in place on its next use."""
    cache[_KV_STALE] = set(cache.get(_KV_MODULES, ()))


def kv_refreshable(cache):
    """Whether kv_refresh can bring `cache` up to date, i.e. a forward has filled it."""
    return _KV_MODULES in cache


def kv_refresh(cache, c):
    """Recompute every stale entry in place from context `c` (prepared like the forward's: VD_v2_0._prep) without a forward."""
    stale = cache.get(_KV_STALE, ())
    for mid, module in cache[_KV_MODULES].items():
        if mid in stale:
            cache[mid].copy_(module[0].project_context(c))
    cache[_KV_STALE] = set()


# ---- DeepCache (x_info['deep_cache']): reuse the deep features of the previous full forward ------------------------------------
# Ma, Fang, Wang, "DeepCache: Accelerating Diffusion Models for Free" (CVPR 2024).  A forward in "store" mode is today's forward
# plus one side copy of the tensor that enters the last `depth` skip loads; a forward in "reuse" mode runs only the blocks in front
# of the first `depth` saves and behind those loads, and reads that copy in place of everything in between.
_SAVES, _LOADS = ("save", "save_hidden_feature"), ("load", "load_hidden_feature")


def deep_cut(net, depth):
    """(a, b) of the cached walk at `depth` for a 2-D data net (or its flat i_order + m_order + o_order list).  With S / L the
    positions of the n saves / loads of the walk: a = S[depth - 1] + 1, so steps[0:a] ends with the depth-th save, and
    b = L[n - depth], so steps[b:] begins with the depth-th load from the end and pops exactly those `depth` skips, last in first
    out.  The stored feature is the tensor about to enter steps[b] (in front of the load's concat).  ValueError unless
    1 <= depth <= n - 1 and the net is 2-D: the 0-D text flow has nothing deep to skip."""
    if isinstance(net, (list, tuple)):
        order = list(net)
    else:
        from .openaimodel import UNetModel0D_Next
        if isinstance(net, UNetModel0D_Next) or not all(hasattr(net, k) for k in ("i_order", "m_order", "o_order")):
            raise ValueError("deep_cut: DeepCache needs a 2-D data net (x_info['type'] == 'image'), got %s" % type(net).__name__)
        order = list(net.i_order) + list(net.m_order) + list(net.o_order)
    S = [i for i, s in enumerate(order) if s in _SAVES]
    L = [i for i, s in enumerate(order) if s in _LOADS]
    n = len(S)
    if len(L) != n:
        raise ValueError("deep_cut: the walk has %d saves and %d loads" % (n, len(L)))
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 1 <= int(depth) <= n - 1:
        raise ValueError("deep_cut: depth must be an int in [1, %d], got %r" % (n - 1, depth))
    return S[int(depth) - 1] + 1, L[n - int(depth)]


class DeepCache(object):
    """What x_info['deep_cache'] = (cache, "store" | "reuse") hands from a full forward to the shallow ones behind it: the depth
    of the cut and the kept feature (channels-last fp16, all repeat * B rows; allocated by the first "store" forward, which must
    run outside graph capture -- a captured forward only ever dereferences that one buffer)."""

    def __init__(self, depth=1):
        self.depth = depth
        self.buf = None
        self.key = None     # (data net, depth) of the forward that filled buf

    def store(self, h, key):
        if self.buf is None or self.buf.shape != h.shape or self.buf.device != h.device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("deep_cache: the kept buffer must exist before a 'store' forward is captured into a graph")
            self.buf = torch.empty(h.shape, device=h.device, dtype=h.dtype)
        self.buf.copy_(h)
        self.key = key

    def load(self, key, like):
        """The kept feature for a walk whose innermost kept skip is `like` (the tensor the first load concatenates it with)."""
        if self.buf is None or self.key != key:
            raise ValueError("deep_cache: 'reuse' needs a 'store' forward of the same net at the same depth first")
        if self.buf.shape[:-1] != like.shape[:-1] or self.buf.device != like.device:
            raise ValueError("deep_cache: the kept feature has shape %s, this forward needs %s + channels"
                             % (tuple(self.buf.shape), tuple(like.shape[:-1])))
        return self.buf


def _deep_arg(x_info):
    """x_info['deep_cache'] validated: None, or (DeepCache, "store" | "reuse") on the 2-D image flow."""
    deep = x_info.get("deep_cache")
    if deep is None:
        return None
    if x_info.get("type") != "image":
        raise ValueError("deep_cache applies to x_info['type'] == 'image' only, got %r" % (x_info.get("type"),))
    if not (isinstance(deep, (tuple, list)) and len(deep) == 2 and isinstance(deep[0], DeepCache) and deep[1] in ("store", "reuse")):
        raise ValueError("x_info['deep_cache'] must be (DeepCache, 'store' | 'reuse'), got %r" % (deep,))
    return deep[0], deep[1]


# ---- FreeU (x_info['freeu']): backbone scaling and Fourier-filtered skips at the decoder's skip loads ----------------------------
# Si et al., "FreeU: Free Lunch in Diffusion U-Net" (CVPR 2024).  The setting is (b1, b2, s1, s2); a load whose entering h has the
# width W1 of the widest h that enters any output-stage block is stage 1 (b1, s1), the width W1 // 2 is stage 2 (b2, s2), any other
# load is untouched.  What a stage does to h and the popped skip: ops.freeu (contract in include/vd_hip.h).
_FREEU_KEYS = ("b1", "b2", "s1", "s2")


def freeu_entering_widths(model_channels, channel_mult, num_res_blocks):
    """The width of the h that enters each output-stage block (= each skip load, in walk order) of a UNetModel2D_Next with these
    arguments: the decoder starts at the middle block's width and every block leaves its level's width behind."""
    mult = list(channel_mult)
    nrb = [num_res_blocks] * len(mult) if isinstance(num_res_blocks, (int, np.integer)) else list(num_res_blocks)
    ch, widths = int(model_channels) * int(mult[-1]), []
    for level in reversed(range(len(mult))):
        for _ in range(int(nrb[level]) + 1):
            widths.append(ch)
            ch = int(model_channels) * int(mult[level])
    return widths


def freeu_stages(net):
    """(W1, W2, blocks1, blocks2) of FreeU on a 2-D data net (or on a dict of its arguments model_channels, channel_mult,
    num_res_blocks): the two stage widths and the output-block indices of either stage.  ValueError for a net without planes."""
    if isinstance(net, dict):
        args = net
    else:
        from .openaimodel import UNetModel0D_Next
        if isinstance(net, UNetModel0D_Next) or not all(hasattr(net, k) for k in ("model_channels", "channel_mult", "num_res_blocks")):
            raise ValueError("freeu needs a 2-D data net (x_info['type'] == 'image'), got %s" % type(net).__name__)
        args = {k: getattr(net, k) for k in ("model_channels", "channel_mult", "num_res_blocks")}
    widths = freeu_entering_widths(args["model_channels"], args["channel_mult"], args["num_res_blocks"])
    W1 = max(widths)
    W2 = W1 // 2
    return W1, W2, [i for i, w in enumerate(widths) if w == W1], [i for i, w in enumerate(widths) if w == W2]


def freeu_setting(value):
    """x_info['freeu'] as (b1, b2, s1, s2) floats, or None when it is absent, None or all ones (FreeU off: today's forward).
    Accepted: a sequence of four values in that order or a dict with exactly those four keys; every value a finite real number
    (no bool).  ValueError for anything else.  Touches no device."""
    if value is None:
        return None
    if isinstance(value, dict):
        if set(value.keys()) != set(_FREEU_KEYS):
            raise ValueError("x_info['freeu'] as a dict needs exactly the keys b1, b2, s1, s2, got %r" % (sorted(map(str, value.keys())),))
        vals = [value[k] for k in _FREEU_KEYS]
    elif isinstance(value, (tuple, list)) or (isinstance(value, np.ndarray) and value.ndim == 1):
        vals = list(value)
        if len(vals) != 4:
            raise ValueError("x_info['freeu'] must hold four values (b1, b2, s1, s2), got %d" % len(vals))
    else:
        raise ValueError("x_info['freeu'] must be None, a sequence (b1, b2, s1, s2) or a dict with those keys, got %r" % (value,))
    out = []
    for k, v in zip(_FREEU_KEYS, vals):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(float(v)):
            raise ValueError("x_info['freeu']: %s must be a finite real number, got %r" % (k, v))
        out.append(float(v))
    return None if all(v == 1.0 for v in out) else tuple(out)


def _freeu_arg(x_info):
    """x_info['freeu'] validated (freeu_setting) for the flow of x_info: None, or (b1, b2, s1, s2) on the 2-D image flow."""
    setting = freeu_setting(x_info.get("freeu"))
    if x_info.get("freeu") is not None and x_info.get("type") != "image":
        raise ValueError("freeu applies to x_info['type'] == 'image' only (the 0-D text flow has no planes), got %r"
                         % (x_info.get("type"),))
    return setting


# ---- perturbed-attention guidance (x_info['pag_scale'], x_info['pag_layers']; forward key x_info['pag']) -------------------------
# Ahn et al., "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance" (2024); diffusers' pag_scale and
# pag_applied_layers.  The samplers append one replica to the batch whose self-attention map is the identity in the chosen
# context blocks (run_unet(pag=...)) and fold its prediction into the step's eps (ops.pag_fold, contract in include/vd_hip.h).
def pag_context_blocks(net):
    """(n, mid): the number of context blocks in the walk i_order + m_order + o_order of a 2-D data net and the walk index of the
    middle stage's first one ("mid": 6 of the 16 at full width).  ValueError for a net without such a walk."""
    from .openaimodel import UNetModel0D_Next
    if isinstance(net, UNetModel0D_Next) or not all(hasattr(net, k) for k in ("i_order", "m_order", "o_order")):
        raise ValueError("pag needs a 2-D data net (x_info['type'] == 'image'), got %s" % type(net).__name__)
    i_order, m_order, o_order = list(net.i_order), list(net.m_order), list(net.o_order)
    n = sum(s == "c" for s in i_order + m_order + o_order)
    if "c" not in m_order:
        raise ValueError("pag: the middle stage of %s has no context block" % type(net).__name__)
    return n, sum(s == "c" for s in i_order)


def pag_layers(value, net):
    """x_info['pag_layers'] as a sorted tuple of context-block indices in walk order: "mid" (also for None, the default) is the
    middle stage's block; else an iterable of ints in [0, n).  ValueError (matching 'pag') for an empty list, duplicates, indices
    out of range or anything that is no int.  Touches no device."""
    n, mid = pag_context_blocks(net)
    if value is None or (isinstance(value, str) and value == "mid"):
        return (mid,)
    if isinstance(value, (str, bytes)) or not hasattr(value, "__iter__"):
        raise ValueError("x_info['pag_layers'] must be 'mid' or an iterable of context-block indices, got %r" % (value,))
    out = []
    for v in value:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < n:
            raise ValueError("x_info['pag_layers']: %r is no context-block index in [0, %d)" % (v, n))
        out.append(int(v))
    if not out:
        raise ValueError("x_info['pag_layers'] is empty: pag needs at least one context block")
    if len(set(out)) != len(out):
        raise ValueError("x_info['pag_layers'] names a context block twice: %r" % (out,))
    return tuple(sorted(out))


def _pag_arg(x_info, model):
    """The sampler keys of perturbed-attention guidance validated: None when x_info['pag_scale'] is absent, None or 0 (off: today's
    call, 'pag_layers' is then ignored), else (s_pag as a float, the normalised layers of pag_layers) on the 2-D image flow.
    ValueError (matching 'pag') for a scale that is no real number, negative or not finite, for another flow, and for the
    combinations left out of scope on purpose: cache_interval > 1 (DeepCache would keep the deep feature of three replicas and
    reuse a perturbed one) and region_masks (one perturbed replica per region).  Touches no device."""
    value = x_info.get("pag_scale")
    if value is None:
        return None
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) \
            or not np.isfinite(float(value)) or float(value) < 0.:
        raise ValueError("x_info['pag_scale'] must be a finite real number >= 0, got %r" % (value,))
    if float(value) == 0.:
        return None
    if x_info.get("type") != "image":
        raise ValueError("pag_scale applies to x_info['type'] == 'image' only (perturbed self-attention of the 2-D net), got %r"
                         % (x_info.get("type"),))
    cache = x_info.get("cache_interval", 1)
    if not isinstance(cache, (bool, str)) and isinstance(cache, (int, np.integer)) and cache > 1:
        raise ValueError("pag_scale with cache_interval > 1 is out of scope on purpose: DeepCache and pag do not combine")
    if x_info.get("region_masks") is not None:
        raise ValueError("pag_scale with region_masks is out of scope on purpose: regional prompts and pag do not combine")
    return float(value), pag_layers(x_info.get("pag_layers"), model.diffuser[x_info["type"]])


def _pag_fwd_arg(x_info, net):
    """x_info['pag'] (extension key of apply_model*, set by the samplers) validated: None, or (layers, row0) -- the rows >= row0
    of the batch, counted after replication, take identity self-attention in the context blocks `layers` (pag_layers) of `net`."""
    pag = x_info.get("pag")
    if pag is None:
        return None
    if x_info.get("type") != "image":
        raise ValueError("pag applies to x_info['type'] == 'image' only, got %r" % (x_info.get("type"),))
    if not (isinstance(pag, (tuple, list)) and len(pag) == 2):
        raise ValueError("x_info['pag'] must be (layers, row0), got %r" % (pag,))
    row0 = pag[1]
    if isinstance(row0, (bool, np.bool_)) or not isinstance(row0, (int, np.integer)) or row0 < 0:
        raise ValueError("x_info['pag']: row0 must be an int >= 0, got %r" % (row0,))
    return pag_layers(pag[0], net), int(row0)


# ---- smoothed energy guidance (x_info['seg_scale'], ['seg_blur_sigma'], ['seg_layers']; forward key x_info['seg']) ---------------
# Hong, "Smoothed Energy Guidance: Guiding Diffusion Models with Reduced Energy Curvature of Attention" (NeurIPS 2024); ComfyUI's SEG
# node and diffusers' SmoothedEnergyGuidance.  The perturbed replica of perturbed-attention guidance, with a milder perturbation: the
# chosen context blocks keep their softmax and Gaussian-blur the replica's queries over the token grid (run_unet(seg=...),
# ops.attention(blur_from=...), contract in include/vd_hip.h).  The samplers fold its prediction with ops.pag_fold, like pag's.
SEG_DEFAULT_SCALE = 3.0         # the upstream default of seg_scale (the key itself defaults to off)
SEG_MEAN_SIGMA = 9999.0         # from here on (the upstream rule), and at math.inf, every query becomes the sample's mean query


def seg_taps(sigma):
    """(R, taps) of x_info['seg_blur_sigma']: (-1, None) in mean mode (sigma >= 9999 or infinite); else ks = ceil(6 sigma), made odd by
    adding 1, R = (ks - 1) / 2 and taps = fp32 [2 R + 1], w[d] = exp(-0.5 (d / sigma)^2) normalised to sum 1 in float64 and rounded
    once.  ValueError (matching 'seg') for a sigma that is no real number, NaN, not > 0, or so small that R < 1."""
    if isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating)) or np.isnan(float(sigma)) \
            or not float(sigma) > 0.:
        raise ValueError("x_info['seg_blur_sigma'] (seg) must be a real number > 0 or math.inf, got %r" % (sigma,))
    sigma = float(sigma)
    if np.isinf(sigma) or sigma >= SEG_MEAN_SIGMA:
        return -1, None
    ks = int(np.ceil(6.0 * sigma))
    ks += 1 - ks % 2
    R = (ks - 1) // 2
    if R < 1:
        raise ValueError("x_info['seg_blur_sigma'] (seg) = %r leaves a single tap: ceil(6 sigma) must be >= 2" % (sigma,))
    w = np.exp(-0.5 * (np.arange(-R, R + 1, dtype=np.float64) / sigma) ** 2)
    return R, (w / w.sum()).astype(np.float32)


def seg_refl(i, n):
    """Reflection without repeating the edge (torch's 'reflect' padding), folded as often as needed (period 2 (n - 1)); 0 for n == 1."""
    if n == 1:
        return 0
    p = 2 * (n - 1)
    i %= p
    return i if i < n else p - i


def seg_grids(net, H0, W0):
    """[(H, W)] per context block of the 2-D data net `net` in walk order on an H0 x W0 latent: every Downsample halves a side,
    rounding up, the way up returns to the sizes of the way down."""
    from .openaimodel import Downsample, Upsample
    pag_context_blocks(net)
    d_iter = iter(net.data_blocks)
    sizes = [(int(H0), int(W0))]
    level, out = 0, []
    for s in list(net.i_order) + list(net.m_order) + list(net.o_order):
        if s == "d":
            blk = next(d_iter)
            if any(isinstance(m, Downsample) for m in blk.modules()):
                level += 1
                if level == len(sizes):
                    sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
            elif any(isinstance(m, Upsample) for m in blk.modules()):
                level -= 1
        elif s == "c":
            out.append(sizes[level])
    return out


def seg_workspace_elems(model, c_types, H0, W0, layers):
    """The fp16 elements one perturbed sample's blurred queries take at most in the context blocks `layers` (walk indices) of the
    image flow on an H0 x W0 latent (or window): max H W C over those blocks and the context types `c_types`."""
    grids = seg_grids(model.diffuser["image"], H0, W0)
    need = 0
    for ct in c_types:
        blocks = list(model.diffuser[ct].context_blocks)
        for ci in layers:
            st = blocks[ci]
            st = st[0] if isinstance(st, (nn.Sequential, list, tuple)) else st
            need = max(need, grids[ci][0] * grids[ci][1] * int(st.proj_in.out_channels))
    return need


def _seg_arg(x_info, model, shape=None):
    """The sampler keys of smoothed energy guidance validated: None when x_info['seg_scale'] is absent, None or 0 (off: today's call,
    the other keys are then ignored), else (s_seg as a float, the layers of x_info['seg_layers'] -- pag_layers' values and validator,
    default "mid" -- and sigma = x_info['seg_blur_sigma'], default math.inf) on the 2-D image flow; 3.0 is the upstream default of
    the scale.  ValueError (matching 'seg') for a scale that is no real number, negative or not finite, a bad sigma (seg_taps), bad
    layers, another flow, and for the combinations left out of scope on purpose: pag_scale or sag_scale (one replica-0 fold per
    step), tome_ratio (the token grid is gone), cache_interval > 1 and region_masks (as pag), and, when `shape` ([B, C, H, W]) is
    given, a chosen layer that HyperTile tiles.  Touches no device."""
    value = x_info.get("seg_scale")
    if value is None:
        return None
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) \
            or not np.isfinite(float(value)) or float(value) < 0.:
        raise ValueError("x_info['seg_scale'] must be a finite real number >= 0, got %r" % (value,))
    if float(value) == 0.:
        return None
    sigma = x_info.get("seg_blur_sigma")
    sigma = float("inf") if sigma is None else sigma
    seg_taps(sigma)
    if x_info.get("type") != "image":
        raise ValueError("seg_scale applies to x_info['type'] == 'image' only (blurred self-attention queries of the 2-D net), got %r"
                         % (x_info.get("type"),))
    if x_info.get("pag_scale") not in (None, 0, 0.) or x_info.get("pag") is not None:
        raise ValueError("seg_scale with pag_scale is out of scope on purpose: one replica-0 fold per step")
    if x_info.get("sag_scale") not in (None, 0, 0.) or x_info.get("sag") is not None:
        raise ValueError("seg_scale with sag_scale is out of scope on purpose: one replica-0 fold per step")
    if x_info.get("tome_ratio") not in (None, 0, 0.) or x_info.get("tome") is not None:
        raise ValueError("seg_scale with tome_ratio is out of scope on purpose: merged tokens have no grid to blur over")
    cache = x_info.get("cache_interval", 1)
    if not isinstance(cache, (bool, str)) and isinstance(cache, (int, np.integer)) and cache > 1:
        raise ValueError("seg_scale with cache_interval > 1 is out of scope on purpose: DeepCache and seg do not combine")
    if x_info.get("region_masks") is not None:
        raise ValueError("seg_scale with region_masks is out of scope on purpose: regional prompts and seg do not combine")
    net = model.diffuser[x_info["type"]]
    try:
        layers = pag_layers(x_info.get("seg_layers"), net)
    except ValueError as e:
        raise ValueError(str(e).replace("pag_layers", "seg_layers").replace("pag", "seg")) from None
    if shape is not None and x_info.get("hypertile") is not None:
        ht = _hypertile_arg(x_info, model, shape)
        if ht is not None:
            H, W = int(shape[2]), int(shape[3])
            if x_info.get("window") is not None:
                from . import windows
                h, w = windows.int_pair("window", x_info["window"])
                H, W = min(h, H), min(w, W)
            tiled = {b[0] for b in hypertile_blocks(net, H, W, ht)}
            if tiled & set(layers):
                raise ValueError("seg_layers %r: HyperTile tiles the context block(s) %r, whose queries seg would blur over the whole "
                                 "grid: lower hypertile_max_downsample or choose other layers" % (layers, sorted(tiled & set(layers))))
    return float(value), layers, float(sigma)


def _seg_fwd_arg(x_info, net, device):
    """x_info['seg'] (extension key of apply_model*, set by the samplers) validated: None, or (layers, row0, taps, R, qb) for
    run_unet -- x_info['seg'] = (layers, row0, sigma): the rows >= row0 of the batch, counted after replication, blur their
    self-attention queries with seg_taps(sigma) in the context blocks `layers` (pag_layers) of `net`.  x_info['seg_buffers'] =
    (taps, qb), when present (a captured step: nothing is uploaded or allocated then), are the device fp32 taps (None in mean mode)
    and the fp16 workspace [context types, perturbed rows, seg_workspace_elems]; else the taps are uploaded here."""
    seg = x_info.get("seg")
    if seg is None:
        return None
    if x_info.get("type") != "image":
        raise ValueError("seg applies to x_info['type'] == 'image' only, got %r" % (x_info.get("type"),))
    if not (isinstance(seg, (tuple, list)) and len(seg) == 3):
        raise ValueError("x_info['seg'] must be (layers, row0, sigma), got %r" % (seg,))
    if x_info.get("pag") is not None or x_info.get("sag") is not None or x_info.get("tome") is not None:
        raise ValueError("seg with pag, sag or tome in the same forward is out of scope on purpose")
    row0 = seg[1]
    if isinstance(row0, (bool, np.bool_)) or not isinstance(row0, (int, np.integer)) or row0 < 0:
        raise ValueError("x_info['seg']: row0 must be an int >= 0, got %r" % (row0,))
    try:
        layers = pag_layers(seg[0], net)
    except ValueError as e:
        raise ValueError(str(e).replace("pag_layers", "seg_layers").replace("pag", "seg")) from None
    R, taps = seg_taps(seg[2])
    bufs = x_info.get("seg_buffers")
    if bufs is not None:
        taps_dev, qb = bufs
    else:
        taps_dev, qb = (None if taps is None else torch.from_numpy(taps).to(device)), None
    return layers, int(row0), taps_dev, R, qb


# ---- token merging (x_info['tome_ratio'], x_info['tome_max_downsample']; forward key x_info['tome']) ---------------------------
# Bolya & Hoffman, "Token Merging for Fast Stable Diffusion" (2023); tomesd.apply_patch(model, ratio, max_downsample) with
# sx = sy = 2 and use_rand = False.  In the context blocks whose token grid is the latent grid (or, max_downsample = 2, half of it
# per side) the self-attention runs on N - r tokens: CrossAttention.forward(tome=...), contract in include/vd_hip.h.
class TokenMerge(object):
    """The setting of token merging: ratio, a real number in [0, 0.75] (0 = off), and max_downsample, 1 or 2.  ValueError (matching
    'tome') for anything else.  record: None, or a list that receives (walk index of the context block, row_of.clone()) from every
    merging block of every forward -- an eager-only test hook, a ValueError under graph capture."""

    def __init__(self, ratio, max_downsample=1):
        if isinstance(ratio, (bool, np.bool_)) or not isinstance(ratio, (int, float, np.integer, np.floating)) \
                or not np.isfinite(float(ratio)) or not 0. <= float(ratio) <= 0.75:
            raise ValueError("tome_ratio must be a real number in [0, 0.75], got %r" % (ratio,))
        if isinstance(max_downsample, (bool, np.bool_)) or not isinstance(max_downsample, (int, np.integer)) \
                or int(max_downsample) not in (1, 2):
            raise ValueError("tome_max_downsample must be 1 or 2, got %r" % (max_downsample,))
        self.ratio = float(ratio)
        self.max_downsample = int(max_downsample)
        self.record = None

    def key(self):
        return self.ratio, self.max_downsample

    def r(self, H, W):
        """How many of the H W tokens of a merging block are merged: min(int(N ratio), Ns), Ns = 3 N / 4."""
        N = int(H) * int(W)
        return min(int(N * self.ratio), N - N // 4)


def tome_blocks(net, H0, W0, tm):
    """[(walk index of the context block, H, W, r)] of the blocks of the 2-D data net `net` that merge under the TokenMerge `tm` on
    an H0 x W0 latent, in walk order (a block after k Downsamples has the grid H0 / 2^k x W0 / 2^k).  ValueError (matching
    'tome') for a net without such a walk and for a merging level whose grid is odd on a side."""
    from .openaimodel import Downsample, UNetModel0D_Next, Upsample
    if isinstance(net, UNetModel0D_Next) or not all(hasattr(net, k) for k in ("i_order", "m_order", "o_order", "data_blocks")):
        raise ValueError("tome needs a 2-D data net (x_info['type'] == 'image'), got %s" % type(net).__name__)
    d_iter = iter(net.data_blocks)
    level, ci, out = 0, 0, []
    for s in list(net.i_order) + list(net.m_order) + list(net.o_order):
        if s == "d":
            blk = next(d_iter)
            if any(isinstance(m, Downsample) for m in blk.modules()):
                level += 1
            elif any(isinstance(m, Upsample) for m in blk.modules()):
                level -= 1
        elif s == "c":
            if 2 ** level <= tm.max_downsample:
                f = 2 ** level
                if H0 % (2 * f) or W0 % (2 * f):
                    raise ValueError("tome: a %d x %d latent (or window) leaves the merging level %d with an odd token grid; both "
                                     "sides must be multiples of %d" % (H0, W0, level, 2 * f))
                H, W = H0 // f, W0 // f
                if tm.r(H, W) > 0:
                    out.append((ci, H, W, tm.r(H, W)))
            ci += 1
    return out


def _tome_arg(x_info, model, shape=None):
    """The sampler keys of token merging validated: None when x_info['tome_ratio'] is absent, None or 0 (off: today's call), else the
    TokenMerge(ratio, x_info.get('tome_max_downsample', 1)).  x_info['tome'] may hold a ready TokenMerge instead (the way to set its
    `record` hook on a sampler call).  ValueError (matching 'tome') for a bool, a non-number or a ratio outside [0, 0.75], a
    max_downsample other than 1 or 2, another flow than the 2-D image flow, perturbed-attention guidance in the same call (identity-map
    replicas are out of scope) and, when `shape` ([B, C, H, W]) is given, a latent -- or with x_info['window'] a window -- side that
    leaves a merging level with an odd grid.  Touches no device."""
    tm = x_info.get("tome")
    if tm is not None and not isinstance(tm, TokenMerge):
        raise ValueError("x_info['tome'] must be a TokenMerge, got %r" % (tm,))
    if tm is not None and x_info.get("tome_ratio") is not None:
        raise ValueError("x_info holds both 'tome' and 'tome_ratio': pass one")
    if tm is None:
        ratio = x_info.get("tome_ratio")
        if ratio is None:
            if x_info.get("tome_max_downsample") is not None:
                TokenMerge(0., x_info["tome_max_downsample"])
            return None
        tm = TokenMerge(ratio, x_info.get("tome_max_downsample", 1))
    if tm.ratio == 0.:
        return None
    if x_info.get("type") != "image":
        raise ValueError("tome_ratio applies to x_info['type'] == 'image' only (self-attention over a token grid), got %r"
                         % (x_info.get("type"),))
    if _pag_arg(x_info, model) is not None or x_info.get("pag") is not None:
        raise ValueError("tome_ratio with pag_scale is out of scope on purpose: token merging and identity-map replicas do not combine")
    if shape is not None:
        shape = tuple(int(s) for s in shape)
        if len(shape) != 4:
            raise ValueError("tome: the latent shape must be [B, C, H, W], got %s" % (shape,))
        H, W = shape[2:]
        if x_info.get("window") is not None:
            from . import windows
            h, w = windows.int_pair("window", x_info["window"])
            H, W = min(h, H), min(w, W)
        tome_blocks(model.diffuser[x_info["type"]], H, W, tm)
    return tm


def _tome_fwd_arg(x_info):
    """x_info['tome'] (extension key of apply_model*, set by the samplers) validated: None (absent, or ratio 0), or the TokenMerge."""
    tm = x_info.get("tome")
    if tm is None:
        return None
    if not isinstance(tm, TokenMerge):
        raise ValueError("x_info['tome'] must be a TokenMerge, got %r" % (tm,))
    if tm.ratio == 0.:
        return None
    if x_info.get("type") != "image":
        raise ValueError("tome applies to x_info['type'] == 'image' only, got %r" % (x_info.get("type"),))
    if x_info.get("pag") is not None:
        raise ValueError("tome with pag is out of scope on purpose: token merging and identity-map replicas do not combine")
    return tm


# ---- HyperTile (x_info['hypertile'], x_info['hypertile_max_downsample']; the forward key is x_info['hypertile'] too) -------------
# tfernd, "HyperTile: Tiled-optimizations for Stable-Diffusion" (2023; shipped in ComfyUI, A1111 and SD.Next) with scale_depth and a
# FIXED divisor: the original draws the divisor of a level at random per call, here the tile side is the same at every level and in
# every call, which keeps one step graph per setting and run-to-run identical bits.  In the context blocks after k Downsamples,
# 2^k <= max_downsample, the self-attention runs inside square tiles of the token grid: CrossAttention.forward(tile=...), contract in
# include/vd_hip.h.  An approximation like token merging and DeepCache, meant for canvases larger than the trained size.
class HyperTile(object):
    """The setting of HyperTile: tile, the side of a square tile in tokens (an int >= 2, the same at every level), and
    max_downsample, 1, 2 or 4.  ValueError (matching 'hypertile') for anything else."""

    def __init__(self, tile, max_downsample=1):
        if isinstance(tile, (bool, np.bool_)) or not isinstance(tile, (int, np.integer)) or int(tile) < 2:
            raise ValueError("hypertile must be an int >= 2 (the tile side in tokens), got %r" % (tile,))
        if isinstance(max_downsample, (bool, np.bool_)) or not isinstance(max_downsample, (int, np.integer)) \
                or int(max_downsample) not in (1, 2, 4):
            raise ValueError("hypertile_max_downsample must be 1, 2 or 4, got %r" % (max_downsample,))
        self.tile = int(tile)
        self.max_downsample = int(max_downsample)

    def key(self):
        return self.tile, self.max_downsample


def hypertile_blocks(net, H0, W0, ht):
    """[(walk index of the context block, H, W, nty, ntx)] of the blocks of the 2-D data net `net` whose self-attention is tiled
    under the HyperTile `ht` on an H0 x W0 latent, in walk order.  A block after k Downsamples, 2^k <= ht.max_downsample, has the
    grid H0 / 2^k x W0 / 2^k (every Downsample halves a side, rounding up); a grid that fits in one tile (H, W <= tile) is absent:
    that block runs the untiled path.  ValueError (matching 'hypertile') for a net without such a walk and for a grid larger than
    one tile with a side that is not a multiple of the tile."""
    from .openaimodel import Downsample, UNetModel0D_Next, Upsample
    if isinstance(net, UNetModel0D_Next) or not all(hasattr(net, k) for k in ("i_order", "m_order", "o_order", "data_blocks")):
        raise ValueError("hypertile needs a 2-D data net (x_info['type'] == 'image'), got %s" % type(net).__name__)
    d_iter = iter(net.data_blocks)
    sizes = [(int(H0), int(W0))]        # the grid per level, as the way down produced it
    level, ci, out = 0, 0, []
    for s in list(net.i_order) + list(net.m_order) + list(net.o_order):
        if s == "d":
            blk = next(d_iter)
            if any(isinstance(m, Downsample) for m in blk.modules()):
                level += 1
                if level == len(sizes):
                    sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
            elif any(isinstance(m, Upsample) for m in blk.modules()):
                level -= 1
        elif s == "c":
            H, W = sizes[level]
            if 2 ** level <= ht.max_downsample and (H > ht.tile or W > ht.tile):
                if H % ht.tile or W % ht.tile:
                    raise ValueError("hypertile: the tile side %d does not divide the %d x %d token grid of level %d of a %d x %d "
                                     "latent (or window)" % (ht.tile, H, W, level, H0, W0))
                out.append((ci, H, W, H // ht.tile, W // ht.tile))
            ci += 1
    return out


def _hypertile_arg(x_info, model, shape=None):
    """The sampler keys of HyperTile validated: None when x_info['hypertile'] is absent, None or 0 (off: today's call), else the
    HyperTile(x_info['hypertile'], x_info.get('hypertile_max_downsample', 1)); a ready HyperTile is taken as it is.  ValueError
    (matching 'hypertile') for a bool, a non-int or a side < 2, a max_downsample other than 1, 2 or 4, another flow than the 2-D image
    flow, tome_ratio in the same call and, when `shape` ([B, C, H, W]) is given, a latent -- or with x_info['window'] a window --
    with a tiled level the tile does not divide, and self-attention guidance whose map block would be tiled.  Perturbed-attention
    guidance combines: a perturbed layer that is also tiled keeps its identity rows.  Touches no device."""
    value = x_info.get("hypertile")
    md = x_info.get("hypertile_max_downsample")
    if isinstance(value, HyperTile):
        if md is not None and md != value.max_downsample:
            raise ValueError("x_info holds a ready HyperTile in 'hypertile' and another 'hypertile_max_downsample': pass one")
        ht = value
    else:
        if value is None or (not isinstance(value, (bool, np.bool_)) and isinstance(value, (int, np.integer)) and int(value) == 0):
            if md is not None:
                HyperTile(2, md)
            return None
        ht = HyperTile(value, 1 if md is None else md)
    if x_info.get("type") != "image":
        raise ValueError("hypertile applies to x_info['type'] == 'image' only (self-attention over a token grid), got %r"
                         % (x_info.get("type"),))
    if x_info.get("tome_ratio") not in (None, 0, 0.) or x_info.get("tome") is not None:
        raise ValueError("hypertile with tome_ratio is out of scope on purpose: one plan per self-attention")
    if shape is not None:
        shape = tuple(int(s) for s in shape)
        if len(shape) != 4:
            raise ValueError("hypertile: the latent shape must be [B, C, H, W], got %s" % (shape,))
        H, W = shape[2:]
        if x_info.get("window") is not None:
            from . import windows
            h, w = windows.int_pair("window", x_info["window"])
            H, W = min(h, H), min(w, W)
        net = model.diffuser[x_info["type"]]
        blocks = hypertile_blocks(net, H, W, ht)
        if x_info.get("sag_scale") not in (None, 0, 0.) and pag_context_blocks(net)[1] in [b[0] for b in blocks]:
            raise ValueError("hypertile would tile the block self-attention guidance reads its map from (sag_scale): lower "
                             "hypertile_max_downsample or raise the tile side")
    return ht


def _hypertile_fwd_arg(x_info):
    """x_info['hypertile'] as apply_model* sees it (set by the samplers) validated: None (absent, None or 0), or the HyperTile -- an
    int side is taken with x_info.get('hypertile_max_downsample', 1), like the sampler key."""
    value = x_info.get("hypertile")
    if value is None:
        return None
    if not isinstance(value, HyperTile):
        if not isinstance(value, (bool, np.bool_)) and isinstance(value, (int, np.integer)) and int(value) == 0:
            return None
        md = x_info.get("hypertile_max_downsample")
        value = HyperTile(value, 1 if md is None else md)
    if x_info.get("type") != "image":
        raise ValueError("hypertile applies to x_info['type'] == 'image' only, got %r" % (x_info.get("type"),))
    if x_info.get("tome") is not None:
        raise ValueError("hypertile with tome is out of scope on purpose: one plan per self-attention")
    return value


# ---- self-attention guidance (x_info['sag_scale'], x_info['sag_blur_sigma']; forward key x_info['sag']) ------------------------
# Hong et al., "Improving Sample Quality of Diffusion Models Using Self-Attention Guidance" (ICCV 2023); diffusers'
# StableDiffusionSAGPipeline(sag_scale).  A forward with x_info['sag'] also writes the column mass of the middle context block's
# self-attention map of replica 0 (ops.sag_mass); the samplers degrade the latent with it (ops.sag_degrade), predict a second time
# and fold that prediction into the step's eps (ops.sag_fold; contracts in include/vd_hip.h).
SAG_MAX_TOKENS = 1024


def sag_map_size(net, H, W):
    """(Hm, Wm): the token grid of the middle stage's first context block of the 2-D data net `net` on an H x W latent -- the block
    pag_layers names "mid"; every Downsample in front of it halves a side, rounding up.  ValueError (matching 'sag') for a net
    without such a walk."""
    from .openaimodel import Downsample, UNetModel0D_Next, Upsample
    if isinstance(net, UNetModel0D_Next) or not all(hasattr(net, k) for k in ("i_order", "m_order", "o_order", "data_blocks")):
        raise ValueError("sag needs a 2-D data net (x_info['type'] == 'image'), got %s" % type(net).__name__)
    if "c" not in list(net.m_order):
        raise ValueError("sag: the middle stage of %s has no context block" % type(net).__name__)
    d_iter = iter(net.data_blocks)
    Hm, Wm = int(H), int(W)
    for i, s in enumerate(list(net.i_order) + list(net.m_order)):
        if s == "d":
            blk = next(d_iter)
            if any(isinstance(m, Downsample) for m in blk.modules()):
                Hm, Wm = (Hm + 1) // 2, (Wm + 1) // 2
            elif any(isinstance(m, Upsample) for m in blk.modules()):
                Hm, Wm = Hm * 2, Wm * 2
        elif s == "c" and i >= len(net.i_order):
            break
    return Hm, Wm


def sag_taps(sigma):
    """float64 [9]: g[k] = exp(-((k - 4) / sigma)^2 / 2) / sum, the normalised Gaussian of diffusers' gaussian_blur_2d at kernel
    size 9."""
    g = np.exp(-0.5 * ((np.arange(9, dtype=np.float64) - 4.0) / float(sigma)) ** 2)
    return g / g.sum()


def _sag_real(value):
    return not isinstance(value, (bool, np.bool_)) and isinstance(value, (int, float, np.integer, np.floating)) and np.isfinite(float(value))


def _sag_arg(x_info, model, shape=None):
    """The sampler keys of self-attention guidance validated: None when x_info['sag_scale'] is absent, None or 0 (off: today's call,
    'sag_blur_sigma' is then ignored), else (s_sag, sigma) as floats, sigma = x_info['sag_blur_sigma'] (default 1.0) on the 2-D
    image flow.  ValueError (matching 'sag') for a scale that is no real number, negative or not finite, a sigma that is no finite
    real number > 0, another flow, with `shape` ([B, C, H, W]) a latent side below 5 (the reflected 9-tap blur) or a middle token
    grid of more than 1024 tokens, and for the combinations left out of scope on purpose: window / region_masks, cache_interval > 1,
    pag_scale and tome_ratio.  Touches no device."""
    value = x_info.get("sag_scale")
    if value is None:
        return None
    if not _sag_real(value) or float(value) < 0.:
        raise ValueError("x_info['sag_scale'] must be a finite real number >= 0, got %r" % (value,))
    if float(value) == 0.:
        return None
    sigma = x_info.get("sag_blur_sigma", 1.0)
    if not _sag_real(sigma) or not float(sigma) > 0.:
        raise ValueError("x_info['sag_blur_sigma'] (sag) must be a finite real number > 0, got %r" % (sigma,))
    if x_info.get("type") != "image":
        raise ValueError("sag_scale applies to x_info['type'] == 'image' only (the self-attention map of the 2-D net), got %r"
                         % (x_info.get("type"),))
    if x_info.get("window") is not None or x_info.get("region_masks") is not None:
        raise ValueError("sag_scale with window / region_masks is out of scope on purpose: one attention map per window")
    cache = x_info.get("cache_interval", 1)
    if not isinstance(cache, (bool, str)) and isinstance(cache, (int, np.integer)) and cache > 1:
        raise ValueError("sag_scale with cache_interval > 1 is out of scope on purpose: DeepCache and sag do not combine")
    if x_info.get("pag_scale") not in (None, 0, 0.) or x_info.get("pag") is not None:
        raise ValueError("sag_scale with pag_scale is out of scope on purpose: one replica-0 fold per step")
    if x_info.get("tome_ratio") not in (None, 0, 0.) or x_info.get("tome") is not None:
        raise ValueError("sag_scale with tome_ratio is out of scope on purpose: the mass is taken on the unmerged token grid")
    net = model.diffuser[x_info["type"]]
    if shape is not None:
        shape = tuple(int(s) for s in shape)
        if len(shape) != 4:
            raise ValueError("sag: the latent shape must be [B, C, H, W], got %s" % (shape,))
        if shape[2] < 5 or shape[3] < 5:
            raise ValueError("sag: the latent is %d x %d, the reflected 9-tap blur needs H, W >= 5" % shape[2:])
        Hm, Wm = sag_map_size(net, shape[2], shape[3])
        if Hm * Wm > SAG_MAX_TOKENS:
            raise ValueError("sag: the middle block has %d x %d tokens, at most %d" % (Hm, Wm, SAG_MAX_TOKENS))
    else:
        sag_map_size(net, 8, 8)
    return float(value), float(sigma)


# ---- adaptive projected guidance (x_info['apg_eta'], ['apg_norm_threshold'], ['apg_momentum']) -----------------------------------
# Sadat, Hilliges, Weber, "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion Models" (2024); diffusers'
# AdaptiveProjectedGuidance.  Nothing in the forward: the samplers fold it into the step's prediction (ddim.apg_guided_eps).
APG_NEUTRAL = (1.0, 0.0, 0.0)       # eta, norm threshold, momentum: plain classifier-free guidance


def _apg_arg(x_info):
    """The sampler keys of adaptive projected guidance validated: None when none of x_info['apg_eta'] (default 1),
    ['apg_norm_threshold'] (default 0 = no clipping) and ['apg_momentum'] (default 0) is present (a key that is None counts as
    absent) or when the triple is the neutral (1, 0, 0) (off: today's call), else (eta, r, beta) as floats.  ValueError (matching
    'apg') for an eta that is no real number in [0, 1], a threshold that is no finite real number >= 0, a momentum that is no finite
    real number with |beta| < 1 (a bool or a string is no real number), and for the combination left out of scope on purpose:
    sag_scale, whose fold reads replica 0 as the first forward's e_u, which this fold has rewritten.  Touches no device."""
    raw = [x_info.get(k) for k in ("apg_eta", "apg_norm_threshold", "apg_momentum")]
    if all(v is None for v in raw):
        return None
    real = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(float(v))
    eta, r, beta = [d if v is None else v for v, d in zip(raw, APG_NEUTRAL)]
    if not real(eta) or not 0. <= float(eta) <= 1.:
        raise ValueError("x_info['apg_eta'] must be a real number in [0, 1], got %r" % (eta,))
    if not real(r) or float(r) < 0.:
        raise ValueError("x_info['apg_norm_threshold'] must be a finite real number >= 0, got %r" % (r,))
    if not real(beta) or not abs(float(beta)) < 1.:
        raise ValueError("x_info['apg_momentum'] must be a finite real number with |beta| < 1, got %r" % (beta,))
    out = (float(eta), float(r), float(beta))
    if out == APG_NEUTRAL:
        return None
    if x_info.get("sag_scale") not in (None, 0, 0.):
        raise ValueError("apg with sag_scale is out of scope on purpose: the fold of self-attention guidance reads replica 0 as the "
                         "first forward's e_u, which the apg fold has rewritten")
    return out


def _sag_fwd_arg(x_info, contexts):
    """x_info['sag'] (extension key of apply_model*, set by the samplers) validated: None, or the caller-owned fp32 [T, B, Nm] device
    tensor -- T the number of context types of the call, B the samples of ONE replica, Nm the tokens of the middle context block."""
    buf = x_info.get("sag")
    if buf is None:
        return None
    if x_info.get("type") != "image":
        raise ValueError("sag applies to x_info['type'] == 'image' only, got %r" % (x_info.get("type"),))
    if not (torch.is_tensor(buf) and buf.dtype == torch.float32 and buf.dim() == 3 and buf.is_contiguous()
            and buf.shape[0] == contexts and buf.shape[1] == x_info["x"].shape[0]):
        raise ValueError("x_info['sag'] must be a contiguous fp32 [%d, %d, Nm] tensor, got %r"
                         % (contexts, x_info["x"].shape[0], tuple(buf.shape) if torch.is_tensor(buf) else buf))
    if buf.device != x_info["x"].device:
        raise ValueError("x_info['sag'] lives on %s, the latent on %s" % (buf.device, x_info["x"].device))
    return buf


def kv_rows(cache, rows):
    """A context K/V cache for forwards on the first `rows` samples of the batch `cache` was filled for: the same entries as
    batch-slice views, projected by the forward that filled `cache` (nothing is projected again).  None without a cache; an entry
    still marked stale is left out (it would be projected from the sliced context on use)."""
    if cache is None:
        return None
    stale = cache.get(_KV_STALE, ())
    out = {mid: kv[:rows] for mid, kv in cache.items() if not isinstance(mid, str) and mid not in stale}
    out[_KV_MODULES] = {mid: m for mid, m in cache.get(_KV_MODULES, {}).items() if mid in out}
    return out


def run_unet(data_net, ctx_specs, x, emb_silu, mixing_type="attention", repeat=1, emb_rows=None, deep=None, freeu=None, pag=None,
             tome=None, sag=None, hypertile=None, seg=None):
    """Walk i/m/o orders of `data_net` (reference vd.py:352-378 / 429-453).

    ctx_specs: list of (context_blocks, context [B, L, Dc], ratio, kv_cache or None), one per context type.
    x: NCHW latent; returns NCHW eps in fp16.
    repeat > 1: the batch the reference would feed is `x` replicated `repeat` times ([x; x] of classifier-free guidance,
    ddim.py:144-149) with identical timesteps per replica, while contexts / emb carry the full repeat * B rows.  The data
    blocks in front of the first context block see identical inputs in every replica, so they run once on B rows and the
    result (and the skip tensors saved so far) is replicated where the contexts make the replicas diverge.  With one context
    type that is INSIDE the first context block, behind its self-attention (CFG_HEAD_SHARE): the block takes h un-replicated and
    returns all repeat * B samples; with several types h is replicated in front of the block.
    emb_rows: {data block index: [Cout] fp16} complete first-conv bias vectors of the ResBlocks for the ONE timestep the whole
    batch shares (VD_v2_0.precompute_step_emb); emb_silu may then be None.
    deep: None, or (DeepCache, "store" | "reuse") with (a, b) = deep_cut(data_net, cache.depth).  "store": steps[0:b], a side
    copy of h into the cache, steps[b:] -- the eps of the plain forward, bit for bit.  "reuse": steps[0:a] for its skips (its h
    is dropped), h = the kept feature, steps[b:].
    freeu: None, or (b1, b2, s1, s2) of freeu_setting: every skip load of a stage whose (b, s) is not (1, 1) hands h and the popped
    skip to ops.freeu and goes on with its two fresh tensors (freeu_stages gives the widths).  In a cached walk the kept feature
    stays the tensor in front of the load; the stage is applied each time a walk consumes it.
    pag: None, or (layers, row0) of _pag_fwd_arg: in the context blocks whose walk index is in `layers` the rows >= row0 of the batch
    (after replication; every context type's block at that index) run their self-attention with the identity map
    (SpatialTransformer.forward(ident_from=...)); a half-batch branch holding samples [b0, b1) gets clamp(row0 - b0, 0, b1 - b0).
    A forward with pag replicates h IN FRONT of the first context block (share = 1): the shared CFG head is not used, whichever
    layers are named, so block 0 can be a perturbed layer and a perturbed replica never reads a shared self-attention.  It does
    not combine with deep (ValueError).
    tome: None, or a TokenMerge with ratio > 0: the context blocks of tome_blocks (every context type's block at those walk
    indices) merge r tokens in their self-attention (SpatialTransformer.forward(tome=(r, sink))); with its `record` set every such
    block appends (walk index, row_of.clone()) -- not under graph capture (ValueError).  It does not combine with pag (ValueError).
    sag: None, or the fp32 [T, B, Nm] buffer of _sag_fwd_arg (T context types, B = x.shape[0], the rows of one replica): the middle
    stage's first context block (sag_map_size's; pag_layers' "mid") writes the column mass of its self-attention map, ops.sag_mass,
    for the rows [0, B) of the batch -- replica 0 -- type t's module into sag[t], on the stream that module runs on (the joins of the
    forked branches order the writes before the next launch on the caller's stream); a half-batch branch holding samples [b0, b1)
    writes the rows [b0, min(b1, B)).  Nothing else changes: the eps bits are those of the forward without it.  It does not combine
    with tome or deep (ValueError).
    hypertile: None, or a HyperTile: the context blocks of hypertile_blocks (every context type's block at those walk indices) run
    their self-attention inside square tiles of their token grid (SpatialTransformer.forward(tile=(side, side))), the block that
    takes a guided batch un-replicated too.  Every other block, and a forward without it, keeps today's launches and bits.  It
    combines with pag (a perturbed layer that is tiled keeps its identity rows), deep and freeu; not with tome, nor with a sag whose
    map block is tiled (ValueError).
    seg: None, or (layers, row0, taps, R, qb) of _seg_fwd_arg: pag's walk with another perturbation -- in the context blocks whose
    walk index is in `layers` the rows >= row0 blur their self-attention queries over the block's token grid
    (SpatialTransformer.forward(blur_from=..., blur=(taps, R[, qb]))), a half-batch branch gets the clamped index, h is replicated in
    front of the first context block.  qb: None (every call allocates its workspace), or fp16 [context types, perturbed rows, *]:
    type t's module writes the blurred queries of the perturbed rows [p0, p1) it holds into qb[t, p0:p1], so forked branches and
    forked context types never share a byte.  It does not combine with pag, tome, sag, deep or a tiled chosen layer (ValueError)."""
    if seg is not None:
        if x.dim() != 4:
            raise ValueError("seg needs a 2-D data net (x_info['type'] == 'image')")
        if pag is not None or tome is not None or sag is not None or deep is not None:
            raise ValueError("seg does not combine with pag, tome, sag or deep_cache")
        if not 0 <= seg[1] <= repeat * x.shape[0]:
            raise ValueError("seg: row0 = %d is outside the batch of %d x %d rows" % (seg[1], repeat, x.shape[0]))
        if seg[4] is not None and (seg[4].dim() != 3 or seg[4].shape[0] < len(ctx_specs) or seg[4].shape[1] < repeat * x.shape[0] - seg[1]):
            raise ValueError("seg: the workspace %s is not [>= %d context types, >= %d perturbed rows, *]"
                             % (tuple(seg[4].shape), len(ctx_specs), repeat * x.shape[0] - seg[1]))
    hmap = None
    if hypertile is not None:
        if x.dim() != 4:
            raise ValueError("hypertile needs a 2-D data net (x_info['type'] == 'image')")
        if tome is not None:
            raise ValueError("hypertile does not combine with tome")
        hmap = {b[0] for b in hypertile_blocks(data_net, x.shape[-2], x.shape[-1], hypertile)}
        if sag is not None and pag_context_blocks(data_net)[1] in hmap:
            raise ValueError("hypertile would tile the block sag reads its map from")
        if seg is not None and hmap & set(seg[0]):
            raise ValueError("seg: hypertile tiles the chosen context block(s) %r" % (sorted(hmap & set(seg[0])),))
        hmap = (hmap, (hypertile.tile, hypertile.tile)) if hmap else None
    smap = None
    if sag is not None:
        if x.dim() != 4:
            raise ValueError("sag needs a 2-D data net (x_info['type'] == 'image')")
        if tome is not None or deep is not None:
            raise ValueError("sag does not combine with tome or deep_cache")
        if mixing_type != "attention":
            raise ValueError("sag needs mixing_type 'attention' (one mass per context type)")
        Hm, Wm = sag_map_size(data_net, x.shape[-2], x.shape[-1])
        if sag.shape[0] != len(ctx_specs) or sag.shape[1] != x.shape[0] or sag.shape[2] != Hm * Wm:
            raise ValueError("sag: the mass buffer %s is not [%d, %d, %d x %d]" % (tuple(sag.shape), len(ctx_specs), x.shape[0], Hm, Wm))
        smap = (pag_context_blocks(data_net)[1], sag)
    tmap = None
    if tome is not None:
        if x.dim() != 4:
            raise ValueError("tome needs a 2-D data net (x_info['type'] == 'image')")
        if pag is not None:
            raise ValueError("tome does not combine with pag")
        if tome.record is not None and x.is_cuda and torch.cuda.is_current_stream_capturing():
            raise ValueError("tome: TokenMerge.record is an eager-only hook, this forward is being captured into a graph")
        tmap = {ci: r for ci, _, _, r in tome_blocks(data_net, x.shape[-2], x.shape[-1], tome)}
        tmap = (tmap, tome.record) if tmap else None
    if pag is not None:
        if x.dim() != 4:
            raise ValueError("pag needs a 2-D data net (x_info['type'] == 'image')")
        if deep is not None:
            raise ValueError("pag does not combine with deep_cache")
        if not 0 <= pag[1] <= repeat * x.shape[0]:
            raise ValueError("pag: row0 = %d is outside the batch of %d x %d rows" % (pag[1], repeat, x.shape[0]))
    cut = None
    fmap = None
    if freeu is not None:
        if x.dim() != 4:
            raise ValueError("freeu needs a 2-D data net (x_info['type'] == 'image')")
        W1, W2 = freeu_stages(data_net)[:2]
        fmap = {w: bs for w, bs in ((W1, (freeu[0], freeu[2])), (W2, (freeu[1], freeu[3]))) if bs != (1.0, 1.0)}
    if deep is not None:
        if x.dim() != 4:
            raise ValueError("deep_cache needs a 2-D data net (x_info['type'] == 'image')")
        cut = deep_cut(data_net, deep[0].depth)
    d_iter = iter(enumerate(data_net.data_blocks))
    if emb_rows is not None:
        emb_outs = {}
    else:
        emb_rows = {}
        emb_outs = data_net.precompute_emb(emb_silu) if hasattr(data_net, "precompute_emb") else {}
    c_iters = [iter(spec[0]) for spec in ctx_specs]
    ratios = np.array([float(spec[2]) for spec in ctx_specs], dtype=np.float64)
    ratios = ratios / ratios.sum()

    # the walk, resolved to modules once: ("d", index, block) / ("c", modules, specs, ratios) / ("save",) / ("load",)
    steps = []
    c_index = 0
    for ltype in list(data_net.i_order) + list(data_net.m_order) + list(data_net.o_order):
        if ltype == "d":
            di, blk = next(d_iter)
            steps.append(("d", di, blk))
        elif ltype == "c":
            modules = [next(it) for it in c_iters]
            if mixing_type == "layer":
                pick = int(npr.choice(len(modules), p=ratios))
                steps.append(("c", [modules[pick]], [ctx_specs[pick]], [1.0], c_index))
            else:
                steps.append(("c", modules, list(ctx_specs), ratios, c_index))
            c_index += 1
        elif ltype == "save_hidden_feature":
            steps.append(("save",))
        elif ltype == "load_hidden_feature":
            steps.append(("load",))

    def context_kv(module, spec):
        return kv_lookup(spec[3], module, spec[1])

    def run_context(h, modules, specs, rs, sl=None, repeat=1, ident_from=None, tome=None, sag=None, tile=None, blur=None):
        """sl = (b0, b1): h holds samples b0 .. b1 - 1 of the batch (a half-batch branch): contexts and K/V are sliced alike.
        repeat > 1 (one context type, whole batch): h holds one replica, the block returns all of them.
        ident_from: None, or the first row of h that takes identity self-attention in these blocks (pag).
        tome: None, or (r, sink) of token merging for these blocks' self-attention.
        sag: None, or the mass buffer [T, B, Nm] of self-attention guidance: module t writes the rows of replica 0 that h holds.
        tile: None, or (th, tw) of HyperTile for these blocks' self-attention.
        blur: None, or (blur_from, p0, taps, R, qb) of smoothed energy guidance: the rows of h from blur_from on blur their queries in
        these blocks; they are the perturbed rows p0 ... of the batch, and module t's workspace is qb[t, p0:p0 + their count]."""
        single = len(modules) == 1
        pkw = {} if ident_from is None else {"ident_from": int(ident_from)}
        if tome is not None:
            pkw["tome"] = tome
        if tile is not None:
            pkw["tile"] = tile
        skw = [{} for _ in modules]
        if blur is not None:
            assert repeat == 1
            bf, p0, taps, R, qb = blur
            cnt = h.shape[0] - bf
            skw = [{"blur_from": int(bf), "blur": (taps, R) + (() if qb is None or cnt <= 0 else (qb[t, p0:p0 + cnt].reshape(-1),))}
                   for t in range(len(modules))]
        if sag is not None:
            lo, hi = (0, sag.shape[1]) if sl is None else (sl[0], min(sl[1], sag.shape[1]))
            if hi > lo:
                skw = [{"sag": sag[t, lo:hi]} for t in range(len(modules))]
        if repeat > 1:
            assert single and sl is None and ident_from is None
            return modules[0](h, None, specs[0][1], kv=context_kv(modules[0], specs[0]), alpha=1.0, res=None, repeat=repeat, **pkw,
                              **skw[0])
        kvs = [context_kv(m, sp) for m, sp in zip(modules, specs)]
        if sl is not None:
            kvs = [None if kv is None else kv[sl[0]:sl[1]] for kv in kvs]
            specs = [(sp[0], None if sp[1] is None else sp[1][sl[0]:sl[1]]) + tuple(sp[2:]) for sp in specs]
        # h_out = sum_i r_i * ST_i(h) = sum_i r_i * proj_i + h   (sum r_i = 1): chained through the epilogue of each type's LAST
        # launch (alpha = r_i, res = the previous type's output).  Everything in front of that launch depends on h only, so the
        # types run as forked branches (side streams; inside the sampler's HIP graph: parallel branches): at the per-GPU batch of
        # the multi-context workloads one type's launches fill half the chip.  Only the last launches are ordered, by events.
        if single or not CTX_FORK or not h.is_cuda:
            out = None
            for module, spec, kv, r, sk in zip(modules, specs, kvs, rs, skw):
                out = module(h, None, spec[1], kv=kv, alpha=1.0 if single else float(r), res=out, **pkw, **sk)
            return out
        main = torch.cuda.current_stream()
        sides = _side_streams(h.device, len(modules) - 1)
        order = _BranchOrder(main)
        outs, done = [], []
        for i, (module, spec, kv, r) in enumerate(zip(modules, specs, kvs, rs)):
            st = main if i == 0 else sides[i - 1]
            prev = outs[-1] if outs else None
            prev_done = done[-1] if done else None
            with torch.cuda.stream(st):
                tok = order.enter(st, first=i == 0)
                out = module(h, None, spec[1], kv=kv, alpha=float(r), res=prev,
                             sync=(None if prev_done is None else (lambda e=prev_done, s_=st: s_.wait_event(e))), **pkw, **skw[i])
                ev = torch.cuda.Event()
                ev.record(st)
                order.leave(st, tok)
            if i > 0:
                out.record_stream(main)
                st_ = getattr(out, "_vd_stats", None)   # ChanStats of the block output, written by the branch's last launch
                if st_ is not None and torch.is_tensor(getattr(st_, "buf", None)):
                    st_.buf.record_stream(main)
            outs.append(out)
            done.append(ev)
        main.wait_event(done[-1])
        for ev in done[1:-1]:
            main.wait_event(ev)
        return outs[-1]

    h = x
    nb = x.shape[0]
    shared = repeat > 1
    # LayerNorm row statistics accumulated by producer epilogues live in one arena per forward, zeroed by ONE fill
    # (the arena object is per CALL -- two threads running forwards of one net must not hand out overlapping slices -- the module
    # remembers only how many rows the previous forward took)
    # (a shallow forward takes less than a full one and the two alternate: one remembered value per kind of forward)
    need_key = "_vd_rowsum_need" if deep is None or deep[1] == "store" else "_vd_rowsum_need_reuse%d" % deep[0].depth
    # (so do the two forwards of a self-attention-guidance step, all replicas and one: the batch the net saw first keeps the plain
    # key, any other number of rows remembers its own value)
    if repeat * nb != data_net.__dict__.setdefault("_vd_rowsum_rows", repeat * nb):
        need_key += "_rows%d" % (repeat * nb)
    arena = ops.RowSumArena(data_net.__dict__.get(need_key, 0))
    arena.begin(x.device)
    try:
        return _run_unet_body(steps, emb_outs, emb_rows, emb_silu, run_context, lambda ms, sps: [context_kv(m, sp) for m, sp in zip(ms, sps)],
                              h, nb, shared, repeat, None if deep is None else (deep[0], deep[1], cut, (id(data_net), deep[0].depth)),
                              fmap or None, pag, tmap, smap, hmap, seg)
    finally:
        arena.end()
        data_net.__dict__[need_key] = arena.need


def _shares_cfg_head(module):
    """Whether the context block `module` can take a guided batch un-replicated: its consumers behind the self-attention are the
    kernels with a batch period (width 320: vd_xattn_rep_f16 and vd_ff_chain_f16).  Every other block gets the replicas in front."""
    st = module[0] if isinstance(module, (nn.Sequential, list, tuple)) else module
    return bool(getattr(st, "shares_cfg_head", lambda: False)())


def _fork_region(steps, hw0, thr):
    """[a, b) of `steps`: from the Downsample that brings the rows per sample to <= thr up to (not including) the Upsample that
    leaves that range again, or None.  The region must keep its skip tensors to itself (as many loads as saves, never below)."""
    from .openaimodel import Downsample, Upsample
    hw, a, b = hw0, None, None
    for i, st in enumerate(steps):
        if st[0] != "d":
            continue
        layers = list(st[2]) if isinstance(st[2], (nn.Sequential, list, tuple)) else [st[2]]
        if any(isinstance(l, Downsample) for l in layers):
            hw //= 4
            if a is None and hw <= thr:
                a = i
        elif any(isinstance(l, Upsample) for l in layers):
            if a is not None and b is None and hw <= thr and hw * 4 > thr:
                b = i
            hw *= 4
    if a is None or b is None or b <= a:
        return None
    depth = 0
    for st in steps[a:b]:
        depth += 1 if st[0] == "save" else (-1 if st[0] == "load" else 0)
        if depth < 0:
            return None
    return (a, b) if depth == 0 and any(st[0] == "c" for st in steps[a:b]) else None


def _run_unet_body(steps, emb_outs, emb_rows, emb_silu, run_context, prepare_context, h, nb, shared, repeat, deep=None, fmap=None,
                   pag=None, tome=None, sag=None, hypertile=None, seg=None):
    """seg: None, or (layers, row0, taps, R, qb) of run_unet.  hypertile: None, or ({walk index of a tiled context block}, (th, tw)) of run_unet.  sag: None, or (walk index of the middle stage's first context block, the mass buffer) of run_unet.  deep: None, or (DeepCache, mode, (a, b), key) of run_unet's cached walk.  fmap: None, or {width of the entering h: (b, s)} of
    the active FreeU stages.  pag: None, or (layers, row0) of run_unet.  tome: None, or ({walk index of a merging context block: r},
    the TokenMerge's record list or None)."""
    state = {"shared": shared}

    def walk(lo, hi, h, hs, sl=None):
        """steps[lo:hi] on h; sl = (b0, b1): h is that slice of the batch (per-sample inputs are sliced alike)."""
        rows = (lambda t: t) if sl is None else (lambda t: None if t is None else t[sl[0]:sl[1]])
        skip = None
        for st in steps[lo:hi]:
            if st[0] == "d":
                di, blk = st[1], st[2]
                eo = emb_outs.get(di)
                if state["shared"]:
                    h = blk(h, None if emb_silu is None else emb_silu[:nb], None, emb_out=None if eo is None else eo[:nb],
                            emb_bias=emb_rows.get(di))
                else:
                    h = blk(h, rows(emb_silu), None, skip=skip, emb_out=rows(eo), emb_bias=emb_rows.get(di))
                skip = None
            elif st[0] == "c":
                share = 1
                if state["shared"]:  # the replicas diverge here
                    rep = lambda t: ops.repeat_batch(t, repeat)   # per-channel statistics of the tensors travel along
                    hs[:] = [rep(t) for t in hs]
                    if CFG_HEAD_SHARE and pag is None and seg is None and len(st[1]) == 1 and sl is None and h.dim() == 4 and _shares_cfg_head(st[1][0]):
                        share = repeat   # ... inside the block, behind its self-attention: h goes in un-replicated
                    else:
                        h = rep(h)
                    state["shared"] = False
                tkw = {} if hypertile is None or st[4] not in hypertile[0] else {"tile": hypertile[1]}
                if pag is not None and st[4] in pag[0]:
                    b0, b1 = (0, h.shape[0]) if sl is None else sl
                    h = run_context(h, st[1], st[2], st[3], sl, repeat=share, ident_from=min(max(pag[1] - b0, 0), b1 - b0), **tkw)
                elif seg is not None and st[4] in seg[0]:
                    b0, b1 = (0, h.shape[0]) if sl is None else sl
                    bf = min(max(seg[1] - b0, 0), b1 - b0)
                    h = run_context(h, st[1], st[2], st[3], sl, repeat=share, blur=(bf, b0 + bf - seg[1], seg[2], seg[3], seg[4]))
                elif tome is not None and st[4] in tome[0]:
                    sink = None if tome[1] is None else (lambda row_of, ci=st[4], rec=tome[1]: rec.append((ci, row_of.clone())))
                    h = run_context(h, st[1], st[2], st[3], sl, repeat=share, tome=(tome[0][st[4]], sink))
                elif sag is not None and st[4] == sag[0]:
                    h = run_context(h, st[1], st[2], st[3], sl, repeat=share, sag=sag[1])
                else:
                    h = run_context(h, st[1], st[2], st[3], sl, repeat=share, **tkw)
            elif st[0] == "save":
                hs.append(h)
            elif st[0] == "load":
                skip = hs.pop()
                bs = None if fmap is None else fmap.get(h.shape[-1])
                if bs is not None:
                    # two fresh tensors (the skip belongs to the stack, h may be the kept feature of a cached walk); a copy
                    # carries no producer statistics, so the consuming GroupNorm and the folded 1x1 skip conv measure them
                    h, skip = ops.freeu(h, skip, bs[0], bs[1])
        assert skip is None
        return h

    hs = []
    region = None
    if BATCH_FORK != "0" and h.is_cuda and h.dim() == 4 and all(len(st[1]) == 1 for st in steps if st[0] == "c"):
        region = _fork_region(steps, h.shape[-2] * h.shape[-1], BATCH_FORK_HW)

    def span(lo, hi, h):
        """steps[lo:hi] on the whole batch; the half-batch fork region is forked where it lies wholly inside the span (a cached
        walk that is cut inside the region walks it unforked)."""
        if region is None or not (lo <= region[0] and region[1] <= hi):
            return walk(lo, hi, h, hs)
        a, b = region
        h = walk(lo, a, h, hs)
        B = h.shape[0]
        if state["shared"] or B < 2 or B % 2 or (BATCH_FORK != "1" and B < BATCH_FORK_MIN):
            return walk(a, hi, h, hs)
        else:
            # two half-batch branches: samples 0 .. B/2 - 1 on the current stream, the rest on a side stream (inside the sampler's
            # HIP graph: parallel branches).  Batch slices of channels-last tensors are contiguous views; the region's skip tensors
            # stay inside it; nothing in it is consumed with producer statistics outside (the Upsample conv behind it takes none).
            # (cached context K/V of the region's blocks are projected -- or refreshed -- HERE, in front of the fork: a branch that
            # projected them on first use would hand the other branch a tensor its stream has not waited for)
            for st in steps[a:b]:
                if st[0] == "c":
                    prepare_context(st[1], st[2])
            # (weight packs are built lazily -- at first use, and again after a weight change or at a new embedding mode -- on the
            # stream of the branch that meets them first: _BranchOrder starts the side branch behind the main branch then; both
            # halves have the same shapes, so the main branch builds every pack the side branch needs)
            main = torch.cuda.current_stream()
            side = _side_streams(h.device, 1, kind="batch")[0]
            order = _BranchOrder(main)
            tok = order.enter(main, first=True)
            h0 = walk(a, b, h[:B // 2], [], (0, B // 2))
            order.leave(main, tok)
            with torch.cuda.stream(side):
                tok = order.enter(side)
                h1 = walk(a, b, h[B // 2:], [], (B // 2, B))
                done = torch.cuda.Event()
                done.record(side)
                order.leave(side, tok)
            h1.record_stream(main)
            main.wait_event(done)
            h = torch.cat([h0, h1], 0)
            return walk(b, hi, h, hs)

    if deep is None:
        h = span(0, len(steps), h)
    else:
        cache, mode, (a, b), key = deep
        if mode == "store":
            h = span(0, b, h)
            cache.store(h, key)     # a side copy: h itself goes on, so the eps is the plain forward's
        else:
            span(0, a, h)           # for its skips alone
            if state["shared"]:     # no context block in front of the cut: the replicas diverge at the jump
                hs[:] = [ops.repeat_batch(t, repeat) for t in hs]
                state["shared"] = False
            h = cache.load(key, hs[-1])   # (a copy carries no producer statistics: the consuming GroupNorm measures it)
        h = span(b, len(steps), h)
    assert not state["shared"], "run_unet(repeat > 1) needs a context block in the input or middle stage"
    return h if h.dim() == 2 else ops.nhwc_to_nchw(h)   # 0-D (text-latent) data flow ends in [B, D]


@register("vd_v2_0")
class VD_v2_0(nn.Module):
    def __init__(self, vae_cfg_list, ctx_cfg_list, diffuser_cfg_list, global_layer_ptr=None, parameterization="eps",
                 timesteps=1000, use_ema=False, beta_schedule="linear", beta_linear_start=1e-4, beta_linear_end=2e-2,
                 given_betas=None, cosine_s=8e-3, loss_type="l2", l_simple_weight=1., l_elbo_weight=0.,
                 v_posterior=0., learn_logvar=False, logvar_init=0, latent_scale_factor=None):
        super().__init__()
        assert parameterization in ["eps", "x0"], 'currently only supporting "eps" and "x0"'
        assert not use_ema, "EMA is a training feature (the reference itself cannot enable it, vd.py:84)"
        self.parameterization = parameterization
        print_log("Running in {} mode".format(parameterization))
        self.vae = self.get_model_list(vae_cfg_list)
        self.ctx = self.get_model_list(ctx_cfg_list)
        self.diffuser = self.get_model_list(diffuser_cfg_list)
        self.global_layer_ptr = global_layer_ptr
        assert self.check_diffuser(), "diffuser layers are not aligned!"
        self.use_ema = use_ema
        self.loss_type, self.l_simple_weight, self.l_elbo_weight = loss_type, l_simple_weight, l_elbo_weight
        self.v_posterior = v_posterior
        self.device = "cpu"
        self.register_schedule(given_betas=given_betas, beta_schedule=beta_schedule, timesteps=timesteps,
                               linear_start=beta_linear_start, linear_end=beta_linear_end, cosine_s=cosine_s)
        self.learn_logvar = learn_logvar
        self.logvar = torch.full(fill_value=logvar_init, size=(self.num_timesteps,))
        self.latent_scale_factor = {} if latent_scale_factor is None else dict(latent_scale_factor)
        self.parameter_group = {}
        for namei, diffuseri in self.diffuser.items():
            self.parameter_group.update({"diffuser_{}_{}".format(namei, pgni): pgi
                                         for pgni, pgi in diffuseri.parameter_group.items()})

    def to(self, device):
        # reference quirk kept on purpose: returns None and records the device (vd.py:114-116)
        self.device = device
        super().to(device)

    def get_model_list(self, cfg_list):
        net = nn.ModuleDict()
        for name, cfg in cfg_list:
            net[name] = String_Reg_Buffer(cfg) if isinstance(cfg, str) else get_model()(cfg)
        return net

    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4,
                          linear_end=2e-2, cosine_s=8e-3):
        betas = given_betas if given_betas is not None else make_beta_schedule(
            beta_schedule, timesteps, linear_start=linear_start, linear_end=linear_end, cosine_s=cosine_s)
        alphas = 1. - betas
        alphas_cumprod = np.cumprod(alphas, axis=0)
        alphas_cumprod_prev = np.append(1., alphas_cumprod[:-1])
        timesteps, = betas.shape
        self.num_timesteps = int(timesteps)
        self.linear_start, self.linear_end = linear_start, linear_end
        assert alphas_cumprod.shape[0] == self.num_timesteps, "alphas have to be defined for each timestep"
        to_torch = partial(torch.tensor, dtype=torch.float32)
        reg = lambda name, arr: self.register_buffer(name, to_torch(arr))
        reg("betas", betas)
        reg("alphas_cumprod", alphas_cumprod)
        reg("alphas_cumprod_prev", alphas_cumprod_prev)
        reg("sqrt_alphas_cumprod", np.sqrt(alphas_cumprod))
        reg("sqrt_one_minus_alphas_cumprod", np.sqrt(1. - alphas_cumprod))
        reg("log_one_minus_alphas_cumprod", np.log(1. - alphas_cumprod))
        reg("sqrt_recip_alphas_cumprod", np.sqrt(1. / alphas_cumprod))
        reg("sqrt_recipm1_alphas_cumprod", np.sqrt(1. / alphas_cumprod - 1))
        posterior_variance = (1 - self.v_posterior) * betas * (1. - alphas_cumprod_prev) / (1. - alphas_cumprod) \
            + self.v_posterior * betas
        reg("posterior_variance", posterior_variance)
        reg("posterior_log_variance_clipped", np.log(np.maximum(posterior_variance, 1e-20)))
        reg("posterior_mean_coef1", betas * np.sqrt(alphas_cumprod_prev) / (1. - alphas_cumprod))
        reg("posterior_mean_coef2", (1. - alphas_cumprod_prev) * np.sqrt(alphas) / (1. - alphas_cumprod))
        # host copies in float32: the sampler reads schedule scalars without a device sync
        self._host_schedule = {"alphas_cumprod": alphas_cumprod.astype(np.float32),
                               "sqrt_alphas_cumprod": np.sqrt(alphas_cumprod).astype(np.float32),
                               "sqrt_one_minus_alphas_cumprod": np.sqrt(1. - alphas_cumprod).astype(np.float32)}

    def host_schedule(self, name):
        """fp32 host copy of a schedule buffer (re-derived from the buffer if a checkpoint overwrote it)."""
        return self._host_schedule[name]

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        for name in list(self._host_schedule):
            if prefix + name in state_dict:
                self._host_schedule[name] = state_dict[prefix + name].detach().float().cpu().numpy()

    def check_diffuser(self):
        orders = [d.layer_order for d in self.diffuser.values()]
        return all(o == orders[0] for o in orders)

    # ---- q(x_t | x_0) ----------------------------------------------------------------------------
    def q_sample(self, x_start, t, noise=None):
        """sqrt(acp_t) x0 + sqrt(1 - acp_t) noise (reference vd.py:221-224); fp16 in / fp16 out on the device."""
        if noise is None:
            noise = torch.randn_like(x_start)
        sa = extract_into_tensor(self.sqrt_alphas_cumprod, t, (t.shape[0],)).float().contiguous()
        sb = extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, (t.shape[0],)).float().contiguous()
        dt = x_start.dtype
        out = ops.q_sample(x_start.to(torch.float16).contiguous(), noise.to(torch.float16).contiguous(), sa.view(-1), sb.view(-1))
        return out.to(dt)

    # ---- VAE / context encoders --------------------------------------------------------------------
    @torch.no_grad()
    def vae_encode(self, x, which, **kwargs):
        scale = (self.latent_scale_factor or {}).get(which, None)
        if scale is not None and hasattr(self.vae[which], "encode_scaled"):
            return self.vae[which].encode_scaled(x, scale=scale, **kwargs)
        z = self.vae[which].encode(x, **kwargs)
        return z if scale is None else scale * z

    @torch.no_grad()
    def vae_decode(self, z, which, **kwargs):
        scale = (self.latent_scale_factor or {}).get(which, None)
        if scale is not None and hasattr(self.vae[which], "decode_scaled"):
            return self.vae[which].decode_scaled(z, inv_scale=1. / scale, **kwargs)
        if scale is not None:
            z = 1. / scale * z
        return self.vae[which].decode(z, **kwargs)

    @torch.no_grad()
    def ctx_encode(self, x, which, **kwargs):
        if which.find("vae_") == 0:
            return self.vae[which[4:]].encode(x, **kwargs)
        return self.ctx[which].encode(x, **kwargs)

    # ---- the UNet forward ----------------------------------------------------------------------------
    def _emb_silu(self, glayer_ptr, timesteps):
        net = self.diffuser[glayer_ptr]
        return net.time_embed.forward_silu(timestep_embedding(timesteps, net.model_channels))

    @torch.no_grad()
    def precompute_step_emb(self, x_type, timesteps, multicontext=False):
        """Everything of the UNet forward that depends on t alone -- timestep_embedding -> time_embed MLP -> SiLU -> every
        ResBlock's emb_layers projection (reference vd.py:339-349, openaimodel.py:2627-2633, :263) -- for ALL `timesteps` [S]
        at once: (fp16 [S, total], layout) of UNetModel2D_Next.precompute_emb_table, or None when the data flow has no such
        table (0-D text-latent flow).  A caller whose batch shares one timestep per step hands row i to apply_model* as
        x_info['emb_rows'] (DDIMSampler does, through a static buffer the step graph reads)."""
        net = self.diffuser[x_type]
        if not hasattr(net, "precompute_emb_table"):
            return None
        glayer_ptr = x_type if (multicontext or self.global_layer_ptr is None) else self.global_layer_ptr
        return net.precompute_emb_table(self._emb_silu(glayer_ptr, timesteps))

    @staticmethod
    def _prep(x):
        if not x.is_cuda:
            raise RuntimeError("VD_v2_0.apply_model needs the latent on the GPU: this package has no CPU path")
        return x.to(torch.float16).contiguous()

    @torch.no_grad()
    def apply_model(self, x_info, timesteps, c_info):
        x_type, x = x_info["type"], x_info["x"]
        c_type, c = c_info["type"], c_info["c"]
        glayer_ptr = x_type if self.global_layer_ptr is None else self.global_layer_ptr
        rows = x_info.get("emb_rows")   # extension key: the t-only part precomputed for a batch that shares its timestep
        deep = _deep_arg(x_info)        # extension key: (DeepCache, "store" | "reuse"), see run_unet
        freeu = _freeu_arg(x_info)      # extension key: (b1, b2, s1, s2), see run_unet
        pag = _pag_fwd_arg(x_info, self.diffuser[x_type])   # extension key: (layers, row0), see run_unet
        seg = _seg_fwd_arg(x_info, self.diffuser[x_type], x.device)   # extension key: (layers, row0, sigma), see run_unet
        tome = _tome_fwd_arg(x_info)    # extension key: a TokenMerge, see run_unet
        hypertile = _hypertile_fwd_arg(x_info)      # extension key: a HyperTile, see run_unet
        sag = _sag_fwd_arg(x_info, 1)   # extension key: the fp32 [1, B, Nm] mass buffer of self-attention guidance, see run_unet
        emb = self._emb_silu(glayer_ptr, timesteps) if rows is None else None
        spec = (self.diffuser[c_type].context_blocks, self._prep(c), 1.0, c_info.get("kv_cache"))
        return run_unet(self.diffuser[x_type], [spec], self._prep(x), emb, repeat=int(x_info.get("repeat", 1)),
                        emb_rows=rows, deep=deep, freeu=freeu, pag=pag, tome=tome, sag=sag,
                        hypertile=hypertile, seg=seg).to(x.dtype)

    @torch.no_grad()
    def apply_model_multicontext(self, x_info, timesteps, c_info_list, mixing_type="attention"):
        """c_info_list: [{type, c, ratio}, ...]; 'attention' mixing = ratio-weighted sum of the context blocks."""
        x_type, x = x_info["type"], x_info["x"]
        assert mixing_type in ("attention", "layer")
        rows = x_info.get("emb_rows")
        deep = _deep_arg(x_info)
        freeu = _freeu_arg(x_info)
        pag = _pag_fwd_arg(x_info, self.diffuser[x_type])
        seg = _seg_fwd_arg(x_info, self.diffuser[x_type], x.device)
        tome = _tome_fwd_arg(x_info)
        hypertile = _hypertile_fwd_arg(x_info)
        sag = _sag_fwd_arg(x_info, len(c_info_list))
        # reference takes time_embed from diffuser[x_type] here (vd.py:415-417)
        emb = self._emb_silu(x_type, timesteps) if rows is None else None
        specs = [(self.diffuser[ci["type"]].context_blocks, self._prep(ci["c"]), ci["ratio"], ci.get("kv_cache"))
                 for ci in c_info_list]
        return run_unet(self.diffuser[x_type], specs, self._prep(x), emb, mixing_type,
                        repeat=int(x_info.get("repeat", 1)), emb_rows=rows, deep=deep, freeu=freeu, pag=pag,
                        tome=tome, sag=sag, hypertile=hypertile, seg=seg).to(x.dtype)
