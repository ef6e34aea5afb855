"""HyperTile on the host: the index map of tests/hypertile_cases.py (a permutation, its inverse, the reshape / permute form), which
blocks of the tiny and of the full-width walk tile at which latent, the validation of x_info['hypertile'] /
['hypertile_max_downsample'] at sampler level (nothing is drawn and no device is touched before a raise), the step graph's key, the
sharding helper's forwarding, the C ABI listing and the entries' argument checks (they need no device).  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import hypertile_cases as hc
from vdtest_util import meta, synth_into, tiny_vd_cfg


@pytest.fixture(scope="module")
def tiny_cpu():
    """The tiny product model on the CPU (never run) and its fp32 weights."""
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    return net, synth_into(net, m["seed"])


@pytest.fixture(scope="module")
def full_net():
    from lib.cfg_helper import model_cfg_bank
    from lib.model_zoo import get_model
    with torch.device("meta"):          # the structure only: no weight is allocated
        return get_model()(model_cfg_bank()("openai_unet_2d_v1"), verbose=False)


class _NoDevice(object):
    """A model that has the tiny net's diffusers and schedule but raises as soon as a sampler asks for its device."""
    num_timesteps = 1000

    def __init__(self, net):
        self.diffuser = net.diffuser
        self.alphas_cumprod = net.alphas_cumprod

    @property
    def device(self):
        raise AssertionError("the sampler touched the device before validating its arguments")


def _samplers(model):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    from lib.model_zoo.unipc import UniPCSampler
    return [DDIMSampler(model), DPMSolverSampler(model), DPMSolverSDESampler(model, eta=0.), UniPCSampler(model)]


C_INFO = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_conditioning": torch.zeros(1, 7, 128),
          "unconditional_guidance_scale": 7.5}
BAD_TILES = [True, False, 1, -8, 8.0, 0.0, "8", (8,), [8, 8], float("nan"), 1j]
BAD_DOWNSAMPLES = [0, 3, 8, 1.0, 2.0, "1", True, (1,)]


# ---- 1. the index map ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,th,tw", hc.MAP_CASES)
def test_index_map_is_a_permutation_and_its_inverse_undoes_it(H, W, th, tw):
    perm, inv = hc.index_map(H, W, th, tw), hc.inverse_map(H, W, th, tw)
    N = H * W
    assert perm.shape == (N,) and np.array_equal(np.sort(perm), np.arange(N))
    assert np.array_equal(perm[inv], np.arange(N)) and np.array_equal(inv[perm], np.arange(N))
    # the formula of include/vd_hip.h, element by element
    ntx = W // tw
    for ty in range(H // th):
        for tx in range(ntx):
            for i in range(th):
                for j in range(tw):
                    assert perm[(ty * ntx + tx) * th * tw + i * tw + j] == (ty * th + i) * W + tx * tw + j
    # a tile holds exactly the tokens of its rectangle
    for t in range(N // (th * tw)):
        y, x = np.divmod(perm[t * th * tw:(t + 1) * th * tw], W)
        assert y.max() - y.min() == th - 1 and x.max() - x.min() == tw - 1 and y.min() % th == 0 and x.min() % tw == 0
    # the reshape / permute form is the same map, and untile undoes tile
    tok = torch.arange(2 * N * 3).view(2, N, 3)
    tiled = hc.tile_ref(tok, H, W, th, tw)
    assert tuple(tiled.shape) == (2 * N // (th * tw), th * tw, 3)
    assert torch.equal(tiled.reshape(2, N, 3), tok[:, torch.from_numpy(perm)])
    assert torch.equal(hc.untile_ref(tiled, 2, H, W, th, tw), tok)
    if (th, tw) == (H, W):
        assert np.array_equal(perm, np.arange(N))


# ---- 2. the keys -----------------------------------------------------------------------------------------------------------------

def test_sampler_keys_are_validated(tiny_cpu):
    from lib.model_zoo.vd import HyperTile, _hypertile_arg
    net = tiny_cpu[0]
    arg = lambda shape=None, **kw: _hypertile_arg(dict({"type": "image"}, **kw), net, shape)
    assert arg() is None and arg(hypertile=None) is None and arg(hypertile=0) is None
    assert arg(hypertile=0, hypertile_max_downsample=2) is None and arg(hypertile_max_downsample=4) is None
    ht = arg(hypertile=8)
    assert isinstance(ht, HyperTile) and ht.key() == (8, 1) and (ht.tile, ht.max_downsample) == (8, 1)
    assert arg(hypertile=np.int64(4), hypertile_max_downsample=2).key() == (4, 2) and arg(hypertile=2, hypertile_max_downsample=4).key() == (2, 4)
    ready = HyperTile(8, 2)
    assert arg(hypertile=ready) is ready and arg(hypertile=ready, hypertile_max_downsample=2) is ready
    with pytest.raises(ValueError, match="hypertile"):
        arg(hypertile=ready, hypertile_max_downsample=1)
    for bad in BAD_TILES:
        with pytest.raises(ValueError, match="hypertile"):
            arg(hypertile=bad)
    for bad in BAD_DOWNSAMPLES:
        with pytest.raises(ValueError, match="hypertile"):
            arg(hypertile=8, hypertile_max_downsample=bad)
        with pytest.raises(ValueError, match="hypertile"):
            arg(hypertile_max_downsample=bad)           # a bad value is not hidden by the key being off
    with pytest.raises(ValueError, match="hypertile.*image"):
        _hypertile_arg({"type": "text", "hypertile": 8}, net)
    with pytest.raises(ValueError, match="hypertile.*tome"):
        arg(hypertile=8, tome_ratio=0.5)
    assert arg(hypertile=8, tome_ratio=0).key() == (8, 1)
    # perturbed-attention guidance combines (CrossAttention keeps the identity rows of a tiled layer)
    assert arg((1, 4, 16, 16), hypertile=8, pag_scale=3.0, pag_layers=(0,)).key() == (8, 1)
    # grids: a tiled level must be whole tiles; a level that fits in one tile is left alone
    assert arg((1, 4, 16, 24), hypertile=8) is not None and arg((1, 4, 6, 7), hypertile=8) is not None
    for shape in [(1, 4, 16, 20), (1, 4, 12, 16), (1, 4, 4, 12)]:
        with pytest.raises(ValueError, match="hypertile.*divide"):
            arg(shape, hypertile=8)
    with pytest.raises(ValueError, match="hypertile.*divide"):
        arg((1, 4, 16, 24), hypertile=8, hypertile_max_downsample=2)                      # level 1 is 8 x 12: wider than one tile
    assert arg((1, 4, 16, 24), hypertile=4, hypertile_max_downsample=2).key() == (4, 2)   # ... and 4 divides both levels
    # a window's side decides, not the canvas'
    with pytest.raises(ValueError, match="hypertile.*divide"):
        arg((1, 4, 16, 32), hypertile=8, window=(16, 12))
    assert arg((1, 4, 16, 30), hypertile=8, window=(16, 16)) is not None
    # self-attention guidance reads the middle block's map: fine while that block is untiled (8 x 8 on the tiny net) ...
    assert arg((1, 4, 16, 16), hypertile=8, hypertile_max_downsample=2, sag_scale=0.75) is not None
    assert arg((1, 4, 16, 16), hypertile=4, sag_scale=0.75) is not None
    # ... refused when the tile would cut it
    with pytest.raises(ValueError, match="hypertile.*sag"):
        arg((1, 4, 16, 16), hypertile=4, hypertile_max_downsample=2, sag_scale=0.75)
    assert arg((1, 4, 16, 16), hypertile=4, hypertile_max_downsample=2, sag_scale=0) is not None


def test_samplers_raise_before_anything_is_drawn(tiny_cpu):
    model = _NoDevice(tiny_cpu[0])
    state = torch.get_rng_state()
    for s in _samplers(model):
        run = lambda x_type="image", shape=(1, 4, 16, 16), **keys: s.sample(
            steps=5, shape=list(shape), x_info=dict({"type": x_type}, **keys), c_info=dict(C_INFO), verbose=False)
        multi = lambda **keys: s.sample_multicontext(steps=5, shape=[1, 4, 16, 16], x_info=dict({"type": "image"}, **keys),
                                                     c_info_list=[dict(C_INFO)], verbose=False)
        for bad in BAD_TILES:
            with pytest.raises(ValueError, match="hypertile"):
                run(hypertile=bad)
        with pytest.raises(ValueError, match="hypertile"):
            multi(hypertile=8, hypertile_max_downsample=3)
        with pytest.raises(ValueError, match="hypertile.*image"):
            run("text", shape=(1, 768), hypertile=8)
        with pytest.raises(ValueError, match="hypertile.*divide"):
            run(shape=(1, 4, 16, 20), hypertile=8)
        with pytest.raises(ValueError, match="hypertile.*tome"):
            run(hypertile=8, tome_ratio=0.5)
        with pytest.raises(ValueError, match="hypertile.*sag"):
            run(hypertile=4, hypertile_max_downsample=2, sag_scale=0.75)
        with pytest.raises(ValueError, match="hypertile"):
            s.p_sample_ddim({"type": "image", "x": torch.zeros(1, 4, 16, 16), "hypertile": 1}, dict(C_INFO), torch.zeros(1, dtype=torch.long), 0)
    assert torch.equal(torch.get_rng_state(), state)


def test_forward_key_is_validated():
    from lib.model_zoo.vd import HyperTile, TokenMerge, _hypertile_fwd_arg
    ht = HyperTile(8)
    assert _hypertile_fwd_arg({"type": "image"}) is None and _hypertile_fwd_arg({"type": "image", "hypertile": None}) is None
    assert _hypertile_fwd_arg({"type": "image", "hypertile": 0}) is None
    assert _hypertile_fwd_arg({"type": "image", "hypertile": ht}) is ht
    assert _hypertile_fwd_arg({"type": "image", "hypertile": 4, "hypertile_max_downsample": 2}).key() == (4, 2)
    for bad in (0.5, (8, 8), "on", True, 1):
        with pytest.raises(ValueError, match="hypertile"):
            _hypertile_fwd_arg({"type": "image", "hypertile": bad})
    with pytest.raises(ValueError, match="hypertile.*image"):
        _hypertile_fwd_arg({"type": "text", "hypertile": ht})
    with pytest.raises(ValueError, match="hypertile.*tome"):
        _hypertile_fwd_arg({"type": "image", "hypertile": ht, "tome": TokenMerge(0.5)})


# ---- 3. which blocks tile --------------------------------------------------------------------------------------------------------

def test_tiled_blocks_of_the_tiny_net(tiny_cpu):
    from lib.model_zoo.vd import HyperTile, hypertile_blocks
    net = tiny_cpu[0].diffuser["image"]
    # the tiny walk: context blocks 0 (16x16), 1 (8x8), 2 (middle, 8x8), 3, 4 (8x8), 5, 6 (16x16)
    top = [(ci, 16, 16, 2, 2) for ci in (0, 5, 6)]
    assert hypertile_blocks(net, 16, 16, HyperTile(8)) == top
    assert hypertile_blocks(net, 16, 16, HyperTile(8, 2)) == top          # 8 x 8 fits in one tile: absent
    assert hypertile_blocks(net, 16, 16, HyperTile(8, 4)) == top
    assert hypertile_blocks(net, 16, 16, HyperTile(16, 4)) == [] and hypertile_blocks(net, 16, 16, HyperTile(32)) == []
    four = hypertile_blocks(net, 16, 16, HyperTile(4, 2))
    assert [b[0] for b in four] == list(range(7)) and four[0] == (0, 16, 16, 4, 4) and four[1] == (1, 8, 8, 2, 2)
    assert hypertile_blocks(net, 16, 16, HyperTile(4)) == [(ci, 16, 16, 4, 4) for ci in (0, 5, 6)]
    assert hypertile_blocks(net, 16, 24, HyperTile(8))[0] == (0, 16, 24, 2, 3)
    assert hypertile_blocks(net, 8, 16, HyperTile(8)) == [(ci, 8, 16, 1, 2) for ci in (0, 5, 6)]     # one tile high, two wide
    with pytest.raises(ValueError, match="hypertile"):
        hypertile_blocks(tiny_cpu[0].diffuser["text"], 16, 16, HyperTile(8))
    # the restatement's rule names the same blocks
    for ht in (HyperTile(8), HyperTile(4, 2), HyperTile(8, 4)):
        for ci, H, W, nty, ntx in hypertile_blocks(net, 16, 16, ht):
            assert hc.tiles_of((H, W), (16, 16), ht.tile, ht.max_downsample) == (nty, ntx)
    assert hc.tiles_of((8, 8), (16, 16), 8, 2) is None and hc.tiles_of((8, 8), (16, 16), 4, 1) is None


L0, L1, L2 = (0, 1, 13, 14, 15), (2, 3, 10, 11, 12), (4, 5, 7, 8, 9)      # the full walk's context blocks per level; 6 is the middle


@pytest.mark.parametrize("side,tile,md,want", [
    # (H, W), tile, max_downsample -> {level: (nty, ntx)}
    ((16, 16), 32, 4, {}),
    ((16, 16), 8, 1, {0: (2, 2)}),
    ((16, 16), 8, 4, {0: (2, 2)}),                          # 8 x 8 and 4 x 4 fit in one tile
    ((64, 64), 32, 1, {0: (2, 2)}),
    ((64, 64), 32, 2, {0: (2, 2)}),                         # level 1 is 32 x 32: one tile, absent
    ((64, 64), 32, 4, {0: (2, 2)}),
    ((64, 64), 16, 2, {0: (4, 4), 1: (2, 2)}),
    ((64, 64), 8, 4, {0: (8, 8), 1: (4, 4), 2: (2, 2)}),
    ((96, 96), 48, 1, {0: (2, 2)}),
    ((96, 96), 48, 4, {0: (2, 2)}),
    ((96, 96), 24, 4, {0: (4, 4), 1: (2, 2)}),              # level 2 is 24 x 24: one tile
    ((96, 96), 32, 1, {0: (3, 3)}),
    ((64, 256), 32, 1, {0: (2, 8)}),
    ((64, 256), 32, 2, {0: (2, 8), 1: (1, 4)}),
    ((64, 256), 64, 4, {0: (1, 4), 1: None}),               # level 1 is 32 x 128: 32 is no multiple of 64
    ((64, 256), 32, 4, {0: (2, 8), 1: (1, 4), 2: None}),    # level 2 is 16 x 64
    ((64, 256), 16, 4, {0: (4, 16), 1: (2, 8), 2: (1, 4)}),
])
def test_tiled_blocks_of_a_full_width_walk(full_net, side, tile, md, want):
    from lib.model_zoo.vd import HyperTile, hypertile_blocks
    H0, W0 = side
    if any(v is None for v in want.values()):
        with pytest.raises(ValueError, match="hypertile.*divide"):
            hypertile_blocks(full_net, H0, W0, HyperTile(tile, md))
        return
    expect = []
    for level, idx in enumerate((L0, L1, L2)):
        if level in want:
            expect += [(ci, H0 >> level, W0 >> level) + want[level] for ci in idx]
    got = hypertile_blocks(full_net, H0, W0, HyperTile(tile, md))
    assert got == sorted(expect) and all(b[0] != 6 for b in got)


# ---- 4. graph key, sharding, ABI -------------------------------------------------------------------------------------------------

def test_graph_key_tells_settings_apart_and_off_is_the_key_without_it(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(tiny_cpu[0])
    x = torch.zeros(1, 4, 16, 16)
    cis = [{"type": "text", "c": torch.zeros(2, 7, 128)}]
    key = lambda **kw: s._static_key(x, dict({"type": "image"}, **kw), cis, True, True)
    off = key()
    assert key(hypertile=0) == off and key(hypertile=None) == off and key(hypertile=None, hypertile_max_downsample=2) == off
    on = key(hypertile=8)
    assert on[:len(off)] == off and len(on) == len(off) + 1 and on[-1] == ("hypertile", 8, 1)       # off: nothing was added
    keys = [off, on, key(hypertile=4), key(hypertile=8, hypertile_max_downsample=2), key(hypertile=8, sag_scale=0.75), key(sag_scale=0.75)]
    assert len(set(keys)) == 6 and key(hypertile=8) == on


def test_sharded_helper_forwards_the_keys():
    import inspect
    from lib.model_zoo import sharded
    sig = inspect.signature(sharded.vd_sample_sharded)
    assert sig.parameters["hypertile"].default is None and sig.parameters["hypertile_max_downsample"].default is None
    src = inspect.getsource(sharded.vd_sample_sharded)
    assert 'x_info["hypertile"] = hypertile' in src and 'x_info["hypertile_max_downsample"] = hypertile_max_downsample' in src


def test_abi_lists_the_entries_the_library_exports_them_and_stays_at_8():
    import os
    from vd_hip import loader
    names = ("vd_tile_tokens_f16", "vd_untile_tokens_f16")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "vd_hip.h")) as f:
        text = f.read()
    h = loader.lib()
    for name in names:
        assert name in loader.PROTOTYPES and ("int %s(" % name) in text and hasattr(h, name)
    assert "#define VD_HIP_ABI_VERSION 8" in text and h.vd_abi_version() == 8
    from vd_hip import ops
    assert callable(ops.tile_tokens) and callable(ops.untile_tokens)


def test_entries_refuse_bad_arguments_without_a_device():
    """The argument checks run in front of the launch, so they need no GPU: every refusal names its entry and nothing is launched
    (a launch on this host would fail with another message)."""
    from vd_hip import loader
    h = loader.lib()
    buf = (ctypes.c_uint8 * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, q = ctypes.c_void_p(base), ctypes.c_void_p(base + 2048)
    tile = lambda x=p, ldx=8, sx=128, cols=8, B=1, H=4, W=4, th=2, tw=2, out=q: h.vd_tile_tokens_f16(x, ldx, sx, cols, B, H, W, th, tw, out, None)
    untile = lambda a=p, cols=8, B=1, H=4, W=4, th=2, tw=2, out=q, ldo=8, so=128: h.vd_untile_tokens_f16(a, cols, B, H, W, th, tw, out, ldo, so, None)
    odd = ctypes.c_void_p(base + 8)
    bad = [dict(x=None), dict(out=None), dict(cols=12), dict(cols=0), dict(cols=-8), dict(H=5), dict(W=6, tw=4), dict(B=0), dict(H=0), dict(th=0),
           dict(tw=-2), dict(ldx=0), dict(ldx=4), dict(ldx=12, cols=8), dict(sx=132), dict(x=odd), dict(out=odd), dict(B=2, sx=64)]
    for kw in bad:
        assert tile(**kw) < 0, kw
        assert h.vd_last_error().decode().startswith("vd_tile_tokens_f16"), (kw, h.vd_last_error())
        kw = {{"x": "out", "out": "a", "ldx": "ldo", "sx": "so"}.get(k, k): v for k, v in kw.items()}
        assert untile(**kw) < 0, kw
        assert h.vd_last_error().decode().startswith("vd_untile_tokens_f16"), (kw, h.vd_last_error())
