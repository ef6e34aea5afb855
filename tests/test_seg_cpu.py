"""Smoothed energy guidance on the host: the folded reflection and the tap rule of lib/model_zoo/vd.py against the independent
statements of tests/seg_cases.py (and torch's reflect padding + depthwise conv), the validation of x_info['seg_scale'] /
['seg_blur_sigma'] / ['seg_layers'] at sampler level and of the forward key x_info['seg'] at model level (nothing is drawn and no
device is touched before a raise), the step graph's key, the sharding helper's forwarding, the C ABI listing with the entry's
refusals, the combination rule, and the oracle preconditions: that the project's bounds tell SEG on from off.  No GPU."""
import math

import numpy as np
import pytest
import torch

import deepcache_cases as dc
import pag_cases as pc
import seg_cases as sc
from seg_cases import FWD_TOL, INF, LATENT_TOL, SEG_SCALE
from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg


@pytest.fixture(scope="module")
def tiny_cpu():
    """The tiny product model on the CPU (never run) and its fp32 weights."""
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    return net, synth_into(net, m["seed"])


@pytest.fixture(scope="module")
def plan():
    from oracle import vd_oracle as O
    return O.unet_plan(**meta()["unet2d"])


@pytest.fixture(scope="module")
def gold():
    return load_gold("ddim_tiny.npz")


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
BAD_SCALES = [-1.0, -1e-9, float("nan"), float("inf"), "3", True, (3.0,), [3.0], 1j]
BAD_SIGMAS = [0, 0.0, -1.0, float("nan"), -math.inf, 0.1, 1.0 / 6.0, "1", True, (1.0,), 1j]      # 0.1, 1/6: ceil(6 sigma) < 2, R < 1
BAD_LAYERS = [[], (), (2, 2), (7,), (-1,), (0, 7), (1.0,), (True,), "all", "2", 2, ("mid",), [None]]


# ---- 1. the reflection and the taps ----------------------------------------------------------------------------------------------

def test_folded_reflection_is_the_index_walk_and_torchs_reflect_padding():
    from lib.model_zoo.vd import seg_refl
    for n in (1, 2, 3, 5, 8):
        for i in range(-4 * n - 3, 4 * n + 4):
            assert seg_refl(i, n) == sc.refl(i, n), (i, n)
            assert 0 <= seg_refl(i, n) < n
    assert [seg_refl(i, 4) for i in range(-7, 11)] == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]
    assert all(seg_refl(i, 1) == 0 for i in range(-5, 6))
    # R < n: the index walk is F.pad(mode="reflect") followed by a depthwise conv2d
    g = torch.Generator().manual_seed(1)
    for (gh, gw), sigma in (((8, 8), 1.0), ((5, 7), 0.5), ((16, 12), 2.5), ((4, 6), 0.5), ((8, 9), 1.0)):
        R, w = sc.taps_of(sigma)
        assert R < min(gh, gw)
        q = torch.randn((2, gh * gw, 5), generator=g)
        a, b = sc.blur64(q, gh, gw, w, R), sc.blur_conv(q, gh, gw, w, R)
        assert float((a - b).abs().max()) < 1e-13, (gh, gw, sigma)
    # R >= n and n == 1: written out token by token with the package's fold
    for (gh, gw), R in (((4, 6), 7), ((2, 2), 3), ((1, 1), 1), ((1, 5), 2), ((3, 1), 4)):
        w = np.arange(1, 2 * R + 2, dtype=np.float64)
        w /= w.sum()
        q = torch.randn((1, gh * gw, 2), generator=g).double()
        want = torch.zeros_like(q)
        for y in range(gh):
            for x in range(gw):
                for dy in range(-R, R + 1):
                    for dx in range(-R, R + 1):
                        want[0, y * gw + x] += w[dy + R] * w[dx + R] * q[0, seg_refl(y + dy, gh) * gw + seg_refl(x + dx, gw)]
        assert float((sc.blur64(q, gh, gw, w, R) - want).abs().max()) < 1e-13, (gh, gw, R)
    one = torch.randn((2, 1, 3), generator=g)
    assert torch.equal(sc.blur64(one, 1, 1, sc.DYADIC[1], 1), one.double())          # n == 1: every tap reads the one token


def test_tap_rule_radius_normalisation_and_the_mean_mode():
    from lib.model_zoo.vd import seg_taps
    for sigma, R in ((0.5, 1), (1.0, 3), (2.5, 7), (1.0 / 3.0, 1), (0.17, 1), (10.0, 30)):
        r, w = seg_taps(sigma)
        r2, w2 = sc.taps_of(sigma)
        assert r == r2 == R and w.dtype == np.float32 and w.shape == (2 * R + 1,)
        assert np.array_equal(w, w2.astype(np.float32)) and np.array_equal(w, w[::-1]) and abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
        assert abs(float(w2.sum()) - 1.0) < 1e-15 and w2[R] == w2.max()
    for sigma in (INF, float("inf"), np.inf, 9999, 9999.0, 1e6, np.float32(20000.0)):
        assert seg_taps(sigma) == (-1, None) and sc.taps_of(float(sigma)) == (-1, None)
    assert seg_taps(9998.9)[0] == 29997
    for bad in BAD_SIGMAS:
        with pytest.raises(ValueError, match="seg"):
            seg_taps(bad)


# ---- 2. the keys -----------------------------------------------------------------------------------------------------------------

def test_sampler_keys_are_validated_and_normalised(tiny_cpu):
    from lib.model_zoo.vd import SEG_DEFAULT_SCALE, _pag_arg, _seg_arg
    net = tiny_cpu[0]
    arg = lambda **kw: _seg_arg(dict({"type": "image"}, **kw), net)
    assert SEG_DEFAULT_SCALE == SEG_SCALE == 3.0
    assert arg() is None and arg(seg_scale=None) is None and arg(seg_scale=0) is None and arg(seg_scale=0.0) is None
    for bad in BAD_LAYERS:                                   # ignored when SEG is off, and so is the sigma
        assert arg(seg_scale=0, seg_layers=bad) is None and arg(seg_layers=bad) is None
    assert arg(seg_scale=0, seg_blur_sigma=-1) is None and arg(seg_blur_sigma="x") is None
    assert arg(seg_scale=3) == (3.0, (2,), INF) and arg(seg_scale=np.float32(0.5), seg_layers="mid", seg_blur_sigma=None) == (0.5, (2,), INF)
    assert arg(seg_scale=3.0, seg_layers=[3, 1, 2], seg_blur_sigma=1) == (3.0, (1, 2, 3), 1.0)
    assert arg(seg_scale=3.0, seg_layers=np.array([6, 0]), seg_blur_sigma=np.float32(2.5)) == (3.0, (0, 6), 2.5)
    assert arg(seg_scale=3.0, seg_layers=iter([4]), seg_blur_sigma=INF) == (3.0, (4,), INF)
    for bad in BAD_SCALES:
        with pytest.raises(ValueError, match="seg"):
            arg(seg_scale=bad)
    for bad in BAD_SIGMAS:
        with pytest.raises(ValueError, match="seg"):
            arg(seg_scale=3.0, seg_blur_sigma=bad)
    for bad in BAD_LAYERS:
        with pytest.raises(ValueError, match="seg"):
            arg(seg_scale=3.0, seg_layers=bad)
    with pytest.raises(ValueError, match="seg.*image"):
        _seg_arg({"type": "text", "seg_scale": 3.0}, net)
    with pytest.raises(ValueError, match="seg.*pag_scale.*out of scope"):
        arg(seg_scale=3.0, pag_scale=3.0)
    with pytest.raises(ValueError, match="seg.*sag_scale.*out of scope"):
        arg(seg_scale=3.0, sag_scale=0.75)
    with pytest.raises(ValueError, match="seg.*tome_ratio.*out of scope"):
        arg(seg_scale=3.0, tome_ratio=0.5)
    with pytest.raises(ValueError, match="seg.*cache_interval.*out of scope"):
        arg(seg_scale=3.0, cache_interval=2)
    with pytest.raises(ValueError, match="seg.*region_masks.*out of scope"):
        arg(seg_scale=3.0, region_masks=np.ones((1, 16, 16), np.float32), window=16)
    assert arg(seg_scale=3.0, cache_interval=1, pag_scale=0, sag_scale=None, tome_ratio=0.0) == (3.0, (2,), INF)
    assert _pag_arg({"type": "image", "pag_scale": 3.0}, net) == (3.0, (2,))          # pag's own validator is as it was
    # a chosen layer that HyperTile tiles: block 0 has the 16 x 16 grid of a 16 x 16 latent, tiles of 8 cut it (the middle block's
    # 8 x 8 grid fits in one tile, and tiles of 4 cut it once max_downsample reaches its level)
    shaped = lambda **kw: _seg_arg(dict({"type": "image"}, **kw), net, (1, 4, 16, 16))
    with pytest.raises(ValueError, match="seg.*HyperTile"):
        shaped(seg_scale=3.0, seg_layers=(0,), hypertile=8)
    assert shaped(seg_scale=3.0, seg_layers=(1, 2, 3), hypertile=8) == (3.0, (1, 2, 3), INF)
    assert shaped(seg_scale=3.0, hypertile=8, hypertile_max_downsample=2) == (3.0, (2,), INF)
    assert shaped(seg_scale=3.0, hypertile=4) == (3.0, (2,), INF)
    with pytest.raises(ValueError, match="seg.*HyperTile"):
        shaped(seg_scale=3.0, hypertile=4, hypertile_max_downsample=2)


def test_samplers_raise_before_anything_is_drawn(tiny_cpu):
    model = _NoDevice(tiny_cpu[0])
    state = torch.get_rng_state()
    for s in _samplers(model):
        run = lambda x_type="image", shape=(1, 4, 16, 16), **keys: s.sample(
            steps=5, shape=list(shape), x_info=dict({"type": x_type}, **keys), c_info=dict(C_INFO), verbose=False)
        multi = lambda **keys: s.sample_multicontext(steps=5, shape=[1, 4, 16, 16], x_info=dict({"type": "image"}, **keys),
                                                     c_info_list=[dict(C_INFO)], verbose=False)
        for bad in BAD_SCALES:
            with pytest.raises(ValueError, match="seg"):
                run(seg_scale=bad)
            with pytest.raises(ValueError, match="seg"):
                multi(seg_scale=bad)
        for bad in BAD_SIGMAS:
            with pytest.raises(ValueError, match="seg"):
                run(seg_scale=3.0, seg_blur_sigma=bad)
        for bad in BAD_LAYERS:
            with pytest.raises(ValueError, match="seg"):
                run(seg_scale=3.0, seg_layers=bad)
        with pytest.raises(ValueError, match="seg"):
            run("text", (1, 128), seg_scale=3.0)
        for keys in (dict(pag_scale=3.0), dict(sag_scale=0.75), dict(tome_ratio=0.5), dict(cache_interval=2),
                     dict(window=16, region_masks=np.ones((1, 16, 16), np.float32))):
            with pytest.raises(ValueError, match="out of scope"):
                run(seg_scale=3.0, **keys)
        with pytest.raises(ValueError, match="seg.*HyperTile"):
            run(seg_scale=3.0, seg_layers=(0,), hypertile=8)
        with pytest.raises(ValueError, match="out of scope"):
            multi(seg_scale=3.0, cache_interval=3, cache_depth=2)
        for good in (dict(seg_scale=3.0), dict(seg_scale=0), dict(seg_scale=None, seg_layers=[]), dict(seg_scale=1, seg_layers=(0, 6)),
                     dict(seg_scale=3.0, seg_blur_sigma=1.0), dict(seg_scale=3.0, window=8), dict(seg_scale=3.0, hypertile=8)):
            with pytest.raises(AssertionError, match="touched the device"):
                run(**good)
    assert torch.equal(torch.get_rng_state(), state)        # nothing was drawn from the (host) generator on the way


def test_p_sample_ddim_validates_the_keys(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(_NoDevice(tiny_cpu[0]))
    c_info = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_guidance_scale": 1.0}
    for keys in (dict(seg_scale=-1), dict(seg_scale=3.0, seg_layers=[9]), dict(seg_scale=3.0, seg_blur_sigma=0), dict(seg_scale=3.0, pag_scale=1.0)):
        x_info = dict({"type": "image", "x": torch.zeros(1, 4, 16, 16)}, **keys)
        with pytest.raises(ValueError, match="seg"):
            s.p_sample_ddim(x_info, c_info, torch.tensor([1]), 0)
        with pytest.raises(ValueError, match="seg"):
            s.p_sample_ddim_multicontext(x_info, [c_info], torch.tensor([1]), 0)


def test_forward_key_is_validated(tiny_cpu):
    net = tiny_cpu[0]
    c_info = {"type": "text", "c": torch.zeros(3, 7, 128)}
    t = torch.zeros(3, dtype=torch.long)
    x = torch.zeros(1, 4, 16, 16)
    with pytest.raises(ValueError, match="image"):
        net.apply_model({"type": "text", "x": torch.zeros(1, 128), "seg": ((2,), 1, INF)}, t, c_info)
    for bad in (3, (2,), ((2,), 1), ((2,), 1, INF, 0), ((2,), -1, INF), ((2,), 1.0, INF), ((2,), True, INF), ((7,), 1, INF), ((), 1, INF),
                ((2, 2), 1, INF), ("all", 1, INF), ((2,), 1, 0.0), ((2,), 1, 0.1), ((2,), 1, "inf"), ((2,), 1, float("nan"))):
        with pytest.raises(ValueError, match="seg"):
            net.apply_model({"type": "image", "x": x, "repeat": 3, "seg": bad}, t, c_info)
        with pytest.raises(ValueError, match="seg"):
            net.apply_model_multicontext({"type": "image", "x": x, "repeat": 3, "seg": bad}, t, [dict(c_info, ratio=1.0)])
    with pytest.raises(ValueError, match="seg"):
        net.apply_model({"type": "image", "x": x, "repeat": 3, "seg": ((2,), 2, INF), "pag": ((2,), 2)}, t, c_info)


# ---- 3. the graph key, the workspace, the sharding helper, the C ABI listing --------------------------------------------------------

def test_graph_key_carries_layers_and_radius_but_neither_scale_nor_taps(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(tiny_cpu[0])
    x = torch.zeros(1, 4, 16, 16)
    cis = [{"type": "text", "c": torch.zeros(3, 7, 128)}]
    key = lambda **kw: s._static_key(x, dict({"type": "image"}, **kw), cis, True, True)
    off = key()
    assert key(seg_scale=None) == off and key(seg_scale=0) == off and key(seg_scale=0.0, seg_layers=[5], seg_blur_sigma=1.0) == off
    assert key(seg_layers=[1]) == off and key(seg_blur_sigma=2.0) == off
    on = key(seg_scale=3.0)
    assert on[:-1] == off and on[-1] == ("seg", (2,), -1)                                # the key of today's call, and one entry
    assert key(seg_scale=0.5) == on and key(seg_scale=7, seg_layers="mid", seg_blur_sigma=INF) == on and key(seg_scale=3.0, seg_blur_sigma=1e4) == on
    one = key(seg_scale=3.0, seg_blur_sigma=1.0)
    assert one[-1] == ("seg", (2,), 3) and one != on
    assert key(seg_scale=1.0, seg_blur_sigma=1.1) == one and key(seg_scale=1.0, seg_blur_sigma=1.15) == one  # every sigma of R = 3
    assert key(seg_scale=3.0, seg_blur_sigma=1.2)[-1] == ("seg", (2,), 4)
    assert key(seg_scale=3.0, seg_layers=[3, 2, 1])[-1] == ("seg", (1, 2, 3), -1)
    assert key(pag_scale=3.0) not in (on, off) and key(pag_scale=3.0)[-2] == (True, (2,))    # pag's key is as it was
    both = key(seg_scale=3.0, freeu=(1.2, 1.4, 0.9, 0.2))
    assert both[-2] == (1.2, 1.4, 0.9, 0.2) and both[-1] == on[-1]


def test_workspace_covers_the_largest_chosen_layer(tiny_cpu):
    from lib.model_zoo import vd
    net = tiny_cpu[0]
    grids = vd.seg_grids(net.diffuser["image"], 16, 16)
    assert len(grids) == sc.pc.TINY_BLOCKS and grids[0] == (16, 16) and grids[sc.pc.TINY_MID] == (8, 8) and grids[-1] == (16, 16)
    assert vd.seg_grids(net.diffuser["image"], 16, 24)[0] == (16, 24)
    widths = [int(b[0].proj_in.out_channels) if hasattr(b, "__getitem__") else int(b.proj_in.out_channels)
              for b in net.diffuser["text"].context_blocks]
    for layers in ((2,), (0,), (1, 2, 3), (0, 6)):
        want = max(grids[i][0] * grids[i][1] * widths[i] for i in layers)
        assert vd.seg_workspace_elems(net, ["text"], 16, 16, layers) == want
        assert vd.seg_workspace_elems(net, ["text", "image"], 16, 16, layers) >= want


def test_sharding_helper_forwards_the_keys():
    from lib.model_zoo import sharded
    seen = []

    class Net(object):
        device = "cpu"

        def vae_decode(self, z, which):
            return z

    class Sampler(object):
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=False):
            seen.append(tuple(x_info.get(k, "absent") for k in ("seg_scale", "seg_blur_sigma", "seg_layers")))
            return x_info["xt"], {}

    ctx = lambda: {"type": "text", "conditioning": torch.zeros(2, 7, 16), "unconditional_conditioning": torch.zeros(2, 7, 16)}
    sharded.vd_sample_sharded(Net(), Sampler(), 6, [2, 4, 8, 8], [ctx()], seed=3)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, [2, 4, 8, 8], [ctx()], seed=3, seg_scale=3.0)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, [2, 4, 8, 8], [ctx()], seed=3, seg_scale=2.0, seg_blur_sigma=1.0, seg_layers=(1, 2))
    assert seen == [("absent",) * 3, (3.0, "absent", "absent"), (2.0, 1.0, (1, 2))]


def test_entry_is_declared_and_refuses_bad_arguments_without_a_device():
    import ctypes
    import os
    import re
    from vd_hip.loader import PROTOTYPES, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "vd_hip.h")).read()
    assert re.search(r"\bint vd_attention_qblur_f16\(", hdr) and "vd_attention_qblur_f16" in PROTOTYPES
    assert len(PROTOTYPES["vd_attention_qblur_f16"][1]) == len(PROTOTYPES["vd_attention_ident_f16"][1]) + 5
    assert "seg.hip" in open(os.path.join(root, "versatile-diffusion_amd", "build.py")).read()
    L = lib()
    assert L.vd_abi_version() == 8                  # the entry is additive
    P = ctypes.c_void_p
    ok = dict(q=P(4096), k=P(4096 + 128), v=P(4096 + 256), out=P(1 << 20), B=3, H=2, Nq=64, Nk=64, D=40, ldq=240, ldk=240, ldv=240,
              ldo=80, sq=64 * 240, sk=64 * 240, sv=64 * 240, so=64 * 80, causal=0, blur=1, gh=8, gw=8, taps=P(8192), R=1, qb=P(1 << 21))

    def call(**kw):
        a = dict(ok, **kw)
        return L.vd_attention_qblur_f16(a["q"], a["k"], a["v"], a["out"], a["B"], a["H"], a["Nq"], a["Nk"], a["D"], a["ldq"], a["ldk"],
                                        a["ldv"], a["ldo"], a["sq"], a["sk"], a["sv"], a["so"], 0.125, a["causal"], a["blur"], a["gh"],
                                        a["gw"], a["taps"], a["R"], a["qb"], None)

    for kw in (dict(q=None), dict(v=None), dict(out=None), dict(B=0), dict(H=0), dict(Nq=0), dict(Nk=96), dict(Nq=96), dict(causal=1),
               dict(causal=2), dict(blur=-1), dict(blur=4), dict(gh=8, gw=9), dict(gh=0, gw=64), dict(gh=-8, gw=-8), dict(gh=4, gw=8),
               dict(R=-2), dict(R=-100), dict(taps=None), dict(taps=None, R=0), dict(taps=P(8194)), dict(qb=None), dict(qb=P((1 << 21) + 8)),
               dict(ldq=244), dict(ldq=72), dict(sq=64 * 240 + 4), dict(q=P(4096 + 8)), dict(H=1, D=44)):
        assert call(**kw) < 0 and L.vd_last_error().decode().startswith("vd_attention_qblur_f16"), kw


# ---- 4. the combination rule and the oracle's preconditions ----------------------------------------------------------------------

def test_combine_reproduces_the_formula_guided_and_unguided():
    g = torch.Generator().manual_seed(5)
    e_u, e_c, e_p = [torch.randn((2, 4, 8, 8), generator=g) for _ in range(3)]
    s, sg = 7.5, SEG_SCALE
    assert torch.allclose(sc.combine(torch.cat([e_u, e_c, e_p]), s, sg, True, True), e_u + s * (e_c - e_u) + sg * (e_c - e_p), rtol=0, atol=1e-5)
    assert torch.allclose(sc.combine(torch.cat([e_c, e_p]), 1.0, sg, False, True), e_c + sg * (e_c - e_p), rtol=0, atol=1e-5)
    assert torch.equal(sc.combine(torch.cat([e_u, e_c]), s, sg, True, False), e_u + s * (e_c - e_u))
    assert torch.equal(sc.combine(e_c, 1.0, sg, False, False), e_c)
    # the fold's weight (the samplers reuse pag's) turns the unchanged update into that formula
    from lib.model_zoo.ddim import pag_weight
    w = float(pag_weight(s, sg, True))
    a2 = e_u.double() + w * (e_c.double() - e_p.double())
    assert torch.allclose(a2 + s * (e_c.double() - a2), (e_u + s * (e_c - e_u) + sg * (e_c - e_p)).double(), rtol=0, atol=1e-5)


def _contexts(gold, scale):
    return [{"type": "text", "conditioning": torch.from_numpy(gold["c_text"]), "unconditional_conditioning": torch.from_numpy(gold["u_text"]),
             "unconditional_guidance_scale": scale}]


def test_oracle_walk_off_is_the_plain_walk_and_infinity_is_the_explicit_mean(tiny_cpu, plan, gold):
    from oracle import vd_oracle as O
    sd = tiny_cpu[1]
    xT = torch.from_numpy(gold["xT"]).float()
    cs0 = dc.cfg_contexts(_contexts(gold, 7.5), True)
    t = torch.full((4,), 500, dtype=torch.long)
    plain = dc.walk(sd, plan, torch.cat([xT, xT]), t, cs0)
    assert torch.equal(sc.walk(sd, plan, torch.cat([xT, xT]), t, cs0), plain)
    assert torch.equal(sc.walk(sd, plan, torch.cat([xT, xT]), t, cs0, (1, 2, 3), torch.zeros(4, dtype=torch.bool), 1.0), plain)
    assert pc.spatial_transformer.__module__ == "pag_cases"               # the walk put pag's block back
    xin, cs, mask = sc.replicas(xT, cs0, True, True)
    rec = []
    e = sc.walk(sd, plan, xin, torch.full((6,), 500, dtype=torch.long), cs, (1, 2, 3), mask, 1.0, record=rec)
    assert rec == [1, 2, 3] and rel_l2(e[:4], plain) < 1e-5               # the unperturbed replicas do not see the perturbed one
    # sigma = inf, 9999 and the explicit mean query are one thing
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 12, 64), generator=g)
    p = "diffuser.text.context_blocks.0.0.transformer_blocks.0.attn1"
    heads = plan["ctx"][0][1]
    q = torch.nn.functional.linear(x, sd[p + ".to_q.weight"])
    assert torch.allclose(sc.blur64(q, 3, 4, None, -1), q.double().mean(1, keepdim=True).expand(-1, 12, -1), rtol=0, atol=1e-12)
    a_inf = sc.blurred_self_attention(sd, p, x, heads, 3, 4, INF)
    assert torch.equal(a_inf, sc.blurred_self_attention(sd, p, x, heads, 3, 4, 9999.0))
    d = q.shape[-1] // heads
    sp = lambda t_: t_.view(2, t_.shape[1], heads, d).transpose(1, 2)
    k, v = torch.nn.functional.linear(x, sd[p + ".to_k.weight"]), torch.nn.functional.linear(x, sd[p + ".to_v.weight"])
    qm = q.mean(1, keepdim=True).expand_as(q).contiguous()
    want = O._lin(sd, p + ".to_out.0", ((sp(qm) @ sp(k).transpose(-1, -2) * d ** -0.5).softmax(-1) @ sp(v)).transpose(1, 2).reshape(2, 12, -1))
    assert rel_l2(a_inf, want) < 1e-5
    assert rel_l2(sc.blurred_self_attention(sd, p, x, heads, 3, 4, 1.0), O.cross_attention(sd, p, x, None, heads)) > 1e-3


@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("layers", sc.LAYER_CASES)
def test_forward_precondition_the_perturbed_replica_is_far_from_the_conditional(tiny_cpu, plan, gold, layers, sigma):
    sd = tiny_cpu[1]
    xT = torch.from_numpy(gold["xT"]).float()
    xin, cs, mask = sc.replicas(xT, dc.cfg_contexts(_contexts(gold, 7.5), True), True, True)
    e_u, e_c, e_p = sc.walk(sd, plan, xin, torch.full((6,), 500, dtype=torch.long), cs, sc.layers_of(plan, layers), mask, sigma).chunk(3)
    gap = rel_l2(e_p, e_c)
    print("layers %r sigma %r: rel-L2 of e_p vs e_c at t = 500: %.3f" % (layers, sigma, gap))
    assert gap >= 10 * FWD_TOL and bool(torch.isfinite(e_p).all())


@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("scale", [7.5, 1.0])
def test_loop_precondition_five_ddim_steps_on_vs_off(tiny_cpu, plan, gold, scale, sigma):
    from lib.model_zoo.ddim import DDIMSampler
    net, sd = tiny_cpu
    xT = torch.from_numpy(gold["xT"]).float()
    s = DDIMSampler(net)
    s.make_schedule(5, verbose=False)
    on = sc.oracle_loop(sd, plan, s, "ddim", xT, _contexts(gold, scale), scale, SEG_SCALE, sc.LOOP_LAYERS, sigma)
    off = sc.oracle_loop(sd, plan, s, "ddim", xT, _contexts(gold, scale), scale, 0.0)
    assert torch.equal(off, dc.oracle_loop(sd, plan, s, "ddim", xT, _contexts(gold, scale), scale))      # off is the plain oracle loop
    gap = rel_l2(on, off)
    print("s %.1f sigma %r: five DDIM steps on vs off %.3e, max |z| %.1f" % (scale, sigma, gap, float(on.abs().max())))
    assert gap > LATENT_TOL and bool(torch.isfinite(on).all()) and float(on.abs().max()) < 40.


def test_entry_bounds_hold_for_fp32_arithmetic_done_in_numpy():
    """The kernel's chain restated with numpy fp32 stays inside the per-element bounds the GPU tests assert."""
    g = torch.Generator().manual_seed(9)
    for (gh, gw), sigma in (((5, 7), 2.5), ((8, 8), 1.0), ((4, 6), 2.5)):
        R, w64 = sc.taps_of(sigma)
        w = w64.astype(np.float32)
        q = torch.randn((1, gh * gw, 8), generator=g).half()
        qn = q.float().numpy().reshape(gh, gw, 8)
        h = np.zeros_like(qn)
        for d in range(-R, R + 1):      # (numpy has no fma: the product and the sum each round once, within the bound's slack)
            h = (h + w[d + R] * qn[:, [sc.refl(x + d, gw) for x in range(gw)]]).astype(np.float32)
        a = np.zeros_like(qn)
        for d in range(-R, R + 1):
            a = (a + w[d + R] * h[[sc.refl(y + d, gh) for y in range(gh)]]).astype(np.float32)
        out = torch.from_numpy(a).half().double().reshape(1, gh * gw, 8)
        ref, bound = sc.blur_bound(q, gh, gw, w, R)
        assert ((out - ref).abs().numpy() <= 2 * bound).all()       # two roundings per tap here, one in the kernel
        mref, mbound = sc.mean_bound(q)
        acc = np.float32(0)
        m = np.zeros(8, np.float32)
        for n in range(gh * gw):
            m = (m + q[0, n].float().numpy()).astype(np.float32)
        mout = torch.from_numpy((m / np.float32(gh * gw)).astype(np.float32)).half().double()
        assert ((mout[None, None, :] - mref).abs().numpy() <= mbound).all()
