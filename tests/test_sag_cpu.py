"""Self-attention guidance without a GPU: the definition's pieces against torch (taps, reflect padding, nearest neighbour, the blur),
the fold algebra in float64, the sampler keys, what the samplers refuse before anything is drawn, the declared entries, and the
preconditions of the GPU cases of tests/test_sag_gpu.py (the selector lead, the score bound, the mass margin)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_cases as ac
import sag_cases as sc
from sag_cases import SAG_SCALE, STEPS
from vdtest_util import meta, synth_into, tiny_vd_cfg


@pytest.fixture(scope="module")
def tiny_cpu():
    """The tiny product model on the CPU (never run) and its fp32 weights, sharpened like the GPU tests' (sag_cases.sharpen)."""
    from lib.model_zoo import get_model
    from oracle import vd_oracle as O
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    plan = O.unet_plan(**m["unet2d"])
    return net, sc.sharpen(synth_into(net, m["seed"]), plan), plan


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
    return {"ddim": DDIMSampler(model), "2m": DPMSolverSampler(model), "sde": DPMSolverSDESampler(model), "unipc": UniPCSampler(model)}


C_INFO = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_conditioning": torch.zeros(1, 7, 128),
          "unconditional_guidance_scale": 7.5}
BAD_SCALES = [-1.0, -1e-9, float("nan"), float("inf"), "0.75", True, (0.75,), [0.75], 1j]
BAD_SIGMAS = [0, 0.0, -1.0, float("nan"), float("inf"), "1", True, (1.0,)]


# ---- 1. the definition -----------------------------------------------------------------------------------------------------------

def test_taps_sum_to_one_and_are_symmetric():
    from lib.model_zoo.vd import sag_taps
    for sigma in (0.5, 1.0, 2.0, 7.0):
        g = sc.taps(sigma)
        assert g.shape == (9,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 4 and (g > 0).all()
        assert np.array_equal(sag_taps(sigma), g)
        k = torch.arange(9, dtype=torch.float64) - 4
        pdf = torch.exp(-0.5 * (k / sigma) ** 2)                 # diffusers' gaussian_blur_2d at kernel size 9
        assert np.allclose((pdf / pdf.sum()).numpy(), g, rtol=1e-14, atol=0)


def test_refl_is_torchs_reflect_padding():
    for n in (5, 6, 8, 17):
        row = torch.arange(n, dtype=torch.float64).view(1, 1, n)
        padded = F.pad(row, (4, 4), mode="reflect").view(-1).numpy().astype(np.int64)
        assert np.array_equal(sc.refl(np.arange(-4, n + 4), n), padded)
    assert int(sc.refl(-1, 8)) == 1 and int(sc.refl(8, 8)) == 6


def test_nearest_rule_is_interpolate_nearest_on_integer_ratios():
    for H, W, Hm, Wm in ((8, 8, 2, 2), (16, 24, 2, 3), (64, 96, 8, 12), (5, 5, 1, 1), (16, 16, 8, 8)):
        cells = torch.arange(Hm * Wm, dtype=torch.float32).view(1, 1, Hm, Wm)
        up = F.interpolate(cells, size=(H, W), mode="nearest").view(H, W).numpy().astype(np.int64)
        assert np.array_equal(sc.nearest(H, W, Hm, Wm), up)
    idx = sc.nearest(20, 20, 3, 3)                               # no integer ratio: the integer rule itself
    assert idx[6, 7] == (6 * 3 // 20) * 3 + 7 * 3 // 20 and idx.max() == 8 and idx[19, 19] == 8


def test_blur_is_pad_reflect_and_two_convolutions():
    g = torch.Generator().manual_seed(2)
    p0 = torch.randn((2, 3, 7, 11), generator=g, dtype=torch.float64)
    for sigma in (1.0, 2.0):
        ref = sc.blur64(p0.numpy(), sc.taps(sigma))
        assert np.abs(sc.blur32(p0.float(), sigma).double().numpy() - ref).max() < 1e-5
        assert np.abs(sc.blur64(np.ones((5, 5)), sc.taps(sigma)) - 1.0).max() < 1e-15


def test_fold_algebra_in_float64():
    from lib.model_zoo.ddim import pag_weight, sag_weight
    rng = np.random.default_rng(0)
    e_u, e_c, e_d = rng.standard_normal((3, 50))
    for s, s_sag in ((7.5, 0.75), (1.5, 5.0), (0.5, 1.0), (12.0, 0.1)):
        w = sag_weight(s, s_sag, True)
        assert w.dtype == np.float32 and w == np.float32(-np.float64(s_sag) / (np.float64(s) - 1.0)) == pag_weight(s, s_sag, True)
        a = e_u + float(w) * (e_u - e_d)
        target = e_u + s * (e_c - e_u) + s_sag * (e_u - e_d)
        assert np.abs(a + s * (e_c - a) - target).max() <= 2.0 ** -22 * (np.abs(target).max() + s * np.abs(e_u - e_d).max())
        w1 = sag_weight(1.0, s_sag, False)
        assert w1 == np.float32(s_sag)
        target = e_c + s_sag * (e_c - e_d)
        assert np.abs(e_c + float(w1) * (e_c - e_d) - target).max() <= 2.0 ** -23 * s_sag * np.abs(e_c - e_d).max()
    a, d = torch.tensor([3.0, -0.0, 8.0]).half(), torch.tensor([1.0, 4.0, -8.0]).half()
    assert torch.equal(sc.fold_ref64(a, d, -0.5), torch.tensor([2.0, 2.0, 0.0], dtype=torch.float64))


def test_coef_table_and_ratios():
    from lib.model_zoo.ddim import sag_coef_table, sag_ratios
    ac_ = np.linspace(0.999, 0.005, 1000).astype(np.float32)
    ts = np.array([1, 251, 501, 751])
    tab = sag_coef_table(ac_, ts)
    assert tab.dtype == np.float32 and tab.shape == (4, 3)
    for i, t in enumerate(ts):
        assert np.array_equal(tab[i], np.float32(sc.coef_of(np.float64(ac_[t]))))
    assert np.array_equal(sag_ratios([{"ratio": 1.0}]), np.float32([1.0])) and np.array_equal(sag_ratios([{}]), np.float32([1.0]))
    assert np.array_equal(sag_ratios([{"ratio": 0.4}, {"ratio": 0.6}]), (np.array([0.4, 0.6]) / np.array([0.4, 0.6]).sum()).astype(np.float32))


# ---- 2. the keys -----------------------------------------------------------------------------------------------------------------

def test_map_size_of_the_tiny_and_the_full_net(tiny_cpu):
    from lib.model_zoo import vd
    net = tiny_cpu[0].diffuser["image"]
    assert vd.sag_map_size(net, 16, 16) == sc.TINY_MAP and vd.sag_map_size(net, 8, 8) == (4, 4) and vd.sag_map_size(net, 64, 256) == (32, 128)
    with pytest.raises(ValueError, match="sag"):
        vd.sag_map_size(tiny_cpu[0].diffuser["text"], 16, 16)


def test_sampler_keys_are_validated(tiny_cpu):
    from lib.model_zoo.vd import _sag_arg
    net = tiny_cpu[0]
    arg = lambda shape=None, **kw: _sag_arg(dict({"type": "image"}, **kw), net, shape)
    assert arg() is None and arg(sag_scale=None) is None and arg(sag_scale=0) is None and arg(sag_scale=0.0) is None
    for bad in BAD_SIGMAS:                                    # ignored when SAG is off
        assert arg(sag_scale=0, sag_blur_sigma=bad) is None and arg(sag_blur_sigma=bad) is None
    assert arg(sag_scale=0.75) == (0.75, 1.0) and arg(sag_scale=np.float32(0.5), sag_blur_sigma=2) == (0.5, 2.0)
    assert arg([1, 4, 16, 16], sag_scale=1) == (1.0, 1.0) and arg([1, 4, 5, 5], sag_scale=1) == (1.0, 1.0)
    for bad in BAD_SCALES:
        with pytest.raises(ValueError, match="sag"):
            arg(sag_scale=bad)
    for bad in BAD_SIGMAS:
        with pytest.raises(ValueError, match="sag"):
            arg(sag_scale=0.75, sag_blur_sigma=bad)
    with pytest.raises(ValueError, match="sag.*image"):
        _sag_arg({"type": "text", "sag_scale": 0.75}, net)
    for shape in ([1, 4, 4, 8], [1, 4, 8, 4], [1, 4, 16]):
        with pytest.raises(ValueError, match="sag"):
            arg(shape, sag_scale=0.75)
    with pytest.raises(ValueError, match="sag.*1024"):
        arg([1, 4, 64, 80], sag_scale=0.75)                    # 32 x 40 middle tokens
    assert arg([1, 4, 64, 64], sag_scale=0.75) == (0.75, 1.0)  # 1024: the cap itself
    for keys in (dict(window=8), dict(region_masks=np.ones((1, 16, 16), np.float32), window=16), dict(cache_interval=2), dict(pag_scale=3.0),
                 dict(tome_ratio=0.5)):
        with pytest.raises(ValueError, match="sag.*out of scope"):
            arg(sag_scale=0.75, **keys)
    assert arg(sag_scale=0.75, cache_interval=1, pag_scale=0, tome_ratio=0.0, freeu=(1.1, 1.2, 0.9, 0.2)) == (0.75, 1.0)


def test_samplers_raise_before_anything_is_drawn(tiny_cpu):
    model = _NoDevice(tiny_cpu[0])
    state = torch.get_rng_state()
    for kind, s in _samplers(model).items():
        base = {"seeds": [1]} if kind == "sde" else {}
        run = lambda x_type="image", shape=(1, 4, 16, 16), **keys: s.sample(
            steps=5, shape=list(shape), x_info=dict({"type": x_type}, **dict(base, **keys)), c_info=dict(C_INFO), verbose=False)
        multi = lambda **keys: s.sample_multicontext(steps=5, shape=[1, 4, 16, 16], x_info=dict({"type": "image"}, **dict(base, **keys)),
                                                     c_info_list=[dict(C_INFO)], verbose=False)
        for bad in BAD_SCALES:
            with pytest.raises(ValueError, match="sag"):
                run(sag_scale=bad)
            with pytest.raises(ValueError, match="sag"):
                multi(sag_scale=bad)
        for bad in BAD_SIGMAS:
            with pytest.raises(ValueError, match="sag"):
                run(sag_scale=0.75, sag_blur_sigma=bad)
        with pytest.raises(ValueError, match="sag"):
            run("text", (1, 128), sag_scale=0.75)
        with pytest.raises(ValueError, match="sag"):
            run(shape=(1, 4, 4, 8), sag_scale=0.75)
        with pytest.raises(ValueError, match="sag.*1024"):
            run(shape=(1, 4, 64, 80), sag_scale=0.75)
        for keys in (dict(window=8), dict(window=16, region_masks=np.ones((1, 16, 16), np.float32)), dict(cache_interval=2),
                     dict(pag_scale=3.0), dict(tome_ratio=0.5)):
            with pytest.raises(ValueError, match="sag.*out of scope"):
                run(sag_scale=0.75, **keys)
        for good in (dict(sag_scale=0.75), dict(sag_scale=0), dict(sag_scale=None, sag_blur_sigma=-1), dict(sag_scale=1, sag_blur_sigma=2.0),
                     dict(sag_scale=0.75, freeu=(1.1, 1.2, 0.9, 0.2))):
            with pytest.raises(AssertionError, match="touched the device"):
                run(**good)
    assert torch.equal(torch.get_rng_state(), state)        # nothing was drawn from the (host) generator on the way


def test_p_sample_ddim_validates_the_keys(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(_NoDevice(tiny_cpu[0]))
    c_info = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_guidance_scale": 1.0}
    for keys in (dict(sag_scale=-1), dict(sag_scale=0.75, sag_blur_sigma=0), dict(sag_scale=0.75, pag_scale=3.0)):
        x_info = dict({"type": "image", "x": torch.zeros(1, 4, 16, 16)}, **keys)
        with pytest.raises(ValueError, match="sag"):
            s.p_sample_ddim(x_info, c_info, torch.tensor([1]), 0)
        with pytest.raises(ValueError, match="sag"):
            s.p_sample_ddim_multicontext(x_info, [c_info], torch.tensor([1]), 0)
    with pytest.raises(ValueError, match="sag"):
        s.p_sample_ddim({"type": "image", "x": torch.zeros(1, 4, 4, 4), "sag_scale": 0.75}, c_info, torch.tensor([1]), 0)


def test_forward_key_is_validated_without_a_device(tiny_cpu):
    from lib.model_zoo.vd import _sag_fwd_arg
    x = torch.zeros(2, 4, 16, 16)
    assert _sag_fwd_arg({"type": "image", "x": x}, 1) is None
    good = torch.zeros(2, 2, 64)
    assert _sag_fwd_arg({"type": "image", "x": x, "sag": good}, 2) is good
    for bad, T in ((good, 1), (good.half(), 2), (good.transpose(0, 1), 2), (torch.zeros(2, 3, 64), 2), (torch.zeros(2, 64), 2), ("m", 1)):
        with pytest.raises(ValueError, match="sag"):
            _sag_fwd_arg({"type": "image", "x": x, "sag": bad}, T)
    with pytest.raises(ValueError, match="sag.*image"):
        _sag_fwd_arg({"type": "text", "x": x, "sag": good}, 2)


def test_kv_rows_slices_without_projecting():
    from lib.model_zoo import vd

    class Block(object):
        def project_context(self, c):
            raise AssertionError("projected again")

    mod = [Block()]
    kv = torch.arange(24.0).view(4, 3, 2)
    cache = {id(mod): kv, vd._KV_MODULES: {id(mod): mod}}
    rows = vd.kv_rows(cache, 2)
    assert vd.kv_lookup(rows, mod, None).data_ptr() == kv.data_ptr() and tuple(vd.kv_lookup(rows, mod, None).shape) == (2, 3, 2)
    assert vd.kv_rows(None, 2) is None and vd.kv_refreshable(rows)
    vd.kv_mark_stale(cache)
    assert id(mod) not in vd.kv_rows(cache, 2)               # a stale entry is not handed on


def test_graph_key_tells_on_from_off_but_not_scales_or_sigmas(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(tiny_cpu[0])
    x = torch.zeros(1, 4, 16, 16)
    cis = [dict(C_INFO, c=torch.zeros(2, 7, 128))]
    key = lambda **kw: s._static_key(x, dict({"type": "image"}, **kw), cis, True, True)
    base = key()
    assert key(sag_scale=None) == base and key(sag_scale=0) == base and key(sag_scale=0.0, sag_blur_sigma=3.0) == base
    on = key(sag_scale=0.75)
    assert on != base and on[:len(base)] == base and len(on) == len(base) + 1
    assert key(sag_scale=2.0, sag_blur_sigma=2.0) == on


def test_entries_are_declared_and_ops_refuse_without_a_device():
    import os
    from vd_hip import loader, ops
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "vd_hip.h")).read()
    for name, nargs in (("vd_sag_mass_f16", 13), ("vd_sag_degrade_f16", 15), ("vd_sag_fold_f16", 5)):
        assert ("int %s(" % name) in header and len(loader.PROTOTYPES[name][1]) == nargs
    build = open(os.path.join(here, "..", "versatile-diffusion_amd", "build.py")).read()
    assert '"sag.hip"' in build
    z = torch.zeros(1, 64, 80, dtype=torch.float16)
    with pytest.raises(ops.VdHipError):
        ops.sag_mass(z, z, 2)
    with pytest.raises(ops.VdHipError):
        ops.sag_fold(torch.zeros(2, 8, dtype=torch.float16), torch.zeros(1, 8, dtype=torch.float16), torch.zeros(1))
    with pytest.raises(ops.VdHipError):
        ops.sag_degrade(torch.zeros(1, 4, 8, 8, dtype=torch.float16), torch.zeros(1, 4, 8, 8, dtype=torch.float16), torch.zeros(1, 1, 4),
                        torch.ones(1), torch.ones(9), torch.ones(3), 2, 2)


# ---- 3. the preconditions of the GPU cases ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sc.MASS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mass_cases_hold_their_preconditions(shape):
    B, H, N, D = shape
    q, k, ref, counts = sc.mass_case(shape, "selector")
    _, P, logits = ac.softmax_attention(q, k, k, H, False)
    top2 = logits.topk(2, -1).values
    assert float((top2[..., 0] - top2[..., 1]).min()) >= 32.0 and float(logits.abs().max()) <= 80.0     # the selector lead
    assert np.array_equal(P.argmax(-1).numpy().reshape(B, H, N) >= 0, np.ones((B, H, N), bool))
    won = np.stack([[np.bincount(P[b, h].argmax(-1).numpy(), minlength=N) for h in range(H)] for b in range(B)])
    assert np.array_equal(won, counts) and counts.max() > 1 and (counts == 0).any()
    assert np.abs(ref.numpy() - counts.mean(1)).max() <= N * np.exp(-32.0)
    # a sum over keys instead of queries gives 1 everywhere; another head's or sample's counts differ by >= 1 / H somewhere
    assert np.abs(counts.mean(1) - 1.0).max() >= 1.0 / H
    if H > 1:
        assert np.abs(counts[:, 0] - counts[:, 1]).max() >= 1
    if B > 1:
        assert np.abs(counts[0] - counts[1]).max() >= 1
    q, k, ref, _ = sc.mass_case(shape, "random")
    assert float(ac.softmax_attention(q, k, k, H, False)[2].abs().max()) <= 8.0                          # the score bound
    assert float(ref.min()) > 0 and abs(float(ref.sum(1).mean()) - N) < 1e-9 * N
    q, k, ref, _ = sc.mass_case(shape, "uniform")
    assert not bool(q.any()) and float((ref - 1.0).abs().max()) < 1e-12


def test_degrade_cases_hold_their_preconditions():
    up = sc.DEGRADE_MASSES[3]
    assert up > np.float32(1.0) and up - np.float32(1.0) == np.float32(2.0 ** -23)
    for ratio in sc.DEGRADE_RATIOS:
        r = np.float32(ratio)
        assert float(r.astype(np.float64).sum()) == 1.0
        # every combination of the drawn masses: the fma chain of the oracle is the exact rational sum rounded once per fma (the
        # float64 product and sum it is formed from are exact), so the device's fp32 fmas must give these very values; a combined
        # mass of exactly 1.0 and values on both sides of it occur
        from fractions import Fraction
        grid = np.stack(np.meshgrid(*[sc.DEGRADE_MASSES] * len(ratio), indexing="ij"), 0).reshape(len(ratio), 1, -1)
        got = sc.combined_mass(grid, r)
        for j in range(grid.shape[2]):
            m = Fraction(0)
            for t in range(len(ratio)):
                m = Fraction(float(np.float32(float(Fraction(float(r[t])) * Fraction(float(grid[t, 0, j])) + m))))
                assert Fraction(float(np.float64(r[t]) * np.float64(grid[t, 0, j]))) == Fraction(float(r[t])) * Fraction(float(grid[t, 0, j]))
            assert Fraction(float(got[0, j])) == m
        assert (got == 1).any() and (got > 1).any() and (got < 1).any()
    for shape in sc.DEGRADE_SHAPES:
        B, C, H, W, Hm, Wm = shape
        assert H >= 5 and W >= 5
        x, eps, mass = sc.degrade_case(shape, 2, 1.0)
        ref, A, Mpx = sc.degrade_ref64(x, eps, mass, (0.5, 0.5), 1.0, sc.DEGRADE_ALPHA, Hm, Wm)
        assert (A >= np.abs(ref) - 1e-12).all() and Mpx.shape == (B, H, W)
    assert min(sc.DEGRADE_REFUSED[2:4]) < 5


@pytest.mark.parametrize("scale", sc.LOOP_SCALES)
@pytest.mark.parametrize("kind", sc.LOOP_KINDS)
def test_loop_precondition_no_oracle_mass_within_the_margin_of_one(tiny_cpu, kind, scale):
    net, sd, plan = tiny_cpu
    s = _samplers(net)[kind]
    if kind == "sde":
        s._eta, s._s_noise = s.eta, 1.0
    s.make_schedule(STEPS, ddim_eta=s.eta if kind == "sde" else 0., verbose=False)
    margin = []
    xT = sc.loop_inputs((kind, scale))[0]
    on = sc.oracle_loop(sd, plan, s, kind, xT, [sc.loop_context((kind, scale), scale)], scale, SAG_SCALE, margin=margin,
                        noise=sc.sde_noise() if kind == "sde" else None)
    print("%s s %.1f: least |mass - 1| per step %s (margin %.1e)" % (kind, scale, ["%.2e" % m for m in margin], sc.MASS_MARGIN))
    assert len(margin) == STEPS and min(margin) >= sc.MASS_MARGIN and bool(torch.isfinite(on).all())


@pytest.mark.parametrize("combo", ["rescale", "inpaint", "freeu"])
def test_combination_precondition_no_oracle_mass_within_the_margin_of_one(tiny_cpu, combo):
    from freeu_cases import SETTING
    net, sd, plan = tiny_cpu
    kind = "ddim" if combo == "rescale" else "2m"
    s = _samplers(net)[kind]
    s.make_schedule(STEPS, verbose=False)
    x0, mask = sc.loop_inpaint()
    xT = sc.loop_inputs(combo)[0]
    kw = {"rescale": dict(phi=0.7), "inpaint": dict(inpaint=(x0, mask, xT)), "freeu": dict(setting=SETTING)}[combo]
    margin = []
    sc.oracle_loop(sd, plan, s, kind, xT, [sc.loop_context(combo, 7.5)], 7.5, SAG_SCALE, margin=margin, **kw)
    print("%s: least |mass - 1| per step %s" % (combo, ["%.2e" % m for m in margin]))
    assert min(margin) >= sc.MASS_MARGIN
