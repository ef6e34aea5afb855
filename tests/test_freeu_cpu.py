"""FreeU on the host: the seven-sum formula of the contract against the torch.fft definition, the trig tables, the stage rule at
full width and on the tiny model, the restated walk (tests/freeu_cases.py) against the oracle's plain forward, the validation of
x_info['freeu'] at model and sampler level, the step graph's key and the sharding helper's forwarding.  No GPU needed."""
import math

import numpy as np
import pytest
import torch

import deepcache_cases as dc
import freeu_cases as fc
from vdtest_util import meta, synth_into, tiny_vd_cfg

FULL_ARGS = dict(model_channels=320, channel_mult=[1, 2, 4, 4], num_res_blocks=[2, 2, 2, 2])


@pytest.fixture(scope="module")
def tiny_cpu():
    """The tiny product model on the CPU (never run) and its fp32 weights."""
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    return net, synth_into(net, m["seed"])


# ---- 1. the definition -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(2, 2), (4, 4), (5, 7), (8, 8), (16, 32)])
@pytest.mark.parametrize("s", [0.0, 0.2, 0.9, 2.0])
def test_seven_sums_equal_the_fft_definition(H, W, s):
    x = torch.randn((2, 3, H, W), generator=torch.Generator().manual_seed(100 * H + W), dtype=torch.float64)
    ref = fc.fourier_filter(x, 1, s)
    got = fc.seven_sums(x, s)
    err = (got - ref).abs().max().item()
    print("%d x %d s %.1f: seven sums vs torch.fft max abs %.3e" % (H, W, s, err))
    assert err <= 1e-12
    assert torch.equal(fc.fourier_filter(x, 1, 1.0), torch.fft.ifftn(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1)).real)


def test_seven_sums_with_the_fp32_tables():
    """The same formula fed the library's tables (float64 arithmetic on the fp32 table values): within the tables' rounding."""
    from vd_hip import ops
    for H, W in [(2, 2), (4, 4), (5, 7), (8, 8), (16, 32), (6, 10), (8, 24)]:
        x = torch.randn((1, 2, H, W), generator=torch.Generator().manual_seed(H + W), dtype=torch.float64)
        cy, sy, cx, sx, cxy, sxy = [torch.from_numpy(t).double() for t in ops.freeu_tables_host(H, W)]
        planes = [torch.ones(H, W, dtype=torch.float64), cy[:, None].expand(H, W), sy[:, None].expand(H, W),
                  cx[None, :].expand(H, W), sx[None, :].expand(H, W), cxy.view(H, W), sxy.view(H, W)]
        acc = sum((x * t).sum((-2, -1), keepdim=True) * t for t in planes)
        got = x + (0.2 - 1.0) / (H * W) * acc
        assert (got - fc.fourier_filter(x, 1, 0.2)).abs().max().item() <= 7 * 2.0 ** -23 * x.abs().sum((-2, -1)).max().item() / (H * W) * 2


def test_tables_are_exact_at_quarter_turns_and_once_rounded_elsewhere():
    from vd_hip import ops
    for H, W in [(2, 2), (4, 4), (2, 4), (8, 8), (16, 32), (5, 7), (6, 10), (12, 20), (64, 64)]:
        tabs = ops.freeu_tables_host(H, W)
        assert [t.shape for t in tabs] == [(H,), (H,), (W,), (W,), (H * W,), (H * W,)] and all(t.dtype == np.float32 for t in tabs)
        turns = ([(p, H) for p in range(H)], [(q, W) for q in range(W)], [(p * W + q * H, H * W) for p in range(H) for q in range(W)])
        for (c, s), kn in zip((tabs[0:2], tabs[2:4], tabs[4:6]), turns):
            for i, (k, n) in enumerate(kn):
                k %= n
                if (4 * k) % n == 0:
                    want = [(1, 0), (0, 1), (-1, 0), (0, -1)][4 * k // n]
                    assert (float(c[i]), float(s[i])) == (float(want[0]), float(want[1])), (H, W, i)
                else:
                    a = 2 * math.pi * k / n
                    assert c[i] == np.float32(math.cos(a)) and s[i] == np.float32(math.sin(a)), (H, W, i)
    # the xy table is the angle sum: cos(tp + fq) with tp + fq = 2 pi (p W + q H) / (H W)
    cy, sy, cx, sx, cxy, sxy = [t.astype(np.float64) for t in ops.freeu_tables_host(6, 10)]
    assert np.abs(cxy.reshape(6, 10) - (cy[:, None] * cx[None, :] - sy[:, None] * sx[None, :])).max() < 3e-7
    assert np.abs(sxy.reshape(6, 10) - (sy[:, None] * cx[None, :] + cy[:, None] * sx[None, :])).max() < 3e-7
    for bad in [(1, 8), (8, 1), (0, 0)]:
        with pytest.raises(ValueError):
            ops.freeu_tables_host(*bad)


# ---- 2. the stage rule --------------------------------------------------------------------------------------------------------

def test_stage_rule_full_width_and_tiny(tiny_cpu):
    from lib.cfg_helper import model_cfg_bank
    from lib.model_zoo.vd import freeu_entering_widths, freeu_stages
    from oracle import vd_oracle as O
    args = model_cfg_bank()("openai_unet_2d_v1").args
    full = {k: args[k] for k in ("model_channels", "channel_mult", "num_res_blocks")}
    assert {k: (list(v) if isinstance(v, (list, tuple)) else [v] * 4 if k == "num_res_blocks" else v) for k, v in full.items()} == FULL_ARGS
    assert freeu_stages(dict(full)) == fc.FULL_STAGES
    assert freeu_entering_widths(**FULL_ARGS) == [1280] * 7 + [640] * 3 + [320] * 2
    assert fc.stage_blocks(O.unet_plan()) == fc.FULL_STAGES                     # the oracle's own plan says the same
    net = tiny_cpu[0]
    assert freeu_stages(net.diffuser["image"]) == fc.TINY_STAGES
    assert fc.stage_blocks(O.unet_plan(**meta()["unet2d"])) == fc.TINY_STAGES
    # the modules agree: the ResBlock behind every load takes entering width + skip width
    unet = net.diffuser["image"]
    order = list(unet.i_order) + list(unet.m_order) + list(unet.o_order)
    di, prev, widths, stack, expect = 0, None, [], [], None
    for s in order:
        if s == "d":
            blk = list(unet.data_blocks[di])
            if expect is not None:
                assert blk[0].channels == expect, di
                expect = None
            prev = getattr(blk[-1], "out_channels", prev)
            di += 1
        elif s == "save_hidden_feature":
            stack.append(prev)
        elif s == "load_hidden_feature":
            widths.append(prev)
            expect = prev + stack.pop()
    assert widths ==freeu_entering_widths(unet.model_channels, unet.channel_mult, unet.num_res_blocks) == [128, 128, 128, 64]
    with pytest.raises(ValueError, match="2-D"):
        freeu_stages(net.diffuser["text"])


def test_restated_walk_records_the_stages_and_off_is_the_oracle_forward(tiny_cpu):
    from oracle import vd_oracle as O
    _, sd = tiny_cpu
    plan = O.unet_plan(**meta()["unet2d"])
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 4, 16, 16), generator=g)
    ctx = [("text", torch.randn((2, 77, 128), generator=g) * 0.5, 1.0)]
    t = torch.full((2,), 500, dtype=torch.long)
    rec = []
    on = fc.walk(sd, plan, x, t, ctx, fc.SETTING, record=rec)
    assert rec == [(0, 1), (1, 1), (2, 1), (3, 2)]
    plain = dc.walk(sd, plan, x, t, ctx)
    assert torch.equal(fc.walk(sd, plan, x, t, ctx, None), plain)
    assert torch.equal(fc.walk(sd, plan, x, t, ctx, (1.0, 1.0, 1.0, 1.0)), plain) or \
        ((fc.walk(sd, plan, x, t, ctx, (1.0, 1.0, 1.0, 1.0)) - plain).norm() / plain.norm()).item() < 1e-6   # (fft round trip)
    gap = ((on - plain).norm() / plain.norm()).item()
    print("tiny oracle forward, FreeU %r vs off: rel-L2 %.3e" % (fc.SETTING, gap))
    assert gap >= 10 * fc.FWD_TOL


# ---- 3. validation ------------------------------------------------------------------------------------------------------------

BAD = [True, 1.2, "1.2, 1.4, 0.9, 0.2", (1.2, 1.4, 0.9), (1.2, 1.4, 0.9, 0.2, 1.0), (1.2, 1.4, 0.9, True), (1.2, 1.4, 0.9, "0.2"),
       (1.2, 1.4, float("nan"), 0.2), (float("inf"), 1.4, 0.9, 0.2), (1.2, None, 0.9, 0.2), (1.2, 1.4, 0.9, 1j),
       {"b1": 1.2, "b2": 1.4, "s1": 0.9}, {"b1": 1.2, "b2": 1.4, "s1": 0.9, "s2": 0.2, "s3": 1.0}, {"b1": 1.2, "b2": 1.4, "s1": 0.9, "s2": False},
       {"b1": 1.2, "b2": 1.4, "s1": 0.9, "t2": 0.2}]


def test_setting_values():
    from lib.model_zoo.vd import freeu_setting
    assert freeu_setting(None) is None
    assert freeu_setting((1, 1.0, 1, 1.0)) is None and freeu_setting({"b1": 1, "b2": 1, "s1": 1, "s2": 1}) is None
    assert freeu_setting([1.2, 1.4, 0.9, 0.2]) == (1.2, 1.4, 0.9, 0.2)
    assert freeu_setting({"s2": 0.2, "b1": 1.2, "s1": 0.9, "b2": 1.4}) == (1.2, 1.4, 0.9, 0.2)
    assert freeu_setting((np.float32(1.5), 2, np.int64(0), 0.5)) == (1.5, 2.0, 0.0, 0.5)
    assert freeu_setting((1.0, 1.0, 1.0, 0.5)) == (1.0, 1.0, 1.0, 0.5)
    for bad in BAD:
        with pytest.raises(ValueError, match="freeu"):
            freeu_setting(bad)


def test_model_level_key_is_validated(tiny_cpu):
    net = tiny_cpu[0]
    c_info = {"type": "text", "c": torch.zeros(1, 7, 128)}
    t = torch.zeros(1, dtype=torch.long)
    with pytest.raises(ValueError, match="image"):
        net.apply_model({"type": "text", "x": torch.zeros(1, 128), "freeu": fc.SETTING}, t, c_info)
    with pytest.raises(ValueError, match="image"):
        net.apply_model_multicontext({"type": "text", "x": torch.zeros(1, 128), "freeu": (1, 1, 1, 1)}, t, [dict(c_info, ratio=1.0)])
    for bad in BAD:
        with pytest.raises(ValueError, match="freeu"):
            net.apply_model({"type": "image", "x": torch.zeros(1, 4, 16, 16), "freeu": bad}, t, c_info)
        with pytest.raises(ValueError, match="freeu"):
            net.apply_model_multicontext({"type": "image", "x": torch.zeros(1, 4, 16, 16), "freeu": bad}, t, [dict(c_info, ratio=1.0)])


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


def test_samplers_validate_before_device_work(tiny_cpu):
    model = _NoDevice(tiny_cpu[0])
    c_info = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_conditioning": torch.zeros(1, 7, 128),
              "unconditional_guidance_scale": 7.5}
    for s in _samplers(model):
        run = lambda **keys: s.sample(steps=5, shape=[1, 4, 16, 16], x_info=dict({"type": "image"}, **keys), c_info=dict(c_info),
                                      verbose=False)
        for bad in BAD:
            with pytest.raises(ValueError, match="freeu"):
                run(freeu=bad)
            with pytest.raises(ValueError, match="freeu"):
                s.sample_multicontext(steps=5, shape=[1, 4, 16, 16], x_info={"type": "image", "freeu": bad}, c_info_list=[dict(c_info)],
                                      verbose=False)
        with pytest.raises(ValueError, match="image"):
            s.sample(steps=5, shape=[1, 128], x_info={"type": "text", "freeu": fc.SETTING}, c_info=dict(c_info), verbose=False)
        for good in (fc.SETTING, dict(zip(("b1", "b2", "s1", "s2"), fc.SETTING)), None, (1, 1, 1, 1)):
            with pytest.raises(AssertionError, match="touched the device"):
                run(freeu=good)


def test_p_sample_ddim_validates_the_key(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(_NoDevice(tiny_cpu[0]))
    c_info = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_guidance_scale": 1.0}
    for bad in BAD[:4]:
        x_info = {"type": "image", "x": torch.zeros(1, 4, 16, 16), "freeu": bad}
        with pytest.raises(ValueError, match="freeu"):
            s.p_sample_ddim(x_info, c_info, torch.tensor([1]), 0)
        with pytest.raises(ValueError, match="freeu"):
            s.p_sample_ddim_multicontext(x_info, [c_info], torch.tensor([1]), 0)


# ---- 4. the graph key, the sharding helper, the C ABI listing -----------------------------------------------------------------------

def test_graph_key_differs_between_on_and_off(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(tiny_cpu[0])
    x = torch.zeros(1, 4, 16, 16)
    cis = [{"type": "text", "c": torch.zeros(2, 7, 128)}]
    key = lambda **kw: s._static_key(x, dict({"type": "image"}, **kw), cis, True, True)
    off = key()
    assert key(freeu=None) == off and key(freeu=(1, 1, 1, 1)) == off and key(freeu={"b1": 1, "b2": 1, "s1": 1, "s2": 1}) == off
    on = key(freeu=fc.SETTING)
    assert on != off and on[:-1] == off[:-1] and on[-1] == fc.SETTING and off[-1] is None
    assert key(freeu=dict(zip(("b1", "b2", "s1", "s2"), fc.SETTING))) == on
    assert key(freeu=(1.2, 1.4, 0.9, 0.3)) != on and key(freeu=(1.0, 1.0, 1.0, 0.2)) not in (on, off)


def test_sharding_helper_forwards_the_key():
    from lib.model_zoo import sharded
    seen = []

    class Net(object):
        device = "cpu"

        def vae_decode(self, z, which):
            return z

    class Sampler(object):
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=False):
            seen.append(x_info.get("freeu", "absent"))
            return x_info["xt"], {}

    ctx = lambda: {"type": "text", "conditioning": torch.zeros(2, 7, 16), "unconditional_conditioning": torch.zeros(2, 7, 16)}
    sharded.vd_sample_sharded(Net(), Sampler(), 6, [2, 4, 8, 8], [ctx()], seed=3)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, [2, 4, 8, 8], [ctx()], seed=3, freeu=fc.SETTING)
    assert seen == ["absent", fc.SETTING]


def test_entry_point_is_declared_and_refuses_bad_arguments_without_a_device():
    import ctypes
    import os
    import re
    from vd_hip.loader import PROTOTYPES, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "vd_hip.h")).read()
    assert re.search(r"\bint vd_freeu_f16\(", hdr) and "vd_freeu_f16" in PROTOTYPES
    assert "freeu.hip" in open(os.path.join(root, "versatile-diffusion_amd", "build.py")).read()
    L = lib()
    P = ctypes.c_void_p
    ok = dict(h=P(4096), skip=P(8192), ho=P(12288), so=P(16384), B=1, H=4, W=4, C0=16, C1=8, b=1.2, s=0.5)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vd_freeu_f16(a["h"], a["skip"], a["ho"], a["so"], P(64), P(64), P(64), P(64), P(64), P(64), a["B"], a["H"], a["W"],
                              a["C0"], a["C1"], a["b"], a["s"], None)

    for kw in (dict(h=None), dict(so=None), dict(B=0), dict(H=1), dict(W=1), dict(C0=12), dict(C1=4), dict(C1=0), dict(h=P(4100)),
               dict(so=P(16392)), dict(ho=P(4096)), dict(so=P(8192)), dict(b=float("nan")), dict(s=float("inf"))):
        assert call(**kw) < 0 and L.vd_last_error().decode().startswith("vd_freeu_f16"), kw
