"""Perturbed-attention guidance on the host: the validation of x_info['pag_scale'] / ['pag_layers'] at sampler level and of the
forward key x_info['pag'] at model level (nothing is drawn and no device is touched before a raise), the replica layout of
_cfg_contexts, the fold's host weight, the step graph's key, the sharding helper's forwarding, the C ABI listing with the two
entries' refusals, and the oracle preconditions of tests/pag_cases.py: that the project's bounds tell PAG on from off.  No GPU."""
import numpy as np
import pytest
import torch

import deepcache_cases as dc
import pag_cases as pc
from pag_cases import FWD_TOL, LATENT_TOL
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
BAD_LAYERS = [[], (), (2, 2), (7,), (-1,), (0, 7), (1.0,), (True,), "all", "2", 2, ("mid",), [None]]


# ---- 1. the keys -------------------------------------------------------------------------------------------------------------

def test_walk_indices_of_the_tiny_and_the_full_net(tiny_cpu):
    from lib.model_zoo import vd
    assert vd.pag_context_blocks(tiny_cpu[0].diffuser["image"]) == (pc.TINY_BLOCKS, pc.TINY_MID)

    class Full(object):        # the full-width orders: 2 blocks per level with a context block each on three levels, the middle, 9 output
        i_order = ["d"] + ["d", "c", "save_hidden_feature"] * 2 + ["d", "save_hidden_feature"] + (["d", "c", "save_hidden_feature"] * 2 + ["d", "save_hidden_feature"]) * 2 + ["d", "save_hidden_feature"] * 2
        m_order = ["d", "c", "d"]
        o_order = ["load_hidden_feature", "d"] * 3 + ["load_hidden_feature", "d", "c"] * 9

    assert vd.pag_context_blocks(Full()) == (pc.FULL_BLOCKS, pc.FULL_MID)
    assert vd.pag_layers("mid", Full()) == vd.pag_layers(None, Full()) == (6,)
    assert vd.pag_layers([15, 0, 6], Full()) == (0, 6, 15)
    with pytest.raises(ValueError, match="pag"):
        vd.pag_layers([16], Full())
    with pytest.raises(ValueError, match="pag"):
        vd.pag_context_blocks(tiny_cpu[0].diffuser["text"])


def test_sampler_keys_are_validated_and_normalised(tiny_cpu):
    from lib.model_zoo.vd import _pag_arg
    net = tiny_cpu[0]
    arg = lambda **kw: _pag_arg(dict({"type": "image"}, **kw), net)
    assert arg() is None and arg(pag_scale=None) is None and arg(pag_scale=0) is None and arg(pag_scale=0.0) is None
    for bad in BAD_LAYERS:                                   # ignored when PAG is off
        assert arg(pag_scale=0, pag_layers=bad) is None and arg(pag_layers=bad) is None
    assert arg(pag_scale=3) == (3.0, (2,)) and arg(pag_scale=np.float32(0.5), pag_layers="mid") == (0.5, (2,))
    assert arg(pag_scale=3.0, pag_layers=[3, 1, 2]) == (3.0, (1, 2, 3)) and arg(pag_scale=3.0, pag_layers=(0,)) == (3.0, (0,))
    assert arg(pag_scale=3.0, pag_layers=np.array([6, 0])) == (3.0, (0, 6)) and arg(pag_scale=3.0, pag_layers=range(7))[1] == tuple(range(7))
    assert arg(pag_scale=3.0, pag_layers=iter([4])) == (3.0, (4,))
    for bad in BAD_SCALES:
        with pytest.raises(ValueError, match="pag"):
            arg(pag_scale=bad)
    for bad in BAD_LAYERS:
        with pytest.raises(ValueError, match="pag"):
            arg(pag_scale=3.0, pag_layers=bad)
    with pytest.raises(ValueError, match="pag.*image"):
        _pag_arg({"type": "text", "pag_scale": 3.0}, net)
    with pytest.raises(ValueError, match="pag.*cache_interval.*out of scope"):
        arg(pag_scale=3.0, cache_interval=2)
    with pytest.raises(ValueError, match="pag.*region_masks.*out of scope"):
        arg(pag_scale=3.0, region_masks=np.ones((1, 16, 16), np.float32), window=16)
    assert arg(pag_scale=3.0, cache_interval=1, cache_depth=2) == (3.0, (2,))


def test_samplers_raise_before_anything_is_drawn(tiny_cpu):
    model = _NoDevice(tiny_cpu[0])
    state = torch.get_rng_state()
    for s in _samplers(model):
        run = lambda x_type="image", shape=(1, 4, 16, 16), **keys: s.sample(
            steps=5, shape=list(shape), x_info=dict({"type": x_type}, **keys), c_info=dict(C_INFO), verbose=False)
        multi = lambda **keys: s.sample_multicontext(steps=5, shape=[1, 4, 16, 16], x_info=dict({"type": "image"}, **keys),
                                                     c_info_list=[dict(C_INFO)], verbose=False)
        for bad in BAD_SCALES:
            with pytest.raises(ValueError, match="pag"):
                run(pag_scale=bad)
            with pytest.raises(ValueError, match="pag"):
                multi(pag_scale=bad)
        for bad in BAD_LAYERS:
            with pytest.raises(ValueError, match="pag"):
                run(pag_scale=3.0, pag_layers=bad)
        with pytest.raises(ValueError, match="pag"):
            run("text", (1, 128), pag_scale=3.0)
        with pytest.raises(ValueError, match="out of scope"):
            run(pag_scale=3.0, cache_interval=2)
        with pytest.raises(ValueError, match="out of scope"):
            run(pag_scale=3.0, window=16, region_masks=np.ones((1, 16, 16), np.float32))
        with pytest.raises(ValueError, match="out of scope"):
            multi(pag_scale=3.0, cache_interval=3, cache_depth=2)
        for good in (dict(pag_scale=3.0), dict(pag_scale=0), dict(pag_scale=None, pag_layers=[]), dict(pag_scale=1, pag_layers=(0, 6)),
                     dict(pag_scale=3.0, window=8)):
            with pytest.raises(AssertionError, match="touched the device"):
                run(**good)
    assert torch.equal(torch.get_rng_state(), state)        # nothing was drawn from the (host) generator on the way


def test_p_sample_ddim_validates_the_keys(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(_NoDevice(tiny_cpu[0]))
    c_info = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_guidance_scale": 1.0}
    for keys in (dict(pag_scale=-1), dict(pag_scale=3.0, pag_layers=[9]), dict(pag_scale=3.0, pag_layers=[])):
        x_info = dict({"type": "image", "x": torch.zeros(1, 4, 16, 16)}, **keys)
        with pytest.raises(ValueError, match="pag"):
            s.p_sample_ddim(x_info, c_info, torch.tensor([1]), 0)
        with pytest.raises(ValueError, match="pag"):
            s.p_sample_ddim_multicontext(x_info, [c_info], torch.tensor([1]), 0)


def test_forward_key_is_validated(tiny_cpu):
    net = tiny_cpu[0]
    c_info = {"type": "text", "c": torch.zeros(3, 7, 128)}
    t = torch.zeros(3, dtype=torch.long)
    x = torch.zeros(1, 4, 16, 16)
    with pytest.raises(ValueError, match="image"):
        net.apply_model({"type": "text", "x": torch.zeros(1, 128), "pag": ((2,), 1)}, t, c_info)
    for bad in (3, (2,), ((2,), 1, 0), ((2,), -1), ((2,), 1.0), ((2,), True), ((7,), 1), ((), 1), ((2, 2), 1), ("all", 1)):
        with pytest.raises(ValueError, match="pag"):
            net.apply_model({"type": "image", "x": x, "repeat": 3, "pag": bad}, t, c_info)
        with pytest.raises(ValueError, match="pag"):
            net.apply_model_multicontext({"type": "image", "x": x, "repeat": 3, "pag": bad}, t, [dict(c_info, ratio=1.0)])


# ---- 2. the replica layout and the fold's weight ---------------------------------------------------------------------------------

def test_cfg_contexts_row_layout_for_one_two_and_three_replicas(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler, replica_count
    net = tiny_cpu[0]
    net.device = "cpu"
    s = DDIMSampler(net)
    c = torch.arange(2 * 3 * 4, dtype=torch.float32).view(2, 3, 4)
    u = -c - 1
    ci = lambda scale: [{"type": "text", "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale}]
    assert [replica_count(g, p) for g in (False, True) for p in (False, True)] == [1, 2, 2, 3]
    rows = lambda scale, slots, pag: s._cfg_contexts(ci(scale), slots, pag)[0][0]["c"]
    assert torch.equal(rows(1.0, 1, False), c) and torch.equal(s._cfg_contexts(ci(1.0))[0][0]["c"], c)
    assert torch.equal(rows(7.5, 1, False), torch.cat([u, c])) and torch.equal(s._cfg_contexts(ci(7.5), 1)[0][0]["c"], torch.cat([u, c]))
    assert torch.equal(rows(1.0, 1, True), torch.cat([c, c]))                     # [cond ; perturbed]
    assert torch.equal(rows(7.5, 1, True), torch.cat([u, c, c]))                  # [uncond ; cond ; perturbed]
    ri = lambda t: t.repeat_interleave(3, 0)                                      # (replica, sample, window slot)
    assert torch.equal(rows(7.5, 3, True), torch.cat([ri(u), ri(c), ri(c)])) and torch.equal(rows(1.0, 3, True), torch.cat([ri(c), ri(c)]))
    assert torch.equal(rows(7.5, 3, False), torch.cat([ri(u), ri(c)]))
    copies, guided, scale, phi = s._cfg_contexts(ci(7.5), pag=True)
    assert guided and scale == 7.5 and phi == 0. and "c" not in ci(7.5)[0]


def test_fold_weight_against_float64():
    from lib.model_zoo.ddim import pag_weight
    for s, sp in [(7.5, 3.0), (2.0, 0.7), (1.5, 5.0), (12.0, 1e-3), (0.5, 3.0), (1.0 + 2.0 ** -20, 3.0)]:
        w = pag_weight(s, sp, True)
        assert isinstance(w, np.float32) and w == np.float32(-np.float64(sp) / (np.float64(s) - 1.0))
        # a' + s (c - a') with a' = a + w (c - p) is a + s (c - a) + s_pag (c - p):  (1 - s) w = s_pag, up to w's one rounding
        assert abs((1.0 - s) * float(w) - sp) <= 2.0 ** -24 * sp * 1.0000001
    for sp in (3.0, 0.1, 1e-3):
        w = pag_weight(1.0, sp, False)
        assert isinstance(w, np.float32) and w == np.float32(sp)
    # the fold's formula with that weight is the PAG formula: float64 on random operands
    g = torch.Generator().manual_seed(3)
    a, c, p = [torch.randn(1000, generator=g).double() for _ in range(3)]
    w = float(pag_weight(7.5, 3.0, True))
    a2 = a + w * (c - p)
    assert torch.allclose(a2 + 7.5 * (c - a2), a + 7.5 * (c - a) + 3.0 * (c - p), rtol=0, atol=1e-5)


# ---- 3. the graph key, the sharding helper, the C ABI listing -------------------------------------------------------------------

def test_graph_key_tells_on_from_off_and_layers_apart_but_not_scales(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(tiny_cpu[0])
    x = torch.zeros(1, 4, 16, 16)
    cis = [{"type": "text", "c": torch.zeros(3, 7, 128)}]
    key = lambda **kw: s._static_key(x, dict({"type": "image"}, **kw), cis, True, True)
    off = key()
    assert key(pag_scale=None) == off and key(pag_scale=0) == off and key(pag_scale=0.0, pag_layers=[5]) == off and key(pag_layers=[1]) == off
    on = key(pag_scale=3.0)
    assert on != off and on[-2] == (True, (2,)) and off[-2] == (False, None) and on[:-2] == off[:-2]
    assert key(pag_scale=0.5) == on and key(pag_scale=7, pag_layers="mid") == on and key(pag_scale=3.0, pag_layers=[2]) == on
    assert key(pag_scale=3.0, pag_layers=(1, 2, 3)) not in (on, off) and key(pag_scale=3.0, pag_layers=[3, 2, 1]) == key(pag_scale=1.0, pag_layers=(1, 2, 3))
    assert on[-1] is None and off[-1] is None                        # the last element still is the FreeU setting
    both = key(pag_scale=3.0, freeu=(1.2, 1.4, 0.9, 0.2))
    assert both[-1] == (1.2, 1.4, 0.9, 0.2) and both[:-1] == on[:-1]


def test_sharding_helper_forwards_the_keys():
    from lib.model_zoo import sharded
    seen = []

    class Net(object):
        device = "cpu"

        def vae_decode(self, z, which):
            return z

    class Sampler(object):
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=False):
            seen.append((x_info.get("pag_scale", "absent"), x_info.get("pag_layers", "absent")))
            return x_info["xt"], {}

    ctx = lambda: {"type": "text", "conditioning": torch.zeros(2, 7, 16), "unconditional_conditioning": torch.zeros(2, 7, 16)}
    sharded.vd_sample_sharded(Net(), Sampler(), 6, [2, 4, 8, 8], [ctx()], seed=3)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, [2, 4, 8, 8], [ctx()], seed=3, pag_scale=3.0)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, [2, 4, 8, 8], [ctx()], seed=3, pag_scale=2.0, pag_layers=(1, 2))
    assert seen == [("absent", "absent"), (3.0, "absent"), (2.0, (1, 2))]


def test_entries_are_declared_and_refuse_bad_arguments_without_a_device():
    import ctypes
    import os
    import re
    from vd_hip.loader import PROTOTYPES, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "vd_hip.h")).read()
    for name in ("vd_attention_ident_f16", "vd_pag_fold_f16"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in PROTOTYPES
    assert len(PROTOTYPES["vd_attention_ident_f16"][1]) == len(PROTOTYPES["vd_attention_f16"][1]) + 1
    assert "pag.hip" in open(os.path.join(root, "versatile-diffusion_amd", "build.py")).read()
    L = lib()
    assert L.vd_abi_version() == 8                  # the entries are additive
    P = ctypes.c_void_p
    ok = dict(q=P(4096), k=P(4096 + 128), v=P(4096 + 256), out=P(1 << 20), B=3, H=2, Nq=64, Nk=64, D=40, ldq=240, ldk=240, ldv=240,
              ldo=80, sq=64 * 240, sk=64 * 240, sv=64 * 240, so=64 * 80, causal=0, ident=1)

    def ident(**kw):
        a = dict(ok, **kw)
        return L.vd_attention_ident_f16(a["q"], a["k"], a["v"], a["out"], a["B"], a["H"], a["Nq"], a["Nk"], a["D"], a["ldq"], a["ldk"],
                                        a["ldv"], a["ldo"], a["sq"], a["sk"], a["sv"], a["so"], 0.125, a["causal"], a["ident"], None)

    for kw in (dict(q=None), dict(v=None), dict(out=None), dict(B=0), dict(H=0), dict(Nq=0), dict(Nk=96), dict(Nq=96), dict(causal=1),
               dict(causal=2), dict(ident=-1), dict(ident=4), dict(ldv=244), dict(ldo=84), dict(ldv=72), dict(ldo=40), dict(sv=64 * 240 + 4),
               dict(so=64 * 80 + 2), dict(v=P(4096 + 8)), dict(out=P((1 << 20) + 8)), dict(H=1, D=44), dict(ldq=244)):
        assert ident(**kw) < 0 and L.vd_last_error().decode().startswith("vd_attention_ident_f16"), kw

    okf = dict(eps=P(4096), n=24, reps=3, w=P(8192))
    fold = lambda **kw: (lambda a: L.vd_pag_fold_f16(a["eps"], a["n"], a["reps"], a["w"], None))(dict(okf, **kw))
    for kw in (dict(eps=None), dict(w=None), dict(n=0), dict(n=-8), dict(reps=1), dict(reps=4), dict(reps=0), dict(eps=P(4097)), dict(w=P(8194))):
        assert fold(**kw) < 0 and L.vd_last_error().decode().startswith("vd_pag_fold_f16"), kw


# ---- 4. the oracle's preconditions: the project's bounds tell PAG on from off ---------------------------------------------------------

@pytest.fixture(scope="module")
def gold():
    return load_gold("ddim_tiny.npz")


def _contexts(gold, scale):
    return [{"type": "text", "conditioning": torch.from_numpy(gold["c_text"]), "unconditional_conditioning": torch.from_numpy(gold["u_text"]),
             "unconditional_guidance_scale": scale}]


def test_oracle_walk_off_is_the_plain_walk_and_records_the_layers(tiny_cpu, plan, gold):
    sd = tiny_cpu[1]
    xT = torch.from_numpy(gold["xT"]).float()
    cs0 = dc.cfg_contexts(_contexts(gold, 7.5), True)
    t = torch.full((4,), 500, dtype=torch.long)
    plain = dc.walk(sd, plan, torch.cat([xT, xT]), t, cs0)
    assert torch.equal(pc.walk(sd, plan, torch.cat([xT, xT]), t, cs0), plain)
    assert torch.equal(pc.walk(sd, plan, torch.cat([xT, xT]), t, cs0, (1, 2, 3), torch.zeros(4, dtype=torch.bool)), plain)
    xin, cs, mask = pc.replicas(xT, cs0, True, True)
    assert xin.shape[0] == 6 and mask.tolist() == [False] * 4 + [True] * 2 and torch.equal(cs[0][1][4:], cs0[0][1][2:])
    rec = []
    e = pc.walk(sd, plan, xin, torch.full((6,), 500, dtype=torch.long), cs, (1, 2, 3), mask, record=rec)
    assert rec == [1, 2, 3]
    assert rel_l2(e[:4], plain) < 1e-5                       # the unperturbed replicas do not see the perturbed one
    assert pc.layers_of(plan, "mid") == (pc.TINY_MID,) and len([s for s in dc.flat_order(plan) if s == "c"]) == pc.TINY_BLOCKS


@pytest.mark.parametrize("layers,least", [("mid", 10 * FWD_TOL), ((1, 2, 3), 10 * FWD_TOL), ((0,), 10 * FWD_TOL)])
def test_forward_precondition_the_perturbed_replica_is_far_from_the_conditional(tiny_cpu, plan, gold, layers, least):
    sd = tiny_cpu[1]
    xT = torch.from_numpy(gold["xT"]).float()
    xin, cs, mask = pc.replicas(xT, dc.cfg_contexts(_contexts(gold, 7.5), True), True, True)
    e_u, e_c, e_p = pc.walk(sd, plan, xin, torch.full((6,), 500, dtype=torch.long), cs, pc.layers_of(plan, layers), mask).chunk(3)
    gap = rel_l2(e_p, e_c)
    print("layers %r: rel-L2 of e_p vs e_c at t = 500: %.3f" % (layers, gap))
    assert gap >= least and bool(torch.isfinite(e_p).all())


@pytest.mark.parametrize("scale,layers", [(7.5, "mid"), (7.5, (1, 2, 3)), (1.0, "mid"), (1.0, (0, 6))])
def test_loop_precondition_five_ddim_steps_on_vs_off(tiny_cpu, plan, gold, scale, layers):
    from lib.model_zoo.ddim import DDIMSampler
    net, sd = tiny_cpu
    xT = torch.from_numpy(gold["xT"]).float()
    s = DDIMSampler(net)
    s.make_schedule(5, verbose=False)
    on = pc.oracle_loop(sd, plan, s, "ddim", xT, _contexts(gold, scale), scale, pc.PAG_SCALE, layers)
    off = pc.oracle_loop(sd, plan, s, "ddim", xT, _contexts(gold, scale), scale, 0.0)
    assert torch.equal(off, dc.oracle_loop(sd, plan, s, "ddim", xT, _contexts(gold, scale), scale))      # off is the plain oracle loop
    gap = rel_l2(on, off)
    print("s %.1f, layers %r: five DDIM steps on vs off %.3e, max |z| %.1f" % (scale, layers, gap, float(on.abs().max())))
    assert gap > LATENT_TOL and bool(torch.isfinite(on).all()) and float(on.abs().max()) < 40.


def test_fold_reference_and_bound():
    """The float64 statement of the fold on exact operands is an fp16 value; the bound holds for fp32 arithmetic done in numpy."""
    g = torch.Generator().manual_seed(9)
    for reps in (2, 3):
        eps = torch.randint(-8, 9, (reps, 1001), generator=g).half()
        for w in pc.FOLD_WEIGHTS:
            ref = pc.fold_ref64(eps, reps, w)
            assert torch.equal(ref.half().double(), ref)
        eps = (torch.randn((reps, 4099), generator=g) * 2).half()
        for w in (-0.4615384, 3.0, 0.1):
            a, c, p = eps[0].float().numpy(), eps[reps - 2].float().numpy(), eps[reps - 1].float().numpy()
            d = (c - p).astype(np.float32)
            r = (np.float64(np.float32(w)) * d.astype(np.float64) + a.astype(np.float64)).astype(np.float32)     # fmaf: one rounding
            out = r.astype(np.float16).astype(np.float64)
            assert (np.abs(out - pc.fold_ref64(eps, reps, w).numpy()) <= pc.fold_bound(eps, reps, w)).all()
