"""DeepCache sampling on the host: the cut (lib/model_zoo/vd.deep_cut) against the written-out tables, the full / shallow
schedule, the fp32 restatement of the cached walk (tests/deepcache_cases.py) against the oracle's plain forward bit for bit, the
samplers' argument validation and the sharding helper's forwarding of the keys.  No GPU, no library needed."""
import math

import pytest
import torch

import deepcache_cases as dc
from vdtest_util import meta, synth_into, tiny_vd_cfg


@pytest.fixture(scope="module")
def tiny_cpu():
    """The tiny product model on the CPU (never run: its modules only say what the walk looks like) and its fp32 weights."""
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    return net, synth_into(net, m["seed"])


def _plans():
    from oracle import vd_oracle as O
    return O.unet_plan(**meta()["unet2d"]), O.unet_plan()


def test_deep_cut_tables(tiny_cpu):
    from lib.model_zoo.vd import deep_cut
    tiny, full = _plans()
    assert dc.flat_order(tiny).count("save_hidden_feature") == 4 and dc.flat_order(full).count("save_hidden_feature") == 12
    for k, want in dc.TINY_CUTS.items():
        assert deep_cut(dc.flat_order(tiny), k) == want == dc.cut(dc.flat_order(tiny), k)
        assert deep_cut(tiny_cpu[0].diffuser["image"], k) == want          # the product net's own orders
    for k, want in dc.FULL_CUTS.items():
        assert deep_cut(dc.flat_order(full), k) == want
    for k in range(1, 12):
        assert deep_cut(dc.flat_order(full), k) == dc.cut(dc.flat_order(full), k)
    # what the issue says about the full-width cuts: no context block in front of the depth-1 cut, and depth 4 is the first whose
    # prefix holds a Downsample (the third data block without a context block behind it: conv_in, ..., down)
    order = dc.flat_order(full)
    assert order[:deep_cut(order, 1)[0]].count("c") == 0 and order[:deep_cut(order, 2)[0]].count("c") == 1
    kinds = [k for k, *_ in full["data"]]
    downs_in_prefix = lambda k: kinds[:order[:deep_cut(order, k)[0]].count("d")].count("down")
    assert [downs_in_prefix(k) for k in (1, 2, 3, 4)] == [0, 0, 0, 1]


def test_deep_cut_rejects_bad_depths_and_the_0d_net(tiny_cpu):
    from lib.model_zoo.vd import deep_cut
    net = tiny_cpu[0]
    order = dc.flat_order(_plans()[0])
    for bad in (0, 4, -1, True, 1.0, "1", None):
        with pytest.raises(ValueError, match="depth"):
            deep_cut(order, bad)
        with pytest.raises(ValueError, match="depth"):
            deep_cut(net.diffuser["image"], bad)
    with pytest.raises(ValueError, match="2-D"):
        deep_cut(net.diffuser["text"], 1)
    with pytest.raises(ValueError, match="saves"):
        deep_cut(order[:-3] + ["load_hidden_feature"] + order[-3:], 1)


@pytest.mark.parametrize("S", [1, 2, 5, 6, 9, 10, 50])
@pytest.mark.parametrize("N", [1, 2, 3, 5, 7])
def test_schedule_rule(S, N):
    """Exactly ceil(S / N) steps of S are full; the sampler lists the same steps (the list it builds is a plain range)."""
    full = dc.full_steps(S, N)
    assert len(full) == math.ceil(S / N) and full[0] == 0
    assert full == list(range(0, S, N))
    assert all(b - a == N for a, b in zip(full, full[1:]))


@pytest.mark.parametrize("dual", [False, True])
def test_restated_walks_equal_the_oracle_forward_bitwise(tiny_cpu, dual):
    from oracle import vd_oracle as O
    _, sd = tiny_cpu
    plan = _plans()[0]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, 16, 16, generator=g)
    ctx = [("text", torch.randn(2, 77, 128, generator=g) * 0.5, 0.4 if dual else 1.0)]
    if dual:
        ctx.append(("image", torch.randn(2, 50, 128, generator=g) * 0.5, 0.6))
    t = torch.full((2,), 500, dtype=torch.long)
    with torch.no_grad():
        ref = O.apply_model_multicontext(sd, plan, x, t, ctx)
    assert torch.equal(dc.walk(sd, plan, x, t, ctx), ref)
    shapes = {1: (2, 64, 16, 16), 2: (2, 128, 16, 16), 3: (2, 128, 8, 8)}
    for k in (1, 2, 3):
        cache = {}
        assert torch.equal(dc.walk(sd, plan, x, t, ctx, depth=k, cache=cache, mode="full"), ref), k
        assert tuple(cache["f"].shape) == shapes[k]
        assert torch.equal(dc.walk(sd, plan, x, t, ctx, depth=k, cache=cache, mode="shallow"), ref), k
        # the shallow walk really reads the kept feature: another feature, another eps
        cache["f"] = cache["f"] * 1.5
        assert not torch.equal(dc.walk(sd, plan, x, t, ctx, depth=k, cache=cache, mode="shallow"), ref), k


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
        for bad in (True, 2.0, 0, -1, "2", None):
            with pytest.raises(ValueError, match="cache_interval"):
                run(cache_interval=bad)
        for bad in (0, 4, -2, True, 1.5):
            with pytest.raises(ValueError, match="depth"):
                run(cache_interval=2, cache_depth=bad)
        with pytest.raises(ValueError, match="depth"):
            run(cache_depth=4)                                  # checked also while caching is off
        with pytest.raises(ValueError, match="image"):
            s.sample(steps=5, shape=[1, 128], x_info={"type": "text", "cache_interval": 2}, c_info=dict(c_info), verbose=False)
        with pytest.raises(ValueError, match="image"):
            s.sample_multicontext(steps=5, shape=[1, 128], x_info={"type": "text", "cache_interval": 3},
                                  c_info_list=[dict(c_info)], verbose=False)
        # well-formed keys pass the validation: the call then gets as far as the device
        with pytest.raises(AssertionError, match="touched the device"):
            run(cache_interval=2, cache_depth=3)
        with pytest.raises(AssertionError, match="touched the device"):
            run(cache_interval=1)


def test_p_sample_ddim_refuses_caching(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(_NoDevice(tiny_cpu[0]))
    x_info = {"type": "image", "x": torch.zeros(1, 4, 16, 16), "cache_interval": 2}
    c_info = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_guidance_scale": 1.0}
    with pytest.raises(ValueError, match="cache_interval"):
        s.p_sample_ddim(x_info, c_info, torch.tensor([1]), 0)
    with pytest.raises(ValueError, match="cache_interval"):
        s.p_sample_ddim_multicontext(x_info, [c_info], torch.tensor([1]), 0)
    with pytest.raises(ValueError, match="cache_interval"):
        s.p_sample_ddim(dict(x_info, cache_interval=0), c_info, torch.tensor([1]), 0)


def test_model_level_key_is_validated(tiny_cpu):
    """x_info['deep_cache'] of apply_model*: refused on the text flow and when malformed, before the latent is looked at."""
    from lib.model_zoo.vd import DeepCache
    net = tiny_cpu[0]
    c_info = {"type": "text", "c": torch.zeros(1, 7, 128)}
    t = torch.zeros(1, dtype=torch.long)
    with pytest.raises(ValueError, match="image"):
        net.apply_model({"type": "text", "x": torch.zeros(1, 128), "deep_cache": (DeepCache(1), "store")}, t, c_info)
    for bad in (DeepCache(1), (DeepCache(1), "full"), ("cache", "store"), (DeepCache(1),)):
        with pytest.raises(ValueError, match="deep_cache"):
            net.apply_model({"type": "image", "x": torch.zeros(1, 4, 16, 16), "deep_cache": bad}, t, c_info)
        with pytest.raises(ValueError, match="deep_cache"):
            net.apply_model_multicontext({"type": "image", "x": torch.zeros(1, 4, 16, 16), "deep_cache": bad}, t,
                                         [dict(c_info, ratio=1.0)])
    cache = DeepCache(2)
    with pytest.raises(ValueError, match="store"):
        cache.load((0, 2), torch.zeros(1, 16, 16, 8))


def test_sharding_helper_forwards_the_keys():
    """vd_sample_sharded(cache_interval=, cache_depth=) at world size 1: the sampler sees the two keys, default 1 / 1."""
    from lib.model_zoo import sharded
    seen = []

    class Net(object):
        device = "cpu"

        def vae_decode(self, z, which):
            return z

    class Sampler(object):
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=False):
            seen.append((x_info.get("cache_interval"), x_info.get("cache_depth")))
            return x_info["xt"], {}

        def sample_multicontext(self, steps, shape, x_info, c_info_list, eta=0., verbose=False):
            seen.append((x_info.get("cache_interval"), x_info.get("cache_depth"), len(c_info_list)))
            return x_info["xt"], {}

    ctx = lambda: {"type": "text", "conditioning": torch.zeros(2, 7, 16), "unconditional_conditioning": torch.zeros(2, 7, 16)}
    shape = [2, 4, 8, 8]
    out = sharded.vd_sample_sharded(Net(), Sampler(), 6, shape, [ctx()], seed=3)
    assert tuple(out.shape) == tuple(shape)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, shape, [ctx()], seed=3, cache_interval=3, cache_depth=2)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, shape, [ctx(), ctx()], seed=3, cache_interval=2)
    assert seen == [(1, 1), (3, 2), (2, 1, 2)]
