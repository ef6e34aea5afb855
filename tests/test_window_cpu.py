"""Windowed (MultiDiffusion) sampling on the host: the window tables of lib/model_zoo/windows.py against written-out values, the
samplers' argument validation (before the device is touched), the sharding helper's forwarding of the keys, and the fp32
restatement (tests/window_cases.py) pinned to the oracle's forward.  No GPU, no library needed."""
import itertools

import numpy as np
import pytest
import torch

import deepcache_cases as dc
import window_cases as wc
from lib.model_zoo import windows
from vdtest_util import meta, synth_into, tiny_vd_cfg


@pytest.fixture(scope="module")
def tiny_cpu():
    """The tiny product model on the CPU (never run) and its fp32 weights."""
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    return net, synth_into(net, m["seed"])


def _grid(ys, xs):
    return [[y, x] for y in ys for x in xs]


def test_window_offsets_tables():
    o = windows.window_offsets(12, 20, 8, 4)
    assert o.dtype == np.int32 and o.shape == (8, 2)
    assert o.tolist() == _grid([0, 4], [0, 4, 8, 12])                       # y outer, x inner
    assert windows.window_offsets(8, 20, 8, (8, 6)).tolist() == _grid([0], [0, 6, 12])
    assert windows.window_offsets(8, 24, 8, (8, 4), wrap=True).tolist() == _grid([0], [0, 4, 8, 12, 16, 20])
    assert windows.window_offsets(8, 8, 8, 4).tolist() == [[0, 0]]          # L == l
    assert windows.window_offsets(8, 8, (8, 8), (1, 8)).tolist() == [[0, 0]]
    assert windows.window_offsets(12, 20, (8, 8), [8, 6]).tolist() == _grid([0, 4], [0, 6, 12])     # the last one lies flush
    assert windows.window_offsets(9, 13, (5, 7), 3).tolist() == _grid([0, 3, 4], [0, 3, 6])
    assert windows.window_offsets(16, 16, 8, 8, multiple=4).tolist() == _grid([0, 8], [0, 8])


@pytest.mark.parametrize("wrap", [False, True])
def test_every_pixel_is_covered(wrap):
    for L, l in itertools.product((5, 8, 12, 13, 20, 24), (1, 3, 5, 8)):
        if l > L:
            continue
        for s in range(1, l + 1):
            offs = windows.window_offsets(L, L, l, s, wrap=wrap)
            count = np.zeros((L, L), dtype=np.int64)
            for oy, ox in offs:
                xs = (ox + np.arange(l)) % L if wrap else ox + np.arange(l)
                assert oy + l <= L and (wrap or ox + l <= L)
                count[oy:oy + l, xs] += 1
            assert count.min() >= 1, (L, l, s)
            inv = windows.window_inv_den(L, L, offs, windows.window_weights(l, l, "uniform"), wrap)
            assert inv.dtype == np.float32 and np.array_equal(inv, (1.0 / count).astype(np.float32))


def test_window_offsets_errors():
    bad = [dict(window=9), dict(window=(8, 21)), dict(stride=0), dict(stride=-4), dict(stride=9), dict(stride=(4, 9)),
           dict(window=8.0), dict(window=True), dict(stride=4.0), dict(stride=True), dict(stride=None), dict(window="8"),
           dict(window=(8, 8, 8)), dict(window=0), dict(H=True), dict(W=20.0), dict(wrap=1), dict(wrap=None),
           dict(multiple=16), dict(window=(8, 4), multiple=8), dict(window=6, multiple=4)]
    for kw in bad:
        args = dict(H=8, W=20, window=8, stride=4, wrap=False, multiple=1)
        args.update(kw)
        with pytest.raises(ValueError):
            windows.window_offsets(**args)
    with pytest.raises(ValueError, match="holes"):
        windows.window_offsets(8, 20, 8, 9)
    with pytest.raises(ValueError, match="multiple"):
        windows.window_offsets(8, 20, 4, 2, multiple=8)
    with pytest.raises(ValueError, match="uncovered"):
        windows.window_inv_den(8, 20, np.array([[0, 0]], dtype=np.int32), np.ones((8, 8), dtype=np.float32), False)


def test_window_weights():
    assert np.array_equal(windows.window_weights(3, 5, "uniform"), np.ones((3, 5), dtype=np.float32))
    for h, w in ((8, 8), (5, 7), (64, 64)):
        g = windows.window_weights(h, w, "gaussian")
        assert g.dtype == np.float32 and g.shape == (h, w) and np.all(g > 0)
        assert np.array_equal(g, g[::-1]) and np.array_equal(g, g[:, ::-1])            # symmetric
        assert g.max() == g[(h - 1) // 2, (w - 1) // 2] == g[h // 2, w // 2]                 # peak at the centre
        gy = np.exp(-((np.arange(h) - (h - 1) / 2.0) / h) ** 2 / 0.02)
        gx = np.exp(-((np.arange(w) - (w - 1) / 2.0) / w) ** 2 / 0.02)
        assert np.array_equal(g, np.outer(gy, gx).astype(np.float32))
        assert np.all(np.diff(g[: (h + 1) // 2, w // 2]) > 0)                              # rising towards the centre
    inv = windows.window_inv_den(12, 20, windows.window_offsets(12, 20, 8, 4), windows.window_weights(8, 8, "gaussian"), False)
    assert inv.dtype == np.float32 and np.all(np.isfinite(inv)) and np.all(inv > 0)
    for bad in ("gauss", None, 1):
        with pytest.raises(ValueError, match="window_weight"):
            windows.window_weights(8, 8, bad)


def test_window_chunks():
    assert windows.window_chunks(13, 8) == (2, 7)
    assert windows.window_chunks(8, 8) == (1, 8)
    assert windows.window_chunks(5, 1) == (5, 1)
    assert windows.window_chunks(3, 8) == (1, 3)
    for Wn, wb in itertools.product(range(1, 40), range(1, 12)):
        nc, m = windows.window_chunks(Wn, wb)
        assert m <= wb and nc * m >= Wn > (nc - 1) * m           # every forward but the last is full, the last is not empty
    for bad in (0, -1, True, 2.0, "8", None):
        with pytest.raises(ValueError, match="window_batch"):
            windows.window_chunks(8, bad)


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


def test_window_args_plan(tiny_cpu):
    from lib.model_zoo.ddim import _window_args
    model = _NoDevice(tiny_cpu[0])
    assert _window_args({"type": "image"}, [1, 4, 12, 20], model) is None
    assert _window_args({"type": "image", "window": (12, 20)}, [1, 4, 12, 20], model) is None        # one window: the plain call
    assert _window_args({"type": "image", "window": 8, "window_stride": 2}, [1, 4, 8, 8], model) is None
    p = _window_args({"type": "image", "window": 8}, [2, 4, 12, 20], model)                          # stride: half the window
    assert p["key"] == (8, 8, 4, 4, False, "uniform", 1, 8) and (p["n"], p["nc"], p["m"]) == (8, 1, 8)
    assert p["offsets"].dtype == np.int32 and p["offsets"].shape == (1, 8, 2)
    assert p["offsets"][0].tolist() == _grid([0, 4], [0, 4, 8, 12])
    assert p["wgt"].shape == (8, 8) and p["inv_den"].shape == (12, 20)
    p = _window_args({"type": "image", "window": 8, "window_stride": (4, 4), "window_batch": 3, "window_weight": "gaussian"},
                     [2, 4, 12, 20], model)
    assert p["key"] == (8, 8, 4, 4, False, "gaussian", 3, 3) and p["offsets"].shape == (3, 3, 2)
    assert p["offsets"].reshape(-1, 2)[:8].tolist() == _grid([0, 4], [0, 4, 8, 12])
    assert p["offsets"][2, 2].tolist() == [4, 12]                                                    # the padded slot: the last window
    p = _window_args({"type": "image", "window": 8, "window_stride": (8, 4), "window_wrap": True}, [3, 4, 8, 24], model)
    assert p["key"] == (8, 8, 8, 4, True, "uniform", 1, 6)
    # the tiny data net halves the resolution once: a window side must be even
    with pytest.raises(ValueError, match="multiple"):
        _window_args({"type": "image", "window": (8, 7), "window_stride": 2}, [1, 4, 12, 20], model)


def test_samplers_validate_before_device_work(tiny_cpu):
    model = _NoDevice(tiny_cpu[0])
    c_info = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_conditioning": torch.zeros(1, 7, 128),
              "unconditional_guidance_scale": 7.5}
    for s in _samplers(model):
        run = lambda **keys: s.sample(steps=5, shape=[1, 4, 12, 20], x_info=dict({"type": "image"}, **keys), c_info=dict(c_info),
                                      verbose=False)
        for bad in (True, 8.0, 0, -8, "8", (8,), (8, 8, 8), 24, (16, 8), (8, 24), 7):
            with pytest.raises(ValueError, match="window"):
                run(window=bad)
        for bad in (True, 4.0, 0, -1, 9, (4, 9), "4", (4,)):
            with pytest.raises(ValueError, match="window_stride"):
                run(window=8, window_stride=bad)
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="window_wrap"):
                run(window=8, window_wrap=bad)
        for bad in ("gauss", None, 1):
            with pytest.raises(ValueError, match="window_weight"):
                run(window=8, window_weight=bad)
        for bad in (0, -1, True, 2.0, "8", None):
            with pytest.raises(ValueError, match="window_batch"):
                run(window=8, window_batch=bad)
        with pytest.raises(ValueError, match="window_batch"):
            run(window=(12, 20), window_batch=0)                 # checked also when the plan has a single window
        with pytest.raises(ValueError, match="image"):
            s.sample(steps=5, shape=[1, 128], x_info={"type": "text", "window": 8}, c_info=dict(c_info), verbose=False)
        with pytest.raises(ValueError, match="image"):
            s.sample_multicontext(steps=5, shape=[1, 128], x_info={"type": "text", "window": 8}, c_info_list=[dict(c_info)],
                                  verbose=False)
        # DeepCache would need one kept feature per chunk: refused together, allowed when the plan has a single window
        with pytest.raises(ValueError, match="cache_interval"):
            run(window=8, cache_interval=2)
        with pytest.raises(AssertionError, match="touched the device"):
            run(window=(12, 20), cache_interval=2)
        # well-formed keys pass the validation: the call then gets as far as the device
        with pytest.raises(AssertionError, match="touched the device"):
            run(window=8, window_stride=(4, 6), window_wrap=True, window_weight="gaussian", window_batch=3)
        with pytest.raises(AssertionError, match="touched the device"):
            run(window=(8, 8))


def test_p_sample_ddim_refuses_windows(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(_NoDevice(tiny_cpu[0]))
    x_info = {"type": "image", "x": torch.zeros(1, 4, 12, 20), "window": 8}
    c_info = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_guidance_scale": 1.0}
    with pytest.raises(ValueError, match="window"):
        s.p_sample_ddim(x_info, c_info, torch.tensor([1]), 0)
    with pytest.raises(ValueError, match="window"):
        s.p_sample_ddim_multicontext(x_info, [c_info], torch.tensor([1]), 0)


def test_cfg_contexts_follow_the_window_batch():
    """The UNet's batch order is (replica, sample, window slot): [u.repeat_interleave(m) ; c.repeat_interleave(m)]."""
    from lib.model_zoo.ddim import DDIMSampler

    class Model(object):
        num_timesteps = 1000
        device = "cpu"

    s = DDIMSampler(Model())
    u, c = torch.arange(2.).view(2, 1, 1) + 10, torch.arange(2.).view(2, 1, 1) + 20
    ci = {"type": "text", "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": 7.5}
    cis, guided, _, _ = s._cfg_contexts([dict(ci)], 3)
    assert guided and cis[0]["c"].flatten().tolist() == [10, 10, 10, 11, 11, 11, 20, 20, 20, 21, 21, 21]
    cis, guided, _, _ = s._cfg_contexts([dict(ci, unconditional_guidance_scale=1.0)], 2)
    assert not guided and cis[0]["c"].flatten().tolist() == [20, 20, 21, 21]
    assert torch.equal(s._cfg_contexts([dict(ci)])[0][0]["c"], torch.cat([u, c]))          # without windows: as before


def test_sharding_helper_forwards_the_keys():
    """vd_sample_sharded(window=, ...) at world size 1: the sampler sees the five keys; without `window` it sees none of them."""
    from lib.model_zoo import sharded
    seen = []
    keys = ("window", "window_stride", "window_wrap", "window_weight", "window_batch")

    class Net(object):
        device = "cpu"

        def vae_decode(self, z, which):
            return z

    class Sampler(object):
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=False):
            seen.append(tuple(x_info.get(k, "absent") for k in keys))
            return x_info["xt"], {}

        def sample_multicontext(self, steps, shape, x_info, c_info_list, eta=0., verbose=False):
            seen.append(tuple(x_info.get(k, "absent") for k in keys) + (len(c_info_list),))
            return x_info["xt"], {}

    ctx = lambda: {"type": "text", "conditioning": torch.zeros(2, 7, 16), "unconditional_conditioning": torch.zeros(2, 7, 16)}
    shape = [2, 4, 8, 24]
    out = sharded.vd_sample_sharded(Net(), Sampler(), 6, shape, [ctx()], seed=3)
    assert tuple(out.shape) == tuple(shape)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, shape, [ctx()], seed=3, window=8)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, shape, [ctx(), ctx()], seed=3, window=(8, 8), window_stride=(8, 4),
                              window_wrap=True, window_weight="gaussian", window_batch=3)
    assert seen == [("absent",) * 5, (8, None, False, "uniform", 8), ((8, 8), (8, 4), True, "gaussian", 3, 2)]


def _oracle_inputs(seed, rows, H, W, dual=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, 4, H, W), generator=g)
    ctx = [("text", torch.randn((rows, 77, 128), generator=g) * 0.5, 0.4 if dual else 1.0)]
    if dual:
        ctx.append(("image", torch.randn((rows, 50, 128), generator=g) * 0.5, 0.6))
    return x, torch.full((rows,), 500, dtype=torch.long), ctx


@pytest.mark.parametrize("dual", [False, True])
def test_restatement_with_one_window_is_the_oracle_forward_bitwise(tiny_cpu, dual):
    from oracle import vd_oracle as O
    _, sd = tiny_cpu
    plan = O.unet_plan(**meta()["unet2d"])
    x, t, ctx = _oracle_inputs(3, 2, 8, 12, dual)
    with torch.no_grad():
        ref = O.apply_model_multicontext(sd, plan, x, t, ctx)
    geo = wc.geometry(8, 12, (8, 12), 4)
    assert geo["offs"].tolist() == [[0, 0]]
    assert torch.equal(wc.windowed_eps(sd, plan, x, t, ctx, geo), ref)


def test_restated_merge_on_hand_values():
    """Two 1 x 2 windows on a 1 x 3 canvas, one overlap: the chain and its final multiply by hand."""
    offs = windows.window_offsets(1, 3, (1, 2), 1)
    assert offs.tolist() == [[0, 0], [0, 1]]
    wgt = np.array([[0.5, 0.25]], dtype=np.float32)
    inv = windows.window_inv_den(1, 3, offs, wgt, False)
    assert inv.tolist() == [[2.0, float(np.float32(1.0 / 0.75)), 4.0]]
    e = torch.tensor([1.0, 3.0, 5.0, 7.0]).half().view(1, 2, 1, 1, 2)
    out = wc.merge_restated(e, offs, wgt, inv, 1, 3, False)
    mid = np.float32(np.float32(0.25 * 3.0 + 0.5 * 5.0) * np.float32(1.0 / 0.75))
    assert out.dtype == torch.float16 and out.flatten().tolist() == [1.0, float(np.float16(mid)), 7.0]
    ref = wc.merge_ref64(e, offs, wgt, inv, 1, 3, False)
    assert abs(float(ref[0, 0, 0, 1]) - 3.25 * float(np.float32(1.0 / 0.75))) < 1e-15
    # wrapped: window 1 starts at column 2 and ends on column 0
    offs = windows.window_offsets(1, 3, (1, 2), (1, 2), wrap=True)
    assert offs.tolist() == [[0, 0], [0, 2]]
    ones = np.ones((1, 2), dtype=np.float32)
    out = wc.merge_restated(e, offs, ones, windows.window_inv_den(1, 3, offs, ones, True), 1, 3, True)
    assert out.flatten().tolist() == [4.0, 3.0, 5.0]
    assert wc.gather_ref(torch.tensor([[[[1., 2., 3.]]]]), offs, 1, 2, True).flatten().tolist() == [1., 2., 3., 1.]


def test_windowed_oracle_differs_from_the_canvas_forward(tiny_cpu):
    """What the GPU tests' forward bound has to tell apart: the windowed prediction and the plain forward on the whole canvas."""
    from oracle import vd_oracle as O
    from vdtest_util import rel_l2
    _, sd = tiny_cpu
    plan = O.unet_plan(**meta()["unet2d"])
    x, t, ctx = _oracle_inputs(5, 1, 16, 16)
    geo = wc.geometry(16, 16, 8, 8)                                        # no overlap: four windows
    e = wc.windowed_eps(sd, plan, x, t, ctx, geo)
    for (oy, ox) in geo["offs"]:                                           # every window holds its own forward
        own = dc.walk(sd, plan, x[:, :, oy:oy + 8, ox:ox + 8], t, ctx)
        assert rel_l2(e[:, :, oy:oy + 8, ox:ox + 8], own) < 1e-5
    d = rel_l2(e, dc.walk(sd, plan, x, t, ctx))
    print("windowed vs plain canvas forward on the oracle, 16 x 16 in four 8 x 8 windows: rel-L2 %.3f" % d)
    assert d > 2 * wc.FWD_TOL
