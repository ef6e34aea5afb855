"""Regional prompts on the windowed path, on the host: the region tables of lib/model_zoo/windows.py against written-out
values, the plan of ddim._window_args with regions, the samplers' argument validation (before the device is touched), the
sharding helper and app_ops.region_masks, and the restatement (tests/region_cases.py) pinned to the windowed restatement and to
the oracle.  No GPU, no library needed."""
import numpy as np
import pytest
import torch

import region_cases as rc
import window_cases as wc
from lib.model_zoo import windows
from vdtest_util import meta, rel_l2, synth_into, tiny_vd_cfg


@pytest.fixture(scope="module")
def tiny_cpu():
    """The tiny product model on the CPU (never run) and its fp32 weights."""
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    return net, synth_into(net, m["seed"])


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


# ---- tables ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weight", ["uniform", "gaussian"])
@pytest.mark.parametrize("wrap", [False, True])
def test_region_inv_den_of_one_region_of_ones_is_window_inv_den_bitwise(wrap, weight):
    for H, W, win, stride in ((12, 20, (8, 8), (4, 4)), (9, 13, (5, 7), (3, 3)), (8, 8, (8, 8), (4, 4))):
        offs = windows.window_offsets(H, W, win, stride, wrap)
        wgt = windows.window_weights(win[0], win[1], weight)
        inv = windows.region_inv_den(H, W, offs, wgt, np.ones((1, H, W), dtype=np.float32), wrap)
        assert inv.dtype == np.float32 and inv.shape == (H, W)
        assert np.array_equal(inv, windows.window_inv_den(H, W, offs, wgt, wrap))
        # complementary hard masks own every pixel once: the same sums with zeros added
        assert np.array_equal(windows.region_inv_den(H, W, offs, wgt, rc.half_masks(H, W), wrap), inv)


def test_region_inv_den_hand_values_and_uncovered_pixels():
    """Two 1 x 2 windows on a 1 x 3 canvas (offsets 0 and 1, weights 0.5 and 0.25) under two soft regions."""
    offs = windows.window_offsets(1, 3, (1, 2), 1)
    wgt = np.array([[0.5, 0.25]], dtype=np.float32)
    masks = np.array([[[1.0, 0.5, 0.0]], [[0.0, 0.25, 1.0]]], dtype=np.float32)
    inv = windows.region_inv_den(1, 3, offs, wgt, masks, False)
    # pixel 0: window 0 only, 0.5 * 1;  pixel 1: (0.25 + 0.5) * (0.5 + 0.25);  pixel 2: window 1 only, 0.25 * 1
    assert inv.tolist() == [[2.0, float(np.float32(1.0 / (0.75 * 0.75))), 4.0]]
    # the products are rounded to fp32 before they are summed
    third = np.full((1, 1, 3), 1.0 / 3.0, dtype=np.float32)
    w3 = np.array([[0.1, 0.3]], dtype=np.float32)
    exp = 1.0 / (float(np.float32(w3[0, 1] * third[0, 0, 1])) + float(np.float32(w3[0, 0] * third[0, 0, 1])))
    assert windows.region_inv_den(1, 3, offs, w3, third, False)[0, 1] == np.float32(exp)
    masks[1, 0, 2] = 0.0
    with pytest.raises(ValueError, match="leave 1 canvas pixels uncovered; add a background region"):
        windows.region_inv_den(1, 3, offs, wgt, masks, False)
    with pytest.raises(ValueError, match="leave 3 canvas pixels uncovered"):
        windows.region_inv_den(1, 3, offs, wgt, np.zeros((2, 1, 3), dtype=np.float32), False)


def test_region_masks_arg():
    m = windows.region_masks_arg(np.ones((2, 1, 4, 6)), 4, 6)
    assert m.dtype == np.float32 and m.shape == (2, 4, 6) and m.flags["C_CONTIGUOUS"]
    b = windows.region_masks_arg(np.arange(24).reshape(1, 4, 6) % 2 == 0, 4, 6)
    assert b.dtype == np.float32 and b.tolist() == ((np.arange(24).reshape(1, 4, 6) % 2 == 0) * 1.0).tolist()
    assert windows.region_masks_arg([[[0, 1], [0.5, 0.25]]], 2, 2).tolist() == [[[0.0, 1.0], [0.5, 0.25]]]
    ok = np.ones((2, 4, 6), dtype=np.float32)
    bad = [ok[0], ok[None, None], ok[:, :3], ok[:, :, :5], np.ones((2, 2, 4, 6)), ok[:0], np.ones((0, 1, 4, 6)),
           ok * 1.5, ok - 1.5, np.where(np.arange(6) == 2, np.nan, ok), np.where(np.arange(6) == 2, np.inf, ok),
           np.full((2, 4, 6), "a"), None]
    for v in bad:
        with pytest.raises(ValueError, match="region_masks"):
            windows.region_masks_arg(v, 4, 6)


# ---- the plan and the samplers' validation ---------------------------------------------------------------------------------

def test_window_args_plan_with_regions(tiny_cpu):
    from lib.model_zoo.ddim import _window_args
    model = _NoDevice(tiny_cpu[0])
    masks = rc.half_masks(12, 20)
    p = _window_args({"type": "image", "window": 8, "region_masks": masks}, [2, 4, 12, 20], model)
    assert p["key"] == (8, 8, 4, 4, False, "uniform", 1, 8, 2) and p["regions"] == 2 and (p["n"], p["nc"], p["m"]) == (8, 1, 8)
    assert p["masks"].dtype == np.float32 and np.array_equal(p["masks"], masks)
    assert np.array_equal(p["inv_den"], windows.region_inv_den(12, 20, p["offsets"][0], p["wgt"], masks, False))
    # masks as a torch tensor [R, 1, H, W], bool, three regions, chunked
    three = torch.zeros((3, 1, 12, 20), dtype=torch.bool)
    three[0, :, :, :5], three[1, :, :, 5:11], three[2, :, :, 11:] = True, True, True
    p = _window_args({"type": "image", "window": 8, "window_batch": 3, "region_masks": three}, [1, 4, 12, 20], model)
    assert p["key"] == (8, 8, 4, 4, False, "uniform", 3, 3, 3) and p["masks"].shape == (3, 12, 20)
    # a single window is still a plan: the regions need the merge
    p = _window_args({"type": "image", "window": (12, 20), "region_masks": masks}, [1, 4, 12, 20], model)
    assert p is not None and p["key"] == (12, 20, 6, 10, False, "uniform", 1, 1, 2) and (p["n"], p["nc"], p["m"]) == (1, 1, 1)
    assert np.array_equal(p["inv_den"], np.ones((12, 20), dtype=np.float32))
    # without the key: as before
    assert _window_args({"type": "image", "window": (12, 20)}, [1, 4, 12, 20], model) is None
    assert _window_args({"type": "image", "window": 8}, [1, 4, 12, 20], model)["key"] == (8, 8, 4, 4, False, "uniform", 1, 8)
    assert "regions" not in _window_args({"type": "image", "window": 8}, [1, 4, 12, 20], model)


def test_region_contexts_are_region_major():
    from lib.model_zoo.ddim import _region_contexts
    a, b, img, u = (torch.full((2, 3, 4), float(v)) for v in (1, 2, 3, 0))
    text = {"type": "text", "conditioning": [a, b], "unconditional_conditioning": u, "unconditional_guidance_scale": 7.5}
    image = {"type": "image", "conditioning": img, "unconditional_conditioning": u, "unconditional_guidance_scale": 7.5}
    flat = _region_contexts([text, image], {"regions": 2}, 2)
    assert [(c["type"], float(c["conditioning"][0, 0, 0])) for c in flat] == [("text", 1.), ("image", 3.), ("text", 2.), ("image", 3.)]
    assert isinstance(text["conditioning"], list) and all(c["unconditional_conditioning"] is u for c in flat)
    plain = [image]
    assert _region_contexts(plain, None, 2) is plain and _region_contexts(plain, {"key": ()}, 2) is plain
    assert [c["conditioning"] is img for c in _region_contexts(plain, {"regions": 3}, 2)] == [True] * 3


def test_samplers_validate_regions_before_device_work(tiny_cpu):
    model = _NoDevice(tiny_cpu[0])
    z = lambda *shape: torch.zeros(*shape)
    c_info = {"type": "text", "conditioning": z(1, 7, 128), "unconditional_conditioning": z(1, 7, 128),
              "unconditional_guidance_scale": 7.5}
    masks = rc.half_masks(12, 20)
    for s in _samplers(model):
        def run(cond=None, multi=False, **keys):
            ci = dict(c_info) if cond is None else dict(c_info, conditioning=cond)
            x_info = dict({"type": "image"}, **keys)
            if multi:
                other = dict(c_info, type="image", conditioning=z(1, 5, 128), unconditional_conditioning=z(1, 5, 128))
                return s.sample_multicontext(steps=5, shape=[1, 4, 12, 20], x_info=x_info, c_info_list=[ci, other], verbose=False)
            return s.sample(steps=5, shape=[1, 4, 12, 20], x_info=x_info, c_info=ci, verbose=False)

        with pytest.raises(ValueError, match="region_masks needs x_info\\['window'\\]"):
            run(region_masks=masks)
        with pytest.raises(ValueError, match="image"):
            s.sample(steps=5, shape=[1, 128], x_info={"type": "text", "window": 8, "region_masks": masks}, c_info=dict(c_info),
                     verbose=False)
        with pytest.raises(ValueError, match="image"):
            s.sample(steps=5, shape=[1, 128], x_info={"type": "text", "region_masks": masks}, c_info=dict(c_info), verbose=False)
        for bad in (masks[0], masks[:, :, :19], masks * 2, masks - 1, masks[:0], np.where(masks > 0, np.nan, masks)):
            with pytest.raises(ValueError, match="region_masks"):
                run(window=8, region_masks=bad)
        with pytest.raises(ValueError, match="uncovered; add a background region"):
            run(window=8, region_masks=masks * np.array([1.0, 0.0], dtype=np.float32)[:, None, None])
        # a conditioning list: needs the masks, R entries, one shape, the batch of the call
        for multi in (False, True):
            with pytest.raises(ValueError, match="needs x_info\\['region_masks'\\]"):
                run([z(1, 7, 128), z(1, 7, 128)], multi)
            with pytest.raises(ValueError, match="needs x_info\\['region_masks'\\]"):
                run([z(1, 7, 128), z(1, 7, 128)], multi, window=8)
            with pytest.raises(ValueError, match="3 entries for 2 region_masks"):
                run([z(1, 7, 128)] * 3, multi, window=8, region_masks=masks)
            with pytest.raises(ValueError, match="1 entries for 2 region_masks"):
                run((z(1, 7, 128),), multi, window=8, region_masks=masks)
            with pytest.raises(ValueError, match="differ in shape"):
                run([z(1, 7, 128), z(1, 8, 128)], multi, window=8, region_masks=masks)
            with pytest.raises(ValueError, match="expected \\[1, L, D\\]"):
                run([z(2, 7, 128), z(2, 7, 128)], multi, window=8, region_masks=masks)
            # DeepCache refuses windows and so regions
            with pytest.raises(ValueError, match="cache_interval"):
                run([z(1, 7, 128), z(1, 7, 128)], multi, window=8, region_masks=masks, cache_interval=2)
            # well-formed calls pass the validation: they get as far as the device
            with pytest.raises(AssertionError, match="touched the device"):
                run([z(1, 7, 128), z(1, 7, 128)], multi, window=8, region_masks=masks)
            with pytest.raises(AssertionError, match="touched the device"):
                run(None, multi, window=(12, 20), region_masks=torch.from_numpy(masks)[:, None])
            with pytest.raises(AssertionError, match="touched the device"):
                run(None, multi, window=8)


def test_p_sample_ddim_refuses_regions(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(_NoDevice(tiny_cpu[0]))
    c_info = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_guidance_scale": 1.0}
    for keys in ({"window": 8, "region_masks": rc.half_masks(12, 20)}, {"region_masks": rc.half_masks(12, 20)}):
        x_info = dict({"type": "image", "x": torch.zeros(1, 4, 12, 20)}, **keys)
        with pytest.raises(ValueError, match="window"):
            s.p_sample_ddim(x_info, c_info, torch.tensor([1]), 0)
        with pytest.raises(ValueError, match="window"):
            s.p_sample_ddim_multicontext(x_info, [c_info], torch.tensor([1]), 0)


def test_sharding_helper_forwards_the_masks_and_slices_lists_per_sample():
    from lib.model_zoo import sharded
    seen = []

    class Net(object):
        device = "cpu"

        def vae_decode(self, z, which):
            return z

    class Sampler(object):
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=False):
            seen.append((x_info.get("region_masks", "absent"), x_info.get("window", "absent"), c_info["conditioning"]))
            return x_info["xt"], {}

    a, b, u = torch.arange(3.).view(3, 1, 1) + 10, torch.arange(3.).view(3, 1, 1) + 20, torch.zeros(3, 1, 1)
    ctx = lambda cond: {"type": "text", "conditioning": cond, "unconditional_conditioning": u}
    masks = rc.half_masks(8, 24)
    shape = [3, 4, 8, 24]
    sharded.vd_sample_sharded(Net(), Sampler(), 6, shape, [ctx(a)], seed=3, window=8)
    sharded.vd_sample_sharded(Net(), Sampler(), 6, shape, [ctx([a, b])], seed=3, window=8, region_masks=masks)
    assert seen[0][0] == "absent" and torch.equal(seen[0][2], a)
    assert seen[1][0] is masks and seen[1][1] == 8
    assert isinstance(seen[1][2], list) and len(seen[1][2]) == 2 and torch.equal(seen[1][2][0], a) and torch.equal(seen[1][2][1], b)
    # samples [1, 3) of a two-region list (and a tuple): both regions, two samples each
    for kind in (list, tuple):
        sl = sharded._slice_ctx(ctx(kind([a, b])), 1, 3)
        assert isinstance(sl["conditioning"], kind) and len(sl["conditioning"]) == 2
        assert sl["conditioning"][0].flatten().tolist() == [11., 12.] and sl["conditioning"][1].flatten().tolist() == [21., 22.]
        assert tuple(sl["unconditional_conditioning"].shape) == (2, 1, 1)
    assert sharded._slice_ctx(ctx(a), 1, 3)["conditioning"].flatten().tolist() == [11., 12.]


def test_app_ops_region_masks():
    from lib import app_ops
    px = torch.zeros((2, 1, 16, 32))
    px[0, :, :, :16] = 1                             # the left half
    px[1, :, :8, 20:32] = 1                          # the top of the right part, from the middle of a latent pixel on
    m, appended = app_ops.region_masks(px)
    assert appended and m.dtype == torch.float32 and tuple(m.shape) == (3, 2, 4)
    assert m[0].tolist() == [[1, 1, 0, 0]] * 2 and m[1].tolist() == [[0, 0, 0.5, 1], [0, 0, 0, 0]]
    assert m[2].tolist() == [[0, 0, 0.5, 0], [0, 0, 1, 1]] and torch.equal(m.sum(0), torch.ones(2, 4))
    assert windows.region_masks_arg(m.numpy(), 2, 4).shape == (3, 2, 4)
    m2, appended = app_ops.region_masks(px, background=False)
    assert not appended and torch.equal(m2, m[:2])
    m3, appended = app_ops.region_masks(px, mode="max")
    assert appended and m3[1].tolist() == [[0, 0, 1, 1], [0, 0, 0, 0]] and m3[2].tolist() == [[0, 0, 0, 0], [0, 0, 1, 1]]
    full = torch.ones((1, 1, 16, 32), dtype=torch.bool)
    m4, appended = app_ops.region_masks(full)
    assert not appended and tuple(m4.shape) == (1, 2, 4) and bool((m4 == 1).all())
    # overlapping regions: the background is clipped at 0
    m5, appended = app_ops.region_masks(torch.ones((2, 1, 16, 32)), factor=4)
    assert not appended and tuple(m5.shape) == (2, 4, 8)
    for bad in (torch.ones((2, 16, 32)), torch.ones((2, 1, 12, 32)), torch.ones((0, 1, 16, 32))):
        with pytest.raises(ValueError):
            app_ops.region_masks(bad)


# ---- the restated merge ----------------------------------------------------------------------------------------------------

def test_restated_masked_merge_on_hand_values():
    """Two 1 x 2 windows on a 1 x 3 canvas, two regions with soft masks on the shared pixel: the chain by hand."""
    offs = windows.window_offsets(1, 3, (1, 2), 1)
    wgt = np.array([[0.5, 0.25]], dtype=np.float32)
    masks = np.array([[[1.0, 0.5, 0.0]], [[0.0, 0.25, 1.0]]], dtype=np.float32)
    inv = windows.region_inv_den(1, 3, offs, wgt, masks, False)
    eA = torch.tensor([1.0, 3.0, 5.0, float("nan")]).half().view(1, 2, 1, 1, 2)      # region 0 never owns pixel 2
    eB = torch.tensor([float("nan"), 2.0, 4.0, 7.0]).half().view(1, 2, 1, 1, 2)      # region 1 never owns pixel 0
    out = rc.merge_masked_restated([eA, eB], offs, wgt, masks, inv, 1, 3, False)
    # pixel 1, region-major: A window 0 (0.25 * 0.5) 3, A window 1 (0.5 * 0.5) 5, B window 0 (0.25 * 0.25) 2, B window 1 (0.5 * 0.25) 4
    mid = np.float32(0.125 * 3.0 + 0.25 * 5.0 + 0.0625 * 2.0 + 0.125 * 4.0) * inv[0, 1]
    assert out.dtype == torch.float16 and out.flatten().tolist() == [1.0, float(np.float16(mid)), 7.0]
    ref = rc.merge_masked_ref64([eA, eB], offs, wgt, masks, inv, 1, 3, False)
    assert ref.dtype == torch.float64 and abs(float(ref[0, 0, 0, 1]) - 2.25 * float(inv[0, 1])) < 1e-15
    assert ref.flatten()[[0, 2]].tolist() == [1.0, 7.0]


@pytest.mark.parametrize("weight", ["uniform", "gaussian"])
@pytest.mark.parametrize("wrap", [False, True])
def test_restated_complementary_masks_on_duplicated_predictions_are_the_windowed_merge_bitwise(wrap, weight):
    H, W = 12, 16 if wrap else 20
    g = wc.geometry(H, W, (8, 8), (4, 4), wrap, weight)
    e = torch.randn((3, len(g["offs"]), 4, 8, 8), generator=torch.Generator().manual_seed(2)).half()
    ref = wc.merge_restated(e, g["offs"], g["wgt"], g["inv_den"], H, W, wrap)
    for masks in (np.ones((1, H, W), dtype=np.float32), rc.half_masks(H, W), rc.half_masks(H, W, 7)[::-1]):
        rg = rc.geometry(H, W, (8, 8), (4, 4), masks, wrap, weight)
        assert np.array_equal(rg["inv_den"], g["inv_den"])
        out = rc.merge_masked_restated([e] * len(masks), g["offs"], g["wgt"], rg["masks"], rg["inv_den"], H, W, wrap)
        assert torch.equal(out, ref)


# ---- the oracle ------------------------------------------------------------------------------------------------------------

def _oracle_case(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, 4, 12, 20), generator=g)
    cond = lambda: torch.randn((1, 77, 128), generator=g) * 0.5
    u, a, b = cond(), cond(), cond()
    xin, t = torch.cat([x, x]), torch.full((2,), 500, dtype=torch.long)
    return xin, t, [("text", torch.cat([u, a]), 1.0)], [("text", torch.cat([u, b]), 1.0)]


def test_regional_oracle_is_local_and_differs_from_both_single_prompt_predictions(tiny_cpu):
    """Canvas 12 x 20, windows 8 x 8, stride 4, left half prompt A, right half prompt B: on each half the float64 regional merge
    is the single-prompt windowed oracle exactly, and over the canvas it is more than 2 FWD_TOL from either on the conditional
    rows -- what the GPU tests' forward bound has to tell apart.  Measured with generator seed 7 and these draws: 0.0250 and
    0.0236; the two guided single-prompt predictions are 0.24 apart."""
    from oracle import vd_oracle as O
    _, sd = tiny_cpu
    plan = O.unet_plan(**meta()["unet2d"])
    xin, t, ctx_a, ctx_b = _oracle_case(7)
    geo = rc.geometry(12, 20, 8, 4, rc.half_masks(12, 20))
    with torch.no_grad():
        reg = rc.regional_eps(sd, plan, xin, t, [ctx_a, ctx_b], geo)
        only_a = wc.windowed_eps(sd, plan, xin, t, ctx_a, geo)
        only_b = wc.windowed_eps(sd, plan, xin, t, ctx_b, geo)
    assert torch.equal(reg[..., :10], only_a[..., :10]) and torch.equal(reg[..., 10:], only_b[..., 10:])
    assert torch.equal(reg[:1], only_a[:1]) and torch.equal(reg[:1], only_b[:1])          # the unconditional rows: one prompt
    gap_a, gap_b = rel_l2(reg[1:], only_a[1:]), rel_l2(reg[1:], only_b[1:])
    eg = lambda e: e[:1] + 7.5 * (e[1:] - e[:1])
    print("regional vs single-prompt windowed oracle, conditional rows: rel-L2 %.4f (A) %.4f (B); guided A vs B %.3f"
          % (gap_a, gap_b, rel_l2(eg(only_a), eg(only_b))))
    assert gap_a > 2 * rc.FWD_TOL and gap_b > 2 * rc.FWD_TOL
