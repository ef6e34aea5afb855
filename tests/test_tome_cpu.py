"""Token merging on the host: the restatement of tests/tome_cases.py against a literal transcription of the tomesd algorithm, the
shape of a plan (row_of is a valid map; r = 0 is the identity), the crafted rounding case, the validation of x_info['tome_ratio'] /
['tome_max_downsample'] at sampler level (nothing is drawn and no device is touched before a raise), r and the merging levels of the
tiny and the full-width walks, the step graph's key, the sharding helper's forwarding and the C ABI listing.  No GPU."""
import numpy as np
import pytest
import torch

import tome_cases as tc
from vdtest_util import meta, synth_into, tiny_vd_cfg


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


C_INFO = {"type": "text", "conditioning": torch.zeros(1, 7, 128), "unconditional_conditioning": torch.zeros(1, 7, 128),
          "unconditional_guidance_scale": 7.5}
BAD_RATIOS = [-0.1, 0.76, 1.0, float("nan"), float("inf"), "0.5", True, False, (0.5,), [0.5], 1j]
BAD_DOWNSAMPLES = [0, 3, 4, 1.0, 2.0, "1", True, None.__class__, (1,)]


# ---- 1. the definition -----------------------------------------------------------------------------------------------------------

def test_sets_and_ordinals():
    src, dst = tc.sets(4, 6)
    assert list(dst) == [0, 2, 4, 12, 14, 16] and len(src) == 18 and list(src[:5]) == [1, 3, 5, 6, 7]
    assert tc.r_of(64, 64, 0.5) == 2048 and tc.r_of(64, 64, 0.75) == 3072 and tc.r_of(4, 4, 0.3) == 4 and tc.r_of(6, 10, 0.25) == 15
    assert tc.r_of(8, 8, 0.7) == int(64 * 0.7) == 44 and tc.r_of(8, 8, 0.75) == 48


@pytest.mark.parametrize("H,W,C,B", tc.GRIDS[:4])
@pytest.mark.parametrize("ratio", [0.25, 0.5, 0.75])
def test_restatement_vs_the_tomesd_transcription(H, W, C, B, ratio):
    """Random metrics have distinct scores (asserted), so argsort and the stable rank agree and the comparison is exact: the same
    rows in the same order, the same means (sums of a few fp16 values are exact in float64), the same unmerged tensor."""
    h = tc.random_metric(H, W, C, B, 11 * H + W)
    x = tc.random_metric(H, W, 24, B, 5 * H + W)
    r = tc.r_of(H, W, ratio)
    idx, mx = tc.match_ref(h, H, W)
    mx32 = mx.astype(np.float32)
    for b in range(B):
        assert len(np.unique(mx32[b])) == mx32.shape[1], "tied scores: pick another seed"
    row_of = tc.plan_ref(idx, mx32, H, W, r)
    merged = tc.merge_ref(x, row_of, r)
    back = tc.unmerge_ref(merged, row_of)
    ref_m, ref_u = tc.tomesd_ref(h.double(), x.double(), H, W, r)
    assert merged.shape == (B, H * W - r, 24)
    assert np.array_equal(merged, ref_m.numpy().astype(np.float16))
    assert np.array_equal(back, ref_u.numpy().astype(np.float16))


@pytest.mark.parametrize("H,W,C,B", tc.GRIDS)
def test_row_of_is_a_valid_map_and_r0_is_the_identity(H, W, C, B):
    h = tc.random_metric(H, W, C, B, 3)
    idx, mx = tc.match_ref(h, H, W)
    src, dst = tc.sets(H, W)
    Ns = len(src)
    for r in (0, 1, Ns // 2, Ns):
        row_of = tc.plan_ref(idx, mx.astype(np.float32), H, W, r)
        assert row_of.dtype == np.int32 and row_of.shape == (B, H * W)
        for b in range(B):
            assert set(row_of[b]) == set(range(H * W - r))                       # onto: every merged row has a token
            assert np.array_equal(row_of[b, dst], Ns - r + np.arange(len(dst)))   # destinations in ordinal order, at the end
            own = row_of[b, src] < Ns - r
            assert own.sum() == Ns - r and len(set(row_of[b, src][own])) == Ns - r  # unmerged sources: one row each
            assert np.array_equal(row_of[b, src][~own], Ns - r + idx[b][~own])     # merged ones: their destination's row
    x = tc.random_metric(H, W, 16, B, 4)
    row_of = tc.plan_ref(idx, mx.astype(np.float32), H, W, 0)
    assert np.array_equal(tc.unmerge_ref(tc.merge_ref(x, row_of, 0), row_of), x.numpy())


def test_plan_ties_are_stable_and_negative_scores_rank_last():
    idx = np.zeros((1, 12), dtype=np.int32)
    mx = np.array([[0.5, -1.0, 0.5, 0.25, 0.5, -1.0, 0.0, 0.25, 1.0, -0.0, 0.5, 1.0]], dtype=np.float32)
    src, _ = tc.sets(4, 4)
    row_of = tc.plan_ref(idx, mx, 4, 4, 5)     # merged: the two 1.0 and the first three 0.5 (sources 8, 11, 0, 2, 4)
    merged = row_of[0, src] >= 12 - 5
    assert list(np.nonzero(merged)[0]) == [0, 2, 4, 8, 11]
    # the others keep the descending, stable order: 0.5 (10), 0.25 (3, 7), 0.0 and -0.0 (6, 9: equal), -1.0 (1, 5)
    assert [int(row_of[0, src][i]) for i in (10, 3, 7, 6, 9, 1, 5)] == list(range(7))


def test_the_crafted_mean_rounds_once():
    vals, direct = tc.double_rounding_rows()
    x = np.zeros((1, 16, 8), dtype=np.float16)
    src, dst = tc.sets(4, 4)
    x[0, dst[0]], x[0, src[0]], x[0, src[1]] = vals[0], vals[1], vals[2]
    idx = np.zeros((1, 12), dtype=np.int32)
    mx = np.linspace(1.0, 0.0, 12, dtype=np.float32)[None]
    merged = tc.merge_ref(x, tc.plan_ref(idx, mx, 4, 4, 2), 2)
    assert merged[0, 12 - 2, 0] == direct and float(direct) != float(np.float16(np.float32(vals.astype(np.float64).sum() / 3)))


# ---- 2. the keys -----------------------------------------------------------------------------------------------------------------

def test_sampler_keys_are_validated(tiny_cpu):
    from lib.model_zoo.vd import TokenMerge, _tome_arg
    net = tiny_cpu[0]
    arg = lambda shape=None, **kw: _tome_arg(dict({"type": "image"}, **kw), net, shape)
    assert arg() is None and arg(tome_ratio=None) is None and arg(tome_ratio=0) is None and arg(tome_ratio=0.0) is None
    assert arg(tome_ratio=0, tome_max_downsample=2) is None
    tm = arg(tome_ratio=0.5)
    assert isinstance(tm, TokenMerge) and tm.key() == (0.5, 1) and tm.record is None
    assert arg(tome_ratio=np.float32(0.25), tome_max_downsample=2).key() == (0.25, 2) and arg(tome_ratio=0.75).key() == (0.75, 1)
    ready = TokenMerge(0.5, 2)
    assert arg(tome=ready) is ready and arg(tome=TokenMerge(0.0)) is None
    for bad in BAD_RATIOS:
        with pytest.raises(ValueError, match="tome"):
            arg(tome_ratio=bad)
    for bad in BAD_DOWNSAMPLES:
        with pytest.raises(ValueError, match="tome"):
            arg(tome_ratio=0.5, tome_max_downsample=bad)
    with pytest.raises(ValueError, match="tome"):
        arg(tome=0.5)
    with pytest.raises(ValueError, match="tome"):
        arg(tome=ready, tome_ratio=0.5)
    with pytest.raises(ValueError, match="tome.*image"):
        _tome_arg({"type": "text", "tome_ratio": 0.5}, net)
    with pytest.raises(ValueError, match="tome.*pag.*out of scope"):
        arg(tome_ratio=0.5, pag_scale=3.0)
    assert arg(tome_ratio=0.5, pag_scale=0).key() == (0.5, 1)
    # grids: level 0 must be even; with max_downsample 2 also the half grid
    assert arg((1, 4, 16, 12), tome_ratio=0.5) is not None and arg((1, 4, 6, 10), tome_ratio=0.5) is not None
    for shape in [(1, 4, 15, 16), (1, 4, 16, 7)]:
        with pytest.raises(ValueError, match="tome.*odd"):
            arg(shape, tome_ratio=0.5)
    with pytest.raises(ValueError, match="tome.*odd"):
        arg((1, 4, 6, 16), tome_ratio=0.5, tome_max_downsample=2)
    assert arg((1, 4, 8, 16), tome_ratio=0.5, tome_max_downsample=2) is not None
    # a window's side decides, not the canvas'
    with pytest.raises(ValueError, match="tome.*odd"):
        arg((1, 4, 16, 32), tome_ratio=0.5, window=(16, 10), tome_max_downsample=2)
    assert arg((1, 4, 16, 30), tome_ratio=0.5, window=(16, 12)) is not None


def test_samplers_raise_before_anything_is_drawn(tiny_cpu):
    model = _NoDevice(tiny_cpu[0])
    state = torch.get_rng_state()
    for s in _samplers(model):
        run = lambda x_type="image", shape=(1, 4, 16, 16), **keys: s.sample(
            steps=5, shape=list(shape), x_info=dict({"type": x_type}, **keys), c_info=dict(C_INFO), verbose=False)
        multi = lambda **keys: s.sample_multicontext(steps=5, shape=[1, 4, 16, 16], x_info=dict({"type": "image"}, **keys),
                                                     c_info_list=[dict(C_INFO)], verbose=False)
        for bad in BAD_RATIOS:
            with pytest.raises(ValueError, match="tome"):
                run(tome_ratio=bad)
        with pytest.raises(ValueError, match="tome"):
            multi(tome_ratio=0.5, tome_max_downsample=3)
        with pytest.raises(ValueError, match="tome.*image"):
            run("text", shape=(1, 768), tome_ratio=0.5)
        with pytest.raises(ValueError, match="tome.*odd"):
            run(shape=(1, 4, 16, 15), tome_ratio=0.5)
        with pytest.raises(ValueError, match="tome.*pag"):
            run(tome_ratio=0.5, pag_scale=3.0)
        with pytest.raises(ValueError, match="tome"):
            s.p_sample_ddim({"type": "image", "x": torch.zeros(1, 4, 16, 16), "tome_ratio": 2.0}, dict(C_INFO), torch.zeros(1, dtype=torch.long), 0)
    assert torch.equal(torch.get_rng_state(), state)


def test_forward_key_is_validated(tiny_cpu):
    from lib.model_zoo.vd import TokenMerge, _tome_fwd_arg
    tm = TokenMerge(0.5)
    assert _tome_fwd_arg({"type": "image"}) is None and _tome_fwd_arg({"type": "image", "tome": TokenMerge(0)}) is None
    assert _tome_fwd_arg({"type": "image", "tome": tm}) is tm
    for bad in (0.5, (0.5, 1), "on"):
        with pytest.raises(ValueError, match="tome"):
            _tome_fwd_arg({"type": "image", "tome": bad})
    with pytest.raises(ValueError, match="tome.*image"):
        _tome_fwd_arg({"type": "text", "tome": tm})
    with pytest.raises(ValueError, match="tome.*pag"):
        _tome_fwd_arg({"type": "image", "tome": tm, "pag": ("mid", 1)})


# ---- 3. r and the merging levels -------------------------------------------------------------------------------------------------

def test_merging_blocks_of_the_tiny_net(tiny_cpu):
    from lib.model_zoo.vd import TokenMerge, tome_blocks
    net = tiny_cpu[0].diffuser["image"]
    # the tiny walk: context blocks 0 (16x16), 1 (8x8), 2 (middle, 8x8), 3, 4 (8x8), 5, 6 (16x16)
    assert tome_blocks(net, 16, 16, TokenMerge(0.5)) == [(0, 16, 16, 128), (5, 16, 16, 128), (6, 16, 16, 128)]
    two = tome_blocks(net, 16, 16, TokenMerge(0.5, 2))
    assert [b[0] for b in two] == list(range(7)) and two[1] == (1, 8, 8, 32) and two[0] == (0, 16, 16, 128)
    assert tome_blocks(net, 16, 24, TokenMerge(0.75))[0] == (0, 16, 24, 288)
    assert tome_blocks(net, 4, 4, TokenMerge(0.05)) == []           # int(16 * 0.05) = 0: nothing merges
    with pytest.raises(ValueError, match="tome"):
        tome_blocks(tiny_cpu[0].diffuser["text"], 16, 16, TokenMerge(0.5))


def test_merging_blocks_of_a_full_width_walk():
    """The full-width structure as data: four levels, context blocks on the first three; at 64x64 the 320-wide level merges 2048 of
    4096 tokens, with max_downsample 2 the 640-wide level 512 of 1024."""
    from lib.cfg_helper import model_cfg_bank
    from lib.model_zoo import get_model
    from lib.model_zoo.vd import TokenMerge, tome_blocks
    with torch.device("meta"):          # the structure only: no weight is allocated
        full = get_model()(model_cfg_bank()("openai_unet_2d_v1"), verbose=False)
    one = tome_blocks(full, 64, 64, TokenMerge(0.5))
    assert one == [(ci, 64, 64, 2048) for ci in (0, 1, 13, 14, 15)]
    two = tome_blocks(full, 64, 64, TokenMerge(0.5, 2))
    assert [b for b in two if b[1] == 32] == [(ci, 32, 32, 512) for ci in (2, 3, 10, 11, 12)] and len(two) == 10
    assert tome_blocks(full, 64, 128, TokenMerge(0.25))[0] == (0, 64, 128, 2048)
    with pytest.raises(ValueError, match="tome.*odd"):
        tome_blocks(full, 64, 66, TokenMerge(0.5, 2))


# ---- 4. graph key, sharding, ABI -------------------------------------------------------------------------------------------------

def test_graph_key_tells_settings_apart(tiny_cpu):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(tiny_cpu[0])
    x = torch.zeros(1, 4, 16, 16)
    cis = [{"type": "text", "c": torch.zeros(2, 7, 128)}]
    key = lambda **kw: s._static_key(x, dict({"type": "image"}, **kw), cis, True, True)
    off = key()
    assert key(tome_ratio=0) == off and key(tome_ratio=None) == off
    keys = [off, key(tome_ratio=0.5), key(tome_ratio=0.25), key(tome_ratio=0.5, tome_max_downsample=2)]
    assert len(set(keys)) == 4 and key(tome_ratio=0.5) == keys[1]


def test_sharded_helper_forwards_the_keys(tiny_cpu, monkeypatch):
    import inspect
    from lib.model_zoo import sharded
    sig = inspect.signature(sharded.vd_sample_sharded)
    assert sig.parameters["tome_ratio"].default is None and sig.parameters["tome_max_downsample"].default is None
    src = inspect.getsource(sharded.vd_sample_sharded)
    assert 'x_info["tome_ratio"] = tome_ratio' in src and 'x_info["tome_max_downsample"] = tome_max_downsample' in src


def test_abi_lists_the_entries_and_stays_at_8():
    import os
    from vd_hip import loader
    for name in ("vd_tome_match_f16", "vd_tome_plan", "vd_tome_merge_f16", "vd_tome_unmerge_f16"):
        assert name in loader.PROTOTYPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "vd_hip.h")) as f:
        text = f.read()
    for name in ("vd_tome_match_f16", "vd_tome_plan", "vd_tome_merge_f16", "vd_tome_unmerge_f16"):
        assert ("int %s(" % name) in text
    assert "#define VD_HIP_ABI_VERSION 8" in text or "ABI_VERSION 8" in text
