"""The tiled VAE path on the CPU: the 'tent' weight table, the restated blend against the exact one, the exactness the GPU
test's bit-for-bit claim stands on, the roll property of the reference that "no seam" means, every ValueError of the keys with no
device present, and the sharding helper's keyword pass-through."""
import numpy as np
import pytest
import torch

import tile_cases as tc
from vdtest_util import check_exact_reference, exact_ints, meta, rel_l2, synth_into, tiny_vd_cfg

from lib.model_zoo import vae_tiles, windows

# (H, W, tile, stride, wrap) on the grid the blend writes: the kernel cases of tests/test_tile_vae_gpu.py and the model cases
GEOS = [(10, 26, (10, 10), (10, 6), False), (10, 26, (10, 10), (10, 6), True), (6, 11, (4, 4), (2, 4), False),
        (7, 9, (7, 9), (7, 9), False), (16, 40, (16, 16), (12, 12), False), (16, 40, (16, 16), (12, 12), True)]


@pytest.fixture(scope="module")
def tiny_cpu():
    """The tiny product model on the CPU (never run) and its fp32 weights."""
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    return net, synth_into(net, m["seed"])


def _vae_kw():
    dd = meta()["vae"]["ddconfig"]
    return {"ch_mult": tuple(dd["ch_mult"]), "num_res_blocks": dd["num_res_blocks"]}


# ---- 1. the tent weights ---------------------------------------------------------------------------------------------------

def test_tent_values_symmetry_and_exactness():
    t = lambda n: windows.window_weights(1, n, "tent")[0].tolist()
    assert t(1) == [1] and t(2) == [1, 1] and t(5) == [1, 2, 3, 2, 1] and t(8) == [1, 2, 3, 4, 4, 3, 2, 1]
    for h, w in ((1, 1), (2, 5), (8, 8), (5, 8), (128, 96)):
        wg = windows.window_weights(h, w, "tent")
        assert wg.dtype == np.float32 and wg.shape == (h, w)
        assert np.array_equal(wg, wg[::-1]) and np.array_equal(wg, wg[:, ::-1])
        exact = np.outer(np.minimum(np.arange(h) + 1, h - np.arange(h)), np.minimum(np.arange(w) + 1, w - np.arange(w)))
        assert np.array_equal(wg.astype(np.float64), exact.astype(np.float64))            # small integers: exact in fp32
        assert wg.min() == 1.0 and np.array_equal(wg[0], windows.window_weights(1, w, "tent")[0])
    with pytest.raises(ValueError, match="window_weight"):
        windows.window_weights(4, 4, "tents")


@pytest.mark.parametrize("geo", GEOS)
def test_tent_denominator_is_finite_and_one_tile_borders_come_out_with_weight_one(geo):
    H, W, tile, stride, wrap = geo
    g = tc.geometry(H, W, tile, stride, wrap, "tent")
    assert g["inv_den"].dtype == np.float32 and np.all(np.isfinite(g["inv_den"])) and np.all(g["inv_den"] > 0)
    cover = tc.coverage(g["out_offs"], g["h"], g["w"], H, W, wrap)
    assert cover.min() >= 1
    ratio = np.zeros((H, W), dtype=np.float64)                 # the sum over tiles of w * inv_den: 1 everywhere, to fp32 rounding
    single = np.zeros((H, W), dtype=bool)
    for oy, ox in g["offs"]:
        xs = tc._cols(ox, g["w"], W, wrap)
        prod = g["wgt"] * g["inv_den"][oy:oy + g["h"]][:, xs]                             # fp32 products
        ratio[oy:oy + g["h"], xs] += prod
        one = cover[oy:oy + g["h"]][:, xs] == 1
        assert np.all(prod[one] == 1.0)                        # a pixel one tile covers: w * inv_den == 1 exactly
        single[oy:oy + g["h"], xs] |= one
    assert np.allclose(ratio, 1.0, rtol=0, atol=4 * 2.0 ** -24 * cover.max())
    if not wrap:                                               # the canvas's left and right border columns have one tile in x
        assert single[:, 0].any() and single[:, -1].any()


# ---- 2. the restated blend -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weight", ["tent", "uniform", "gaussian"])
@pytest.mark.parametrize("geo", GEOS[:4])
def test_restated_blend_is_the_exact_blend_to_one_fp16_rounding(geo, weight):
    H, W, tile, stride, wrap = geo
    g = tc.geometry(H, W, tile, stride, wrap, weight)
    n = len(g["offs"])
    tiles = torch.randn((2, n, g["h"], g["w"], 3), generator=torch.Generator().manual_seed(n)).half().numpy()
    for tail in (dict(scale=0.5, shift=0.5, clamp01=True), dict(scale=1.0, shift=0.0, clamp01=False, out_nhwc=True)):
        out = tc.blend_restated(tiles, g["out_offs"], g["wgt"], g["inv_den"], H, W, wrap, **tail).astype(np.float64)
        ref = tc.blend_ref64(tiles, g["out_offs"], g["wgt"], g["inv_den"], H, W, wrap, **tail)
        assert out.shape == ref.shape == ((2, H, W, 3) if tail.get("out_nhwc") else (2, 3, H, W))
        # one fp16 rounding of the exact value plus the fp32 chain's slack (at most 4 terms, a product and an fma)
        assert np.all(np.abs(out - ref) <= 2.0 ** -11 * np.abs(ref) + 2.0 ** -24 + 8 * 2.0 ** -24 * np.abs(ref))


def test_restated_blend_on_hand_values():
    """Two 1 x 2 tiles on a 1 x 3 canvas, one overlap, tent weights (all ones at n = 2): the chain and its tail by hand."""
    offs = windows.window_offsets(1, 3, (1, 2), 1)
    wgt = windows.window_weights(1, 2, "tent")
    inv = windows.window_inv_den(1, 3, offs, wgt, False)
    assert offs.tolist() == [[0, 0], [0, 1]] and wgt.tolist() == [[1.0, 1.0]] and inv.tolist() == [[1.0, 0.5, 1.0]]
    tiles = np.array([1.0, -3.0, 0.5, 7.0], dtype=np.float16).reshape(1, 2, 1, 2, 1)
    assert tc.blend_restated(tiles, offs, wgt, inv, 1, 3, False).flatten().tolist() == [1.0, -1.25, 7.0]
    img = tc.blend_restated(tiles, offs, wgt, inv, 1, 3, False, scale=0.5, shift=0.5, clamp01=True)
    assert img.flatten().tolist() == [1.0, 0.0, 1.0]                                      # 0.5 v + 0.5 = 1, -0.125, 4 -> clamped
    assert tc.blend_ref64(tiles, offs, wgt, inv, 1, 3, False, 0.5, 0.5, True).flatten().tolist() == [1.0, 0.0, 1.0]
    # a NaN tile pixel reaches the pixels it covers and no other; the clamp turns it into 0, as fmaxf does
    tiles[0, 1, 0, 0, 0] = np.nan
    out = tc.blend_restated(tiles, offs, wgt, inv, 1, 3, False)
    assert np.isnan(out.flatten()).tolist() == [False, True, False]
    assert tc.blend_restated(tiles, offs, wgt, inv, 1, 3, False, 0.5, 0.5, True).flatten().tolist() == [1.0, 0.0, 1.0]


@pytest.mark.parametrize("weight", ["tent", "uniform"])
@pytest.mark.parametrize("geo", GEOS[:4])
def test_exact_int_tiles_sum_exactly(geo, weight):
    """The GPU test compares bit for bit; that claim stands on this: with exact_ints tiles and tent (integer) weights every
    partial sum is an integer far below 2^24, so the fp32 chain is exact in any implementation that follows the order."""
    H, W, tile, stride, wrap = geo
    g = tc.geometry(H, W, tile, stride, wrap, weight)
    n = len(g["offs"])
    tiles = exact_ints((3, n, g["h"], g["w"], 3), 7 + n).numpy()
    ones = np.ones((H, W), dtype=np.float32)
    total = tc.blend_ref64(tiles, g["out_offs"], g["wgt"], ones, H, W, wrap)
    peak, _ = check_exact_reference(total, what="tile sum %s" % (geo,))
    bound = 8 * float(g["wgt"].max()) * tc.coverage(g["out_offs"], g["h"], g["w"], H, W, wrap).max()
    assert peak <= bound < 2 ** 24                             # the bound on every partial sum (all terms of one sign)
    assert np.array_equal(tc.blend_sum_restated(tiles, g["out_offs"], g["wgt"], H, W, wrap).astype(np.float64), total)
    # split into two launches the chain continues from the exact accumulator
    k = max(n // 2, 1)
    a = tc.blend_sum_restated(tiles[:, :k], g["out_offs"][:k], g["wgt"], H, W, wrap)
    if k < n:
        a = tc.blend_sum_restated(tiles[:, k:], g["out_offs"][k:], g["wgt"], H, W, wrap, acc=a)
    assert np.array_equal(a.astype(np.float64), total)


# ---- 3. the reference on the oracle -----------------------------------------------------------------------------------------

def test_raw_decode_is_the_oracles_decode_before_its_clamp(tiny_cpu):
    from oracle import vd_oracle as O
    _, sd = tiny_cpu
    z = torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        raw = tc.decode_raw(sd, "vae.image", z, **_vae_kw())
        assert torch.equal(torch.clamp((raw + 1) / 2, 0, 1), O.vae_decode(sd, "vae.image", z, **_vae_kw()))
    # one tile == the canvas: the tiled reference is the oracle's decode
    g = tc.geometry(8, 8, 8, 8, False, "tent", f=2)
    assert g["offs"].tolist() == [[0, 0]] and np.all(g["wgt"] * g["inv_den"] == 1.0)
    ref = tc.tiled_decode_ref(sd, z, g, **_vae_kw())
    assert rel_l2(ref, O.vae_decode(sd, "vae.image", z, **_vae_kw())) < 1e-6


def test_wrapped_reference_commutes_with_a_roll_by_one_stride(tiny_cpu):
    """What "no seam" means: with tile_wrap the tiled decode of a latent rolled by one stride along x is the tiled decode rolled
    by f strides -- the tiles are the same tiles, so x = 0 is no special column.  Canvas latent 8 x 24, tile 8, stride 6."""
    _, sd = tiny_cpu
    g = tc.geometry(8, 24, 8, 6, True, "tent", f=2)
    assert g["offs"][:, 1].tolist() == [0, 6, 12, 18] and g["PW"] == 48
    z = torch.randn((1, 4, 8, 24), generator=torch.Generator().manual_seed(11))
    a = tc.tiled_decode_ref(sd, z, g, **_vae_kw())
    b = tc.tiled_decode_ref(sd, torch.roll(z, 6, dims=3), g, **_vae_kw())
    assert a.shape == (1, 3, 16, 48) and 0.0 <= a.min() and a.max() <= 1.0 and a.std() > 1e-3
    assert rel_l2(b, np.roll(a, 12, axis=3)) < 1e-12                                      # float64 rounding (the order of a sum)
    assert rel_l2(b, a) > 1e-3                                                            # the roll moved something
    # the encode's reference has the property too (image 16 x 48, rolled by 12 pixels -> moments rolled by 6)
    ge = tc.geometry(8, 24, 8, 6, True, "tent", f=2, encode=True)
    im = torch.rand((1, 3, 16, 48), generator=torch.Generator().manual_seed(12))
    ma = tc.tiled_moments_ref(sd, im, ge, **_vae_kw())
    mb = tc.tiled_moments_ref(sd, torch.roll(im, 12, dims=3), ge, **_vae_kw())
    assert ma.shape == (1, 8, 8, 24) and rel_l2(mb, np.roll(ma, 6, axis=3)) < 1e-12


# ---- 4. the plan and its errors ----------------------------------------------------------------------------------------------

def test_plan_tables_for_decode_and_encode():
    p = vae_tiles.tile_plan({"tile": 8, "tile_stride": 6, "tile_wrap": True, "tile_batch": 3}, 8, 20, 2)
    assert p["key"] == (8, 20, 8, 8, 6, 6, True, "tent", 2, 2) and (p["n"], p["nc"], p["m"], p["valid"]) == (4, 2, 2, [2, 2])
    assert p["gather"].reshape(-1, 2).tolist() == [[0, 0], [0, 6], [0, 12], [0, 18]] and p["gather_hw"] == (8, 8)
    wgt, inv_den = vae_tiles.tile_tables(p)
    assert np.array_equal(p["blend"], 2 * p["gather"]) and p["tile_hw"] == wgt.shape == (16, 16) and inv_den.shape == (16, 40)
    g = tc.geometry(8, 20, 8, 6, True, "tent", f=2)
    assert np.array_equal(wgt, g["wgt"]) and np.array_equal(inv_den, g["inv_den"])
    e = vae_tiles.tile_plan({"tile": 8, "tile_stride": 6, "tile_wrap": True, "tile_batch": 3}, 8, 20, 2, encode=True)
    wgt, inv_den = vae_tiles.tile_tables(e)
    ge = tc.geometry(8, 20, 8, 6, True, "tent", f=2, encode=True)
    assert np.array_equal(e["gather"], 2 * e["blend"]) and e["gather_hw"] == (16, 16) and e["tile_hw"] == wgt.shape == (8, 8)
    assert e["out_hw"] == inv_den.shape == (8, 20) and p["out_hw"] == (16, 40)
    assert np.array_equal(wgt, ge["wgt"]) and np.array_equal(inv_den, ge["inv_den"])
    # defaults: stride three quarters of the tile (at least 1), tent, 8 tiles per pass; the padded slots repeat the last tile
    d = vae_tiles.tile_plan({"tile": (8, 1)}, 8, 11, 8)
    assert d["key"] == (8, 11, 8, 1, 6, 1, False, "tent", 2, 6) and d["n"] == 11 and d["valid"] == [6, 5]
    assert d["gather"][1, 5].tolist() == d["gather"][1, 4].tolist() == [0, 10]
    assert vae_tiles.tile_tables(d)[1].shape == (64, 88) and np.all(np.isfinite(vae_tiles.tile_tables(d)[1]))   # 11 tiles, not 12
    # no tile, and one tile without wrap: the plain call
    assert vae_tiles.tile_plan({}, 8, 20, 2) is None and vae_tiles.tile_plan({"tile": None}, 8, 20, 2) is None
    assert vae_tiles.tile_plan({"tile": (8, 20), "tile_weight": "gaussian"}, 8, 20, 2) is None
    assert vae_tiles.tile_plan({"tile": (8, 20), "tile_wrap": True}, 8, 20, 2)["n"] == 2       # the default stride, wrapped
    assert vae_tiles.tile_plan({"tile": (8, 20), "tile_stride": (8, 20), "tile_wrap": True}, 8, 20, 2)["n"] == 1
    assert vae_tiles.encode_canvas(16, 40, 2) == (8, 20) and vae_tiles.vae_factor((1, 2, 4, 4)) == 8


def test_every_bad_key_raises_before_the_device(tiny_cpu):
    """ValueError with CPU tensors: a call that got as far as the device would raise RuntimeError (no CPU path) instead."""
    net, _ = tiny_cpu
    vae = net.vae["image"]
    assert vae.factor == 2
    z, im = torch.zeros(1, 4, 8, 20), torch.zeros(1, 3, 16, 40)
    calls = [lambda **k: vae.decode(z, **k), lambda **k: vae.decode_scaled(z, 2.0, **k), lambda **k: vae.encode(im, **k),
             lambda **k: vae.encode_scaled(im, 0.5, **k), lambda **k: net.vae_decode(z, which="image", **k),
             lambda **k: net.vae_encode(im, which="image", **k)]
    for run in calls:
        for bad in (True, 8.0, 0, -8, "8", (8,), (8, 8, 8), 24, (16, 8), (8, 24)):      # a tile side < 1, > the canvas, no int
            with pytest.raises(ValueError, match="tile"):
                run(tile=bad)
        for bad in (True, 4.0, 0, -1, 9, (4, 9), "4", (4,)):                           # a stride < 1 or > the tile, no int
            with pytest.raises(ValueError, match="tile_stride"):
                run(tile=8, tile_stride=bad)
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match="tile_wrap"):
                run(tile=8, tile_wrap=bad)
        for bad in ("tents", None, 1):
            with pytest.raises(ValueError, match="tile_weight"):
                run(tile=8, tile_weight=bad)
        for bad in (0, -1, True, 2.0, "8", None):
            with pytest.raises(ValueError, match="tile_batch"):
                run(tile=8, tile_batch=bad)
        with pytest.raises(ValueError, match="tile_batch"):
            run(tile=(8, 20), tile_batch=0)                      # checked also when the plan has a single tile
        for key, v in (("tile_stride", 4), ("tile_wrap", True), ("tile_weight", "tent"), ("tile_batch", 2)):
            with pytest.raises(ValueError, match="%s needs `tile`" % key):
                run(**{key: v})
            with pytest.raises(ValueError, match="%s needs `tile`" % key):
                run(tile=None, **{key: v})
        with pytest.raises(TypeError, match="tile_stripe"):
            run(tile=8, tile_stripe=4)
        with pytest.raises(RuntimeError, match="GPU"):          # a good call gets past the checks and finds no device
            run(tile=8, tile_stride=6, tile_wrap=True)
        with pytest.raises(RuntimeError, match="GPU"):
            run()
    for shape in ((1, 3, 16, 41), (1, 3, 15, 40), (1, 3, 1, 40)):    # encode: an image side that is not f times an integer
        bad = torch.zeros(shape)
        for run in (lambda: vae.encode(bad, tile=4), lambda: vae.encode_scaled(bad, 0.5, tile=4),
                    lambda: net.vae_encode(bad, which="image", tile=4)):
            with pytest.raises(ValueError, match="down-sampling factor 2 times an integer"):
                run()
    assert not vae._tile_cache                                  # nothing was built


def test_sharding_helper_forwards_the_vae_keys():
    """vd_sample_sharded(vae_tile=, ...) at world size 1: vae_encode and vae_decode both see the keys under the autoencoder's
    names; with the defaults they see none."""
    from lib.model_zoo import sharded
    seen = []

    class Net(object):
        device = "cpu"

        def vae_encode(self, x, which, noise=None, **kw):
            seen.append(("encode", kw))
            return torch.zeros(x.shape[0], 4, 8, 24)

        def vae_decode(self, z, which, **kw):
            seen.append(("decode", kw))
            return z

    class Sampler(object):
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=False):
            return x_info.get("xt", x_info.get("x0")), {}

    ctx = lambda: {"type": "text", "conditioning": torch.zeros(2, 7, 16), "unconditional_conditioning": torch.zeros(2, 7, 16)}
    shape = [2, 4, 8, 24]
    sharded.vd_sample_sharded(Net(), Sampler(), 6, shape, [ctx()], seed=3)
    assert seen == [("decode", {})]
    del seen[:]
    keys = dict(vae_tile=(8, 8), vae_tile_stride=6, vae_tile_wrap=True, vae_tile_weight="uniform", vae_tile_batch=2)
    want = {"tile": (8, 8), "tile_stride": 6, "tile_wrap": True, "tile_weight": "uniform", "tile_batch": 2}
    sharded.vd_sample_sharded(Net(), Sampler(), 6, shape, [ctx()], seed=3, images=torch.zeros(2, 3, 64, 192), fidelity=0.5, **keys)
    assert seen == [("encode", want), ("decode", want)]
    del seen[:]
    sharded.vd_sample_sharded(Net(), Sampler(), 6, shape, [ctx()], seed=3, vae_tile=8)
    assert seen == [("decode", {"tile": 8})]
