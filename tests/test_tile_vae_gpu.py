"""The tiled VAE path on the GPU: vd_tile_blend_f16 per element and bit for bit against the restated chain of
tests/tile_cases.py (exact-integer tiles, so the comparison has no tolerance; tests/test_tile_vae_cpu.py shows the sums are
exact), the entry point's refusals, and the tiled decode / encode of the tiny and the full-width autoencoder against the fp32
oracle run per tile and blended in float64, with the identities (no key = the plain call, one tile = the plain call, twice the
same bits) and the seam property."""
import ctypes

import numpy as np
import pytest
import torch

import tile_cases as tc
from tile_cases import FWD_TOL
from vdtest_util import assert_exact, exact_ints, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

TAILS = [(0.5, 0.5, True), (1.0, 0.0, False)]          # (scale, shift, clamp01): the decode's and the encode's, the only ones used
TAIL_IDS = ["image", "moments"]
AXES = {False: ("row", "channel", "y", "x"), True: ("row", "y", "x", "channel")}


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _blend(dev, tiles, g, tail, out_nhwc, batch=None, shift_bytes=False):
    """ops.tile_blend over the tiles [RB, n, ph, pw, C] (numpy fp16) of geometry g, as one launch or in chunks of `batch` slots
    whose unused slots hold NaN and repeat the last tile's offsets (never read); acc and out start as NaN (never read before
    they are written).  shift_bytes: the tile buffer and out start 2 bytes past a 16-byte boundary."""
    from lib.model_zoo import windows
    from vd_hip import ops
    RB, n, ph, pw, C = tiles.shape
    nc, m = (1, n) if batch is None else windows.window_chunks(n, batch)
    offs = np.concatenate([g["out_offs"], np.repeat(g["out_offs"][-1:], nc * m - n, 0)]).reshape(nc, m, 2)
    padded = np.full((RB, nc * m, ph, pw, C), np.nan, dtype=np.float16)
    padded[:, :n] = tiles
    wgt, inv = _dev(g["wgt"], dev), _dev(g["inv_den"], dev)
    PH, PW = g["PH"], g["PW"]
    oshape = (RB, PH, PW, C) if out_nhwc else (RB, C, PH, PW)
    acc = torch.full((RB, C, PH, PW), float("nan"), dtype=torch.float32, device=dev) if nc > 1 else None
    obuf = torch.full((RB * C * PH * PW + 1,), float("nan"), dtype=torch.float16, device=dev)
    out = obuf[1:].view(oshape) if shift_bytes else obuf[:-1].view(oshape)
    res = None
    for k in range(nc):
        chunk = np.ascontiguousarray(padded[:, k * m:(k + 1) * m])
        tbuf = torch.empty(chunk.size + 1, dtype=torch.float16, device=dev)
        t = (tbuf[1:] if shift_bytes else tbuf[:-1]).view(chunk.shape)
        t.copy_(torch.from_numpy(chunk))
        res = ops.tile_blend(t, _dev(offs[k], dev), wgt, inv, PH, PW, min(m, n - k * m), g["wrap"], k == 0, k == nc - 1, acc=acc,
                             out=out, out_nhwc=out_nhwc, scale=tail[0], shift=tail[1], clamp01=tail[2])
    assert res.data_ptr() == out.data_ptr() and res.dtype == torch.float16
    torch.cuda.synchronize()
    assert bool(torch.isnan(obuf[0 if shift_bytes else -1]))            # nothing next to the buffer was written
    return res.cpu().numpy()


def _restated(tiles, g, tail, out_nhwc):
    return tc.blend_restated(tiles, g["out_offs"], g["wgt"], g["inv_den"], g["PH"], g["PW"], g["wrap"], tail[0], tail[1], tail[2],
                             out_nhwc)


# ---- 1. the kernel, per element -------------------------------------------------------------------------------------------

# (C, out_nhwc, canvas, tile, stride, wrap, tiles): odd sizes with no 16-byte alignment anywhere; the last tile straddling the
# seam; two-axis tiling with a pixel under four tiles and the 16-byte accesses of C = 8; one tile equal to the canvas at C = 16
KERNEL_CASES = [(3, False, (10, 26), (10, 10), (10, 6), False, 4), (3, False, (10, 26), (10, 10), (10, 6), True, 5),
                (8, True, (6, 11), (4, 4), (2, 4), False, 6), (16, True, (7, 9), (7, 9), (7, 9), False, 1)]
KERNEL_IDS = ["c3-nchw-flat", "c3-nchw-wrap", "c8-nhwc-2x3", "c16-nhwc-one-tile"]


@pytest.mark.parametrize("tail", TAILS, ids=TAIL_IDS)
@pytest.mark.parametrize("weight", ["tent", "uniform"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=KERNEL_IDS)
def test_blend_is_the_restated_chain_bitwise(dev, case, weight, tail):
    C, nhwc, (PH, PW), tile, stride, wrap, n = case
    g = tc.geometry(PH, PW, tile, stride, wrap, weight)
    assert len(g["offs"]) == n
    if (C, wrap) == (3, False):
        assert g["offs"][:, 1].tolist() == [0, 6, 12, 16]
    if wrap:
        assert g["offs"][-1].tolist() == [0, 24] and 24 + 10 > PW                          # the last tile straddles the seam
    if C == 8:
        assert tc.coverage(g["offs"], 4, 4, PH, PW, False).max() == 4                      # a pixel under four tiles
    tiles = exact_ints((2, n, g["h"], g["w"], C), 31 * C + n).numpy()
    ref = _restated(tiles, g, tail, nhwc)
    out = _blend(dev, tiles, g, tail, nhwc)
    assert_exact(out, ref.astype(np.float64), AXES[nhwc], "%s %s %s" % (KERNEL_IDS[KERNEL_CASES.index(case)], weight, tail))
    # the same elements through other accesses: buffers that start 2 bytes past a 16-byte boundary
    assert np.array_equal(_blend(dev, tiles, g, tail, nhwc, shift_bytes=True), out)


@pytest.mark.parametrize("tail", TAILS, ids=TAIL_IDS)
@pytest.mark.parametrize("weight", ["tent", "uniform"])
def test_blend_has_the_same_bits_however_the_tiles_are_chunked(dev, weight, tail):
    """The five wrapped tiles as one launch and as 2 chunks of 3 slots (valid = 3 and 2; the unused slot is NaN and must not
    show), and with tile_batch 1, 2 and 8: acc is exact fp32 between launches, so the split decides no bit."""
    from lib.model_zoo import windows
    g = tc.geometry(10, 26, (10, 10), (10, 6), True, weight)
    tiles = exact_ints((2, 5, 10, 10, 3), 17).numpy()
    ref = _restated(tiles, g, tail, False).astype(np.float64)
    one = _blend(dev, tiles, g, tail, False)
    assert windows.window_chunks(5, 3) == (2, 3)
    for batch in (3, 1, 2, 8):
        out = _blend(dev, tiles, g, tail, False, batch=batch)
        assert_exact(out, ref, AXES[False], "tile_batch %d %s %s" % (batch, weight, tail))
        assert np.array_equal(out, one)
    # random (inexact) tiles and gaussian weights: still the same bits for every split, and the restated chain's
    rnd = torch.randn((2, 5, 10, 10, 3), generator=torch.Generator().manual_seed(3)).half().numpy()
    gg = tc.geometry(10, 26, (10, 10), (10, 6), True, "gaussian")
    outs = [_blend(dev, rnd, gg, tail, False, batch=b) for b in (None, 3, 1, 2)]
    assert all(np.array_equal(o, outs[0]) for o in outs[1:]) and np.array_equal(outs[0], _restated(rnd, gg, tail, False))


def test_a_nan_tile_reaches_exactly_the_pixels_it_covers(dev):
    g = tc.geometry(6, 11, (4, 4), (2, 4), False, "tent")
    assert g["offs"].tolist() == [[0, 0], [0, 4], [0, 7], [2, 0], [2, 4], [2, 7]]
    tiles = exact_ints((2, 6, 4, 4, 8), 23).numpy()
    clean = _blend(dev, tiles, g, TAILS[1], True)
    bad = tiles.copy()
    bad[1, 4] = np.nan                                                  # row 1, the tile at (2, 4)
    out = _blend(dev, bad, g, TAILS[1], True)
    hit = np.zeros((2, 6, 11, 8), dtype=bool)
    hit[1, 2:6, 4:8] = True
    assert np.array_equal(np.isnan(out), hit) and np.array_equal(out[~hit], clean[~hit])
    ref = _restated(bad, g, TAILS[1], True)
    assert np.array_equal(np.isnan(ref), hit)                           # the restated chain says the same
    img = _blend(dev, bad, g, TAILS[0], True)                           # the clamp turns the NaN into 0 (fmaxf), nothing else moves
    assert not np.isnan(img).any() and np.all(img[hit] == 0) and np.array_equal(img, _restated(bad, g, TAILS[0], True))


def test_entry_point_refuses_bad_arguments(dev):
    """Every refusal of the contract, with valid device data only."""
    from vd_hip import ops
    from vd_hip.loader import VdHipError, lib
    L = lib()
    f16 = dict(device=dev, dtype=torch.float16)
    tiles = torch.zeros((1, 2, 8, 8, 3), **f16)
    offs = torch.zeros((2, 2), device=dev, dtype=torch.int32)
    wgt, inv = torch.ones((8, 8), device=dev), torch.ones((8, 12), device=dev)
    acc, out = torch.zeros((1, 3, 8, 12), device=dev), torch.zeros((1, 3, 8, 12), **f16)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def blend(t=tiles, acc=acc, out=out, wgt=wgt, inv=inv, offs=offs, RB=1, C=3, PH=8, PW=12, ph=8, pw=8, slots=2, valid=2, wrap=0,
              first=1, last=1, nhwc=0):
        return L.vd_tile_blend_f16(P(t), P(acc), P(out), P(wgt), P(inv), P(offs), RB, C, PH, PW, ph, pw, slots, valid, wrap, first,
                                   last, nhwc, 1.0, 0.0, 0, stream)

    assert blend() == 0 and blend(acc=None) == 0 and blend(first=1, last=0, out=None) == 0 and blend(first=0, last=1) == 0
    assert blend(nhwc=1) == 0 and blend(C=1) == 0
    bad = [dict(t=None), dict(wgt=None), dict(inv=None), dict(offs=None), dict(out=None), dict(acc=None, last=0),
           dict(acc=None, first=0), dict(RB=0), dict(C=0), dict(C=-3), dict(C=17), dict(PH=0), dict(PW=0), dict(ph=0), dict(pw=0),
           dict(slots=0), dict(ph=9), dict(pw=13), dict(valid=0), dict(valid=3), dict(valid=-1)]
    for kw in bad:
        assert blend(**kw) < 0 and L.vd_last_error().decode().startswith("vd_tile_blend_f16"), kw
    assert L.vd_abi_version() == 8                                      # the entry is additive
    torch.cuda.synchronize()
    # the wrapper checks shape, dtype and device before the library is called
    B = ops.tile_blend
    args = lambda **kw: dict(dict(tiles=tiles, offs=offs, wgt=wgt, inv_den=inv, PH=8, PW=12, valid=2, wrap=False, first=True,
                                  last=True), **kw)
    assert tuple(B(**args()).shape) == (1, 3, 8, 12) and tuple(B(**args(out_nhwc=True)).shape) == (1, 8, 12, 3)
    assert B(**args(last=False)).dtype == torch.float32
    for kw in (dict(tiles=tiles.float()), dict(tiles=tiles.cpu()), dict(tiles=tiles[:, :1]), dict(tiles=tiles[..., :2]),
               dict(tiles=torch.zeros((1, 2, 8, 8, 17), **f16)), dict(offs=offs.long()), dict(offs=offs[:, :1]),
               dict(wgt=wgt[:4]), dict(wgt=wgt.half()), dict(inv_den=inv[:, :8]), dict(PH=7), dict(PW=7), dict(valid=0),
               dict(valid=3), dict(first=False), dict(acc=acc[:, :2]), dict(acc=acc.half()), dict(out=out.float()),
               dict(out=out, out_nhwc=True), dict(out=out[:, :2])):
        with pytest.raises(VdHipError):
            B(**args(**kw))


# ---- 2. the tiny autoencoder against the oracle ------------------------------------------------------------------------------

SCALE = 0.18215
KEYS = dict(tile=8, tile_stride=6)


@pytest.fixture(scope="module")
def tiny(dev):
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    sd = synth_into(net, m["seed"])
    net = net.half()
    net.to(dev)
    dd = m["vae"]["ddconfig"]
    return net, sd, {"ch_mult": tuple(dd["ch_mult"]), "num_res_blocks": dd["num_res_blocks"]}


@pytest.fixture(scope="module")
def canvas(tiny):
    """The inputs every model test shares (batch 2, canvas latent 8 x 20, image 16 x 40) and the oracle's references, made once."""
    _, sd, kw = tiny
    g = torch.Generator().manual_seed(21)
    z = torch.randn((2, 4, 8, 20), generator=g)
    im = torch.rand((2, 3, 16, 40), generator=g)
    nz = torch.randn((2, 4, 8, 20), generator=g)
    flat = tc.geometry(8, 20, 8, 6, False, "tent", f=2)
    wrap = tc.geometry(8, 20, 8, 6, True, "tent", f=2)
    assert flat["offs"][:, 1].tolist() == [0, 6, 12] and wrap["offs"][:, 1].tolist() == [0, 6, 12, 18]     # the last across the seam
    return {"z": z, "im": im, "nz": nz,
            "dec_flat": tc.tiled_decode_ref(sd, z / SCALE, flat, **kw), "dec_wrap": tc.tiled_decode_ref(sd, z / SCALE, wrap, **kw),
            "mom_wrap": tc.tiled_moments_ref(sd, im, tc.geometry(8, 20, 8, 6, True, "tent", f=2, encode=True), **kw)}


def test_the_tiny_network_takes_the_canvas_sides(tiny, canvas, dev):
    """The precondition of everything below: the plain whole-canvas decode and encode of 8 x 20 / 16 x 40 meet the oracle."""
    from oracle import vd_oracle as O
    net, sd, kw = tiny
    with torch.no_grad():
        ref = O.vae_decode(sd, "vae.image", canvas["z"] / SCALE, **kw)
        mom = O.vae_encode_moments(sd, "vae.image", canvas["im"], **kw)
    dec = net.vae_decode(canvas["z"].half().to(dev), which="image")
    assert tuple(dec.shape) == (2, 3, 16, 40) and rel_l2(dec, ref) < FWD_TOL
    assert rel_l2(net.vae["image"].encode(canvas["im"].half().to(dev), out_posterior=True).parameters, mom) < FWD_TOL


@pytest.mark.parametrize("wrap,batch,n", [(False, 8, 3), (True, 8, 4), (True, 2, 4)], ids=["flat-3", "wrap-4", "wrap-4-in-2-chunks"])
def test_tiled_decode_vs_oracle(tiny, canvas, dev, wrap, batch, n):
    net, _, _ = tiny
    ref = canvas["dec_wrap" if wrap else "dec_flat"]
    dec = net.vae_decode(canvas["z"].half().to(dev), which="image", tile_wrap=wrap, tile_batch=batch, **KEYS)
    assert dec.dtype == torch.float16 and tuple(dec.shape) == (2, 3, 16, 40)
    assert float(dec.min()) >= 0 and float(dec.max()) <= 1
    err = rel_l2(dec, ref)
    print("tiled decode (tiny, wrap=%s, tile_batch=%d, %d tiles): rel_l2 %.3e vs the per-tile oracle" % (wrap, batch, n, err))
    assert err < FWD_TOL
    plain = net.vae_decode(canvas["z"].half().to(dev), which="image")
    assert rel_l2(dec, plain) > 10 * FWD_TOL           # the tiled result is not the whole-canvas result, and is not meant to be


def test_tile_batch_does_not_move_the_decode(tiny, canvas, dev):
    """tile_batch 1, 2 and 8: the blend's bits do not depend on the split (shown at kernel level above); the decoder may plan a
    batch of 2, 4 or 8 tiles differently, so the images are compared at FWD_TOL / 10."""
    net, _, _ = tiny
    z = canvas["z"].half().to(dev)
    outs = [net.vae_decode(z, which="image", tile_wrap=True, tile_batch=b, **KEYS) for b in (1, 2, 8)]
    for o in outs[:2]:
        err = rel_l2(o, outs[2])
        print("tile_batch against tile_batch=8: rel_l2 %.3e" % err)
        assert err < FWD_TOL / 10


def test_tiled_encode_vs_oracle(tiny, canvas, dev):
    from oracle import vd_oracle as O
    net, _, _ = tiny
    vae = net.vae["image"]
    im = canvas["im"].half().to(dev)
    post = vae.encode(im, out_posterior=True, tile_wrap=True, **KEYS)
    assert tuple(post.parameters.shape) == (2, 8, 8, 20)
    err = rel_l2(post.parameters, canvas["mom_wrap"])
    print("tiled encode moments (tiny, wrap, 4 tiles): rel_l2 %.3e" % err)
    assert err < FWD_TOL
    zref = O.diag_gaussian_sample(torch.from_numpy(canvas["mom_wrap"]), canvas["nz"].double()) * SCALE
    z = vae.encode_scaled(im, SCALE, noise=canvas["nz"], tile_wrap=True, **KEYS)
    assert tuple(z.shape) == (2, 4, 8, 20)
    err = rel_l2(z, zref)
    print("tiled encode_scaled (tiny, wrap, injected noise): rel_l2 %.3e" % err)
    assert err < FWD_TOL
    assert torch.equal(z, net.vae_encode(im, which="image", noise=canvas["nz"], tile_wrap=True, **KEYS))
    assert torch.equal(post.mode(), post.sample(torch.zeros(2, 4, 8, 20)))      # one posterior over the canvas: mode() is its mean


def test_identities(tiny, canvas, dev):
    net, _, _ = tiny
    vae = net.vae["image"]
    z, im = canvas["z"].half().to(dev), canvas["im"].half().to(dev)
    vae._tile_cache.clear()
    plain = vae.decode_scaled(z, 1.0 / SCALE)
    # no tile key: the call of before, in the same process
    assert torch.equal(net.vae_decode(z, which="image"), plain) and torch.equal(net.vae_decode(z, which="image", tile=None), plain)
    # a tile equal to the canvas without wrap is the plain call, whatever the other keys say
    assert torch.equal(net.vae_decode(z, which="image", tile=(8, 20), tile_weight="uniform", tile_batch=1), plain)
    assert not vae._tile_cache                                          # and builds no tables
    mom = vae.encode(im, out_posterior=True).parameters
    assert torch.equal(vae.encode(im, out_posterior=True, tile=(8, 20)).parameters, mom)
    assert torch.equal(vae.encode_scaled(im, SCALE, noise=canvas["nz"], tile=(8, 20), tile_stride=3),
                       vae.encode_scaled(im, SCALE, noise=canvas["nz"]))
    # two calls with the same keys: the same bits, one cached set of tables
    a = net.vae_decode(z, which="image", tile_wrap=True, **KEYS)
    b = net.vae_decode(z, which="image", tile_wrap=True, **KEYS)
    assert torch.equal(a, b) and len(vae._tile_cache) == 1
    ma = vae.encode(im, out_posterior=True, tile_wrap=True, **KEYS).parameters
    assert torch.equal(ma, vae.encode(im, out_posterior=True, tile_wrap=True, **KEYS).parameters) and len(vae._tile_cache) == 2
    # the other weights run too and differ from the tent
    for weight in ("uniform", "gaussian"):
        o = net.vae_decode(z, which="image", tile_wrap=True, tile_weight=weight, **KEYS)
        assert bool(torch.isfinite(o).all()) and not torch.equal(o, a)


def test_no_seam_under_wrap(tiny, dev):
    """With tile_wrap, decoding a latent rolled by one stride gives the image rolled by f strides: x = 0 is no special column.
    Both decodes lie within FWD_TOL of references that are equal (tests/test_tile_vae_cpu.py's roll test).  A roll by one stride
    moves tiles onto tiles only on a canvas whose width the stride divides, so this test runs on the 8 x 24 canvas of that CPU
    test (on 8 x 20 the tiles at x = 18 and x = 0 lie 2 apart and the rolled call is another tiling: 5.7e-2 on the oracle).
    Counter-check that the test can fail: the plain whole-canvas decode of the same pair does have a seam."""
    net, sd, kw = tiny
    z = torch.randn((2, 4, 8, 24), generator=torch.Generator().manual_seed(22)).half()
    zr = torch.roll(z, 6, dims=3)
    a = net.vae_decode(z.to(dev), which="image", tile_wrap=True, **KEYS)
    b = net.vae_decode(zr.to(dev), which="image", tile_wrap=True, **KEYS)
    err = rel_l2(torch.roll(b, -12, dims=3), a)
    pa = net.vae_decode(z.to(dev), which="image")
    pb = net.vae_decode(zr.to(dev), which="image")
    gap = rel_l2(torch.roll(pb, -12, dims=3), pa)
    print("seam: tiled+wrap rel_l2 %.3e, plain whole-canvas decode %.3e" % (err, gap))
    assert tuple(a.shape) == (2, 3, 16, 48) and err < FWD_TOL
    assert gap > FWD_TOL


# ---- 3. full width ---------------------------------------------------------------------------------------------------------

def test_full_width_tiled_decode_vs_oracle(dev):
    """KL-f8 at full width (f = 8, mid attention at C = 512), small tiles so the oracle stays cheap: canvas latent 16 x 40, tile 16,
    stride 12, wrap -- four 16 x 16 tiles, the last across the seam."""
    from lib.cfg_helper import model_cfg_bank
    from lib.model_zoo import get_model
    cfg = model_cfg_bank()("autokl_v1")
    cfg.pop("pth", None)
    vae = get_model()(cfg, verbose=False)
    sd = {"vae.image." + k: v for k, v in synth_into(vae, 7).items()}
    vae = vae.half().to(dev)
    assert vae.factor == 8
    g = tc.geometry(16, 40, 16, 12, True, "tent", f=8)
    assert g["offs"].tolist() == [[0, 0], [0, 12], [0, 24], [0, 36]]
    z = torch.randn((1, 4, 16, 40), generator=torch.Generator().manual_seed(9))
    ref = tc.tiled_decode_ref(sd, z / SCALE, g)
    dec = vae.decode_scaled(z.half().to(dev), 1.0 / SCALE, tile=16, tile_stride=12, tile_wrap=True)
    assert tuple(dec.shape) == (1, 3, 128, 320)
    err = rel_l2(dec, ref)
    print("tiled decode (full width, 4 tiles of 16 x 16): rel_l2 %.3e" % err)
    assert err < FWD_TOL
