"""The phase form of the upsample convolution, without a GPU: the weight pack against its definition, the algebra against
conv2d(interpolate(x)), the index maps of the TAPS = 4 instances of conv3x3_halo_kernel, and the preconditions of the exact GPU
cases.  Each check is also run with a deliberate mistake (a wrong R set, the two phase indices swapped, the window origin off by
one) that it has to catch.  torch / numpy only.
"""
import numpy as np
import pytest
import torch

import ups_phase_cases as U
from vd_hip.pack import UPS_PHASE_TAPS, pack_conv_weight_ups_phase
from vdtest_util import check_exact_reference


def _w64(co, ci, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((co, ci, 3, 3), generator=g, dtype=torch.float64)


def _x64(B, H, W, C, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((B, H, W, C), generator=g, dtype=torch.float64)


def test_r_sets_are_the_definition():
    assert UPS_PHASE_TAPS == U.R_SETS
    # derived: tap k (offset k - 1) of upsampled row 2i + a reads source row floor((2i + a + k - 1) / 2) = i + a - 1 + p
    for a in (0, 1):
        for p in (0, 1):
            assert tuple(k for k in range(3) if (a + k - 1) // 2 == a - 1 + p) == U.R_SETS[a, p]


def test_pack_equals_definition_float64():
    w = _w64(24, 16, 1)
    got = pack_conv_weight_ups_phase(w)            # float64 in, float64 out: no rounding in the way
    assert got.dtype == torch.float64 and got.shape == (4, 24, 4 * 16)
    want = U.pack_phase_def(w)
    for a in (0, 1):
        for b in (0, 1):
            assert torch.allclose(got[2 * a + b].reshape(24, 2, 2, 16), want[a, b], rtol=0, atol=1e-15), (a, b)
    # every 3x3 tap lands in exactly one (p, q) of every phase: the phase weights sum to the kernel's sum
    assert torch.allclose(got.reshape(4, 24, 4, 16).sum(2), w.sum((2, 3))[None].expand(4, -1, -1), rtol=0, atol=1e-13)


def test_pack_rounds_fp16_sums_once():
    g = torch.Generator(device="cpu").manual_seed(5)
    w = (torch.randn((8, 64, 3, 3), generator=g) * 0.05).half()
    got = pack_conv_weight_ups_phase(w)
    assert got.dtype == torch.float16
    want = U.pack_phase_def(w.double()).reshape(4, 8, 256)
    assert torch.equal(got, want.float().half())    # fp32 sums of up to four fp16 values are exact; one rounding to fp16


def test_pack_is_cached_and_rebuilt_after_a_weight_change():
    from lib.model_zoo.hip_layers import Conv2d
    conv = Conv2d(64, 32, 3, padding=1)
    p0 = conv._w_phase()
    assert p0.shape == (4, 32, 256) and p0.dtype == torch.float16
    assert conv._w_phase() is p0                      # built on first use, then served from the cache
    with torch.no_grad():
        conv.weight.mul_(2.0)                          # an in-place edit bumps the parameter's version
    p1 = conv._w_phase()
    assert p1 is not p0 and torch.equal(p1, pack_conv_weight_ups_phase(conv.weight.detach().half()))
    assert not torch.equal(p1, p0)


@pytest.mark.parametrize("B,H,W,C,Co", [(1, 1, 1, 8, 4), (2, 2, 2, 8, 4), (1, 5, 7, 8, 6), (2, 8, 8, 64, 16)])
def test_phase_form_equals_upsampled_conv_float64(B, H, W, C, Co):
    """All four phases, the four borders and the corners, a 1x1 and a 2x2 low-resolution image."""
    x, w = _x64(B, H, W, C, 10 + H), _w64(Co, C, 20 + W)
    ref = U.upsampled_conv(x, w)
    got = U.phase_conv(x, pack_conv_weight_ups_phase(w))
    assert got.shape == ref.shape == (B, 2 * H, 2 * W, Co)
    tol = 1e-12 * ref.abs().max().item()
    for a in (0, 1):
        for b in (0, 1):
            assert (got[:, a::2, b::2] - ref[:, a::2, b::2]).abs().max().item() <= tol, "phase (%d, %d)" % (a, b)
    regions = {"top": (slice(0, 1), slice(None)), "bottom": (slice(-1, None), slice(None)), "left": (slice(None), slice(0, 1)),
               "right": (slice(None), slice(-1, None)), "corner00": (slice(0, 1), slice(0, 1)), "corner01": (slice(0, 1), slice(-1, None)),
               "corner10": (slice(-1, None), slice(0, 1)), "corner11": (slice(-1, None), slice(-1, None))}
    for name, (ys, xs) in regions.items():
        assert (got[:, ys, xs] - ref[:, ys, xs]).abs().max().item() <= tol, name


@pytest.mark.parametrize("B,H,W,C,Co", [(1, 1, 1, 8, 4), (2, 2, 2, 8, 4), (2, 6, 5, 16, 8)])
def test_integer_case_is_exact(B, H, W, C, Co):
    g = torch.Generator(device="cpu").manual_seed(H * 10 + W)
    x = torch.randint(-3, 4, (B, H, W, C), generator=g).half()
    w = torch.randint(-3, 4, (Co, C, 3, 3), generator=g).half()
    got = U.phase_conv(x, pack_conv_weight_ups_phase(w))       # fp16 pack: sums of up to four integers in -3 .. 3 are exact
    assert torch.equal(got, U.upsampled_conv(x, w))


@pytest.mark.parametrize("mistake", ["r_set", "swap_ab", "origin"])
def test_algebra_check_catches_mistakes(mistake):
    x, w = _x64(1, 4, 4, 8, 3), _w64(4, 8, 4)
    ref = U.upsampled_conv(x, w)
    if mistake == "r_set":
        bad = dict(U.R_SETS)
        bad[0, 1], bad[1, 0] = U.R_SETS[1, 0], U.R_SETS[0, 1]      # {0, 1} and {1, 2} exchanged
        got = U.phase_conv(x, U.pack_phase_def(w, r_sets=bad))
    elif mistake == "swap_ab":
        got = U.phase_conv(x, U.pack_phase_def(w, swap_ab=True))
    else:
        got = U.phase_conv(x, U.pack_phase_def(w), origin=0)
    assert (got - ref).abs().max().item() > 1e-3 * ref.abs().max().item()
    assert (U.phase_conv(x, U.pack_phase_def(w)) - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


# ---- index model ----------------------------------------------------------------------------------------------------------------
# (images, low-resolution H, W): the exact cases, the UNet's three upsample layers at the benchmark batch, the VAE decoder's three
GEOMETRIES = [(4, 8, 8), (1, 32, 32), (2, 16, 16), (1, 16, 16), (8, 32, 32), (8, 16, 16), (8, 8, 8), (1, 64, 64), (2, 128, 128),
              (1, 256, 256), (3, 64, 24)]


def _blocks(g, seed):
    rng = np.random.RandomState(seed)
    L = g["tiles_low"]
    picks = {0, g["tiles_m"] - 1, L - 1, L, 2 * L + L // 2, 3 * L}
    picks.update(int(v) for v in rng.randint(0, g["tiles_m"], 2))
    return sorted(picks)


@pytest.mark.parametrize("nimg,Hl,Wl", GEOMETRIES)
@pytest.mark.parametrize("WM", [32, 64])
def test_phase_halo_and_fragment_addresses(nimg, Hl, Wl, WM):
    g = U.phase_geometry(nimg, Hl, Wl)
    assert g is not None
    assert 2 * g["halo_bytes"] + 3 * 160 * 128 <= 160 * 1024
    for tm_all in _blocks(g, nimg + Hl):
        padded = U.check_fragments(g, tm_all, WM)
        # reads outside the image are exactly the padded ones: count them from the patch position
        phase, tm = U.block_of(g, tm_all)
        pa, pb = phase >> 1, phase & 1
        img0, y0, x0 = U.patch_origin(g, tm)
        want = 0
        for grp in range(g["ngrp"]):
            for iy in range(y0, y0 + g["rg"]):
                for ix in range(x0, x0 + g["tw"]):
                    for p in (0, 1):
                        for q in (0, 1):
                            vy, vx = iy + pa - 1 + p, ix + pb - 1 + q
                            want += 0 if (0 <= vy < Hl and 0 <= vx < Wl) else 1
        assert padded == want * 8          # 2 (hi) x 4 (k-steps) fragment reads per (pixel, tap)


def test_geometry_rejections():
    assert U.phase_geometry(1, 8, 8) is None        # four 8x8 images make a patch: one is not enough
    assert U.phase_geometry(2, 12, 12) is None      # no 8-pixel column tile


@pytest.mark.parametrize("nimg,Hl,Wl", [(8, 8, 8), (2, 16, 16), (1, 32, 32)])
def test_origin_off_by_one_is_caught(nimg, Hl, Wl):
    g = U.phase_geometry(nimg, Hl, Wl)
    for origin in (0, -2):
        with pytest.raises(AssertionError):
            U.check_fragments(g, 0, 32, origin=origin)


@pytest.mark.parametrize("nimg,Hl,Wl", GEOMETRIES)
def test_output_row_map_is_a_bijection(nimg, Hl, Wl):
    g = U.phase_geometry(nimg, Hl, Wl)
    M = nimg * 4 * Hl * Wl
    seen = np.zeros(M, dtype=np.int32)
    for tm_all in range(g["tiles_m"]):
        rows = U.out_rows(g, tm_all)
        # the row is pixel (2 y + a, 2 x + b) of the block's phase
        phase, _ = U.block_of(g, tm_all)
        y, x = (rows // (2 * Wl)) % (2 * Hl), rows % (2 * Wl)
        assert ((y & 1) == (phase >> 1)).all() and ((x & 1) == (phase & 1)).all()
        seen[rows] += 1
    assert (seen == 1).all()


def test_swapped_phase_indices_are_caught():
    """a and b exchanged in the output map alone still covers every pixel once: the phase test of the map is what catches it, and
    the values catch it in test_algebra_check_catches_mistakes."""
    g = U.phase_geometry(1, 32, 32)
    L = g["tiles_low"]
    rows = U.out_rows(g, L, swap_ab=True)          # phase 1 = (a, b) = (0, 1)
    y, x = (rows // 64) % 64, rows % 64
    assert not (((y & 1) == 0).all() and ((x & 1) == 1).all())


@pytest.mark.parametrize("nimg,Hl,Wl", GEOMETRIES)
def test_statistics_partials(nimg, Hl, Wl):
    """One partial per block (and whole small image) and channel; the consuming GroupNorm sees exactly HW / R partials per image,
    all of them rows of that image, and every output pixel is counted once."""
    g = U.phase_geometry(nimg, Hl, Wl)
    HW = 4 * Hl * Wl
    R = U.BM // g["ngrp"]
    T = HW // R
    owner = {}
    counted = np.zeros(nimg * HW, dtype=np.int32)
    for tm_all in range(g["tiles_m"]):
        rows = U.out_rows(g, tm_all)
        for idx, sub in U.stat_partials(g, tm_all):
            assert idx not in owner, "two blocks write the same partial"
            imgs = np.unique(rows[sub] // HW)
            assert len(imgs) == 1 and imgs[0] == idx // T, "a partial mixes images or lies in another image's run"
            assert len(sub) == R
            owner[idx] = tm_all
            counted[rows[sub]] += 1
    assert sorted(owner) == list(range(nimg * T))
    assert (counted == 1).all()


# ---- preconditions of the exact GPU cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.CASES))
def test_exact_case_preconditions(name):
    t = U.exact_case(name)
    c = t.case
    assert U.phase_geometry(c["B"], c["H"], c["W"]) is not None
    check_exact_reference(t.ref, 1.0, name)
    # every fp32 sum is exact: integers, and the sum of the magnitudes of all terms of an output stays below 2^24
    for v in (t.x, t.w, t.bias):
        assert torch.equal(v.double(), v.double().round())
    wph = pack_conv_weight_ups_phase(t.w)
    assert torch.equal(wph.double(), U.pack_phase_def(t.w.double()).reshape(wph.shape))      # the summed weights are fp16 values
    bound = 9 * c["Cin"] * t.x.abs().max().item() * t.w.abs().max().item() + t.bias.abs().max().item()
    assert bound < 2 ** 24
    # asymmetric operands: a transposed phase or tap must change the result
    assert not torch.equal(t.w, t.w.transpose(2, 3)) and not torch.equal(t.x, t.x.transpose(1, 2))
    assert torch.equal(U.phase_conv(t.x, wph) + t.bias.double(), t.ref)
    assert not torch.equal(U.phase_conv(t.x, U.pack_phase_def(t.w.double(), swap_ab=True)) + t.bias.double(), t.ref)
