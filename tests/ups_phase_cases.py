"""Cases, operands and CPU models of the phase form of the upsample convolution (vd_conv3x3_ups_phase_f16).

conv3x3(nearest_2x(x), w) == four 2x2 convolutions of x with weights summed per output phase (vd_hip/pack.py:
pack_conv_weight_ups_phase).  tests/test_ups_phase_cpu.py checks the algebra, the index maps of the TAPS = 4 instances of
conv3x3_halo_kernel and the preconditions of the exact cases without a GPU; tests/test_ups_phase_gpu.py runs the kernels.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from vdtest_util import exact_ints, exact_operand

# taps (0..2 for offsets -1..+1) of the 3x3 kernel that read source tap p of output phase a: upsampled row 2i + a + k - 1 is
# source row i + a - 1 + p
R_SETS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}

# name: B, low-resolution H x W, Cin, Cout, forced split (0 = the launcher's choice), what it exercises
CASES = {
    "a_small_images": dict(B=4, H=8, W=8, Cin=64, Cout=160, split=0),       # whole small images per patch, one chunk
    "b_seams_borders": dict(B=1, H=32, W=32, Cin=128, Cout=320, split=0),   # patch seams inside an image, 2 chunks, 2 column tiles
    "c_split_chunks": dict(B=2, H=16, W=16, Cin=256, Cout=320, split=2),    # split over chunks: slabs + the reduce launch
    "d_vae_128": dict(B=1, H=16, W=16, Cin=128, Cout=128, split=0),         # the VAE tile (256 x 128 blocks)
    "d_vae_256": dict(B=1, H=16, W=16, Cin=128, Cout=256, split=0),
}


def pack_phase_def(w, r_sets=R_SETS, swap_ab=False):
    """The definition, term by term, in the dtype of w (float64 in the tests): Wph[a][b][n][p][q][c]."""
    co, ci = w.shape[:2]
    out = torch.zeros((2, 2, co, 2, 2, ci), dtype=w.dtype)
    for a in (0, 1):
        for b in (0, 1):
            for p in (0, 1):
                for q in (0, 1):
                    acc = torch.zeros((co, ci), dtype=w.dtype)
                    for ky in r_sets[a, p]:
                        for kx in r_sets[b, q]:
                            acc = acc + w[:, :, ky, kx]
                    if swap_ab:
                        out[b, a, :, p, q, :] = acc
                    else:
                        out[a, b, :, p, q, :] = acc
    return out


def phase_conv(x_nhwc, wph, origin=-1):
    """The phase form on float64 tensors: out[n, 2i + a, 2j + b, :] = sum_{p, q} wph[a, b, :, p, q, :] . x[n, i + a + origin + p,
    j + b + origin + q, :], zero outside the image.  wph [2, 2, Co, 2, 2, Ci] (or the packed [4, Co, 4 Ci])."""
    B, H, W, C = x_nhwc.shape
    wph = wph.double().reshape(2, 2, -1, 2, 2, C)
    co = wph.shape[2]
    x = x_nhwc.double()
    xp = F.pad(x, (0, 0, 2, 2, 2, 2))   # two zero pixels on every side
    out = torch.zeros((B, 2 * H, 2 * W, co), dtype=torch.float64)
    for a in (0, 1):
        for b in (0, 1):
            acc = torch.zeros((B, H, W, co), dtype=torch.float64)
            for p in (0, 1):
                for q in (0, 1):
                    oy, ox = 2 + a + origin + p, 2 + b + origin + q
                    acc = acc + xp[:, oy:oy + H, ox:ox + W, :] @ wph[a, b, :, p, q, :].t()
            out[:, a::2, b::2, :] = acc
    return out


def upsampled_conv(x_nhwc, w):
    """float64 conv2d(interpolate(x, 2, 'nearest'), w, padding=1), channels-last."""
    x = F.interpolate(x_nhwc.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    return F.conv2d(x, w.double(), None, padding=1).permute(0, 2, 3, 1).contiguous()


def _seed(name):
    return 7000 + 100 * list(CASES).index(name)


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """Integer operands ({-1, 0, 0, +1} inputs and weights, bias in -8 .. 8): every product, every sum of up to four weights and
    every partial sum is an integer far below 2^24, so fp32 accumulation is exact in any order and both forms give the same bits."""
    c, s = CASES[name], _seed(name)
    t = SimpleNamespace(case=c, x=exact_operand((c["B"], c["H"], c["W"], c["Cin"]), s + 1),
                        w=exact_operand((c["Cout"], c["Cin"], 3, 3), s + 2), bias=exact_ints((c["Cout"],), s + 3))
    t.ref = upsampled_conv(t.x, t.w) + t.bias.double()
    return t


@functools.lru_cache(maxsize=None)
def random_case(name):
    """Normal inputs, fan-in-scaled normal weights (fp16 storage); the reference is float64 on the fp16 values."""
    c, s = CASES[name], _seed(name)
    g = torch.Generator(device="cpu").manual_seed(s + 11)
    t = SimpleNamespace(case=c, x=torch.randn((c["B"], c["H"], c["W"], c["Cin"]), generator=g).half(),
                        w=(torch.randn((c["Cout"], c["Cin"], 3, 3), generator=g) / (9 * c["Cin"]) ** 0.5).half(),
                        bias=(torch.randn((c["Cout"],), generator=g) * 0.1).half())
    t.ref = upsampled_conv(t.x, t.w) + t.bias.double()
    return t


# ---- index model of the TAPS = 4 instances (conv_ups_phase.hip: phase_geometry; conv_halo_kernel.h) ------------------------------
BM = 256
OOB = -1


def phase_geometry(nimg, Hl, Wl, BM=BM):
    tw = 32 if Wl % 32 == 0 else 16 if Wl % 16 == 0 else 8 if Wl % 8 == 0 else 0
    if tw == 0:
        return None
    th = BM // tw
    if Hl % th == 0:
        ngrp, rg = 1, th
    elif th % Hl == 0 and tw == Wl and (Hl & (Hl - 1)) == 0 and nimg % (th // Hl) == 0:
        ngrp, rg = th // Hl, Hl
    else:
        return None
    g = dict(tw=tw, ltw=tw.bit_length() - 1, rg=rg, ngrp=ngrp, lgsz=(tw * rg).bit_length() - 1, pitch=tw + 1, Hv=Hl, Wv=Wl, nimg=nimg)
    g["gpx"] = (rg + 1) * g["pitch"]
    g["hpx"] = ngrp * g["gpx"]
    if g["hpx"] > BM * 100 // 64 + 16:
        return None
    g["mg_pitch"] = (1 << 20) // g["pitch"] + 1
    g["mg_gpx"] = (1 << 20) // g["gpx"] + 1
    g["tiles_x"] = Wl // tw
    g["tiles_y"] = Hl // rg if ngrp == 1 else 1
    g["halo_bytes"] = ((g["hpx"] + 7) // 8) * 1024
    g["tiles_low"] = nimg * Hl * Wl // BM
    g["tiles_m"] = 4 * g["tiles_low"]
    return g


def block_of(g, tm_all):
    """(phase, low-resolution patch) of a row tile: phase slowest."""
    phase = tm_all // (g["tiles_m"] >> 2)
    return phase, tm_all - phase * (g["tiles_m"] >> 2)


def patch_origin(g, tm):
    if g["ngrp"] == 1:
        tpi = g["tiles_x"] * g["tiles_y"]
        img0 = tm // tpi
        r = tm - img0 * tpi
        ty = r // g["tiles_x"]
        return img0, ty * g["rg"], (r - ty * g["tiles_x"]) * g["tw"]
    return tm * g["ngrp"], 0, 0


def build_halo_image(g, tm_all, NW=8, origin=-1, TAPS=4):
    """LDS halo buffer as the DMA pieces of a block write it: [halo pixel][physical slot] -> (source pixel or OOB, logical slot)."""
    phase, tm = block_of(g, tm_all)
    pa, pb = phase >> 1, phase & 1
    img0, y0, x0 = patch_origin(g, tm)
    npieces = g["halo_bytes"] // 1024
    lds = np.full((npieces * 8, 8, 2), -7, dtype=np.int64)      # -7 = never written
    HPXMAX = BM * 100 // 64 + 16
    NHP = (HPXMAX + 7) // 8
    HPW = (NHP + NW - 1) // NW
    HPT = (HPW + TAPS - 2) // (TAPS - 1)
    MAXHP = HPT * (TAPS - 1)
    for wave in range(NW):
        for j in range(MAXHP):
            q = j * NW + wave
            if not (q * 8 < g["hpx"]):
                continue
            assert j // HPT < TAPS - 1, "a piece of the next chunk must be issued before the last tap"
            for lane in range(64):
                hp = q * 8 + (lane >> 3)
                grp = (hp * g["mg_gpx"]) >> 20
                rem = hp - grp * g["gpx"]
                hy = (rem * g["mg_pitch"]) >> 20
                hx = rem - hy * g["pitch"]
                if hp < g["hpx"]:
                    assert grp == hp // g["gpx"] and hy == rem // g["pitch"]
                vy, vx = y0 + hy + pa + origin, x0 + hx + pb + origin
                ok = hp < g["hpx"] and 0 <= vy < g["Hv"] and 0 <= vx < g["Wv"]
                pix = ((img0 + grp) * g["Hv"] + vy) * g["Wv"] + vx
                slot = (lane & 7) ^ ((hp >> 1) & 7)
                assert q * 1024 + lane * 16 == hp * 128 + (lane & 7) * 16
                lds[hp, lane & 7] = (pix, slot) if ok else (OOB, slot)
    return lds, (phase, img0, y0, x0)


def check_fragments(g, tm_all, WM=32, origin=-1):
    """Every operand fragment a lane reads for (tap, k-step) is x[i + a - 1 + p][j + b - 1 + q] of its output pixel's source
    pixel (i, j), or zeros exactly where that index lies outside the image.  Returns the number of padded reads."""
    MI = WM // 32
    lds, (phase, img0, y0, x0) = build_halo_image(g, tm_all, origin=origin)
    pa, pb = phase >> 1, phase & 1
    assert (lds[: g["hpx"], :, 0] != -7).all(), "every halo pixel of the patch must be written by some piece"
    padded = 0
    for wm in range(BM // WM):
        for i in range(MI):
            for l31 in range(32):
                m = wm * WM + i * 32 + l31
                grp = m >> g["lgsz"]
                r = m - (grp << g["lgsz"])
                hp_base = grp * g["gpx"] + (r >> g["ltw"]) * g["pitch"] + (r & (g["tw"] - 1))
                iy, ix = y0 + (r >> g["ltw"]), x0 + (r & (g["tw"] - 1))       # low-resolution pixel of this lane
                for t in range(4):
                    p, q = t >> 1, t & 1
                    hp = hp_base + p * g["pitch"] + q
                    for hi in range(2):
                        a0 = (hp << 7) + ((((hp >> 1) & 7) ^ hi) << 4)
                        for ks in range(4):
                            addr = a0 ^ (ks << 5)
                            src, slot = lds[addr >> 7, (addr >> 4) & 7]
                            assert slot == 2 * ks + hi, "lane must receive k-slice 2 ks + hi of the 64-channel chunk"
                            vy, vx = iy + pa - 1 + p, ix + pb - 1 + q
                            inside = 0 <= vy < g["Hv"] and 0 <= vx < g["Wv"]
                            want = ((img0 + grp) * g["Hv"] + vy) * g["Wv"] + vx if inside else OOB
                            assert src == want, (tm_all, m, t, hi, ks)
                            padded += 0 if inside else 1
    return padded


def out_rows(g, tm_all, swap_ab=False):
    """Output row (pixel index over [image][2 Hl][2 Wl]) of each of the block's BM tile rows."""
    phase, tm = block_of(g, tm_all)
    pa, pb = (phase & 1, phase >> 1) if swap_ab else (phase >> 1, phase & 1)
    img0, y0, x0 = patch_origin(g, tm)
    m = np.arange(BM)
    grp = m >> g["lgsz"]
    r = m - (grp << g["lgsz"])
    return ((img0 + grp) * 2 * g["Hv"] + 2 * (y0 + (r >> g["ltw"])) + pa) * 2 * g["Wv"] + 2 * (x0 + (r & (g["tw"] - 1))) + pb


def stat_partials(g, tm_all):
    """[(partial index, tile rows of the sub-block)] a block writes to out_stats: index 4 (low-resolution sub-block) + phase."""
    phase, tm = block_of(g, tm_all)
    nsub, R = g["ngrp"], BM // g["ngrp"]
    return [((tm * nsub) * 4 + phase + 4 * s, np.arange(s * R, (s + 1) * R)) for s in range(nsub)]
