"""Case table of the exact (tolerance-free) tests of the MFMA GEMM and convolution kernels.

Every operand is a small integer (vdtest_util.exact_operand / exact_ints), so each product and each partial sum is an exactly
representable integer in whatever order a kernel adds them: the output must equal the float64 reference in every element.
tests/test_exact_linear_cpu.py checks the preconditions of every row without a GPU; tests/test_exact_linear_gpu.py runs the
kernels.  Shapes are the smallest at which each path can still go wrong (ragged tiles, patch seams, split boundaries); none is a
workload shape.  build(name) draws the operands and computes the reference once per process.
"""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from vdtest_util import exact_ints, exact_operand

CASES = {}


def _add(name, family, kind, **kw):
    assert name not in CASES, name
    CASES[name] = dict(name=name, family=family, kind=kind, **kw)


def _gemm(name, family, M, N, K, k1=0, bias=True, rpb=0, res=True, **kw):
    _add(name, family, "gemm", M=M, N=N, K=K, k1=k1, bias=bias, rpb=rpb, res=res, **kw)


def _conv(name, family, B, H, W, c0, c1, Co, ks=3, stride=1, pad=1, pad_hi=None, ups=0, rv=False, res=False, img_const=False, **kw):
    _add(name, family, "conv", B=B, H=H, W=W, c0=c0, c1=c1, Co=Co, ks=ks, stride=stride, pad=pad, pad_hi=pad_hi, ups=ups, rv=rv,
         res=res, img_const=img_const, **kw)


# ---- gemm_f16_kernel ---------------------------------------------------------------------------------------------------------
# M above the tallest tile and ragged, N a multiple of 8 but of no tile width, K no multiple of 64
_gemm("gemm_ragged", "gemm_f16", 300, 328, 200, rpb=150)
_gemm("gemm_two_source", "gemm_f16", 130, 72, 192, k1=64, bias=False, res=False)
_gemm("gemm_width_100", "gemm_f16", 300, 100, 64, rpb=150)    # widths that are no multiple of 8 / of 4: the element-wise tail
_gemm("gemm_width_102", "gemm_f16", 300, 102, 64, rpb=150)
_gemm("gemm_split_k", "gemm_f16", 130, 72, 64 * 33, splits=(2, 5, 32))
_add("bgemm_alpha_f32", "gemm_f16", "bgemm", form="alpha_f32", Bt=3, M=200, N=136, K=128, alpha=0.25)
_add("bgemm_shared_a_bias_m", "gemm_f16", "bgemm", form="shared_a", Bt=3, M=200, N=136, K=128, alpha=1.0)
_add("bgemm_split_k", "gemm_f16", "bgemm", form="split", Bt=3, M=200, N=136, K=128, alpha=1.0, split=2)
# implicit convolution on gemm_f16_kernel (vd_conv_halo_set_variant(0))
_conv("iconv_17x13", "gemm_f16", 1, 17, 13, 64, 0, 72)
_conv("iconv_stride2", "gemm_f16", 1, 32, 32, 64, 0, 64, stride=2)
_conv("iconv_stride2_pad_hi", "gemm_f16", 1, 16, 16, 64, 0, 64, stride=2, pad=0, pad_hi=1)
_conv("iconv_upsample", "gemm_f16", 2, 8, 8, 128, 0, 64, ups=1)
_conv("iconv_concat_3x3", "gemm_f16", 2, 16, 16, 128, 64, 128, rv=True, res=True)
_conv("iconv_concat_1x1", "gemm_f16", 2, 16, 16, 128, 64, 128, ks=1, pad=0, rv=True, res=True)

# ---- conv3x3_halo_kernel -----------------------------------------------------------------------------------------------------
# planner: whether vd_conv_halo_set_variant(-1) sends the case to the halo kernel (>= 32 tiles and a width 160 or 128 divides);
# the forced variants (3, 6, 13) take every one of them
_conv("halo_32wide_tiles_xy", "halo", 1, 32, 64, 64, 0, 160, res=True, planner=False)         # 8 patches of 8 x 32: 2 in x, 4 in y
_conv("halo_16wide", "halo", 2, 16, 16, 128, 0, 128, planner=False)
_conv("halo_upsample", "halo", 2, 8, 8, 128, 0, 128, ups=1, planner=False)
# four whole 8x8 images per patch; a distinct constant per image, so a halo row read from the neighbouring image cannot cancel
_conv("halo_8wide_four_images", "halo", 8, 8, 8, 128, 64, 160, rv=True, res=True, img_const=True, planner=False)
_conv("halo_three_patches_per_row", "halo", 1, 96, 96, 64, 0, 160, planner=True)
_conv("halo_ragged_columns", "halo", 2, 64, 32, 64, 0, 72, planner=False)
_conv("halo_split_3_chunks", "halo", 2, 16, 16, 192, 0, 160, split_k=2, planner=False)         # 2 + 1 chunks: a ragged split
_conv("halo_split_planner", "halo", 2, 16, 16, 640, 0, 320, planner=False)                     # 10 chunks, the planner's split
_add("halo_skip_fewer_chunks_than_splits", "halo", "skipconv", B=2, H=64, C=320, cs0=64, cs1=64, stream=False)
_add("halo_skip_single_source", "halo", "skipconv", B=2, H=32, C=640, cs0=320, cs1=0, stream=False)

# ---- conv3x3_wstream_kernel / conv3x3_wsk_kernel (8x8 images) ------------------------------------------------------------------
_conv("wstream_2_chunks", "wstream_conv", 2, 8, 8, 128, 0, 256)
_conv("wstream_3_chunks", "wstream_conv", 6, 8, 8, 192, 0, 256, rv=True, res=True)
_conv("wstream_5_chunks_two_sources", "wstream_conv", 4, 8, 8, 192, 128, 512)
_conv("wstream_4_chunks", "wstream_conv", 2, 8, 8, 256, 0, 256, rv=True, res=True)
_add("wstream_skip", "wstream_conv", "skipconv", B=4, H=8, C=256, cs0=64, cs1=64, stream=True)

# ---- gemm_wstream_kernel -------------------------------------------------------------------------------------------------------
_gemm("gemm_wstream_1_chunk", "gemm_wstream", 128, 256, 64, split=0)
_gemm("gemm_wstream_33_chunks", "gemm_wstream", 128, 256, 2112, split=0)    # one more chunk than the kernel unrolls: must split
_gemm("gemm_wstream_split_2", "gemm_wstream", 384, 256, 4096, split=2)

# ---- rowgemm320_kernel ---------------------------------------------------------------------------------------------------------
for _n in (320, 960):
    for _r in (False, True):
        _gemm("row320_n%d%s" % (_n, "_res" if _r else ""), "row320", 128 * 3 + 5, _n, 320, res=_r)

FAMILIES = ("gemm_f16", "halo", "wstream_conv", "gemm_wstream", "row320")


def names(family=None, kind=None):
    return [n for n, c in CASES.items() if (family is None or c["family"] == family) and (kind is None or c["kind"] == kind)]


def _seed(name):
    return 1000 * (1 + list(CASES).index(name))


def conv_ref(x_nhwc, w, stride, pad, ups, pad_hi=None):
    """float64 convolution in the formulation of the tolerance tests: nearest 2x upsampling or asymmetric padding, then F.conv2d."""
    x = x_nhwc.double().permute(0, 3, 1, 2)
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if pad_hi is not None:
        x = F.pad(x, (pad, pad_hi, pad, pad_hi))
        y = F.conv2d(x, w.double(), None, stride=stride)
    else:
        y = F.conv2d(x, w.double(), None, stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).contiguous()


def _build_gemm(c, s):
    M, N, K, k1 = c["M"], c["N"], c["K"], c["k1"]
    t = SimpleNamespace(a0=exact_operand((M, K - k1), s + 1), a1=exact_operand((M, k1), s + 2) if k1 else None,
                        w=exact_operand((N, K), s + 3), bias=exact_ints((N,), s + 4) if c["bias"] else None,
                        rowvec=exact_ints((M // c["rpb"], N), s + 5) if c["rpb"] else None,
                        res=exact_ints((M, N), s + 6) if c["res"] else None, unit=1.0)
    a = torch.cat([t.a0, t.a1], 1) if k1 else t.a0
    ref = a.double() @ t.w.double().t()
    t.ref_plain = ref.clone()
    if t.bias is not None:
        ref = ref + t.bias.double()
    t.ref_bias = ref.clone()
    if t.rowvec is not None:
        ref = ref + t.rowvec.double().repeat_interleave(c["rpb"], 0)
    if t.res is not None:
        ref = ref + t.res.double()
    t.ref = ref
    return t


def _build_bgemm(c, s):
    Bt, M, N, K = c["Bt"], c["M"], c["N"], c["K"]
    t = SimpleNamespace(w=exact_operand((Bt, N, K), s + 2), unit=c["alpha"])
    if c["form"] == "shared_a":     # out[b] = A W[b]^T + bias[:, None]   (V^T = Wv x^T + bv)
        t.a = exact_operand((M, K), s + 3)
        t.bias = exact_ints((M,), s + 4)
        t.ref = torch.einsum("mk,bnk->bmn", t.a.double(), t.w.double()) + t.bias.double().view(1, M, 1)
    else:
        t.a = exact_operand((Bt, M, K), s + 1)
        t.bias = None
        t.ref = torch.einsum("bmk,bnk->bmn", t.a.double(), t.w.double()) * c["alpha"]
    return t


def _build_conv(c, s):
    B, H, W, c0, c1, Co, ks = c["B"], c["H"], c["W"], c["c0"], c["c1"], c["Co"], c["ks"]
    t = SimpleNamespace(x=exact_operand((B, H, W, c0), s + 1), x1=exact_operand((B, H, W, c1), s + 2) if c1 else None,
                        w=exact_operand((Co, c0 + c1, ks, ks), s + 3), bias=exact_ints((Co,), s + 4), unit=1.0)
    if c["img_const"]:   # -4 .. 3 over eight images (fp16 integers still)
        k = (torch.arange(B) % 8 - 4).view(B, 1, 1, 1)
        t.x = (t.x.float() + k).half()
        t.x1 = (t.x1.float() - k).half() if c1 else None
    ref = conv_ref(torch.cat([t.x, t.x1], -1) if c1 else t.x, t.w, c["stride"], c["pad"], c["ups"], c["pad_hi"]) + t.bias.double()
    _, Ho, Wo, _ = ref.shape
    t.rows_per_image = Ho * Wo
    t.rowvec = exact_ints((B, Co), s + 5) if c["rv"] else None
    t.res = exact_ints((B, Ho, Wo, Co), s + 6) if c["res"] else None
    if t.rowvec is not None:
        ref = ref + t.rowvec.double().view(B, 1, 1, Co)
    if t.res is not None:
        ref = ref + t.res.double()
    t.ref = ref
    return t


def _build_skipconv(c, s):
    """ResBlock's conv3x3(h) + bias + conv1x1(cat(s0, s1)): the reference of the folded skip convolution."""
    B, H, C, cs0, cs1 = c["B"], c["H"], c["C"], c["cs0"], c["cs1"]
    t = SimpleNamespace(h=exact_operand((B, H, H, C), s + 1), s0=exact_operand((B, H, H, cs0), s + 2),
                        s1=exact_operand((B, H, H, cs1), s + 3) if cs1 else None, w3=exact_operand((C, C, 3, 3), s + 4),
                        w1=exact_operand((C, cs0 + cs1), s + 5), bias=exact_ints((C,), s + 6), unit=1.0)
    xs = torch.cat([t.s0, t.s1], -1) if cs1 else t.s0
    t.ref = (conv_ref(t.h, t.w3, 1, 1, 0) + t.bias.double()
             + (xs.double().reshape(-1, cs0 + cs1) @ t.w1.double().t()).view(B, H, H, C))
    return t


_BUILDERS = {"gemm": _build_gemm, "bgemm": _build_bgemm, "conv": _build_conv, "skipconv": _build_skipconv}


@functools.lru_cache(maxsize=None)
def build(name):
    """Operands (CPU fp16) and the float64 reference `ref` of a case; computed once per process and shared -- do not modify."""
    c = CASES[name]
    t = _BUILDERS[c["kind"]](c, _seed(name))
    t.case = c
    return t
