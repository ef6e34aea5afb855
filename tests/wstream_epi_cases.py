"""Operands for the tests of vd_gemm_wstream_epi_f16 (tests/test_wstream_epi_cpu.py, tests/test_wstream_epi_gpu.py): the
weight-streaming GEMM with the fused epilogue against gemm_f16_kernel on the same operands.

Epilogues: "bias" (no fold), "table" (LayerNorm fold, (mean, rstd) rows from vd_row_stats_f16), "sums" (fold, the producer's int64
fixed-point row sums), each plain and with GEGLU.  Integer cases: A small sparse integers, W in {-1, 0, 1} and sparse, bias small
integers -- every product and partial sum is an integer far below 2^24, exact in fp32 in any order, so both kernels hold the same
accumulators and whatever follows is the epilogue alone.  Normal cases: unit-variance rows with a per-row offset, fan-in-scaled
weights, a float64 reference of the folded form on the same fp16 operands."""
import itertools

import torch

MS = (128, 256, 384)
KS = (64, 128, 192, 1280, 1984, 2048)      # 1, 2, 3, 20, 31, 32 chunks: the prologue preloads two; the wait count changes at 31 -> 32
NS = (256, 384, 512, 768)                  # 384: the last block's waves 2 and 3 lie past N
EPILOGUES = tuple(itertools.product(("bias", "table", "sums"), ("none", "geglu")))
LN_EPS = 1e-5
SUM_SCALE, SQ_SCALE = 2.0 ** 24, 2.0 ** 16   # VdGemmDesc.row_sums: sum x 2^24, sum of squares x 2^16


def grid():
    """(M, N, K, fold, act): every K with every epilogue, M and N cycling so that each value meets each K and each epilogue kind."""
    out = []
    for ki, K in enumerate(KS):
        for ei, (fold, act) in enumerate(EPILOGUES):
            out.append((MS[(ki + ei) % 3], NS[(ki * 6 + ei + ki // 2) % 4], K, fold, act))
    return out


def _sparse_int(g, shape, lim, keep):
    v = torch.randint(-lim, lim + 1, shape, generator=g).double()
    return v * (torch.rand(shape, generator=g) < keep).double()


def row_sums_fixed(a):
    """int64 [M, 2] = (sum x 2^24, sum of squares x 2^16) of the rows of `a`, as a producer launch accumulates them."""
    a = a.double()
    return torch.stack([(a.sum(1) * SUM_SCALE).round(), ((a * a).sum(1) * SQ_SCALE).round()], 1).to(torch.int64).contiguous()


def integer_case(M, N, K, seed):
    """(a [M, K], w [N, K], bias [N]) fp16 with integer values; |a| w^T stays below 1024, so the plain output and half of it are
    exact in fp16."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = _sparse_int(g, (M, K), 2, 0.25)
    w = _sparse_int(g, (N, K), 1, 0.125)
    b = _sparse_int(g, (N,), 3, 1.0)
    assert (a.abs() @ w.abs().t()).max() + 3 < 1024
    return a.half(), w.half(), b.half()


def normal_case(M, N, K, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = (torch.randn((M, K), generator=g) + 0.5 * torch.randn((M, 1), generator=g)).half()
    w = (torch.randn((N, K), generator=g) / K ** 0.5).half()
    b = (0.1 * torch.randn((N,), generator=g)).half()
    return a, w, b


def colsum_of(w):
    return w.float().sum(1).contiguous()


def reference(a, w, b, fold, act, alpha=1.0):
    """float64 value of the launch on the fp16 operands: y = rstd (a w^T - mean colsum) + b with the fold (biased variance, LN_EPS;
    for "sums" from the fixed-point sums, as the kernel decodes them), a w^T + b without; GEGLU pairs per 64 packed rows [32 value |
    32 gate]; times alpha."""
    a64, w64 = a.double(), w.double()
    y = a64 @ w64.t()
    if fold != "bias":
        K = a.shape[1]
        if fold == "sums":
            s = row_sums_fixed(a).double()
            mean = s[:, 0] / SUM_SCALE / K
            var = (s[:, 1] / SQ_SCALE / K - mean * mean).clamp_min(0.0)
        else:
            mean = a64.mean(1)
            var = ((a64 - mean[:, None]) ** 2).mean(1)
        rstd = (var + LN_EPS).rsqrt()
        y = rstd[:, None] * (y - mean[:, None] * w64.sum(1)[None, :])
    y = y + b.double()[None, :]
    if act == "geglu":
        y = y.view(a.shape[0], -1, 2, 32)
        v, gt = y[:, :, 0, :], y[:, :, 1, :]
        y = (v * 0.5 * gt * (1.0 + torch.erf(gt * 0.5 ** 0.5))).reshape(a.shape[0], -1)
    return y * alpha
