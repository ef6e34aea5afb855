"""Operands for the tests of the feed-forward / proj_out fold (tests/test_ff_proj_fold_cpu.py, tests/test_ff_proj_fold_gpu.py).

The block tail   y = x2 + h W2^T + b2,   out = alpha (y Wp^T + bp) + r   against its merged form
out = alpha ([h | x2] [Wp W2 | Wp]^T + Wp b2 + bp) + r  (vd_hip/pack.py: pack_ff_proj_fold).

Integer cases: W2 and Wp in {-1, 0, 1} and sparse, h and x2 small integers, alpha a power of two.  Then every product and every
partial sum of either form is an integer far below 2^24 (exact in fp32 in any order), Wm = Wp W2 and y are integers below 2048
(exact in fp16), and both forms round ONE and the same real number to fp16: they agree bit for bit with each other and with the
float64 value rounded once.  Normal cases: fan-in-scaled weights, unit-variance activations."""
import collections

import torch

Tail = collections.namedtuple("Tail", "h x2 w2 b2 wp bp r alpha ref y")


def _sparse_int(g, shape, lim, keep):
    v = torch.randint(-lim, lim + 1, shape, generator=g).double()
    return v * (torch.rand(shape, generator=g) < keep).double()


def tail_ref(h, x2, w2, b2, wp, bp, r, alpha):
    """(out, y) of the two-line form in float64, nothing rounded."""
    y = x2.double() + h.double() @ w2.double().t() + b2.double()
    return alpha * (y @ wp.double().t() + bp.double()) + r.double(), y


def integer_tail(M, C, seed, alpha=0.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    h = _sparse_int(g, (M, 4 * C), 2, 0.25)
    x2 = _sparse_int(g, (M, C), 3, 0.5)
    w2 = _sparse_int(g, (C, 4 * C), 1, 0.125)
    wp = _sparse_int(g, (C, C), 1, 0.125)
    b2 = _sparse_int(g, (C,), 2, 1.0)
    bp = _sparse_int(g, (C,), 2, 1.0)
    r = _sparse_int(g, (M, C), 4, 1.0)
    ref, y = tail_ref(h, x2, w2, b2, wp, bp, r, alpha)
    t = Tail(*[v.half() for v in (h, x2, w2, b2, wp, bp, r)], alpha, ref, y)
    # the preconditions of exactness, checked where the case is made
    wm = wp @ w2
    assert wm.abs().max() <= 2048 and y.abs().max() < 2048 and (wp @ b2 + bp).abs().max() <= 2048
    assert (h.abs() @ w2.abs().t()).max() + x2.abs().max() + b2.abs().max() < 2 ** 22
    assert (y.abs() @ wp.abs().t()).max() < 2 ** 22
    assert (torch.cat([h, x2], 1).abs() @ torch.cat([wm, wp], 1).abs().t()).max() < 2 ** 22
    return t


def normal_tail(M, C, seed, alpha=0.7):
    g = torch.Generator(device="cpu").manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    h, x2, r = rn(M, 4 * C).half(), rn(M, C).half(), rn(M, C).half()
    w2, wp = (rn(C, 4 * C) / (4 * C) ** 0.5).half(), (rn(C, C) / C ** 0.5).half()
    b2, bp = (0.1 * rn(C)).half(), (0.1 * rn(C)).half()
    ref, y = tail_ref(h, x2, w2, b2, wp, bp, r, alpha)
    return Tail(h, x2, w2, b2, wp, bp, r, alpha, ref, y)


def integer_gemm(M, N, c0, c1, seed):
    """a0 [M, c0], a1 [M, c1], w [N, c0 + c1] in {-1, 0, 1}: every fp32 partial sum is an integer below 2^24 and the result is far
    below 2048 in magnitude (asserted), so any split and any order of the sums gives the float64 value in every element."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    a0, a1 = _sparse_int(g, (M, c0), 1, 0.6), _sparse_int(g, (M, c1), 1, 0.6)
    w = _sparse_int(g, (N, c0 + c1), 1, 0.6)
    ref = torch.cat([a0, a1], 1) @ w.t()
    assert ref.abs().max() < 2048
    return a0.half(), a1.half(), w.half(), ref
