"""Case table of the per-element tests of the fused GEMM epilogues and of the one-launch feed-forward / row-resident kernels
(tests/test_exact_epilogue_cpu.py proves every precondition without a GPU, tests/test_exact_epilogue_gpu.py runs the kernels).
build(name) draws the operands and computes the reference once per process.

The operands leave a kernel no rounding freedom, so a mislocated bias, colsum entry, statistics row, weight tile or hidden chunk
changes some element by a whole fp16 step.  Four families:

  integer accumulators  A, W and the biases are small sparse integers (wstream_epi_cases.integer_case): every MFMA partial sum is
                        an integer far below 2^24, exact in any order; what differs from float64 is the epilogue alone.
  code rows             a LayerNorm input row is x[i] = a_i code_i + o_i: code_i a balanced +-1 vector (a permutation of its own per
                        row), a_i in {1, 2, 4}, o_i an integer offset.  The row mean is o_i and the variance a_i^2 exactly, the
                        normalised value +-(1 + eps / a_i^2)^-1/2.
                        - Kernels that normalise the row in registers (ff_geglu_kernel, rowgemm320_kernel<LN>; ff_fused.hip: mean,
                          two-pass q, rsqrtf, fmaf(x, rstd, nmr), round to fp16) hand +-1 EXACTLY to the MFMA (ln_rows_fp32 models
                          the formula in fp32; the CPU test runs it for every row, also with rstd moved by 8 units of 2^-24 where
                          |o| <= 100); every third row has 100 <= |o_i| <= 1000.  Their outputs are integers.
                        - gemm_f16_kernel / gemm_wstream_epi_kernel apply rstd to the accumulator: y = rstd acc - (mean rstd)
                          colsum + b.  Here o_i = a_i k_i with |k_i| <= 1, every third row |k_i| = 3 (o^2 / a^2 <= 9: the in-loop
                          variance E[x^2] - mean^2 keeps its bits), the rows of W have an ODD number of +-1 entries and the bias is
                          even, so code . w + b is odd: never zero (a zero would come out as the 1e-6 residue of rstd o colsum -
                          (mean rstd) colsum).  The float64 value is (1 + eps / a^2)^-1/2 D + b; the kernel's fp32 value lies within
                          dy of it (below), and the CPU test asserts that the whole interval rounds to the one fp16 integer D + b.
  saturated gates       GEGLU gate biases are +-16 (70 % positive, signs mixed inside every 32-column group) and the gate rows of W
                        so sparse that |g| >= 8: vd_erf (vd_common.h; vd_erf_fp32 models it) returns exactly +-1 from |g| = 6 on, so
                        v gelu(g) is exactly v g or exactly 0.  |v g| <= 2048.  Closed gates are zero by construction (about
                        30 % of a GEGLU output), so the zero-share cap of the exact suites is asserted on the open gates
                        here, and on the final output where a second projection follows.
  mid-range             integer accumulators plus dyadic biases (multiples of 2^-6): pre-activations spread over [-12, 12]
                        (GEGLU gates over [-2.5, 12]: below about -3 the absolute error of vd_erf exceeds an fp16 step of
                        v gelu(g) and an element would say nothing).  The float64 value widened by the bound below is rounded to
                        fp16 at both ends; the CPU test asserts that every such interval holds at most two adjacent fp16 values,
                        and an element passes if it is one of them (vdtest_util.interval_mismatch).

Tolerances (u = 2^-24; none is measured):
  dy, LayerNorm fold    |fp32 y - float64 y| <= u (kD |rstd (acc - mean colsum)| + 3 |mean rstd colsum| + 2 |b| + 2 |y|): the error
                        of rstd is common to both products (nmr = -mean * rstd), so it multiplies their difference only -- kD = 8:
                        rsqrtf to 2 ulp (4 u), the two roundings of its argument (1 u), the products (2 u), rounded up; in-loop
                        statistics add 4 u (1 + o^2 / a^2) (s2 / K and mean^2 are rounded at the size of E[x^2], and the variance is
                        a^2 of it) --; nmr and nmr * colsum are one rounding each and mean = s1 / K one more (3 u); the bias add and
                        the last fma 1 u each at the size of their result (doubled).
  activations           apply_act (gemm_kernel.h) is v * rcp(1 + __expf(-s)), s = v * fmaf(c3, v * v, c1): s carries 3 roundings, the
                        product with log2(e) and the constant 2 more, each moving exp(-s) by u |s|; v_exp_f32 2 u, the sum 1 u, v_rcp_f32
                        2 u, the product with v 1 u, alpha 1 u, one spare: rel = (5 S + 8) u with S the largest |s| that still
                        matters: SiLU 12, quick GELU 1.702 * 12 = 20.5, tanh GELU 88 (beyond it exp leaves the fp32 range, the
                        kernel returns exactly v or -0 and the float64 value is within 1e-37 of that).  The float64 reference is
                        the same formula with the kernel's fp32 constants.
  GEGLU                 v * (0.5 g (1 + vd_erf(g * 2^-1/2))) * alpha: 6 roundings (rel 6 u) and the absolute error of vd_erf --
                        1.5e-7 (Abramowitz-Stegun 7.1.26, as vd_common.h states) plus 8 u for its fp32 evaluation (five fma, v_rcp_f32,
                        v_exp_f32 and the last subtraction, each at magnitude <= 1) -- times |v g| / 2.  Saturated gates: vd_erf is
                        exactly +-1, only the 3 roundings of the products remain.
  residual              part 2 of the epilogue rounds the tile to fp16 and then adds the residual: fp16(fp32(fp16(y)) + res), and the
                        feed-forward kernels round once more after b2.  The (at most two) fp16 values of the tile are carried
                        through these stages in float32 arithmetic (numpy); the output must be the image of one of them.

Shapes (none is a workload shape):
  gemm_f16_kernel       M = 128 * 2 + 5: ragged against every tile height (64, 128); N = 200 (a multiple of 8 and of no tile
                        width) or 256 (GEGLU: packed pairs need 128-column tiles); K = 192 / 320 (3 and 5 k-tiles).  The tile sweep
                        forces every instantiated tile; the 320-column tile takes the epilogue in two passes (EP = 2).
  gemm_wstream_epi      M = 256, N = 256, K = 128 and 2048: 2 chunks (the prologue's preload is the whole stream) and 32 (the unrolled
                        maximum, where the wait count changes).
  rowgemm320<LN>        M = 128 * 3 + 5, N = 320 (single group), 960 and 1920 (MULTI: 3 and 6 column groups through the slots).
  ff_geglu_kernel       M = 128 and 128 * 2 + 5; the 20 hidden chunks and both W2 halves differ (asserted).
  side outputs          M = 256 = 2 images of 128 rows, N = 264, K = 192, |y| <= 32: the fp32 sums of squares of a row segment and
                        Q - S S / n of a 128-row partial are integers (or multiples of 1 / 128) below 2^24 -- exact, so row_sums,
                        stat_sums and the (mean, M2) partials are compared without a tolerance.
  ff_chain_kernel       the three instantiated (PRE, POST) pairs (neither: the library refuses, asserted), each at M = 128 * 2 + 5
                        (a ragged last tile) and as two replicas of 256 rows (REP: grid.y = replica, x0 and r read at row m % 256).
                        PRE: x1 = a Wo^T + bo + x0 is a code row built from both operands (builder's docstring); POST: Wp rows
                        are a +1 / -1 pair, alpha = 1/2, the output an exact multiple of 1/2.  With POST and M % 128 == 0 the
                        statistics ride along; the stored values reach a few hundred, so Q = sum (v - k)^2 is no longer exact:
                        test_exact_epilogue_gpu._chan_stats_mismatch derives |mean - ref| <= 2 u |ref| and |M2 - ref| <=
                        u (34 Q + 2 S^2 / n) from emit_chan_stats, and stat_sums must equal the fp64 image of the partials exactly.
  rowchain320_kernel    M = 384 = 3 images of 128 rows with their own sc (1/2 or 1), sh, ctr (integers), plain and centred map
                        (exact in packed fp16); N2 = 960 (three q | k | v groups behind the proj_in group).  dense: h exact.
                        perm: W1 = 2 x permutation, b1 constant -- the rows of h are code rows (scale 2 a, offset 2 o + b1), so
                        the LayerNorm of the second stage hands +-1 to the MFMA and y2 is exact too.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import wstream_epi_cases as W

U = 2.0 ** -24
LN_EPS = W.LN_EPS
GATE_SAT = 8.0            # |g| of every saturated gate (vd_erf is exactly +-1 from 6 on)
ERF_ABS = 1.5e-7 + 8 * U
ACT_C = {"quick_gelu": (float(np.float32(1.702)), 0.0), "silu": (1.0, 0.0),
         "gelu_tanh": (float(np.float32(1.5957691216057308)), float(np.float32(0.07135481627260025)))}
ACT_REL = {"quick_gelu": (5 * 20.5 + 8) * U, "silu": (5 * 12 + 8) * U, "gelu_tanh": (5 * 88 + 8) * U}
GEGLU_REL = 6 * U
ARG_MAX = 12.0
GATE_MIN = -2.5
CASES = {}


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ---- operand draws -------------------------------------------------------------------------------------------------------------
def code_rows(M, C, seed, scaled, big=(100, 1000)):
    """(x fp16 [M, C], code float64 +-1 [M, C], a [M], o [M]): x = a code + o.  scaled: o = a k, |k| <= 1 and 3 on every third row
    (the fold of the GEMM kernels); else |o| <= 8 and `big` = 100 .. 1000 on every third row (the kernels that normalise in
    registers)."""
    g = _gen(seed)
    order = torch.rand((M, C), generator=g).argsort(1)
    code = torch.where(order < C // 2, 1.0, -1.0).double()
    a = (2.0 ** torch.randint(0, 3, (M,), generator=g)).double()
    sign = torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0).double()
    third = torch.arange(M) % 3 == 2
    if scaled:
        o = a * torch.where(third, 3.0 * sign, torch.randint(-1, 2, (M,), generator=g).double())
    else:
        o = torch.where(third, sign * torch.randint(big[0], big[1] + 1, (M,), generator=g).double(), torch.randint(-8, 9, (M,), generator=g).double())
    x = code * a[:, None] + o[:, None]
    assert torch.equal(x.half().double(), x)
    return x.half(), code, a, o


def sparse_pm1(g, shape, nnz):
    """+-1 entries kept with probability nnz / K (float64)."""
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()
    return sign * (torch.rand(shape, generator=g) < float(nnz) / shape[-1]).double()


def cap_nnz(w, cap):
    """The first `cap` non-zero entries of every row."""
    return w * ((w != 0).cumsum(1) <= cap).double()


def force_odd(w):
    """Every row gets an odd number of non-zero entries: a row with an even count has entry (row % K) toggled between 0 and +1."""
    w = w.clone()
    rows = ((w != 0).sum(1) % 2 == 0).nonzero().flatten()
    cols = rows % w.shape[1]
    w[rows, cols] = torch.where(w[rows, cols] != 0, 0.0, 1.0).double()
    return w


def dyadic(g, shape, lo, hi):
    """Multiples of 2^-6 in [lo, hi] (float64)."""
    return torch.randint(int(lo * 64), int(hi * 64) + 1, shape, generator=g).double() / 64.0


def gate_mask(N):
    """True on the gate rows of GEGLU-packed weights: per 64 rows [32 value | 32 gate] (pack.pack_geglu)."""
    return (torch.arange(N) % 64) >= 32


def gate_bias_sat(g, n):
    return torch.where(torch.rand(n, generator=g) < 0.7, 16.0, -16.0).double()


def unpack_geglu_vector(bp):
    """The inverse of pack.pack_geglu on a bias: [all values | all gates] from the packed [32 value | 32 gate] groups."""
    v = bp.reshape(-1, 2, 32)
    return torch.cat([v[:, 0].reshape(-1), v[:, 1].reshape(-1)])


# ---- fp32 models of the kernels' written formulas (numpy float32 arithmetic) --------------------------------------------------------
def ln_rows_fp32(x, eps=LN_EPS, drift=0):
    """ff_fused.hip / gemm_row320.hip: mean = s * (1 / C), q = sum (x - mean)^2, rstd = rsqrtf(q * (1 / C) + eps) (moved by `drift`
    units of 2^-24), nmr = -mean * rstd, fp16(fmaf(x, rstd, nmr)) -> float64 [M, C].  The fma is formed in float64 and rounded once."""
    f = np.float32
    x32 = np.asarray(x, np.float32)
    C = x32.shape[1]
    inv = f(1.0) / f(C)
    mean = x32.sum(1, dtype=np.float32) * inv
    d = x32 - mean[:, None]
    q = (d * d).sum(1, dtype=np.float32)
    rstd = (f(1.0) / np.sqrt((q * inv + f(eps)).astype(np.float64))).astype(np.float32)
    rstd = (rstd.astype(np.float64) * (1.0 + drift * U)).astype(np.float32)
    nmr = -mean * rstd
    y = (x32.astype(np.float64) * rstd[:, None].astype(np.float64) + nmr[:, None].astype(np.float64)).astype(np.float32)
    return y.astype(np.float16).astype(np.float64)


def vd_erf_fp32(x):
    """vd_common.h: vd_erf in float32 arithmetic (fma in float64, rounded once; rcp and exp2 correctly rounded)."""
    f = np.float32
    x = np.asarray(x, np.float32)
    ax = np.abs(x)

    def fma(a, b, c):
        return (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(np.float32)

    t = (1.0 / fma(ax, f(0.3275911), f(1.0)).astype(np.float64)).astype(np.float32)
    p = fma(t, f(1.061405429), f(-1.453152027))
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = (p.astype(np.float64) * t.astype(np.float64) + np.float64(f(c))).astype(np.float32)
    e = np.exp2(((-ax * ax) * f(1.44269504088896340736)).astype(np.float64)).astype(np.float32)
    r = f(1.0) - (p * t) * e
    return np.copysign(r, x).astype(np.float64)


# ---- float64 references ------------------------------------------------------------------------------------------------------------
def act_f64(act, y, alpha=1.0):
    """x * sigmoid(x (c1 + c3 x^2)) with the kernel's fp32 constants, times alpha (numpy float64)."""
    c1, c3 = ACT_C[act]
    y = np.asarray(y, np.float64)
    with np.errstate(over="ignore"):
        return y / (1.0 + np.exp(-(y * (c1 + c3 * y * y)))) * alpha


def geglu_f64(v, g, alpha=1.0):
    v, g = np.asarray(v, np.float64), np.asarray(g, np.float64)
    erf = torch.erf(torch.from_numpy(np.ascontiguousarray(g * 0.5 ** 0.5))).numpy()      # (float64)
    return v * 0.5 * g * (1.0 + erf) * alpha


def split_packed(y):
    """(value, gate) [M, N / 2] of a GEGLU-packed pre-activation [M, N]."""
    M = y.shape[0]
    y = y.reshape(M, -1, 2, 32)
    return y[:, :, 0, :].reshape(M, -1), y[:, :, 1, :].reshape(M, -1)


def to_f16(v):
    return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def add_f16(tile, other):
    """fp16(fp32(tile) + fp32(other)): one more rounding stage of an epilogue, on fp16-valued float64 arrays."""
    return (np.asarray(tile, np.float32) + np.asarray(other, np.float32)).astype(np.float16).astype(np.float64)


def geglu_interval(v, g, dv, dg, alpha, saturated):
    """(value, lo, hi) float64 of v gelu(g) alpha for pre-activations known to +-dv, +-dg."""
    if saturated:
        assert (np.abs(g) - dg >= GATE_SAT).all(), "a gate is not saturated: |g| = %g" % np.abs(g).min()
        opened = g > 0
        f = lambda vv, gg: np.where(opened, vv * gg * alpha, 0.0)
        rel, ab = 3 * U, 0.0
        true = geglu_f64(v, g, alpha)
        assert np.abs(true - f(v, g)).max() <= 1e-9, "the true GELU is not within 1e-9 of the saturated value"
    else:
        f = lambda vv, gg: geglu_f64(vv, gg, alpha)
        rel, ab = GEGLU_REL, np.abs(v * g) * 0.5 * ERF_ABS * abs(alpha)
    val = f(v, g)
    c = np.stack([val] + [f(v + sv * dv, g + sg * dg) for sv in (-1, 1) for sg in (-1, 1)])
    lo, hi = c.min(0), c.max(0)
    return val, lo - rel * np.abs(lo) - ab, hi + rel * np.abs(hi) + ab


def gemm_expect(a, w, bias, res, fold, act, alpha, ln_eps=LN_EPS, colsum=None, stat_rows=None):
    """The launch of ops.gemm on fp16 operands -> SimpleNamespace(val, lo, hi, y, dy): the float64 value of every output element, the
    fp16 interval an element must lie in (lo == hi: a single value), the float64 pre-activation y and the bound dy of the kernel's
    fp32 error in it.  fold: "off" / "table" / "inloop" / "sums"; act: "none", "geglu_sat", "geglu_mid" or an activation's name.
    colsum / stat_rows: a mislocated operand on purpose -- the colsum vector the launch is given instead of the row sums of w, the
    matrix whose row statistics it is given instead of those of a."""
    a64, w64 = a.double(), w.double()
    acc = a64 @ w64.t()
    b = bias.double()[None, :] if bias is not None else torch.zeros((1, w.shape[0]), dtype=torch.float64)
    if fold == "off":
        y, dy = acc + b, torch.zeros_like(acc)
    else:
        s64 = a64 if stat_rows is None else stat_rows.double()
        mean = s64.mean(1)
        var = ((s64 - mean[:, None]) ** 2).mean(1)
        rstd = (var + ln_eps).rsqrt()
        cs = w64.sum(1) if colsum is None else colsum.double()
        lin = rstd[:, None] * (acc - mean[:, None] * cs[None, :])
        y = lin + b
        kd = 8.0 + (4.0 * (1.0 + mean * mean / var) if fold == "inloop" else 0.0) + torch.zeros_like(mean)
        dy = U * (kd[:, None] * lin.abs() + 3.0 * (mean * rstd).abs()[:, None] * cs.abs()[None, :] + 2.0 * b.abs() + 2.0 * y.abs())
    y, dy = y.numpy(), dy.numpy()
    if act == "none":
        val, lo, hi = y * alpha, (y - dy) * alpha, (y + dy) * alpha
        lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    elif act in ("geglu_sat", "geglu_mid"):
        (v, g), (dv, dg) = split_packed(y), split_packed(dy)
        val, lo, hi = geglu_interval(v, g, dv, dg, alpha, act == "geglu_sat")
    else:
        c = np.stack([act_f64(act, y + s * dy, alpha) for s in (-1, 0, 1)])
        val, lo, hi = c[1], c.min(0), c.max(0)
        lo, hi = lo - ACT_REL[act] * np.abs(lo), hi + ACT_REL[act] * np.abs(hi)
    lo, hi = to_f16(lo), to_f16(hi)
    tlo, thi = lo, hi          # the tile that part 1 of the epilogue rounds to fp16
    if res is not None:
        r = res.double().numpy()
        lo, hi, val = add_f16(lo, r), add_f16(hi, r), to_f16(val) + r
    return SimpleNamespace(val=val, lo=lo, hi=hi, tlo=tlo, thi=thi, y=y, dy=dy)


# ---- the table -------------------------------------------------------------------------------------------------------------------
def _add(name, kernel, **kw):
    assert name not in CASES, name
    CASES[name] = dict(name=name, kernel=kernel, **kw)


FOLDS = ("off", "table", "inloop", "sums")
ACTS = ("none", "geglu_sat", "geglu_mid", "quick_gelu", "silu", "gelu_tanh")
EXACT_ACTS = ("none", "geglu_sat")

_i = 0
for _fold in FOLDS:
    for _act in ACTS:
        if _act == "geglu_mid" and _fold != "off":
            continue   # (the fold's dy moves a mid-range gate by more than the interval rule can use; the fold meets GEGLU saturated)
        _geglu = _act.startswith("geglu")
        _add("gemm_%s_%s" % (_fold, _act), "gemm", M=128 * 2 + 5, N=256 if _geglu else 200, K=(192, 320)[_i % 2], fold=_fold, act=_act,
             alpha=(1.0, 0.5)[(_i // 2) % 2], bias=True, res=_act in ("none", "silu"), seed=1000 + _i)
        _i += 1
_add("gemm_off_none_nobias", "gemm", M=128 * 2 + 5, N=200, K=192, fold="off", act="none", alpha=0.5, bias=False, res=False, seed=1100)
_add("gemm_table_none_nobias", "gemm", M=128 * 2 + 5, N=200, K=320, fold="table", act="none", alpha=1.0, bias=False, res=True, seed=1101)
_add("gemm_sums_none_nobias", "gemm", M=128 * 2 + 5, N=200, K=192, fold="sums", act="none", alpha=0.5, bias=False, res=False, seed=1102)
TILE_SWEEP = ("gemm_table_none", "gemm_table_geglu_sat", "gemm_off_gelu_tanh")

_i = 0
for _K in (128, 2048):
    for _fold, _act in (("table", "none"), ("sums", "none"), ("table", "geglu_sat"), ("sums", "geglu_sat"), ("off", "geglu_sat"), ("off", "geglu_mid")):
        _add("wstream_%s_%s_k%d" % (_fold, _act, _K), "wstream_epi", M=256, N=256, K=_K, fold=_fold, act=_act, alpha=(1.0, 0.5)[_i % 2],
             bias=True, res=False, seed=2000 + _i)
        _i += 1

for _N in (320, 960, 1920):
    for _res in (False, True):
        _add("row320_ln_n%d%s" % (_N, "_res" if _res else ""), "row320", M=128 * 3 + 5, N=_N, res=_res, seed=3000 + _N + int(_res))

for _M in (128, 128 * 2 + 5):
    _add("ff_geglu_sat_m%d" % _M, "ff_geglu", M=_M, family="sat", seed=4000 + _M)
    _add("ff_geglu_gather_m%d" % _M, "ff_geglu", M=_M, family="gather", seed=4100 + _M)

_add("side_outputs", "side", M=256, N=264, K=192, img_rows=128, seed=5000)

# ff_chain_kernel<PRE, POST, REP>: the three instantiated (PRE, POST) pairs, each also with two replicas that share the residual
# operands (neither projection: the library refuses the launch, asserted by the GPU module)
for _pre, _post in ((True, False), (False, True), (True, True)):
    for _rep in (1, 2):
        _add("ff_chain_%d%d_rep%d" % (_pre, _post, _rep), "ff_chain", pre=_pre, post=_post, repeat=_rep, M=128 * 2 + 5 if _rep == 1 else 512,
             alpha=0.5, seed=6000 + 100 * _rep + 2 * _pre + _post)

# rowchain320_kernel: three images of 128 rows with their own scale / shift / centre
for _fam in ("dense", "perm"):
    for _ctr in (False, True):
        _add("rowchain_%s%s" % (_fam, "_centred" if _ctr else ""), "rowchain", family=_fam, centred=_ctr, M=384, rows_per_image=128, N2=960,
             seed=7000 + 10 * (_fam == "perm") + _ctr)


def names(kernel, **where):
    return [n for n, c in CASES.items() if c["kernel"] == kernel and all(c.get(k) == v for k, v in where.items())]


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def _gemm_operands(c):
    """(a, w, bias or None, res or None, extra) fp16 for a case of gemm_f16_kernel / gemm_wstream_epi_kernel."""
    M, N, K, fold, act = c["M"], c["N"], c["K"], c["fold"], c["act"]
    g = _gen(c["seed"])
    gm = gate_mask(N)
    extra = {}
    if fold == "off":
        a = W._sparse_int(g, (M, K), 2, 0.25)
        if act == "none":
            w = sparse_pm1(g, (N, K), K / 8.0)
            b = torch.randint(-3, 4, (N,), generator=g).double()
        elif act == "geglu_sat":     # |a| <= 2 and at most 4 entries in a gate row: |D_g| <= 8
            w = sparse_pm1(g, (N, K), K / 8.0)
            w[gm] = cap_nnz(w[gm], 4)
            b = torch.randint(-2, 3, (N,), generator=g).double()
            b[gm] = gate_bias_sat(g, int(gm.sum()))
        elif act == "geglu_mid":     # one entry in a gate row: |D_g| <= 2, gate bias in [-0.5, 10]: g in [-2.5, 12]
            w = cap_nnz(sparse_pm1(g, (N, K), 8), 4)
            w[gm] = cap_nnz(w[gm], 1)
            b = dyadic(g, (N,), -3.0, 3.0)
            b[gm] = dyadic(g, (int(gm.sum()),), GATE_MIN + 2.0, ARG_MAX - 2.0)
        else:                        # at most 4 entries: |D| <= 8, bias in [-4, 4]
            w = cap_nnz(sparse_pm1(g, (N, K), 8), 4)
            b = dyadic(g, (N,), -4.0, 4.0)
        a = a.half()
    else:
        a, code, sa, so = code_rows(M, K, c["seed"] + 50000, scaled=True)
        extra.update(code=code, a_scale=sa, offset=so)
        even = lambda n, lim: 2.0 * torch.randint(-lim, lim + 1, (n,), generator=g).double()
        if act == "none":
            w = force_odd(cap_nnz(sparse_pm1(g, (N, K), 20), 31))
            b = even(N, 2)
        elif act == "geglu_sat":     # |D_g| <= 7 and odd, gate bias +-16
            w = cap_nnz(sparse_pm1(g, (N, K), 12), 15)
            w[gm] = cap_nnz(w[gm], 7)
            w = force_odd(w)
            b = even(N, 1)
            b[gm] = gate_bias_sat(g, int(gm.sum()))
        else:                        # |D| <= 9 and odd, bias in {-2, 0, 2}: |y| <= 11
            w = force_odd(cap_nnz(sparse_pm1(g, (N, K), 6), 9))
            b = even(N, 1)
    res = torch.randint(-8, 9, (M, N // 2 if act.startswith("geglu") else N), generator=g).half() if c["res"] else None
    return a, w.half(), (b.half() if c["bias"] else None), res, extra


@functools.lru_cache(maxsize=None)
def build(name):
    """Operands, reference and intervals of a case, drawn once per process (leave them unchanged)."""
    c = CASES[name]
    return {"gemm": _build_gemm, "wstream_epi": _build_gemm, "row320": _build_row320, "ff_geglu": _build_ff, "side": _build_side,
            "ff_chain": _build_ff_chain, "rowchain": _build_rowchain}[c["kernel"]](c)


def _build_gemm(c):
    a, w, b, res, extra = _gemm_operands(c)
    e = gemm_expect(a, w, b, res, c["fold"], c["act"], c["alpha"])
    exact = c["act"] in EXACT_ACTS
    t = SimpleNamespace(case=c, a=a, w=w, bias=b, res=res, colsum=W.colsum_of(w), ln_sums=W.row_sums_fixed(a), exact=exact,
                        unit=c["alpha"], lo=e.lo, hi=e.hi, tlo=e.tlo, thi=e.thi, val=e.val, y=e.y, dy=e.dy, **extra)
    if exact:   # the one fp16 value of the interval (the CPU test asserts lo == hi and that it is a multiple of `unit`)
        t.ref = torch.from_numpy(e.lo.copy())
    return t


def _build_row320(c):
    M, N = c["M"], c["N"]
    g = _gen(c["seed"])
    x, code, sa, so = code_rows(M, 320, c["seed"] + 50000, scaled=False)
    w = sparse_pm1(g, (N, 320), 20)
    b = torch.randint(-3, 4, (N,), generator=g).double()
    res = torch.randint(-8, 9, (M, N), generator=g).double() if c["res"] else None
    ref = code @ w.t() + b[None, :] + (res if res is not None else 0.0)
    return SimpleNamespace(case=c, x=x, code=code, a_scale=sa, offset=so, w=w.half(), bias=b.half(), res=None if res is None else res.half(),
                           ref=ref, exact=True, unit=1.0)


FF_C = 320


def _build_ff(c):
    """ff_geglu_kernel: y = res + (v gelu(g)) W2^T + b2, [v | g] = LayerNorm(x) W1^T + b1 (W1 / b1 GEGLU-packed).  sat: saturated
    gates, everything an integer.  gather: mid-range gates, W2 rows one-hot times a power of two: out = res + s h[:, sel] + b2."""
    M, C = c["M"], FF_C
    g = _gen(c["seed"])
    x, code, sa, so = code_rows(M, C, c["seed"] + 50000, scaled=False)
    gm = gate_mask(8 * C)
    ng = int(gm.sum())
    res = torch.randint(-8, 9, (M, C), generator=g).double()
    if c["family"] == "sat":
        w1 = sparse_pm1(g, (8 * C, C), 5)
        w1[gm] = cap_nnz(w1[gm], 8)
        b1 = torch.randint(-2, 3, (8 * C,), generator=g).double()
        b1[gm] = gate_bias_sat(g, ng)
        w2 = sparse_pm1(g, (C, 4 * C), 40)
        b2 = torch.randint(-4, 5, (C,), generator=g).double()
    else:
        w1 = cap_nnz(sparse_pm1(g, (8 * C, C), 5), 8)
        w1[gm] = cap_nnz(w1[gm], 2)
        b1 = dyadic(g, (8 * C,), -3.0, 3.0)
        b1[gm] = dyadic(g, (ng,), GATE_MIN + 2.0, ARG_MAX - 2.0)
        sel = torch.randperm(4 * C, generator=g)[:C]                      # distinct hidden units, spread over the 20 chunks
        s = 2.0 ** torch.randint(-1, 2, (C,), generator=g).double()
        w2 = torch.zeros((C, 4 * C), dtype=torch.float64)
        w2[torch.arange(C), sel] = s
        b2 = torch.randint(-4, 5, (C,), generator=g).double()
    pre = code @ w1.t() + b1[None, :]                                       # LayerNorm hands +-1 to the MFMA: exact
    v, gt = split_packed(pre.numpy())
    zero = np.zeros_like(v)
    hval, hlo, hhi = geglu_interval(v, gt, zero, zero, 1.0, c["family"] == "sat")
    t = SimpleNamespace(case=c, x=x, code=code, a_scale=sa, offset=so, w1=w1.half(), b1=b1.half(), w2=w2.half(), b2=b2.half(),
                        res=res.half(), v=v, gate=gt, h=hval, exact=c["family"] == "sat", unit=1.0)
    if t.exact:
        h = np.rint(hval)
        t.h = h
        t.ref = torch.from_numpy(h) @ w2.t() + b2[None, :] + res
    else:
        sel_n, s_n, b2n, r = sel.numpy(), s.numpy()[None, :], b2.numpy()[None, :], res.numpy()
        t.sel = sel
        stage = lambda h16: add_f16(add_f16(h16[:, sel_n] * s_n, b2n), r)   # s h is exact: a power of two times an fp16 value
        t.hlo, t.hhi = to_f16(hlo), to_f16(hhi)
        t.lo, t.hi = stage(t.hlo), stage(t.hhi)
        t.val = to_f16(to_f16(hval)[:, sel_n] * s_n + b2n) + r
    return t


def _build_side(c):
    """Plain integer GEMM with a residual whose stored rows feed the three side outputs of the epilogue."""
    M, N, K = c["M"], c["N"], c["K"]
    g = _gen(c["seed"])
    a = W._sparse_int(g, (M, K), 2, 0.25)
    w = sparse_pm1(g, (N, K), K / 16.0)
    b = torch.randint(-3, 4, (N,), generator=g).double()
    res = torch.randint(-4, 5, (M, N), generator=g).double()
    ref = a @ w.t() + b[None, :] + res
    return SimpleNamespace(case=c, a=a.half(), w=w.half(), bias=b.half(), res=res.half(), ref=ref, exact=True, unit=1.0)


def side_expect(stored, img_rows, R):
    """From the stored fp16 rows (float64 [M, N]): row_sums int64 [M, 2], stat_sums int64 [M / img_rows, N, 2] and the (mean, M2)
    partials float64 [M / R, N, 2] of blocks of R rows."""
    s = torch.as_tensor(stored).double()
    M, N = s.shape
    rows = torch.stack([(s.sum(1) * 2.0 ** 24).round(), ((s * s).sum(1) * 2.0 ** 16).round()], 1).to(torch.int64)
    im = s.view(M // img_rows, img_rows, N)
    sums = torch.stack([(im.sum(1) * 2.0 ** 32).round(), ((im * im).sum(1) * 2.0 ** 16).round()], 2).to(torch.int64)
    blk = s.view(M // R, R, N)
    mean = blk.mean(1)
    part = torch.stack([mean, ((blk - mean[:, None, :]) ** 2).sum(1)], 2)
    return rows, sums, part


def _ff_sat_weights(g, C, w2_nnz):
    """(w1 [8C, C], b1, w2 [C, 4C], b2) float64 of the saturated feed-forward family (GEGLU-packed w1 / b1)."""
    gm = gate_mask(8 * C)
    w1 = sparse_pm1(g, (8 * C, C), 5)
    w1[gm] = cap_nnz(w1[gm], 8)
    b1 = torch.randint(-2, 3, (8 * C,), generator=g).double()
    b1[gm] = gate_bias_sat(g, int(gm.sum()))
    w2 = sparse_pm1(g, (C, 4 * C), w2_nnz)
    b2 = torch.randint(-4, 5, (C,), generator=g).double()
    return w1, b1, w2, b2


def ff_sat_core(code, w1, b1, w2, b2):
    """(v, gate, h, h W2^T + b2) float64 of the saturated feed-forward on rows the LayerNorm turns into `code`."""
    pre = code @ w1.t() + b1[None, :]
    v, gt = split_packed(pre.numpy())
    assert np.abs(gt).min() >= GATE_SAT
    h = np.where(gt > 0, v * gt, 0.0)
    return v, gt, h, torch.from_numpy(h) @ w2.t() + b2[None, :]


def _build_ff_chain(c):
    """x1 = a Wo^T + bo + x0 (PRE);  y = x1 + FF(LayerNorm(x1));  out = alpha (y Wp^T + bp) + r (POST).  x1 is a code row: its even
    columns come from the projection (Wo has two +1 entries per even row and none in the odd rows; `a` carries the code there), its
    odd columns from x0 (which holds the row offset in the even columns), and each half is balanced -- so both operands matter in
    every column pair.  Replicas share x0 and r (rows m % P), hence the scale, the offset and the odd half of the code, and differ
    in the even half.  Wp rows are a +1 / -1 pair: the row offset cancels and alpha (y Wp^T + bp) stays a small multiple of 1/2."""
    M, C, rep = c["M"], FF_C, c["repeat"]
    P = M // rep
    g = _gen(c["seed"])
    _, base, sa, so = code_rows(P, C, c["seed"] + 50000, scaled=False, big=(100, 400))
    half = lambda rows: torch.where(torch.rand((rows, C // 2), generator=g).argsort(1) < C // 4, 1.0, -1.0).double()
    code_e, code_o = half(M), half(P)
    idx = torch.arange(M) % P
    code = torch.empty((M, C), dtype=torch.float64)
    code[:, 0::2], code[:, 1::2] = code_e, code_o[idx]
    A, O = sa[idx], so[idx]
    x1 = A[:, None] * code + O[:, None]
    t = SimpleNamespace(case=c, code=code, a_scale=A, offset=O, x1=x1, exact=True, P=P)
    if c["pre"]:
        bo = 3.0
        x0 = torch.empty((P, C), dtype=torch.float64)
        x0[:, 0::2] = (so - bo)[:, None]
        x0[:, 1::2] = sa[:, None] * code_o + (so - bo)[:, None]
        perm = torch.randperm(C, generator=g)
        k0, k1 = perm[:C // 2], perm[C // 2:]
        wo = torch.zeros((C, C), dtype=torch.float64)
        wo[torch.arange(0, C, 2), k0] = 1.0
        wo[torch.arange(0, C, 2), k1] = 1.0
        a = torch.empty((M, C), dtype=torch.float64)
        a[:, k1] = torch.randint(-3, 4, (M, C // 2), generator=g).double()
        a[:, k0] = A[:, None] * code_e - a[:, k1]
        assert torch.equal(a @ wo.t() + bo + x0[idx], x1)
        t.x, t.a, t.wo, t.bo = x0.half(), a.half(), wo.half(), torch.full((C,), bo).half()
    else:
        t.x, t.a, t.wo, t.bo = x1.half(), None, None, None
    w1, b1, w2, b2 = _ff_sat_weights(g, C, 12)
    t.v, t.gate, t.h, ff = ff_sat_core(code, w1, b1, w2, b2)
    t.ff = ff
    y = x1 + ff
    t.y = y
    t.w1, t.b1, t.w2, t.b2 = w1.half(), b1.half(), w2.half(), b2.half()
    if c["post"]:
        cols = torch.rand((C, C), generator=g).argsort(1)[:, :2]
        wp = torch.zeros((C, C), dtype=torch.float64)
        wp[torch.arange(C), cols[:, 0]], wp[torch.arange(C), cols[:, 1]] = 1.0, -1.0
        bp = torch.randint(-4, 5, (C,), generator=g).double()
        r = torch.randint(-8, 9, (P, C), generator=g).double()
        t.proj = (y @ wp.t() + bp[None, :]) * c["alpha"]
        t.ref, t.unit = t.proj + r[idx], c["alpha"]
        t.wp, t.bp, t.res = wp.half(), bp.half(), r.half()
    else:
        t.ref, t.unit, t.wp, t.bp, t.res = y, 1.0, None, None, None
    return t


def _build_rowchain(c):
    """h = ((x - ctr) sc[img] + sh[img]) W1^T + b1;  y2 = LayerNorm(h) W2^T + b2.  sc in {1/2, 1}, sh and ctr integers per (image,
    channel): the packed fp16 map is exact.  dense: the mapped rows are small sparse integers, W1 sparse -- h is checked.  perm: the
    mapped rows are code rows, W1 = 2 x a permutation matrix and b1 constant, so the rows of h are code rows too (scale 2 a, offset
    2 o + b1) and y2 is exact as well."""
    M, C, N2, rpi = c["M"], FF_C, c["N2"], c["rows_per_image"]
    g = _gen(c["seed"])
    imgs = M // rpi
    sc = 2.0 ** torch.randint(-1, 1, (imgs, C), generator=g).double()
    sh = torch.randint(-2, 3, (imgs, C), generator=g).double()
    ctr = torch.randint(-2, 3, (imgs, C), generator=g).double() if c["centred"] else None
    img = torch.arange(M) // rpi
    t = SimpleNamespace(case=c, exact=True, unit=1.0, sc=sc.half(), sh=sh.half(), ctr=None if ctr is None else ctr.half())
    w2 = sparse_pm1(g, (N2, C), 20)
    b2 = torch.randint(-3, 4, (N2,), generator=g).double()
    if c["family"] == "dense":
        xm = W._sparse_int(g, (M, C), 4, 0.25)
        w1 = sparse_pm1(g, (C, C), 20)
        b1 = torch.randint(-3, 4, (C,), generator=g).double()
        t.ref_h, t.ref_y2 = xm @ w1.t() + b1[None, :], None
    else:
        _, code, sa, so = code_rows(M, C, c["seed"] + 50000, scaled=False, big=(100, 400))
        xm = sa[:, None] * code + so[:, None]
        perm = torch.randperm(C, generator=g)
        w1 = torch.zeros((C, C), dtype=torch.float64)
        w1[torch.arange(C), perm] = 2.0
        b1 = torch.full((C,), 3.0, dtype=torch.float64)
        t.ref_h = xm @ w1.t() + b1[None, :]
        t.code, t.a_scale, t.offset = code[:, perm], 2.0 * sa, 2.0 * so + 3.0
        assert torch.equal(t.ref_h, t.a_scale[:, None] * t.code + t.offset[:, None])
        t.ref_y2 = t.code @ w2.t() + b2[None, :]
    x = (xm - sh[img]) / sc[img] + (ctr[img] if ctr is not None else 0.0)
    assert torch.equal(x.half().double(), x) and torch.equal(((x - (ctr[img] if ctr is not None else 0.0)) * sc[img] + sh[img]), xm)
    t.x, t.xm, t.w1, t.b1, t.w2, t.b2 = x.half(), xm, w1.half(), b1.half(), w2.half(), b2.half()
    return t
