"""Case table, operands, float64 reference and acceptance rule of the per-element tests of the normalisation kernels
(csrc/norm.hip, csrc/gn_fused.hip).

Inputs whose sums are exact in any order.  Every kernel of the family accumulates fp32 sums of (x - k) and (x - k)^2 with k a
sample of the same group or channel, through float LDS atomics, fixed point or trees.  The operands live on a dyadic grid,
x = (mu[b, g] + d) * step with integers mu and |d| <= amp[b, g] <= 6 and step a power of two: every shifted value is an integer
multiple of step of magnitude <= 12 step, so every partial sum of values (of squares) is an integer below 2^24 in units of step
(step^2) for groups of up to 2^16 elements, hence exact in fp32 in ANY order.  What remains is a short, fixed list of roundings.

  direct GroupNorm    d iid per element; |mu| in [3 amp, 4 amp] with a random sign ("a few sigma", and |mean| >= |mean - k|);
                      large-mean cases: |mu| in [1000, 1040] at step 2^-6 (mean ~ 16), eps 1e-6.
  stats-fed kernels   d = o[b, t, c] + z with z a zero-sum multiset (pairs +-d, permuted) inside every block of R rows of a
                      channel and an integer offset |o| <= 1: the partial (mean, M2) of a block is ((mu + o) step, sum z^2 step^2)
                      exactly, and so is every term of Chan's combination (n_i dm_i, M2_i + n_i dm_i^2: integers).
  0-D GroupNorm       as the direct cases, with the group's shift sample (s = 0, first channel) within one step of mu: a group has as
                      few as 16 elements, and (mean - k)^2 <= RHO_MAX var has to hold in each.
  rows (LayerNorm)    zero-sum multiset per row plus an integer row offset o_i (every third row |o_i| = 1000 >> sigma): the row
                      mean is o_i step exactly, v - mean and the sum of its squares are exact.
  gamma = 1 + 0.5 N(0, 1), beta = 0.5 N(0, 1) as fp16, distinct per channel (per (s, c) for the 0-D kernel).  mu, amp and d are drawn
  per (sample, group): exchanging two groups or two samples changes the answer.

The acceptance rule, mismatch(): with the float64 result `ref` of the whole operation on the fp16 operands (and the fp32 eps the
ABI takes), every fp16 output must satisfy

    |out - ref| <= half the fp16 spacing at ref (2^-25 below 2^-14)  +  K * 2^-24 * scale,     scale = |x sc| + |mean sc| + |beta|

per element (sc = rstd * gamma).  K counts the roundings of the kernels' formulas in units of u = 2^-24 (one fp32 rounding to
nearest).  gn_partial_kernel + gn_apply_kernel / gn_slab_kernel, with A = |x sc|, M = |mean sc|, Bt = |beta|, S and Q the exact sums:
    inv_count = 1 / (HW cg)                    1 u   (HW cg < 2^24 is exact)
    ms = S inv_count                           1 u   -> |d ms| <= 2 u |ms|
    mean = ms + k                              1 u   -> |d mean| <= 2 u |ms| + u |mean| <= 3 u |mean|     (|ms| <= |mean|, checked)
    var = Q inv_count - ms ms                  Q inv_count: 2 u (var + ms^2); ms ms: 5 u ms^2; the difference: 1 u var
                                               -> |d var| <= (3 + 7 rho) u var with rho = ms^2 / var <= 4 (checked per group)
    rstd = rsqrt(var + eps)                    the sum 1 u, v_rsq_f32 one ulp = 2 u -> |d rstd| <= ((3 + 28) / 2 + 1 / 2 + 2) u = 18 u
    sc = rstd gamma                            1 u   -> 19 u
    sh = beta - mean sc                        product 1 u M, difference 1 u (Bt + M), from d sc 19 u M, from d mean 3 u M
    y = x sc + sh                              product 1 u A, from d sc 19 u A, sum 1 u (A + M + Bt)
    total                                      21 u A + 25 u M + 2 u Bt <= 25 u scale
The contracted forms (fma) only drop roundings.  The other kernels stay below the same count: gn0d_kernel forms (x - mean) rstd
gamma + beta (1 + 3 + 18 + 1 + 1 + 1 u); gn_table_kernel folds exact terms around a pivot that is itself a block mean (same list
with dmean for ms); gn_from_stats_kernel sums n_i mean_i exactly, its second pass adds at most 10 + 9 inexact terms of one sign
(<= 23 u on var, 11.5 u on rstd, below the 15.5 u above); the sums form works in fp64 and rounds (mean, var) once; layernorm_kernel
and row_stats_kernel have an exact mean and an exact sum of squares (rstd within 3 u).  K = 32 = 25 rounded up to a power of two:
K * 2^-24 = 2^-19, an eighth of the 2^-16 the fp16 half-ulp leaves room for.  With SiLU the term passes through |silu'| <= 1.1
and x / (1 + __expf(-x)) adds at most 8 u |silu| (argument product and constant 2 u |x| (1 - s) <= 0.6 u, v_exp_f32 2 u, the sum 1 u,
the division or v_rcp_f32 and product 3 u): K_SILU = 1.1 K + 8.  The same K holds for every case; no case is widened.

fp32 outputs have no fp16 term: the chan_stats partials and the row_stats mean must be bit-exact; rstd of row_stats within
4 u relative; the table's scale within K u |sc| and its shift within K u (|beta| + |mean sc|).

tests/test_exact_norm_cpu.py proves the preconditions without a GPU; tests/test_exact_norm_gpu.py runs the kernels.
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
K = 32
K_SILU = 1.1 * K + 8
RHO_MAX = 4.0            # (mean - k)^2 / var per (sample, group), the bound the derivation of K uses
RSTD_ROWS_REL = 4 * U    # row_stats rstd: q / C 1 u and + eps 1 u under the root (1 u together), v_rsq_f32 2 u -> 3 u, rounded up
GROUPS = 32
CASES = {}


def _case(name, family, **kw):
    assert name not in CASES, name
    CASES[name] = dict(name=name, family=family, **kw)


def _gn(name, family, B, HW, c0, c1=0, eps=1e-5, big=False, R0=None, R1=None, **kw):
    _case(name, family, B=B, HW=HW, c0=c0, c1=c1, C=c0 + c1, groups=GROUPS, eps=1e-6 if big else eps, big=big,
          step=2.0 ** -6 if big else 2.0 ** -2, R0=R0, R1=R1, **kw)


# ---- gn_slab_kernel<2|6|12>: one block per (sample, slab of lcm(cg, 8) channels); a thread keeps one 8-channel chunk and
# `items` = ceil(HW / rows_per_pass) rows, rows_per_pass = 256 / (chunks per slab).  Each shape is the smallest with its property.
_gn("slab2_one_pass", "direct", 2, 16, 1280, nitem=2)                 # cg 40: 5 chunks, 51 rows per pass, one ragged pass (<2>, u = 1 all weight 0)
_gn("slab2_two_passes", "direct", 2, 64, 1280, eps=1e-6, nitem=2)     # second pass ragged: 13 of 51 rows
_gn("slab6_last_pass_one_row", "direct", 2, 256, 1280, nitem=6)       # six passes, the last of one row
_gn("slab12_640", "direct", 2, 600, 640, eps=1e-6, nitem=12)          # cg 20: twelve passes, the last of 39 rows
_gn("slab12_320", "direct", 2, 576, 320, nitem=12)                    # cg 10: a slab is four groups crossing 8-channel chunks
_gn("slab6_cg5", "direct", 2, 200, 160, nitem=6)                      # cg 5: eight groups per slab, the per-lane branch of gn_shift8
_gn("slab2_cg6", "direct", 3, 100, 192, eps=1e-6, nitem=2)            # cg 6: slab of 24 channels, 85 rows per pass
_gn("slab2_cg2", "direct", 2, 512, 64, nitem=2)                       # cg 2: one chunk per slab, 256 rows per pass
_gn("slab2_cg4", "direct", 2, 64, 128, nitem=2)                       # cg 4: the two-load branch of gn_shift8 with cg < 8
_gn("slab6_cg60", "direct", 2, 100, 1920, nitem=6)                    # cg 60: 15 chunks, 17 rows per pass
_gn("slab6_seam", "direct", 2, 64, 640, 320, nitem=6)                 # cg 30: group 21 (channels 630 .. 659) spans the concat seam
_gn("slab2_concat", "direct", 2, 16, 1280, 1280, eps=1e-6, nitem=2)   # cg 80, two sources of equal width
_gn("slab2_big_mean", "direct", 2, 64, 1280, big=True, nitem=2)       # mean ~ 16, sigma ~ 0.03, eps 1e-6
# ---- gn_partial_kernel + gn_apply_kernel: one row past the slab limit (13 items) or otherwise minimal
_gn("two_1280", "direct", 2, 613, 1280, nitem=0)        # R = 1, 12-row chunks, 52 chunks: the 8-way fold of the partials runs and leaves a tail; last chunk of one row
_gn("two_320", "direct", 2, 700, 320, eps=1e-6, nitem=0)  # TC = 40, R = 6: 240 of 256 threads, 54 rows per chunk, the last of 52
_gn("two_npos2", "direct", 2, 337, 2304, nitem=0)       # npos = 2 with 32 valid threads at the second position
_gn("two_concat_2560", "direct", 2, 301, 1280, 1280, nitem=0)
_gn("two_4096", "direct", 2, 193, 4096, eps=1e-6, nitem=0)   # the width limit
_gn("two_concat_640", "direct", 2, 700, 320, 320, nitem=0)
# cg 65: a slab would have 65 chunks > 64, so two launches at any HW; npos = 2 with 4 valid threads.  HW = 64 keeps "one row more"
# (1 / 65 of the count) above the K 2^-24 scale ~ 2e-3 the rule grants at |mean| / sigma ~ 500
_gn("two_big_mean", "direct", 2, 64, 2080, big=True, nitem=0)
# ---- gn0d_kernel: HW = S = 4, gamma / beta [S, C] distinct per s
_gn("gn0d_320", "gn0d", 3, 4, 320)
_gn("gn0d_64_64", "gn0d", 3, 4, 64, 64, eps=1e-6, seed=1)       # cg 4: 16 elements per group
_gn("gn0d_2560", "gn0d", 3, 4, 1280, 1280)
_gn("gn0d_seam", "gn0d", 3, 4, 640, 320)                # cg 30: group 21 spans the seam
# ---- gn_affine_kernel (ops.groupnorm_affine on a tensor without statistics) and the fp16 outputs of gn_table_kernel (with them)
_gn("affine_700", "affine", 2, 700, 320)
_gn("affine_4096", "affine", 2, 4096, 320, R0=256)      # the row320 chain's own geometry; zero-sum blocks of 256 rows
# ---- gn_table_kernel, gn_apply_table_kernel<false|true>, gn_from_stats_kernel: partials of R0 / R1 rows per source
_gn("stats_single", "stats", 2, 256, 320, R0=64)                        # cg 10, T = 4
_gn("stats_concat_seam", "stats", 2, 256, 640, 320, R0=128, R1=256)     # T0 = 2 != T1 = 1; group 21 spans the seam
_gn("stats_concat_2560", "stats", 2, 256, 1280, 1280, R0=64, R1=256, eps=1e-6)
_gn("stats_deep", "stats", 2, 1024, 1280, R0=64)                        # cg T = 640 > 512: the loop past the register list runs
_gn("stats_cg128", "stats", 2, 64, 4096, R0=64, eps=1e-6)               # cg = 128 (second gamma slot), C > 2048: npos = 2 of the apply kernel
_gn("stats_ragged_rows", "stats", 2, 320, 320, R0=64)                   # 30 rows per apply chunk: the last has 20
_gn("stats_big_mean", "stats", 2, 64, 1280, R0=64, big=True)            # HW cg 1040 < 2^24: the sum of n_i mean_i stays exact; HW as two_big_mean
# ---- chan_stats_kernel: HW = 2 R, B = 2 (B T = 4)
for _C in (64, 200, 320, 1280):         # 200: the last 64-channel block is ragged (C = 200 has no 32 groups: 8 groups here)
    for _R in (64, 128, 256):
        _gn("chan_%d_R%d" % (_C, _R), "chan", 2, 2 * _R, _C, R0=_R, big=(_C == 320 and _R == 128))
        if _C == 200:
            CASES["chan_200_R%d" % _R]["groups"] = 8
# ---- layernorm_kernel: one wave per row, four rows per block (rows % 4 != 0: a last block with idle waves)
for _C in (64, 320, 640, 768, 1024, 1280, 2048):
    for _rows in (1, 5, 77, 130):
        _case("ln_%d_x%d" % (_C, _rows), "ln", rows=_rows, C=_C, eps=1e-5, step=2.0 ** -3, pad=0)
# ---- row_stats_kernel<3|5|10|16>: 16 lanes per row, NCH 16-byte loads per lane
for _C, _nch in ((64, 3), (384, 3), (392, 5), (640, 5), (648, 10), (1280, 10), (1288, 16), (2048, 16)):
    for _rows in (1, 17, 300):
        for _pad in (0, 32):
            _case("rows_%d_x%d_pad%d" % (_C, _rows, _pad), "rows", rows=_rows, C=_C, eps=1e-5, step=2.0 ** -3, pad=_pad, nch=_nch)

PAD_SENTINEL = 60000.0   # fills the columns between C and ldx: one of them in a row sum wrecks the mean


def names(family):
    return [n for n, c in CASES.items() if c["family"] == family]


# ---- Python mirror of the dispatch (labels only; both test modules check it against the library) ----------------------------

def gn_geom(HW, C):
    """gn_geom() of csrc/norm.hip: the row chunks of gn_partial_kernel / gn_apply_kernel."""
    C8 = C // 8
    TC = min(C8, 256)
    R = 256 // TC
    rpc = max(16384 // C, 1, -(-HW // 256))
    rpc = -(-rpc // R) * R
    return dict(C8=C8, TC=TC, R=R, npos=-(-C8 // TC), rows_per_chunk=rpc, nchunk=-(-HW // rpc))


def gn_slab(HW, C, groups=GROUPS):
    """The slab test of vd_groupnorm_silu_f16: None (two launches) or the slab geometry with the template argument `nitem`."""
    cg = C // groups
    slab = cg
    while slab % 8:
        slab += cg
    chunks = slab // 8
    if C % slab or slab // cg > 16 or chunks > 64:
        return None
    rp = 256 // chunks
    items = -(-HW // rp)
    if items > 12:
        return None
    return dict(slab=slab, chunks=chunks, rows_per_pass=rp, items=items, nitem=2 if items <= 2 else (6 if items <= 6 else 12))


def gn_partial_floats(B, HW, C, groups=GROUPS):
    return B * gn_geom(HW, C)["nchunk"] * groups * 2


def gn_workspace_bytes(B, HW, C, groups=GROUPS):
    return (gn_partial_floats(B, HW, C, groups) + B * groups * 2) * 4


def apply_geom(HW, C):
    """gn_apply_launch() of csrc/gn_fused.hip: the row chunks of gn_apply_table_kernel."""
    C8 = C // 8
    TC = min(C8, 256)
    R = 256 // TC
    rpc = max(8192 // C, 1)
    rpc = min(-(-rpc // R) * R, HW)
    return dict(TC=TC, R=R, npos=-(-C8 // TC), rows_per_chunk=rpc, nchunk=-(-HW // rpc))


def locate(case, row, ch):
    """Where the kernel of `case` handles (row, channel): slab and pass, or row chunk, with the position inside it."""
    fam = case["family"]
    if fam in ("ln", "rows"):
        per = 4 if fam == "ln" else 16
        return "block %d, row %d of its %d" % (row // per, row % per, per)
    if fam == "gn0d":
        return "s = %d" % row
    HW, C = case["HW"], case["C"]
    p = gn_slab(HW, C, case["groups"]) if fam == "direct" else None
    if p is not None:
        rp = p["rows_per_pass"]
        n = min(rp, HW - row // rp * rp)
        return "slab %d, chunk %d of it, pass %d of %d, row %d of its %d%s" % (
            ch // p["slab"], ch % p["slab"] // 8, row // rp, p["items"], row % rp, n, " (last row)" if row % rp == n - 1 else "")
    g = gn_geom(HW, C) if fam in ("direct", "affine") else apply_geom(HW, C)
    rpc = g["rows_per_chunk"]
    n = min(rpc, HW - row // rpc * rpc)
    return "row chunk %d of %d, row %d of its %d%s, channel position %d" % (
        row // rpc, g["nchunk"], row % rpc, n, " (last row)" if row % rpc == n - 1 else "", ch // 8 // g["TC"])


# ---- operands ---------------------------------------------------------------------------------------------------------------------

def _rng(name, salt=0):
    return np.random.default_rng(zlib.crc32(name.encode()) + salt)


def _affine(rng, shape):
    gamma = (1.0 + 0.5 * rng.standard_normal(shape)).astype(np.float16)
    beta = (0.5 * rng.standard_normal(shape)).astype(np.float16)
    return gamma, beta


def _gn_ints(c, rng):
    """Integer grid values mu[b, g] + d [B, HW, C] of a GroupNorm case (see the module docstring), with mu and amp [B, groups]."""
    B, HW, C, G = c["B"], c["HW"], c["C"], c["groups"]
    cg = C // G
    amp = rng.integers(2, 7, (B, G))
    sign = rng.choice([-1, 1], (B, G))
    mu = sign * (rng.integers(1000, 1041, (B, G)) if c["big"] else rng.integers(3 * amp, 4 * amp + 1))
    ampc = np.repeat(amp, cg, 1)                                            # [B, C]
    d = np.empty((B, HW, C), np.int64)
    for lo, hi, R in ((0, c["c0"], c["R0"]), (c["c0"], C, c["R1"])):
        if hi == lo:
            continue
        a = ampc[:, None, lo:hi]
        if R is None:
            d[:, :, lo:hi] = np.floor(rng.random((B, HW, hi - lo)) * (2 * a + 1)).astype(np.int64) - a
        else:
            T = HW // R
            assert T * R == HW
            half = rng.integers(0, np.broadcast_to(a[:, None], (B, T, R // 2, hi - lo)))       # 0 .. amp - 1
            z = rng.permuted(np.concatenate([half, -half], 2), axis=2)
            o = rng.integers(-1, 2, (B, T, 1, hi - lo))
            d[:, :, lo:hi] = (z + o).reshape(B, HW, hi - lo)
    if c["family"] == "gn0d":     # groups of 16 .. 320 elements: the shift sample stays within one step of mu, which keeps rho <= RHO_MAX
        d[:, 0, ::cg] = rng.integers(-1, 2, (B, G))
    return np.repeat(mu, cg, 1)[:, None, :] + d, mu, amp


def _row_ints(c, rng):
    """[rows, C] integers o_i + z: z a zero-sum multiset (pairs +-d, d <= amp_i, permuted), o_i the row offset."""
    rows, C = c["rows"], c["C"]
    amp = rng.integers(2, 7, (rows, 1))
    half = rng.integers(0, np.broadcast_to(amp + 1, (rows, C // 2)))
    z = rng.permuted(np.concatenate([half, -half], 1), axis=1)
    o = rng.integers(-20, 21, (rows, 1))
    o[::3] = 1000 * rng.choice([-1, 1], (len(o[::3]), 1))
    return o + z, o


def half_ulp16(ref):
    """Half the fp16 spacing at |ref|: 2^(floor(log2 |ref|) - 11), 2^-25 below 2^-14."""
    a = np.maximum(np.abs(ref), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 11)


def silu(y):
    with np.errstate(over="ignore"):
        return y / (1.0 + np.exp(-y))


def group_stats(x, groups):
    """float64 (mean, var) [B, groups] of x [B, HW, C]."""
    B, HW, C = x.shape
    xg = x.reshape(B, HW, groups, C // groups)
    mean = xg.mean((1, 3))
    return mean, ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))


def affine_map(mean, var, gamma, beta, eps, cg):
    """float64 (sc, sh, |mean sc| + |beta|) per (sample, [s,] channel) from group statistics [B, groups]; gamma / beta [C] or [S, C]."""
    rstd = np.repeat(1.0 / np.sqrt(var + float(eps)), cg, 1)
    meanc = np.repeat(mean, cg, 1)
    if gamma.ndim == 2:
        rstd, meanc = rstd[:, None, :], meanc[:, None, :]
    sc = rstd * gamma.astype(np.float64)
    return sc, beta.astype(np.float64) - meanc * sc, np.abs(meanc * sc) + np.abs(beta.astype(np.float64))


def apply_map(x, sc, sh, base):
    """(y, scale) [B, HW, C] of y = x sc + sh."""
    if sc.ndim == 2:
        sc, sh, base = sc[:, None, :], sh[:, None, :], base[:, None, :]
    return x * sc + sh, np.abs(x * sc) + base


def block_partials(x, R):
    """float64 (mean, M2) [B * T, C] over blocks of R rows: the producers' partial statistics."""
    B, HW, C = x.shape
    xb = x.reshape(B * (HW // R), R, C)
    mean = xb.mean(1)
    return mean, ((xb - mean[:, None, :]) ** 2).sum(1)


@functools.lru_cache(maxsize=6)
def build(name):
    """Operands (numpy fp16) and the float64 reference of a case, computed once and shared -- do not modify.
    GroupNorm families: x0, x1 (or None), gamma, beta, eps (the fp32 value the ABI takes), x (float64 concat), mean / var
    [B, groups], sc / sh [B, C] ([B, S, C] for gn0d), y (before SiLU) and scale [B, HW, C].
    rows families: x [rows, ldx] (pad columns hold PAD_SENTINEL), mean / rstd [rows]; ln: gamma, beta, y, scale."""
    c = CASES[name]
    rng = _rng(name, c.get("seed", 0))
    t = SimpleNamespace(case=c, eps=np.float32(c["eps"]), step=c["step"])
    if c["family"] in ("ln", "rows"):
        ints, o = _row_ints(c, rng)
        t.ints, t.offset = ints, o[:, 0] * t.step
        xd = ints * t.step
        t.x = np.full((c["rows"], c["C"] + c["pad"]), PAD_SENTINEL, np.float16)
        t.x[:, :c["C"]] = xd
        t.mean = xd.mean(1)
        t.var = ((xd - t.mean[:, None]) ** 2).mean(1)
        t.rstd = 1.0 / np.sqrt(t.var + float(t.eps))
        if c["family"] == "ln":
            t.gamma, t.beta = _affine(rng, c["C"])
            sc = t.rstd[:, None] * t.gamma.astype(np.float64)
            t.y = (xd - t.mean[:, None]) * sc + t.beta.astype(np.float64)
            t.scale = np.abs((xd - t.mean[:, None]) * sc) + np.abs(t.beta.astype(np.float64))     # (x - mean is exact: the tighter scale)
        return t
    ints, t.mu, t.amp = _gn_ints(c, rng)
    t.ints = ints
    x16 = (ints * t.step).astype(np.float16)
    t.x0 = np.ascontiguousarray(x16[..., :c["c0"]])
    t.x1 = np.ascontiguousarray(x16[..., c["c0"]:]) if c["c1"] else None
    t.x = ints * t.step
    t.gamma, t.beta = _affine(rng, (c["HW"], c["C"]) if c["family"] == "gn0d" else c["C"])
    t.mean, t.var = group_stats(t.x, c["groups"])
    if c["family"] != "chan":
        t.sc, t.sh, t.base = affine_map(t.mean, t.var, t.gamma, t.beta, t.eps, c["C"] // c["groups"])
        if c["family"] != "affine":
            t.y, t.scale = apply_map(t.x, t.sc, t.sh, t.base)
    return t


def partials(t, which):
    """fp32 [B * T, c, 2] (mean, M2) of source `which` of a stats-fed case in blocks of its R rows, with T (exact: see the CPU module)."""
    c = t.case
    lo, hi, R = ((0, c["c0"], c["R0"]), (c["c0"], c["C"], c["R1"]))[which]
    mean, m2 = block_partials(t.x[..., lo:hi], R)
    return np.stack([mean, m2], -1).astype(np.float32), c["HW"] // R


def fixed_point_sums(t, which):
    """int64 [B * c, 2]: sum x * 2^32 and sum x^2 * 2^16 per (sample, channel), exact integers (VdGemmDesc.stat_sums format)."""
    c = t.case
    lo, hi = ((0, c["c0"]), (c["c0"], c["C"]))[which]
    unit = int(round(t.step * 2 ** 16))          # x = ints * step; step >= 2^-6
    assert unit * 2.0 ** -16 == t.step
    v = t.ints[..., lo:hi] * unit                # x * 2^16
    return np.stack([(v * 65536).sum(1), (v * v).sum(1) // 65536], -1).reshape(-1, 2)


# ---- the acceptance rule --------------------------------------------------------------------------------------------------------

def share(out, ref, scale, act=False):
    """(|out - ref| - half fp16 spacing) / (K 2^-24 scale) per element: the share of the fp32 allowance an output uses (<= 0: none;
    above 1: a failure; inf where the output is not finite).  act: the output went through SiLU (`ref` is the value after it)."""
    out = np.asarray(out, np.float64)
    err = np.abs(out - ref) - half_ulp16(ref)
    allow = (K_SILU if act else K) * U * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(err <= 0, 0.0, err / allow)
    return np.where(np.isfinite(out), s, np.inf)


def mismatch(out, ref, scale, case, act=False, what="", limit=6):
    """The acceptance rule on [sample, row, channel] (or [row, channel]) arrays.  None when every element passes, else a report: the
    count, the first failing coordinates with their group and their slab / row chunk and the position inside it, and the failures
    per group."""
    out, ref, scale = [np.asarray(a, np.float64) for a in (out, ref, scale)]
    if out.shape != ref.shape:
        return "%s %s: shape %s, expected %s" % (case["name"], what, out.shape, ref.shape)
    if out.ndim == 2:
        out, ref, scale = out[None], ref[None], np.broadcast_to(scale, ref.shape)[None]
    s = share(out, ref, np.broadcast_to(scale, ref.shape), act)
    bad = ~(s <= 1.0)
    if not bad.any():
        return None
    idx = np.argwhere(bad)
    cg = case["C"] // case["groups"] if "groups" in case else None
    lines = ["%s %s: %d of %d elements fail (K = %g, largest share %.3g)" % (case["name"], what, len(idx), ref.size, K_SILU if act else K, s.max())]
    for b, r, ch in idx[:limit].tolist():
        grp = "" if cg is None else ", group %d" % (ch // cg)
        lines.append("  (sample %d, row %d, channel %d%s; %s): got %.8g, expected %.10g" % (b, r, ch, grp, locate(case, r, ch), out[b, r, ch], ref[b, r, ch]))
    lines.append("  rows %d..%d, channels %d..%d" % (idx[:, 1].min(), idx[:, 1].max(), idx[:, 2].min(), idx[:, 2].max()))
    if cg is not None:
        per = np.bincount(idx[:, 0] * case["groups"] + idx[:, 2] // cg, minlength=ref.shape[0] * case["groups"]).reshape(ref.shape[0], -1)
        hit = np.argwhere(per)
        lines.append("  failures per (sample, group): " + ", ".join("(%d, %d): %d" % (b, g, per[b, g]) for b, g in hit[:24].tolist()) +
                     (" ... %d more" % (len(hit) - 24) if len(hit) > 24 else ""))
    return "\n".join(lines)


def bad_groups(out, ref, scale, case, act=False):
    """bool [B, groups]: the (sample, group) pairs with a failing element."""
    s = share(out, ref, np.broadcast_to(scale, ref.shape), act)
    B, HW, C = ref.shape
    return (~(s <= 1.0)).reshape(B, HW, case["groups"], -1).any((1, 3))


def mismatch_f32(out, ref, tol, case, what="", limit=6):
    """fp32 outputs: |out - ref| <= tol per element (tol = 0: bit-exact against the fp32 value of ref)."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    if out.shape != ref.shape:
        return "%s %s: shape %s, expected %s" % (case["name"], what, out.shape, ref.shape)
    bad = ~(np.abs(out - ref) <= tol)
    if not bad.any():
        return None
    idx = np.argwhere(bad)
    lines = ["%s %s: %d of %d values fail" % (case["name"], what, len(idx), ref.size)]
    for i in idx[:limit].tolist():
        lines.append("  %s: got %.10g, expected %.10g" % (tuple(i), out[tuple(i)], ref[tuple(i)]))
    lines.append("  extent: " + ", ".join("%d..%d" % (idx[:, k].min(), idx[:, k].max()) for k in range(idx.shape[1])))
    return "\n".join(lines)
