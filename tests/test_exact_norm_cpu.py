"""Preconditions of the per-element tests of the normalisation kernels (tests/norm_cases.py), proved without a GPU:
every operand is an exact fp16 value; every sum the derivation of the acceptance rule calls exact is an integer below 2^24 in its
unit; an fp32 emulation of each kernel's formula sequence (numpy float32, one operation per line, in the kernel's order, exact sums)
passes the rule with at most half of the allowance used; the rule rejects each of six deliberate errors in every (sample, group) or
row they touch; and the Python mirror of the dispatch agrees with the library's host code.

The discrimination tests cover every case with a per-element output (direct, 0-D, stats-fed GroupNorm and LayerNorm); the affine,
chan_stats and row_stats cases have [sample, channel] or [row] outputs only and are covered by the exactness and emulation tests."""
import numpy as np
import pytest

import norm_cases as N

F = np.float32
LIMIT = 2 ** 24
GN_Y = N.names("direct") + N.names("gn0d") + N.names("stats")


def rsqrt32(v):
    return (F(1) / np.sqrt(v.astype(F))).astype(F)


def silu32(v):                       # vd_silu: x / (1 + __expf(-x))
    return (v / (F(1) + np.exp(-v))).astype(F)


def silu32_rcp(y):                   # gn_fused.hip: y * rcp(1 + exp2(-log2(e) y))
    e = np.exp2(F(-1.44269504088896) * y)
    return (y * (F(1) / (F(1) + e))).astype(F)


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def f32_exact(v, what):
    v = np.asarray(v, np.float64)
    assert np.array_equal(v.astype(F).astype(np.float64), v), "%s is not exact in fp32" % what
    return v.astype(F)


def shifted_sums(t):
    """k [B, G] (the group's first sample), S = sum (x - k), Q = sum (x - k)^2 in float64, and sum |x - k|."""
    c = t.case
    B, HW, C, G = c["B"], c["HW"], c["C"], c["groups"]
    cg = C // G
    k = t.x[:, 0, ::cg]
    v = (t.x - np.repeat(k, cg, 1)[:, None, :]).reshape(B, HW, G, cg)
    return k, v.sum((1, 3)), (v * v).sum((1, 3)), np.abs(v).sum((1, 3))


# ---- operands ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(N.CASES))
def test_operands_are_exact_fp16_values(name):
    t = N.build(name)
    c = t.case
    assert np.abs(t.ints).max() <= 2048 and np.log2(t.step) == round(np.log2(t.step))
    if c["family"] in ("ln", "rows"):
        assert np.array_equal(t.x[:, :c["C"]].astype(np.float64), t.ints * t.step)
        assert c["pad"] == 0 or bool((t.x[:, c["C"]:] == N.PAD_SENTINEL).all())
    else:
        x16 = t.x0 if t.x1 is None else np.concatenate([t.x0, t.x1], -1)
        assert x16.dtype == np.float16 and np.array_equal(x16.astype(np.float64), t.ints * t.step)
        assert np.array_equal(t.x, t.ints * t.step)
        # mu, amp and d differ per (sample, group): exchanging two groups or two samples changes the answer
        assert len({(int(m), int(a)) for m, a in zip(t.mu.ravel(), t.amp.ravel())}) > t.mu.size // 3
    if c["family"] not in ("rows", "chan"):
        assert t.gamma.dtype == np.float16 and t.beta.dtype == np.float16
        assert len(np.unique(t.gamma)) > t.gamma.size // 8 and len(np.unique(t.beta)) > t.beta.size // 8
    assert float(t.eps) == float(np.float32(c["eps"]))


# ---- exactness of the sums ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", N.names("direct") + N.names("gn0d") + N.names("affine"))
def test_shifted_sums_are_exact_in_any_order(name):
    """sum |x - k| and sum (x - k)^2 over a WHOLE group stay below 2^24 in units of step and step^2: every partial sum any chunk,
    slab pass, thread or tree of the kernels can form (a subset of the group's integers) is an exactly representable integer, and
    so is each addend of the fixed-point accumulation.  Also the two bounds the derivation of K uses: |mean - k| <= |mean| and
    (mean - k)^2 <= RHO_MAX var."""
    t = N.build(name)
    k, S, Q, A = shifted_sums(t)
    assert np.abs((t.x - np.repeat(k, t.case["C"] // t.case["groups"], 1)[:, None, :]) / t.step).max() <= 12
    assert A.max() / t.step < LIMIT and Q.max() / t.step ** 2 < LIMIT
    assert np.array_equal(S / t.step, np.round(S / t.step)) and np.array_equal(Q / t.step ** 2, np.round(Q / t.step ** 2))
    f32_exact(S, "S"), f32_exact(Q, "Q")
    n = t.case["HW"] * (t.case["C"] // t.case["groups"])
    assert n < 2 ** 16
    ms = S / n
    assert bool((np.abs(ms) <= np.abs(t.mean)).all()), "|mean - k| > |mean|"
    rho = ms ** 2 / t.var
    assert rho.max() <= N.RHO_MAX, "rho = %.2f in (sample, group) %s: change the seed, not the bound" % (rho.max(), np.argwhere(rho == rho.max())[0])
    if t.case["big"]:
        assert np.abs(t.mean).min() > 15 and np.sqrt(t.var).max() < 0.1


def chan_terms(t):
    """Per source: (mean_i, M2_i) [B, T, c] float64 and n_i of the block partials of a stats-fed case."""
    c = t.case
    out = []
    for w in range(2 if c["c1"] else 1):
        p, T = N.partials(t, w)
        out.append((p[..., 0].astype(np.float64).reshape(c["B"], T, -1), p[..., 1].astype(np.float64).reshape(c["B"], T, -1), c["HW"] // T))
    return out


def pivot_sums(t):
    """gn_table_kernel in float64: pivot [B, G] (first partial mean of the group), s1 = sum n_i (mean_i - pivot),
    s2 = sum M2_i + n_i (mean_i - pivot)^2, the sums of their magnitudes, and sum n_i mean_i of gn_from_stats_kernel."""
    c = t.case
    G, cg = c["groups"], c["C"] // c["groups"]
    pivc = np.concatenate([m[:, 0, :] for m, _, _ in chan_terms(t)], -1)[:, ::cg]
    pc = np.repeat(pivc, cg, 1)
    cols, lo = [], 0
    for m, m2, n in chan_terms(t):
        dm = m - pc[:, None, lo:lo + m.shape[2]]
        cols.append(np.stack([(n * dm).sum(1), (m2 + n * dm * dm).sum(1), np.abs(n * dm).sum(1), (n * m).sum(1), np.abs(n * m).sum(1)]))
        lo += m.shape[2]
    s = np.concatenate(cols, -1).reshape(5, c["B"], G, cg).sum(-1)
    return pivc, s[0], s[1], s[2], s[3], s[4]


@pytest.mark.parametrize("name", N.names("stats") + ["affine_4096"])
def test_block_partials_and_chan_terms_are_exact(name):
    """The partial (mean, M2) of every block of R rows is an integer multiple of (step, step^2) and an exact fp32 value; every term
    of Chan's combination around the pivot is an integer, their magnitudes sum to less than 2^24 per group (exact in any order and
    in the 8-per-lane register list or the loop behind it alike), and so does sum n_i |mean_i| of gn_from_stats_kernel's first pass."""
    t = N.build(name)
    c = t.case
    for w in range(2 if c["c1"] else 1):
        lo, hi, R = ((0, c["c0"], c["R0"]), (c["c0"], c["C"], c["R1"]))[w]
        assert R in (64, 128, 256)
        mean, m2 = N.block_partials(t.x[..., lo:hi], R)
        assert np.array_equal(mean / t.step, np.round(mean / t.step)) and np.array_equal(m2 / t.step ** 2, np.round(m2 / t.step ** 2))
        f32_exact(mean, "partial mean"), f32_exact(m2, "partial M2")
    _, s1, s2, a1, sm, am = pivot_sums(t)
    assert a1.max() / t.step < LIMIT and s2.max() / t.step ** 2 < LIMIT and am.max() / t.step < LIMIT
    for v, u in ((s1, t.step), (s2, t.step ** 2), (sm, t.step)):
        assert np.array_equal(v / u, np.round(v / u))
    n = c["HW"] * (c["C"] // c["groups"])
    assert np.allclose(sm / n, t.mean, rtol=1e-12, atol=1e-12) and np.allclose(s2 / n - (s1 / n) ** 2, t.var, rtol=1e-9)
    sums = [N.fixed_point_sums(t, w) for w in range(2 if c["c1"] else 1)]
    s = np.concatenate([v.reshape(c["B"], -1, 2) for v in sums], 1).astype(np.float64)
    assert np.array_equal(s[..., 0] * 2.0 ** -32, t.x.sum(1)) and np.array_equal(s[..., 1] * 2.0 ** -16, (t.x ** 2).sum(1))


def emu_chan_stats(t):
    """chan_stats_kernel: k = the block's first row; out = (k + S / n, max(Q - S S / n, 0)) in fp32."""
    c = t.case
    R = c["R0"]
    xb = t.x.reshape(-1, R, c["C"])
    k = xb[:, 0, :]
    v = xb - k[:, None, :]
    S, Q = f32_exact(v.sum(1), "S"), f32_exact((v * v).sum(1), "Q")
    assert np.abs(v).sum(1).max() / t.step < LIMIT and Q.max() / t.step ** 2 < LIMIT
    n = F(R)
    mean = k.astype(F) + S / n
    m2 = np.maximum(Q - S * S / n, F(0))
    return np.stack([mean, m2], -1)


@pytest.mark.parametrize("name", N.names("chan"))
def test_chan_stats_partials_are_exact_fp32_values(name):
    """R is a power of two and amp <= 6: S / n, S^2 / n, k + S / n and Q - S^2 / n are exact, so the fp32 emulation equals the
    float64 (mean, M2) bit for bit -- the GPU test may ask for equality."""
    t = N.build(name)
    R = t.case["R0"]
    assert R & (R - 1) == 0
    mean, m2 = N.block_partials(t.x, R)
    emu = emu_chan_stats(t)
    assert np.array_equal(emu[..., 0].astype(np.float64), mean) and np.array_equal(emu[..., 1].astype(np.float64), m2)
    assert m2.min() > 0


@pytest.mark.parametrize("name", N.names("ln") + N.names("rows"))
def test_row_sums_are_exact(name):
    """The row mean is the row offset exactly; every partial sum of a row and the sum of squared deviations are integers < 2^24."""
    t = N.build(name)
    c = t.case
    assert np.array_equal(t.mean, t.offset) and np.array_equal(t.ints.sum(1) * t.step, c["C"] * t.offset)
    assert np.abs(t.ints).sum(1).max() < LIMIT and ((t.ints - t.ints.mean(1, keepdims=True)) ** 2).sum(1).max() < LIMIT
    f32_exact(t.mean, "row mean")
    assert np.abs(t.offset).max() > 100 * np.sqrt(t.var).max()        # a large offset, |o_i| >> sigma
    if c["family"] == "rows":
        assert (c["C"] // 8 + 15) // 16 <= c["nch"] and c["nch"] == next(n for n in (3, 5, 10, 16) if (c["C"] // 8 + 15) // 16 <= n)


# ---- fp32 emulations of the kernels' formula sequences ---------------------------------------------------------------------------------

def emu_direct_stats(t):
    """gn_apply_kernel / gn_slab_kernel / gn0d_kernel: (mean, rstd) [B, G] in fp32 from the exact sums."""
    c = t.case
    k, S, Q, _ = shifted_sums(t)
    S, Q, k = f32_exact(S, "S"), f32_exact(Q, "Q"), k.astype(F)
    inv_count = F(1) / (F(c["HW"]) * F(c["C"] // c["groups"]))
    ms = S * inv_count
    a = Q * inv_count
    b = ms * ms
    var = np.maximum(a - b, F(0))
    mean = ms + k
    rstd = rsqrt32(var + t.eps)
    return mean, rstd


def emu_map(mean, rstd, gamma, beta, cg):
    """sc = rstd gamma, sh = beta - mean sc per (sample, channel), two roundings in sh."""
    sc = np.repeat(rstd, cg, 1) * gamma.astype(F)
    p = np.repeat(mean, cg, 1) * sc
    return sc, beta.astype(F) - p


def emu_direct(t):
    cg = t.case["C"] // t.case["groups"]
    mean, rstd = emu_direct_stats(t)
    x = t.x.astype(F)
    if t.case["family"] == "gn0d":
        d = x - np.repeat(mean, cg, 1)[:, None, :]
        d = d * np.repeat(rstd, cg, 1)[:, None, :]
        d = d * t.gamma.astype(F)
        return d + t.beta.astype(F)
    sc, sh = emu_map(mean, rstd, t.gamma, t.beta, cg)
    y = x * sc[:, None, :]
    return y + sh[:, None, :]


def emu_table(t):
    """gn_table_kernel: the fold around the pivot with exact s1, s2, then the map in fp32."""
    c = t.case
    cg = c["C"] // c["groups"]
    piv, s1, s2, _, _, _ = pivot_sums(t)
    ntot = F(c["HW"]) * F(cg)
    dmean = f32_exact(s1, "s1") / ntot
    mean = piv.astype(F) + dmean
    var = np.maximum(f32_exact(s2, "s2") / ntot - dmean * dmean, F(0))
    rstd = rsqrt32(var + t.eps)
    return emu_map(mean, rstd, t.gamma, t.beta, cg) + (mean,)


def emu_from_stats(t):
    """gn_from_stats_kernel: mean = sum n_i mean_i / ntot (exact sum), second pass M2 = sum M2_i + n_i (mean_i - mean)^2 in fp32."""
    c = t.case
    G, cg = c["groups"], c["C"] // c["groups"]
    ntot = F(c["HW"]) * F(cg)
    mean = f32_exact(pivot_sums(t)[4], "sum n mean") / ntot
    mc = np.repeat(mean, cg, 1)
    cols, lo = [], 0
    for m, m2, n in chan_terms(t):
        dm = m.astype(F) - mc[:, None, lo:lo + m.shape[2]]
        cols.append((m2.astype(F) + F(n) * dm * dm).sum(1, dtype=F))
        lo += m.shape[2]
    acc = np.concatenate(cols, -1).reshape(c["B"], G, cg).sum(-1, dtype=F)
    rstd = rsqrt32(acc / ntot + t.eps)
    return emu_map(mean, rstd, t.gamma, t.beta, cg)


def emu_sums(t):
    """gn_apply_table_kernel<true>: the group's fixed-point sums in fp64, (mean, var) rounded to fp32 once."""
    c = t.case
    G, cg = c["groups"], c["C"] // c["groups"]
    s = np.concatenate([N.fixed_point_sums(t, w).reshape(c["B"], -1, 2) for w in range(2 if c["c1"] else 1)], 1).astype(np.float64)
    s = s.reshape(c["B"], G, cg, 2).sum(2)
    n = float(c["HW"]) * cg
    mean = s[..., 0] / (4294967296.0 * n)
    var = np.maximum(s[..., 1] / (65536.0 * n) - mean * mean, 0.0)
    return emu_map(mean.astype(F), rsqrt32(var.astype(F) + t.eps), t.gamma, t.beta, cg)


def assert_half(out16, ref, scale, case, act, what):
    msg = N.mismatch(out16, ref, scale, case, act, what)
    assert msg is None, msg
    top = N.share(out16, ref, np.broadcast_to(scale, ref.shape), act).max()
    assert top <= 0.5, "%s %s: the emulation uses %.2f of the allowance" % (case["name"], what, top)
    return top


@pytest.mark.parametrize("name", N.names("direct") + N.names("gn0d"))
def test_emulation_of_the_direct_kernels(name):
    t = N.build(name)
    y = emu_direct(t)
    assert_half(y.astype(np.float16), t.y, t.scale, t.case, False, "plain")
    assert_half(silu32(y).astype(np.float16), N.silu(t.y), t.scale, t.case, True, "silu")


@pytest.mark.parametrize("name", N.names("stats"))
def test_emulation_of_the_stats_fed_kernels(name):
    t = N.build(name)
    c = t.case
    sc, sh, _ = emu_table(t)
    assert N.mismatch_f32(sc, t.sc, N.K * N.U * np.abs(t.sc) / 2, c, "table scale") is None
    assert N.mismatch_f32(sh, t.sh, N.K * N.U * t.base / 2, c, "table shift") is None
    x = t.x.astype(F)
    for what, (a, b) in (("table", (sc, sh)), ("from_stats", emu_from_stats(t)), ("sums", emu_sums(t))):
        y = fma32(x, a[:, None, :], b[:, None, :])
        assert_half(y.astype(np.float16), t.y, t.scale, c, False, what)
        assert_half(silu32_rcp(y).astype(np.float16), N.silu(t.y), t.scale, c, True, what + " silu")


def centered_shift_ref(t, center):
    """float64 shift' = beta - (mean - center) sc of the centred fp16 map, for the center the kernel chose (fp16(mean): either
    neighbour next to a tie), and the magnitude its fp32 roundings scale with."""
    cg = t.case["C"] // t.case["groups"]
    dm = np.repeat(t.mean, cg, 1) - center
    return t.beta.astype(np.float64) - dm * t.sc, np.abs(t.beta.astype(np.float64)) + (np.abs(dm) + N.U * np.abs(center)) * np.abs(t.sc)


@pytest.mark.parametrize("name", N.names("affine"))
def test_emulation_of_the_affine_outputs(name):
    """gn_affine_kernel (scale, shift as fp16) and, with block statistics, the fp16 outputs of gn_table_kernel, plain and centred."""
    t = N.build(name)
    c = t.case
    sc, sh = emu_map(*emu_direct_stats(t), t.gamma, t.beta, c["C"] // c["groups"])
    assert_half(sc.astype(np.float16), t.sc, np.abs(t.sc), c, False, "scale")
    assert_half(sh.astype(np.float16), t.sh, t.base, c, False, "shift")
    if c["R0"]:
        sc, sh, mean = emu_table(t)
        mc = np.repeat(mean, c["C"] // c["groups"], 1)
        assert_half(sc.astype(np.float16), t.sc, np.abs(t.sc), c, False, "scale16")
        assert_half(sh.astype(np.float16), t.sh, t.base, c, False, "shift16")
        c16 = mc.astype(np.float16)
        assert_half(c16, np.repeat(t.mean, c["C"] // c["groups"], 1), np.abs(mc), c, False, "center16")
        d = (mc - c16.astype(F)) * sc
        ref, mag = centered_shift_ref(t, c16.astype(np.float64))
        assert_half((t.beta.astype(F) - d).astype(np.float16), ref, mag, c, False, "centred shift16")


@pytest.mark.parametrize("name", N.names("ln"))
def test_emulation_of_layernorm(name):
    """layernorm_kernel: mean = s / C (exact), q = sum (v - mean)^2 (exact), rstd = rsqrt(q / C + eps), (v - mean) rstd gamma + beta."""
    t = N.build(name)
    C = t.case["C"]
    x = t.x.astype(F)
    mean = f32_exact(t.ints.sum(1) * t.step, "s") / F(C)
    dlt = x - mean[:, None]
    q = f32_exact((dlt.astype(np.float64) ** 2).sum(1), "q")
    rstd = rsqrt32(q / F(C) + t.eps)
    y = dlt * rstd[:, None]
    y = y * t.gamma.astype(F)
    y = y + t.beta.astype(F)
    assert np.array_equal(mean.astype(np.float64), t.mean)
    assert_half(y.astype(np.float16), t.y, t.scale, t.case, False, "layernorm")


@pytest.mark.parametrize("name", N.names("rows"))
def test_emulation_of_row_stats(name):
    t = N.build(name)
    C = t.case["C"]
    mean = f32_exact(t.ints.sum(1) * t.step, "s") / F(C)
    q = f32_exact(((t.x[:, :C].astype(F) - mean[:, None]).astype(np.float64) ** 2).sum(1), "q")
    rstd = rsqrt32(q / F(C) + t.eps)
    assert np.array_equal(mean.astype(np.float64), t.mean)
    assert N.mismatch_f32(rstd, t.rstd, N.RSTD_ROWS_REL * t.rstd / 2, t.case, "rstd") is None


# ---- the rule discriminates ---------------------------------------------------------------------------------------------------------

def _y(t, mean=None, var=None, gamma=None, beta=None, x=None):
    c = t.case
    sc, sh, base = N.affine_map(t.mean if mean is None else mean, t.var if var is None else var, t.gamma if gamma is None else gamma,
                                t.beta if beta is None else beta, t.eps, c["C"] // c["groups"])
    return N.apply_map(t.x if x is None else x, sc, sh, base)[0]


def _rejected(t, y, touched, what, refs, report=False):
    for act in (False, True):
        out = (N.silu(y) if act else y).astype(np.float16)
        bad = N.bad_groups(out, refs[act], t.scale, t.case, act)
        miss = np.argwhere(touched & ~bad)
        assert len(miss) == 0, "%s: %s%s is accepted in (sample, group) %s" % (t.case["name"], what, " + silu" if act else "", miss[:8].tolist())
        if report and not act:     # the report names the case, the first element with its group and place, and the groups that fail
            msg = N.mismatch(out, refs[act], t.scale, t.case, act, what)
            assert msg.startswith(t.case["name"]) and "group" in msg and "failures per (sample, group)" in msg and "sample 0, row 0" in msg


@pytest.mark.parametrize("name", GN_Y)
def test_rule_rejects_wrong_statistics_affine_rows_and_counts(name):
    t = N.build(name)
    c = t.case
    B, HW, C, G = c["B"], c["HW"], c["C"], c["groups"]
    cg = C // G
    every = np.ones((B, G), bool)
    refs = {False: t.y, True: N.silu(t.y)}
    _rejected(t, _y(t, mean=np.roll(t.mean, 1, 1), var=np.roll(t.var, 1, 1)), every, "the statistics of the neighbouring group", refs, True)
    _rejected(t, _y(t, mean=np.roll(t.mean, 1, 0), var=np.roll(t.var, 1, 0)), every, "the statistics of the other sample", refs)
    ax = 0 if c["family"] == "gn0d" else -1       # 0-D: gamma / beta [S, C] taken at the wrong s
    _rejected(t, _y(t, gamma=np.roll(t.gamma, 1, ax), beta=np.roll(t.beta, 1, ax)), every, "gamma / beta shifted by one %s" % ("s" if ax == 0 else "channel"), refs)
    _rejected(t, _y(t, x=np.roll(t.x, -1, 1)), every, "x taken one row later", refs)
    k, S, Q, _ = shifted_sums(t)
    n1 = (HW + 1) * cg
    _rejected(t, _y(t, mean=S / n1 + k, var=Q / n1 - (S / n1) ** 2), every, "inv_count off by one row", refs)
    if c["c1"]:      # the group's shift k_g read at the same offset of the other source
        first = np.arange(G) * cg
        other = np.where(first < c["c0"], c["c0"] + first % c["c1"], (first - c["c0"]) % c["c0"])
        kw = t.x[:, 0, other]
        _rejected(t, _y(t, mean=t.mean + (kw - k)), kw != k, "a group's shift taken from the other concat source", refs)
        assert (kw != k).mean() > 0.5


@pytest.mark.parametrize("name", N.names("ln"))
def test_rule_rejects_wrong_rows_and_affine_in_layernorm(name):
    t = N.build(name)
    c = t.case
    xd = t.x.astype(np.float64)
    g, b = t.gamma.astype(np.float64), t.beta.astype(np.float64)

    def y(x=xd, mean=t.mean, rstd=t.rstd, g=g, b=b):
        return (x - mean[:, None]) * rstd[:, None] * g + b

    def rejected(out, what):
        bad = ~(N.share(out.astype(np.float16), t.y, t.scale) <= 1.0)
        assert bool(bad.any(1).all()), "%s: %s is accepted in rows %s" % (c["name"], what, np.argwhere(~bad.any(1))[:8, 0].tolist())

    rejected(y(g=np.roll(g, 1), b=np.roll(b, 1)), "gamma / beta shifted by one channel")
    if c["rows"] > 1:
        rejected(y(mean=np.roll(t.mean, 1), rstd=np.roll(t.rstd, 1)), "the statistics of the neighbouring row")
        rejected(y(x=np.roll(xd, -1, 0), mean=np.roll(t.mean, -1)), "x taken one row later")
    rejected(y(rstd=1.0 / np.sqrt(t.var * c["C"] / (c["C"] + 8) + float(t.eps))), "a count off by one 8-channel chunk")


# ---- the dispatch mirror against the library's host code ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", N.names("direct") + N.names("affine"))
def test_dispatch_mirror_matches_the_library(name):
    from vd_hip.loader import lib
    c = N.CASES[name]
    B, HW, C, G = c["B"], c["HW"], c["C"], c["groups"]
    assert lib().vd_groupnorm_workspace_bytes(B, HW, C, G) == N.gn_workspace_bytes(B, HW, C, G)      # pins nchunk
    if c["family"] == "direct":
        p = N.gn_slab(HW, C, G)
        assert (p["nitem"] if p else 0) == c["nitem"], (p, c["nitem"])
        one = N.gn_slab(1, C, G)
        if p is None and one and -(-HW // one["rows_per_pass"]) == 13:       # one row past the slab limit: one row fewer takes the slab kernel
            assert N.gn_slab(HW - 1, C, G)["nitem"] == 12
        assert p is not None or one is None or HW in (613, 337, 301, 193, 700)


def test_case_comments_state_the_geometry():
    g = N.gn_geom(613, 1280)
    assert (g["R"], g["rows_per_chunk"], g["nchunk"], 613 - 51 * 12) == (1, 12, 52, 1) and 52 > 8 * (256 // 64) and 52 % 32 != 0
    g = N.gn_geom(700, 320)
    assert (g["TC"], g["R"], g["rows_per_chunk"], g["nchunk"], 700 - 12 * 54) == (40, 6, 54, 13, 52)
    g = N.gn_geom(337, 2304)
    assert (g["npos"], g["C8"] - g["TC"]) == (2, 32)
    assert N.gn_geom(193, 4096)["npos"] == 2 and N.gn_geom(193, 4096)["C8"] == 512
    p = N.gn_slab(64, 1280)
    assert (p["rows_per_pass"], p["items"], 64 - 51) == (51, 2, 13)
    p = N.gn_slab(256, 1280)
    assert (p["items"], 256 - 5 * 51) == (6, 1)
    assert N.gn_slab(576, 320)["slab"] == 40 and N.gn_slab(200, 160)["slab"] // 5 == 8 and N.gn_slab(512, 64)["rows_per_pass"] == 256
    assert N.gn_slab(100, 1920)["chunks"] == 15 and N.gn_slab(100, 1920)["rows_per_pass"] == 17
    assert 21 * 30 < 640 < 22 * 30                                          # group 21 spans the seam of 640 + 320
    assert 40 * (1024 // 64) > 512 and 4096 // 32 == 128                    # stats_deep, stats_cg128
    a = N.apply_geom(320, 320)
    assert (a["rows_per_chunk"], 320 % a["rows_per_chunk"]) == (30, 20)
    assert N.apply_geom(64, 4096)["npos"] == 2
    assert {c["nitem"] for c in N.CASES.values() if c["family"] == "direct"} == {0, 2, 6, 12}
    assert {c["nch"] for c in N.CASES.values() if c["family"] == "rows"} == {3, 5, 10, 16}
    assert N.K * N.U <= 2.0 ** -16 and N.K_SILU * N.U <= 2.0 ** -16
