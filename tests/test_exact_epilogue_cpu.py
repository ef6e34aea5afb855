"""The inputs of the per-element epilogue tests (tests/epilogue_cases.py), checked without a GPU: fp16-exact operands, partial sums
far below 2^24, the code-row properties and the fp32 model of the in-register LayerNorm, saturated gates, exact references that are
integers with few zeros, intervals of at most two adjacent fp16 values, and references that change when two rows, the two halves
of a GEGLU pair or two hidden chunks are exchanged."""
import numpy as np
import pytest
import torch

import epilogue_cases as E
from vdtest_util import EXACT_LIMIT, EXACT_ZERO_SHARE, check_exact_reference, exact_mismatch, fp16_steps, interval_mismatch, rel_l2

GEMM_CASES = E.names("gemm") + E.names("wstream_epi")
RC = ("row", "col")


def _fp16_exact(t, what):
    assert t.dtype == torch.float16 and bool(torch.isfinite(t).all()), what
    q = t.double() * 64.0
    assert torch.equal(q, q.round()) and t.abs().max().item() <= EXACT_LIMIT, "%s is not a small dyadic number" % what


def _code_row_properties(x, code, a, o, scaled, scales=(1.0, 2.0, 4.0)):
    M, C = code.shape
    assert bool((code.abs() == 1).all()) and bool((code.sum(1) == 0).all()), "a code row is not balanced"
    assert torch.unique(code, dim=0).shape[0] == M, "two rows share a code"
    assert set(a.tolist()) == set(scales)
    x64 = x.double()
    mean = x64.mean(1)
    assert torch.equal(mean, o) and torch.equal(((x64 - mean[:, None]) ** 2).mean(1), a * a)      # exactly o and a^2
    if scaled:
        assert float((o * o / (a * a)).max()) <= 9.0 and bool((o.abs()[2::3] == 3 * a[2::3]).all())
    else:       # every third row of the draw (replicas repeat the draw) has a large offset
        assert 0.3 < float((o.abs() >= 100).double().mean()) < 0.4 and float(o.abs().max()) <= 1000


def _ln_model_gives_the_code(x, code, o):
    """ff_fused.hip's in-register LayerNorm in fp32 hands exactly +-1 to the MFMA for every row, and still does with rstd moved by
    8 units of 2^-24 either way where |o| <= 100."""
    xn, cn = x.double().numpy(), code.numpy()
    assert np.array_equal(E.ln_rows_fp32(xn), cn)
    small = (o.abs() <= 100).numpy()
    assert small.sum() > 0.6 * len(small)
    for drift in (-8, 8):
        assert np.array_equal(E.ln_rows_fp32(xn[small], drift=drift), cn[small]), drift


def _rows_are_told_apart(val, what):
    """Exchanging row r with row r + 1, r + 32 or r + 128 (a lane, a wave tile, a block away) changes the answer."""
    v = np.asarray(val)
    for step in (1, 32, 128):
        if step < v.shape[0]:
            same = (v == np.roll(v, -step, 0)).all(1)
            assert not same.any(), "%s: rows %d apart are equal" % (what, step)


def _chunk_exchange_changes_the_output(t, ff):
    """Two hidden chunks exchanged in W1 alone, in b1 alone, or in W2 alone (a weight tile, a b1 slice or a W2 half of the
    neighbouring chunk) change most of the feed-forward's output."""
    C = E.FF_C
    order = list(range(20))
    order[3], order[4] = 4, 3
    w1, b1, w2, b2 = t.w1.double(), t.b1.double(), t.w2.double(), t.b2.double()
    swapped = {"w1": (w1.view(20, 128, C)[order].reshape(8 * C, C), b1, w2), "b1": (w1, b1.view(20, 128)[order].reshape(-1), w2),
               "w2": (w1, b1, w2.view(C, 20, 64)[:, order].reshape(C, 4 * C))}
    for what, (a, b, c) in swapped.items():
        v, g = E.split_packed((t.code @ a.t() + b[None, :]).numpy())
        h = torch.from_numpy(E.geglu_f64(v, g)).round()
        assert float((h @ c.t() + b2[None, :] != ff).double().mean()) > 0.5, what


def test_erf_model_saturates():
    """vd_erf in fp32 (vd_common.h) is exactly +-1 from |g| = 6 on (its argument is g / sqrt 2), so GELU is exactly g or 0 there."""
    g = np.arange(6 * 64, 30 * 64 + 1, dtype=np.float64) / 64.0
    z = (g.astype(np.float32) * np.float32(0.70710678118654752440)).astype(np.float32)
    assert np.array_equal(E.vd_erf_fp32(z), np.ones_like(g)) and np.array_equal(E.vd_erf_fp32(-z), -np.ones_like(g))
    # and within the stated bound of the true erf elsewhere
    x = np.linspace(-6.0, 6.0, 4001)
    true = np.vectorize(__import__("math").erf)(x.astype(np.float32).astype(np.float64))
    assert np.abs(E.vd_erf_fp32(x) - true).max() <= E.ERF_ABS


def test_every_kernel_has_cases():
    for k in ("gemm", "wstream_epi", "row320", "ff_geglu", "side", "ff_chain", "rowchain"):
        assert E.names(k), k
    for fold in E.FOLDS:     # every statistics source meets plain, GEGLU and each activation
        acts = {E.CASES[n]["act"] for n in E.names("gemm", fold=fold)}
        assert acts >= set(E.ACTS) - {"geglu_mid"}, (fold, acts)
    for key in ("alpha", "bias", "res", "K"):
        assert len({E.CASES[n][key] for n in E.names("gemm")}) == 2, key
    assert all(n in E.CASES for n in E.TILE_SWEEP)


@pytest.mark.parametrize("name", GEMM_CASES)
def test_gemm_case_preconditions(name):
    t = E.build(name)
    c = t.case
    M, N, K, fold, act = c["M"], c["N"], c["K"], c["fold"], c["act"]
    geglu = act.startswith("geglu")
    for nm in ("a", "w", "bias", "res"):
        if getattr(t, nm) is not None:
            _fp16_exact(getattr(t, nm), "%s.%s" % (name, nm))
    assert t.a.shape == (M, K) and t.w.shape == (N, K) and (t.bias is None) == (not c["bias"]) and (t.res is None) == (not c["res"])
    a64, w64 = t.a.double(), t.w.double()
    b = t.bias.double() if t.bias is not None else torch.zeros(N, dtype=torch.float64)
    assert float((a64.abs() @ w64.abs().t()).max() + b.abs().max()) <= 2.0 ** 22        # every partial sum, in any order
    acc = a64 @ w64.t()
    assert torch.equal(acc, acc.round())
    if fold != "off":
        _code_row_properties(t.a, t.code, t.a_scale, t.offset, scaled=True)
        assert bool(((w64 != 0).sum(1) % 2 == 1).all()) and bool((w64.abs() <= 1).all()) and bool((b % 2 == 0).all())
        d = t.code @ w64.t()
        assert torch.equal(acc, t.a_scale[:, None] * d + t.offset[:, None] * w64.sum(1)[None, :])
        assert bool(((d + b[None, :]) % 2 == 1).all())          # odd: no element of the pre-activation is zero
        # o colsum: the fp32 error of nmr * colsum stays below a quarter of the fp16 half-spacing at the smallest expected value
        oc = 3 * E.U * float(((t.offset / t.a_scale).abs()[:, None] * w64.sum(1).abs()[None, :]).max())
        assert oc <= 0.25 * 2.0 ** -12 * min(1.0, abs(c["alpha"])), oc
        assert torch.equal(t.ln_sums, E.W.row_sums_fixed(t.a))
    gates = None
    if geglu:
        v, gates = E.split_packed(t.y)
        dg = E.split_packed(t.dy)[1]
        gm = E.gate_mask(N)
        assert bool((gm.view(-1, 64)[:, :32] == 0).all()) and bool(gm.view(-1, 64)[:, 32:].all())
        if act == "geglu_sat":
            assert float((np.abs(gates) - dg).min()) >= E.GATE_SAT
            sign = (t.bias.double()[gm] > 0).view(-1, 32)
            assert bool((sign.any(1) & (~sign).any(1)).all()), "a 32-column group has gates of one sign only"
            assert float(np.abs(v * gates).max()) <= EXACT_LIMIT
        else:
            assert gates.min() >= E.GATE_MIN and gates.max() <= E.ARG_MAX and gates.min() < -2.0 and gates.max() > 10.0
    elif act != "none":
        assert np.abs(t.y).max() <= E.ARG_MAX and t.y.min() < -8.0 and t.y.max() > 8.0, (t.y.min(), t.y.max())
    steps = fp16_steps(t.tlo, t.thi)
    assert steps.min() >= 0 and steps.max() <= 1, "an interval holds more than two adjacent fp16 values"
    if t.exact:
        assert np.array_equal(t.lo, t.hi), "an exact case leaves the kernel a choice"
        ref = t.ref
        opened = torch.from_numpy(gates > 0) if geglu else torch.ones_like(ref, dtype=torch.bool)
        assert bool((ref[~opened] == 0).all())
        if geglu:
            assert 0.5 < opened.double().mean().item() < 0.85
        check_exact_reference(ref[opened], t.unit, name)
        assert float(np.abs(t.val - ref.numpy()).max()) <= (1e-9 if fold == "off" else 0.02), "the float64 value is far from its integer"
    else:
        assert (steps == 1).mean() < 0.1 and (np.asarray(t.val) == 0).mean() < EXACT_ZERO_SHARE
    _rows_are_told_apart(t.val, name)


@pytest.mark.parametrize("name", GEMM_CASES)
def test_gemm_reference_notices_mislocated_operands(name):
    """Every case tells apart what a kernel could get wrong, and the acceptance rule reports it with its row and column: the two
    halves of a GEGLU pair (bias and weights) exchanged, a bias that skipped pack_geglu, a bias or colsum entry of the neighbouring
    column, the statistics of the neighbouring row, alpha applied in front of the activation.  (The GPU module feeds the same
    mislocated operands to the kernels from the host side.)"""
    t = E.build(name)
    c = t.case

    def located(what, **kw):
        # (the general GELU formula: a mislocated operand need not leave the gates saturated)
        args = dict(a=t.a, w=t.w, bias=t.bias, res=t.res, fold=c["fold"], act=c["act"].replace("geglu_sat", "geglu_mid"), alpha=c["alpha"])
        args.update(kw)
        wrong = E.gemm_expect(**args)
        for end in (wrong.lo, wrong.hi):
            msg = interval_mismatch(torch.from_numpy(end), t.lo, t.hi, RC, "%s, %s" % (name, what))
            assert msg is not None and "row=" in msg and "col=" in msg, (name, what)

    if c["act"].startswith("geglu"):
        swap = lambda v: v.reshape((-1, 2, 32) + v.shape[1:]).flip(1).reshape(v.shape).contiguous()
        located("value and gate bias exchanged", bias=swap(t.bias))
        located("value and gate rows exchanged", w=swap(t.w), colsum=t.colsum)
        located("bias not packed", bias=E.unpack_geglu_vector(t.bias))
    if c["bias"]:
        located("bias of the neighbouring column", bias=torch.roll(t.bias, 1, 0))
    if c["fold"] != "off":
        located("colsum of the neighbouring column", colsum=torch.roll(t.colsum, 1, 0))
        located("statistics of the neighbouring row", stat_rows=torch.roll(t.a, 1, 0))
    if c["act"] in E.ACT_C and c["alpha"] != 1.0:
        early = E.to_f16(E.act_f64(c["act"], t.y * c["alpha"]))
        if t.res is not None:
            early = E.add_f16(early, t.res.double().numpy())
        assert interval_mismatch(torch.from_numpy(early), t.lo, t.hi, RC, name) is not None


def test_a_wrong_colsum_entry_on_a_ragged_tile_passes_the_aggregate_bound_and_fails_per_element():
    """A LayerNorm-folded projection that reads the colsum entry of the neighbouring column for ONE column in the rows of its ragged
    last tile (5 rows behind 4096): with Gaussian operands as in test_gemm_layernorm_fold the result stays under that test's
    rel_l2 < 3e-3; with the code rows of this table the same defect is a mismatch located in that column and those rows."""
    g = torch.Generator(device="cpu").manual_seed(50)
    M, K, N, col = 4096 + 5, 320, 320, 7
    x = (torch.randn((M, K), generator=g) * 1.5 + 0.5).half().double()
    w = (torch.randn((N, K), generator=g) * 0.05).half().double()
    mean, var = x.mean(1), x.var(1, unbiased=False)
    rstd, cs = (var + 1e-5).rsqrt(), w.sum(1)
    true = rstd[:, None] * (x @ w.t() - mean[:, None] * cs[None, :])
    wrong = true.clone()
    wrong[4096:, col] = rstd[4096:] * ((x @ w.t())[4096:, col] - mean[4096:] * cs[col - 1])
    assert 0 < rel_l2(wrong.half(), true) < 3e-3                  # invisible to the aggregate bound ...
    t = E.build("gemm_table_none")
    c = t.case
    cs = t.colsum.clone()
    col = next(n for n in range(1, c["N"]) if cs[n] != cs[n - 1])      # (small integers: neighbours can be equal)
    cs[col] = cs[col - 1]
    bad = E.gemm_expect(t.a, t.w, t.bias, t.res, c["fold"], c["act"], c["alpha"], colsum=cs).lo
    out = t.ref.clone()
    out[256:] = torch.from_numpy(bad)[256:]
    msg = exact_mismatch(out, t.ref, RC, "ragged tile")
    assert msg is not None and "extent: row 25" in msg and "col %d..%d" % (col, col) in msg, msg      # ... and located per element


@pytest.mark.parametrize("name", E.names("row320"))
def test_row320_case_preconditions(name):
    t = E.build(name)
    c = t.case
    for nm in ("x", "w", "bias", "res"):
        if getattr(t, nm) is not None:
            _fp16_exact(getattr(t, nm), "%s.%s" % (name, nm))
    _code_row_properties(t.x, t.code, t.a_scale, t.offset, scaled=False)
    _ln_model_gives_the_code(t.x, t.code, t.offset)
    assert float(t.w.double().abs().sum(1).max()) + 16 <= 2.0 ** 22
    check_exact_reference(t.ref, 1.0, name)
    _rows_are_told_apart(t.ref.numpy(), name)
    groups = t.w.view(c["N"] // 320, 320, 320)      # the column groups of MULTI stream through the same slots: all different
    for i in range(groups.shape[0]):
        for j in range(i + 1, groups.shape[0]):
            assert not torch.equal(groups[i], groups[j])
    kt = t.w.view(c["N"], 5, 64)                    # and so are the five 64-deep K tiles of every group
    assert all(not torch.equal(kt[:, i], kt[:, j]) for i in range(5) for j in range(i + 1, 5))


@pytest.mark.parametrize("name", E.names("ff_geglu"))
def test_ff_geglu_case_preconditions(name):
    t = E.build(name)
    C = E.FF_C
    for nm in ("x", "w1", "b1", "w2", "b2", "res"):
        _fp16_exact(getattr(t, nm), "%s.%s" % (name, nm))
    _code_row_properties(t.x, t.code, t.a_scale, t.offset, scaled=False)
    _ln_model_gives_the_code(t.x, t.code, t.offset)
    # the 20 hidden chunks (128 packed rows of W1 / b1, 64 columns of W2) and the two 160-row halves of W2 all differ
    w1c, b1c, w2c = t.w1.view(20, 128, C), t.b1.view(20, 128), t.w2.view(C, 20, 64)
    for i in range(20):
        for j in range(i + 1, 20):
            assert not torch.equal(w1c[i], w1c[j]) and not torch.equal(b1c[i], b1c[j]) and not torch.equal(w2c[:, i], w2c[:, j]), (i, j)
        assert not torch.equal(w2c[:160, i], w2c[160:, i]), i
    pre = t.code @ t.w1.double().t() + t.b1.double()[None, :]
    v, g = E.split_packed(pre.numpy())
    assert np.array_equal(v, t.v) and np.array_equal(g, t.gate)
    if t.exact:
        assert float(np.abs(g).min()) >= E.GATE_SAT
        assert np.array_equal(t.h, np.rint(t.h)) and float(np.abs(t.h).max()) <= EXACT_LIMIT
        y = torch.from_numpy(t.h) @ t.w2.double().t() + t.b2.double()[None, :]
        assert float((torch.from_numpy(np.abs(t.h)) @ t.w2.double().abs().t()).max()) + 12 <= EXACT_LIMIT      # every later sum
        check_exact_reference(y, 1.0, name + " before the residual")
        check_exact_reference(t.ref, 1.0, name)
        final = t.ref.numpy()
        _chunk_exchange_changes_the_output(t, y)
    else:
        assert g.min() >= E.GATE_MIN and g.max() <= E.ARG_MAX and g.min() < -2.0 and g.max() > 10.0
        steps = fp16_steps(t.hlo, t.hhi)
        assert steps.min() >= 0 and steps.max() <= 1 and (steps == 1).mean() < 0.1
        assert len(set(t.sel.tolist())) == C and set((t.sel // 64).tolist()) == set(range(20))     # every chunk is gathered from
        s = t.w2.double()[torch.arange(C), t.sel]
        assert bool(((t.w2 != 0).sum(1) == 1).all()) and set(s.tolist()) <= {0.5, 1.0, 2.0}
        assert float(np.abs(t.val).max()) <= EXACT_LIMIT and (t.val == 0).mean() < EXACT_ZERO_SHARE
        final = t.val
    _rows_are_told_apart(final, name)


def test_side_output_case_preconditions():
    """Stored rows so small that the fp32 sums of the side outputs are exact: row sums of squares below 2^24, and for every block
    size a launch may choose the shifted sums S, Q of emit_chan_stats (gemm_kernel.h) and m2 = Q - S * S / n in float32 equal to
    float64."""
    t = E.build("side_outputs")
    c = t.case
    check_exact_reference(t.ref, 1.0, "side_outputs")
    v = t.ref
    assert float(v.abs().max()) <= 32 and float((v * v).sum(1).max()) < 2.0 ** 24
    for R in (16, 32, 64, 128):
        blk = v.view(c["M"] // R, R, c["N"])
        d = blk - blk[:, :1, :]
        S, Q = d.sum(1), (d * d).sum(1)
        assert float(S.abs().max()) < 4096 and float(Q.max()) < 2.0 ** 24          # S * S < 2^24: exact in fp32
        m2 = (Q.numpy().astype(np.float32) - (S.numpy().astype(np.float32) ** 2) / np.float32(R)).astype(np.float64)
        mean = (blk[:, 0, :].numpy().astype(np.float32) + S.numpy().astype(np.float32) / np.float32(R)).astype(np.float64)
        part = E.side_expect(v, c["img_rows"], R)[2].numpy()
        assert np.array_equal(mean, part[..., 0]) and np.array_equal(np.maximum(m2, 0.0), part[..., 1]), R


@pytest.mark.parametrize("name", E.names("ff_chain"))
def test_ff_chain_case_preconditions(name):
    t = E.build(name)
    c = t.case
    C, M, P = E.FF_C, c["M"], t.P
    for nm in ("x", "a", "wo", "bo", "w1", "b1", "w2", "b2", "wp", "bp", "res"):
        if getattr(t, nm) is not None:
            _fp16_exact(getattr(t, nm), "%s.%s" % (name, nm))
    assert P % 128 == 0 or c["repeat"] == 1
    # x1 is a code row, balanced in its even and in its odd columns, and the in-register LayerNorm turns it into the code
    _code_row_properties(t.x1, t.code, t.a_scale, t.offset, scaled=False)
    assert bool((t.code[:, 0::2].sum(1) == 0).all()) and bool((t.code[:, 1::2].sum(1) == 0).all())
    _ln_model_gives_the_code(t.x1, t.code, t.offset)
    if c["pre"]:
        proj = t.a.double() @ t.wo.double().t()
        assert bool((proj[:, 1::2] == 0).all()) and bool((proj[:, 0::2] != 0).all())          # the projection: the even columns only
        x0 = t.x.double()
        assert bool((x0[:, 0::2] == x0[:, :1]).all())                                           # x0: the code in the odd columns only
        assert bool((x0[:, 1::2] - x0[:, :1]).abs().eq(t.a_scale[:P, None]).all())
        idx = torch.arange(M) % P
        assert torch.equal(proj + t.bo.double()[None, :] + x0[idx], t.x1)
        assert float(proj.abs().max() + 3) <= EXACT_LIMIT and float((t.a.double().abs() @ t.wo.double().abs().t()).max()) <= 2.0 ** 22
        assert torch.unique(x0, dim=0).shape[0] == P                                            # a residual row of its own for every row
    if c["repeat"] > 1:
        first = t.a if c["pre"] else t.x
        assert not bool((first[:P] == first[P:]).all(1).any()), "a replica repeats a row of the other one"
    assert float(np.abs(t.gate).min()) >= E.GATE_SAT
    assert np.array_equal(t.h, np.rint(t.h)) and float(np.abs(t.h).max()) <= EXACT_LIMIT
    w2 = t.w2.double()
    assert float((torch.from_numpy(np.abs(t.h)) @ w2.abs().t()).max() + 4 + t.x1.abs().max()) <= EXACT_LIMIT       # every sum behind h
    check_exact_reference(t.ff, 1.0, name + ", feed-forward")
    check_exact_reference(t.y, 1.0, name + ", y")
    w1c, b1c, w2c = t.w1.view(20, 128, C), t.b1.view(20, 128), t.w2.view(C, 20, 64)
    for i in range(20):
        for j in range(i + 1, 20):
            assert not torch.equal(w1c[i], w1c[j]) and not torch.equal(b1c[i], b1c[j]) and not torch.equal(w2c[:, i], w2c[:, j]), (i, j)
    _chunk_exchange_changes_the_output(t, t.ff)
    if c["post"]:
        wp = t.wp.double()
        assert bool(((wp != 0).sum(1) == 2).all()) and bool((wp.sum(1) == 0).all())
        assert float((t.y.abs() @ wp.abs().t()).max() + 4) <= 2.0 ** 22
        check_exact_reference(t.proj, c["alpha"], name + ", alpha (y Wp^T + bp)")
        assert torch.unique(t.res, dim=0).shape[0] == P
    check_exact_reference(t.ref, t.unit, name)
    _rows_are_told_apart(t.ref.numpy(), name)
    if c["repeat"] > 1:
        assert not bool((t.ref[:P] == t.ref[P:]).all(1).any())


@pytest.mark.parametrize("name", E.names("rowchain"))
def test_rowchain_case_preconditions(name):
    t = E.build(name)
    c = t.case
    for nm in ("x", "sc", "sh", "ctr", "w1", "b1", "w2", "b2"):
        if getattr(t, nm) is not None:
            _fp16_exact(getattr(t, nm), "%s.%s" % (name, nm))
    imgs = c["M"] // c["rows_per_image"]
    assert imgs >= 2 and set(t.sc.unique().tolist()) == {0.5, 1.0} and (t.ctr is None) == (not c["centred"])
    for v in (t.sc, t.sh) + ((t.ctr,) if t.ctr is not None else ()):
        assert all(not torch.equal(v[i], v[j]) for i in range(imgs) for j in range(i + 1, imgs)), "two images share a map"
    # the packed fp16 map is exact: every intermediate is an integer or a half of one, far inside fp16
    img = torch.arange(c["M"]) // c["rows_per_image"]
    cen = t.x.double() - (t.ctr.double()[img] if t.ctr is not None else 0.0)
    prod = cen * t.sc.double()[img]
    for v in (cen, prod, prod + t.sh.double()[img]):
        assert torch.equal(v.half().double(), v)
    assert torch.equal(prod + t.sh.double()[img], t.xm)
    w1 = t.w1.double()
    assert float((t.xm.abs() @ w1.abs().t()).max() + 3) <= 2.0 ** 22
    assert torch.equal(t.xm @ w1.t() + t.b1.double()[None, :], t.ref_h)
    assert float(t.ref_h.abs().max()) <= EXACT_LIMIT and torch.equal(t.ref_h, t.ref_h.round())
    _rows_are_told_apart(t.ref_h.numpy(), name)
    if c["family"] == "dense":
        check_exact_reference(t.ref_h, 1.0, name + ", h")
        assert t.ref_y2 is None
    else:
        assert bool(((w1 != 0).sum(1) == 1).all()) and bool(((w1 != 0).sum(0) == 1).all()) and set(w1.unique().tolist()) == {0.0, 2.0}
        assert len(t.b1.unique()) == 1
        _code_row_properties(t.ref_h.half(), t.code, t.a_scale, t.offset, scaled=False, scales=(2.0, 4.0, 8.0))
        _ln_model_gives_the_code(t.ref_h, t.code, t.offset)
        check_exact_reference(t.ref_y2, 1.0, name + ", y2")
        _rows_are_told_apart(t.ref_y2.numpy(), name + ", y2")
        groups = t.w2.view(c["N2"] // 320, 320, 320)
        assert all(not torch.equal(groups[i], groups[j]) for i in range(3) for j in range(i + 1, 3))
