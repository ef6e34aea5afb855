"""The fused GEMM epilogues and the one-launch kernels of the 64x64 level, element by element against float64.

The operands of tests/epilogue_cases.py leave a kernel no rounding freedom (tests/test_exact_epilogue_cpu.py proves that without a
GPU): an exact case must equal its reference in every element (vdtest_util.assert_exact), an interval case must return one of the
at most two adjacent fp16 values its float64 value can round to (vdtest_util.interval_mismatch).  Covered: gemm_f16_kernel's
epilogue (LayerNorm fold from all three statistics sources, GEGLU, the activations, alpha, the residual after the fp16 rounding,
row_sums / out_stats / stat_sums) under the planner and every instantiated tile, gemm_wstream_epi_kernel against float64 itself,
rowgemm320_kernel<LN> with one and several column groups, ff_geglu_kernel, ff_chain_kernel in every instantiated (PRE, POST, REP)
form and rowchain320_kernel.  The last test feeds mislocated operands from the host side and requires a located mismatch for each."""
import pytest
import torch

import epilogue_cases as E
from vdtest_util import assert_exact, exact_mismatch, interval_mismatch

pytestmark = pytest.mark.gpu

RC = ("row", "col")


@pytest.fixture(scope="module")
def ops():
    from vd_hip import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from vd_hip.loader import lib as l
    return l()


def _profiled(ops, fn):
    ops.profile_begin()
    try:
        out = fn()
    finally:
        names = [r[0] for r in ops.profile_end()]
    return out, [n for n in names if n != "row_stats_kernel"]


def _built_configs(lib):
    """Every instantiated tile configuration (slots of removed development tiles refuse); restore with ops.gemm_set_override(-1)."""
    for cfg in range(lib.vd_gemm_num_configs()):
        if lib.vd_gemm_set_override(cfg) == 0:
            yield cfg


def _mismatch(t, out, ctx):
    if t.exact:
        return exact_mismatch(out, t.ref, RC, ctx)
    return interval_mismatch(out, t.lo, t.hi, RC, ctx)


def _act_code(ops, act):
    return {"none": ops.ACT_NONE, "geglu_sat": ops.ACT_GEGLU, "geglu_mid": ops.ACT_GEGLU, "quick_gelu": ops.ACT_QUICK_GELU,
            "silu": ops.ACT_SILU, "gelu_tanh": ops.ACT_GELU_TANH}[act]


def _gemm(ops, dev, t, monkeypatch, stream=False, **swap):
    """The launch of a gemm / wstream_epi case -> (out, kernel names without the statistics launch).  swap: operands replaced from
    the host side (bias, colsum, ln_sums).  stream: hand the fragment-order pack over (gemm_wstream_epi_kernel)."""
    from vd_hip.pack import pack_linear_weight_stream
    c = t.case
    monkeypatch.setattr(ops, "LN_INLOOP", c["fold"] == "inloop")
    monkeypatch.setattr(ops, "LN_SUMS", True)
    monkeypatch.setattr(ops, "GEMM_WSTREAM_EPI", True)
    put = lambda v: None if v is None else v.to(dev)
    kw = dict(bias=put(swap.get("bias", t.bias)), res=put(t.res), act=_act_code(ops, c["act"]), alpha=c["alpha"])
    if c["fold"] != "off":
        kw.update(colsum=put(swap.get("colsum", t.colsum)), ln_eps=E.LN_EPS)
    if c["fold"] == "sums":
        kw.update(ln_sums=put(swap.get("ln_sums", t.ln_sums)))
    w = t.w.to(dev)
    if stream:
        kw.update(w_stream_epi=pack_linear_weight_stream(w))
    a = t.a.to(dev)
    return _profiled(ops, lambda: ops.gemm(a, w, **kw))


# ---- gemm_f16_kernel ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.names("gemm"))
def test_gemm_epilogue_under_the_planner(ops, dev, name, monkeypatch):
    t = E.build(name)
    out, names = _gemm(ops, dev, t, monkeypatch)
    assert len(names) == 1 and names[0].startswith("gemm_f16_kernel"), names
    msg = _mismatch(t, out, "%s (%s)" % (name, names[0]))
    assert msg is None, msg


@pytest.mark.parametrize("name", E.TILE_SWEEP)
def test_gemm_epilogue_on_every_tile(ops, lib, dev, name, monkeypatch):
    """The epilogue is instantiated per tile (the 320-column tile takes it in two passes): the LayerNorm fold, the fold with GEGLU and
    an activation on every forced tile.  A forced tile that cannot take the launch is replaced by plan_gemm -- a GEGLU launch on a
    tile without 128-column pairs keeps the planner's tile, a folded launch moves to the tile's fold instance -- so the profiled
    name is asserted: the forced tile for the plain activation case, some built gemm_f16_kernel tile otherwise, and more than one
    tile over the sweep."""
    t = E.build(name)
    c = t.case
    seen = set()
    try:
        cfgs = list(_built_configs(lib))
        built = {ops.gemm_kernel_name(cfg) for cfg in cfgs}
        for cfg in cfgs:
            ops.gemm_set_override(cfg)
            out, names = _gemm(ops, dev, t, monkeypatch)
            assert len(names) == 1 and names[0].startswith("gemm_f16_kernel") and names[0] in built, (cfg, names)
            if c["fold"] == "off" and not c["act"].startswith("geglu"):
                assert names[0] == ops.gemm_kernel_name(cfg), (cfg, names)
            seen.add(names[0])
            msg = _mismatch(t, out, "%s, override %d (%s)" % (name, cfg, names[0]))
            assert msg is None, msg
    finally:
        ops.gemm_set_override(-1)
    assert len(cfgs) >= 9 and len(seen) >= (2 if c["act"].startswith("geglu") else 5), seen


def test_gemm_side_outputs(ops, dev, monkeypatch):
    """row_sums (int64 pairs: sum x 2^24, sum of squares x 2^16 of the STORED fp16 row), stat_sums (sum x 2^32, sum of squares x 2^16 per
    image and channel) and the out_stats (mean, M2) partials on an integer result: every fp32 sum involved is exact (the CPU module
    proves it for each block size), so all three equal float64 on the stored values without a tolerance."""
    monkeypatch.setattr(ops, "GN_SUMS", True)
    monkeypatch.setattr(ops, "GN_FUSED_MAX", 0)
    monkeypatch.setattr(ops, "LN_SUMS", True)
    t = E.build("side_outputs")
    c = t.case
    M, N, hw = c["M"], c["N"], c["img_rows"]
    a, w, b, r = t.a.to(dev), t.w.to(dev), t.bias.to(dev), t.res.to(dev)
    sums = ops.rowsum_take(M, dev)
    out, names = _profiled(ops, lambda: ops.gemm(a, w, bias=b, res=r, row_sums=sums))
    assert len(names) == 1 and names[0].startswith("gemm_f16_kernel"), names
    assert_exact(out, t.ref, RC, "side_outputs, row_sums")
    got = getattr(out, "_vd_rowsums", None)
    assert got is not None, "the planned launch (%s) did not take row_sums" % names[0]
    out2, names = _profiled(ops, lambda: ops.gemm(a, w, bias=b, res=r, want_stats=True, stat_img_rows=hw))
    assert_exact(out2, t.ref, RC, "side_outputs, statistics")
    st = ops.stats_of(out2)
    assert st is not None and st.sums is not None, "the planned launch (%s) did not emit statistics and sums" % names[0]
    R = hw // st.T
    assert R in (16, 32, 64, 128) and st.buf.shape == (M // R, N, 2), (R, st.buf.shape)
    rows, csum, part = E.side_expect(t.ref, hw, R)
    bad = (got.cpu() != rows).nonzero()
    assert bad.shape[0] == 0, "row_sums: %d entries differ, first (row, which) %s" % (bad.shape[0], bad[:4].tolist())
    bad = (st.sums.view(M // hw, N, 2).cpu() != csum).nonzero()
    assert bad.shape[0] == 0, "stat_sums: %d entries differ, first (image, channel, which) %s" % (bad.shape[0], bad[:4].tolist())
    assert_exact(st.buf, part, ("partial", "channel", "mean / M2"), "out_stats, partials of %d rows" % R)


# ---- gemm_wstream_epi_kernel ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.names("wstream_epi"))
def test_weight_streaming_epilogue_against_float64(ops, dev, name, monkeypatch):
    t = E.build(name)
    out, names = _gemm(ops, dev, t, monkeypatch, stream=True)
    assert names == ["gemm_wstream_epi_kernel" + (" geglu" if t.case["act"].startswith("geglu") else "")], names
    msg = _mismatch(t, out, name)
    assert msg is None, msg


# ---- rowgemm320_kernel<LN = true, MULTI> ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.names("row320"))
def test_row_resident_gemm_with_layernorm(ops, lib, dev, name):
    t = E.build(name)
    c = t.case
    assert lib.vd_gemm_row320_supported(c["M"], c["N"], 320) == 1
    x, w, b = t.x.to(dev), t.w.to(dev), t.bias.to(dev)
    res = None if t.res is None else t.res.to(dev)
    out, names = _profiled(ops, lambda: ops.gemm_row320(x, w, b, res, True, E.LN_EPS))
    assert names == ["rowgemm320_kernel"], names
    assert_exact(out, t.ref, RC, name)


# ---- ff_geglu_kernel -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.names("ff_geglu"))
def test_fused_feed_forward(ops, dev, name):
    t = E.build(name)
    assert ops.ff_geglu_supported(E.FF_C)
    x, w1, b1, w2, b2, res = [v.to(dev) for v in (t.x, t.w1, t.b1, t.w2, t.b2, t.res)]
    out, names = _profiled(ops, lambda: ops.ff_geglu(x, w1, b1, w2, b2, res, E.LN_EPS))
    assert names == ["ff_geglu_kernel"], names
    msg = _mismatch(t, out, name)
    assert msg is None, msg


# ---- ff_chain_kernel<PRE, POST, REP> ------------------------------------------------------------------------------------------------

def _chan_stats_mismatch(st, stored, img_rows):
    """The statistics that ride on a stored [M, C] tensor whose values are NOT small (multiples of 1/2 up to a few hundred), against
    float64 on the stored values.  emit_chan_stats (gemm_kernel.h) sums v - k (k: the partial's first row) per lane and then over
    the lanes: S is exact (below 2^24 halves); Q takes one fp32 rounding per fma and per lane sum, at most 32 for 128 rows on 6
    lanes; mean = k + S / n is one rounding; m2 = Q - S * S / n two more at the size of S^2 / n and Q:
        |mean - ref| <= 2 u |ref|,    |M2 - ref| <= u (34 Q + 2 S^2 / n).
    stat_sums is formed in fp64 from the fp32 partials (gn_sums_add), so it must equal rint(n mean 2^32) and rint((n mean^2 + M2)
    2^16) of the partials the launch itself wrote, summed per image, exactly.  Returns None or a report."""
    v = stored.detach().double().cpu()
    M, C = v.shape
    R = img_rows // st.T
    blk = v.view(M // R, R, C)
    d = blk - blk[:, :1]
    S, Q = d.sum(1), (d * d).sum(1)
    mean = blk.mean(1)
    m2 = ((blk - mean[:, None]) ** 2).sum(1)
    got = st.buf.double().cpu()
    if tuple(got.shape) != (M // R, C, 2):
        return "partials of shape %s, expected %s" % (tuple(got.shape), (M // R, C, 2))
    bad = ((got[..., 0] - mean).abs() > 2 * E.U * mean.abs()) | ((got[..., 1] - m2).abs() > E.U * (34 * Q + 2 * S * S / R)) | ~torch.isfinite(got).all(-1)
    if bool(bad.any()):
        idx = bad.nonzero()
        pi, ch = idx[0].tolist()
        return "%d of %d (partial, channel) pairs fail, first (partial=%d, channel=%d): got (%.9g, %.9g), expected (%.9g, %.9g)" % (
            idx.shape[0], bad.numel(), pi, ch, got[pi, ch, 0], got[pi, ch, 1], mean[pi, ch], m2[pi, ch])
    if st.sums is not None:
        per = img_rows // R
        s1 = (R * got[..., 0] * 2.0 ** 32).round().to(torch.int64).view(M // img_rows, per, C).sum(1)
        s2 = ((R * got[..., 0] * got[..., 0] + got[..., 1]) * 2.0 ** 16).round().to(torch.int64).view(M // img_rows, per, C).sum(1)
        bad = (st.sums.view(M // img_rows, C, 2).cpu() != torch.stack([s1, s2], 2)).nonzero()
        if bad.shape[0]:
            return "stat_sums: %d entries differ from the partials, first (image, channel, which) %s" % (bad.shape[0], bad[:4].tolist())
    return None


@pytest.mark.parametrize("name", E.names("ff_chain"))
def test_feed_forward_chain(ops, dev, name, monkeypatch):
    """attn2.to_out + residual -> LayerNorm -> GEGLU feed-forward -> + residual -> proj_out in one launch, every instantiated (PRE,
    POST) pair, also with two replicas sharing the residual operands: the output is an exact multiple of alpha; with POST and whole
    128-row tiles the statistics ride along."""
    monkeypatch.setattr(ops, "GN_SUMS", True)
    monkeypatch.setattr(ops, "GN_FUSED_MAX", 0)
    t = E.build(name)
    c = t.case
    assert ops.ff_chain_supported(E.FF_C)
    put = lambda v: None if v is None else v.to(dev)
    kw = dict(repeat=c["repeat"])
    if c["pre"]:
        kw.update(a=put(t.a), wo=put(t.wo), bo=put(t.bo))
    if c["post"]:
        kw.update(wp=put(t.wp), bp=put(t.bp), res=put(t.res), alpha=c["alpha"])
    stats = c["post"] and c["M"] % 128 == 0
    if c["repeat"] > 1 or stats:
        kw.update(stat_img_rows=128, want_stats=stats)
    out, names = _profiled(ops, lambda: ops.ff_chain(put(t.x), put(t.w1), put(t.b1), put(t.w2), put(t.b2), E.LN_EPS, **kw))
    assert names == ["ff_chain_kernel<%d,%d>" % (c["pre"], c["post"])], names
    assert_exact(out, t.ref, RC, name)
    st = ops.stats_of(out)
    if stats:
        assert st is not None and st.T == 1 and st.sums is not None, "the launch should emit statistics and sums"
        msg = _chan_stats_mismatch(st, out, 128)
        assert msg is None, "%s: %s" % (name, msg)
    else:
        assert st is None


def test_feed_forward_chain_without_a_projection_is_refused(ops, dev):
    """(PRE, POST) = (0, 0) is ff_geglu_kernel's launch: the chain has no such instance and says so, with one replica or two."""
    from vd_hip import VdHipError
    t = E.build("ff_geglu_sat_m128")
    x, w1, b1, w2, b2 = [v.to(dev) for v in (t.x, t.w1, t.b1, t.w2, t.b2)]
    with pytest.raises(VdHipError, match="neither projection"):
        ops.ff_chain(x, w1, b1, w2, b2, E.LN_EPS)
    with pytest.raises(VdHipError, match="no operand is shared"):
        ops.ff_chain(x, w1, b1, w2, b2, E.LN_EPS, repeat=2, stat_img_rows=64)


# ---- rowchain320_kernel ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", E.names("rowchain"))
def test_row_resident_chain(ops, dev, name):
    """GroupNorm as a per-image fp16 map (plain and centred) -> proj_in -> h -> LayerNorm -> q | k | v: h in every element; with the
    permutation family (the rows of h are code rows) y2 as well."""
    t = E.build(name)
    c = t.case
    put = lambda v: None if v is None else v.to(dev)
    (h, y2), names = _profiled(ops, lambda: ops.row320_chain(put(t.x), put(t.sc), put(t.sh), c["rows_per_image"], put(t.w1), put(t.b1),
                                                             put(t.w2), put(t.b2), E.LN_EPS, center=put(t.ctr)))
    assert names == ["rowchain320_kernel"], names
    assert y2.shape == (c["M"], c["N2"])
    assert_exact(h, t.ref_h, RC, name + ", h")
    if t.ref_y2 is not None:
        assert_exact(y2, t.ref_y2, RC, name + ", y2")


# ---- the tests can fail ----------------------------------------------------------------------------------------------------------------

def test_mislocated_operands_are_reported(ops, dev, monkeypatch):
    """No kernel change: the launches get a wrong operand from the host side -- a colsum rolled by one column, a GEGLU bias (of the
    GEMM and of the fused feed-forward) that skipped pack_geglu, statistics rolled by one row -- and one reference applies alpha in
    front of the activation.  The acceptance
    rule reports each with the row and column of the first failing elements."""
    def located(msg, what):
        assert msg is not None, "%s went unnoticed" % what
        assert "row=" in msg and "col=" in msg, msg

    t = E.build("gemm_table_none")
    out, _ = _gemm(ops, dev, t, monkeypatch, colsum=torch.roll(t.colsum, 1, 0))
    located(_mismatch(t, out, "colsum rolled by one column"), "a colsum rolled by one column")
    t = E.build("gemm_off_geglu_sat")
    out, _ = _gemm(ops, dev, t, monkeypatch, bias=E.unpack_geglu_vector(t.bias).contiguous())
    located(_mismatch(t, out, "bias not packed"), "an unpacked GEGLU bias")
    t = E.build("ff_geglu_sat_m128")
    x, w1, w2, b2, res = [v.to(dev) for v in (t.x, t.w1, t.w2, t.b2, t.res)]
    out = ops.ff_geglu(x, w1, E.unpack_geglu_vector(t.b1).contiguous().to(dev), w2, b2, res, E.LN_EPS)
    located(_mismatch(t, out, "b1 not packed"), "an unpacked b1 of the fused feed-forward")
    t = E.build("gemm_sums_none")
    out, _ = _gemm(ops, dev, t, monkeypatch, ln_sums=torch.roll(t.ln_sums, 1, 0).contiguous())
    located(_mismatch(t, out, "statistics rolled by one row"), "statistics rolled by one row")
    t = E.build("gemm_off_quick_gelu")
    assert t.case["alpha"] == 0.5 and t.res is None
    out, _ = _gemm(ops, dev, t, monkeypatch)
    assert _mismatch(t, out, "gemm_off_quick_gelu") is None
    early = E.to_f16(E.act_f64("quick_gelu", t.y * 0.5))
    located(interval_mismatch(out, early, early, RC, "alpha in front of the activation"), "alpha applied in front of the activation")
