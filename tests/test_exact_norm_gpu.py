"""Every normalisation kernel, element by element: gn_slab_kernel<2|6|12>, gn_partial_kernel + gn_apply_kernel, gn0d_kernel,
gn_affine_kernel, layernorm_kernel, row_stats_kernel<3|5|10|16> (csrc/norm.hip) and chan_stats_kernel, gn_table_kernel,
gn_apply_table_kernel<false|true>, gn_from_stats_kernel (csrc/gn_fused.hip).

The operands of tests/norm_cases.py make every sum the kernels accumulate exact in fp32 in any order, so an fp16 output must be the
float64 result rounded to fp16 up to K 2^-24 of its scale (norm_cases.mismatch: one rule, one K, no case widened), the chan_stats
partials and the row_stats mean must be bit-exact, and the float-atomic path must be run-to-run identical.  A failure names the
failing (sample, row, channel), its group, its slab / row chunk with the position inside it and the failures per group.
tests/test_exact_norm_cpu.py proves the preconditions without a GPU.  Every test prints the largest share of the allowance it used."""
import numpy as np
import pytest
import torch

import norm_cases as N

pytestmark = pytest.mark.gpu

SENTINEL = 1234.0
SPARE_ROWS = 3


@pytest.fixture(scope="module")
def ops():
    from vd_hip import ops as o
    return o


def _dev(a, dev):
    return None if a is None else torch.from_numpy(a).to(dev)


def guarded(shape, dev):
    """(buffer, window): a contiguous [..., C] window for out= with SPARE_ROWS sentinel rows behind its last row (which is the
    last row of the last sample: the outputs of these kernels are contiguous, there is no gap between samples to guard)."""
    rows = int(np.prod(shape[:-1]))
    buf = torch.full((rows + SPARE_ROWS, shape[-1]), SENTINEL, dtype=torch.float16, device=dev)
    return buf, buf[:rows].view(*shape)


def check_guard(buf, name):
    spare = buf[-SPARE_ROWS:].cpu()
    stray = (spare != SENTINEL).nonzero()
    assert stray.shape[0] == 0, "%s: %d elements behind the output were written, first at (spare row, column) %s" % (name, stray.shape[0], stray[0].tolist())


def check(t, out, act, what, used):
    ref = N.silu(t.y) if act else t.y
    got = out.detach().cpu().numpy().reshape(ref.shape)
    msg = N.mismatch(got, ref, t.scale, t.case, act, what)
    assert msg is None, msg
    used.append(float(N.share(got, ref, t.scale, act).max()))


def report(name, used):
    print("%s: largest share of the allowance %.3f" % (name, max(used)))


# ---- csrc/norm.hip: the direct GroupNorm ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", N.names("direct"))
def test_groupnorm_direct(ops, dev, name):
    """ops.groupnorm_silu on tensors without statistics: gn_slab_kernel<nitem> or gn_partial_kernel + gn_apply_kernel, as the case
    table says.  The partial region of the workspace is pre-filled with 0xFF bytes: fully written by the two launches, untouched by
    the slab kernel.  out= is guarded; two runs are bit-identical (fixed point on the slab path; on the float-atomic path because
    the sums are exact in any order -- the property the acceptance rule rests on)."""
    from vd_hip.loader import lib
    t = N.build(name)
    c = t.case
    B, HW, C, G = c["B"], c["HW"], c["C"], c["groups"]
    nbytes = lib().vd_groupnorm_workspace_bytes(B, HW, C, G)
    assert nbytes == N.gn_workspace_bytes(B, HW, C, G)
    p = N.gn_slab(HW, C, G)
    assert (p["nitem"] if p else 0) == c["nitem"]
    x0, x1, gamma, beta = _dev(t.x0, dev), _dev(t.x1, dev), _dev(t.gamma, dev), _dev(t.beta, dev)
    used = []
    for act in (False, True):
        ws = ops.workspace(nbytes, dev, "gn")
        ws.fill_(0xFF)
        buf, win = guarded((B, HW, C), dev)
        ret = ops.groupnorm_silu(x0, gamma, beta, x1=x1, groups=G, eps=c["eps"], silu=act, out=win)
        assert ret.data_ptr() == win.data_ptr() and ops.workspace(nbytes, dev, "gn").data_ptr() == ws.data_ptr()
        part = ws[:N.gn_partial_floats(B, HW, C, G) * 4].cpu().view(torch.int32)
        if c["nitem"]:
            assert bool((part == -1).all()), "%s: the slab case wrote %d partial sums" % (name, int((part != -1).sum()))
        else:
            assert bool((part != -1).all()), "%s: %d of %d partial sums were not written, first %d" % (
                name, int((part == -1).sum()), part.numel(), int((part == -1).nonzero()[0]))
        check(t, win, act, "silu" if act else "plain", used)
        check_guard(buf, name)
        again = ops.groupnorm_silu(x0, gamma, beta, x1=x1, groups=G, eps=c["eps"], silu=act)
        assert torch.equal(again, win), "%s: two runs differ in %d elements" % (name, int((again != win).sum()))
    report(name, used)


@pytest.mark.parametrize("name", N.names("gn0d"))
def test_groupnorm0d(ops, dev, name):
    """gn0d_kernel: gamma / beta are [S, C] and distinct per s; fixed-point sums, so two runs are bit-identical."""
    t = N.build(name)
    c = t.case
    x0, x1, gamma, beta = _dev(t.x0, dev), _dev(t.x1, dev), _dev(t.gamma, dev), _dev(t.beta, dev)
    used = []
    for act in (False, True):
        out = ops.groupnorm0d_silu(x0, gamma, beta, x1=x1, groups=c["groups"], eps=c["eps"], silu=act)
        check(t, out, act, "silu" if act else "plain", used)
        assert torch.equal(out, ops.groupnorm0d_silu(x0, gamma, beta, x1=x1, groups=c["groups"], eps=c["eps"], silu=act))
    report(name, used)


def check16(t, got, ref, mag, what, used):
    got = got.cpu().numpy()
    msg = N.mismatch(got, ref, mag, t.case, False, what)
    assert msg is None, msg
    used.append(float(N.share(got, ref, mag).max()))


@pytest.mark.parametrize("name", N.names("affine"))
def test_groupnorm_affine(ops, dev, name):
    """ops.groupnorm_affine, both values of `centered`: gn_partial_kernel + gn_affine_kernel on a tensor without statistics (the
    centre is then None), and the fp16 outputs of gn_table_kernel (scale16, shift16, center16) with block statistics attached.
    The fp16 rule on each output's own magnitude; the centred shift is taken against the centre the kernel chose."""
    t = N.build(name)
    c = t.case
    cg = c["C"] // c["groups"]
    x, gamma, beta = _dev(t.x0, dev), _dev(t.gamma, dev), _dev(t.beta, dev)
    used = []
    for centered in (False, True):
        r = ops.groupnorm_affine(x, gamma, beta, groups=c["groups"], eps=c["eps"], centered=centered)
        assert len(r) == (3 if centered else 2) and (not centered or r[2] is None)
        check16(t, r[0], t.sc, np.abs(t.sc), "scale", used)
        check16(t, r[1], t.sh, t.base, "shift", used)
    if c["R0"] and ops.GN_STATS:
        p, T = N.partials(t, 0)
        x._vd_stats = ops.ChanStats(_dev(p, dev), T, c["C"], c["HW"])
        sc, sh = ops.groupnorm_affine(x, gamma, beta, groups=c["groups"], eps=c["eps"])
        check16(t, sc, t.sc, np.abs(t.sc), "scale16", used)
        check16(t, sh, t.sh, t.base, "shift16", used)
        sc, sh, ct = ops.groupnorm_affine(x, gamma, beta, groups=c["groups"], eps=c["eps"], centered=True)
        check16(t, sc, t.sc, np.abs(t.sc), "scale16 (centred)", used)
        meanc = np.repeat(t.mean, cg, 1)
        if ops.ST_CENTER:
            check16(t, ct, meanc, np.abs(meanc), "center16", used)
            ctr = ct.cpu().numpy().astype(np.float64)
            dm = meanc - ctr
            check16(t, sh, t.beta.astype(np.float64) - dm * t.sc, np.abs(t.beta.astype(np.float64)) + (np.abs(dm) + N.U * np.abs(ctr)) * np.abs(t.sc),
                    "shift16 (centred)", used)
    report(name, used)


# ---- csrc/norm.hip: rows -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", N.names("ln"))
def test_layernorm(ops, dev, name):
    t = N.build(name)
    c = t.case
    buf, win = guarded((c["rows"], c["C"]), dev)
    ret = ops.layernorm(_dev(t.x, dev), _dev(t.gamma, dev), _dev(t.beta, dev), eps=c["eps"], out=win)
    assert ret.data_ptr() == win.data_ptr()
    used = []
    check(t, win, False, "layernorm", used)
    check_guard(buf, name)
    report(name, used)


@pytest.mark.parametrize("name", N.names("rows"))
def test_row_stats(ops, dev, name):
    """row_stats_kernel<nch>: the mean bit-exact (a pad column or a dropped chunk moves it), rstd within 4 * 2^-24 relative."""
    t = N.build(name)
    c = t.case
    st = ops.row_stats(_dev(t.x, dev), c["C"], c["rows"], c["eps"], ldx=c["C"] + c["pad"]).cpu().numpy()
    assert st.shape == (c["rows"], 2) and st.dtype == np.float32
    msg = N.mismatch_f32(st[:, 0], t.mean, 0.0, c, "mean") or N.mismatch_f32(st[:, 1], t.rstd, N.RSTD_ROWS_REL * t.rstd, c, "rstd")
    assert msg is None, msg
    print("%s: rstd uses %.3f of its bound" % (name, (np.abs(st[:, 1] - t.rstd) / (N.RSTD_ROWS_REL * t.rstd)).max()))


# ---- csrc/gn_fused.hip ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", N.names("chan"))
def test_chan_stats(ops, dev, name):
    """chan_stats_kernel: (mean, M2) per channel and block of R rows, bit-exact."""
    t = N.build(name)
    c = t.case
    st = ops.chan_stats(_dev(t.x0, dev), c["R0"])
    assert (st.T, st.C, st.HW) == (c["HW"] // c["R0"], c["C"], c["HW"])
    mean, m2 = N.block_partials(t.x, c["R0"])
    got = st.buf.cpu().numpy()
    msg = N.mismatch_f32(got[..., 0], mean, 0.0, c, "mean [block, channel]") or N.mismatch_f32(got[..., 1], m2, 0.0, c, "M2 [block, channel]")
    assert msg is None, msg


@pytest.mark.parametrize("name", N.names("stats"))
def test_groupnorm_from_partials(ops, dev, name):
    """gn_table_kernel (fp32 table within K 2^-24 of its magnitudes), gn_apply_table_kernel<false>, gn_from_stats_kernel and
    gn_apply_table_kernel<true> on partials and fixed-point sums computed here from the inputs, not by a kernel; out= guarded, two
    runs bit-identical (no atomics), and the dispatch inside ops.groupnorm_silu equals bitwise the form it documents."""
    t = N.build(name)
    c = t.case
    B, HW, C, G = c["B"], c["HW"], c["C"], c["groups"]
    x0, x1, gamma, beta = _dev(t.x0, dev), _dev(t.x1, dev), _dev(t.gamma, dev), _dev(t.beta, dev)
    p0, T0 = N.partials(t, 0)
    st0 = ops.ChanStats(_dev(p0, dev), T0, c["c0"], HW)
    st1 = sums1 = None
    if c["c1"]:
        p1, T1 = N.partials(t, 1)
        st1 = ops.ChanStats(_dev(p1, dev), T1, c["c1"], HW)
        sums1 = _dev(N.fixed_point_sums(t, 1), dev)
    sums0 = _dev(N.fixed_point_sums(t, 0), dev)
    table = ops.gn_table(st0, gamma, beta, st1=st1, B=B, groups=G, eps=c["eps"])
    tb = table.cpu().numpy()
    msg = N.mismatch_f32(tb[:, 0], t.sc, N.K * N.U * np.abs(t.sc), c, "table scale [sample, channel]") or \
        N.mismatch_f32(tb[:, 1], t.sh, N.K * N.U * t.base, c, "table shift [sample, channel]")
    assert msg is None, msg
    assert torch.equal(table, ops.gn_table(st0, gamma, beta, st1=st1, B=B, groups=G, eps=c["eps"]))
    used = [float(np.max(np.abs(tb[:, 0] - t.sc) / (N.K * N.U * np.abs(t.sc)))), float(np.max(np.abs(tb[:, 1] - t.sh) / (N.K * N.U * t.base)))]
    forms = {
        "apply_table": lambda act, out: ops.gn_apply_table(x0, table, x1=x1, silu=act, out=out),
        "from_stats": lambda act, out: ops.groupnorm_from_stats(x0, gamma, beta, st0, x1=x1, st1=st1, groups=G, eps=c["eps"], silu=act, out=out),
        "apply_sums": lambda act, out: ops.gn_apply_sums(x0, sums0, gamma, beta, x1=x1, sums1=sums1, groups=G, eps=c["eps"], silu=act, out=out),
    }
    outs = {}
    for form, fn in forms.items():
        for act in (False, True):
            buf, win = guarded((B, HW, C), dev)
            ret = fn(act, win)
            assert ret.data_ptr() == win.data_ptr()
            check(t, win, act, form + (" silu" if act else ""), used)
            check_guard(buf, name + " " + form)
            assert torch.equal(fn(act, None), win), "%s %s: two runs differ" % (name, form)
            outs[form, act] = win
    # the dispatch: statistics riding on both sources, no sums -> the fused form for small tensors, else table + apply
    if ops.GN_STATS:
        assert ops._from_stats_ok(C, G)
        x0._vd_stats = st0
        if x1 is not None:
            x1._vd_stats = st1
        small = B * HW * C <= ops.GN_FUSED_MAX or ops.GN_FORM == "fused"
        for act in (False, True):
            got = ops.groupnorm_silu(x0, gamma, beta, x1=x1, groups=G, eps=c["eps"], silu=act)
            assert torch.equal(got, outs["from_stats" if small else "apply_table", act]), "%s: the dispatch is not its %s form" % (name, "fused" if small else "table")
    report(name, used)
