"""vd_gemm_wstream_epi_f16 on the GPU: the weight-streaming GEMM with the fused epilogue against gemm_f16_kernel (ops.gemm without the
fragment-order pack) on the same operands and the same statistics buffers -- integer operands bit for bit, normal operands by
rel-L2 set against the old path's own distance from float64 -- with sentinels around the output, and a width-640
SpatialTransformer with the switch on against off.  Operands: tests/wstream_epi_cases.py."""
import pytest
import torch

import wstream_epi_cases as C
from vdtest_util import rel_l2

pytestmark = pytest.mark.gpu

SENTINEL = 777.0


@pytest.fixture(scope="module")
def ops():
    from vd_hip import ops as o
    return o


def _profiled(ops, fn):
    ops.profile_begin()
    try:
        out = fn()
    finally:
        names = [r[0] for r in ops.profile_end()]
    return out, names


def _run(ops, dev, a, w, b, fold, act, alpha, stream):
    """One launch into a buffer with 128 sentinel rows behind row M and 64 sentinel columns behind the output row; returns
    (the [M, n_out] result, the whole buffer, kernel names).  stream: the fragment-order pack (new path) or None (today's)."""
    M, K = a.shape
    N = w.shape[0]
    n_out = N // 2 if act == "geglu" else N
    buf = torch.full((M + 128, n_out + 64), SENTINEL, dtype=torch.float16, device=dev)
    kw = dict(bias=b, act=ops.ACT_GEGLU if act == "geglu" else ops.ACT_NONE, alpha=alpha, out=buf, ldc=n_out + 64)
    if fold != "bias":
        kw.update(colsum=C.colsum_of(w), ln_eps=C.LN_EPS)
    if fold == "sums":
        kw.update(ln_sums=C.row_sums_fixed(a).to(dev))
    if stream is not None:
        kw.update(w_stream_epi=stream)
    _, names = _profiled(ops, lambda: ops.gemm(a, w, **kw))
    return buf[:M, :n_out], buf, [n for n in names if n != "row_stats_kernel"]


def _pair(ops, dev, a, w, b, fold, act, alpha=1.0):
    from vd_hip.pack import pack_linear_weight_stream
    a, w, b = a.to(dev), w.to(dev), b.to(dev)
    new, nbuf, n_new = _run(ops, dev, a, w, b, fold, act, alpha, pack_linear_weight_stream(w))
    old, _, n_old = _run(ops, dev, a, w, b, fold, act, alpha, None)
    assert n_new == ["gemm_wstream_epi_kernel" + (" geglu" if act == "geglu" else "")], n_new
    assert len(n_old) == 1 and n_old[0].startswith("gemm_f16_kernel"), n_old
    M, n_out = new.shape
    assert bool((nbuf[M:] == SENTINEL).all()), "rows behind M were written"
    assert bool((nbuf[:M, n_out:] == SENTINEL).all()), "columns behind the output row were written"
    return new, old


def _assert_equal(new, old, what):
    bad = (new != old).nonzero()
    assert bad.numel() == 0, "%s: %d elements differ, first (row, column) %s: new %s, old %s" % (
        what, bad.shape[0], bad[0].tolist(), new[tuple(bad[0])].item(), old[tuple(bad[0])].item())


# what fp16 rounding of an exact value leaves in rel-L2 at most: half an ulp, 2^-11, in every element; the erf of the epilogue
# (vd_erf, absolute error ~1e-7) adds nothing visible to it
FP16_HALF_ULP = 2.0 ** -11


@pytest.mark.parametrize("M,N,K,fold,act", C.grid())
def test_integer_operands_bit_for_bit(ops, dev, M, N, K, fold, act):
    """Exact fp32 sums: the accumulators of both kernels are the same integers, so the outputs differ only if the epilogues do.
    Fold off and plain: also the float64 integer value itself; fold off with GEGLU: within fp16 rounding of the float64 value."""
    a, w, b = C.integer_case(M, N, K, seed=M + N + K)
    new, old = _pair(ops, dev, a, w, b, fold, act)
    _assert_equal(new, old, "new vs gemm_f16_kernel")
    if fold == "bias":
        ref = C.reference(a, w, b, fold, act)
        if act == "none":
            _assert_equal(new.double().cpu(), ref, "new vs the integer reference")
        else:
            e = rel_l2(new, ref)
            print("GEGLU on integer sums: rel-L2 from float64 %.3g" % e)
            assert e <= FP16_HALF_ULP, e


def test_alpha_not_one(ops, dev):
    """alpha = 0.5 on integer sums below 1024: halves are exact in fp16, so the plain result is the float64 value; the folded GEGLU
    result is today's bit for bit."""
    a, w, b = C.integer_case(256, 384, 192, seed=5)
    new, old = _pair(ops, dev, a, w, b, "bias", "none", alpha=0.5)
    _assert_equal(new, old, "new vs gemm_f16_kernel")
    _assert_equal(new.double().cpu(), C.reference(a, w, b, "bias", "none", 0.5), "new vs the integer reference")
    new, old = _pair(ops, dev, a, w, b, "table", "geglu", alpha=0.5)
    _assert_equal(new, old, "new vs gemm_f16_kernel (fold, GEGLU)")


# Both kernels add the same 16-deep products in ascending K in fp32 and share the epilogue sequence, so new against old is zero or
# isolated last-place roundings, while a dropped fold term or a double rounding shows at the size of the old path's own distance from
# float64.  FRACTION: the largest ratio the first run on MI355X gave, 0.0722, doubled (profiles/HISTORY.md R8): 17 of the 18 cases
# were bit-identical; at (256, 256, 2048) without the fold today's path splits K, so its sums are ordered differently.
FRACTION = 0.15


@pytest.mark.parametrize("fold,act", C.EPILOGUES)
@pytest.mark.parametrize("M,N,K", [(256, 384, 192), (128, 512, 1280), (256, 256, 2048)])
def test_normal_operands_against_float64(ops, dev, M, N, K, fold, act):
    a, w, b = C.normal_case(M, N, K, seed=K + N)
    new, old = _pair(ops, dev, a, w, b, fold, act, alpha=0.7)
    ref = C.reference(a, w, b, fold, act, 0.7)
    e_old, e_new, d = rel_l2(old, ref), rel_l2(new, ref), rel_l2(new, old)
    print("M=%d N=%d K=%d %s/%s: rel-L2 new vs old %.3g, old vs float64 %.3g, new vs float64 %.3g, ratio %.3g" % (
        M, N, K, fold, act, d, e_old, e_new, d / e_old))
    assert e_old < 2e-3, e_old          # the reference describes the launch at all (fp16 output: ~3e-4)
    assert d <= FRACTION * e_old, (d, e_old)


@pytest.fixture(scope="module")
def st640(dev):
    """A SpatialTransformer of width 640 (8 heads of 80) on 16x16 tokens, B = 2, proj_out randomised (it is zero-initialised)."""
    from lib.model_zoo.attention import SpatialTransformer
    torch.manual_seed(81)
    m = SpatialTransformer(640, 8, 80, context_dim=64)
    with torch.no_grad():
        m.proj_out.weight.normal_(0.0, 640 ** -0.5)
        m.proj_out.bias.normal_(0.0, 0.1)
    m = m.half().to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(82)
    x = torch.randn((2, 16, 16, 640), generator=g).half().to(dev)
    ctx = torch.randn((2, 8, 64), generator=g).half().to(dev)
    return m, x, ctx


def test_spatial_transformer_640_switch_on_off(ops, dev, st640, monkeypatch):
    m, x, ctx = st640
    run = lambda: m(x, ctx)
    monkeypatch.setattr(ops, "GEMM_WSTREAM_EPI", True)
    on, n_on = _profiled(ops, run)
    monkeypatch.setattr(ops, "GEMM_WSTREAM_EPI", False)
    off, n_off = _profiled(ops, run)
    off2 = run()
    monkeypatch.setattr(ops, "GEMM_WSTREAM_EPI", True)
    on2 = run()
    epi = [n for n in n_on if n.startswith("gemm_wstream_epi_kernel")]
    assert sorted(epi) == ["gemm_wstream_epi_kernel", "gemm_wstream_epi_kernel geglu"], n_on      # q | k | v and GEGLU of the block
    assert not [n for n in n_off if n.startswith("gemm_wstream_epi_kernel")] and len(n_on) == len(n_off), (n_on, n_off)
    e = rel_l2(on, off)
    print("SpatialTransformer 640, 16x16, B = 2: rel-L2 switch on vs off %.3g" % e)
    assert e <= 1e-3, e
    assert torch.equal(on2, on) and torch.equal(off2, off)      # each setting bit-identical run to run
