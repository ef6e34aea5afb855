"""The feed-forward / proj_out fold on the GPU: vd_gemm_wstream_cat_f16 against vd_gemm_wstream_f16 on the materialised
concatenation (bit for bit), its long instance (34 chunks per block) against float64 with exact-sum operands, the merged block tail
against the two launches on both kernels (integer operands: bit for bit; normal operands: rel-L2 from float64), and a width-640
SpatialTransformer with two context types, switch on against switch off.  Operands: tests/ff_proj_fold_cases.py."""
import ctypes

import pytest
import torch

import ff_proj_fold_cases as F
from vdtest_util import rel_l2

pytestmark = pytest.mark.gpu


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


def _plain_entry(ops, a, w, ws, bias=None, res=None, alpha=1.0, stats=False, split_k=0):
    """vd_gemm_wstream_f16 called directly (ops.gemm never asks this entry for out_stats): (out, stats buffer or None, split)."""
    from vd_hip.loader import VdGemmDesc, lib
    M, K = a.shape
    N = w.shape[0]
    d = VdGemmDesc()
    d.M, d.N, d.K, d.c0 = M, N, K, K
    out = torch.empty((M, N), dtype=torch.float16, device=a.device)
    d.a0, d.w, d.out = a.data_ptr(), w.data_ptr(), out.data_ptr()
    d.alpha, d.batch, d.split_k = float(alpha), 1, int(split_k)
    flags = 0
    if bias is not None:
        flags |= ops.EPI_BIAS
        d.bias = bias.data_ptr()
    if res is not None:
        flags |= ops.EPI_RESIDUAL
        d.res = res.data_ptr()
    d.flags = flags
    ns = ctypes.c_int(0)
    assert lib().vd_gemm_wstream_plan(ctypes.byref(d), ctypes.byref(ns)) == 0
    d.split_k = max(ns.value, 1)
    d.ws = ops.workspace(lib().vd_gemm_workspace_bytes(ctypes.byref(d)), a.device, "gemm").data_ptr()
    sbuf = None
    if stats:
        sbuf = torch.empty((M // 64, N, 2), dtype=torch.float32, device=a.device)
        d.out_stats = sbuf.data_ptr()
    ops._check(lib().vd_gemm_wstream_f16(ctypes.byref(d), ops._ptr(ws), ops._stream()))
    return out, sbuf, d.split_k


def _cat_plan(ops, M, N, c0, c1, split_k=0):
    from vd_hip.loader import VdGemmDesc, lib
    d = VdGemmDesc()
    d.M, d.N, d.K, d.c0, d.c1, d.split_k = M, N, c0 + c1, c0, c1, split_k
    d.a0 = d.a1 = d.w = d.out = d.ws = 16
    ns = ctypes.c_int(0)
    assert lib().vd_gemm_wstream_cat_supported(ctypes.byref(d)) == 1
    assert lib().vd_gemm_wstream_cat_plan(ctypes.byref(d), ctypes.byref(ns)) == 0
    return ns.value


@pytest.mark.parametrize("epi", ["bare", "full"])
@pytest.mark.parametrize("M,N,c0,c1", [(128, 256, 1024, 256), (256, 512, 256, 64)])
def test_cat_entry_is_bitwise_the_plain_entry_on_the_concatenation(ops, dev, M, N, c0, c1, epi):
    """Same chunk order, same slabs, same reduce: reading chunk c from a0 or a1 instead of from cat(a0, a1) changes no bit --
    with a bare epilogue and with bias, residual, alpha != 1 and out_stats."""
    from vd_hip.pack import pack_linear_weight_stream
    g = torch.Generator(device="cpu").manual_seed(M + c1)
    a0, a1 = torch.randn((M, c0), generator=g).half().to(dev), torch.randn((M, c1), generator=g).half().to(dev)
    w = (torch.randn((N, c0 + c1), generator=g) / (c0 + c1) ** 0.5).half().to(dev)
    ws = pack_linear_weight_stream(w)
    full = epi == "full"
    bias = torch.randn((N,), generator=g).half().to(dev) if full else None
    res = torch.randn((M, N), generator=g).half().to(dev) if full else None
    alpha = 0.7 if full else 1.0
    old, sbuf, split = _plain_entry(ops, torch.cat([a0, a1], 1).contiguous(), w, ws, bias, res, alpha, stats=full)
    assert _cat_plan(ops, M, N, c0, c1) == split          # both entries take the same split
    new, names = _profiled(ops, lambda: ops.gemm(a0, w, a1=a1, bias=bias, res=res, alpha=alpha, want_stats=full, w_stream_cat=ws))
    assert names == ["gemm_wstream_cat_kernel + reduce"], names
    assert torch.equal(new, old)
    st = ops.stats_of(new)
    if full:
        assert st is not None and st.buf.shape == (M // 64, N, 2) and torch.equal(st.buf, sbuf)
        # ... and they are mean and M2 of 64 stored rows each
        o = new.double().view(M // 64, 64, N)
        mean = o.mean(1)
        m2 = ((o - mean[:, None]) ** 2).sum(1)
        dm = (st.buf[..., 0].double() - mean).abs().max().item()
        d2 = (st.buf[..., 1].double() - m2).abs().max().item() / m2.abs().max().item()
        print("stats: |d mean| %.3g, |d M2| / scale %.3g" % (dm, d2))
        assert dm < 2e-4 and d2 < 1e-3, (dm, d2)      # the tolerance of test_kernels_gpu.py::test_gemm_out_stats
    else:
        assert st is None
    # one source through the same entry: the plain entry on a0 alone
    old1, _, split1 = _plain_entry(ops, a0, w[:, :c0].contiguous(), pack_linear_weight_stream(w[:, :c0].contiguous()))
    new1 = ops.gemm(a0, w[:, :c0].contiguous(), w_stream_cat=pack_linear_weight_stream(w[:, :c0].contiguous()))
    assert torch.equal(new1, old1)


def test_long_instance_34_chunks_per_block_exact(ops, dev):
    """K = 6400 as three splits: 34, 34 and 32 chunks per block, the sequence whose last chunk has no weight loads behind its
    tile.  Integer operands: every fp32 sum is exact in any order, so each element must be the float64 value."""
    from vd_hip.pack import pack_linear_weight_stream
    M, N, c0, c1 = 128, 256, 5120, 1280
    a0, a1, w, ref = F.integer_gemm(M, N, c0, c1, seed=11)
    a0, a1, w = a0.to(dev), a1.to(dev), w.to(dev)
    assert _cat_plan(ops, M, N, c0, c1, split_k=3) == 3
    out, names = _profiled(ops, lambda: ops.gemm(a0, w, a1=a1, split_k=3, w_stream_cat=pack_linear_weight_stream(w)))
    assert names == ["gemm_wstream_cat_kernel + reduce"], names
    bad = (out.double().cpu() != ref).nonzero()
    assert bad.numel() == 0, "%d elements differ, first (row, column) %s: got %s, expected %s" % (
        bad.shape[0], bad[0].tolist(), out[tuple(bad[0])].item(), ref[tuple(bad[0])].item())
    # the default split of the same problem (one tile: 32 splits of 4 chunks) and the 32-chunk sequence (4 splits of 25)
    for split in (0, 4):
        assert torch.equal(ops.gemm(a0, w, a1=a1, split_k=split, w_stream_cat=pack_linear_weight_stream(w)), out)


def _two_step(ops, t, dev, stream):
    from vd_hip.pack import pack_linear_weight_stream
    h, x2, w2, b2, wp, bp, r = [v.to(dev) for v in t[:7]]
    kw = dict(w_stream=pack_linear_weight_stream(w2)) if stream else {}
    y = ops.gemm(h, w2, bias=b2, res=x2, **kw)
    return ops.gemm(y, wp, bias=bp, alpha=t.alpha, res=r, want_stats=True)


def _merged(ops, t, dev, stream):
    from vd_hip.pack import pack_ff_proj_fold, pack_linear_weight_stream
    h, x2, w2, b2, wp, bp, r = [v.to(dev) for v in t[:7]]
    w_cat, bm = pack_ff_proj_fold(w2, b2, wp, bp)
    kw = dict(w_stream_cat=pack_linear_weight_stream(w_cat)) if stream else {}
    return ops.gemm(h, w_cat, a1=x2, bias=bm.half(), alpha=t.alpha, res=r, want_stats=True, **kw)


KERNELS = [("gemm_f16", False), ("wstream", True)]


@pytest.mark.parametrize("kernel,stream", KERNELS)
def test_merged_equals_two_launches_bit_for_bit_with_integer_operands(ops, dev, kernel, stream):
    t = F.integer_tail(128, 256, seed=21)
    (new, n_new) = _profiled(ops, lambda: _merged(ops, t, dev, stream))
    (old, n_old) = _profiled(ops, lambda: _two_step(ops, t, dev, stream))
    assert len(n_new) == 1 and len(n_old) == 2, (n_new, n_old)
    assert (n_new[0] == "gemm_wstream_cat_kernel + reduce") == stream, n_new
    assert torch.equal(new, old)
    assert torch.equal(new.cpu(), t.ref.half())
    assert ops.stats_of(new) is not None


@pytest.mark.parametrize("kernel,stream", KERNELS)
def test_merged_rel_l2_within_twice_the_two_launches(ops, dev, kernel, stream):
    """Fan-in-scaled normal weights, M = 128, C = 256.  The merged form rounds Wp W2 to fp16 once more and y to fp16 once less; the
    bound is twice the two-launch form's own distance from float64 on the same operands (the factor of the phase-convolution test).
    Measured on MI355X (merged, two launches): gemm_f16 2.90e-4, 3.29e-4; wstream 2.31e-4, 3.05e-4 (profiles/HISTORY.md R7)."""
    t = F.normal_tail(128, 256, seed=31)
    new, old = _merged(ops, t, dev, stream), _two_step(ops, t, dev, stream)
    e_new, e_old = rel_l2(new, t.ref), rel_l2(old, t.ref)
    print("%s: rel-L2 from float64: merged %.3g, two launches %.3g, ratio %.2f" % (kernel, e_new, e_old, e_new / e_old))
    assert e_new <= 2.0 * e_old, (e_new, e_old)


@pytest.fixture(scope="module")
def st640(dev):
    """Two SpatialTransformers of width 640 (8 heads of 80) for two context types, proj_out randomised (it is zero-initialised)."""
    from lib.model_zoo.attention import SpatialTransformer
    torch.manual_seed(41)
    mods = []
    for cd in (64, 128):
        m = SpatialTransformer(640, 8, 80, context_dim=cd)
        with torch.no_grad():
            m.proj_out.weight.normal_(0.0, 640 ** -0.5)
            m.proj_out.bias.normal_(0.0, 0.1)
        mods.append(m.half().to(dev).eval())
    g = torch.Generator(device="cpu").manual_seed(42)
    x = torch.randn((2, 8, 8, 640), generator=g).half().to(dev)
    ctx = [torch.randn((2, 8, cd), generator=g).half().to(dev) for cd in (64, 128)]
    return mods, x, ctx


def _mix(ops, st640, log=None):
    """sum_i r_i ST_i(x) the way vd.run_unet chains it: the second type's last launch adds onto the first type's output."""
    mods, x, ctx = st640
    out = mods[0](x, ctx[0], alpha=0.3, res=None)
    sync = None if log is None else (lambda: log.append(ops.LIB_CALLS[0]))
    return mods[1](x, ctx[1], alpha=0.7, res=out, sync=sync)


def test_spatial_transformer_640_fold_on_off_eager_captured(ops, dev, st640, monkeypatch):
    from lib.model_zoo import hip_layers
    log = []
    on, n_on = _profiled(ops, lambda: _mix(ops, st640, log))
    end = ops.LIB_CALLS[0]
    assert len(log) == 1 and end - log[0] == 1      # sync ran once, right in front of the last launch (the one that reads res)
    assert ops.stats_of(on) is not None and on.shape == (2, 8, 8, 640)
    monkeypatch.setattr(hip_layers, "FF_PROJ_FOLD", False)
    off, n_off = _profiled(ops, lambda: _mix(ops, st640))
    monkeypatch.setattr(hip_layers, "FF_PROJ_FOLD", True)
    assert len(n_on) == len(n_off) - 2, (n_on, n_off)      # one projection fewer per transformer
    e = rel_l2(on, off)
    print("SpatialTransformer 640, two context types: rel-L2 fold on vs off %.3g" % e)
    assert e < 1e-3
    assert torch.equal(_mix(ops, st640), on)               # eager, repeated
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _mix(ops, st640)                                   # (workspaces of the capture stream exist before the capture)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph, stream=side):
        cap = _mix(ops, st640)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, on)
    ops.drop_workspaces(side.cuda_stream)
