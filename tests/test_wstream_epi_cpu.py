"""vd_gemm_wstream_epi_supported (host code, no launch), the packing the entry reads, and the host rules that hand the pack over."""
import ctypes

import pytest
import torch

import wstream_epi_cases as C

EPI_BIAS, EPI_RESIDUAL, EPI_LNFOLD, EPI_LN_INLOOP, EPI_LN_SUMS, EPI_OUT_F32 = 1, 4, 32, 64, 512, 16
ACT_GEGLU, ACT_SILU = 1, 3


def _desc(M=256, N=512, K=1280, flags=EPI_BIAS, act=0, **kw):
    from vd_hip.loader import VdGemmDesc
    d = VdGemmDesc()
    d.M, d.N, d.K = M, N, K
    d.a0 = d.w = d.out = d.bias = 16
    d.flags, d.act, d.alpha, d.batch = flags, act, 1.0, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _ok(d):
    from vd_hip.loader import lib
    return lib().vd_gemm_wstream_epi_supported(ctypes.byref(d))


def test_supported_takes_the_folded_projections():
    for M, N, K in [(8192, 1920, 640), (2048, 3840, 1280), (512, 3840, 1280), (128, 64, 64), (384, 384, 2048)]:
        assert _ok(_desc(M, N, K)) == 1
        assert _ok(_desc(M, N, K, flags=EPI_BIAS | EPI_LNFOLD, colsum=16, ln_stats=16)) == 1
        assert _ok(_desc(M, N, K, flags=EPI_BIAS | EPI_LNFOLD | EPI_LN_SUMS, colsum=16, ln_stats=16)) == 1
    for M, N, K in [(8192, 5120, 640), (2048, 10240, 1280), (512, 10240, 1280), (128, 128, 64)]:
        assert _ok(_desc(M, N, K, act=ACT_GEGLU, flags=EPI_BIAS | EPI_LNFOLD, colsum=16, ln_stats=16)) == 1
    assert _ok(_desc(batch=0)) == 1                                     # 0 = 1, as everywhere


@pytest.mark.parametrize("why,kw", [
    ("33 chunks", dict(K=2112)),
    ("M = 64", dict(M=64)),
    ("M not a multiple of 128", dict(M=192)),
    ("N not a multiple of 64", dict(N=288)),
    ("K not a multiple of 64", dict(K=96)),
    ("GEGLU with N % 128 != 0", dict(N=192, act=ACT_GEGLU)),
    ("another activation", dict(act=ACT_SILU)),
    ("a residual", dict(flags=EPI_BIAS | EPI_RESIDUAL, res=16)),
    ("fp32 output", dict(flags=EPI_OUT_F32)),
    ("in-loop statistics", dict(flags=EPI_LNFOLD | EPI_LN_INLOOP, colsum=16)),
    ("out_stats", dict(out_stats=16)),
    ("row_sums", dict(row_sums=16)),
    ("batch 2", dict(batch=2)),
    ("a K split", dict(split_k=2)),
    ("a second source", dict(a1=16, c0=640, c1=640)),
    ("a 3x3 conv descriptor", dict(K=5760, Hin=16, Win=16, Hout=16, Wout=16, ksize=3, stride=1, pad=1, c0=640)),
    ("a 1x1 conv descriptor", dict(Hin=16, Win=16, Hout=16, Wout=16, ksize=1, stride=1)),
])
def test_supported_refuses(why, kw):
    assert _ok(_desc(**kw)) == 0, why


def test_supported_null_and_entry_refuses_without_launching():
    from vd_hip.loader import lib
    assert lib().vd_gemm_wstream_epi_supported(None) == 0
    d = _desc(K=2112)
    assert lib().vd_gemm_wstream_epi_f16(ctypes.byref(d), ctypes.c_void_p(16), None) != 0
    assert b"vd_gemm_wstream_epi_f16" in lib().vd_last_error()


def test_fragment_order_of_the_geglu_pack_round_trip():
    """pack_linear_weight_stream(pack_geglu(w)) back to w: lane l of (tile t, chunk c, k-step s) holds packed row 32 t + (l & 31),
    columns 64 c + 16 s + 8 (l >> 5) .. + 8; packed rows 64 u .. + 32 are value rows 32 u .., the next 32 the gate rows."""
    from vd_hip.pack import pack_geglu, pack_linear_weight_stream
    inner, K = 128, 192
    g = torch.Generator().manual_seed(3)
    w = torch.randn((2 * inner, K), generator=g).half()
    b = torch.randn((2 * inner,), generator=g).half()
    wp, bp = pack_geglu(w, b)
    ws = pack_linear_weight_stream(wp)
    assert ws.shape == (2 * inner // 32, K // 64, 4, 64, 8) and ws.is_contiguous()
    back = ws.reshape(2 * inner // 32, K // 64, 4, 2, 32, 8).permute(0, 4, 1, 2, 3, 5).reshape(2 * inner, K)   # (t, l31, c, s, hi, e)
    assert torch.equal(back, wp)
    un = back.reshape(inner // 32, 2, 32, K)
    assert torch.equal(torch.cat([un[:, 0].reshape(inner, K), un[:, 1].reshape(inner, K)], 0), w)
    ub = bp.reshape(inner // 32, 2, 32)
    assert torch.equal(torch.cat([ub[:, 0].reshape(-1), ub[:, 1].reshape(-1)], 0), b)
    # one element spelled out: tile 5 is the gate half of group 2 -> gate row 2 * 32 + 7, i.e. row inner + 71 of w
    t, c, s, lane, e = 5, 2, 3, 32 + 7, 4
    assert ws[t, c, s, lane, e] == w[inner + 2 * 32 + 7, 64 * c + 16 * s + 8 + e]


def test_case_grid_covers_every_size_with_every_epilogue_kind():
    grid = C.grid()
    assert len(grid) == len(C.KS) * len(C.EPILOGUES) and len(set(grid)) == len(grid)
    assert {(K, f, a) for _, _, K, f, a in grid} == {(K, f, a) for K in C.KS for f, a in C.EPILOGUES}
    for vals, idx in ((C.MS, 0), (C.NS, 1)):
        for v in vals:
            assert {g[2] for g in grid if g[idx] == v} == set(C.KS), (idx, v)      # every M and every N meets every K
            assert {g[3] for g in grid if g[idx] == v} == {"bias", "table", "sums"}, (idx, v)
            assert {g[4] for g in grid if g[idx] == v} == {"none", "geglu"}, (idx, v)


def test_reference_of_the_fold_is_layernorm_then_linear():
    """The float64 reference the GPU tests use, against LayerNorm -> Linear -> GEGLU spelled out with torch (gamma = 1, beta = 0)."""
    a, w, b = C.normal_case(128, 256, 192, seed=1)
    ln = torch.nn.functional.layer_norm(a.double(), (192,), eps=C.LN_EPS)
    y = ln @ w.double().t() + b.double()
    for fold in ("table", "sums"):
        assert torch.allclose(C.reference(a, w, b, fold, "none"), y, rtol=0, atol=1e-6 if fold == "table" else 1e-4)
    y = y.view(128, 4, 2, 32)
    gl = (y[:, :, 0] * torch.nn.functional.gelu(y[:, :, 1])).reshape(128, 128)
    assert torch.allclose(C.reference(a, w, b, "table", "geglu", 0.5), 0.5 * gl, rtol=0, atol=1e-6)


def test_pack_handover_levels_and_cache(monkeypatch):
    """The modules hand the fragment-order pack over by (kind, rows, width); the pack is cached on the parameters of the folded
    weight (one build, a hit afterwards, a rebuild after an in-place edit)."""
    from lib.model_zoo import hip_layers
    from lib.model_zoo.attention import GEGLU, CrossAttention
    from lib.model_zoo.hip_layers import LayerNorm, PackCache
    from vd_hip import ops
    for (kind, width), (lo, hi) in hip_layers.WSTREAM_EPI_ROWS.items():
        assert width in (640, 1280) and lo % 128 == 0 and hi % 128 == 0
        if lo <= hi and hi > 0:
            assert hip_layers.wstream_epi_level(kind, lo, width) and hip_layers.wstream_epi_level(kind, hi, width)
            assert not hip_layers.wstream_epi_level(kind, lo + 64, width)      # rows % 128
            monkeypatch.setattr(ops, "GEMM_WSTREAM_EPI", False)
            assert not hip_layers.wstream_epi_level(kind, lo, width)
            monkeypatch.setattr(ops, "GEMM_WSTREAM_EPI", True)
        assert not hip_layers.wstream_epi_level(kind, hi + 128, width)
        assert not hip_layers.wstream_epi_level(kind, 512, 320)               # width 320 has its own kernels
    assert hip_layers.wstream_epi_level("qkv", 512, 640) and hip_layers.wstream_epi_level("geglu", 512, 640)   # the model-level test's block
    torch.manual_seed(0)
    ln, gg, ca = LayerNorm(64), GEGLU(64, 128), CrossAttention(64, heads=2, dim_head=32)
    n = PackCache.builds
    ws = gg.folded_stream(ln)
    assert PackCache.builds == n + 2 and ws.shape == (8, 1, 4, 64, 8)      # the folded weight and its fragment order
    assert gg.folded_stream(ln) is ws and PackCache.builds == n + 2
    with torch.no_grad():
        ln.weight.mul_(2.0)
    ws2 = gg.folded_stream(ln)
    assert PackCache.builds == n + 4 and not torch.equal(ws2, ws)
    n = PackCache.builds
    wq = ca._w_qkv_ln_stream(ln)
    assert PackCache.builds == n + 3 and wq.shape == (6, 1, 4, 64, 8)      # q | k | v, its fold, its fragment order
    assert ca._w_qkv_ln_stream(ln) is wq and PackCache.builds == n + 3
