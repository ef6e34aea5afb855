"""The feed-forward / proj_out fold on the host: the pack against a float64 restatement, exactness of the algebra with integer
operands (both forms emulated with their fp16 roundings), the pack cache's key, the switch and the fall-back conditions, and the
host decisions of the vd_gemm_wstream_cat entries.  The kernels are checked in tests/test_ff_proj_fold_gpu.py."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import ff_proj_fold_cases as F


def test_pack_against_a_float64_restatement():
    from vd_hip.pack import pack_ff_proj_fold
    t = F.normal_tail(4, 64, seed=1)
    w_cat, bm = pack_ff_proj_fold(t.w2, t.b2, t.wp, t.bp)
    assert w_cat.dtype == torch.float16 and w_cat.shape == (64, 5 * 64) and w_cat.is_contiguous()
    assert bm.dtype == torch.float32 and bm.shape == (64,)
    wm = t.wp.double() @ t.w2.double()
    assert torch.equal(w_cat[:, :256], wm.half())          # ONE rounding of the float64 product
    assert torch.equal(w_cat[:, 256:], t.wp)
    bm_ref = t.wp.double() @ t.b2.double() + t.bp.double()
    assert (bm.double() - bm_ref).abs().max() <= 2.0 ** -24 * bm_ref.abs().max()
    # float64 in, nothing rounded: the merged form IS the two-line form
    w64, b64 = pack_ff_proj_fold(t.w2.double(), t.b2.double(), t.wp.double(), t.bp.double())
    assert w64.dtype == torch.float64 and b64.dtype == torch.float64
    merged = t.alpha * (torch.cat([t.h, t.x2], 1).double() @ w64.t() + b64) + t.r.double()
    assert (merged - t.ref).abs().max() < 1e-12 * t.ref.abs().max()


@pytest.mark.parametrize("M,C,seed", [(16, 64, 2), (8, 256, 3)])
def test_integer_operands_make_both_forms_equal_exactly(M, C, seed):
    from vd_hip.pack import pack_ff_proj_fold
    t = F.integer_tail(M, C, seed)
    w_cat, bm = pack_ff_proj_fold(t.w2, t.b2, t.wp, t.bp)
    assert torch.equal(w_cat.double()[:, :4 * C], t.wp.double() @ t.w2.double())     # the product survives its fp16 rounding
    assert torch.equal(bm.half().double(), t.wp.double() @ t.b2.double() + t.bp.double())
    # two launches: y is stored as fp16 in between
    y = (t.x2.double() + t.h.double() @ t.w2.double().t() + t.b2.double()).half()
    assert torch.equal(y.double(), t.y)
    two = (t.alpha * (y.double() @ t.wp.double().t() + t.bp.double()) + t.r.double()).half()
    one = (t.alpha * (torch.cat([t.h, t.x2], 1).double() @ w_cat.double().t() + bm.half().double()) + t.r.double()).half()
    assert torch.equal(one, two) and torch.equal(one, t.ref.half())


def _layers(C=64, bias=True, cout=None):
    from lib.model_zoo.hip_layers import Conv2d, Linear
    torch.manual_seed(5)
    lin = Linear(4 * C, C, bias=bias).half()
    conv = Conv2d(C, C if cout is None else cout, kernel_size=1, stride=1, padding=0).half()
    return lin, conv


def test_cache_key_rebuilds_after_an_in_place_edit_of_either_layer():
    from lib.model_zoo.hip_layers import PackCache
    lin, conv = _layers()
    n0 = PackCache.builds
    w0, b0 = lin._w_proj_fold(conv)
    assert PackCache.builds == n0 + 1
    assert lin._w_proj_fold(conv)[0] is w0 and PackCache.builds == n0 + 1
    s0 = lin._w_proj_fold_stream(conv)
    assert s0.shape == (64 // 32, 5 * 64 // 64, 4, 64, 8) and lin._w_proj_fold_stream(conv) is s0
    with torch.no_grad():
        lin.weight.add_(0.25)
    w1, _ = lin._w_proj_fold(conv)
    assert w1 is not w0 and not torch.equal(w1[:, :256], w0[:, :256]) and torch.equal(w1[:, 256:], w0[:, 256:])
    s1 = lin._w_proj_fold_stream(conv)
    assert s1 is not s0
    with torch.no_grad():
        conv.weight.add_(0.25)
    w2, _ = lin._w_proj_fold(conv)
    assert w2 is not w1 and not torch.equal(w2[:, 256:], w1[:, 256:])
    assert lin._w_proj_fold_stream(conv) is not s1
    with torch.no_grad():
        conv.bias.add_(1.0)
    _, b3 = lin._w_proj_fold(conv)
    assert not torch.equal(b3, b0)
    # the stream is the fragment order of the very matrix the other kernel reads
    from vd_hip.pack import pack_linear_weight_stream
    assert torch.equal(lin._w_proj_fold_stream(conv), pack_linear_weight_stream(lin._w_proj_fold(conv)[0]))


def test_the_switch_and_the_geometry_that_falls_back(monkeypatch):
    from lib.model_zoo import hip_layers
    lin, conv = _layers()
    assert hip_layers.FF_PROJ_FOLD is True      # the default
    assert lin.proj_fold_ok(conv)
    monkeypatch.setattr(hip_layers, "FF_PROJ_FOLD", False)
    assert not lin.proj_fold_ok(conv)
    monkeypatch.setattr(hip_layers, "FF_PROJ_FOLD", True)
    assert not lin.proj_fold_ok(_layers(cout=128)[1])           # proj_out.out_channels != inner
    assert not _layers(bias=False)[0].proj_fold_ok(conv)        # a missing bias, either layer
    from lib.model_zoo.hip_layers import Conv2d
    assert not lin.proj_fold_ok(Conv2d(64, 64, kernel_size=1, bias=False).half())
    assert not lin.proj_fold_ok(Conv2d(64, 64, kernel_size=3, padding=1).half())
    l96, c96 = _layers(C=96)
    assert not l96.proj_fold_ok(c96)                            # widths not a multiple of 64


class _Recorder(object):
    """Stands in for vd_hip.ops on the host: records which launches FeedForward.forward asks for."""

    def __init__(self, ops):
        self.calls, self._ops = [], ops
        self.GEMM_WSTREAM, self.ACT_GEGLU = True, ops.ACT_GEGLU

    def ff_geglu_supported(self, C):
        return False

    def linear(self, x, w, bias=None, **kw):
        self.calls.append(("linear", tuple(w.shape), sorted(kw)))
        n = w.shape[0] // 2 if kw.get("act") == self.ACT_GEGLU else w.shape[0]
        return torch.zeros(x.shape[:-1] + (n,), dtype=torch.float16)

    def gemm(self, a0, w, **kw):
        self.calls.append(("gemm", tuple(w.shape), sorted(kw)))
        return torch.zeros((a0.shape[0], w.shape[0]), dtype=torch.float16)


def test_feed_forward_ends_in_one_launch_or_falls_back(monkeypatch):
    from lib.model_zoo import attention, hip_layers
    from lib.model_zoo.hip_layers import Conv2d, LayerNorm
    from vd_hip import ops
    C = 64
    torch.manual_seed(6)
    ff = attention.FeedForward(C).half()
    ln = LayerNorm(C).half()
    conv = Conv2d(C, C, kernel_size=1).half()
    rec = _Recorder(ops)
    monkeypatch.setattr(attention, "ops", rec)
    monkeypatch.setattr(hip_layers, "ops", rec)
    x = torch.zeros((2, 16, C), dtype=torch.float16)
    pres = torch.zeros((2, 4, 4, C), dtype=torch.float16)
    synced = []

    def run(post, res=x):
        del rec.calls[:], synced[:]
        return ff(x, res=res, ln=ln, post=post, sync=lambda: synced.append(len(rec.calls)))

    out = run((conv, 0.5, pres, 16))
    assert isinstance(out, tuple) and out[1] is True and out[0].shape == (32, C)
    assert [c[0] for c in rec.calls] == ["linear", "gemm"] and rec.calls[1][1] == (C, 5 * C)
    assert {"a1", "alpha", "bias", "res", "want_stats", "stat_img_rows"} <= set(rec.calls[1][2])
    assert "w_stream_cat" not in rec.calls[1][2]            # 32 rows, N = 64: not a shape of the streaming kernel
    assert synced == [1]                                    # right in front of the launch that reads pres
    # without the request, with the switch off, with a strided residual: today's output projection, no sync from here
    for post, flag in ((None, True), ((conv, 0.5, pres, 16), False), ((conv, 0.5, pres.permute(0, 2, 1, 3), 16), True)):
        monkeypatch.setattr(hip_layers, "FF_PROJ_FOLD", flag)
        out = run(post)
        assert not isinstance(out, tuple) and out.shape == (2, 16, C)
        assert [c[0] for c in rec.calls] == ["linear", "linear"] and rec.calls[1][1] == (C, 4 * C) and synced == []
    monkeypatch.setattr(hip_layers, "FF_PROJ_FOLD", True)
    out = run((Conv2d(C, 2 * C, kernel_size=1).half(), 0.5, pres, 16))      # proj_out.out_channels != inner
    assert not isinstance(out, tuple) and synced == []


def test_environment_switch_turns_the_fold_off():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r]\nfrom lib.model_zoo import hip_layers\nprint(hip_layers.FF_PROJ_FOLD)"
            % (root, os.path.join(root, "versatile-diffusion_amd")))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VD_FF_PROJ_FOLD="0"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "False", (out.stdout, out.stderr)


def test_cat_entries_host_decisions_and_the_old_entries_unchanged():
    from vd_hip.loader import VdGemmDesc, lib

    def desc(M, N, K, **kw):
        d = VdGemmDesc()
        d.M, d.N, d.K = M, N, K
        d.a0 = d.w = d.out = d.ws = 16
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def ok(*a, **kw):
        return lib().vd_gemm_wstream_cat_supported(ctypes.byref(desc(*a, **kw)))

    def plan(*a, **kw):
        n = ctypes.c_int(-1)
        assert lib().vd_gemm_wstream_cat_plan(ctypes.byref(desc(*a, **kw)), ctypes.byref(n)) == 0
        return n.value

    two = dict(a1=16, c0=5120, c1=1280)
    assert ok(2048, 1280, 6400, **two) == 1 and ok(512, 1280, 6400, **two) == 1
    assert ok(2048, 1280, 5120) == 1                          # one source is taken too
    assert ok(2048, 640, 3200, a1=16, c0=2560, c1=640) == 0   # N = 640: no whole 256-column tiles
    assert ok(2000, 1280, 6400, **two) == 0                   # ragged rows
    assert ok(2048, 1280, 6400, a1=16, c0=5152, c1=1248) == 0  # a source that is no multiple of 64
    assert ok(2048, 1280, 6400, a1=16, c0=5120, c1=1216) == 0  # K != c0 + c1
    assert ok(2048, 1280, 6400, act=1, **two) == 0            # GEGLU epilogue
    assert ok(2048, 1280, 6400, ksize=3, stride=1, pad=1, **two) == 0
    # 100 chunks on 80 tiles: 3 splits of 34 (240 blocks, one round); the 8x8 level: 13 splits of 8 on 20 tiles
    assert plan(2048, 1280, 6400, **two) == 3 and plan(512, 1280, 6400, **two) == 13
    assert plan(128, 256, 6400, split_k=3, a1=16, c0=5120, c1=1280) == 3
    assert plan(128, 256, 35 * 64, split_k=1) == 2            # 35 chunks: one more than a block unrolls
    # the single-source entries answer what they answered: no second source, 32 chunks per block
    old = ctypes.c_int(-1)
    assert lib().vd_gemm_wstream_supported(ctypes.byref(desc(2048, 1280, 6400, **two))) == 0
    assert lib().vd_gemm_wstream_plan(ctypes.byref(desc(2048, 1280, 6400)), ctypes.byref(old)) == 0 and old.value == 4
    assert lib().vd_gemm_wstream_plan(ctypes.byref(desc(2048, 1280, 5120)), ctypes.byref(old)) == 0 and old.value == 3
