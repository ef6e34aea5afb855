"""Every MFMA GEMM and convolution path, element by element and without a tolerance.

The operands of tests/exact_cases.py are small integers, so every product and every partial sum -- fp32 accumulators, fp32 split-K
slabs, the in-kernel fix-up, the reduce launch, the final fp16 rounding -- is exact in any order: the output of a kernel equals the
float64 reference in every element, whatever tile shape, split factor or summation order it uses, and a dropped, duplicated or
mislocated term changes some element by at least 1.  A failure reports the mismatching coordinates and the active override, variant
or split (vdtest_util.exact_mismatch).  Only exact epilogues are covered (bias, row vector, residual, power-of-two alpha, two-source
concat, folded skip convolution); activations, GEGLU and the LayerNorm fold are checked per element by test_exact_epilogue_gpu.py.
"""
import pytest
import torch

import exact_cases as X
from vdtest_util import assert_exact, check_exact_reference

pytestmark = pytest.mark.gpu

RC = ("row", "col")
BRC = ("batch", "row", "col")
NYXC = ("image", "y", "x", "channel")


@pytest.fixture(scope="module")
def ops():
    from vd_hip import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from vd_hip.loader import lib as l
    return l()


def _case(name, dev):
    """(case, operands on the device, operands / reference on the host); the reference's preconditions are asserted first."""
    t = X.build(name)
    check_exact_reference(t.ref, t.unit, name)
    d = {k: (v.to(dev) if torch.is_tensor(v) and not k.startswith("ref") else v) for k, v in vars(t).items()}
    return t.case, type(t)(**d), t


def _built_configs(lib):
    """-1 (the planner) and every instantiated tile configuration; restore with ops.gemm_set_override(-1)."""
    yield -1
    for cfg in range(lib.vd_gemm_num_configs()):
        if lib.vd_gemm_set_override(cfg) == 0:   # slots of removed development tiles refuse
            yield cfg


def _profiled(ops, fn):
    ops.profile_begin()
    try:
        out = fn()
    finally:
        names = [r[0] for r in ops.profile_end()]
    return out, names


# ---- gemm_f16_kernel -----------------------------------------------------------------------------------------------------------

def _gemm_kw(c, g, res=True, rowvec=True):
    kw = dict(bias=g.bias)
    if c["k1"]:
        kw.update(a1=g.a1, K=c["K"], N=c["N"])
    if rowvec and g.rowvec is not None:
        kw.update(rowvec=g.rowvec, rows_per_batch=c["rpb"])
    if res and g.res is not None:
        kw.update(res=g.res)
    return kw


@pytest.mark.parametrize("name", ["gemm_ragged", "gemm_two_source"])
def test_gemm_every_tile_configuration(ops, lib, dev, name):
    """Ragged M / N / K with bias + row vector + residual, and a two-source A, on every instantiated tile (problems narrower than
    96 columns keep the planner's 64 x 64 tile under an override: plan_gemm)."""
    c, g, t = _case(name, dev)
    ran = 0
    try:
        for cfg in _built_configs(lib):
            ops.gemm_set_override(cfg)
            ctx = "%s, override %d (%s)" % (name, cfg, ops.gemm_kernel_name(cfg) if cfg >= 0 else "planner")
            assert_exact(ops.gemm(g.a0, g.w, **_gemm_kw(c, g)), t.ref, RC, ctx)
            if g.rowvec is not None:
                assert_exact(ops.gemm(g.a0, g.w, **_gemm_kw(c, g, res=False, rowvec=False)), t.ref_bias, RC, ctx + ", bias only")
            ran += 1
    finally:
        ops.gemm_set_override(-1)
    assert ran >= 10


@pytest.mark.parametrize("name", ["gemm_width_100", "gemm_width_102"])
def test_gemm_unaligned_widths(ops, dev, name):
    """Widths that are no multiple of 8 (100) or of 4 (102): the element-wise tail of the epilogue; the planner's tile."""
    c, g, t = _case(name, dev)
    assert_exact(ops.gemm(g.a0, g.w, **_gemm_kw(c, g)), t.ref, RC, name)
    assert_exact(ops.gemm(g.a0, g.w, bias=g.bias), t.ref_bias, RC, name + ", bias only")
    assert_exact(ops.gemm(g.a0, g.w), t.ref_plain, RC, name + ", no epilogue")


def test_gemm_split_k_both_fixup_forms(ops, lib, dev):
    """33 k-tiles over 2 / 5 / 32 splits (ragged last split) through the reduce launch and through the arrival-counter fix-up, which
    runs twice so that the counters re-arm; afterwards the counters are all zero."""
    c, g, t = _case("gemm_split_k", dev)
    try:
        for cfg in _built_configs(lib):
            ops.gemm_set_override(cfg)
            for split in c["splits"]:
                for fixup, reps in ((False, 1), (True, 2)):
                    for rep in range(reps):
                        out = ops.gemm(g.a0, g.w, bias=g.bias, res=g.res, split_k=split, fixup=fixup)
                        assert_exact(out, t.ref, RC, "override %d, split_k %d, fixup %s, launch %d" % (cfg, split, fixup, rep))
    finally:
        ops.gemm_set_override(-1)
    assert int(ops.sync_counters(dev).abs().sum()) == 0


def test_gemm_batched(ops, lib, dev):
    """Batched launches with strides: alpha = 0.25 into fp32, a shared A (stride 0) with the bias along M, and batched split-K in both
    fix-up forms."""
    try:
        for cfg in _built_configs(lib):
            ops.gemm_set_override(cfg)
            c, g, t = _case("bgemm_alpha_f32", dev)
            Bt, M, N, K = c["Bt"], c["M"], c["N"], c["K"]
            out = ops.gemm(g.a, g.w, M=M, N=N, K=K, batch=Bt, strides=(M * K, N * K, M * N, 0), alpha=c["alpha"], out_f32=True)
            assert out.dtype == torch.float32
            assert_exact(out, t.ref, BRC, "alpha 0.25 -> fp32, override %d" % cfg)
            c, g, t = _case("bgemm_shared_a_bias_m", dev)
            out = ops.gemm(g.a, g.w, bias=g.bias, bias_along_m=True, M=M, N=N, K=K, batch=Bt, strides=(0, N * K, M * N, 0))
            assert_exact(out, t.ref, BRC, "shared A, bias along M, override %d" % cfg)
            c, g, t = _case("bgemm_split_k", dev)
            for fixup in (False, True, True):
                out = ops.gemm(g.a, g.w, M=M, N=N, K=K, batch=Bt, strides=(M * K, N * K, M * N, 0), split_k=c["split"], fixup=fixup)
                assert_exact(out, t.ref, BRC, "batched split_k %d, fixup %s, override %d" % (c["split"], fixup, cfg))
    finally:
        ops.gemm_set_override(-1)
    assert int(ops.sync_counters(dev).abs().sum()) == 0


def _conv_call(ops, c, g, wp, **extra):
    kw = dict(ksize=c["ks"], stride=c["stride"], pad=c["pad"], ups=c["ups"], x1=g.x1, pad_hi=c["pad_hi"])
    if g.rowvec is not None:
        kw.update(rowvec=g.rowvec, rows_per_batch=g.rows_per_image)
    if g.res is not None:
        kw.update(res=g.res)
    kw.update(extra)
    return ops.conv2d_nhwc(g.x, wp, g.bias, **kw)


@pytest.mark.parametrize("name", [n for n in X.names("gemm_f16", "conv")])
def test_implicit_convolution_on_the_gemm_kernel(ops, lib, dev, name):
    """The implicit-GEMM gather of gemm_f16_kernel (halo kernel switched off): ragged 17 x 13 grid, stride 2 with symmetric and with
    one-sided padding, nearest-2x upsampling, 3x3 and 1x1 on a two-source concat with row vector and residual; every tile."""
    from vd_hip.pack import pack_conv_weight
    c, g, t = _case(name, dev)
    wp = pack_conv_weight(g.w)
    try:
        assert lib.vd_conv_halo_set_variant(0) == 0
        for cfg in _built_configs(lib):
            ops.gemm_set_override(cfg)
            out, names = _profiled(ops, lambda: _conv_call(ops, c, g, wp))
            assert names and all(n.startswith("gemm_f16_kernel") for n in names), names
            assert_exact(out, t.ref, NYXC, "%s, override %d" % (name, cfg))
    finally:
        ops.gemm_set_override(-1)
        lib.vd_conv_halo_set_variant(-1)


# ---- conv3x3_halo_kernel -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", X.names("halo", "conv"))
def test_halo_convolution_every_variant(ops, lib, dev, name):
    """conv3x3_halo_kernel, forced variants 3 / 6 / 13 (instances 2, 5 and 12) and the planner: several patches in x and y, 16- and
    8-wide patches (four whole images per patch, told apart by a per-image constant), upsampling in front, three patches per row,
    ragged output columns, a ragged and a planned split over channel chunks.  The profile must show the halo kernel for every forced
    variant, and for the planner where the table says it takes the case."""
    from vd_hip.pack import pack_conv_weight
    c, g, t = _case(name, dev)
    wp = pack_conv_weight(g.w)
    extra = dict(split_k=c["split_k"]) if c.get("split_k") else {}
    try:
        for v in (-1, 3, 6, 13):
            assert lib.vd_conv_halo_set_variant(v) == 0
            out, names = _profiled(ops, lambda: _conv_call(ops, c, g, wp, **extra))
            if v > 0 or c["planner"]:
                assert len(names) == 1 and names[0].startswith("conv3x3_halo_kernel"), (v, names)
            assert_exact(out, t.ref, NYXC, "%s, halo variant setting %d (%s)" % (name, v, names))
    finally:
        lib.vd_conv_halo_set_variant(-1)


@pytest.mark.parametrize("name", X.names("halo", "skipconv"))
def test_halo_convolution_with_folded_skip_conv(ops, lib, dev, name):
    """Instance 12: the 1x1 skip convolution as one-tap chunks behind the 3x3 chunks (fewer skip chunks than splits; one skip
    source), against conv3x3(h) + conv1x1(cat(s0, s1)).  Only the planner and setting 3 lead to instance 12 (conv_halo.hip)."""
    from vd_hip.pack import pack_conv_weight
    c, g, t = _case(name, dev)
    wp = pack_conv_weight(g.w3)
    try:
        for v in (-1, 3):
            assert lib.vd_conv_halo_set_variant(v) == 0
            out, names = _profiled(ops, lambda: ops.conv2d_nhwc(g.h, wp, g.bias, ksize=3, pad=1, skip=(g.s0, g.s1, g.w1)))
            assert out is not None, "the halo kernel should take this launch (setting %d)" % v
            assert len(names) == 1 and names[0].startswith("conv3x3_halo_kernel") and "skip" in names[0], (v, names)
            assert_exact(out, t.ref, NYXC, "%s, halo variant setting %d" % (name, v))
    finally:
        lib.vd_conv_halo_set_variant(-1)


# ---- weight-streaming 8x8 convolutions -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", X.names("wstream_conv", "conv"))
def test_weight_streaming_convolution(ops, lib, dev, name, monkeypatch):
    """conv3x3_wsk_kernel (whole K per block; it takes inputs of at least 4 chunks) and conv3x3_wstream_kernel + reduce in every
    instance at three grid targets: 2 to 5 chunks, ragged splits, two sources, row vector and residual."""
    from vd_hip.pack import pack_conv_weight, pack_conv_weight_stream
    c, g, t = _case(name, dev)
    wp, wsm = pack_conv_weight(g.w), pack_conv_weight_stream(g.w)
    monkeypatch.setenv("VD_WSK", "1")
    monkeypatch.setenv("VD_WSK_MIN_BLOCKS", "1")
    out, names = _profiled(ops, lambda: _conv_call(ops, c, g, wp, w_stream=wsm))
    whole_k = (c["c0"] + c["c1"]) // 64 >= 4
    assert names == ["conv3x3_wsk_kernel" if whole_k else "conv3x3_wstream_kernel + reduce"], names
    assert_exact(out, t.ref, NYXC, "%s, VD_WSK=1 (%s)" % (name, names[0]))
    monkeypatch.setenv("VD_WSK", "0")
    try:
        for var in range(4):
            for target in (64, 256, 1024):
                assert lib.vd_conv3x3_wstream_set_variant(var, target) == 0
                out, names = _profiled(ops, lambda: _conv_call(ops, c, g, wp, w_stream=wsm))
                assert names == ["conv3x3_wstream_kernel + reduce"], names
                assert_exact(out, t.ref, NYXC, "%s, split kernel instance %d, grid target %d" % (name, var, target))
    finally:
        lib.vd_conv3x3_wstream_set_variant(0, 256)


def test_weight_streaming_convolution_with_folded_skip_conv(ops, lib, dev, monkeypatch):
    """The split kernel with the fragment-ordered skip weights (one-tap chunks behind the 3x3 chunks, fewer skip chunks than splits)."""
    from vd_hip.pack import pack_conv_weight, pack_conv_weight_stream, pack_linear_weight_stream
    name = "wstream_skip"
    c, g, t = _case(name, dev)
    wp, wsm, w1s = pack_conv_weight(g.w3), pack_conv_weight_stream(g.w3), pack_linear_weight_stream(g.w1)
    try:
        for target in (64, 256, 1024):
            assert lib.vd_conv3x3_wstream_set_variant(0, target) == 0
            out, names = _profiled(ops, lambda: ops.conv2d_nhwc(g.h, wp, g.bias, ksize=3, pad=1, w_stream=wsm, skip=(g.s0, g.s1, g.w1, w1s)))
            assert out is not None and names == ["conv3x3_wstream_kernel + reduce"], names
            assert_exact(out, t.ref, NYXC, "%s, grid target %d" % (name, target))
    finally:
        lib.vd_conv3x3_wstream_set_variant(0, 256)


# ---- gemm_wstream_kernel, rowgemm320_kernel --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", X.names("gemm_wstream"))
def test_weight_streaming_gemm(ops, dev, name):
    """gemm_wstream_kernel + reduce: one chunk, 33 chunks (one more than a block unrolls: the launcher must split) and an explicit
    split of 2, with bias and with bias + residual."""
    from vd_hip.pack import pack_linear_weight_stream
    c, g, t = _case(name, dev)
    ws = pack_linear_weight_stream(g.w)
    for res, ref, what in ((None, t.ref_bias, "bias"), (g.res, t.ref, "bias + residual")):
        out, names = _profiled(ops, lambda: ops.gemm(g.a0, g.w, bias=g.bias, res=res, w_stream=ws, split_k=c["split"]))
        assert names == ["gemm_wstream_kernel + reduce"], names
        assert_exact(out, ref, RC, "%s, %s, split_k %d" % (name, what, c["split"]))


@pytest.mark.parametrize("name", X.names("row320"))
def test_row_resident_gemm_320(ops, lib, dev, name):
    """rowgemm320_kernel called directly: three full 128-row blocks and a ragged one of 5 rows, one and three 320-column panels,
    with and without the residual (which must arrive on the ragged block too)."""
    c, g, t = _case(name, dev)
    assert lib.vd_gemm_row320_supported(c["M"], c["N"], 320) == 1
    out, names = _profiled(ops, lambda: ops.gemm_row320(g.a0, g.w, g.bias, g.res, False, 1e-5))
    assert names == ["rowgemm320_kernel"], names
    assert_exact(out, t.ref, RC, name)


# ---- fixed-point channel sums emitted with the stored output ---------------------------------------------------------------------

@pytest.mark.parametrize("name,setting", [("halo_three_patches_per_row", -1), ("halo_split_planner", 3), ("iconv_concat_1x1", 0)])
def test_emitted_channel_sums(ops, lib, dev, name, setting, monkeypatch):
    """VdGemmDesc.stat_sums (want_stats=True, st.sums) from the halo epilogue (256-pixel patches), from the split-K reduce launch
    (64-row blocks) and from the epilogue of gemm_f16_kernel: sum x 2^32 per (image, channel) must equal the int64 sum of the
    reference.  A partial's mean is pivot + S / R with integer S and R a power of two, and R * mean * 2^32 is formed in fp64: exact.
    The sum of squares is NOT exact by construction and is left out: M2 = Q - S * S / R is formed in fp32 (gemm_kernel.h,
    emit_chan_stats: `m2 = fmaxf(Q - S * S / n, 0.f)`; gemm.hip, splitk_reduce_stats_kernel: `Q - S * S / 64.f`), and S * S passes
    2^24 as soon as a partial's mean lies 16 (R = 256) or 64 (R = 64) away from its pivot row; its tolerance test is
    test_gemm_out_stats."""
    from vd_hip.pack import pack_conv_weight
    monkeypatch.setattr(ops, "GN_SUMS", True)       # (opt-in in the product: VD_GN_SUMS=1)
    monkeypatch.setattr(ops, "GN_FUSED_MAX", 0)     # tensors of any size carry the sums
    c, g, t = _case(name, dev)
    wp = pack_conv_weight(g.w)
    B, Co = c["B"], c["Co"]
    try:
        assert lib.vd_conv_halo_set_variant(setting) == 0
        out, names = _profiled(ops, lambda: _conv_call(ops, c, g, wp, want_stats=True))
    finally:
        lib.vd_conv_halo_set_variant(-1)
    assert names[0].startswith("conv3x3_halo_kernel") == (setting != 0), names
    assert_exact(out, t.ref, NYXC, "%s with statistics (%s)" % (name, names))
    st = ops.stats_of(out)
    assert st is not None and st.sums is not None, "this producer should emit statistics and sums"
    got = st.sums.view(B, Co, 2)[..., 0].cpu()
    exp = (t.ref.view(B, -1, Co).sum(1) * 2.0 ** 32).long()
    bad = (got != exp).nonzero()
    assert bad.shape[0] == 0, "%s: %d of %d channel sums differ, first (image, channel) %s: got %s / 2^32, expected %s" % (
        name, bad.shape[0], exp.numel(), bad[:4].tolist(), [got[tuple(i)].item() / 2.0 ** 32 for i in bad[:4]],
        [exp[tuple(i)].item() / 2.0 ** 32 for i in bad[:4]])
