"""vd_conv3x3_ups_phase_f16 (the upsample convolution as four 2x2 phase convolutions) on the GPU, against the upsampled 3x3 form
on vd_gemm_f16 (ops.conv2d_nhwc(..., ups=1) without a phase pack) and against float64.

Exact cases (tests/ups_phase_cases.py; preconditions in tests/test_ups_phase_cpu.py): integer operands for which every fp32 sum
and every summed weight is exact, so the two forms must agree bit for bit and equal the float64 reference in every element.
Random cases: rel-L2 from float64 of both forms on the same operands; the phase form adds one weight rounding of the size of the
output rounding (CPU emulation: 2.9e-4 against 2.1e-4, a factor 1.4) and may not exceed twice the 3x3 form's distance.
Measured on MI355X, (phase form, 3x3 form) per case: see the docstring of test_random_rel_l2_within_twice_the_3x3_form.
"""
import pytest
import torch

import ups_phase_cases as U
from vdtest_util import assert_exact, rel_l2

pytestmark = pytest.mark.gpu

NYXC = ("image", "y", "x", "channel")
UNET_NAME = "conv3x3_halo_kernel<256,160,32,160,512,2,phase4>"
VAE_NAME = "conv3x3_halo_kernel<256,128,64,64,512,2,phase4>"


@pytest.fixture(scope="module")
def ops():
    from vd_hip import ops as o
    return o


@pytest.fixture(autouse=True)
def _phase_on(ops, monkeypatch):
    monkeypatch.setattr(ops, "UPS_PHASE", True)


def _profiled(ops, fn):
    ops.profile_begin()
    try:
        out = fn()
    finally:
        names = [r[0] for r in ops.profile_end()]
    return out, names


def _both(ops, t, dev, **kw):
    """(phase form, 3x3 form, names of the phase form's launches, names of the 3x3 form's) on the operands of case t."""
    from vd_hip.pack import pack_conv_weight, pack_conv_weight_ups_phase
    x, b = t.x.to(dev), t.bias.to(dev)
    wp, wph = pack_conv_weight(t.w).to(dev), pack_conv_weight_ups_phase(t.w).to(dev)
    split = t.case["split"]
    new, n_new = _profiled(ops, lambda: ops.conv2d_nhwc(x, wp, b, ups=1, w_phase=wph, split_k=split, **kw))
    old, n_old = _profiled(ops, lambda: ops.conv2d_nhwc(x, wp, b, ups=1, **kw))
    return new, old, n_new, n_old


def _expect_name(c):
    return UNET_NAME if c["Cout"] % 160 == 0 else VAE_NAME


def _folded(buf, B, T, R):
    """Partials [B * T, C, 2] of R rows each -> per-(image, channel) (mean, M2), Chan's update in float64."""
    p = buf.double().view(B, T, -1, 2)
    mean = p[..., 0].mean(1)
    m2 = p[..., 1].sum(1) + (R * (p[..., 0] - mean[:, None]) ** 2).sum(1)
    return mean, m2


def _check_stats(ops, out, B, HW, Co):
    st = ops.stats_of(out)
    assert st is not None, "the phase form should emit statistics"
    assert st.HW == HW and st.C == Co and st.buf.shape == (B * st.T, Co, 2)
    mean, m2 = _folded(st.buf, B, st.T, HW // st.T)
    o = out.double().view(B, HW, Co)
    rmean = o.mean(1)
    rm2 = ((o - rmean[:, None]) ** 2).sum(1)
    # the tolerance of test_kernels_gpu.py::test_gemm_out_stats (_stats_close): mean to 2e-4, M2 to 1e-3 of its scale
    dm = (mean - rmean).abs().max().item()
    d2 = (m2 - rm2).abs().max().item() / (rm2.abs().max().item() + 1e-6)
    print("stats: |d mean| %.3g, |d M2| / scale %.3g, T = %d" % (dm, d2, st.T))
    assert dm < 2e-4 and d2 < 1e-3, (dm, d2)


@pytest.mark.parametrize("name", list(U.CASES))
def test_exact_bit_for_bit(ops, dev, name):
    t = U.exact_case(name)
    c = t.case
    new, old, n_new, n_old = _both(ops, t, dev)
    assert n_new[0].startswith(_expect_name(c)), n_new
    assert not any("phase4" in n for n in n_old), n_old
    assert_exact(new, t.ref, NYXC, "phase form, %s" % name)
    assert_exact(old, t.ref, NYXC, "3x3 form, %s" % name)
    assert torch.equal(new, old)


@pytest.mark.parametrize("name", ["a_small_images", "b_seams_borders", "c_split_chunks"])
def test_exact_with_statistics(ops, dev, name):
    """out_stats from the kernel's epilogue (one phase of a whole small image / of a 256-pixel patch per partial) and from the
    split-K reduce: the output is unchanged by the request, and the folded partials are mean and M2 of the stored tensor."""
    t = U.exact_case(name)
    c = t.case
    new, _, n_new, _ = _both(ops, t, dev, want_stats=True)
    assert n_new[0].startswith(_expect_name(c)), n_new
    assert_exact(new, t.ref, NYXC, "phase form with statistics, %s" % name)
    _check_stats(ops, new, c["B"], 4 * c["H"] * c["W"], c["Cout"])


@pytest.mark.parametrize("name", list(U.CASES))
def test_random_rel_l2_within_twice_the_3x3_form(ops, dev, name):
    """Measured on MI355X (phase form, 3x3 form): a_small_images 2.92e-4, 2.08e-4; b_seams_borders 2.92e-4, 2.08e-4;
    c_split_chunks 2.92e-4, 2.08e-4; d_vae_128 2.93e-4, 2.09e-4; d_vae_256 2.92e-4, 2.07e-4 -- a ratio of 1.40 .. 1.41 in every case."""
    t = U.random_case(name)
    new, old, n_new, _ = _both(ops, t, dev)
    assert n_new[0].startswith(_expect_name(t.case)), n_new
    e_new, e_old = rel_l2(new, t.ref), rel_l2(old, t.ref)
    print("%s: rel-L2 from float64: phase form %.3g, 3x3 form %.3g, ratio %.2f" % (name, e_new, e_old, e_new / e_old))
    assert e_new <= 2.0 * e_old, (e_new, e_old)
    assert e_new < 1e-3


# (module, channels, images, low-resolution size): the three UNet upsample layers and the widest VAE one at a small image
REAL_LAYERS = [("unet", 640, 1, 16), ("unet", 1280, 1, 16), ("unet", 1280, 4, 8), ("vae", 512, 1, 16)]


@pytest.mark.parametrize("which,C,B,S", REAL_LAYERS)
def test_upsample_layers_launch_the_phase_instance(ops, dev, monkeypatch, which, C, B, S):
    if which == "unet":
        from lib.model_zoo.openaimodel import Upsample
        up = Upsample(C, True)
    else:
        from lib.model_zoo.autokl_modules import Upsample
        up = Upsample(C, with_conv=True)
    up = up.half().to(dev)
    g = torch.Generator(device="cpu").manual_seed(C + S)
    x = torch.randn((B, S, S, C), generator=g).half().to(dev)
    new, n_new = _profiled(ops, lambda: up(x))
    assert len(n_new) == 1 and n_new[0].startswith(UNET_NAME if which == "unet" else VAE_NAME), n_new
    assert new.shape == (B, 2 * S, 2 * S, C) and ops.stats_of(new) is not None
    monkeypatch.setattr(ops, "UPS_PHASE", False)      # VD_UPS_PHASE=0: today's launches
    old, n_old = _profiled(ops, lambda: up(x))
    assert n_old and not any("phase4" in n for n in n_old), n_old
    e = rel_l2(new, old)
    print("%s C=%d: rel-L2 phase form vs 3x3 form %.3g" % (which, C, e))
    assert e < 1e-3      # two fp16 roundings of O(1) outputs apart (each 2^-11 / sqrt(3) = 2.8e-4 rel-L2)


def test_tiny_model_forward_launches_the_phase_instance(ops, dev, monkeypatch):
    """The fixture model: a CFG-batched UNet forward (four 8x8 images into the 128-channel upsample) and a VAE decode."""
    from lib.model_zoo import get_model
    from vdtest_util import load_gold, meta, synth_into, tiny_vd_cfg
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    synth_into(net, m["seed"])
    net = net.half()
    net.to(dev)
    g = load_gold("unet_tiny.npz")
    x = torch.from_numpy(g["x"]).half().to(dev)
    t = torch.from_numpy(g["t"]).to(dev)
    c = torch.from_numpy(g["c_text"]).half().to(dev)
    x4, t4, c4 = torch.cat([x, x]), torch.cat([t, t]), torch.cat([c, c])
    z = torch.from_numpy(load_gold("ddim_tiny.npz")["z_t2i"]).half().to(dev)

    def run():
        eps = net.apply_model({"type": "image", "x": x4}, t4, {"type": "text", "c": c4})
        return eps, net.vae_decode(z, which="image")

    (eps, img), names = _profiled(ops, run)
    assert sum(1 for n in names if n.startswith(VAE_NAME)) >= 2, [n for n in names if "halo" in n]   # 128 channels: the 256 x 128 tile
    monkeypatch.setattr(ops, "UPS_PHASE", False)
    (eps0, img0), names0 = _profiled(ops, run)
    assert not any("phase4" in n for n in names0)
    assert rel_l2(eps, eps0) < 5e-3 and rel_l2(img, img0) < 5e-3
