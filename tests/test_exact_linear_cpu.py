"""The inputs of the exact GPU tests (tests/exact_cases.py), checked without a GPU: every case's float64 reference consists of
integers (or multiples of alpha for the fp32 outputs) of magnitude <= 2048 with fewer than 15 % zeros -- the conditions under which
a kernel output must equal it in every element -- and one demonstration of what the aggregate bound cannot see."""
import pytest
import torch

import exact_cases as X
from vdtest_util import check_exact_reference, exact_ints, exact_mismatch, exact_operand, rel_l2


def test_exact_operand_values_and_seeding():
    a = exact_operand((512, 64), 7)
    assert a.dtype == torch.float16 and torch.equal(a, exact_operand((512, 64), 7)) and not torch.equal(a, exact_operand((512, 64), 8))
    share = [(a == v).float().mean().item() for v in (-1.0, 0.0, 1.0)]
    assert set(a.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert abs(share[0] - 0.25) < 0.02 and abs(share[1] - 0.5) < 0.02 and abs(share[2] - 0.25) < 0.02
    b = exact_ints((4096,), 9)
    assert b.dtype == torch.float16 and b.min().item() == -8 and b.max().item() == 8 and torch.equal(b, b.round())


def test_every_family_has_cases():
    for fam in X.FAMILIES:
        assert X.names(fam), fam


@pytest.mark.parametrize("name", list(X.CASES))
def test_case_reference_is_exactly_representable(name):
    t = X.build(name)
    check_exact_reference(t.ref, t.unit, name)
    for extra in ("ref_plain", "ref_bias"):   # the launches without the additive terms (GEMM cases)
        if hasattr(t, extra):
            check_exact_reference(getattr(t, extra), t.unit, name + "." + extra)


def test_mismatch_report_names_the_coordinates():
    ref = torch.arange(24, dtype=torch.float64).view(2, 3, 4)
    out = ref.clone().half()
    assert exact_mismatch(out, ref, ("image", "row", "col")) is None
    out[1, 2, 3] += 1
    out[1, 0, 1] -= 2
    msg = exact_mismatch(out, ref, ("image", "row", "col"), "override 3")
    assert msg.startswith("override 3: 2 of 24 elements differ") and "extent: image 1..1, row 0..2, col 1..3" in msg
    assert "(image=1, row=0, col=1): got 11, expected 13" in msg and "(image=1, row=2, col=3): got 24, expected 23" in msg


def test_one_missing_corner_tap_passes_the_aggregate_bound_and_fails_the_exact_one():
    """A halo convolution that pads the (-1, -1) tap wrongly at pixel (0, 0) for 8 output channels -- the tap lies in the padding
    there, so a wrong pad is a clamped address: it reads the pixel itself instead of the zero -- on (1, 32, 64, 64 -> 160) with
    bias and residual: with Gaussian operands as in test_conv3x3_halo_every_variant the result stays under the rel_l2 < 2e-3 bound
    of that test; with the exact operands the same defect is a mismatch located at (image 0, y 0, x 0)."""
    c = X.CASES["halo_32wide_tiles_xy"]
    B, H, W, Cin, Co = c["B"], c["H"], c["W"], c["c0"], c["Co"]

    def corner_tap(x, w):   # what the wrongly padded tap adds at (0, 0): sum_c x[0, 0, 0, c] * w[n, c, 0, 0] for 8 channels
        return x[0, 0, 0].double() @ w[:8, :, 0, 0].double().t()

    def rnd(shape, scale, seed):   # the tolerance tests' generator (tests/test_kernels_gpu.py: rnd), seeds of that test
        return (torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed)) * scale).half()

    x, w = rnd((B, H, W, Cin), 1.0, 100), rnd((Co, Cin, 3, 3), 0.04, 102)
    true = X.conv_ref(x, w, 1, 1, 0) + rnd((Co,), 0.3, 103).double() + rnd((B, H, W, Co), 1.0, 105).double()
    wrong = true.clone()
    wrong[0, 0, 0, :8] += corner_tap(x, w)
    assert not torch.equal(wrong, true)
    assert rel_l2(wrong, true) < 2e-3      # invisible to the aggregate bound ...
    t = X.build("halo_32wide_tiles_xy")
    wrong = t.ref.clone()
    wrong[0, 0, 0, :8] += corner_tap(t.x, t.w)
    msg = exact_mismatch(wrong.half(), t.ref, ("image", "y", "x", "channel"), "variant 3")
    assert msg is not None and "image=0, y=0, x=0" in msg      # ... and a located mismatch for the exact comparison
