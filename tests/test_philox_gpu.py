"""The seeded noise generator on the GPU (vd_philox_normal, through the C ABI) against the numpy restatement of
tests/test_philox_cpu.py: values, the single fp16 rounding, independence of the batch a sample runs in, and the draw /
stream words of the counter."""
import numpy as np
import pytest
import torch

from test_philox_cpu import normals_ref_batch

pytestmark = pytest.mark.gpu

SEEDS = [7, 2 ** 40 + 12345, 2 ** 63 - 1]          # low word only, both words, the largest seed
# |z| <= sqrt(48 ln 2) ~ 5.77 and the fp32 rounding of an angle <= 2 pi, plus a few ulp of logf / sincosf, give ~2e-6
ATOL = 2e-5


def _seeds(dev, seeds=SEEDS):
    return torch.tensor(seeds, dtype=torch.int64, device=dev)


@pytest.fixture(scope="module")
def ref():
    return {(p, d, s): normals_ref_batch(SEEDS, p, d, s) for p in (105, 4096) for d, s in ((0, 0), (3, 2))}


@pytest.mark.parametrize("per_sample", [105, 4096])
@pytest.mark.parametrize("draw,stream", [(0, 0), (3, 2)])
def test_fill_matches_restatement(dev, ref, per_sample, draw, stream):
    from vd_hip import ops
    z32 = ops.philox_normal(_seeds(dev), (3, per_sample), draw=draw, stream=stream, dtype=torch.float32)
    z16 = ops.philox_normal(_seeds(dev), (3, per_sample), draw=draw, stream=stream)
    torch.cuda.synchronize()
    assert z32.shape == (3, per_sample) and z32.dtype == torch.float32 and z16.dtype == torch.float16
    err = np.abs(z32.cpu().numpy().astype(np.float64) - ref[per_sample, draw, stream]).max()
    print("max |z - ref| = %.3e" % err)
    assert err < ATOL
    assert torch.equal(z16, z32.half())            # the fp32 value rounded once


def test_scale_and_shape(dev, ref):
    from vd_hip import ops
    z = ops.philox_normal(_seeds(dev), (3, 4, 32, 32), dtype=torch.float32)
    zs = ops.philox_normal(_seeds(dev), (3, 4, 32, 32), dtype=torch.float32, scale=0.5)
    assert z.shape == (3, 4, 32, 32)
    assert torch.equal(zs, z * 0.5)
    assert np.abs(z.reshape(3, -1).cpu().numpy().astype(np.float64) - ref[4096, 0, 0]).max() < ATOL


@pytest.mark.parametrize("per_sample", [105, 4096])
def test_rows_do_not_depend_on_the_batch(dev, per_sample):
    from vd_hip import ops
    for dtype in (torch.float32, torch.float16):
        kw = dict(draw=2, stream=2, dtype=dtype)
        whole = ops.philox_normal(_seeds(dev), (3, per_sample), **kw)
        first = ops.philox_normal(_seeds(dev, SEEDS[:1]), (1, per_sample), **kw)
        rest = ops.philox_normal(_seeds(dev, SEEDS[1:]), (2, per_sample), **kw)
        assert torch.equal(whole, torch.cat([first, rest]))


@pytest.mark.parametrize("per_sample", [105, 4096])
def test_draw_and_stream_change_every_block(dev, per_sample):
    from vd_hip import ops

    def blocks(draw, stream):
        z = ops.philox_normal(_seeds(dev), (3, per_sample), draw=draw, stream=stream, dtype=torch.float32)
        pad = (-per_sample) % 4
        return torch.nn.functional.pad(z, (0, pad)).reshape(3, -1, 4)

    base = blocks(0, 0)
    for other in (blocks(1, 0), blocks(0, 1), blocks(0, 2), blocks(1, 2)):
        assert bool((other != base).any(-1).all())
    assert torch.equal(base, blocks(0, 0))


def test_argument_checks(dev):
    from vd_hip import ops
    from vd_hip.loader import VdHipError
    with pytest.raises(VdHipError):
        ops.philox_normal(_seeds(dev), (2, 16))                                      # one seed per sample
    with pytest.raises(VdHipError):
        ops.philox_normal(_seeds(dev).int(), (3, 16))
    with pytest.raises(VdHipError):
        ops.philox_normal(torch.tensor(SEEDS), (3, 16))                              # host seeds
    with pytest.raises(VdHipError):
        ops.philox_normal(_seeds(dev), (3, 16), dtype=torch.bfloat16)
    with pytest.raises(VdHipError):
        ops.philox_normal(_seeds(dev), (3, 16), draw=-1)
