"""Every attention kernel, element by element: attn_fwd_kernel<40|64|80|160, 4>, attn_pipe_kernel<40>, attn_fwd_kernel<40, 8>,
attn_wide_kernel<128|256|512>, xattn_kernel<40|80|160> and softmax_rows_kernel.

The operands of tests/attn_cases.py make every probability a kernel forms exactly 0 or one constant per row and v a small non-zero
integer, so the output must be the float64 softmax result correctly rounded to fp16 (bit-for-bit equal where the reference is an
fp16 value: every selector case) -- vdtest_util.attn_mismatch, one rule for every case, no case widened.  The reference is the
float64 result of the whole operation on the fp16 operands (for the fused kernel: LayerNorm, projection with the folded fp16 weight,
q rounded to fp16, softmax . V); tests/test_exact_attention_cpu.py checks its preconditions without a GPU.  A failure reports the
failing coordinates, their extent, the selected key and the query block and wave of the first failure.
"""
import os
import subprocess
import sys

import pytest
import torch

import attn_cases as A
from vdtest_util import attn_mismatch

pytestmark = pytest.mark.gpu

SENTINEL = 1234.0


@pytest.fixture(scope="module")
def ops():
    from vd_hip import ops as o
    return o


def run_attention(ops, dev, name):
    """ops.attention on a case of attn_cases -> out [B, Nq, H, D] on the host"""
    t = A.build(name)
    c = t.case
    out = ops.attention(t.q.to(dev), t.k.to(dev), t.v.to(dev), c["H"], causal=c["causal"])
    return t, out.cpu().view(c["B"], c["Nq"], c["H"], c["D"])


def check(t, out, **where):
    msg = attn_mismatch(out, t.ref, t.case["name"], win_key=t.pi, **where)
    assert msg is None, msg


@pytest.mark.parametrize("name", [n for n in A.names("fwd4") if not A.CASES[n].get("views")])
def test_attn_fwd_kernel_4_waves(ops, dev, name):
    """attn_fwd_kernel<D, 4>: the three block mappings, ragged query blocks and key tiles, the causal diagonal, double- and
    single-buffered tiles, row sums from the column of ones (D = 40, 80) and from the VALU (D = 64, 160)."""
    check(*run_attention(ops, dev, name))


@pytest.mark.parametrize("name", [n for n in A.names("fwd4") if A.CASES[n].get("views")])
def test_attn_fwd_kernel_strided_views_and_guarded_output(ops, dev, name):
    """q, k, v are column slices of one fused [B, N, 3C] projection; out= is a column slice of a wider buffer (ldo = C + 8) with
    spare rows after Nq, pre-filled with a sentinel: every element outside the [B, Nq, C] window must still hold it."""
    t = A.build(name)
    c = t.case
    B, H, D, N = c["B"], c["H"], c["D"], c["Nq"]
    C = H * D
    qkv = torch.cat([t.q, t.k, t.v], -1).to(dev)
    buf = torch.full((B, N + 3, C + 8), SENTINEL, dtype=torch.float16, device=dev)
    window = buf[:, :N, 4:4 + C]
    ret = ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], H, causal=c["causal"], out=window)
    assert ret.data_ptr() == window.data_ptr()
    host = buf.cpu()
    check(t, host[:, :N, 4:4 + C].reshape(B, N, H, D))
    guard = torch.ones_like(host, dtype=torch.bool)
    guard[:, :N, 4:4 + C] = False
    stray = (guard & (host != SENTINEL)).nonzero()
    assert stray.shape[0] == 0, "%s: %d elements outside the output window were written, first at (batch, row, column) %s" % (
        name, stray.shape[0], stray[0].tolist())


@pytest.mark.parametrize("name", A.names("pipe"))
def test_attn_pipe_kernel(ops, dev, name):
    """attn_pipe_kernel<40>: both block mappings, a last block with empty row blocks and waves, last tiles of one and six keys,
    winners at key 0, in the last tile and one 32-key step before the end."""
    check(*run_attention(ops, dev, name), qblock=512, wave_rows=64)


@pytest.mark.parametrize("name", A.names("wide"))
def test_attn_wide_kernel(ops, dev, name):
    """attn_wide_kernel<128|256|512>: partial scores of four waves meet in LDS; ragged key tiles and query blocks."""
    t, out = run_attention(ops, dev, name)
    check(t, out, qblock=32, wave_cols=t.case["D"] // 4)


@pytest.mark.parametrize("name", A.names("xattn"))
def test_xattn_kernel(ops, dev, name):
    """xattn_kernel<40|80|160> through ops.xattn with hip_layers.fold_layernorm: plain and XCD block order, two-buffer tile ring."""
    from lib.model_zoo.hip_layers import fold_layernorm
    t = A.build(name)
    c = t.case
    B, H, D, Nq = c["B"], c["H"], c["D"], c["Nq"]
    C = H * D
    assert ops.xattn_supported(H, D)
    ln = torch.nn.LayerNorm(C, eps=A.LN_EPS).to(dev)
    with torch.no_grad():
        ln.weight.copy_(t.gamma)
        ln.bias.copy_(t.beta)
    w, b, cs = fold_layernorm(t.wq.to(dev), None, ln)
    assert torch.equal(w.cpu(), t.w_fold) and bool((b == 0).all())
    if c["kind"] == "uniform":
        b = None
    out = ops.xattn(t.x.to(dev), w, b, cs, A.LN_EPS, t.k.to(dev), t.v.to(dev), H)
    check(t, out.cpu().view(B, Nq, H, D))


# ---- softmax_rows_kernel, both output types --------------------------------------------------------------------------------------

def _softmax_rows_input(n):
    """[6, n] fp32 logits, all multiples of 2^-8 of magnitude < 64 (so x - max is exact in fp32 and the only error left is the
    kernel's): two random rows (sigma 5), a row whose maximum is its last element, a row of equal values, a row that falls to 40
    below its maximum, and a random row shifted by -30."""
    g = torch.Generator(device="cpu").manual_seed(100 + n)
    s = (torch.randn(6, n, generator=g) * 5).clamp(-20, 20)
    s[2, n - 1] = s[2].max() + 3
    s[3] = 1.75
    s[4] = torch.linspace(0, -40, n) if n > 1 else 0.0
    s[5] -= 30
    return (s * 256).round() / 256


@pytest.mark.parametrize("n", [1, 77, 255, 256, 257, 1000])
def test_softmax_rows_per_element(ops, dev, n):
    s = _softmax_rows_input(n)
    ref = torch.softmax(s.double(), -1)
    out = ops.softmax_rows(s.to(dev)).cpu()
    assert out.dtype == torch.float16
    # fp16 output: half an ulp (2^-11 relative) plus the fast exp (below 2^-17 at arguments down to -40: the fp32 rounding of
    # x * log2(e), 58 * 2^-24 * ln 2) where ref is a normal fp16 value; below that the spacing is 2^-24 and half of it suffices
    tol = torch.where(ref >= 2.0 ** -14, ref * 2.0 ** -10, torch.full_like(ref, 2.0 ** -24))
    err = (out.double() - ref).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), "fp16, n=%d: %d elements, first (row, col) %s: got %g, expected %g" % (
        n, int(bad.sum()), bad.nonzero()[0].tolist(), out[tuple(bad.nonzero()[0])].item(), ref[tuple(bad.nonzero()[0])].item())
    for scale in (1.0, 0.5):     # powers of two: scale * x is exact, the reference is softmax of the same numbers
        ref = torch.softmax(s.double() * scale, -1)
        out = ops.softmax_rows_f32(s.to(dev), scale=scale).cpu()
        assert out.dtype == torch.float32
        # fp32 output: the fast exp's argument (half an ulp of x * log2(e) plus the rounding of that constant: below 2^-18 relative
        # at |x| <= 43), one ulp of exp2, of the reciprocal and of the product and a few of the row sum (2^-24 each) stay below
        # 2^-17 relative; 2^-126 is the smallest normal fp32 value
        err = (out.double() - ref).abs()
        bad = ~(err <= ref * 2.0 ** -17 + 2.0 ** -126)
        assert not bool(bad.any()), "fp32, n=%d, scale %g: %d elements, first (row, col) %s: got %g, expected %g" % (
            n, scale, int(bad.sum()), bad.nonzero()[0].tolist(), out[tuple(bad.nonzero()[0])].item(), ref[tuple(bad.nonzero()[0])].item())


# ---- attn_fwd_kernel<40, 8>: the serial 8-wave loop behind VD_ATTN_PIPE=0 (read once per process: a fresh child; last in the module) ----

def test_attn_fwd_kernel_8_waves_in_a_child_process():
    """The two attn_pipe_kernel shapes on attn_fwd_kernel<40, 8> (256 queries per block), every operand family, under the same
    acceptance rule: tests/exact_attention_child.py in one fresh interpreter with VD_ATTN_PIPE=0."""
    env = dict(os.environ, VD_ATTN_PIPE="0")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "exact_attention_child.py")
    r = subprocess.run([sys.executable, child], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300,
                       universal_newlines=True)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout and "all cases pass" in r.stdout, "exit status %d\n%s" % (r.returncode, r.stdout[-6000:])
