"""LoRA adapters restated for the tests: a numpy emulator of vd_lora_merge's rounding contract (include/vd_hip.h), the float64
statement base + sum_a s_a up_a down_a, a per-element bound counted from the contract's roundings, operand generators whose sums are
exact in every order, and builders of adapters for the tiny model.  Shared by the CPU and the GPU tests; imports neither torch.cuda
nor the kernel library."""
import collections

import numpy as np
import torch

# (N, K, ranks) of the kernel cases
#   (5, 7, [1])                  everything is tail
#   (64, 36, [4])                the input conv's 4 * 3 * 3: K % 4 == 0 but one tile
#   (130, 129, [33, 1, 16])      three terms, ragged in both dimensions, a rank across the chunk boundary (32)
#   (128, 576, [8])              a 3x3 conv of the tiny UNet
EXACT_CASES = [(5, 7, [1]), (64, 36, [4]), (130, 129, [33, 1, 16]), (128, 576, [8])]
RANDOM_CASES = [(130, 129, [33, 1, 16]), (128, 576, [8])]
TIE_SHARE = 1e-6                  # the share of elements that may differ from the emulator by its double-rounding ties

FWD_TOL = 5e-3                    # tests/test_parity_gpu.py:18, the bound of the tiny forward against the oracle
ADAPTER_SCALE = 0.75              # the strength of the model tests
ADAPTER_RANK = 4
ADAPTER_AMP = 0.2                 # the standard deviation of up and of down; tests/test_lora_cpu.py shows that it moves the model


# ---- the contract ----------------------------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in float64 and the sum is rounded to float64 first; the double
    rounding differs from fmaf only when that sum sits within 2^-53 of an fp32 tie (tests/apg_cases.py's emulator)."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def scale32(s):
    return np.float32(s)


def emulate(base, terms):
    """The contract, operation by operation: base fp32 or fp16 [N, K], terms a list of (up fp32 [N, r], down fp32 [r, K], scale).
    Returns an array of base's dtype."""
    base = np.asarray(base)
    assert base.dtype in (np.float32, np.float16)
    acc = base.astype(np.float32)
    for up, down, s in terms:
        up, down = np.asarray(up, np.float32), np.asarray(down, np.float32)
        d = np.zeros(acc.shape, np.float32)
        for j in range(up.shape[1]):
            d = fma32(up[:, j:j + 1], down[j:j + 1, :], d)
        acc = fma32(scale32(s), d, acc)
    return acc if base.dtype == np.float32 else acc.astype(np.float16)       # numpy rounds fp32 -> fp16 to nearest even, once


def statement64(base, terms):
    """base + sum_a s_a up_a down_a in float64, s_a the fp32 scale the kernel reads."""
    ref = np.asarray(base).astype(np.float64)
    for up, down, s in terms:
        ref = ref + float(scale32(s)) * (np.asarray(up, np.float64) @ np.asarray(down, np.float64))
    return ref


def ulp16(a):
    """The spacing of fp16 at |a| (float64 array); subnormals: 2^-24."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    return 2.0 ** (np.maximum(np.floor(np.log2(np.maximum(a, 2.0 ** -14))), -14) - 10)


def bound(base, terms, out_f16):
    """Per element, how far the contract's result may lie from statement64, counted from its roundings.  With A_a = |up_a| |down_a|
    (the sum of the magnitudes of term a's products, which no partial sum of the chain exceeds) and M_a = |base| + sum_{b <= a}
    |s_b| A_b (which no value of acc exceeds up to term a):
      d = fmaf(u, w, d)      r_a roundings per term, each at most 2^-24 of the running |d| <= A_a; carried into acc times |s_a|:
                             |s_a| r_a 2^-24 A_a
      acc = fmaf(s, d, acc)  one rounding per term, at most 2^-24 of the new |acc| <= M_a:   2^-24 M_a
    that is r_a + 1 roundings per term.  The rounded partial sums can exceed A_a and M_a by the errors already made, a factor of at
    most (1 + 2^-24)^(8 * 257) < 1 + 2^-12 on every line: the total is scaled by it.  fp16 output: half a unit in the last place of
    fp16 at |statement| + the fp32 error, a rounding of its own."""
    mag = np.abs(np.asarray(base).astype(np.float64))
    err = np.zeros_like(mag)
    for up, down, s in terms:
        a = np.abs(np.asarray(up, np.float64)) @ np.abs(np.asarray(down, np.float64))
        sa = abs(float(scale32(s)))
        mag = mag + sa * a
        err = err + 2.0 ** -24 * (sa * up.shape[1] * a + mag)
    err = err * (1.0 + 2.0 ** -12)
    if out_f16:
        err = err + 0.5 * ulp16(np.abs(statement64(base, terms)) + err)
    return err


# ---- operands whose sums are exact in every order ----------------------------------------------------------------------------------

Q_UP, Q_DOWN, Q_SCALE, Q_BASE = 1.0, 0.5, 0.5, 0.25       # every operand is an integer multiple of its quantum


def exact_operands(N, K, ranks, f16, seed):
    """(base, terms) of small integers times powers of two: up in {-2, -1, 1, 2}, down in {-1, -0.5, 0.5, 1} (no zeros: a rank-1
    term moves every element), scale a multiple of 0.5 of magnitude <= 2, base a multiple of 0.25 of magnitude <= 4.  check_exact
    (called here) proves in float64 that EVERY partial sum of base and the products s u w, in every order and grouping, is exactly
    representable in fp32 -- and in fp16 when the output is fp16 -- so a kernel that keeps to fp32 fma / add / mul in ANY order must give statement64 bit for bit, and the
    comparison does not depend on how an emulator breaks ties."""
    rs = np.random.RandomState(seed)
    base = (rs.randint(-16, 17, size=(N, K)) * Q_BASE).astype(np.float16 if f16 else np.float32)
    scales = [0.5, -1.5, 2.0, -0.5, 1.0, 1.5, -2.0, -1.0]
    terms = []
    for a, r in enumerate(ranks):
        up = (rs.choice([-2, -1, 1, 2], size=(N, r)) * Q_UP).astype(np.float32)
        down = (rs.choice([-2, -1, 1, 2], size=(r, K)) * Q_DOWN).astype(np.float32)
        terms.append((up, down, scales[a % len(scales)]))
    check_exact(base, terms, f16)
    return base, terms


def check_exact(base, terms, f16):
    """The proof obligation of exact_operands, in float64 (every quantity below is a small dyadic number: float64 holds it exactly).
    All summands -- base and every product s u w -- are integer multiples of q = Q_SCALE Q_UP Q_DOWN (Q_BASE is a multiple of q
    too), so every partial sum in every order is a multiple of q whose magnitude is at most S = |base| + sum |s u w|.  A multiple of
    q below 2^p q has at most p significant bits: p = 24 makes it an fp32 value, p = 11 an fp16 value (q >= 2^-24 and S < 65504
    keep it in fp16's range).  The partial sums of the d chain, u w without s, are multiples of Q_UP Q_DOWN bounded by A the same
    way."""
    q = Q_SCALE * Q_UP * Q_DOWN
    b = np.asarray(base).astype(np.float64)
    assert np.array_equal(b / q, np.round(b / q))
    S = np.abs(b)
    for up, down, s in terms:
        u, w, sf = np.asarray(up, np.float64), np.asarray(down, np.float64), float(s)
        assert float(scale32(s)) == sf
        for v, qq in ((u, Q_UP), (w, Q_DOWN), (np.array([sf]), Q_SCALE)):
            assert np.array_equal(v / qq, np.round(v / qq))
        A = np.abs(u) @ np.abs(w)
        assert float(A.max()) / (Q_UP * Q_DOWN) < 2.0 ** (11 if f16 else 24)
        S = S + abs(sf) * A
    assert float(S.max()) / q < 2.0 ** (11 if f16 else 24), float(S.max()) / q
    if f16:
        assert q >= 2.0 ** -24 and float(S.max()) < 65504.0
    ref = statement64(base, terms)
    assert np.array_equal(ref.astype(np.float16 if f16 else np.float32).astype(np.float64), ref)
    assert float(np.mean(ref == b)) < 0.2, "the terms leave too many elements where they were"
    return ref


def random_operands(N, K, ranks, seed):
    """fp32 operands of order one: base ~ N(0, 1), up and down ~ N(0, 1) / sqrt(r), scales of mixed sign and size."""
    rs = np.random.RandomState(seed)
    base = rs.standard_normal((N, K)).astype(np.float32)
    scales = [0.75, -1.3, 0.31, 1.0, -0.6, 0.2, 1.7, -0.9]
    terms = [((rs.standard_normal((N, r)) / np.sqrt(r)).astype(np.float32), rs.standard_normal((r, K)).astype(np.float32),
              scales[a % len(scales)]) for a, r in enumerate(ranks)]
    return base, terms


# ---- adapters for the tiny model ---------------------------------------------------------------------------------------------------

ATTN = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v")
RES = "diffuser.image.data_blocks.3.0"          # a ResBlock with a skip connection (64 -> 128 channels)


def adapter_paths(net, text_ctx=True):
    """The layers the model tests adapt: in every SpatialTransformer of diffuser.image the attention projections, the GEGLU proj,
    ff.net.2 and the 1x1 convolutions proj_in / proj_out; one ResBlock's two 3x3 convolutions, its skip_connection and its
    emb_layers.1; the attention projections of diffuser.text.context_blocks."""
    mods = dict(net.named_modules())
    paths = []
    for p in mods:
        if p.startswith("diffuser.image.context_blocks.") and p.endswith(".transformer_blocks.0"):
            st = p[:-len(".transformer_blocks.0")]
            paths += [st + ".proj_in"] + [p + "." + a for a in ATTN] + [p + ".ff.net.0.proj", p + ".ff.net.2", st + ".proj_out"]
        if text_ctx and p.startswith("diffuser.text.context_blocks.") and p.endswith(".transformer_blocks.0"):
            paths += [p + "." + a for a in ATTN]
    paths += [RES + ".in_layers.2", RES + ".out_layers.3", RES + ".skip_connection", RES + ".emb_layers.1"]
    assert all(p in mods for p in paths)
    return paths


def make_adapter(net, paths, seed, rank=ADAPTER_RANK, amp=ADAPTER_AMP, alpha=None, form="native", dtype=torch.float32):
    """A dict of tensors in one of the three key forms ("native", "peft", "flat"): up and down ~ N(0, amp^2), seeded per call."""
    g = torch.Generator().manual_seed(seed)
    mods = dict(net.named_modules())
    out = collections.OrderedDict()
    for p in paths:
        w = mods[p].weight
        if w.dim() == 4:
            down = torch.randn((rank,) + tuple(w.shape[1:]), generator=g) * amp
            up = torch.randn((w.shape[0], rank, 1, 1), generator=g) * amp
        else:
            down = torch.randn((rank, w.shape[1]), generator=g) * amp
            up = torch.randn((w.shape[0], rank), generator=g) * amp
        stem = "lora_vd_" + p.replace(".", "_") if form == "flat" else p
        dn, un = (".lora_A.weight", ".lora_B.weight") if form == "peft" else (".lora_down.weight", ".lora_up.weight")
        out[stem + dn], out[stem + un] = down.to(dtype), up.to(dtype)
        if alpha is not None and form != "peft":
            out[stem + ".alpha"] = torch.tensor(float(alpha))
    return out


def pairs_of(tensors):
    """{path: (up [N, r], down [r, K], alpha or None)} of a native-form dict as float64 numpy matrices."""
    out = {}
    for k, v in tensors.items():
        if k.endswith(".lora_down.weight"):
            p = k[:-len(".lora_down.weight")]
            up = tensors[p + ".lora_up.weight"]
            a = tensors.get(p + ".alpha")
            r = v.shape[0]
            out[p] = (up.double().reshape(up.shape[0], r).numpy(), v.double().reshape(r, -1).numpy(), None if a is None else float(a))
    return out


def layer_terms(adapters, path):
    """The kernel-level terms of one layer: adapters a list of (native-form dict, strength, default alpha or None) in attach order.
    Returns [(up fp32, down fp32, scale)] with scale = fp32(strength * alpha / r), formed in float64."""
    terms = []
    for tensors, strength, alpha in adapters:
        pr = pairs_of(tensors)
        if path in pr:
            up, down, a = pr[path]
            r = up.shape[1]
            a = a if a is not None else (alpha if alpha is not None else r)
            terms.append((up.astype(np.float32), down.astype(np.float32), float(np.float32(float(strength) * (float(a) / r)))))
    return terms


def merged_state_dict(sd, adapters):
    """The fp32 state dict the oracle consumes with the adapters merged in: statement64 per layer, rounded once to fp32."""
    out = dict(sd)
    paths = set(p for tensors, _, _ in adapters for p in pairs_of(tensors))
    for p in paths:
        w = sd[p + ".weight"]
        ref = statement64(w.detach().float().reshape(w.shape[0], -1).numpy(), layer_terms(adapters, p))
        out[p + ".weight"] = torch.from_numpy(ref.astype(np.float32)).reshape(w.shape)
    return out
