"""The inputs of the exact attention tests (tests/attn_cases.py), checked without a GPU on the float64 reference alone, and proof
that the acceptance rule (vdtest_util.attn_mismatch) bites.

Why the kernels have no rounding freedom on these operands: every operand is an fp16 value; the probabilities that survive are one
constant P per row (exactly 1 in the kernels whose running maximum is an fp32 value, exp2(s - fp16(m)) in the pipelined one), an
fp16 value of at most 11 significant bits; and in every row the sum of |v| over the keys that carry probability is below
2^13, so every partial sum of O = sum P v stays below 2^24 units of P's last bit: the fp32 accumulation is exact IN ANY ORDER, and so
is the row sum l.  The values a row adds in one channel share a sign (uniform, group), so the result is no smaller than any partial
sum and the last bit of one -- which the losers' remains in the accumulator can cost -- is 2^-23 of it.  What is left is the fp32 reciprocal of l and one fp32 product (<= 2^-24 relative each) and, for the selector
families, the losers' mass, bounded here by 2^-40 -- together far inside the 2^-20 of the rule.
"""
import numpy as np
import pytest
import torch

import attn_cases as A
from vdtest_util import ATTN_AXES, attn_bad, attn_mismatch, fp16_interval

FP16_MIN_NORMAL = 2.0 ** -14


def test_every_family_and_kind_has_cases():
    for fam in A.FAMILIES:
        for kind in ("uniform", "selector"):
            assert A.names(fam, kind), (fam, kind)
    for fam in ("fwd4", "pipe", "wide"):
        assert A.names(fam, "group"), fam


def test_fp16_interval_is_equality_for_fp16_values_and_correct_rounding_otherwise():
    ref = np.array([3.0, -255.0, 1.0 / 3.0, -(2.0 + 2.0 ** -10), 0.0, 2.0 + 2.0 ** -9 + 2.0 ** -10 - 2.0 ** -40])
    lo, hi = fp16_interval(ref)
    assert lo[0] == hi[0] == 3.0 and lo[1] == hi[1] == -255.0 and lo[4] == hi[4] == 0.0
    assert lo[2] == hi[2] == float(np.float16(1.0 / 3.0))
    assert (lo[3], hi[3]) == (-(2.0 + 2.0 ** -9), -2.0)      # an exact tie: either neighbour is a correct rounding within 2^-20
    assert (lo[5], hi[5]) == (2.0 + 2.0 ** -9, 2.0 + 2.0 ** -8)   # 2^-40 below a tie
    out = torch.tensor([3.0, -255.0, 1.0 / 3.0, -2.0, 0.0, 2.0 + 2.0 ** -8]).half()
    assert not attn_bad(out, ref).any()
    out[2] = float(np.nextafter(np.float16(1.0 / 3.0), np.float16(1.0)))
    assert attn_bad(out, ref).tolist() == [False, False, True, False, False, False]
    assert attn_bad(torch.tensor([float("nan")]), np.array([1.0])).all()


def _bh(x, c):   # [B, N, H * D] -> [B * H, N, D] float64
    B, H, D = c["B"], c["H"], c["D"]
    return x.double().view(B, -1, H, D).permute(0, 2, 1, 3).reshape(B * H, -1, D)


@pytest.mark.parametrize("name", list(A.CASES))
def test_case_preconditions(name):
    t = A.build(name)
    c = t.case
    B, H, D, Nq, Nk = c["B"], c["H"], c["D"], c["Nq"], c["Nk"]
    for op in ("q", "k", "v") + (("x", "wq", "w_fold") if c["family"] == "xattn" else ()):
        x = getattr(t, op)
        assert x.dtype == torch.float16 and bool(torch.isfinite(x).all()), op      # exactly representable: they ARE fp16 values
    assert tuple(t.ref.shape) == (B, Nq, H, D) and t.ref.dtype == torch.float64
    assert t.carried * 2 ** 11 < 2 ** 24, "%s: sum of |v| over the keys that carry probability is %g" % (name, t.carried)
    v = _bh(t.v, c)
    assert bool((v != 0).all()) and torch.equal(v, v.round())
    if c["kind"] == "uniform":
        assert t.max_logit == 0.0                       # q is exactly 0 (for the fused kernel: after LayerNorm and projection)
        assert bool((t.q == 0).all())
        assert v.abs().max().item() <= 16
        assert t.ref.abs().min().item() >= FP16_MIN_NORMAL
        assert not t.cancels and (t.ref - t.selected).abs().max().item() <= 2.0 ** -40
    else:
        assert t.off_mass <= 2.0 ** -40, "%s: mass off the winner %g" % (name, t.off_mass)
        assert 0 < t.max_logit <= 100.0, "%s: largest |logit| %g" % (name, t.max_logit)
        assert bool((t.q.double().abs() == t.g).all())  # also for the fused kernel, whose q is LayerNorm -> projection -> fp16
        assert not t.cancels and t.selected.abs().min().item() >= 1.0     # the v rows a query adds have one sign per channel
        assert ((t.ref - t.selected).abs() < 2.0 ** -24 * t.selected.abs()).all()
        assert v.abs().max().item() <= 255
        if c["kind"] == "selector":
            lo, hi = fp16_interval(t.ref)
            assert np.array_equal(lo, hi) and np.array_equal(lo, t.selected.numpy())   # the rule is bit-for-bit equality
        codes = t.codes.reshape(B * H, Nk, D)
        for i in range(B * H):
            n_ids = len(np.unique(t.cid.reshape(B * H, Nk)[i]))
            assert len(np.unique(codes[i], axis=0)) == n_ids == (Nk if c["kind"] == "selector" else Nk // 3 + Nk % 3)
            assert len(np.unique(v[i].numpy(), axis=0)) == Nk
    # exchanging any two (batch, head) slices of v changes the reference (the probabilities do not depend on v; 64 rows suffice)
    rows = np.unique(np.r_[np.arange(min(Nq, 32)), np.arange(max(Nq - 32, 0), Nq)])
    w = t.win.reshape(B * H, Nq, Nk)[:, rows].double()
    w = w / w.sum(-1, keepdim=True)
    for i in range(B * H):
        own = w[i] @ v[i]
        for j in range(B * H):
            if j != i:
                assert not torch.equal(w[i] @ v[j], own), (name, i, j)


def test_winners_cover_the_tiles_and_both_rescale_orders():
    """Selector winners sit in the first tile, a middle tile and the last ragged tile, key 0 / Nk - 1 / Nk - 33 included, and come
    both before and after the key with the largest loser logit of their row."""
    for name in A.names(kind="selector") + A.names(kind="group"):
        t = A.build(name)
        c = t.case
        Nk = c["Nk"]
        last_tile = ((min(Nk, c["Nq"]) if c["causal"] else Nk) - 1) // 64 * 64      # ... that any row can see
        for p in t.pi.reshape(-1, c["Nq"]):
            if not c["causal"]:
                assert {0, Nk - 1, max(Nk - 33, 0), last_tile}.issubset(set(p.tolist())), name
            assert (p < 64).any() and (p >= last_tile).any()
    t = A.build("pipe_pairs-selector")
    _, P, logits = A.softmax_attention(t.q[:, :256], t.k, t.v, t.case["H"], False)
    top_loser = logits.masked_fill(t.win[:, :, :256], float("-inf")).argmax(-1)
    pi = torch.from_numpy(t.pi[:, :, :256])
    assert bool((top_loser < pi).any()) and bool((top_loser > pi).any())


# ---- the checker bites: faults applied to a plain torch emulation ---------------------------------------------------------------

def _emulate(t, drop_last=False, pad_key=False, diag=None, rotate_tile=None, swap_heads=None, swap_samples=None, swap_slices=None):
    c = t.case
    B, H, D, Nq, Nk = c["B"], c["H"], c["D"], c["Nq"], c["Nk"]
    q = t.q.double().view(B, Nq, H, D).permute(0, 2, 1, 3).clone()
    k = t.k.double().view(B, Nk, H, D).permute(0, 2, 1, 3)
    v = t.v.double().view(B, Nk, H, D).permute(0, 2, 1, 3).clone()
    if swap_slices is not None:      # two waves of the wide kernel exchange their slices of Q (head dim split over four waves)
        a, b = swap_slices
        w = D // 4
        q[..., a * w:(a + 1) * w], q[..., b * w:(b + 1) * w] = q[..., b * w:(b + 1) * w].clone(), q[..., a * w:(a + 1) * w].clone()
    vis = torch.from_numpy(A.visible(Nq, Nk, c["causal"]))[None, None].repeat(B, H, 1, 1)
    if diag is not None:             # the causal diagonal moved by `shift` for one query row
        b, h, i, shift = diag
        vis[b, h, i] = torch.arange(Nk) <= i + shift
    if drop_last:
        vis[..., Nk - 1] = False
    s = (q @ k.transpose(-1, -2) * D ** -0.5).masked_fill(~vis, float("-inf"))
    if rotate_tile is not None:      # P of key j meets v of key j - 4 inside one 64-key tile
        sl = slice(64 * rotate_tile, min(64 * rotate_tile + 64, Nk))
        v[:, :, sl] = torch.roll(v[:, :, sl], 4, 2)
    if pad_key:                      # one key past Nk (K reads as zeros: logit 0, v = 0) escapes the mask
        s = torch.cat([s, torch.zeros(B, H, Nq, 1, dtype=torch.float64)], -1)
        v = torch.cat([v, torch.zeros(B, H, 1, D, dtype=torch.float64)], 2)
    out = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).contiguous()
    if swap_heads is not None:
        out[:, :, list(swap_heads)] = out[:, :, list(swap_heads)[::-1]]
    if swap_samples is not None:
        out[list(swap_samples)] = out[list(swap_samples)[::-1]]
    return torch.from_numpy(out.numpy().astype(np.float16))


def _bad_rows(t, out):
    """set of (batch, query, head) with a failing element, and the report"""
    bad = attn_bad(out, t.ref)
    msg = attn_mismatch(out, t.ref, t.case["name"], win_key=t.pi)
    assert (msg is None) == (not bad.any())
    rows = set(map(tuple, np.argwhere(bad.any(-1)).tolist()))
    if msg is not None:
        idx = np.argwhere(bad)
        assert "%d of %d elements fail" % (idx.shape[0], bad.size) in msg
        assert "extent: " + ", ".join("%s %d..%d" % (n, idx[:, i].min(), idx[:, i].max()) for i, n in enumerate(ATTN_AXES)) in msg
        b, i, h, ch = idx[0].tolist()
        assert "(batch=%d, query=%d, head=%d, channel=%d): got" % (b, i, h, ch) in msg and "selected key %d" % t.pi[b, h, i] in msg
        assert "first failure: query block %d, wave %d" % (i // 128, (i % 128) // 32) in msg
    return rows, msg


REPRESENTATIVE = ["fwd40_ctx_map-uniform", "fwd64_clip-uniform", "fwd64_clip-selector", "fwd80_five_tiles-group", "wide256-selector"]


@pytest.mark.parametrize("name", REPRESENTATIVE)
def test_emulation_without_a_fault_passes(name):
    t = A.build(name)
    assert _bad_rows(t, _emulate(t))[0] == set()


def _rows_where(mask_bhq):   # [B, H, Nq] bool -> set of (batch, query, head)
    return set((b, i, h) for b, h, i in np.argwhere(np.asarray(mask_bhq)).tolist())


@pytest.mark.parametrize("name", REPRESENTATIVE)
def test_fault_last_key_dropped(name):
    """Fails exactly in the rows whose probability reaches the last key (every row of a non-causal uniform case)."""
    t = A.build(name)
    rows, _ = _bad_rows(t, _emulate(t, drop_last=True))
    c = t.case
    sees = torch.from_numpy(A.visible(c["Nq"], c["Nk"], c["causal"]).sum(-1) > 1)      # (a row that sees only that key shows nothing)
    reach = _rows_where(t.win[..., -1] & sees[None, None])
    assert rows and rows <= reach
    if t.case["kind"] != "uniform":
        assert rows == reach


@pytest.mark.parametrize("name", ["fwd40_ctx_map-uniform", "fwd64_clip-uniform"])
def test_fault_padded_key_in_the_row_sum(name):
    """A zero-logit padded key shrinks every mean by n / (n + 1): every row of a uniform case fails.  (Against a selector's
    winner its mass is exp(-70) -- the uniform family is what sees it.)"""
    t = A.build(name)
    c = t.case
    rows, _ = _bad_rows(t, _emulate(t, pad_key=True))
    assert len(rows) == c["B"] * c["Nq"] * c["H"]


@pytest.mark.parametrize("name,shift", [("fwd64_clip-uniform", -1), ("fwd64_clip-uniform", 1), ("fwd64_clip-selector", -1)])
def test_fault_causal_diagonal_off_by_one_in_one_row(name, shift):
    """One query row (a row that selects its own diagonal key in the selector case) sees one key fewer or one more: exactly that
    row fails.  One key more is invisible to a selector (the extra key loses) and is what the uniform prefix mean pins."""
    t = A.build(name)
    b, h, i = 2, 7, 40
    assert t.pi[b, h, i] == i
    rows, msg = _bad_rows(t, _emulate(t, diag=(b, h, i, shift)))
    assert rows == {(b, i, h)}
    assert "batch 2..2, query 40..40, head 7..7" in msg


@pytest.mark.parametrize("name", REPRESENTATIVE[:4])
def test_fault_two_heads_exchanged(name):
    t = A.build(name)
    c = t.case
    rows, msg = _bad_rows(t, _emulate(t, swap_heads=(2, 5)))
    assert {r[2] for r in rows} == {2, 5} and len(rows) == 2 * c["B"] * c["Nq"]
    assert "head 2..5" in msg


@pytest.mark.parametrize("name", REPRESENTATIVE)
def test_fault_two_samples_exchanged(name):
    t = A.build(name)
    c = t.case
    s = (0, c["B"] - 1)
    rows, msg = _bad_rows(t, _emulate(t, swap_samples=s))
    assert {r[0] for r in rows} == set(s) and len(rows) == 2 * c["H"] * c["Nq"]
    assert "batch 0..%d" % s[1] in msg


@pytest.mark.parametrize("name,tile", [("fwd64_clip-selector", 0), ("fwd64_clip-selector", 1), ("fwd80_five_tiles-group", 2),
                                       ("wide256-selector", 5)])
def test_fault_keys_of_one_tile_rotated(name, tile):
    """The keys of one 64-key tile rotated by 4 against their values: exactly the rows with a winner in that tile fail (a uniform
    non-causal mean is invariant under it -- the selector families are what sees it)."""
    t = A.build(name)
    rows, _ = _bad_rows(t, _emulate(t, rotate_tile=tile))
    hit = t.win[..., 64 * tile:64 * tile + 64].any(-1)
    if t.case["causal"]:   # a row that sees the rotated-in value instead of its own
        assert rows and rows <= _rows_where(hit)
    else:
        assert rows == _rows_where(hit)


def test_fault_two_waves_of_the_wide_kernel_exchange_their_slices():
    """attn_wide_kernel splits the head dim over four waves; the codes span all of D, so exchanging the Q slices of two waves moves
    the winner."""
    t = A.build("wide256-selector")
    rows, msg = _bad_rows(t, _emulate(t, swap_slices=(1, 3)))
    c = t.case
    assert len(rows) > 0.4 * c["B"] * c["Nq"]     # (a winner that is a decoy of a quarter the exchange leaves alone keeps its lead)
    m = attn_mismatch(_emulate(t, swap_slices=(1, 3)), t.ref, "wide", win_key=t.pi, qblock=32, wave_cols=c["D"] // 4)
    i, ch = [(r[1], r[3]) for r in np.argwhere(attn_bad(_emulate(t, swap_slices=(1, 3)), t.ref)).tolist()][0]
    assert "first failure: query block %d, wave %d" % (i // 32, ch // 64) in m


def test_print_summary(capsys):
    """The largest |logit| and the largest mass off the winner per kernel family (shown with -s)."""
    with capsys.disabled():
        for fam in A.FAMILIES:
            ts = [A.build(n) for n in A.names(fam) if A.CASES[n]["kind"] != "uniform"]
            print("\n%-6s largest |logit| %.2f, largest mass off the winner %.3g (2^%.1f), largest carried sum of |v| %d"
                  % (fam, max(t.max_logit for t in ts), max(t.off_mass for t in ts), np.log2(max(t.off_mass for t in ts)),
                     max(A.build(n).carried for n in A.names(fam))), end="")
        print()
