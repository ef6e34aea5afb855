"""Shared helpers for the parity tests (test infrastructure)."""
import contextlib
import json
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_gold(name):
    return {k: v for k, v in np.load(os.path.join(GOLD, name), allow_pickle=False).items()}


def meta():
    with open(os.path.join(GOLD, "meta.json")) as f:
        return json.load(f)


def rel_l2(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def tiny_vd_cfg(m=None):
    from lib.cfg_helper import CfgDict
    m = meta() if m is None else m
    return CfgDict(type="vd_v2_0", args=CfgDict(
        vae_cfg_list=[["image", CfgDict(type="autoencoderkl", args=m["vae"])]],
        ctx_cfg_list=[["image", "ctx-image-placeholder"], ["text", "ctx-text-placeholder"]],
        diffuser_cfg_list=[["image", CfgDict(type="openai_unet_2d_next", args=m["unet2d"])],
                           ["text", CfgDict(type="openai_unet_0d_next", args=m["unet0d"])]],
        global_layer_ptr="image", latent_scale_factor={"image": 0.18215}, beta_linear_start=0.00085,
        beta_linear_end=0.012, timesteps=1000, use_ema=False))


def full_vd_cfg(with_vae=True):
    """vd_four_flow_v1-0 with the CLIP / Optimus entries replaced by string placeholders (keeps the test light)."""
    from lib.cfg_helper import CfgDict, model_cfg_bank
    bank = model_cfg_bank()
    vae = [["image", bank("autokl_v1")]] if with_vae else []
    for _, c in vae:
        c.pop("pth", None)
    return CfgDict(type="vd_v2_0", args=CfgDict(
        vae_cfg_list=vae, ctx_cfg_list=[["image", "ctx-image-placeholder"], ["text", "ctx-text-placeholder"]],
        diffuser_cfg_list=[["image", bank("openai_unet_2d_v1")], ["text", bank("openai_unet_0d_v1_c")]],
        global_layer_ptr="image", latent_scale_factor={"image": 0.18215}, beta_linear_start=0.00085,
        beta_linear_end=0.012, timesteps=1000, use_ema=False))


def synth_into(net, seed):
    """Load the deterministic synthetic weights (oracle/synth.py) into a product model; returns the fp32 state dict
    the oracle consumes."""
    from oracle import synth
    shapes = synth.shapes_of(net)
    sd = synth.synth_state_dict(shapes, seed)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected
    full = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    full.update(sd)
    return full


# ---- race amplifier of the stream-ordering tests -------------------------------------------------------------------------------
_DELAY = {}


def _elapsed_ms(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def gpu_delay(target_ms=30.0):
    """(fn, ms): fn enqueues a harmless kernel of about target_ms on the current stream (torch.cuda._sleep, a bounded spin),
    calibrated once per process with CUDA events; ms is what the calibrated delay measured.  Asserts 20 <= ms <= 50, so a test
    built on it cannot go vacuous."""
    import torch
    if "fn" not in _DELAY:
        torch.cuda._sleep(1000)
        cycles = [1 << 20]
        fn = lambda: torch.cuda._sleep(cycles[0])
        ms = _elapsed_ms(fn)
        assert ms > 0.05, "torch.cuda._sleep does not spin on this device (%.4f ms)" % ms
        for _ in range(2):   # linear in the cycle count; the second pass absorbs the launch overhead of the probe
            cycles[0] = max(1, int(cycles[0] * target_ms / ms))
            ms = _elapsed_ms(fn)
        _DELAY.update(fn=fn, ms=ms)
    assert 20.0 <= _DELAY["ms"] <= 50.0, "race amplifier delay measured %.2f ms" % _DELAY["ms"]
    return _DELAY["fn"], _DELAY["ms"]


class _Amp(object):
    ms = 0.0
    builds = 0


@contextlib.contextmanager
def delayed_pack_builds(target_ms=30.0):
    """Race amplifier: while active, every weight-pack build (a cache miss of hip_layers.PackCache._packed) first enqueues a
    ~target_ms kernel on the current stream.  A branch on another stream that reads a freshly built pack without waiting for
    the building stream then reads allocated but unwritten memory -- wrong values on every run, never a fault (packs are
    weights and biases: no kernel uses them as addresses or indices).  Yields a record with the measured delay (.ms) and the
    number of delayed builds (.builds)."""
    from lib.model_zoo import hip_layers
    delay, ms = gpu_delay(target_ms)
    real = hip_layers.PackCache._packed
    amp = _Amp()
    amp.ms = ms

    def _packed(self, key, tensors, fn):
        def slow():
            amp.builds += 1
            delay()
            return fn()
        return real(self, key, tensors, slow)

    hip_layers.PackCache._packed = _packed
    try:
        yield amp
    finally:
        hip_layers.PackCache._packed = real


def unet_middle(unet):
    """(ResBlock, SpatialTransformer) of the middle block of a UNetModel2D_Next: the lowest level, inside the half-batch
    fork region at every geometry that has one."""
    d, c = unet.i_order.count("d"), unet.i_order.count("c")
    return unet.data_blocks[d][0], unet.context_blocks[c][0]


def clear_pack_caches(net):
    for m in net.modules():
        m.__dict__.pop("_vd_pack_cache", None)


# ---- inputs of the differential tests against the reference (oracle/gen_golden_ref_dumps.py stores its outputs) ----
STATE_DICT_MODELS = ["openai_unet_2d_v1", "openai_unet_0d_v1_dc", "openai_unet_0d_v1_c", "autokl_v1", "optimus_bert_encoder",
                     "optimus_gpt2_decoder"]
SCHEDULE_GRID = {"steps": list(range(1, 121)) + [200, 250, 500, 1000], "etas": [0.0, 0.25, 1.0], "methods": ["uniform", "quad"],
                 "schedules": [["linear", 1000, 0.00085, 0.012], ["linear", 1000, 1e-4, 2e-2], ["linear", 250, 0.0015, 0.0195],
                               ["cosine", 1000, 1e-4, 2e-2], ["sqrt_linear", 1000, 1e-4, 2e-2], ["sqrt", 1000, 1e-4, 2e-2]]}


def random_tokenizer_texts():
    """300 seeded random strings (ASCII words, digits, punctuation runs, accents, CJK, emoji, odd whitespace, control
    characters, contractions) + a few edge cases; whitespace-only input dropped (documented difference)."""
    import random
    rnd = random.Random(20260924)
    words = ["the", "a", "Photo", "of", "cat", "sitting", "don't", "it's", "I'm", "we've", "they're", "can not", "do not",
             "unaffable", "naïve", "café", "São", "Zürich", "山", "水", "画", "日本語", "☕", "🙂", "12:30", "3.14", "#42", "e-mail",
             "U.S.A.", "o'keeffe", "(oil)", "[x]", "{y}", "a/b", "50%", "$5", "x_y", "--", "...", "?!", "\t", "\n", "\u00a0", "\u2009",
             "\x07", "\ufffd", "Ωmega", "straße", "İstanbul", "supercalifragilisticexpialidocious", "aaaaaaaaaa" * 11]
    seps = [" ", " ", " ", "  ", ", ", ". ", "! ", "\t", "\n", "", "-", "' "]
    texts = []
    for _ in range(300):
        n = rnd.randint(1, 9)
        t = ""
        for _ in range(n):
            t += rnd.choice(words) + rnd.choice(seps)
        texts.append(t.strip() if rnd.random() < 0.5 else t)
    texts += ["", " ", "a", "A", ".", "hello world", "Hello, World!"]
    return [t for t in texts if t.strip()]


def published_vocab_files(tmp_dir):
    """The published GPT-2 vocabulary / merges and BERT vocabulary restricted to the entries the tokenizer fixtures use
    (tests/golden/optimus_vocab_subset.json.gz), every other id a placeholder: (gpt2 vocab, gpt2 merges, bert vocab) paths.
    Same results on those texts as the full files: BPE applies the lowest-ranked merge present, and every merge it
    applies is kept in its published order; WordPiece takes the longest piece present, and every piece it takes is kept."""
    sub = load_ref_json("optimus_vocab_subset.json.gz")
    g = sub["gpt2"]
    vocab = {"[unused-%d]" % i: i for i in range(g["len"])}
    for i in set(g["tokens"].values()) | {g["unk"][1]}:
        vocab.pop("[unused-%d]" % i)
    vocab.update(g["tokens"])
    vocab[g["unk"][0]] = g["unk"][1]
    assert len(vocab) == g["len"]
    paths = [os.path.join(str(tmp_dir), n) for n in ("gpt2-vocab.json", "gpt2-merges.txt", "bert-base-cased-vocab.txt")]
    with open(paths[0], "w", encoding="utf-8") as f:
        json.dump(vocab, f, ensure_ascii=False)
    with open(paths[1], "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(g["merges"]) + "\n")
    b = sub["bert"]
    lines = ["[unused-%d]" % i for i in range(b["len"])]
    for piece, i in b["pieces"].items():
        lines[i] = piece
    with open(paths[2], "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return paths


def live_case_inputs(d, k):
    """Inputs of case k of oracle/ref_live_cases.py, drawn again from the seeds it uses (the fixture holds the reference's
    outputs, the geometry and the timesteps only)."""
    from oracle.gen_golden import seeded
    B, H, W, Lt, Li, Hi, Wi = [int(v) for v in d["%d_dims" % k]]
    return {"x": seeded((B, 4, H, W), 100 + k), "ct": seeded((B, Lt, 128), 200 + k, 0.5), "ci": seeded((B, Li, 128), 300 + k, 0.5),
            "ut": seeded((1, Lt, 128), 400 + k, 0.5).repeat(B, 1, 1), "xT": seeded((B, 4, H, W), 500 + k),
            "img": torch.rand((B, 3, Hi, Wi), generator=torch.Generator().manual_seed(600 + k)),
            "zl": seeded((B, 4, Hi // 2, Wi // 2), 700 + k), "x0d": seeded((B, 128), 800 + k)}


def fullwidth_inputs():
    """Inputs of oracle/ref_live_fullwidth.py, drawn again from the seeds it uses."""
    from oracle.gen_golden import seeded
    B, H, W = 2, 16, 16
    return {"x": seeded((B, 4, H, W), 1), "ct": seeded((B, 77, 768), 2, 0.5), "ci": seeded((B, 257, 768), 3, 0.5),
            "x0d": seeded((B, 768), 4), "ut": seeded((1, 77, 768), 5, 0.5).repeat(B, 1, 1), "xT": seeded((B, 4, H, W), 6)}


def exact_digest(arrays):
    """SHA-256 over dtype, shape and bytes of each array in turn: what the schedule fixture stores for bit-exact arrays."""
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        a = np.asarray(a)
        h.update(("%s%s" % (a.dtype, list(a.shape))).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def load_ref_json(name):
    """A gzip-compressed JSON dump of the reference's own code (oracle/gen_golden_ref_dumps.py)."""
    import gzip
    with gzip.open(os.path.join(GOLD, name), "rt", encoding="utf-8") as f:
        return json.load(f)


# ---- exact (tolerance-free) checks of the linear kernels: tests/exact_cases.py holds the case table --------------------
EXACT_LIMIT = 2048        # fp16 holds every integer of magnitude <= 2048
EXACT_ZERO_SHARE = 0.15   # a reference with more zeros than this says little about dropped terms


def exact_operand(shape, seed):
    """fp16 values drawn from {-1, 0, 0, +1} with equal weight on the four slots, seeded on the CPU.  Products and partial sums of
    such operands are integers in any order, so fp32 accumulation, fp32 split-K slabs and the final fp16 rounding are all exact."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    slots = torch.tensor([-1.0, 0.0, 0.0, 1.0])
    return slots[torch.randint(0, 4, tuple(shape), generator=g)].half()


def exact_ints(shape, seed, lo=-8, hi=8):
    """fp16 integers in [lo, hi] (bias, row vector, residual of the exact tests), seeded on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).half()


def check_exact_reference(ref, unit=1.0, what=""):
    """The preconditions of an exact comparison: every reference output is a multiple of `unit` (1: an integer; a power of two
    below 1 for the fp32 outputs scaled by alpha) of magnitude <= 2048, and fewer than 15 % of them are zero."""
    ref = torch.as_tensor(ref).double()
    q = ref / unit
    assert torch.equal(q, q.round()), "%s: reference is not a multiple of %g" % (what, unit)
    peak = ref.abs().max().item()
    assert peak <= EXACT_LIMIT, "%s: |reference| reaches %g > %d" % (what, peak, EXACT_LIMIT)
    zeros = (ref == 0).double().mean().item()
    assert zeros < EXACT_ZERO_SHARE, "%s: %.1f %% of the reference is zero (change the seed, not the cap)" % (what, 100 * zeros)
    return peak, zeros


def exact_mismatch(out, ref, names, context="", limit=6):
    """None when `out` equals the float64 reference in every element, else a report: the number of mismatching elements, the
    first `limit` coordinates (named by `names`, e.g. ("row", "col") or ("image", "y", "x", "channel")) with got / expected, the
    extent of the mismatching region per axis, and `context` (the active override, variant or split)."""
    got = torch.as_tensor(out).detach().double().cpu()
    ref = torch.as_tensor(ref).double()
    if tuple(got.shape) != tuple(ref.shape):
        return "%s: shape %s, expected %s" % (context, tuple(got.shape), tuple(ref.shape))
    if torch.equal(got, ref):
        return None
    bad = (got != ref) | torch.isnan(got)
    idx = bad.nonzero()
    lines = ["%s: %d of %d elements differ" % (context, idx.shape[0], ref.numel())]
    lines.append("  extent: " + ", ".join("%s %d..%d" % (n, idx[:, i].min().item(), idx[:, i].max().item()) for i, n in enumerate(names)))
    for c in idx[:limit].tolist():
        where = ", ".join("%s=%d" % (n, v) for n, v in zip(names, c))
        lines.append("  (%s): got %g, expected %g" % (where, got[tuple(c)].item(), ref[tuple(c)].item()))
    return "\n".join(lines)


def assert_exact(out, ref, names, context=""):
    msg = exact_mismatch(out, ref, names, context)
    assert msg is None, msg


# ---- per-element checks of the attention kernels: tests/attn_cases.py holds the case table --------------------------------------
ATTN_REL = 2.0 ** -20     # the kernels' inexact steps are the fp32 1 / l and one fp32 product (<= 2^-24 each); eightfold margin
ATTN_AXES = ("batch", "query", "head", "channel")


def fp16_interval(ref, rel=ATTN_REL):
    """(lo, hi) float64 arrays: the fp16 values of ref * (1 - rel) and ref * (1 + rel), smaller first (numpy rounds float64 to
    fp16 directly, to nearest even).  Where `ref` is itself an fp16 value the interval is that value alone."""
    r = np.asarray(torch.as_tensor(ref).detach().double().cpu().numpy(), np.float64)
    a = (r * (1.0 - rel)).astype(np.float16).astype(np.float64)
    b = (r * (1.0 + rel)).astype(np.float16).astype(np.float64)
    return np.minimum(a, b), np.maximum(a, b)


def attn_bad(out, ref, rel=ATTN_REL):
    """bool array: the elements of `out` outside fp16_interval(ref, rel), NaN included."""
    got = torch.as_tensor(out).detach().double().cpu().numpy()
    lo, hi = fp16_interval(ref, rel)
    return ~((got >= lo) & (got <= hi))


def attn_mismatch(out, ref, context="", rel=ATTN_REL, win_key=None, qblock=128, wave_rows=32, wave_cols=None, limit=6):
    """The acceptance rule of the exact attention tests on [batch, query, head, channel] arrays: an element passes if it lies
    between fp16(ref * (1 - rel)) and fp16(ref * (1 + rel)) inclusive -- bit-for-bit equality where `ref` is an fp16 value,
    "correctly rounded" otherwise.  None when every element passes, else a report: the number of failing elements, their extent
    per axis, the first `limit` coordinates with got / expected and the selected key (win_key [batch, head, query], if given), and
    the query block and wave of the first failure: query // qblock and (query % qblock) // wave_rows, or channel // wave_cols for
    a kernel that splits the head dim over its waves."""
    got = torch.as_tensor(out).detach().double().cpu().numpy()
    refn = torch.as_tensor(ref).detach().double().cpu().numpy()
    if got.shape != refn.shape:
        return "%s: shape %s, expected %s" % (context, got.shape, refn.shape)
    bad = attn_bad(got, refn, rel)
    if not bad.any():
        return None
    idx = np.argwhere(bad)
    lo, hi = fp16_interval(refn, rel)
    lines = ["%s: %d of %d elements fail" % (context, idx.shape[0], refn.size)]
    lines.append("  extent: " + ", ".join("%s %d..%d" % (n, idx[:, i].min(), idx[:, i].max()) for i, n in enumerate(ATTN_AXES)))
    b, i, h, c = [int(x) for x in idx[0]]
    wave = c // wave_cols if wave_cols else (i % qblock) // wave_rows
    lines.append("  first failure: query block %d, wave %d" % (i // qblock, wave))
    for b, i, h, c in idx[:limit].tolist():
        sel = "" if win_key is None else ", selected key %d" % int(win_key[b][h][i])
        want = "%.10g" % refn[b, i, h, c] if lo[b, i, h, c] == hi[b, i, h, c] else "%.10g (fp16 %g..%g)" % (refn[b, i, h, c], lo[b, i, h, c], hi[b, i, h, c])
        lines.append("  (batch=%d, query=%d, head=%d, channel=%d): got %g, expected %s%s" % (b, i, h, c, got[b, i, h, c], want, sel))
    return "\n".join(lines)


# ---- per-element checks of the fused epilogues: tests/epilogue_cases.py holds the case table -------------------------------------
def fp16_steps(lo, hi):
    """How many fp16 steps lie between the fp16-valued arrays lo <= hi (0: the same value; +-0 count as one value)."""
    def key(v):
        bits = np.asarray(v, np.float16).view(np.int16).astype(np.int64)
        return np.where(bits < 0, -(bits & 0x7fff), bits)
    return key(hi) - key(lo)


def interval_mismatch(out, lo, hi, names, context="", limit=6):
    """The acceptance rule of the interval cases: the value a kernel rounds to fp16 is known to lie between two ADJACENT fp16 values
    (or on one), and `lo` / `hi` are those two values carried through the roundings that follow (a residual add).  An element of
    `out` passes if it equals lo or hi -- where no rounding follows that is every fp16 value of the interval.  None when every
    element passes, else a report in the form of exact_mismatch: count, extent per axis, the first `limit` coordinates."""
    got = torch.as_tensor(out).detach().double().cpu().numpy()
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if got.shape != lo.shape:
        return "%s: shape %s, expected %s" % (context, got.shape, lo.shape)
    bad = ~((got == lo) | (got == hi))
    if not bad.any():
        return None
    idx = np.argwhere(bad)
    lines = ["%s: %d of %d elements fail" % (context, idx.shape[0], lo.size)]
    lines.append("  extent: " + ", ".join("%s %d..%d" % (n, idx[:, i].min(), idx[:, i].max()) for i, n in enumerate(names)))
    for c in idx[:limit].tolist():
        where = ", ".join("%s=%d" % (n, v) for n, v in zip(names, c))
        k = tuple(c)
        want = "%.10g" % lo[k] if lo[k] == hi[k] else "%.10g or %.10g" % (lo[k], hi[k])
        lines.append("  (%s): got %.10g, expected %s" % (where, got[k], want))
    return "\n".join(lines)
