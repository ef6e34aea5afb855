"""LoRA adapters without a GPU: the parser (three key forms, alpha precedence, conv reshapes, every ValueError), the file round trip,
the self-check of the exact-sum generators and of the counted bound, the entry's declaration and argument checks, and the
precondition of the GPU parity test: the adapted tiny model differs from the base model by far more than the parity bound."""
import numpy as np
import pytest
import torch

import lora_cases as lc
from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg


@pytest.fixture(scope="module")
def tiny_cpu():
    """The tiny product model on the CPU (never run) and its fp32 weights."""
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    return net, synth_into(net, m["seed"])


@pytest.fixture()
def clean(tiny_cpu):
    from lib.model_zoo import lora
    net = tiny_cpu[0]
    lora.reset(net)
    yield net
    lora.reset(net)


LIN = "diffuser.image.context_blocks.1.0.transformer_blocks.0.attn2.to_k"       # Linear 128 <- 128
CONV3 = "diffuser.image.data_blocks.3.0.in_layers.2"                              # Conv2d 128 <- 64, 3x3
CONV1 = "diffuser.image.context_blocks.1.0.proj_in"                               # Conv2d 128 <- 128, 1x1
VAE = "vae.image.decoder.mid.block_1.conv1"


# ---- 1. the parser -------------------------------------------------------------------------------------------------------------------

def test_three_key_forms_resolve_to_the_same_plan(clean):
    from lib.model_zoo import lora
    net = clean
    paths = lc.adapter_paths(net) + [VAE]
    plans = [lora.parse(net, lc.make_adapter(net, paths, 5, form=form)) for form in ("native", "peft", "flat")]
    assert list(plans[0]) == [p for p in dict(net.named_modules()) if p in set(paths)]       # every path, in the model's order
    for other in plans[1:]:
        assert list(other) == list(plans[0])
        for p in other:
            assert torch.equal(other[p][0], plans[0][p][0]) and torch.equal(other[p][1], plans[0][p][1]) and other[p][2] == plans[0][p][2]
    up, down, factor = plans[0][LIN]
    assert up.shape == (128, lc.ADAPTER_RANK) and down.shape == (lc.ADAPTER_RANK, 128) and factor == 1.0       # alpha defaults to r
    assert up.dtype == down.dtype == torch.float32 and up.is_contiguous() and down.is_contiguous()


def test_alpha_precedence_file_then_argument_then_rank(clean):
    from lib.model_zoo import lora
    net = clean
    r = lc.ADAPTER_RANK
    with_alpha = lc.make_adapter(net, [LIN, CONV3], 6, alpha=2.0)
    without = lc.make_adapter(net, [LIN, CONV3], 6)
    assert lora.parse(net, with_alpha, alpha=16.0)[LIN][2] == 2.0 / r           # the file's alpha wins
    assert lora.parse(net, without, alpha=16.0)[LIN][2] == 16.0 / r             # else the argument
    assert lora.parse(net, without)[CONV3][2] == 1.0                            # else r
    mixed = dict(without)
    mixed[LIN + ".alpha"] = torch.tensor([8.0], dtype=torch.float16)            # per layer, any float dtype, one element
    plan = lora.parse(net, mixed, alpha=16.0)
    assert plan[LIN][2] == 8.0 / r and plan[CONV3][2] == 16.0 / r
    # the term's scale: strength * alpha / r in float64, rounded to fp32 once
    assert lora.term_scale(0.3, 2.0 / 3.0) == float(np.float32(0.3 * (2.0 / 3.0)))


def test_conv_reshapes_and_widening(clean):
    from lib.model_zoo import lora
    net = clean
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        ad = lc.make_adapter(net, [CONV3, CONV1], 7, dtype=dtype)
        plan = lora.parse(net, ad)
        up, down, _ = plan[CONV3]
        assert up.shape == (128, lc.ADAPTER_RANK) and down.shape == (lc.ADAPTER_RANK, 64 * 9)
        src_d, src_u = ad[CONV3 + ".lora_down.weight"], ad[CONV3 + ".lora_up.weight"]
        assert torch.equal(down.double(), src_d.double().reshape(lc.ADAPTER_RANK, -1))        # [r, Cin kh kw], widened exactly
        assert torch.equal(up.double(), src_u.double().reshape(128, lc.ADAPTER_RANK))
        assert plan[CONV1][0].shape == (128, lc.ADAPTER_RANK) and plan[CONV1][1].shape == (lc.ADAPTER_RANK, 128)
    # the merged conv weight in its own layout: W[o, c, y, x] + s sum_j up[o, j] down[j, c, y, x]
    ad = lc.make_adapter(net, [CONV3], 8)
    w = net.state_dict()[CONV3 + ".weight"].double()
    want = w + 0.5 * torch.einsum("oj,jcyx->ocyx", ad[CONV3 + ".lora_up.weight"].double()[:, :, 0, 0], ad[CONV3 + ".lora_down.weight"].double())
    got = lc.merged_state_dict({CONV3 + ".weight": w.float()}, [(ad, 0.5, None)])[CONV3 + ".weight"]
    assert got.shape == w.shape and rel_l2(got, want) < 1e-6


def _bad_cases(net):
    r = lc.ADAPTER_RANK
    good = lambda: lc.make_adapter(net, [LIN, CONV3], 9)
    def edit(fn):
        d = good()
        fn(d)
        return d
    dn, un = LIN + ".lora_down.weight", LIN + ".lora_up.weight"
    cdn, cun = CONV3 + ".lora_down.weight", CONV3 + ".lora_up.weight"
    flat_ok = "lora_vd_" + LIN.replace(".", "_")
    return {
        "a key that matches no form": edit(lambda d: d.update({LIN + ".lora_mid.weight": torch.zeros(r, r)})),
        "a bare suffix": edit(lambda d: d.update({".alpha": torch.tensor(1.0)})),
        "a path that is no module": edit(lambda d: d.update({"diffuser.image.nowhere.lora_down.weight": torch.zeros(r, 4)})),
        "a path that is a norm": edit(lambda d: d.update({"diffuser.image.context_blocks.1.0.norm.lora_down.weight": torch.zeros(r, 4)})),
        "a flattened path that is no module": edit(lambda d: d.update({flat_ok + "_x.lora_down.weight": torch.zeros(r, 4)})),
        "an up without its down": edit(lambda d: d.pop(dn)),
        "a down without its up": edit(lambda d: d.pop(cun)),
        "an alpha alone": {LIN + ".alpha": torch.tensor(4.0)},
        "a rank mismatch": edit(lambda d: d.update({un: torch.zeros(128, r + 1)})),
        "a down that does not fit": edit(lambda d: d.update({dn: torch.zeros(r, 127)})),
        "an up that does not fit": edit(lambda d: d.update({un: torch.zeros(127, r)})),
        "a conv down with the wrong kernel": edit(lambda d: d.update({cdn: torch.zeros(r, 64, 1, 1)})),
        "a conv down given as a matrix": edit(lambda d: d.update({cdn: torch.zeros(r, 64 * 9)})),
        "a conv up that is not 1x1": edit(lambda d: d.update({cun: torch.zeros(128, r, 3, 3)})),
        "rank 0": edit(lambda d: d.update({dn: torch.zeros(0, 128), un: torch.zeros(128, 0)})),
        "rank 257": edit(lambda d: d.update({dn: torch.zeros(257, 128), un: torch.zeros(128, 257)})),
        "a NaN": edit(lambda d: d[dn].__setitem__((0, 0), float("nan"))),
        "an infinity": edit(lambda d: d[cun].__setitem__((3, 1, 0, 0), float("inf"))),
        "a non-finite alpha": edit(lambda d: d.update({LIN + ".alpha": torch.tensor(float("inf"))})),
        "an alpha that is no scalar": edit(lambda d: d.update({LIN + ".alpha": torch.ones(2)})),
        "the same layer in two forms": edit(lambda d: d.update({flat_ok + ".lora_down.weight": torch.zeros(r, 128)})),
        "an integer tensor": edit(lambda d: d.update({dn: torch.zeros(r, 128, dtype=torch.int32)})),
    }


def test_every_value_error_of_attach(clean):
    from lib.model_zoo import lora
    net = clean
    before = {k: v.clone() for k, v in net.state_dict().items()}
    for what, tensors in _bad_cases(net).items():
        with pytest.raises(ValueError, match="lora.attach"):
            lora.attach(net, "bad", tensors)
        assert lora.attached(net) == [], what
    with pytest.raises(ValueError):
        lora.attach(net, "bad", lc.make_adapter(net, [LIN], 9), alpha=float("nan"))
    # rank 256 is in range; strict=False skips what names no module -- and nothing else
    lora.attach(net, "wide", {LIN + ".lora_down.weight": torch.zeros(256, 128), LIN + ".lora_up.weight": torch.zeros(128, 256)})
    loose = lc.make_adapter(net, [LIN], 9)
    loose["lora_unet_down_blocks_0_attentions_0_proj_in.lora_down.weight"] = torch.zeros(4, 4)
    with pytest.raises(ValueError):
        lora.attach(net, "loose", loose)
    assert lora.attach(net, "loose", loose, strict=False) == [LIN]
    with pytest.raises(ValueError, match="matches no form"):
        lora.attach(net, "loose2", dict(loose, junk=torch.zeros(1)), strict=False)
    with pytest.raises(ValueError, match="already"):
        lora.attach(net, "loose", lc.make_adapter(net, [LIN], 9))                  # a duplicate name
    assert lora.attached(net) == ["wide", "loose"] and lora.active(net) == {}
    # attach activates nothing and writes nothing
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())


def test_an_ambiguous_flattening_is_an_error():
    from lib.model_zoo import lora
    net = torch.nn.Module()
    net.a = torch.nn.Module()
    net.a.b_c = torch.nn.Linear(4, 4)
    net.a_b = torch.nn.Module()
    net.a_b.c = torch.nn.Linear(4, 4)
    net.d = torch.nn.Conv2d(4, 4, 3, groups=2)              # grouped: no target
    t = {"lora_vd_a_b_c.lora_down.weight": torch.zeros(2, 4), "lora_vd_a_b_c.lora_up.weight": torch.zeros(4, 2)}
    with pytest.raises(ValueError, match="ambiguous"):
        lora.attach(net, "x", t)
    assert lora.attach(net, "x", {"a.b_c.lora_down.weight": torch.zeros(2, 4), "a.b_c.lora_up.weight": torch.zeros(4, 2)}) == ["a.b_c"]
    with pytest.raises(ValueError, match="names no"):
        lora.attach(net, "y", {"d.lora_down.weight": torch.zeros(2, 2, 3, 3), "d.lora_up.weight": torch.zeros(4, 2, 1, 1)})


def test_set_adapters_validates_before_it_writes_and_needs_a_gpu(clean):
    from lib.model_zoo import lora
    net = clean
    for i in range(9):
        lora.attach(net, "a%d" % i, lc.make_adapter(net, [LIN] if i else [LIN, CONV3], 20 + i))
    before = {k: v.clone() for k, v in net.state_dict().items()}
    vers = {k: v._version for k, v in net.named_parameters()}
    with pytest.raises(ValueError, match="no adapter named"):
        lora.set_adapters(net, {"nope": 1.0})
    for s in (float("nan"), float("inf"), "1.0", None):
        with pytest.raises(ValueError, match="finite"):
            lora.set_adapters(net, {"a0": s})
    with pytest.raises(ValueError, match="at most 8"):
        lora.set_adapters(net, {"a%d" % i: 1.0 for i in range(9)})
    with pytest.raises(RuntimeError, match="GPU"):          # the parameters are on the CPU: no fallback
        lora.set_adapters(net, {"a0": 1.0})
    lora.set_adapters(net, {})                               # nothing active, nothing to write
    assert lora.active(net) == {}
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert vers == {k: v._version for k, v in net.named_parameters()}
    with pytest.raises(ValueError):
        lora.detach(net, "nope")
    lora.detach(net, "a0")
    assert lora.attached(net) == ["a%d" % i for i in range(1, 9)]
    lora.reset(net)
    assert lora.attached(net) == [] and lora.active(net) == {}


def test_op_refuses_bad_operands_before_any_launch():
    from vd_hip import ops
    b = torch.zeros(4, 6)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.lora_merge(b, [(torch.zeros(4, 2), torch.zeros(2, 6), 1.0)])
    for base, terms in ((torch.zeros(4, 6, dtype=torch.float64), [(torch.zeros(4, 2), torch.zeros(2, 6), 1.0)]),
                        (torch.zeros(24), [(torch.zeros(4, 2), torch.zeros(2, 6), 1.0)]),
                        (torch.zeros(6, 4).t(), [(torch.zeros(4, 2), torch.zeros(2, 6), 1.0)])):
        with pytest.raises(ValueError, match="lora_merge"):
            ops.lora_merge(base, terms)


# ---- 2. files ------------------------------------------------------------------------------------------------------------------------

def test_file_round_trip_through_torch_save(clean, tmp_path):
    from lib.model_zoo import lora
    net = clean
    ad = lc.make_adapter(net, [LIN, CONV3], 12, alpha=3.0, dtype=torch.float16)
    path = tmp_path / "adapter.pt"
    torch.save(dict(ad), str(path))
    back = lora.load_file(str(path))
    assert set(back) == set(ad) and all(torch.equal(back[k], ad[k]) and back[k].dtype == ad[k].dtype for k in ad)
    assert sorted(lora.attach(net, "file", back)) == sorted([CONV3, LIN]) and lora.attached(net) == ["file"]
    torch.save([1, 2, 3], str(path))
    with pytest.raises(ValueError):
        lora.load_file(str(path))


def test_safetensors_without_the_package_is_a_clear_error(tmp_path, monkeypatch):
    import sys
    from lib.model_zoo import lora
    monkeypatch.setitem(sys.modules, "safetensors", None)           # as if it were not installed
    monkeypatch.setitem(sys.modules, "safetensors.torch", None)
    with pytest.raises(RuntimeError, match="safetensors"):
        lora.load_file(str(tmp_path / "adapter.safetensors"))


def test_file_round_trip_through_safetensors(clean, tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from lib.model_zoo import lora
    ad = lc.make_adapter(clean, [LIN, CONV3], 13, alpha=3.0)
    path = str(tmp_path / "adapter.safetensors")
    st.save_file({k: v.contiguous() for k, v in ad.items()}, path)
    back = lora.load_file(path)
    assert set(back) == set(ad) and all(torch.equal(back[k], ad[k]) for k in ad)


# ---- 3. the reference arithmetic of the kernel tests -----------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,ranks", lc.EXACT_CASES)
@pytest.mark.parametrize("f16", [False, True])
def test_exact_sum_generators_check_themselves(N, K, ranks, f16):
    base, terms = lc.exact_operands(N, K, ranks, f16, 100 + N)           # asserts the proof obligation (check_exact)
    ref = lc.statement64(base, terms)
    assert base.dtype == (np.float16 if f16 else np.float32) and len(terms) == len(ranks)
    # exact in ANY order: the emulator's order, the terms reversed, the rank walked backwards
    for order in (terms, terms[::-1], [(u[:, ::-1].copy(), d[::-1].copy(), s) for u, d, s in terms]):
        out = lc.emulate(base, order)
        assert out.dtype == base.dtype and np.array_equal(out.astype(np.float64), ref)
    # and the generator refuses operands that are not: one more bit in a single base element
    worse = base.copy()
    worse[0, 0] = np.float32(0.125) if not f16 else np.float16(0.125)
    with pytest.raises(AssertionError):
        lc.check_exact(worse, terms, f16)


@pytest.mark.parametrize("N,K,ranks", lc.RANDOM_CASES)
def test_emulator_lies_within_the_counted_bound_and_the_order_matters(N, K, ranks):
    base, terms = lc.random_operands(N, K, ranks, 200 + N)
    ref = lc.statement64(base, terms)
    for b, f16 in ((base, False), (base.astype(np.float16), True)):
        out = lc.emulate(b, terms)
        err, bd = np.abs(out.astype(np.float64) - lc.statement64(b, terms)), lc.bound(b, terms, f16)
        assert np.all(err <= bd) and float(err.max()) > 0
        # the bound is one of roundings, not of sizes: a unit of fp32 (fp16) resolution times the rank count at most
        assert float((bd / (np.abs(ref) + 1)).max()) < (2e-3 if f16 else 2e-5)
    if len(terms) > 1:
        swapped = [terms[1], terms[0]] + terms[2:]
        assert np.any(lc.emulate(base, swapped) != lc.emulate(base, terms))


def test_entry_is_declared_bound_and_refuses_bad_arguments_without_a_device():
    import ctypes
    import os
    import re
    from vd_hip import ops
    from vd_hip.loader import PROTOTYPES, VdLoraTerm, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "vd_hip.h")).read()
    assert re.search(r"\bint vd_lora_merge\(", hdr) and "typedef struct VdLoraTerm" in hdr
    assert "#define VD_HIP_ABI_VERSION 8" in hdr
    assert len(PROTOTYPES["vd_lora_merge"][1]) == 8 and '"lora.hip"' in open(os.path.join(root, "versatile-diffusion_amd", "build.py")).read()
    assert ctypes.sizeof(VdLoraTerm) == 24 and callable(ops.lora_merge)
    L = lib()
    assert L.vd_abi_version() == 8                  # the entry is additive
    assert L.vd_lora_merge.argtypes == PROTOTYPES["vd_lora_merge"][1]
    P = ctypes.c_void_p

    def call(base=4096, out=1 << 20, f16=0, n_terms=1, N=8, K=8, up=1 << 24, down=1 << 25, r=4, table=True):
        t = (VdLoraTerm * 8)(*[VdLoraTerm(up, down, 1.0, r) for _ in range(8)])
        return L.vd_lora_merge(P(base), P(out), f16, t if table else None, n_terms, N, K, None)
    for kw in (dict(base=None), dict(out=None), dict(table=False), dict(up=None), dict(down=None), dict(n_terms=0), dict(n_terms=9),
               dict(n_terms=-1), dict(r=0), dict(r=257), dict(r=-3), dict(N=0), dict(K=0), dict(N=-8), dict(K=-8), dict(out=4096),
               dict(out=4096 + 128), dict(base=4098), dict(out=(1 << 20) + 1, f16=1), dict(up=(1 << 24) + 2)):
        assert call(**kw) < 0 and L.vd_last_error().decode().startswith("vd_lora_merge"), kw


# ---- 4. the precondition of the GPU parity test -------------------------------------------------------------------------------------

def test_adapted_model_differs_from_the_base_model_by_far_more_than_the_parity_bound(tiny_cpu):
    """tests/test_lora_gpu.py holds the adapted forward to FWD_TOL against the oracle run on the merged weights.  That shows
    something only if the adapter moves the output by much more than FWD_TOL: here by at least ten times as much, on the single-
    context call and on the dual-context call of that test."""
    from oracle import vd_oracle as O
    net, sd = tiny_cpu
    m = meta()
    plan = O.unet_plan(**m["unet2d"])
    g = load_gold("unet_tiny.npz")
    x, t, ci, ct = (torch.from_numpy(g[k]) for k in ("x", "t", "c_img", "c_text"))
    ad = lc.make_adapter(net, lc.adapter_paths(net), 11)
    msd = lc.merged_state_dict(sd, [(ad, lc.ADAPTER_SCALE, None)])
    mix = [("text", ct, 0.4), ("image", ci, 0.6)]
    with torch.no_grad():
        d1 = rel_l2(O.apply_model(msd, plan, x, t, ci, c_type="image", global_ptr="image"),
                    O.apply_model(sd, plan, x, t, ci, c_type="image", global_ptr="image"))
        d2 = rel_l2(O.apply_model_multicontext(msd, plan, x, t, mix, "image", "image"),
                    O.apply_model_multicontext(sd, plan, x, t, mix, "image", "image"))
    print("adapter moves the tiny forward by rel-L2 %.4f (image context), %.4f (text + image)" % (d1, d2))
    assert d1 >= 10 * lc.FWD_TOL and d2 >= 10 * lc.FWD_TOL
