"""LoRA adapters on the GPU: the merge kernel (vd_lora_merge through ops.lora_merge) bit for bit on exact-sum operands and per element
against the float64 statement with a bound counted from the contract's roundings (tests/lora_cases.py), the bytes it must not touch,
the order of its terms, its argument checks -- and the model layer (lib/model_zoo/lora.py) on the tiny model: the parameters, every
kernel-layout pack following an edit, parity with the oracle on the merged weights, off giving the old bits back, independence of the
history of switches, the samplers' kept graphs, and edits made by someone else."""
import numpy as np
import pytest
import torch

import lora_cases as lc
from lora_cases import ADAPTER_SCALE, FWD_TOL
from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

GUARD = 64          # guard elements on either side of out: 256 / 128 bytes, so offset 0 keeps out 16-byte aligned


def _view(dev, host, offset):
    """`host` on the device as a view `offset` elements into a larger allocation (offset = 1: misaligned)."""
    base = torch.empty((host.numel() + offset,), device=dev, dtype=host.dtype)
    out = base[offset:]
    out.copy_(host.reshape(-1))
    return out.view(host.shape)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _merge(dev, base, terms, offset=0):
    """One launch on views `offset` elements into larger allocations; out lies between two guards of GUARD elements holding a
    pattern, and starts out as NaN.  Returns the result on the host (numpy, base's dtype) after checking the guards and base."""
    from vd_hip import ops
    N, K = base.shape
    hb = torch.from_numpy(base)
    bd = _view(dev, hb, offset)
    td = [(_view(dev, torch.from_numpy(u), offset), _view(dev, torch.from_numpy(d), offset), s) for u, d, s in terms]
    alloc = torch.full((2 * GUARD + offset + N * K,), float("nan"), device=dev, dtype=hb.dtype)
    pattern = torch.arange(GUARD + offset, device=dev).to(hb.dtype) + 0.5
    alloc[:GUARD + offset] = pattern
    alloc[GUARD + offset + N * K:] = pattern[:GUARD]
    out = alloc[GUARD + offset:GUARD + offset + N * K].view(N, K)
    assert (out.data_ptr() % 16 == 0) == (offset == 0) and (bd.data_ptr() % 16 == 0) == (offset == 0)
    got = ops.lora_merge(bd, td, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(_bits(alloc[:GUARD + offset]), _bits(pattern)) and torch.equal(_bits(alloc[GUARD + offset + N * K:]), _bits(pattern[:GUARD]))
    assert torch.equal(_bits(bd.cpu()), _bits(hb))                                   # base is read only
    for (u, d, _), (hu, hd, _) in zip(td, terms):
        assert torch.equal(u.cpu(), torch.from_numpy(hu)) and torch.equal(d.cpu(), torch.from_numpy(hd))
    return out.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(a.view(np.int16 if a.dtype == np.float16 else np.int32), b.view(np.int16 if b.dtype == np.float16 else np.int32))


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("N,K,ranks", lc.EXACT_CASES)
def test_exact_sum_operands_bit_for_bit(dev, N, K, ranks, f16, offset):
    base, terms = lc.exact_operands(N, K, ranks, f16, 100 + N)
    want = lc.emulate(base, terms)
    assert np.array_equal(want.astype(np.float64), lc.statement64(base, terms))      # exact: nothing was rounded anywhere
    got = _merge(dev, base, terms, offset)
    assert got.dtype == base.dtype and _same_bits(got, want), int((got != want).sum())


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("N,K,ranks", lc.RANDOM_CASES)
def test_random_operands_within_the_counted_bound_and_equal_to_the_emulator(dev, N, K, ranks, f16):
    base, terms = lc.random_operands(N, K, ranks, 200 + N)
    if f16:
        base = base.astype(np.float16)
    ref, bound, emu = lc.statement64(base, terms), lc.bound(base, terms, f16), lc.emulate(base, terms)
    for offset in (0, 1):
        got = _merge(dev, base, terms, offset)
        err = np.abs(got.astype(np.float64) - ref)
        print("N %d K %d f16 %d offset %d: max err / bound %.3f, share off the emulator %.2e" % (
            N, K, f16, offset, float((err / bound).max()), float(np.mean(got != emu))))
        assert np.all(err <= bound), float((err / bound).max())
        assert float(np.mean(got != emu)) < lc.TIE_SHARE                 # the emulator's fma ties (double rounding) only


def test_term_order_is_the_tables_order(dev):
    N, K, ranks = lc.RANDOM_CASES[0]
    base, terms = lc.random_operands(N, K, ranks, 300)
    swapped = [terms[1], terms[0]] + terms[2:]
    a, b = _merge(dev, base, terms), _merge(dev, base, swapped)
    assert float(np.mean(a != lc.emulate(base, terms))) < lc.TIE_SHARE and float(np.mean(b != lc.emulate(base, swapped))) < lc.TIE_SHARE
    assert int((a != b).sum()) >= 1                                       # or the test would be vacuous
    assert np.any(lc.emulate(base, terms) != lc.emulate(base, swapped))


def test_argument_checks_return_errors_not_launches(dev):
    import ctypes
    from vd_hip import ops
    from vd_hip.loader import VdLoraTerm, lib
    z = lambda *s, **k: torch.zeros(s, device=dev, **k)
    base, out = z(8, 12), torch.full((8, 12), 7.0, device=dev)
    good = [(z(8, 4), z(4, 12), 1.0)]
    bad = [
        dict(base=z(8, 12, dtype=torch.float64)), dict(base=z(8, 12, dtype=torch.bfloat16)), dict(base=z(96)), dict(base=z(12, 8).t()),
        dict(base=z(0, 12)), dict(terms=[]), dict(terms=good * 9), dict(terms=[(z(8, 4).half(), z(4, 12), 1.0)]),
        dict(terms=[(z(8, 4), z(4, 12, dtype=torch.float64), 1.0)]), dict(terms=[(z(8, 4), z(5, 12), 1.0)]),
        dict(terms=[(z(7, 4), z(4, 12), 1.0)]), dict(terms=[(z(8, 4), z(4, 11), 1.0)]), dict(terms=[(z(4, 8).t(), z(4, 12), 1.0)]),
        dict(terms=[(z(8, 4), z(12, 4).t(), 1.0)]), dict(terms=[(z(8, 257), z(257, 12), 1.0)]), dict(terms=[(z(8, 0), z(0, 12), 1.0)]),
        dict(terms=[(torch.zeros(8, 4), z(4, 12), 1.0)]), dict(terms=[(z(8, 4), torch.zeros(4, 12), 1.0)]),
        dict(out=base), dict(out=z(8, 12).half()), dict(out=z(12, 8)), dict(out=torch.zeros(8, 12)), dict(out=z(12, 8).t()),
        dict(out=torch.nn.Parameter(z(8, 12))),
    ]
    for kw in bad:
        a = dict(dict(base=base, terms=good, out=out), **kw)
        with pytest.raises(ValueError, match="lora_merge"):
            ops.lora_merge(a["base"], a["terms"], out=a["out"])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.lora_merge(torch.zeros(8, 12), good)
    # the C entry on device pointers
    L, P = lib(), ctypes.c_void_p
    up, down = good[0][0], good[0][1]

    def call(b=base.data_ptr(), o=out.data_ptr(), n_terms=1, N=8, K=12, u=up.data_ptr(), d=down.data_ptr(), r=4, table=True):
        t = (VdLoraTerm * 8)(*[VdLoraTerm(u, d, 1.0, r) for _ in range(8)])
        return L.vd_lora_merge(P(b), P(o), 0, t if table else None, n_terms, N, K, P(torch.cuda.current_stream().cuda_stream))
    for kw in (dict(b=None), dict(o=None), dict(table=False), dict(u=None), dict(d=None), dict(n_terms=0), dict(n_terms=9), dict(r=0),
               dict(r=257), dict(N=0), dict(K=0), dict(N=-1), dict(o=base.data_ptr()), dict(o=base.data_ptr() + 16)):
        assert call(**kw) < 0 and L.vd_last_error().decode().startswith("vd_lora_merge"), kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((base == 0).all())           # nothing ran
    assert bool((ops.lora_merge(base, good, out=out) == 0).all())         # and the good call does


# ---- 2. the model --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sd32():
    """The synthetic fp32 weights of the tiny model (what the oracle consumes)."""
    from lib.model_zoo import get_model
    m = meta()
    return synth_into(get_model()(tiny_vd_cfg(m), verbose=False), m["seed"])


def _net(dev, state, half=True):
    """A tiny model that never saw lora, holding `state`."""
    from lib.model_zoo import get_model
    net = get_model()(tiny_vd_cfg(meta()), verbose=False)
    if half:
        net = net.half()
    net.to(dev)
    net.load_state_dict(state, strict=False)
    return net


@pytest.fixture(scope="module")
def plan():
    from oracle import vd_oracle as O
    return O.unet_plan(**meta()["unet2d"])


@pytest.fixture(scope="module")
def gold():
    return load_gold("unet_tiny.npz")


def _merged_net(dev, net, sd32):
    """A tiny model that never saw lora, built like `net` was (the fp32 state, so the same schedule) and then handed every
    parameter of `net` as it is now."""
    fresh = _net(dev, sd32)
    missing, unexpected = fresh.load_state_dict({k: p.detach() for k, p in net.named_parameters()}, strict=False)
    assert not unexpected
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(fresh.parameters(), net.parameters()))
    return fresh


def _params(net):
    return {k: v.detach().clone() for k, v in net.named_parameters()}


def _versions(net):
    return {k: v._version for k, v in net.named_parameters()}


def _np2(t):
    return t.detach().cpu().reshape(t.shape[0], -1).numpy()


def _check_params(net, base, adapters, touched):
    """Every touched parameter within the counted bound of the float64 merge of its base (in the parameter's dtype: the bound has the
    fp16 rounding when the model is .half()); every other parameter bit for bit what it was."""
    worst, off, total = 0.0, 0, 0
    for k, v in net.named_parameters():
        path = k[:-len(".weight")] if k.endswith(".weight") else None
        if path in touched:
            b = _np2(base[k])
            terms = lc.layer_terms(adapters, path)
            assert terms, path
            err = np.abs(_np2(v).astype(np.float64) - lc.statement64(b, terms))
            bd = lc.bound(b, terms, v.dtype == torch.float16)
            assert np.all(err <= bd), (path, float((err / bd).max()))
            off, total = off + int((_np2(v) != lc.emulate(b, terms)).sum()), total + v.numel()
            assert not torch.equal(v, base[k]), path
            worst = max(worst, float((err / bd).max()))
        else:
            assert torch.equal(_bits(v), _bits(base[k])), k
    assert off <= max(1, int(lc.TIE_SHARE * total)), (off, total)         # the emulator's fma ties only, over all layers together
    return worst


def _calls(dev, gold):
    """The forwards of the model tests, as (name, callable(net)): the golden 16 x 16 batch with an image context (every layer of
    diffuser.image), with a text context, the dual-context call, and a guided pair on an 8 x 8 latent handed over un-replicated."""
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dev).half()
    x, t, ci, ct = T(gold["x"]), torch.from_numpy(gold["t"]).to(dev), T(gold["c_img"]), T(gold["c_text"])
    x8 = T(gold["x"])[:1, :, :8, :8].contiguous()
    t2 = torch.full((2,), 501, device=dev, dtype=torch.long)
    c2 = torch.cat([ct[:1] * 0.0, ct[:1]])
    return [
        ("image", lambda n: n.apply_model({"type": "image", "x": x}, t, {"type": "image", "c": ci})),
        ("text", lambda n: n.apply_model({"type": "image", "x": x}, t, {"type": "text", "c": ct})),
        ("dual", lambda n: n.apply_model_multicontext({"type": "image", "x": x}, t, [
            {"type": "text", "c": ct, "ratio": 0.4}, {"type": "image", "c": ci, "ratio": 0.6}])),
        ("guided 8x8", lambda n: n.apply_model({"type": "image", "x": x8, "repeat": 2}, t2, {"type": "text", "c": c2})),
    ]


def _pack_keys(net):
    return sorted(set(k for m in net.modules() for k in m.__dict__.get("_vd_pack_cache", {})))


@pytest.mark.parametrize("half", [True, False])
def test_parameters_touched_within_the_bound_untouched_bit_identical(dev, sd32, half):
    from lib.model_zoo import lora
    net = _net(dev, sd32, half)
    paths = lc.adapter_paths(net)
    ad = lc.make_adapter(net, paths, 11)
    base, vers, ptrs = _params(net), _versions(net), [p.data_ptr() for p in net.parameters()]
    assert sorted(lora.attach(net, "a", ad)) == sorted(paths)
    assert _versions(net) == vers and lora.active(net) == {}              # attach writes nothing
    lora.set_adapters(net, {"a": ADAPTER_SCALE})
    assert lora.active(net) == {"a": ADAPTER_SCALE}
    worst = _check_params(net, base, [(ad, ADAPTER_SCALE, None)], set(paths))
    print("half %d: %d layers, worst error / bound %.3f" % (half, len(paths), worst))
    now = _versions(net)
    for k in vers:
        touched = k.endswith(".weight") and k[:-len(".weight")] in paths
        assert now[k] == vers[k] + (1 if touched else 0), k                # one write per touched layer, none elsewhere
    assert [p.data_ptr() for p in net.parameters()] == ptrs               # written in place: no storage moved


def test_every_pack_follows_the_edit(dev, sd32, gold):
    """The adapted net against a fresh net that was handed the adapted net's own state_dict(): bit-identical outputs on calls that
    walk every pack kind the tiny model reaches.  The packs were all built BEFORE the switch (the base forwards below), so each one
    that reads an adapted weight had to be rebuilt.  Pack keys built by these calls on the tiny model: see PACKS."""
    from lib.model_zoo import lora
    from lib.model_zoo.hip_layers import PackCache
    net = _net(dev, sd32)
    calls = _calls(dev, gold)
    base_out = [f(net) for _, f in calls]
    keys = _pack_keys(net)
    print("pack keys built:", keys)
    assert set(PACKS) <= set(keys), (keys, PACKS)
    ad = lc.make_adapter(net, lc.adapter_paths(net), 11)
    lora.attach(net, "a", ad)
    lora.set_adapters(net, {"a": ADAPTER_SCALE})
    builds = PackCache.builds
    out = [f(net) for _, f in calls]
    assert PackCache.builds > builds
    fresh = _net(dev, net.state_dict())
    assert not hasattr(fresh, "_vd_lora")
    ref = [f(fresh) for _, f in calls]
    for (name, _), o, r, b in zip(calls, out, ref, base_out):
        assert torch.equal(o, r), (name, rel_l2(o, r))
        print("%s: the adapter moves the output by rel-L2 %.3f" % (name, rel_l2(o, b)))
        assert not torch.equal(o, b), name                                 # and the adapter moved the output


# what the calls of _calls build on the tiny model (widths 64 and 128), as listed from _vd_pack_cache on an MI355X: the plain packs
# ("w"), the stacked time-embedding projection ("emb_w"), the fused q|k|v and the k|v pack of cross-attention ("qkv", "kv"), the
# LayerNorm-folded q|k|v / q / GEGLU projections ("qkv_ln", "q_ln", "geglu_ln"), ff.net.2 folded with proj_out ("proj_fold"), the
# per-phase weights of the upsample conv ("w_phase"), the fragment-ordered skip convolution of the 8 x 8 level ("w_stream_1x1") and
# the pre-combined ResBlock biases ("b1", "b2s").  The weight-streaming packs of the wide levels ("w_stream", "*_ln_stream",
# "proj_fold_stream") need widths the tiny model does not have.
PACKS = ("b1", "b2s", "emb_w", "geglu_ln", "kv", "proj_fold", "q_ln", "qkv", "qkv_ln", "w", "w_phase", "w_stream_1x1")


def test_parity_with_the_oracle_on_the_merged_weights(dev, sd32, plan, gold):
    """The bound is the one tests/test_parity_gpu.py holds this same tiny forward to (FWD_TOL = 5e-3, test_parity_gpu.py:18, used at
    :42-:47 in test_tiny_unet_vs_golden), unchanged.  tests/test_lora_cpu.py shows the adapter moves the output by > 10 FWD_TOL."""
    from lib.model_zoo import lora
    from oracle import vd_oracle as O
    net = _net(dev, sd32)
    ad = lc.make_adapter(net, lc.adapter_paths(net), 11)
    lora.attach(net, "a", ad)
    lora.set_adapters(net, {"a": ADAPTER_SCALE})
    msd = lc.merged_state_dict(sd32, [(ad, ADAPTER_SCALE, None)])
    x, t, ci, ct = (torch.from_numpy(gold[k]) for k in ("x", "t", "c_img", "c_text"))
    mix = [("text", ct, 0.4), ("image", ci, 0.6)]
    with torch.no_grad():
        ref1 = O.apply_model(msd, plan, x, t, ci, c_type="image", global_ptr="image")
        ref2 = O.apply_model_multicontext(msd, plan, x, t, mix, "image", "image")
        off1 = O.apply_model(sd32, plan, x, t, ci, c_type="image", global_ptr="image")
    calls = dict(_calls(dev, gold))
    e1, e2 = calls["image"](net), calls["dual"](net)
    print("adapted forward vs oracle on merged weights: %.2e (image context), %.2e (text + image); the adapter moves it by %.3f" % (
        rel_l2(e1, ref1), rel_l2(e2, ref2), rel_l2(ref1, off1)))
    assert rel_l2(e1, ref1) < FWD_TOL
    assert rel_l2(e2, ref2) < FWD_TOL
    assert rel_l2(e1, off1) > 10 * FWD_TOL


def test_off_means_the_old_bits(dev, sd32, gold):
    from lib.model_zoo import lora
    from lib.model_zoo.hip_layers import PackCache
    net = _net(dev, sd32)
    calls = _calls(dev, gold)
    paths = lc.adapter_paths(net)
    ad = lc.make_adapter(net, paths, 11)
    before = _params(net)
    out0 = [f(net) for _, f in calls]
    lora.attach(net, "a", ad)
    lora.set_adapters(net, {"a": ADAPTER_SCALE})
    out1 = [f(net) for _, f in calls]                                      # packs of the adapted weights are built here
    assert not torch.equal(out1[0], out0[0])
    # the same dict twice: no write, no pack build
    vers, builds = _versions(net), None
    lora.set_adapters(net, {"a": ADAPTER_SCALE})
    assert _versions(net) == vers
    builds = PackCache.builds
    assert all(torch.equal(f(net), o) for (_, f), o in zip(calls, out1))
    assert PackCache.builds == builds
    # another scale: exactly the touched layers are rewritten, once
    lora.set_adapters(net, {"a": 0.25})
    now = _versions(net)
    bumped = sorted(k[:-len(".weight")] for k in vers if now[k] != vers[k])
    assert bumped == sorted(paths) and all(now[k] - vers[k] in (0, 1) for k in vers)
    _check_params(net, before, [(ad, 0.25, None)], set(paths))
    # off: the parameters and the forward have the old bits
    lora.set_adapters(net, {})
    assert lora.active(net) == {}
    after = dict(net.named_parameters())
    assert all(torch.equal(_bits(after[k]), _bits(before[k])) for k in before)
    assert all(torch.equal(f(net), o) for (_, f), o in zip(calls, out0))
    # detach of an active adapter switches it off first
    lora.set_adapters(net, {"a": ADAPTER_SCALE})
    lora.detach(net, "a")
    assert lora.active(net) == {} and lora.attached(net) == []
    assert all(torch.equal(_bits(after[k]), _bits(before[k])) for k in before)
    assert all(torch.equal(f(net), o) for (_, f), o in zip(calls, out0))


def test_history_independence_and_stacking(dev, sd32):
    from lib.model_zoo import lora
    net = _net(dev, sd32)
    paths = lc.adapter_paths(net)
    pa, pb = paths[: 2 * len(paths) // 3], paths[len(paths) // 3:]           # overlapping: a alone, both, b alone
    a, b = lc.make_adapter(net, pa, 21), lc.make_adapter(net, pb, 22, rank=7, alpha=3.5)
    base = _params(net)
    lora.attach(net, "a", a)
    lora.attach(net, "b", b)
    target = {"a": 0.5, "b": -1.0}
    lora.set_adapters(net, target)                                          # reached directly
    direct = _params(net)
    _check_params(net, base, [(a, 0.5, None), (b, -1.0, None)], set(paths))
    lora.set_adapters(net, {})
    lora.set_adapters(net, {"a": 1.0})                                      # via a alone at another scale
    lora.set_adapters(net, target)
    via_a = _params(net)
    lora.set_adapters(net, {"b": 2.0})                                      # via b alone, then nothing
    lora.set_adapters(net, {})
    assert all(torch.equal(_bits(p), _bits(base[k])) for k, p in net.named_parameters())
    lora.set_adapters(net, dict(reversed(list(target.items()))))            # the order of the dict does not matter: attach order does
    via_b = _params(net)
    for k in direct:
        assert torch.equal(_bits(direct[k]), _bits(via_a[k])) and torch.equal(_bits(direct[k]), _bits(via_b[k])), k
    assert lora.active(net) == target


def _sample(sampler, xT, c, u, steps=4):
    z, _ = sampler.sample(steps=steps, shape=list(xT.shape), x_info={"type": "image", "xt": xT},
                          c_info={"type": "text", "conditioning": c, "unconditional_conditioning": u,
                                  "unconditional_guidance_scale": 7.5}, verbose=False)
    return z


@pytest.mark.parametrize("kind", ["2m", "ddim"])
def test_samplers_and_kept_graphs_follow_the_switch(dev, sd32, kind):
    """One sampler object (its kept step graphs, packs and whatever else it holds) across off -> on -> off: on equals a fresh net
    holding the merged weights, off equals the first run.  Batch 2, 4 steps, an 8 x 8 latent (the smallest the parity tests run the
    tiny UNet at), fixed xt.

    The fresh net is _merged_net: it holds the adapted net's parameters and the SAME schedule.  (Handing it the .half() net's whole
    state_dict() would also hand it the schedule buffers rounded to fp16, which VD_v2_0._load_from_state_dict turns into the host
    schedule the samplers read: two nets with identical weights then sample 2e-3 apart, adapters or not.)"""
    from lib.model_zoo import lora
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    cls = {"2m": DPMSolverSampler, "ddim": DDIMSampler}[kind]
    net = _net(dev, sd32)
    g = torch.Generator().manual_seed(41)
    xT = torch.randn((2, 4, 8, 8), generator=g).half().to(dev)
    c = (torch.randn((2, 9, 128), generator=g) * 2.0).half().to(dev)
    u = torch.zeros_like(c)
    sampler = cls(net)
    assert sampler.graph_cache
    z_a = _sample(sampler, xT, c, u)
    assert torch.equal(_sample(sampler, xT, c, u), z_a)                     # replayed: the same bits
    lora.attach(net, "a", lc.make_adapter(net, lc.adapter_paths(net), 11))
    lora.set_adapters(net, {"a": ADAPTER_SCALE})
    z_b = _sample(sampler, xT, c, u)
    lora.set_adapters(net, {})
    z_c = _sample(sampler, xT, c, u)
    assert torch.equal(z_c, z_a)
    print("%s: the adapter moves the latent by rel-L2 %.3f" % (kind, rel_l2(z_b, z_a)))
    assert not torch.equal(z_b, z_a) and bool(torch.isfinite(z_b).all())
    lora.set_adapters(net, {"a": ADAPTER_SCALE})
    fresh = _merged_net(dev, net, sd32)
    assert not hasattr(fresh, "_vd_lora")
    assert torch.equal(_sample(cls(fresh), xT, c, u), z_b)                  # no stale graph, pack or K/V entry survived the switch
    assert torch.equal(_sample(sampler, xT, c, u), z_b)


def test_external_edits(dev, sd32):
    from lib.model_zoo import lora
    net = _net(dev, sd32)
    paths = lc.adapter_paths(net)
    ad = lc.make_adapter(net, paths, 11)
    other = {k: (v * 1.25 if k.endswith(".weight") and v.dim() >= 2 else v) for k, v in sd32.items()}
    # an edit while the adapter is merged in: refuse, whatever is asked for
    lora.attach(net, "a", ad)
    lora.set_adapters(net, {"a": ADAPTER_SCALE})
    net.load_state_dict(other, strict=False)
    for want in ({"a": ADAPTER_SCALE}, {"a": 0.5}, {}):
        with pytest.raises(RuntimeError, match="reset"):
            lora.set_adapters(net, want)
    with pytest.raises(RuntimeError, match="reset"):
        lora.detach(net, "a")
    edited = _params(net)
    lora.reset(net)                                                        # forgets, writes nothing
    assert lora.attached(net) == [] and all(torch.equal(_bits(p), _bits(edited[k])) for k, p in net.named_parameters())
    lora.attach(net, "a", ad)
    lora.set_adapters(net, {"a": ADAPTER_SCALE})                           # succeeds, on the new weights
    _check_params(net, edited, [(ad, ADAPTER_SCALE, None)], set(paths))
    lora.set_adapters(net, {})
    assert all(torch.equal(_bits(p), _bits(edited[k])) for k, p in net.named_parameters())
    # the same edit with no adapter active (attached, and switched on and off before): adopted as the new base
    net2 = _net(dev, sd32)
    lora.attach(net2, "a", ad)
    lora.set_adapters(net2, {"a": 0.5})
    lora.set_adapters(net2, {})
    net2.load_state_dict(other, strict=False)
    edited2 = _params(net2)
    lora.set_adapters(net2, {"a": ADAPTER_SCALE})
    _check_params(net2, edited2, [(ad, ADAPTER_SCALE, None)], set(paths))
    lora.set_adapters(net2, {})
    assert all(torch.equal(_bits(p), _bits(edited2[k])) for k, p in net2.named_parameters())
    # .half() moves every parameter: with nothing active that is adopted too
    net3 = _net(dev, sd32, half=False)
    lora.attach(net3, "a", ad)
    net3 = net3.half()
    base3 = _params(net3)
    lora.set_adapters(net3, {"a": ADAPTER_SCALE})
    _check_params(net3, base3, [(ad, ADAPTER_SCALE, None)], set(paths))
