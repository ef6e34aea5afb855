"""Self-attention guidance on the GPU: the column mass (vd_sag_mass_f16 through ops.sag_mass), the degrade (vd_sag_degrade_f16
through ops.sag_degrade) and the fold (vd_sag_fold_f16 through ops.sag_fold) per element against the float64 oracles of
tests/sag_cases.py, the forward with x_info['sag'] (same eps bits, the mass of the middle attn1's own operands), the four samplers'
loops against the oracle loop, graph replay against eager bodies, the kept graph across scales and sigmas, and the combinations
with the guidance rescale, inpainting and FreeU."""
import numpy as np
import pytest
import torch

import pag_cases as pc
import sag_cases as sc
from sag_cases import FWD_TOL, LATENT_TOL, SAG_SCALE, SHAPE, STEPS
from vdtest_util import meta, rel_l2, tiny_vd_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plan():
    from oracle import vd_oracle as O
    return O.unet_plan(**meta()["unet2d"])


@pytest.fixture(scope="module")
def tiny(dev, plan):
    """The tiny net with the middle attn1.to_q.weight scaled by sag_cases.SHARPEN, on the device in fp16, and the same fp32 weights
    for the oracle."""
    from lib.model_zoo import get_model
    from vdtest_util import synth_into
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    sd = sc.sharpen(synth_into(net, m["seed"]), plan)
    net.load_state_dict(sd, strict=False)
    net = net.half()
    net.to(dev)
    return net, sd


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def f32bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- 1. the column mass ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sc.MASS_KINDS)
@pytest.mark.parametrize("shape", sc.MASS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mass_vs_the_float64_softmax_per_element(dev, shape, kind):
    from vd_hip import ops
    B, H, N, D = shape
    q, k, ref, counts = sc.mass_case(shape, kind)
    got = ops.sag_mass(q.to(dev), k.to(dev), H)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, N) and got.is_contiguous()
    again = ops.sag_mass(q.to(dev), k.to(dev), H)
    assert torch.equal(f32bits(got), f32bits(again))                            # two calls: the same bits
    ref = ref.numpy()
    if kind == "uniform":
        assert np.abs(ref - 1.0).max() < 1e-12
    if kind == "selector":      # attention as a count: how many queries chose key j, averaged over the heads, up to exp(-32)
        assert np.abs(ref - counts.mean(1)).max() <= N * np.exp(-32.0) and counts.max() > 1 and (counts == 0).any()
    err = np.abs(got.double().cpu().numpy() - ref)
    bound = sc.mass_bound(ref)
    print("mass %s %s: max |got - ref| / bound %.3f; sum per sample / N %s" % (shape, kind, float((err / bound).max()),
                                                                            (got.double().sum(1) / N).tolist()))
    assert (err <= bound).all()


def test_mass_on_column_slices_of_a_fused_projection_and_a_batch_slice(dev):
    from vd_hip import ops
    B, H, N, D = 2, 2, 70, 40
    C = H * D
    g = torch.Generator().manual_seed(5)
    fused = (torch.randn((B + 1, N, 3 * C), generator=g) * 0.7).half().to(dev)
    kept = fused.clone()
    for base in (fused[:B], fused[1:]):
        q, k = base[..., :C], base[..., C:2 * C]
        ref = sc.mass_ref64(q.cpu(), k.cpu(), H).numpy()
        got = ops.sag_mass(q, k, H)
        assert (np.abs(got.double().cpu().numpy() - ref) <= sc.mass_bound(ref)).all()
        assert torch.equal(f32bits(got), f32bits(ops.sag_mass(q.contiguous(), k.contiguous(), H)))      # the views change no bit
        out = torch.full((B + 1, N), 7.0, dtype=torch.float32, device=dev)                              # into a caller's rows
        assert ops.sag_mass(q, k, H, scale=0.1, out=out[:B]).data_ptr() == out.data_ptr()
        ref = sc.mass_ref64(q.cpu(), k.cpu(), H, 0.1).numpy()
        assert (np.abs(out[:B].double().cpu().numpy() - ref) <= sc.mass_bound(ref)).all() and bool((out[B] == 7.0).all())
    assert torch.equal(fused, kept)


def test_mass_refuses_more_than_1024_tokens_and_bad_operands(dev):
    from vd_hip import ops
    t = lambda *s: torch.zeros(s, dtype=torch.float16, device=dev)
    with pytest.raises(ops.VdHipError, match="sag_mass"):
        ops.sag_mass(t(1, 1025, 80), t(1, 1025, 80), 2)
    with pytest.raises(ops.VdHipError, match="sag_mass"):
        ops.sag_mass(t(1, 64, 80), t(1, 65, 80), 2)
    with pytest.raises(ops.VdHipError, match="vd_sag_mass_f16.*head dim"):
        ops.sag_mass(t(1, 64, 48), t(1, 64, 48), 1)
    shifted = t(1, 64, 3 * 80 + 8)
    with pytest.raises(ops.VdHipError, match="vd_sag_mass_f16"):
        ops.sag_mass(shifted[..., 4:84], shifted[..., 84:164], 2)
    with pytest.raises(ops.VdHipError, match="sag_mass"):
        ops.sag_mass(t(1, 64, 80), t(1, 64, 80), 2, out=torch.zeros((1, 63), dtype=torch.float32, device=dev))


# ---- 2. the degrade --------------------------------------------------------------------------------------------------------------

def _degrade(dev, x, eps, mass, ratio, sigma, a, Hm, Wm, out=None):
    from vd_hip import ops
    f32 = lambda v: torch.tensor(np.asarray(v, dtype=np.float32), device=dev)
    return ops.sag_degrade(x.to(dev), eps.to(dev), f32(mass), f32(ratio), f32(sc.taps(sigma)), f32(sc.coef_of(a)), Hm, Wm, out=out)


@pytest.mark.parametrize("sigma", [1.0, 2.0])
@pytest.mark.parametrize("ratio", sc.DEGRADE_RATIOS, ids=lambda r: "r" + "-".join(str(v) for v in r))
@pytest.mark.parametrize("shape", sc.DEGRADE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_degrade_vs_the_float64_definition_per_element(dev, shape, ratio, sigma):
    B, C, H, W, Hm, Wm = shape
    for fill in (None, 0.0, 2.0):
        x, eps, mass = sc.degrade_case(shape, len(ratio), sigma, fill)
        ref, A, Mpx = sc.degrade_ref64(x, eps, mass, ratio, sigma, sc.DEGRADE_ALPHA, Hm, Wm)
        if fill is not None:
            assert bool(Mpx.all()) == (fill == 2.0) and bool(Mpx.any()) == (fill == 2.0)      # an all-zero and an all-one mask
        elif Hm * Wm > 1:
            assert Mpx.any() and not Mpx.all()
        got = _degrade(dev, x, eps, mass, ratio, sigma, sc.DEGRADE_ALPHA, Hm, Wm)
        assert got.dtype == torch.float16 and tuple(got.shape) == (B, C, H, W)
        err = np.abs(got.double().cpu().numpy() - ref)
        bound = sc.degrade_bound(ref, A)
        print("degrade %s ratio %s sigma %.1f fill %s: masked share %.2f; max |got - ref| / bound %.3f"
              % (shape, ratio, sigma, fill, float(Mpx.mean()), float((err / bound).max())))
        assert (err <= bound).all()


def test_degrade_threshold_is_strict_and_the_mask_is_exact(dev):
    """Masses of exactly 1.0 (and ratio sums that give exactly 1.0) stay unmasked, the next fp32 above is masked: on a constant-per-cell
    check the output equals the unblurred re-noising bit for bit exactly where the mask is off."""
    shape = (1, 4, 20, 20, 3, 3)
    x, eps, _ = sc.degrade_case(shape, 2, 1.0)
    up = np.nextafter(np.float32(1.0), np.float32(2.0))
    mass = np.array([[[1.0, up, 2.0, 0.5, 1.0, 0.0, up, 1.0, 2.0]], [[1.0, up, 0.0, 2.0, up, 2.0, 1.0, 0.5, 2.0]]], np.float32)
    for ratio in ((0.5, 0.5), (0.25, 0.75)):
        ref, A, Mpx = sc.degrade_ref64(x, eps, mass, ratio, 1.0, sc.DEGRADE_ALPHA, 3, 3)
        got = _degrade(dev, x, eps, mass, ratio, 1.0, sc.DEGRADE_ALPHA, 3, 3)
        off = _degrade(dev, x, eps, np.zeros_like(mass), ratio, 1.0, sc.DEGRADE_ALPHA, 3, 3)       # nothing masked: d = p0
        same = (bits(got) == bits(off)).numpy()
        assert same[:, :, ~Mpx[0]].all() and not same[:, :, Mpx[0]].all()
        assert (np.abs(got.double().cpu().numpy() - ref) <= sc.degrade_bound(ref, A)).all()
    assert not Mpx.reshape(-1)[0] and Mpx.any()                                                      # cell 0: exactly 1.0, unmasked


def test_degrade_writes_nothing_outside_and_refuses_small_planes(dev):
    from vd_hip import ops
    shape = (1, 4, 16, 24, 2, 3)
    x, eps, mass = sc.degrade_case(shape, 1, 1.0)
    n = x.numel()
    buf = torch.full((n + 16,), 3.0, dtype=torch.float16, device=dev)
    out = buf[8:8 + n].view(x.shape)
    xd, ed = x.to(dev), eps.to(dev)
    f32 = lambda v: torch.tensor(np.asarray(v, dtype=np.float32), device=dev)
    md, rd, td, cd = f32(mass), f32((1.0,)), f32(sc.taps(1.0)), f32(sc.coef_of(0.3))
    keep = [t.clone() for t in (xd, ed, md, rd, td, cd)]
    assert ops.sag_degrade(xd, ed, md, rd, td, cd, 2, 3, out=out).data_ptr() == out.data_ptr()
    assert bool((buf[:8] == 3.0).all()) and bool((buf[8 + n:] == 3.0).all())
    assert all(torch.equal(a, b) for a, b in zip(keep, (xd, ed, md, rd, td, cd)))
    assert torch.equal(bits(out), bits(ops.sag_degrade(xd, ed, md, rd, td, cd, 2, 3)))
    B, C, H, W, Hm, Wm = sc.DEGRADE_REFUSED
    z = torch.zeros((B, C, H, W), dtype=torch.float16, device=dev)
    with pytest.raises(ValueError, match="sag_degrade"):
        ops.sag_degrade(z, z.clone(), torch.zeros((1, B, 1), dtype=torch.float32, device=dev), rd, td, cd, Hm, Wm)
    with pytest.raises(ops.VdHipError, match="sag_degrade"):
        ops.sag_degrade(xd, ed, md, rd, td[:8], cd, 2, 3)
    with pytest.raises(ops.VdHipError, match="sag_degrade"):
        ops.sag_degrade(xd, ed, md, rd, td, cd, 3, 3)


# ---- 3. the fold -----------------------------------------------------------------------------------------------------------------

def test_fold_exact_operands_give_the_float64_formula_bit_for_bit(dev):
    from vd_hip import ops
    g = torch.Generator().manual_seed(19)
    for n in pc.FOLD_SIZES:
        host = torch.randint(-8, 9, (3, n), generator=g).half()
        e_d = torch.randint(-8, 9, (n,), generator=g).half()
        for j, w in enumerate(pc.FOLD_WEIGHTS if n < (1 << 20) else pc.FOLD_WEIGHTS[:1]):
            ref = sc.fold_ref64(host[0], e_d, w)
            assert torch.equal(ref.half().double(), ref)                                    # an fp16 value
            # aligned, and (odd j) starting one element into a buffer: nothing is 16-byte aligned, n % 8 or not
            buf = torch.zeros((3 * n + 1,), dtype=torch.float16, device=dev)
            eps = buf[j % 2:j % 2 + 3 * n].view(3, n)
            eps.copy_(host)
            dbuf = torch.zeros((n + 1,), dtype=torch.float16, device=dev)
            dd = dbuf[j % 2:j % 2 + n]
            dd.copy_(e_d)
            wd = torch.full((1,), w, dtype=torch.float32, device=dev)
            assert ops.sag_fold(eps, dd.view(1, n), wd).data_ptr() == eps.data_ptr()
            assert torch.equal(bits(eps[0]), bits(ref.half())), (n, w)
            assert torch.equal(bits(eps[1:]), bits(host[1:])) and torch.equal(bits(dd), bits(e_d)), (n, w, "nothing else is written")
            assert float(wd.item()) == w and float(buf[-1 if j % 2 == 0 else 0].item()) == 0.0


def test_fold_weight_zero_keeps_the_bits(dev):
    from vd_hip import ops
    g = torch.Generator().manual_seed(29)
    wd = lambda w: torch.full((1,), w, dtype=torch.float32, device=dev)
    host = torch.randn((4, 4, 16, 16), generator=g).half()
    host[0, 0, 0, :4] = torch.tensor([-0.0, 0.0, 65504.0, -6e-8]).half()
    e_d = torch.randn((2, 4, 16, 16), generator=g).half()
    eps = host.to(dev)
    ops.sag_fold(eps, e_d.to(dev), wd(0.0))
    assert torch.equal(bits(eps), bits(host))
    ops.sag_fold(eps, e_d.to(dev), wd(-0.1154))
    assert not torch.equal(bits(eps[:2]), bits(host[:2])) and torch.equal(bits(eps[2:]), bits(host[2:]))
    ref = sc.fold_ref64(host[:2], e_d, -0.1154)
    assert float((eps[:2].double().cpu() - ref).abs().max()) <= 2.0 ** -10 * float(ref.abs().max())
    with pytest.raises(ops.VdHipError, match="sag_fold"):
        ops.sag_fold(eps, e_d[:, :3].contiguous().to(dev), wd(1.0))
    with pytest.raises(ops.VdHipError, match="sag_fold"):
        ops.sag_fold(eps[:3], e_d.to(dev), wd(1.0))


# ---- 4. the forward --------------------------------------------------------------------------------------------------------------

def _inputs(seed, B, dual, guided):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B,) + tuple(SHAPE[1:]), generator=g).half().float()
    rows = lambda L: (torch.randn(((2 if guided else 1) * B, L, 128), generator=g) * 0.5).half().float()
    ctx = [("text", rows(77), 0.4 if dual else 1.0)]
    if dual:
        ctx.append(("image", rows(50), 0.6))
    return x, ctx


def _fwd(net, dev, x, t, ctx, reps, **keys):
    x_info = dict({"type": "image", "x": x.half().to(dev), "repeat": reps}, **keys)
    ts = torch.full((reps * x.shape[0],), t, dtype=torch.long, device=dev)
    if len(ctx) == 1:
        return net.apply_model(x_info, ts, {"type": ctx[0][0], "c": ctx[0][1].half().to(dev)})
    return net.apply_model_multicontext(x_info, ts, [{"type": ct, "c": c.half().to(dev), "ratio": r} for ct, c, r in ctx])


@pytest.mark.parametrize("fork", [True, False], ids=["fork", "serial"])
@pytest.mark.parametrize("dual", [False, True], ids=["single", "dual"])
def test_forward_keeps_its_bits_and_writes_the_mass_of_the_middle_attn1(tiny, plan, dev, monkeypatch, dual, fork):
    from lib.model_zoo import vd
    from vd_hip import ops
    net, sd = tiny
    monkeypatch.setattr(vd, "CTX_FORK", fork)
    B, T = SHAPE[0], 2 if dual else 1
    Nm = sc.TINY_MAP[0] * sc.TINY_MAP[1]
    assert vd.sag_map_size(net.diffuser["image"], SHAPE[2], SHAPE[3]) == sc.TINY_MAP
    worst = 0.0
    for guided in (True, False):
        reps = 2 if guided else 1
        x, ctx = _inputs(71 + dual + 2 * guided, B, dual, guided)
        plain = _fwd(net, dev, x, 500, ctx, reps)
        seen, real = [], ops.attention

        def recorded(q, k, v, heads, **kw):
            if q.shape[1] == k.shape[1] and q.stride(1) == 3 * q.shape[2]:      # q | k | v of one fused projection: an attn1
                seen.append((q.clone(), k.clone(), heads, kw.get("scale")))
            return real(q, k, v, heads, **kw)

        monkeypatch.setattr(ops, "attention", recorded)
        mass = torch.full((T, B, Nm), -1.0, dtype=torch.float32, device=dev)
        e = _fwd(net, dev, x, 500, ctx, reps, sag=mass)
        monkeypatch.setattr(ops, "attention", real)
        assert torch.equal(bits(e), bits(plain))                                 # the attention itself is untouched
        assert len(seen) == pc.TINY_BLOCKS * T
        oracle = sc.walk(sd, plan, torch.cat([x] * reps), torch.full((reps * B,), 500, dtype=torch.long), ctx)[1]
        for t in range(T):
            q, k, heads, scale = seen[pc.TINY_MID * T + t]
            assert q.shape[0] == reps * B and q.shape[1] == Nm
            ref = sc.mass_ref64(q[:B].cpu(), k[:B].cpu(), heads, scale).numpy()
            got = mass[t].double().cpu().numpy()
            assert (np.abs(got - ref) <= sc.mass_bound(ref)).all(), (guided, t)
            assert (np.abs(got.sum(1) - Nm) <= 2.0 ** -16 * Nm).all()
            diff = float(np.abs(got - oracle[t][:B].numpy()).max())
            worst = max(worst, diff)
            print("dual %d fork %d guided %d type %d: max |device mass - oracle mass| %.3e; masses in [%.3f, %.3f]"
                  % (dual, fork, guided, t, diff, got.min(), got.max()))
        assert torch.equal(f32bits(mass), f32bits(_mass_again(net, dev, x, ctx, reps, T, B, Nm)))
    assert worst <= sc.MASS_DIFF_MEASURED       # the recorded device-vs-oracle difference that MASS_MARGIN is four times of


def _mass_again(net, dev, x, ctx, reps, T, B, Nm):
    mass = torch.zeros((T, B, Nm), dtype=torch.float32, device=dev)
    _fwd(net, dev, x, 500, ctx, reps, sag=mass)
    return mass


def test_forward_mass_is_the_same_inside_the_half_batch_fork(tiny, dev, monkeypatch):
    """VD_BATCH_FORK=1 semantics with the threshold lowered to 64 rows per sample: the 8 x 8 level and the middle block run as two
    half-batch branches.  Guided, B = 2: the first branch holds exactly replica 0; unguided, B = 4: each branch writes two rows."""
    from lib.model_zoo import vd
    net, _ = tiny
    Nm = sc.TINY_MAP[0] * sc.TINY_MAP[1]
    for guided, B in ((True, 2), (False, 4)):
        reps = 2 if guided else 1
        x, ctx = _inputs(91, B, False, guided)
        monkeypatch.setattr(vd, "BATCH_FORK", "0")
        whole = _mass_again(net, dev, x, ctx, reps, 1, B, Nm)
        plain = _fwd(net, dev, x, 500, ctx, reps)
        monkeypatch.setattr(vd, "BATCH_FORK", "1")
        monkeypatch.setattr(vd, "BATCH_FORK_HW", 64)
        forked = _mass_again(net, dev, x, ctx, reps, 1, B, Nm)
        assert bool((forked > 0).all()) and float((forked - whole).abs().max()) <= 4 * sc.MASS_DIFF_MEASURED
        assert (np.abs(forked.double().sum(2).cpu().numpy() - Nm) <= 2.0 ** -16 * Nm).all()
        assert rel_l2(_fwd(net, dev, x, 500, ctx, reps), plain) < 1e-3


def test_forward_key_is_validated(tiny, dev):
    net, _ = tiny
    x, ctx = _inputs(3, 2, False, False)
    Nm = sc.TINY_MAP[0] * sc.TINY_MAP[1]
    for bad in (torch.zeros((1, 2, Nm), device=dev, dtype=torch.float16), torch.zeros((2, 2, Nm), device=dev), torch.zeros((1, 3, Nm), device=dev),
                torch.zeros((1, 2, Nm + 1), device=dev), torch.zeros((1, 2, Nm)), "mass"):
        with pytest.raises(ValueError, match="sag"):
            _fwd(net, dev, x, 500, ctx, 1, sag=bad)


# ---- 5. loops --------------------------------------------------------------------------------------------------------------------

def _make(kind, net, **kw):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    from lib.model_zoo.unipc import UniPCSampler
    return {"ddim": DDIMSampler, "2m": DPMSolverSampler, "unipc": UniPCSampler, "sde": DPMSolverSDESampler}[kind](net, **kw)


def _on_dev(c, dev):
    return dict(c, conditioning=c["conditioning"].half().to(dev), unconditional_conditioning=c["unconditional_conditioning"].half().to(dev))


def _sample(sampler, dev, scale=7.5, c_keys=None, call=None, kind=None, case=("ddim", 7.5), **keys):
    """One sample() call on the inputs of the loop case `case` (sag_cases.LOOP_SEED)."""
    xT = sc.loop_inputs(case)[0]
    if kind == "sde":
        keys = dict({"seeds": sc.LOOP_SEEDS}, **keys)
    x_info = dict({"type": "image", "xt": xT.half().to(dev)}, **keys)
    return sampler.sample(steps=STEPS, shape=list(xT.shape), x_info=x_info, c_info=_on_dev(sc.loop_context(case, scale, **(c_keys or {})), dev),
                          verbose=False, **(call or {}))


def _check_loop(sd, plan, sampler, kind, scale, z, case, **kw):
    what = str(case)
    margin = []
    xT, cs = sc.loop_inputs(case)[0], [sc.loop_context(case, scale)]
    ref = sc.oracle_loop(sd, plan, sampler, kind, xT, cs, scale, SAG_SCALE, margin=margin, **kw)
    off = sc.oracle_loop(sd, plan, sampler, kind, xT, cs, scale, 0.0, **kw)
    err, gap = rel_l2(z, ref), rel_l2(ref, off)
    print("%s: final latent vs the oracle loop with SAG %.3e; oracle loop on vs off %.3e; latent vs the oracle loop off %.3e; least "
          "|mass - 1| over the steps %.3e" % (what, err, gap, rel_l2(z, off), min(margin)))
    assert len(margin) == STEPS and min(margin) >= sc.MASS_MARGIN       # precondition, on the oracle alone (also in test_sag_cpu.py)
    assert err < LATENT_TOL
    return err, gap


@pytest.mark.parametrize("scale", sc.LOOP_SCALES)
@pytest.mark.parametrize("kind", sc.LOOP_KINDS)
def test_loops_vs_the_oracle_loop(tiny, plan, dev, kind, scale):
    net, sd = tiny
    sampler = _make(kind, net)
    z, inter = _sample(sampler, dev, scale, kind=kind, case=(kind, scale), sag_scale=SAG_SCALE)
    assert len(sampler.ddim_timesteps) == STEPS and inter["sag_map"] == (4, 4)
    noise = sc.sde_noise() if kind == "sde" else None
    err, gap = _check_loop(sd, plan, sampler, kind, scale, z, (kind, scale), noise=noise)
    assert gap > err                                                    # the loop follows the guided oracle, not the plain one


@pytest.mark.parametrize("kind", sc.LOOP_KINDS)
def test_graph_replay_eager_bodies_scales_and_off_calls(tiny, dev, kind):
    net, _ = tiny
    shared = _make(kind, net)
    run = lambda s, **keys: _sample(s, dev, kind=kind, **keys)
    z_off0, i_off = run(shared)                                         # before any call with the key
    z_on, _ = run(shared, sag_scale=SAG_SCALE)
    z_off, _ = run(shared)
    assert torch.equal(z_off, z_off0) and not torch.equal(z_on, z_off) and "sag_map" not in i_off
    assert len(shared._static) == 2 and all(st["graph"] is not None for st in shared._static.values())
    on_state = [st for st in shared._static.values() if "sag" in st]
    assert len(on_state) == 1
    graph = on_state[0]["graph"]
    assert torch.equal(run(shared, sag_scale=SAG_SCALE)[0], z_on)       # on the kept graph
    for off_keys in (dict(sag_scale=0), dict(sag_scale=None, sag_blur_sigma=-1), dict(sag_scale=0.0, sag_blur_sigma=2.0)):
        assert torch.equal(run(shared, **off_keys)[0], z_off)
    # another scale and sigma replay the same kept graph with other buffers' contents
    z_two, _ = run(shared, sag_scale=1.5, sag_blur_sigma=2.0)
    assert len(shared._static) == 2 and on_state[0]["graph"] is graph and [st for st in shared._static.values() if "sag" in st][0] is on_state[0]
    assert not torch.equal(z_two, z_on) and not torch.equal(z_two, z_off)
    assert torch.equal(run(_make(kind, net), sag_scale=SAG_SCALE)[0], z_on)                     # a fresh sampler
    eager = _make(kind, net)
    eager.use_graph = False                                             # eager bodies: every launch of every step on the stream
    assert torch.equal(run(eager, sag_scale=SAG_SCALE)[0], z_on)
    assert torch.equal(run(eager, sag_scale=1.5, sag_blur_sigma=2.0)[0], z_two)
    assert torch.equal(run(eager)[0], z_off)


def test_off_values_keep_the_static_key(tiny, dev):
    net, _ = tiny
    s = _make("ddim", net)
    x = sc.loop_inputs(("ddim", 7.5))[0].half().to(dev)
    c = _on_dev(sc.loop_context(("ddim", 7.5), 7.5), dev)
    cis = s._cfg_contexts([c])[0]
    key = lambda **kw: s._static_key(x, dict({"type": "image"}, **kw), cis, True, True)
    base = key()
    assert key(sag_scale=None) == base and key(sag_scale=0) == base and key(sag_scale=0.0, sag_blur_sigma=3.0) == base
    on = key(sag_scale=SAG_SCALE)
    assert on != base and on[:len(base)] == base and key(sag_scale=2.0, sag_blur_sigma=2.0) == on


def test_eager_ddim_loop_is_the_static_loop_and_single_steps_honour_the_key(tiny, dev):
    """eta = 0 with a noise dropout (which only draws: sigma = 0 takes no noise) runs the eager loop of _step.  That loop computes
    the time embedding inside every forward, so the static loop it is compared with does too (emb_hoist off)."""
    net, _ = tiny
    s = _make("ddim", net)
    s.emb_hoist = False
    z_on = _sample(s, dev, sag_scale=SAG_SCALE)[0]
    z_off = _sample(s, dev)[0]
    e_on, inter = _sample(_make("ddim", net), dev, call={"noise_dropout": 0.25}, sag_scale=SAG_SCALE)
    e_off = _sample(_make("ddim", net), dev, call={"noise_dropout": 0.25})[0]
    print("eager vs static DDIM loop, eta 0: off %.3e on %.3e" % (rel_l2(e_off, z_off), rel_l2(e_on, z_on)))
    assert torch.equal(e_off, z_off) and torch.equal(e_on, z_on) and inter["sag_map"] == (4, 4)
    torch.manual_seed(3)
    z_eta = _sample(_make("ddim", net), dev, call={"eta": 0.5}, sag_scale=SAG_SCALE)[0]
    torch.manual_seed(3)
    assert rel_l2(z_eta, _sample(_make("ddim", net), dev, call={"eta": 0.5})[0]) > 1e-3
    s.make_schedule(STEPS, verbose=False)
    t = torch.full((1,), int(s.ddim_timesteps[STEPS - 1]), dtype=torch.long, device=dev)
    x = sc.loop_inputs(("ddim", 7.5))[0].half().to(dev)
    for scale in sc.LOOP_SCALES:
        c = _on_dev(sc.loop_context(("ddim", 7.5), scale), dev)
        step = lambda **kw: s.p_sample_ddim(dict({"type": "image", "x": x}, **kw), c, t, STEPS - 1)[0]
        on, off = step(sag_scale=SAG_SCALE), step()
        assert torch.equal(step(sag_scale=0), off) and rel_l2(on, off) > 1e-4 and torch.equal(step(sag_scale=SAG_SCALE), on)


# ---- 6. combinations -------------------------------------------------------------------------------------------------------------

def test_with_guidance_rescale_vs_the_oracle_loop(tiny, plan, dev):
    net, sd = tiny
    sampler = _make("ddim", net)
    z, inter = _sample(sampler, dev, c_keys={"guidance_rescale": 0.7}, case="rescale", sag_scale=SAG_SCALE)
    assert len(inter["guidance_rescale"]) >= 1
    _check_loop(sd, plan, sampler, "ddim", 7.5, z, "rescale", phi=0.7)


def test_with_inpainting_vs_the_oracle_loop(tiny, plan, dev):
    net, sd = tiny
    x0, mask = sc.loop_inpaint()
    sampler = _make("2m", net)
    z, _ = _sample(sampler, dev, case="inpaint", sag_scale=SAG_SCALE, x0=x0.half().to(dev), inpaint_mask=mask.half().to(dev))
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(z.cpu()[keep], x0.half()[keep])                  # the known region comes back bit for bit
    _check_loop(sd, plan, sampler, "2m", 7.5, z, "inpaint", inpaint=(x0, mask, sc.loop_inputs("inpaint")[0]))


def test_with_freeu_vs_the_oracle_loop(tiny, plan, dev):
    from freeu_cases import SETTING
    net, sd = tiny
    sampler = _make("2m", net)
    z, _ = _sample(sampler, dev, case="freeu", sag_scale=SAG_SCALE, freeu=SETTING)
    _check_loop(sd, plan, sampler, "2m", 7.5, z, "freeu", setting=SETTING)


def test_refused_combinations_raise(tiny, dev):
    net, _ = tiny
    s = _make("2m", net)
    for keys in (dict(window=8), dict(window=8, region_masks=np.ones((1, 8, 8), np.float32)), dict(cache_interval=2), dict(pag_scale=3.0),
                 dict(tome_ratio=0.5), dict(sag_blur_sigma=0.0), dict(sag_blur_sigma=float("nan"))):
        with pytest.raises(ValueError, match="sag"):
            _sample(s, dev, sag_scale=SAG_SCALE, **keys)
    for bad in (-1.0, float("inf"), "0.75", True):
        with pytest.raises(ValueError, match="sag"):
            _sample(s, dev, sag_scale=bad)
    assert len(s._static) == 0
