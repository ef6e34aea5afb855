"""UniPC on the GPU: the fused CFG + corrector + predictor kernel (vd_cfg_unipc_step_dev_f16 and its _rs twin, through the C
ABI) against an fp64 torch formula, its two loops against each other bit for bit, and UniPCSampler against DDIMSampler
(order 1, no corrector), DPMSolverSampler (order 2, no corrector) and the fp32 CPU oracle driven by the same coefficient
table (orders 2 and 3 with the corrector); graph replay and kept graphs, the RNG contract, inpainting, the guidance rescale
and the sharding helper."""
import ctypes

import numpy as np
import pytest
import torch

from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

LATENT_TOL = 1e-2            # the project's bound on a final latent against the fp32 oracle loop
RTOL, ATOL = 2 ** -10, 2e-4  # of test_dpm_solver_gpu.test_kernel_vs_fp64_formula, for fp16 outputs
SHAPE = [2, 4, 16, 16]
STATE = ("x_last", "m1", "m2", "m3")


def T(a, dev, dtype=torch.float16):
    return torch.from_numpy(np.asarray(a)).to(dev).to(dtype)


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------

def _rows(scale=7.5):
    """Four consecutive rows of an order-3 table (10 uniform steps): step 0 (nothing read), the order-1 corrector with an
    order-2 predictor, the order-2 corrector with an order-3 predictor, and order 3 in both."""
    from lib.model_zoo import unipc
    from lib.model_zoo.diffusion_utils import make_ddim_timesteps
    from oracle import vd_oracle as O
    tab = unipc.unipc_coef_table(O.register_schedule()["alphas_cumprod"].numpy(),
                                 make_ddim_timesteps("uniform", 10, 1000, verbose=False), order=3, scale=scale)
    rows = tab[::-1][:4]
    assert [int(r[unipc.HIST]) for r in rows] == [0, 1, 2, 3] and [int(r[unipc.CORR]) for r in rows] == [0, 1, 1, 1]
    assert rows[1][unipc.C_2] == 0 and rows[1][unipc.P_1] != 0 and rows[1][unipc.P_2] == 0      # corrector 1, predictor 2
    assert rows[2][unipc.C_2] != 0 and rows[2][unipc.C_3] == 0 and rows[2][unipc.P_2] != 0      # corrector 2, predictor 3
    assert rows[3][unipc.C_3] != 0 and rows[3][unipc.P_2] != 0                                  # order 3
    return rows


def _buf(dev, m, dtype, offset, fill=None):
    """a view `offset` elements into a larger allocation: misaligned for offset = 1"""
    base = torch.empty((m + offset,), device=dev, dtype=dtype)
    if fill is not None:
        base.fill_(fill)
    return base[offset:]


def _formula(r, xd, ed, n, guided, st, kf=None):
    """One step in fp64 from the fp32 row r and the state st = [x_last, m1, m2, m3] (fp64): (x_next, m_t, new state)."""
    e = ed[:n] + r[0] * (ed[n:] - ed[:n]) if guided else ed
    if kf is not None:
        e = kf * e
    mt = (xd - r[2] * e) * r[1]
    if r[3] != 0:
        xc = r[4] * st[0] + r[8] * mt
        for c, m in ((r[5], st[1]), (r[6], st[2]), (r[7], st[3])):
            if c != 0:
                xc = xc + c * m
    else:
        xc = xd
    xn = r[9] * xc + r[10] * mt
    for c, m in ((r[11], st[1]), (r[12], st[2])):
        if c != 0:
            xn = xn + c * m
    hist = int(r[13])
    return xn, mt, [xc, mt, st[1] if hist >= 1 else mt, st[2] if hist >= 2 else mt]


def _run_steps(dev, n, guided, offset, alias, seed, kfac=None, per=None, check=True):
    """The four rows of _rows() in turn on one set of buffers whose state starts as NaN.  Returns every output and state of
    every step (for the bitwise comparisons).  kfac: the _rs twin with these factors."""
    from vd_hip import ops
    gen = torch.Generator().manual_seed(seed)
    ne = 2 * n if guided else n
    x = _buf(dev, n, torch.float16, offset)
    x.copy_(torch.randn(n, generator=gen).half())
    p0 = _buf(dev, n, torch.float16, offset)
    state = [_buf(dev, n, torch.float32, offset, float("nan")) for _ in STATE]
    kf64 = None if kfac is None else kfac.double().repeat_interleave(per)
    seen = []
    for row in _rows(7.5 if guided else 1.0):
        r = [float(v) for v in row.astype(np.float64)]
        eps = _buf(dev, ne, torch.float16, offset)
        eps.copy_(torch.randn(ne, generator=gen).half())
        coef = torch.from_numpy(np.ascontiguousarray(row)).to(dev)
        xd, ed, sd = x.double(), eps.double(), [s.double().clone() for s in state]
        x_next = x if alias else _buf(dev, n, torch.float16, offset)
        if kfac is None:
            ops.cfg_unipc_step_dev(x, eps, coef, tuple(state), guided=guided, x_next=x_next, pred_x0=p0)
        else:
            ops.cfg_unipc_step_dev_rs(x.view(-1, per), eps, coef, tuple(state), kfac, guided=guided,
                                      x_next=x_next.view(-1, per), pred_x0=p0)
        torch.cuda.synchronize()
        if check:
            xn, mt, want = _formula(r, xd, ed, n, guided, sd, kf64)
            assert bool(torch.isfinite(x_next).all()) and bool(torch.isfinite(p0).all())
            assert all(bool(torch.isfinite(s).all()) for s in state)
            torch.testing.assert_close(x_next.double(), xn, rtol=RTOL, atol=ATOL)
            torch.testing.assert_close(p0.double(), mt, rtol=RTOL, atol=ATOL)
            for s, w, name in zip(state, want, STATE):
                assert rel_l2(s, w) < 1e-6, (name, r[13])
        seen.append([t.clone() for t in [x_next, p0] + state])
        x = x_next
    return seen


@pytest.mark.parametrize("n,offset", [(65536, 0), (4099, 0), (4099, 1)])
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("alias", [False, True])
def test_kernel_vs_fp64_formula(dev, n, offset, guided, alias):
    _run_steps(dev, n, guided, offset, alias, n + 7 * offset + 3 * guided + alias)


@pytest.mark.parametrize("guided", [True, False])
def test_vector_and_scalar_loops_give_the_same_bits(dev, guided):
    """The same data at offset 0 (16-byte lanes + a 3-element tail) and at offset 1 (the scalar loop throughout)."""
    a = _run_steps(dev, 4099, guided, 0, True, 5, check=False)
    b = _run_steps(dev, 4099, guided, 1, True, 5, check=False)
    for step, (sa, sb) in enumerate(zip(a, b)):
        for ta, tb, name in zip(sa, sb, ("x_next", "pred_x0") + STATE):
            assert torch.equal(ta, tb), (step, name)


def test_rs_twin_factors_of_one_give_the_plain_bits(dev):
    for n, per, offset in ((8 * 4099, 4099, 0), (3 * 4099, 4099, 0), (2 * 16384, 16384, 0), (8 * 4099, 4099, 1)):
        ones = torch.ones((n // per,), device=dev, dtype=torch.float32)
        a = _run_steps(dev, n, True, offset, True, 9, check=False)
        b = _run_steps(dev, n, True, offset, True, 9, kfac=ones, per=per, check=False)
        for sa, sb in zip(a, b):
            assert all(torch.equal(ta, tb) for ta, tb in zip(sa, sb)), (n, per, offset)


@pytest.mark.parametrize("B,per", [(8, 4099), (3, 4099), (2, 16384)])
def test_rs_twin_vs_fp64_formula_and_samples_alone(dev, B, per):
    """Per-sample factors against the formula, and every row of the batch bit for bit what the sample gives when it runs
    alone.  8 x 4099: every stream is 16-byte aligned and lanes of the 16-byte loop straddle samples; 3 x 4099 is odd, so its
    conditional half is not aligned and the scalar loop looks the factor up per element."""
    from vd_hip import ops
    kfac = torch.tensor([0.5, 0.8125, 1.25, 1.0, 0.75, 1.5, 0.625, 0.9375][:B], device=dev)
    batch = _run_steps(dev, B * per, True, 0, False, 21, kfac=kfac, per=per)
    # the same inputs again, sample by sample (the generator of _run_steps draws x, then per step eps = [eu ; ec])
    gen = torch.Generator().manual_seed(21)
    n = B * per
    x = torch.randn(n, generator=gen).half().to(dev).view(B, per)
    state = [torch.full((B, per), float("nan"), device=dev) for _ in STATE]
    for step, row in enumerate(_rows(7.5)):
        eps = torch.randn(2 * n, generator=gen).half().to(dev).view(2, B, per)
        coef = torch.from_numpy(np.ascontiguousarray(row)).to(dev)
        x_next, p0 = torch.empty_like(x), torch.empty_like(x)
        for b in range(B):
            ops.cfg_unipc_step_dev_rs(x[b:b + 1], eps[:, b].contiguous(), coef, tuple(s[b] for s in state), kfac[b:b + 1],
                                      guided=True, x_next=x_next[b:b + 1], pred_x0=p0[b:b + 1])
        torch.cuda.synchronize()
        for alone, both, name in zip([x_next, p0] + state, batch[step], ("x_next", "pred_x0") + STATE):
            assert torch.equal(alone.reshape(-1), both), (step, name)
        x = x_next


def test_argument_checks(dev):
    from vd_hip import VdHipError, ops
    from vd_hip.loader import lib
    n = 64
    x = torch.zeros((2, n // 2), device=dev, dtype=torch.float16)
    eps = torch.zeros((4, n // 2), device=dev, dtype=torch.float16)
    coef = torch.from_numpy(np.ascontiguousarray(_rows()[0])).to(dev)
    st = tuple(torch.zeros((n,), device=dev) for _ in STATE)
    kfac = torch.ones((2,), device=dev)
    ops.cfg_unipc_step_dev(x, eps, coef, st, guided=True, x_next=x)                    # the well-formed calls pass
    ops.cfg_unipc_step_dev_rs(x, eps, coef, st, kfac, guided=True, x_next=x)
    for bad in (lambda: ops.cfg_unipc_step_dev(x, eps[:2], coef, st, guided=True, x_next=x),
                lambda: ops.cfg_unipc_step_dev(x, eps, coef[:13], st, guided=True, x_next=x),
                lambda: ops.cfg_unipc_step_dev(x, eps, coef, st[:3], guided=True, x_next=x),
                lambda: ops.cfg_unipc_step_dev(x, eps, coef, (st[0], st[1], st[1], st[3]), guided=True, x_next=x),
                lambda: ops.cfg_unipc_step_dev(x, eps, coef, (st[0].half(),) + st[1:], guided=True, x_next=x),
                lambda: ops.cfg_unipc_step_dev(x, eps, coef, (st[0][:8],) + st[1:], guided=True, x_next=x),
                lambda: ops.cfg_unipc_step_dev(x, eps, coef.cpu(), st, guided=True, x_next=x),
                lambda: ops.cfg_unipc_step_dev_rs(x, eps[:2], coef, st, kfac, guided=False, x_next=x),
                lambda: ops.cfg_unipc_step_dev_rs(x, eps, coef, st, kfac[:1], guided=True, x_next=x),
                lambda: ops.cfg_unipc_step_dev_rs(x, eps, coef, st, kfac.half(), guided=True, x_next=x)):
        with pytest.raises(VdHipError):
            bad()
    # the C ABI itself: negative codes with a message
    h, p = lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    s = [p(t) for t in st]
    plain, rs = h.vd_cfg_unipc_step_dev_f16, h.vd_cfg_unipc_step_dev_rs_f16
    assert plain(None, p(eps), *s, p(x), None, n, 1, p(coef), None) < 0 and b"vd_cfg_unipc_step_dev_f16" in h.vd_last_error()
    assert plain(p(x), p(eps), s[0], None, s[2], s[3], p(x), None, n, 1, p(coef), None) < 0
    assert plain(p(x), p(eps), *s, p(x), None, 0, 1, p(coef), None) < 0
    assert plain(p(x), p(eps), *s, p(x), None, n, 1, None, None) < 0
    assert plain(p(x), p(eps), s[0], s[1], s[1], s[3], p(x), None, n, 1, p(coef), None) < 0
    assert b"four buffers" in h.vd_last_error()
    assert rs(p(x), p(eps), *s, p(x), None, n, n // 2, 1, p(coef), None, None) < 0
    assert rs(p(x), p(eps), *s, p(x), None, n, n // 2, 0, p(coef), p(kfac), None) < 0 and b"guided" in h.vd_last_error()
    assert rs(p(x), p(eps), *s, p(x), None, n, 0, 1, p(coef), p(kfac), None) < 0
    assert rs(p(x), p(eps), *s, p(x), None, n, 24, 1, p(coef), p(kfac), None) < 0 and b"multiple" in h.vd_last_error()
    assert rs(p(x), p(eps), s[0], s[0], s[2], s[3], p(x), None, n, n // 2, 1, p(coef), p(kfac), None) < 0
    torch.cuda.synchronize()


# ---- 2. the sampler -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny(dev):
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    sd = synth_into(net, m["seed"])
    net = net.half()
    net.to(dev)
    return net, sd


@pytest.fixture(scope="module")
def gold():
    return load_gold("ddim_tiny.npz")


def _ci(c, u, scale, ctype="text", **kw):
    return dict({"type": ctype, "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale},
                **kw)


def _on_dev(c, dev):
    return dict(c, conditioning=c["conditioning"].half().to(dev),
                unconditional_conditioning=c["unconditional_conditioning"].half().to(dev))


def _oracle_unipc(sd, plan, sampler, xT, contexts, scale, x_type="image", phi=0.):
    """The solver loop in fp32 on the CPU oracle, driven by the table the sampler used for its last call; phi > 0 inserts the
    guidance rescale of ddim.cfg_rescale_factors after the guidance combine."""
    from lib.model_zoo.ddim import cfg_rescale_factors
    from lib.model_zoo.unipc import unipc_coef_table
    from oracle import vd_oracle as O
    ts = sampler.ddim_timesteps
    tab = unipc_coef_table(sampler.alphas_cumprod, ts, order=sampler.order, corrector=sampler.corrector,
                           lower_order_final=sampler.lower_order_final, scale=scale)
    x = xT.float()
    xl = m1 = m2 = m3 = None
    cs = [(c["type"], torch.cat([c["unconditional_conditioning"], c["conditioning"]]).float(), c.get("ratio", 1.0))
          for c in contexts]
    for i in reversed(range(len(ts))):
        r = [float(v) for v in tab[i]]
        t = torch.full((2 * x.shape[0],), int(ts[i]), dtype=torch.long)
        with torch.no_grad():
            eps = O.apply_model_multicontext(sd, plan, torch.cat([x, x]), t, cs, x_type, "image")
        e_u, e_c = eps.chunk(2)
        e = e_u + r[0] * (e_c - e_u)
        if phi > 0:
            e = cfg_rescale_factors(eps, scale, phi).float().view([-1] + [1] * (x.dim() - 1)) * e
        mt = (x - r[2] * e) * r[1]
        xc = x
        if r[3] != 0:
            xc = r[4] * xl + r[8] * mt
            for c, m in ((r[5], m1), (r[6], m2), (r[7], m3)):
                if c != 0:
                    xc = xc + c * m
        xn = r[9] * xc + r[10] * mt
        for c, m in ((r[11], m1), (r[12], m2)):
            if c != 0:
                xn = xn + c * m
        xl, m1, m2, m3, x = xc, mt, m1, m2, xn
    return x


def _t2i(sampler, xT, c, u, scale, steps, **kw):
    x_info = {"type": "image"}
    if xT is not None:
        x_info["xt"] = xT
    z, _ = sampler.sample(steps=steps, shape=list(c.shape[:1]) + SHAPE[1:], x_info=x_info, c_info=_ci(c, u, scale, **kw),
                          verbose=False)
    return z


def _case(dev, seed, shape=tuple(SHAPE)):
    g = torch.Generator().manual_seed(seed)
    xT = torch.randn(shape, generator=g).half().to(dev)
    c = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half().to(dev)
    u = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half().to(dev)
    return xT, c, u


def test_order1_without_corrector_reproduces_ddim(tiny, dev, gold):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.unipc import UniPCSampler
    net, _ = tiny
    xT = T(gold["xT"], dev)
    ct = _ci(T(gold["c_text"], dev), T(gold["u_text"], dev), 7.5)
    run = lambda s: s.sample(steps=6, shape=SHAPE, x_info={"type": "image", "xt": xT}, c_info=dict(ct), verbose=False)
    z_ddim, i_ddim = run(DDIMSampler(net))
    z, inter = run(UniPCSampler(net, order=1, corrector=False))
    assert z.shape == z_ddim.shape and rel_l2(z, z_ddim) < 2e-3
    assert rel_l2(inter["pred_x0"][-1], i_ddim["pred_x0"][-1]) < 2e-3
    assert len(inter["pred_xt"]) == len(i_ddim["pred_xt"])


def test_order2_without_corrector_reproduces_2m(tiny, dev, gold):
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    from lib.model_zoo.unipc import UniPCSampler
    net, _ = tiny
    xT = T(gold["xT"], dev)
    ct = _ci(T(gold["c_text"], dev), T(gold["u_text"], dev), 7.5)
    run = lambda s: s.sample(steps=10, shape=SHAPE, x_info={"type": "image", "xt": xT}, c_info=dict(ct), verbose=False)
    z_2m, i_2m = run(DPMSolverSampler(net))
    z, inter = run(UniPCSampler(net, order=2, corrector=False))
    assert rel_l2(z, z_2m) < 2e-3
    assert rel_l2(inter["pred_x0"][-1], i_2m["pred_x0"][-1]) < 2e-3
    print("UniPC-2 vs 2M, 10 steps: rel-L2 %.3e without the corrector, %.3e with it"
          % (rel_l2(z, z_2m), rel_l2(run(UniPCSampler(net, order=2))[0], z_2m)))


@pytest.mark.parametrize("order", [2, 3])
def test_corrected_orders_tiny_vs_oracle(tiny, dev, gold, order):
    from lib.model_zoo.unipc import UniPCSampler
    from oracle import vd_oracle as O
    net, sd = tiny
    plan = O.unet_plan(**meta()["unet2d"])
    xT = torch.from_numpy(gold["xT"]).float()
    ct = _ci(torch.from_numpy(gold["c_text"]), torch.from_numpy(gold["u_text"]), 7.5)
    sampler = UniPCSampler(net, order=order)
    z, inter = sampler.sample(steps=10, shape=SHAPE, x_info={"type": "image", "xt": xT.half().to(dev)},
                              c_info=_on_dev(ct, dev), verbose=False)
    err = rel_l2(z, _oracle_unipc(sd, plan, sampler, xT, [ct], 7.5))
    print("10-step UniPC order %d rel-L2 vs the fp32 oracle loop: %.3e" % (order, err))
    assert err < LATENT_TOL
    assert len(inter["pred_x0"]) == 2 and inter["pred_x0"][-1].shape == z.shape


def test_dual_context_and_text_latent_vs_oracle(tiny, dev, gold):
    """One dual-context call, and one call on the 0-D text latent ([B, D]: D = 768 at full width, 128 on the tiny model)."""
    from lib.model_zoo.unipc import UniPCSampler
    from oracle import vd_oracle as O
    net, sd = tiny
    m = meta()
    xT = torch.from_numpy(gold["xT"]).float()
    ct = _ci(torch.from_numpy(gold["c_text"]), torch.from_numpy(gold["u_text"]), 7.5)
    ci = _ci(torch.from_numpy(gold["c_img"]), torch.from_numpy(gold["u_img"]), 7.5, "image")
    mc = [dict(ct, ratio=0.4), dict(ci, ratio=0.6)]
    sampler = UniPCSampler(net)
    z, _ = sampler.sample_multicontext(steps=10, shape=SHAPE, x_info={"type": "image", "xt": xT.half().to(dev)},
                                       c_info_list=[_on_dev(c, dev) for c in mc], verbose=False)
    assert rel_l2(z, _oracle_unipc(sd, O.unet_plan(**m["unet2d"]), sampler, xT, mc, 7.5)) < LATENT_TOL
    g0 = load_gold("unet0d_tiny.npz")
    c0 = torch.from_numpy(g0["c_img"])
    c0 = _ci(c0, torch.zeros_like(c0), 4.0, "image")
    x0d = torch.randn((2, 128), generator=torch.Generator().manual_seed(31))
    z, _ = sampler.sample(steps=10, shape=[2, 128], x_info={"type": "text", "xt": x0d.half().to(dev)}, c_info=_on_dev(c0, dev),
                          verbose=False)
    assert z.shape == (2, 128)
    assert rel_l2(z, _oracle_unipc(sd, O.unet0d_plan(**m["unet0d"]), sampler, x0d, [c0], 4.0, x_type="text")) < LATENT_TOL


def test_x0_forward_flow_ends_where_the_oracle_loop_ends(tiny, dev, gold):
    """x0 + x0_forward_timesteps (unguided, image context): the shortened schedule gets its own table."""
    from lib.model_zoo.unipc import UniPCSampler
    from oracle import vd_oracle as O
    net, sd = tiny
    ci = _ci(torch.from_numpy(gold["c_img"]), torch.from_numpy(gold["u_img"]), 7.5, "image")
    sampler = UniPCSampler(net)
    x0, noise = torch.from_numpy(gold["x0"]).float(), torch.from_numpy(gold["q_noise"]).float()
    z, _ = sampler.sample(steps=10, shape=SHAPE, x_info={"type": "image", "x0": x0.half().to(dev), "x0_forward_timesteps": 6,
                                                         "x0_noise": noise.half().to(dev)},
                          c_info=_on_dev(ci, dev), verbose=False)
    k = 6
    a = float(np.float32(sampler.alphas_cumprod[sampler.ddim_timesteps[k]]))
    xk = (np.sqrt(a) * x0.half().float() + np.sqrt(1 - a) * noise.half().float())
    sampler.ddim_timesteps = sampler.ddim_timesteps[:k]          # the loop the call walked
    ref = _oracle_unipc(sd, O.unet_plan(**meta()["unet2d"]), sampler, xk, [ci], 7.5)
    assert rel_l2(z, ref) < LATENT_TOL


def test_graph_replay_matches_eager_bitwise(tiny, dev, monkeypatch):
    from lib.model_zoo.unipc import UniPCSampler
    net, _ = tiny
    xT, c, u = _case(dev, 5)
    z_graph = _t2i(UniPCSampler(net, order=3), xT, c, u, 7.5, 8)
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = UniPCSampler(net, order=3)
    assert not eager.use_graph
    assert torch.equal(z_graph, _t2i(eager, xT, c, u, 7.5, 8))


def test_kept_graph_reused_with_other_steps_latent_and_context(tiny, dev):
    """Call 2 on the kept graph (another step count, latent, context and scale) == a fresh sampler: no state is read on the
    first step of a call, the coefficient rows and the static inputs are refreshed in place."""
    from lib.model_zoo.unipc import UniPCSampler
    net, _ = tiny
    shared = UniPCSampler(net, order=3)
    a, b = _case(dev, 6), _case(dev, 7)
    z_a = _t2i(shared, *a, 7.5, 6)
    st = next(iter(shared._static.values()))
    graph = st["graph"]
    assert graph is not None and st["coef"].numel() == 16
    assert all(st[k].dtype == torch.float32 and st[k].shape == st["xs"].shape for k in STATE)
    z_b = _t2i(shared, *b, 3.0, 10)
    assert len(shared._static) == 1 and st["graph"] is graph       # replayed, not captured again
    assert torch.equal(z_b, _t2i(UniPCSampler(net, order=3), *b, 3.0, 10))
    assert torch.equal(z_a, _t2i(UniPCSampler(net, order=3), *a, 7.5, 6))
    assert rel_l2(z_a, z_b) > 0.1


def test_interleaved_with_ddim_and_2m_on_one_model(tiny, dev):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    from lib.model_zoo.unipc import UniPCSampler
    net, _ = tiny
    ddim, dpm, uni = DDIMSampler(net), DPMSolverSampler(net), UniPCSampler(net)
    cases = [_case(dev, 20 + k) for k in range(2)]
    runs = lambda k, args, s: (_t2i(s[0], *args, 7.5, 5 + k), _t2i(s[1], *args, 7.5, 6 + k), _t2i(s[2], *args, 7.5, 7 + k))
    first = [runs(k, args, (ddim, uni, dpm)) for k, args in enumerate(cases)]
    again = [runs(k, args, (ddim, uni, dpm)) for k, args in enumerate(cases)]
    for k, args in enumerate(cases):
        assert torch.equal(first[k][1], again[k][1]), k                         # repeatable, bit for bit
        assert torch.equal(first[k][1], _t2i(UniPCSampler(net), *args, 7.5, 6 + k)), k
        # its neighbours, unchanged code, within the bound their own interleaving tests use
        assert rel_l2(first[k][0], _t2i(DDIMSampler(net), *args, 7.5, 5 + k)) < 5e-3, k
        assert rel_l2(first[k][2], _t2i(DPMSolverSampler(net), *args, 7.5, 7 + k)) < 5e-3, k


def test_rng_draws_only_the_initial_latent(tiny, dev, gold):
    from lib.model_zoo.unipc import UniPCSampler
    net, _ = tiny
    torch.manual_seed(77)
    UniPCSampler(net).sample(steps=6, shape=SHAPE, x_info={"type": "image"},
                             c_info=_ci(T(gold["c_text"], dev), T(gold["u_text"], dev), 7.5), verbose=False)
    after = torch.randn(8, device=dev)
    torch.manual_seed(77)
    torch.randn(SHAPE, device=dev, dtype=torch.float16)
    assert torch.equal(after, torch.randn(8, device=dev))


def test_inpainting_returns_the_known_region_bitwise(tiny, dev):
    from lib.model_zoo.unipc import UniPCSampler
    net, _ = tiny
    _, c, u = _case(dev, 9)
    x0 = (torch.randn(SHAPE, generator=torch.Generator().manual_seed(4)) * 0.5).half().to(dev)
    mask = torch.ones((2, 1, 16, 16))
    mask[..., :6, :] = 0                         # keep the top rows
    mask = mask.half().to(dev)
    sampler = UniPCSampler(net)
    z, _ = sampler.sample(steps=6, shape=SHAPE, x_info={"type": "image", "x0": x0, "inpaint_mask": mask},
                          c_info=_ci(c, u, 7.5), verbose=False)
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(z[keep], x0[keep])
    assert rel_l2(z[~keep], x0[~keep]) > 0.1 and bool(torch.isfinite(z).all())
    st = next(iter(sampler._static.values()))
    assert all(bool(torch.isfinite(st[k]).all()) for k in STATE)
    # the state keeps the raw values: in the kept region the last data prediction is not x0
    assert not torch.equal(st["m1"].half()[keep], x0[keep])


def test_guidance_rescale(tiny, dev, gold):
    """phi = 0 is the call without the key, bit for bit; phi = 0.7 against the oracle loop with ddim.cfg_rescale_factors, with
    the conditional context 8 times as large so that the factors are well below 1 (test_cfg_rescale_gpu's set-up)."""
    from lib.model_zoo.unipc import UniPCSampler
    from oracle import vd_oracle as O
    net, sd = tiny
    xT = torch.from_numpy(gold["xT"]).float()
    ct = _ci(torch.from_numpy(gold["c_text"]) * 8.0, torch.from_numpy(gold["u_text"]), 7.5)
    run = lambda s, **kw: s.sample(steps=10, shape=SHAPE, x_info={"type": "image", "xt": xT.half().to(dev)},
                                   c_info=dict(_on_dev(ct, dev), **kw), verbose=False)
    z_plain, i_plain = run(UniPCSampler(net))
    z_zero, i_zero = run(UniPCSampler(net), guidance_rescale=0.)
    assert torch.equal(z_zero, z_plain) and "guidance_rescale" not in i_zero
    sampler = UniPCSampler(net)
    z, inter = run(sampler, guidance_rescale=0.7)
    err = rel_l2(z, _oracle_unipc(sd, O.unet_plan(**meta()["unet2d"]), sampler, xT, [ct], 7.5, phi=0.7))
    print("rescaled 10-step UniPC rel-L2 vs the rescaled oracle loop %.3e, vs phi = 0 %.3e" % (err, rel_l2(z, z_plain)))
    assert err < LATENT_TOL
    assert rel_l2(z, z_plain) > 10 * LATENT_TOL             # the rescale really ran
    assert len(inter["guidance_rescale"]) == 2 and all(bool((k > 0).all()) and bool((k <= 1).all())
                                                       for k in inter["guidance_rescale"])


def test_sharded_world1_matches_direct_sample(tiny, dev, gold):
    from lib.model_zoo import sharded
    from lib.model_zoo.unipc import UniPCSampler
    net, _ = tiny
    ct = _ci(T(gold["c_text"], dev), T(gold["u_text"], dev), 7.5)
    seed, steps = 3, 6
    imgs = sharded.vd_sample_sharded(net, UniPCSampler(net), steps, SHAPE, [dict(ct)], seed, guidance_scale=7.5,
                                     device_generator=True)
    torch.manual_seed(seed + 100)
    z, _ = UniPCSampler(net).sample(steps=steps, shape=SHAPE, x_info={"type": "image"}, c_info=dict(ct), verbose=False)
    ref = net.vae_decode(z, which="image")
    assert imgs.shape == ref.shape and rel_l2(imgs, ref) < 2e-3
