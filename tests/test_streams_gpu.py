"""Cross-stream ordering of the forked UNet branches (vd.run_unet) on the tiny model: the context types of a multi-context
stage (vd.CTX_FORK) and the half-batch branches of the low-resolution levels (vd.BATCH_FORK).

A branch may read a weight pack only once the stream that built it has written it.  The packs are built lazily -- at first
use, after a weight change, at a new embedding mode -- so the tests run those forwards with the race amplifier of
vdtest_util (every pack build first spins ~30 ms on its stream): a missing order then shows as wrong bits on every run.
Kernels and split factors are the same on both sides of each comparison, so the comparisons are bit for bit; each test
also asserts that its geometry is bit-reproducible run to run."""
import pytest
import torch

from vdtest_util import delayed_pack_builds, meta, rel_l2, synth_into, tiny_vd_cfg, unet_middle

pytestmark = pytest.mark.gpu

FWD_TOL = 5e-3


def _tiny(dev, seed):
    """A fresh tiny net (no pack built yet) with the synthetic weights of `seed`; returns (net, fp32 state dict)."""
    from lib.model_zoo import get_model
    net = get_model()(tiny_vd_cfg(meta()), verbose=False)
    sd = synth_into(net, seed)
    net = net.half()
    net.to(dev)
    return net, sd


@pytest.fixture(scope="module")
def tiny(dev):
    return _tiny(dev, meta()["seed"])


def _rand(shape, g, dev, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).half().to(dev)


def _mc(net, x, t, entries, x_type="image"):
    if x_type == "text":
        # the 0-D (text-latent) flow: apply_model_multicontext takes time_embed from diffuser[x_type] as the reference does, and
        # the text diffuser has none -- run_unet with the global layer's embedding reaches the multi-context walk of that flow
        from lib.model_zoo import vd
        with torch.no_grad():
            specs = [(net.diffuser[ty].context_blocks, c, r, None) for ty, c, r in entries]
            return vd.run_unet(net.diffuser["text"], specs, x, net._emb_silu("image", t)).float()
    return net.apply_model_multicontext({"type": x_type, "x": x}, t, [
        {"type": ty, "c": c, "ratio": r} for ty, c, r in entries]).float()


def _ctx_cases(dev):
    g = torch.Generator().manual_seed(41)
    x, x0d = _rand((2, 4, 16, 16), g, dev), _rand((2, 128), g, dev)
    ct, ci1, ci2 = _rand((2, 77, 128), g, dev, 0.5), _rand((2, 257, 128), g, dev, 0.5), _rand((2, 257, 128), g, dev, 0.5)
    t = torch.tensor([741, 301], device=dev)
    return {
        "dual": (x, t, [("text", ct, 0.4), ("image", ci1, 0.6)], "image"),
        "repeated_type": (x, t, [("text", ct, 0.3), ("image", ci1, 0.3), ("image", ci2, 0.4)], "image"),
        "text_latent": (x0d, t, [("text", ct, 0.5), ("image", ci1, 0.5)], "text"),
    }


@pytest.mark.parametrize("case", ["dual", "repeated_type", "text_latent"])
def test_context_fork_equals_sequential_context_types(tiny, dev, monkeypatch, case):
    """vd.CTX_FORK on (types as forked branches on side streams) against off (one after the other on the caller's stream):
    the same kernels with the same split factors, so the same bits -- eager, and captured with torch.cuda.graph and replayed."""
    from lib.model_zoo import vd
    net, _ = tiny
    x, t, entries, x_type = _ctx_cases(dev)[case]
    fwd = lambda: _mc(net, x, t, entries, x_type)
    monkeypatch.setattr(vd, "CTX_FORK", False)
    ref = fwd()
    assert torch.equal(ref, fwd()), "geometry not bit-reproducible run to run"
    monkeypatch.setattr(vd, "CTX_FORK", True)
    assert torch.equal(fwd(), ref)
    fwd()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        cap = fwd()
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, ref)


def test_repeated_context_type_vs_oracle(tiny, dev):
    """apply_model_multicontext with one context type listed twice (two differently weighted image contexts: legal in the
    reference's API) against the fp32 oracle."""
    from oracle import vd_oracle as O
    net, sd = tiny
    x, t, entries, _ = _ctx_cases(dev)["repeated_type"]
    with torch.no_grad():
        ref = O.apply_model_multicontext(sd, O.unet_plan(**meta()["unet2d"]), x.float().cpu(), t.cpu(),
                                         [(ty, c.float().cpu(), r) for ty, c, r in entries])
    assert rel_l2(_mc(net, x, t, entries), ref) < FWD_TOL


def test_repeated_context_type_on_a_fresh_net(dev, monkeypatch):
    """First forward of a fresh net is text + image + image: the image SpatialTransformer sits in two branches, and the one
    that meets it first builds its packs on its own stream; the other branch must start behind that build."""
    from lib.model_zoo import vd
    x, t, entries, _ = _ctx_cases(dev)["repeated_type"]
    net, _ = _tiny(dev, 5101)
    with delayed_pack_builds() as amp:
        out = _mc(net, x, t, entries)
    assert amp.builds > 0
    monkeypatch.setattr(vd, "CTX_FORK", False)
    ref = _mc(net, x, t, entries)
    assert torch.equal(ref, _mc(net, x, t, entries)), "geometry not bit-reproducible run to run"
    assert torch.equal(out, ref)


def _count_batch_forks(monkeypatch):
    """Counts the half-batch forks run_unet takes (each asks for its side stream)."""
    from lib.model_zoo import vd
    n = [0]
    real = vd._side_streams

    def spy(device, k, kind="ctx"):
        n[0] += kind == "batch"
        return real(device, k, kind)
    monkeypatch.setattr(vd, "_side_streams", spy)
    return n


def _batch_fork_inputs(dev, same_t=False):
    g = torch.Generator().manual_seed(43)
    x, c = _rand((4, 4, 32, 32), g, dev), _rand((4, 77, 128), g, dev, 0.5)   # 32x32: the 16x16 level is the fork region
    t = torch.full((4,), 601, device=dev) if same_t else torch.tensor([741, 741, 301, 301], device=dev)
    return x, t, c


def _edit(net, how, seed):
    if how == "load_state_dict":
        from oracle import synth
        missing, unexpected = net.load_state_dict(synth.synth_state_dict(synth.shapes_of(net), seed), strict=False)
        assert not unexpected
    else:
        rb, st = unet_middle(net.diffuser["image"])
        with torch.no_grad():
            rb.in_layers[2].weight.mul_(0.75)
            st.transformer_blocks[0].ff.net[2].weight.mul_(1.25)


@pytest.mark.parametrize("how", ["load_state_dict", "in_place"])
def test_half_batch_fork_after_a_weight_change(dev, monkeypatch, how):
    """vd.BATCH_FORK after the weights of the fork region changed on a warm net: the main branch rebuilds the packs on its
    stream, and the side branch must read the rebuilt ones.  The first forward after the change equals the second bit for
    bit, and the second equals the unforked forward of a fresh net with the same weights (other split factors: FWD_TOL)."""
    from lib.model_zoo import vd
    x, t, c = _batch_fork_inputs(dev)
    fwd = lambda n: n.apply_model({"type": "image", "x": x}, t, {"type": "text", "c": c}).float()
    net, _ = _tiny(dev, 5201)
    monkeypatch.setattr(vd, "BATCH_FORK", "0")
    r0 = fwd(net)
    assert torch.equal(r0, fwd(net)), "geometry not bit-reproducible run to run"
    monkeypatch.setattr(vd, "BATCH_FORK", "1")
    forks = _count_batch_forks(monkeypatch)
    fwd(net)
    assert forks[0] == 1
    _edit(net, how, 5202)
    with delayed_pack_builds() as amp:
        first = fwd(net)
    assert amp.builds > 0
    second = fwd(net)
    assert forks[0] == 3
    assert torch.equal(first, second)
    fresh, _ = _tiny(dev, 5201)
    _edit(fresh, how, 5202)
    monkeypatch.setattr(vd, "BATCH_FORK", "0")
    ref = fwd(fresh)
    assert not torch.equal(ref, r0)   # (the edit reached the forward)
    assert rel_l2(second, ref) < FWD_TOL


def test_half_batch_fork_when_the_embedding_mode_changes(dev, monkeypatch):
    """A geometry warmed through x_info['emb_rows'] (what DDIMSampler passes) and then run as a plain apply_model builds each
    ResBlock's "b1" bias pack inside the forked forward; the side branch must read it built."""
    from lib.model_zoo import vd
    x, t, c = _batch_fork_inputs(dev, same_t=True)
    net, _ = _tiny(dev, 5301)
    pre = net.precompute_step_emb("image", t[:1])
    rows = {di: pre[0][0][o:o + n] for di, (o, n) in pre[1].items()}
    hoisted = lambda: net.apply_model({"type": "image", "x": x, "emb_rows": rows}, t, {"type": "text", "c": c}).float()
    plain = lambda: net.apply_model({"type": "image", "x": x}, t, {"type": "text", "c": c}).float()
    monkeypatch.setattr(vd, "BATCH_FORK", "0")
    assert torch.equal(hoisted(), hoisted()), "geometry not bit-reproducible run to run"
    monkeypatch.setattr(vd, "BATCH_FORK", "1")
    forks = _count_batch_forks(monkeypatch)
    warm = hoisted()
    with delayed_pack_builds() as amp:
        out = plain()
    assert amp.builds > 0
    again = plain()
    assert forks[0] == 3
    assert torch.equal(out, again)
    assert rel_l2(out, warm) < 2e-3   # the two embedding modes agree to fp16 rounding of the bias sums
