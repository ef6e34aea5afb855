"""The context K/V cache protocol of lib/model_zoo/vd.py (kv_lookup / kv_mark_stale / kv_refreshable / kv_refresh) on CPU
tensors with a fake context block: what the sampler's kept step graph relies on -- a new context refills the SAME storage,
by the next forward's lookup or by the up-front refresh, and every entry is projected exactly once per context."""
import torch


class _Attn:
    """Stands in for the SpatialTransformer of a context block: project_context(c) -> a new [B, L, 2] tensor."""

    def __init__(self, gain):
        self.gain, self.calls = gain, 0

    def project_context(self, c):
        self.calls += 1
        return torch.stack([c.sum(-1) * self.gain, c.mean(-1) - self.gain], dim=-1)


def _blocks():
    return [[_Attn(2.0)], [_Attn(-3.0)]]     # a context block is indexable; [0] projects


def _ctx(seed):
    return torch.randn((2, 5, 8), generator=torch.Generator().manual_seed(seed))


def test_first_use_projects_once_and_caches():
    from lib.model_zoo.vd import kv_lookup, kv_refreshable
    blocks, c = _blocks(), _ctx(1)
    assert kv_lookup(None, blocks[0], c) is None and blocks[0][0].calls == 0      # no cache: the block projects for itself
    cache = {}                                                                     # what callers hand in as c_info['kv_cache']
    assert not kv_refreshable(cache)
    first = [kv_lookup(cache, b, c) for b in blocks]
    for b, kv in zip(blocks, first):
        assert torch.equal(kv, _Attn(b[0].gain).project_context(c))
    assert kv_refreshable(cache)
    for _ in range(3):                                                             # the later forwards that share the dict
        again = [kv_lookup(cache, b, c) for b in blocks]
        assert all(a is f for a, f in zip(again, first))
    assert [b[0].calls for b in blocks] == [1, 1]
    assert not torch.equal(first[0], first[1])                                     # one entry per block, not one for all


def test_stale_entries_are_refilled_in_place_by_the_next_lookup():
    from lib.model_zoo.vd import kv_lookup, kv_mark_stale
    blocks, c1, c2 = _blocks(), _ctx(1), _ctx(2)
    cache = {}
    kv_mark_stale(cache)                                # a sampler's first call marks before anything was projected
    first = [kv_lookup(cache, b, c1) for b in blocks]
    assert [b[0].calls for b in blocks] == [1, 1]
    ptrs, old = [kv.data_ptr() for kv in first], [kv.clone() for kv in first]
    kv_mark_stale(cache)
    assert kv_lookup(cache, blocks[0], c2) is first[0] and [b[0].calls for b in blocks] == [2, 1]
    assert torch.equal(first[1], old[1])                # the other entry waits for its own lookup
    assert kv_lookup(cache, blocks[1], c2) is first[1]
    for b, kv, p, o in zip(blocks, first, ptrs, old):
        assert kv.data_ptr() == p and not torch.equal(kv, o)
        assert torch.equal(kv, _Attn(b[0].gain).project_context(c2))
    for _ in range(2):
        assert [kv_lookup(cache, b, c2) for b in blocks][0] is first[0]
    assert [b[0].calls for b in blocks] == [2, 2]       # refreshed once each


def test_stale_entries_are_refilled_in_place_by_the_up_front_refresh():
    from lib.model_zoo.vd import kv_lookup, kv_mark_stale, kv_refresh, kv_refreshable
    blocks, c1, c2 = _blocks(), _ctx(1), _ctx(3)
    cache = {}
    first = [kv_lookup(cache, b, c1) for b in blocks]
    ptrs, old = [kv.data_ptr() for kv in first], [kv.clone() for kv in first]
    kv_mark_stale(cache)
    assert kv_refreshable(cache)
    kv_refresh(cache, c2)
    assert [b[0].calls for b in blocks] == [2, 2]
    for b, kv, p, o in zip(blocks, first, ptrs, old):
        assert kv.data_ptr() == p and not torch.equal(kv, o)
        assert torch.equal(kv, _Attn(b[0].gain).project_context(c2))
    # the forward that follows finds everything fresh, and a second refresh has nothing to do
    assert all(kv_lookup(cache, b, c2) is f for b, f in zip(blocks, first))
    kv_refresh(cache, c2)
    assert [b[0].calls for b in blocks] == [2, 2]
