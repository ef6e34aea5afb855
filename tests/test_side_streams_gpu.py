"""vd._side_streams: the streams the forked UNet branches run on are never the stream the fork starts from and never one another.

torch hands streams out round-robin from a pool of 32 per device, so the 33rd torch.cuda.Stream() of a process IS the first one
again.  Which streams meet therefore depends on how many the process has created: a branch forked onto the caller's own stream
(the capture stream of torch.cuda.graph, a sampler's capture stream) is ordered through events of that one stream, and ending
such a capture crashed the runtime once the suite's stream count moved.  No kernel runs here: the selection alone is checked,
with every stream of the pool in turn as the current one."""
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_side_streams_are_distinct_and_never_the_current_stream(dev):
    from lib.model_zoo import vd
    pool = {}
    for _ in range(64):   # two rounds of the pool
        s = torch.cuda.Stream(device=dev)
        pool.setdefault(s.cuda_stream, s)
    assert 2 <= len(pool) <= 32, len(pool)   # handles recur: the premise
    for kind, n in (("ctx", 2), ("batch", 1), ("ctx", 3)):
        for h, s in pool.items():
            with torch.cuda.stream(s):
                pick = [p.cuda_stream for p in vd._side_streams(dev, n, kind)]
            assert len(pick) == n and len(set(pick)) == n and h not in pick, (kind, n, hex(h), [hex(p) for p in pick])
    mine = [s.cuda_stream for k, l in vd._SIDE.items() if k[2] == threading.get_ident() and k[1] == dev.index for s in l]
    assert len(set(mine)) == len(mine)   # this thread's kinds share no stream either
    assert set(mine) <= vd.side_stream_handles(dev)
    # on the default stream the picks are stable from call to call (the eager warm-up step and later forwards meet the same streams)
    assert [p.cuda_stream for p in vd._side_streams(dev, 2)] == [p.cuda_stream for p in vd._side_streams(dev, 2)]


def test_sampler_capture_stream_is_no_side_stream(dev):
    """vd.capture_stream -- what DDIMSampler._capture_step captures on -- passes over pool streams that are kept as side streams, for
    more than a full round of the pool; and a step captured through the sampler runs on such a stream."""
    from lib.model_zoo import vd
    from lib.model_zoo.ddim import DDIMSampler
    vd._side_streams(dev, 2)
    busy = vd.side_stream_handles(dev)
    assert busy
    seen = {vd.capture_stream(dev).cuda_stream for _ in range(40)}
    assert len(seen) >= 2 and not (seen & vd.side_stream_handles(dev))
    used, buf = [], torch.zeros(4, device=dev)

    def body():
        used.append(torch.cuda.current_stream().cuda_stream)
        buf.add_(1.0)
    for _ in range(34):   # more captures than the pool has streams
        graph = DDIMSampler._capture_step(DDIMSampler.__new__(DDIMSampler), body)
        assert graph is not None
    assert len(used) == 34 and not (set(used) & vd.side_stream_handles(dev))
