"""The seeded noise generator on the host: a numpy restatement of Philox4x32-10 and of the normal map of include/vd_hip.h
(fp64 transcendentals) against the published known answers, and the first two moments of its normals.  The GPU tests
import the restatement from here.  No GPU, no library needed."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11): ctr = four uint64 arrays (or ints) holding 32-bit words, key = two ints.
    Returns four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in np.broadcast_arrays(*ctr))
    k0, k1 = int(key[0]), int(key[1])
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def normals_ref(seed, per_sample, draw=0, stream=0):
    """float64 [per_sample]: the normals of one sample, by the contract of include/vd_hip.h -- key = (low, high word of
    the seed), counter = (j, 0, draw, stream) for elements 4j .. 4j+3, words (r0, r1) -> elements 4j, 4j+1 and
    (r2, r3) -> 4j+2, 4j+3 through Box-Muller on u = ((r >> 9) + 0.5) 2^-23."""
    seed = int(seed)
    assert 0 <= seed < 2 ** 63
    nblk = (per_sample + 3) // 4
    j = np.arange(nblk, dtype=np.uint64)
    r = philox4x32_10((j, 0, int(draw), int(stream)), (seed & MASK, seed >> 32))
    u = [((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23 for w in r]
    z = np.empty((nblk, 4), dtype=np.float64)
    for a in (0, 2):
        rad = np.sqrt(-2.0 * np.log(u[a]))
        z[:, a] = rad * np.cos(2.0 * np.pi * u[a + 1])
        z[:, a + 1] = rad * np.sin(2.0 * np.pi * u[a + 1])
    return z.reshape(-1)[:per_sample]


def normals_ref_batch(seeds, per_sample, draw=0, stream=0):
    return np.stack([normals_ref(s, per_sample, draw, stream) for s in seeds])


def _words(ctr, key):
    return ["%08x" % int(w) for w in philox4x32_10(ctr, key)]


def test_known_answers():
    """Random123's published vectors for philox4x32 with 10 rounds."""
    assert _words((0, 0, 0, 0), (0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert _words((f, f, f, f), (f, f)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert _words((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_vectorised_counter_equals_one_at_a_time():
    j = np.arange(5, dtype=np.uint64)
    many = philox4x32_10((j, 0, 3, 2), (17, 99))
    for k in range(5):
        one = philox4x32_10((k, 0, 3, 2), (17, 99))
        assert [int(w[k]) for w in many] == [int(w) for w in one]


def test_uniforms_are_exact_in_fp32_and_inside_the_unit_interval():
    for r in (0, 1 << 9, 0xFFFFFFFF, 0x12345678):
        u = ((r >> 9) + 0.5) * 2.0 ** -23
        assert 0.0 < u < 1.0 and float(np.float32(u)) == u


def test_moments_of_the_normals():
    """2^20 normals of one seed: |mean| < 5 / sqrt(n) and |var - 1| < 5 sqrt(2 / n) (5 sigma bounds)."""
    n = 1 << 20
    z = normals_ref(20221101, n, draw=0, stream=2)
    assert z.shape == (n,) and np.isfinite(z).all()
    assert abs(z.mean()) < 5.0 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / n), z.var()
    assert np.abs(z).max() <= np.sqrt(48.0 * np.log(2.0))       # u1 >= 2^-24


def test_partial_block_and_streams():
    a = normals_ref(5, 105)
    assert a.shape == (105,) and np.array_equal(a, normals_ref(5, 108)[:105])
    for other in (normals_ref(5, 105, draw=1), normals_ref(5, 105, stream=1), normals_ref(6, 105)):
        assert not np.any(other == a)
