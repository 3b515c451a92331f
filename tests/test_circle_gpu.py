"""GPU: the circle transform over Mersenne31 through the C ABI and sppark_amd.circle, bit for bit against the host
model (tests/circle_model.py).  Device tensors are torch.int32: canonical residues are below 2^31, the same 32 bits."""
import numpy as np
import pytest

import circle_model as M

pytestmark = pytest.mark.gpu

CACHE_CAP = (64 << 20) + (32 << 10)         # SPPARK_CIRCLE_CACHE_CAP_BYTES


@pytest.fixture(scope="module")
def C():
    import torch
    import sppark_amd
    from sppark_amd import circle
    assert torch.cuda.is_available() and sppark_amd.cuda_available("m31")
    return circle


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _inputs(k, seed):
    """random | all p-1 | all zero | a single one at the top index (every bit of j set), as four rows"""
    n = 1 << k
    x = np.zeros((4, n), dtype=np.uint32)
    x[0] = np.random.default_rng(seed).integers(0, M.P, n, dtype=np.uint32)
    x[1] = M.P - 1
    x[3, n - 1] = 1
    return x


# 2^21 is the first size with one more launch than 2^20 (circle_route.hpp: 1 + ceil((k - 12) / 8) above 2^12); the next
# change, 2^28 -> 2^29, lies beyond the sizes a host model checks in seconds
@pytest.mark.parametrize("k", list(range(1, 22)))
def test_bit_exact_every_size(C, k):
    x = _inputs(k, 1000 + k)
    # the model runs once per direction: NATURAL is BITREV with position q moved to bitrev(q), on the output of a
    # forward transform and on the input of an inverse one
    want_f, want_i, perm = M.forward(x, k, M.BITREV), M.inverse(x, k, M.BITREV), M.bitrev_perm(k)
    d = _dev(x)
    C.ntt(0, d, C.FORWARD, M.BITREV)
    assert (_host(d) == want_f).all(), (k, "forward, BITREV")
    d = _dev(x)
    C.ntt(0, d, C.FORWARD, M.NATURAL)
    assert (_host(d)[:, perm] == want_f).all(), (k, "forward, NATURAL")
    d = _dev(x)
    C.ntt(0, d, C.INVERSE, M.BITREV)
    assert (_host(d) == want_i).all(), (k, "inverse, BITREV")
    nat = np.empty_like(x)
    nat[:, perm] = x
    d = _dev(nat)
    C.ntt(0, d, C.INVERSE, M.NATURAL)
    assert (_host(d) == want_i).all(), (k, "inverse, NATURAL")


def test_round_trip_2_24(C):
    import torch
    k = 24
    x = np.random.default_rng(24).integers(0, M.P, 1 << k, dtype=np.uint32)
    d = _dev(x)
    ref = d.clone()
    for order in (M.BITREV, M.NATURAL):
        C.evaluate(0, d, order)
        assert not torch.equal(d, ref)
        C.interpolate(0, d, order)
        assert torch.equal(d, ref), order


@pytest.mark.parametrize("k", [24, 26])
def test_sparse_samples_large(C, k):
    import torch
    n = 1 << k
    idx = [0, 1, 5, n // 2 + 3, n - 2, n - 1]
    val = [3, M.P - 1, 123456789, 7, 2, 1]
    pos = np.random.default_rng(k).integers(0, n, 4096)
    for order in (M.BITREV, M.NATURAL):
        d = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        d[torch.tensor(idx, device="cuda:0")] = torch.tensor(val, dtype=torch.int32, device="cuda:0")
        C.evaluate(0, d, order)
        got = _host(d[torch.from_numpy(pos).to("cuda:0")])
        assert (got == M.sparse_evaluate(idx, val, k, pos, order)).all(), (k, order)


def test_2_30_offsets_past_4_gib(C):
    """The first size whose byte offsets pass 2^32: six non-zero coefficients, 4096 sampled outputs, and the way back."""
    import torch
    k = 30
    n = 1 << k
    idx = [0, 3, (1 << 29) + 17, (1 << 30) - (1 << 12) - 1, n - 2, n - 1]
    val = [5, M.P - 1, 99, 1 << 30, 12345, 1]
    pos = np.concatenate([np.random.default_rng(30).integers(0, n, 4090), [0, 1, n // 2, n // 2 + 1, n - 2, n - 1]])
    dpos, didx = torch.from_numpy(pos).to("cuda:0"), torch.tensor(idx, device="cuda:0")
    d = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d[didx] = torch.tensor(val, dtype=torch.int32, device="cuda:0")
    for order in (M.BITREV, M.NATURAL):
        C.evaluate(0, d, order)
        assert (_host(d[dpos]) == M.sparse_evaluate(idx, val, k, pos, order)).all(), order
        C.interpolate(0, d, order)
        assert int(torch.count_nonzero(d)) == len(idx), order
        assert _host(d[didx]).tolist() == val, order
    del d
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [2, 6, 7, 11, 12, 13])
def test_batches_strided_with_sentinels(C, k):
    n = 1 << k
    rng = np.random.default_rng(50 + k)
    for batch in (1, 3, 65):
        stride = n + 5
        for off in (0, 1):                              # off = 1: an unaligned first column
            buf = rng.integers(0, M.P, batch * stride + off + 3, dtype=np.uint32)
            cols = buf[off:off + batch * stride].reshape(batch, stride)[:, :n]
            for order in (M.BITREV, M.NATURAL):
                for direction, model in ((C.FORWARD, M.forward), (C.INVERSE, M.inverse)):
                    single = np.stack([np.ascontiguousarray(c).copy() for c in cols])
                    for row in single:
                        C.ntt(0, row, direction, order)  # the single call, host buffer
                    assert (single == model(cols, k, order)).all()
                    d = _dev(buf)
                    view = d[off:off + batch * stride].view(batch, stride)[:, :n]
                    C.ntt(0, view, direction, order)
                    got = _host(d)
                    g = got[off:off + batch * stride].reshape(batch, stride)
                    assert (g[:, :n] == single).all(), (k, batch, off, order, int(direction))
                    want = buf.copy()
                    want[off:off + batch * stride].reshape(batch, stride)[:, :n] = single
                    assert (got == want).all(), "sentinels between the columns were touched"
                    h = buf.copy()                       # the same strided batch from a host buffer
                    hv = h[off:off + batch * stride].reshape(batch, stride)[:, :n]
                    C.ntt(0, hv, direction, order)
                    assert (h == want).all()


def test_batch_beyond_one_launch(C):
    k, batch = 2, 70000
    x = np.random.default_rng(70).integers(0, M.P, (batch, 1 << k), dtype=np.uint32)
    for order in (M.BITREV, M.NATURAL):
        d = _dev(x)
        C.evaluate(0, d, order)
        assert (_host(d) == M.forward(x, k, order)).all(), order
        C.interpolate(0, d, order)
        assert (_host(d) == x).all(), order


def test_host_device_and_stream_agree(C):
    import torch
    k = 14
    x = np.random.default_rng(14).integers(0, M.P, (3, 1 << k), dtype=np.uint32)
    want = M.forward(x, k)
    h = x.copy()
    C.evaluate(0, h)
    assert (h == want).all()
    d = _dev(x)
    C.evaluate(0, d)
    assert (_host(d) == want).all()
    s = torch.cuda.Stream()
    d2 = _dev(x)
    torch.cuda.synchronize()
    C.evaluate(0, d2, stream=s.cuda_stream)
    C.interpolate(0, d2, stream=s.cuda_stream)
    C.evaluate(0, d2, M.NATURAL, stream=s.cuda_stream)
    s.synchronize()
    assert (_host(d2) == M.forward(x, k, M.NATURAL)).all()


def test_cache_cap_and_release(C):
    rng = np.random.default_rng(3)
    assert C.cached_bytes(0) <= CACHE_CAP               # whatever ran before, the 2^30 inverse included
    C.release_cached(0)
    assert C.cached_bytes(0) == 0
    for k in range(1, 19):
        d = _dev(rng.integers(0, M.P, 1 << k, dtype=np.uint32))
        C.interpolate(0, d)
    used = C.cached_bytes(0)
    assert 0 < used <= CACHE_CAP, used
    # the tables of sizes 2 .. 18: two families of 2^(m-2) four-byte entries, and 4096 points of eight bytes
    assert used == 2 * 4 * sum(1 << (m - 2) for m in range(2, 19)) + 4096 * 8, used
    C.release_cached(0)
    assert C.cached_bytes(0) == 0
    x = rng.integers(0, M.P, 1 << 10, dtype=np.uint32)
    d = _dev(x)
    C.interpolate(0, d)
    assert (_host(d) == M.inverse(x, 10)).all()
    C.evaluate(0, d)
    assert (_host(d) == x).all()


def test_two_threads_build_the_same_tables(C):
    """Two threads, each on its own stream, run the first inverse of a size at once: whichever finds the other's table in
    the cache must find it complete (the driver synchronises before a table enters the cache)."""
    import threading
    import torch
    torch.cuda.synchronize()
    C.release_cached(0)
    k = 20
    xs = [np.random.default_rng(900 + i).integers(0, M.P, 1 << k, dtype=np.uint32) for i in range(2)]
    ds = [_dev(x) for x in xs]
    streams = [torch.cuda.Stream() for _ in xs]
    torch.cuda.synchronize()
    errors = []

    def work(i):
        try:
            C.interpolate(0, ds[i], stream=streams[i].cuda_stream)
            streams[i].synchronize()
        except Exception as e:                          # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for x, d in zip(xs, ds):
        assert (_host(d) == M.inverse(x, k)).all()


@pytest.mark.parametrize("k", list(range(1, 13)))
def test_lde(C, k):
    rng = np.random.default_rng(400 + k)
    for b in (1, 2, 3):
        for order in (M.BITREV, M.NATURAL):
            for batch in (1, 5):
                e = rng.integers(0, M.P, (batch, 1 << k), dtype=np.uint32)
                coeffs, want = M.lde(e, k, b, order)
                for with_aux in (False, True):
                    buf = rng.integers(0, M.P, (batch, 1 << (k + b)), dtype=np.uint32)
                    buf[:, :1 << k] = e
                    d = _dev(buf)
                    aux = _dev(np.zeros((batch, 1 << k), dtype=np.uint32)) if with_aux else None
                    C.lde(0, d, k, b, order, aux_out=aux)
                    assert (_host(d) == want).all(), (k, b, order, batch)
                    if with_aux:
                        assert (_host(aux) == coeffs).all()
                        # the output restricted to the coefficients: aux_out re-evaluated (zero-padded) is the output
                        pad = np.zeros_like(buf)
                        pad[:, :1 << k] = _host(aux)
                        dp = _dev(pad)
                        C.evaluate(0, dp, order)
                        assert (_host(dp) == _host(d)).all()
    hb = np.zeros((2, 1 << (k + 1)), dtype=np.uint32)      # host buffers, host aux_out
    e = rng.integers(0, M.P, (2, 1 << k), dtype=np.uint32)
    hb[:, :1 << k] = e
    ha = np.zeros((2, 1 << k), dtype=np.uint32)
    C.lde(0, hb, k, 1, M.BITREV, aux_out=ha)
    coeffs, want = M.lde(e, k, 1, M.BITREV)
    assert (hb == want).all() and (ha == coeffs).all()


def test_lde_2_20_to_2_22(C):
    k, b = 20, 2
    e = np.random.default_rng(2022).integers(0, M.P, 1 << k, dtype=np.uint32)
    coeffs, want = M.lde(e, k, b, M.BITREV)
    buf = np.zeros(1 << (k + b), dtype=np.uint32)
    buf[:1 << k] = e
    d, aux = _dev(buf), _dev(np.zeros(1 << k, dtype=np.uint32))
    C.lde(0, d, k, b, M.BITREV, aux_out=aux)
    assert (_host(aux) == coeffs).all()
    assert (_host(d) == want).all()
