"""The checks of tests/_poison.py themselves, on numpy arrays: an untouched record is found wherever it lies, a real miss is not mistaken for one,
and a touched guard word is reported."""
import numpy as np
import pytest

import _poison as P

HIT = np.dtype([("id", "<i4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4")])


def _written(n):
    h = np.zeros(n, dtype=HIT)
    h["id"] = np.arange(n); h["t"] = np.float32(0.5)
    return h


def _untouch(a, i):
    a.view(np.uint8).reshape(a.shape[0], -1)[i] = 0xFF


@pytest.mark.parametrize("n", [1, 2, 1000])
def test_an_untouched_record_is_found_at_every_position(n):
    P.assert_all_written(_written(n))
    for i in sorted({0, n // 2, n - 1}):
        for a in (_written(n), np.arange(n, dtype=np.int32), np.arange(3 * n, dtype=np.uint32).reshape(n, 3), _written(n)["id"]):
            a = np.ascontiguousarray(a)
            _untouch(a, i)
            with pytest.raises(AssertionError, match="never written"):
                P.assert_all_written(a)


def test_an_untouched_hit_fails_the_comparisons_the_parity_tests_make():
    h = np.zeros(1, dtype=HIT); _untouch(h, 0)
    assert h["id"][0] == -1 and h["t"].view(np.uint32)[0] == 0xFFFFFFFF and not (h["u"] == 0).any() and not (h["v"] == 0).any()
    miss = np.zeros(1, dtype=HIT); miss["id"] = -1; miss["t"] = np.float32(3.4e38)
    assert (h["id"] == miss["id"]).all() and not (h["t"].view(np.uint32) == miss["t"].view(np.uint32)).any()


def test_a_miss_is_a_written_record():
    h = _written(10)
    h["id"][[0, 5, 9]] = -1; h["t"][[0, 5, 9]] = np.float32(3.4028235e38)
    P.assert_all_written(h)
    h["t"][5] = np.float32(100.0)
    P.assert_all_written(h)
    # a partly written record counts as written (the field comparisons catch it), an empty array has nothing to miss
    h.view(np.uint32).reshape(10, 4)[3, 1:] = 0xFFFFFFFF
    P.assert_all_written(h)
    P.assert_all_written(np.zeros(0, dtype=HIT))
    # a 2-D word array: one untouched word in a row is no untouched record
    w = np.zeros((4, 3), np.int32); w[2, 1] = -1
    P.assert_all_written(w)


def test_a_touched_guard_word_is_reported():
    g = np.full(P.GUARD, 0xFF, np.uint8)
    P.check_guard(g)
    P.check_guard(g[:0])
    for at in (0, 100, P.GUARD - 4):
        bad = g.copy(); bad.view(np.uint32)[at // 4] = 7
        with pytest.raises(AssertionError, match="written beyond the buffer"):
            P.check_guard(bad)
    bad = g.copy(); bad[-1] = 0xFE
    with pytest.raises(AssertionError, match="written beyond the buffer"):
        P.check_guard(bad)


class _FakeMem:
    """host memory behind the three calls of a MemManager the helper uses"""
    def __init__(self): self.bufs = {}
    def alloc(self, n): p = 4096 * (len(self.bufs) + 1); self.bufs[p] = np.zeros(n, np.uint8); return p
    def one(self, p, n): self.bufs[p][:n] = 0xFF
    def download(self, p, dtype, count): return self.bufs[p][: np.dtype(dtype).itemsize * count].copy().view(dtype)


def test_fetch_returns_the_payload_and_checks_the_guard():
    mem = _FakeMem()
    n = 37
    d = P.alloc_out(mem, 16 * n)
    assert mem.bufs[d].size == 16 * n + P.GUARD and (mem.bufs[d] == 0xFF).all()
    got = P.fetch(mem, d, HIT, n)
    assert got.shape == (n,) and (got["id"] == -1).all()
    with pytest.raises(AssertionError, match="never written"):
        P.assert_all_written(got)
    mem.bufs[d][:16 * n] = _written(n).view(np.uint8)
    got = P.fetch(mem, d, HIT, n)
    assert (got == _written(n)).all()
    P.assert_all_written(got)
    mem.bufs[d][16 * n + 8] = 0                              # one byte behind the payload
    with pytest.raises(AssertionError, match="written beyond the buffer"):
        P.fetch(mem, d, HIT, n)
    P.poison(mem, d, 16 * n)
    assert (mem.bufs[d] == 0xFF).all()
    # a shorter batch in the same buffer: the guard lies right behind ITS payload
    P.poison(mem, d, 16 * 10)
    mem.bufs[d][:16 * 10] = _written(10).view(np.uint8)
    assert (P.fetch(mem, d, HIT, 10) == _written(10)).all()
    mem.bufs[d][16 * 10] = 1
    with pytest.raises(AssertionError, match="written beyond the buffer"):
        P.fetch(mem, d, HIT, 10)
