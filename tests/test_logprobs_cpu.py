"""Log-probabilities of device generation without a GPU: sampling.logprobs (the specification the
kernels are measured against) checked against a math.fsum log-sum-exp and on hand-made orders, the new
entry points of the built library, and the Python layer against a fake library object."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'rwkv.cppy_amd', 'python'))

from rwkv_cpp import sampling  # noqa: E402
from rwkv_cpp import rwkv_cpp_shared_library as shared  # noqa: E402
from rwkv_cpp.rwkv_cpp_model import RWKVModel  # noqa: E402
from rwkv_lib import library  # noqa: E402


def fsum_logz(l):
    """log sum exp l with the sum exactly rounded (math.fsum)."""
    ld = [float(x) for x in np.asarray(l, np.float32)]
    m = max(ld)
    return m + math.log(math.fsum(math.exp(x - m) for x in ld))


def order_by_hand(l):
    """Larger l first, lower index first among equal l; NaNs dropped.  Plain Python."""
    return [i for i in sorted(range(len(l)), key=lambda i: (-float(l[i]), i)) if not math.isnan(float(l[i]))]


# ------------------------------------------------------------------------------------ sampling.logprobs
@pytest.mark.parametrize('V', [5, 1025, 65537])
def test_logz_is_the_fsum_log_sum_exp(V):
    rng = np.random.default_rng(V)
    l = (4.0 * rng.standard_normal(V)).astype(np.float32)
    logz, ids, lps = sampling.logprobs(l, min(V, 20))
    # a sum of V non-negative float64 terms, any association: relative error <= (V - 1) 2^-53
    assert abs(logz - fsum_logz(l)) <= V * 2.0 ** -52 + 1e-12
    assert ids.dtype == np.uint32 and lps.dtype == np.float64
    assert list(ids) == order_by_hand(l)[:min(V, 20)]
    assert np.array_equal(lps, l[ids].astype(np.float64) - logz)
    # the probabilities of all the tokens sum to one
    _, _, every = sampling.logprobs(l, V)
    assert abs(math.fsum(np.exp(every)) - 1.0) < 1e-9


def test_ties_are_listed_by_index():
    rng = np.random.default_rng(7)
    l = np.round(2.0 * rng.standard_normal(1025)).astype(np.float32)
    _, ids, lps = sampling.logprobs(l, 20)
    ids = [int(i) for i in ids]
    assert ids == order_by_hand(l)[:20]
    # runs of equal values among the 20: their indices ascend
    runs = [sum(1 for i in ids if l[i] == v) for v in sorted({float(l[i]) for i in ids}, reverse=True)]
    assert max(runs) >= 3 and sum(runs) == 20 and len(runs) >= 2, runs
    for a, b in zip(ids, ids[1:]):
        assert l[a] > l[b] or (l[a] == l[b] and a < b)
    assert all(x >= y for x, y in zip(lps, lps[1:]))


def test_nan_entries_are_never_listed():
    l = np.array([0.5, np.nan, 2.0, -np.inf, np.nan, 2.0, 1.0], np.float32)
    logz, ids, lps = sampling.logprobs(l, 7)
    assert list(ids) == [2, 5, 6, 0, 3]  # five elements are not NaN: five entries, however many are asked for
    assert math.isnan(logz) and np.isnan(lps).all()  # exp(NaN) is in the sum
    logz, ids, lps = sampling.logprobs(np.array([0.5, -np.inf, 2.0], np.float32), 3)
    assert list(ids) == [2, 0, 1] and lps[2] == -np.inf and math.isfinite(logz)


def test_top_k_zero_and_top_k_v():
    l = np.array([0.25, -1.0, 3.0, 3.0, 0.0], np.float32)
    logz, ids, lps = sampling.logprobs(l, 0)
    assert ids.shape == (0,) and lps.shape == (0,) and abs(logz - fsum_logz(l)) < 1e-14
    _, ids, lps = sampling.logprobs(l, 5)
    assert list(ids) == [2, 3, 0, 4, 1] and lps[0] == lps[1]
    with pytest.raises(ValueError):
        sampling.logprobs(l, 6)
    with pytest.raises(ValueError):
        sampling.logprobs(l, -1)


def test_penalised_row_is_what_is_scored():
    """The row the log-probabilities are taken of: penalize, then the bias."""
    l = np.array([1.0, 4.0, 3.5, 0.0], np.float32)
    row = sampling.penalize(l, np.array([0, 2, 0, 0]), 0.5, 0.25)  # token 1 was drawn twice: 4 - (0.5 + 2 * 0.25) = 3
    row[3] += np.float32(3.25)
    _, ids, _ = sampling.logprobs(row, 2)
    assert list(ids) == [2, 3]  # the penalty pushed token 1 out, the bias lifted token 3 in


# ------------------------------------------------------------------------------------ the built library
NEW = ['rwkv_mi355x_sample_logprobs', 'rwkv_mi355x_generate_logprobs', 'rwkv_mi355x_generate_batch_logprobs',
       'rwkv_mi355x_generate_queue_logprobs', 'rwkv_mi355x_selftest_sample_logprobs',
       'rwkv_mi355x_selftest_sample_rows_logprobs']


def test_the_library_exports_the_entry_points():
    L = library().library
    for name in NEW:
        assert hasattr(L, name), name
    assert shared.MAX_TOP_LOGPROBS == 20


def test_null_context_is_refused_as_by_the_sibling_calls():
    """Without a device there is no context: the four calls return false for NULL, as their siblings do."""
    L = library().library
    lp, _ = shared.make_logprobs(1, 4, 5)
    p = shared.make_sampling(0.0, 0.5)
    bp = shared.make_batch_sampling(1, 0.0, 0.5)
    tok = (ctypes.c_uint32 * 4)()
    one = (ctypes.c_uint32 * 1)(4)
    assert not L.rwkv_mi355x_sample(None, ctypes.byref(p), tok)
    assert not L.rwkv_mi355x_sample_logprobs(None, ctypes.byref(p), tok, ctypes.byref(lp))
    assert not L.rwkv_mi355x_generate_logprobs(None, ctypes.byref(p), 4, tok, None, ctypes.byref(lp))
    assert not L.rwkv_mi355x_generate_batch_logprobs(None, 1, ctypes.byref(bp), 4, tok, one, None, ctypes.byref(lp))
    assert not L.rwkv_mi355x_generate_queue_logprobs(None, 1, 1, ctypes.byref(bp), one, 4, tok, one, None, None, None,
                                                     ctypes.byref(lp))


def test_selftests_refuse_bad_arguments_before_any_device_call():
    lib = library()
    l = np.zeros((1, 8), np.float32)
    for k in (21, 9):  # above 20, above V
        with pytest.raises(ValueError):
            lib.rwkv_mi355x_selftest_sample(l, 0.5, logprobs=k)
        with pytest.raises(ValueError):
            lib.rwkv_mi355x_selftest_sample_rows(l, 0.5, 1.0, 0.5, logprobs=k)
    P_D, P_U, P_F = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)
    p = shared.make_sampling(0.0, 0.5)
    u, tok = np.zeros(1, np.float32), np.zeros(1, np.uint32)
    ids, d = np.zeros(2, np.uint32), np.zeros(2, np.float64)
    args = (l.ctypes.data_as(P_F), 1, 8, ctypes.byref(p), u.ctypes.data_as(P_F), tok.ctypes.data_as(P_U), None, None, 2)
    assert not lib.library.rwkv_mi355x_selftest_sample_logprobs(*args, None, ids.ctypes.data_as(P_U), d.ctypes.data_as(P_D))
    assert not lib.library.rwkv_mi355x_selftest_sample_logprobs(*args, d.ctypes.data_as(P_D), None, d.ctypes.data_as(P_D))
    assert not lib.library.rwkv_mi355x_selftest_sample_logprobs(*args, d.ctypes.data_as(P_D), ids.ctypes.data_as(P_U), None)


def test_make_logprobs_poisons_the_host_arrays():
    lp, out = shared.make_logprobs(2, 3, 4)
    assert lp.top_k == 4 and out.token_logprob.shape == (2, 3) and out.top_ids.shape == (2, 3, 4)
    assert (out.top_ids == 0xA5A5A5A5).all() and (out.token_logprob.view(np.uint64) == 0xA5A5A5A5A5A5A5A5).all()
    with pytest.raises(ValueError):
        shared.make_logprobs(1, 1, 21)


# ------------------------------------------------------------------------------------ the Python layer
class FakeLibrary:
    """Records the calls of RWKVModel and answers with fixed tokens and log-probabilities."""

    def __init__(self):
        self.calls = []

    def rwkv_mi355x_batch_slots(self, ctx):
        return 256

    def rwkv_mi355x_prefill_batch(self, ctx, prompts, slots, cont):
        pass

    def rwkv_mi355x_generate_batch(self, ctx, rows, n, params, logprobs=None):
        self.calls.append(('generate_batch', logprobs))
        tokens = np.arange(rows * n, dtype=np.uint32).reshape(rows, n)
        lengths = np.array([n - r for r in range(rows)], np.uint32)
        if logprobs is None:
            return tokens, lengths, n
        lp = shared.Logprobs(-np.arange(rows * n, dtype=np.float64).reshape(rows, n),
                             np.zeros((rows, n, logprobs), np.uint32), np.zeros((rows, n, logprobs), np.float64))
        return tokens, lengths, n, lp

    def rwkv_mi355x_generate(self, ctx, n, temperature, top_p, logit_bias, seed, offset, logits_out_address=None,
                             logprobs=None):
        self.calls.append(('generate', n, offset, logprobs))
        tokens = list(range(offset, offset + n))
        if logprobs is None:
            return tokens
        return tokens, shared.Logprobs(-np.array(tokens, np.float64), np.zeros((n, logprobs), np.uint32),
                                       np.zeros((n, logprobs), np.float64))


def fake_model():
    m = RWKVModel.__new__(RWKVModel)
    m._library, m._ctx, m._valid = FakeLibrary(), object(), True
    return m


def test_generate_batch_trims_the_logprobs_to_the_token_lists():
    m = fake_model()
    lists, lps = m.generate_batch([[1], [2], [3]], 4, batched_prefill=True, logprobs=3)
    assert [len(x) for x in lists] == [4, 3, 2]
    for toks, lp in zip(lists, lps):
        assert lp.token_logprob.shape == (len(toks),) and lp.top_ids.shape == (len(toks), 3)
        assert list(lp.token_logprob) == [-float(t) for t in toks]
    # without the keyword: exactly what it returned before
    assert m.generate_batch([[1], [2], [3]], 4, batched_prefill=True) == lists
    assert m._library.calls == [('generate_batch', 3), ('generate_batch', None)]
    m._valid = False


def test_generate_cuts_the_logprobs_where_it_cuts_the_tokens():
    m = fake_model()
    tokens, lp = m.generate(10, stop_tokens=[6], block=4, logprobs=2)
    assert tokens == [0, 1, 2, 3, 4, 5, 6]
    assert list(lp.token_logprob) == [-float(t) for t in tokens] and lp.top_ids.shape == (7, 2)
    assert m.generate(10, stop_tokens=[6], block=4) == tokens
    tokens, lp = m.generate(5, block=4, logprobs=0)
    assert tokens == [0, 1, 2, 3, 4] and lp.token_logprob.shape == (5,) and lp.top_logprobs.shape == (5, 0)
    m._valid = False
