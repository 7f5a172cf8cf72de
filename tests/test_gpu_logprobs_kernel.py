"""k_logprobs and the sampler's LP form (csrc/logprobs.hip, sample.hip) through the two self-tests, on
host operands, against sampling.logprobs (float64 numpy).

Tolerance.  Ids are compared exactly.  Values: |gpu - ref| <= V * 2**-52 + 1e-12.  The first term is
twice the worst-case bound (V - 1) * 2**-53 on the relative error of a sum of V non-negative float64
terms in any association, which carries through log as an absolute error; the second leaves room for the
few-ulp errors of the device exp / log and of the final subtraction at |values| < 100.

Three rows per call, so that an odd V gives rows that start on every alignment."""
import numpy as np
import pytest

from rwkv_lib import library
from rwkv_cpp import sampling

pytestmark = pytest.mark.gpu

# the thread boundary (1024), the register boundary (65536) and the streamed tail beyond it
VOCABS = [5, 20, 1023, 1024, 1025, 65535, 65536, 65537, 131073]
TOP_KS = [0, 1, 5, 20]
FILL = 0xA5  # every byte of the caller's arrays before a call
FILL_U32, FILL_F64 = 0xA5A5A5A5, np.array([0xA5A5A5A5A5A5A5A5], np.uint64).view(np.float64)[0]


def tol(V):
    return V * 2.0 ** -52 + 1e-12


def close(got, want, t):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid='ignore'):
        return bool(np.all((got == want) | (np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= t)))


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def input_sets(V):
    """Named sets of three rows [3][V] float32."""
    rng = np.random.default_rng(4000 + V)
    gauss = (3.0 * rng.standard_normal((3, V))).astype(np.float32)
    ties = np.round(2.0 * rng.standard_normal((3, V))).astype(np.float32)
    ties[0, [0, V - 1, V // 2]] = 9.0  # the maximum three times, first and last element among them
    for edge, val in ((1024, 8.0), (65536, 7.0)):  # equal values on both sides of the two boundaries
        if V > edge:
            ties[1, [edge - 1, edge]] = val
            ties[2, [edge, edge - 1, 0]] = val
    odd = gauss.copy()
    odd[0, rng.permutation(V)[:max(1, V // 3)]] = -np.inf
    odd[1, [1, V - 2]] = np.nan
    return dict(gauss=gauss, ties=ties, odd=odd)


def biases(V, row):
    """A bias that lifts a low element of `row` to the top and pushes its maximum down; beyond the
    registers too where the row has a streamed tail."""
    order = np.argsort(np.nan_to_num(row, nan=0.0))
    b = {int(order[0]): 60.0, int(order[-1]): -30.0}
    if V > 65536:
        b[int(65536 + np.argmin(np.nan_to_num(row[65536:], nan=0.0)))] = 55.0
        b[7] = b.get(7, 0.0) + 0.25
    return b


def biased_rows(logits, bias):
    l = np.array(logits, np.float32, copy=True)
    for i, v in bias.items():  # the kernel adds the entries one after the other, in float32
        l[:, i] = l[:, i] + np.float32(v)
    return l


def check_rows(V, k, l, live, tokens, lp, name):
    """lp (Logprobs [rows] / [rows][k]) against sampling.logprobs of the rows l the sampler drew from."""
    t = tol(V)
    for r in range(l.shape[0]):
        tag = (name, V, k, r)
        if not live[r]:  # a finished row: the caller's values, untouched
            assert bits64(lp.token_logprob[r:r + 1])[0] == bits64([FILL_F64])[0], tag
            assert (lp.top_ids[r] == FILL_U32).all() and (bits64(lp.top_logprobs[r]) == bits64([FILL_F64])[0]).all(), tag
            continue
        logz, ids, vals = sampling.logprobs(l[r], k)
        n = len(ids)  # < k only where fewer than k elements are not NaN
        assert list(lp.top_ids[r][:n]) == list(ids), tag
        assert close(lp.top_logprobs[r][:n], vals, t), (tag, lp.top_logprobs[r][:n], vals)
        assert (lp.top_ids[r][n:] == FILL_U32).all() and (bits64(lp.top_logprobs[r][n:]) == bits64([FILL_F64])[0]).all(), tag
        tok = int(tokens[r])
        assert close(lp.token_logprob[r], np.float64(l[r][tok]) - logz, t), (tag, lp.token_logprob[r], l[r][tok], logz)
        for j in range(n):  # the same logZ word: bit-equal where the drawn token is listed
            if int(ids[j]) == tok:
                assert bits64(lp.token_logprob[r:r + 1])[0] == bits64(lp.top_logprobs[r][j:j + 1])[0], tag


def same_lp(a, b):
    return (np.array_equal(bits64(a.token_logprob), bits64(b.token_logprob)) and np.array_equal(a.top_ids, b.top_ids)
            and np.array_equal(bits64(a.top_logprobs), bits64(b.top_logprobs)))


@pytest.mark.parametrize('V', VOCABS)
def test_one_set_of_parameters(V):
    """k_logprobs + k_sample_lp (rwkv_mi355x_sample / _generate): bias only."""
    lib = library()
    u = np.array([0.1, 0.5, 0.9], np.float32)
    listed_token = False
    for name, logits in input_sets(V).items():
        bias = biases(V, logits[0]) if name != 'ties' else None
        l = biased_rows(logits, bias or {})
        for temperature, top_p in ((0.0, 0.5), (0.8, 0.5)):
            plain = lib.rwkv_mi355x_selftest_sample(logits, u, temperature, top_p, bias)
            for k in [k for k in TOP_KS if k <= V]:
                got = lib.rwkv_mi355x_selftest_sample(logits, u, temperature, top_p, bias, logprobs=k, fill=FILL)
                again = lib.rwkv_mi355x_selftest_sample(logits, u, temperature, top_p, bias, logprobs=k, fill=FILL)
                for a, b, c in zip(plain, got, again):  # tokens, kept, cutoff: the plain kernel's bits
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, V, k)
                    assert np.array_equal(b.view(np.uint32), c.view(np.uint32)), (name, V, k)
                assert same_lp(got[3], again[3]), (name, V, k)
                check_rows(V, k, l, [True] * 3, got[0], got[3], name)
                listed_token = listed_token or any(int(got[0][r]) in got[3].top_ids[r] for r in range(3))
    assert listed_token, 'no drawn token was among the listed ones: the bit-equality was never checked'


@pytest.mark.parametrize('V', VOCABS)
def test_rows_with_their_own_parameters(V):
    """k_logprobs + k_sample_rows_lp (rwkv_mi355x_generate_batch / _queue): penalties over counts,
    bias, stop tokens, a finished row."""
    lib = library()
    u = np.array([0.3, 0.7, 0.2], np.float32)
    sets = input_sets(V)
    for name, logits in sets.items():
        bias = biases(V, logits[1]) if name == 'gauss' else None
        counts0 = np.zeros((3, V), np.uint32)
        for r in range(3):  # the row's top element was drawn 40 times: 0.5 + 40 * 0.25 pushes it out
            counts0[r, int(np.argmax(np.nan_to_num(logits[r], nan=-1e30, neginf=-1e30)))] = 40
            counts0[r, V - 1] += 1
        done0 = np.array([0, 0, 1 if name == 'ties' else 0], np.uint32)
        l = biased_rows(np.stack([sampling.penalize(logits[r], counts0[r], 0.5, 0.25) for r in range(3)]), bias or {})
        if name == 'gauss' and V >= 1023:
            for r in range(3):
                assert int(np.argmax(logits[r])) not in sampling.logprobs(l[r], 20)[1], 'the penalty left the top element in'
        kw = dict(temperature=[0.0, 0.8, 1.0], top_p=[0.5, 0.5, 1.0], presence=0.5, frequency=0.25, logit_bias=bias,
                  stop_tokens=[int(np.argmax(l[0]))] if not np.isnan(l[0]).any() else (), step=3)

        def call(**more):
            counts, done = counts0.copy(), done0.copy()
            out = lib.rwkv_mi355x_selftest_sample_rows(logits, u, counts=counts, done=done, **kw, **more)
            out['counts'] = counts
            return out

        plain = call()
        for k in [k for k in TOP_KS if k <= V]:
            got, again = call(logprobs=k, lp_fill=FILL), call(logprobs=k, lp_fill=FILL)
            for key in ('tokens', 'decode_tokens', 'kept', 'cutoff', 'lengths', 'done', 'counts'):
                assert np.array_equal(plain[key].view(np.uint32), got[key].view(np.uint32)), (name, V, k, key)
                assert np.array_equal(got[key].view(np.uint32), again[key].view(np.uint32)), (name, V, k, key)
            assert plain['active'] == got['active'] == again['active']
            assert same_lp(got['logprobs'], again['logprobs']), (name, V, k)
            check_rows(V, k, l, done0 == 0, got['tokens'], got['logprobs'], name)
        if kw['stop_tokens']:  # the stop token is a drawn token: row 0 (greedy) stopped and still reports
            assert plain['done'][0] == 1 and plain['tokens'][0] == kw['stop_tokens'][0]
