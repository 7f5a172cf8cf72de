"""The sampler kernel (csrc/sample.hip) through rwkv_mi355x_selftest_sample against a float64
restatement of its definition (include/rwkv_mi355x.h).

Logits are round(N(0, 3) * 64) / 64 as float32: distinct logits differ by >= 1/64 (a 1.6 %
probability ratio, far above float32 error) and ties are exact.

Tolerance on the normalised CDF: EPS = 3e-5, derived as 2 * (d_w + d * 2^-24): d_w <= 4e-6 is the
relative error of one weight (the rounding of the argument (l - max) / T for |l - max| / T <= 64 plus
a few ulp of expf), d <= 128 the longest summation chain (the kernel's are 64 serial adds per
thread + 6 wave levels + 4 tree levels for the sums, and 6 + 6 + 15 + 6 for the prefix sums), which
gives 2 * (4e-6 + 7.6e-6) = 2.4e-5.  top_p values sit in the middle of a gap of >= 8 * EPS between
two achievable kept masses, so the kept count is exact."""
import functools

import numpy as np
import pytest

from rwkv_lib import library

pytestmark = pytest.mark.gpu

EPS = 3e-5
SIZES = [1, 63, 64, 65, 257, 50277, 65536, 70001]
U_LAST = float(np.float32(1 - 2.0 ** -24))


@functools.lru_cache(maxsize=None)
def logits_for(V):
    """[3][V]: seeds 1..3."""
    rows = [np.round(np.random.default_rng(seed).normal(0, 3, V) * 64) / 64 for seed in (1, 2, 3)]
    a = np.stack(rows).astype(np.float32)
    a.setflags(write=False)
    return a


def biased(row, bias):
    l = np.array(row, np.float32, copy=True)
    for i, b in (bias or {}).items():
        l[i] = np.float32(l[i] + np.float32(b))
    return l


class Ref:
    """float64 restatement for one row: tie groups by descending logit and their cumulative mass."""

    def __init__(self, row, bias=None):
        self.l = biased(row, bias).astype(np.float64)
        e = np.exp(self.l - self.l.max())
        self.p = e / e.sum()
        self.values, counts = np.unique(self.l, return_counts=True)
        self.values, counts = self.values[::-1], counts[::-1]
        pv = np.exp(self.values - self.l.max()) / e.sum()
        self.group_p = pv
        self.mass = np.cumsum(pv * counts)       # kept mass after each group
        self.count = np.cumsum(counts)           # kept tokens after each group

    def top_p_near(self, target):
        """(top_p as float32, kept count, cutoff probability) for the group boundary nearest target
        whose gap is >= 8 * EPS; top_p is the middle of that gap."""
        lo = np.concatenate([[0.0], self.mass[:-1]])
        ok = (self.mass - lo) >= 8 * EPS * 1.01
        assert ok.any(), 'no tie group with a gap of 8 * EPS'
        mid = 0.5 * (lo + self.mass)
        j = int(np.argmin(np.where(ok & (mid < 1.0), np.abs(mid - target), np.inf)))
        top_p = float(np.float32(mid[j]))
        assert 0.0 < top_p < 1.0
        assert self.mass[j] - top_p >= 4 * EPS and top_p - lo[j] >= 4 * EPS
        return top_p, int(self.count[j]), float(self.group_p[j])

    def kept(self, top_p):
        if top_p == 0.0 or top_p >= 1.0:
            return np.ones(len(self.l), bool)
        j = int(np.argmax(self.mass > top_p))
        return self.l >= self.values[j]

    def cdf(self, top_p, temperature):
        w = np.where(self.kept(top_p), self.p ** (1.0 / temperature), 0.0)
        c = np.cumsum(w)
        return w / c[-1], c / c[-1]


def run(logits, u, **kw):
    return library().rwkv_mi355x_selftest_sample(logits, u, **kw)


# ------------------------------------------------------------------------------------ greedy
@pytest.mark.parametrize('V', SIZES)
def test_greedy_is_argmax(V):
    lg = logits_for(V)
    tok, kept, _ = run(lg, 0.5, temperature=0.0)
    assert list(tok) == [int(np.argmax(r)) for r in lg]
    top = float(lg.max()) + 1.0
    plants = [[0], [V - 1], [0, V - 1]]
    if V >= 64:
        plants += [[3, 40]]                    # one wave, different threads
    if V > 3272:
        plants += [[70, 3272], [2948, 3272]]   # different waves; the lower index in the higher thread
    if V > 65536:
        plants += [[V - 1, 65536], [65535, 65536]]  # registers against the rows beyond them
    rows = []
    for idx in plants:
        r = lg[0].copy()
        r[idx] = top
        rows.append(r)
    tok, _, _ = run(np.stack(rows), 0.5, temperature=0.0)
    assert list(tok) == [min(idx) for idx in plants]
    # a bias that moves the winner
    j = (int(np.argmax(lg[1])) + V // 2) % V
    tok, _, _ = run(lg[1], 0.5, temperature=0.0, logit_bias={j: 100.0})
    assert tok[0] == (j if V > 1 else 0)


# ------------------------------------------------------------------------------------ kept set
@pytest.mark.parametrize('V', SIZES)
def test_kept_set(V):
    lg = logits_for(V)
    refs = [Ref(r) for r in lg]
    for target in (0.3, 0.5, 0.8, 0.95):
        # one call per row: top_p is a parameter of the call
        for r, ref in zip(lg, refs):
            top_p, count, cut = ref.top_p_near(target)
            _, kept, cutoff = run(r, 0.5, temperature=1.0, top_p=top_p)
            assert kept[0] == count, (V, target, top_p)
            assert abs(cutoff[0] - cut) <= 1e-5 * cut, (V, target, cutoff[0], cut)
    for top_p in (0.0, 1.0):
        _, kept, _ = run(lg, 0.5, temperature=1.0, top_p=top_p)
        assert list(kept) == [V] * 3


@pytest.mark.parametrize('V', [257, 65536, 70001])
def test_ties_at_the_cutoff_are_all_kept(V):
    r = np.full(V, -20.0, np.float32)
    ties = [2, V // 2, V - 1]  # different threads, waves and register rows
    r[7] = 5.0
    r[ties] = 3.0
    # p(7) = 0.71, the three tied tokens 0.096 each: the cutoff falls inside the tie at 0.8 and 0.9
    for top_p in (0.8, 0.9):
        us = np.linspace(0, U_LAST, 64).astype(np.float32)
        tok, kept, cutoff = run(np.broadcast_to(r, (64, V)), us, temperature=1.0, top_p=top_p)
        assert set(kept) == {4}
        assert set(tok) == set(ties) | {7}
        ref = Ref(r)
        assert abs(cutoff[0] - ref.p[2]) <= 1e-5 * ref.p[2]


# ------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize('temperature', [1.0, 0.8, 1.5])
@pytest.mark.parametrize('V', SIZES)
def test_draw(V, temperature):
    row = logits_for(V)[0]
    ref = Ref(row)
    top_p = ref.top_p_near(0.8)[0]
    w, C = ref.cdf(top_p, temperature)
    lo = np.concatenate([[0.0], C[:-1]])
    kept = ref.kept(top_p)
    # tokens heavy enough that the middle of their CDF interval is 2 * EPS from both ends
    heavy = np.flatnonzero(w >= 4 * EPS)
    if len(heavy) > 64:
        heavy = np.random.default_rng(V).choice(heavy, 64, replace=False)
    assert len(heavy) >= 1
    mids = (0.5 * (lo[heavy] + C[heavy])).astype(np.float32)
    rnd = np.random.default_rng(100 + V).random(256, dtype=np.float32)
    us = np.concatenate([mids, rnd, np.array([0.0, U_LAST], np.float32)])
    tok, _, _ = run(np.broadcast_to(row, (len(us), V)), us, temperature=temperature, top_p=top_p)
    tok = tok.astype(np.int64)
    assert (tok < V).all()
    assert list(tok[:len(heavy)]) == list(heavy)
    assert kept[tok].all() and (w[tok] > 0).all()
    u64 = us.astype(np.float64)
    assert (lo[tok] - EPS <= u64).all() and (u64 < C[tok] + EPS).all()
    assert tok[-2] == np.flatnonzero(kept)[0]  # u = 0: the first kept index


@pytest.mark.parametrize('V', [257, 65536])
def test_logit_bias(V):
    row = logits_for(V)[1]
    top = int(np.argmax(row))
    ref = Ref(row, {top: -1e9})
    top_p, count, cut = ref.top_p_near(0.8)
    us = np.linspace(0, U_LAST, 32).astype(np.float32)
    tok, kept, cutoff = run(np.broadcast_to(row, (32, V)), us, temperature=1.0, top_p=top_p, logit_bias={top: -1e9})
    assert top not in set(tok) and set(kept) == {count}
    assert ref.kept(top_p)[tok.astype(np.int64)].all()
    assert abs(cutoff[0] - cut) <= 1e-5 * cut
    j = (top + V // 3) % V
    tok, kept, _ = run(np.broadcast_to(row, (32, V)), us, temperature=0.8, top_p=0.5, logit_bias={j: 30.0, top: 0.25})
    assert set(tok) == {j} and set(kept) == {1}


def test_non_finite_logits_give_tokens_in_range():
    V = 65536
    base = logits_for(V)[2]
    rows = []
    for bad in (np.nan, np.inf, -np.inf):
        r = base.copy()
        r[[0, 77, 5000, V - 1]] = bad
        rows += [r, np.full(V, bad, np.float32)]
    us = np.linspace(0, U_LAST, len(rows)).astype(np.float32)
    for kw in ({'temperature': 0.0}, {'temperature': 0.8, 'top_p': 0.5}):
        tok, _, _ = run(np.stack(rows), us, **kw)
        assert (tok < V).all()


@pytest.mark.parametrize('V', [65, 65536, 70001])
def test_same_call_same_bits(V):
    lg = logits_for(V)
    us = np.array([0.1, 0.5, 0.9], np.float32)
    kw = dict(temperature=0.8, top_p=0.5, logit_bias={0: 1.5})
    a = run(lg, us, **kw)
    b = run(lg, us, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
