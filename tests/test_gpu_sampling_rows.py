"""The batched sampler kernel (csrc/sample.hip, k_sample_rows) through rwkv_mi355x_selftest_sample_rows:
rows with their own temperature, top_p and draw in one launch, presence / frequency penalties over a
count table, stop tokens and finished rows.

Everything is exact equality with the one-row kernel (rwkv_mi355x_selftest_sample) run on each row
alone, which tests/test_gpu_sampling.py checks against float64 -- except test_penalty_against_float64,
which repeats that file's float64 comparison (its EPS and its rule for the kept count) on penalised
rows: the penalty is pinned to float32 (sampling.penalize), the float64 formula can differ from it by
one rounding of the logit, 2^-24 * |l| <= 1e-6 for these logits, inside the d_w term of EPS."""
import numpy as np
import pytest

from rwkv_lib import library
from rwkv_cpp import sampling
from test_gpu_sampling import EPS, Ref, logits_for

pytestmark = pytest.mark.gpu

SIZES = [63, 65, 50277, 65536, 70001]  # the register / tail boundary and the odd vocabulary
TEMPERATURE = [0.0, 1.0, 0.7]
TOP_P = [0.5, 0.8, 0.3]
U = [0.1, 0.5, 0.9]
FILL = 0xFFFFFFFF


def bits(a):
    return np.asarray(a).view(np.uint32)


def one_row(row, r, **kw):
    tok, kept, cutoff = library().rwkv_mi355x_selftest_sample(row, U[r], temperature=TEMPERATURE[r], top_p=TOP_P[r], **kw)
    return int(tok[0]), int(kept[0]), cutoff[0]


def counts_for(V, lg):
    """[3][V] uint32: about 1 % of the tokens drawn 1 to 4 times, each row's 8 largest logits among them."""
    rng = np.random.default_rng(1000 + V)
    c = np.zeros((3, V), np.uint32)
    for r in range(3):
        idx = rng.choice(V, max(4, V // 100), replace=False)
        c[r, idx] = rng.integers(1, 5, len(idx))
        top = np.argsort(lg[r])[-8:]
        c[r, top] = rng.integers(1, 5, len(top))
    return c


@pytest.mark.parametrize('V', SIZES)
def test_rows_equal_the_one_row_kernel(V):
    lg = logits_for(V)
    for bias in (None, {0: 1.5, V - 1: -2.0, V // 2: 0.75}):
        out = library().rwkv_mi355x_selftest_sample_rows(lg, U, TEMPERATURE, TOP_P, logit_bias=bias)
        for r in range(3):
            tok, kept, cutoff = one_row(lg[r], r, logit_bias=bias)
            assert out['tokens'][r] == tok and out['decode_tokens'][r] == tok, (V, r)
            assert out['kept'][r] == kept, (V, r)
            assert bits(out['cutoff'])[r] == bits(cutoff), (V, r)
        assert list(out['lengths']) == [1, 1, 1] and list(out['done']) == [0, 0, 0] and out['active'] == 3


@pytest.mark.parametrize('V', SIZES)
def test_penalised_rows_equal_the_one_row_kernel_on_penalize(V):
    lg = logits_for(V)
    counts = counts_for(V, lg)
    presence, frequency = [2.0, 0.2, 0.0], [1.0, 0.2, 0.3]
    bias = {1: 0.5, V - 2: 1.25}
    before = counts.copy()
    out = library().rwkv_mi355x_selftest_sample_rows(lg, U, TEMPERATURE, TOP_P, presence, frequency, counts=counts,
                                                     logit_bias=bias)
    moved = 0
    for r in range(3):
        row = sampling.penalize(lg[r], before[r], presence[r], frequency[r])
        tok, kept, cutoff = one_row(row, r, logit_bias=bias)
        assert out['tokens'][r] == tok and out['kept'][r] == kept and bits(out['cutoff'])[r] == bits(cutoff), (V, r)
        moved += (tok, kept) != one_row(lg[r], r, logit_bias=bias)[:2]
        # only the drawn token's count grew, by one
        want = before[r].copy()
        want[tok] += 1
        assert np.array_equal(counts[r], want), (V, r)
    assert moved >= 1, 'the penalties changed no row: the path was not exercised'
    # penalties of 0 do not look at the counts (and a NULL table means no penalties): the unpenalised draw
    zero = library().rwkv_mi355x_selftest_sample_rows(lg, U, TEMPERATURE, TOP_P, [0.0] * 3, [0.0] * 3, counts=before.copy())
    plain = library().rwkv_mi355x_selftest_sample_rows(lg, U, TEMPERATURE, TOP_P, presence, frequency)
    for o in (zero, plain):
        assert [int(t) for t in o['tokens']] == [one_row(lg[r], r)[0] for r in range(3)]


class Ref64(Ref):
    """test_gpu_sampling.Ref over float64 logits as they are (Ref rounds its row to float32 first)."""

    def __init__(self, l64):
        self.l = np.asarray(l64, np.float64)
        e = np.exp(self.l - self.l.max())
        self.p = e / e.sum()
        self.values, counts = np.unique(self.l, return_counts=True)
        self.values, counts = self.values[::-1], counts[::-1]
        self.group_p = np.exp(self.values - self.l.max()) / e.sum()
        self.mass = np.cumsum(self.group_p * counts)
        self.count = np.cumsum(counts)


@pytest.mark.parametrize('V', [65, 50277, 70001])
def test_penalty_against_float64(V):
    lg = logits_for(V)
    counts = counts_for(V, lg)
    presence, frequency, temperature = 0.2, 0.2, 0.8
    for r in range(3):
        c = counts[r].astype(np.float64)
        l64 = lg[r].astype(np.float64) - np.where(c > 0, presence + c * frequency, 0.0)
        ref = Ref64(l64)
        top_p, count, cut = ref.top_p_near(0.8)
        w, C = ref.cdf(top_p, temperature)
        lo = np.concatenate([[0.0], C[:-1]])
        heavy = np.flatnonzero(w >= 4 * EPS)[:32]
        us = np.concatenate([(0.5 * (lo[heavy] + C[heavy])).astype(np.float32),
                             np.random.default_rng(V + r).random(32, dtype=np.float32)])
        n = len(us)
        table = np.ascontiguousarray(np.broadcast_to(counts[r], (n, V)))
        out = library().rwkv_mi355x_selftest_sample_rows(np.broadcast_to(lg[r], (n, V)), us, temperature, top_p,
                                                         presence, frequency, counts=table)
        tok = out['tokens'].astype(np.int64)
        assert set(out['kept']) == {count}, (V, r)
        assert abs(out['cutoff'][0] - cut) <= 1e-5 * cut
        assert list(tok[:len(heavy)]) == list(heavy)
        assert ref.kept(top_p)[tok].all()
        u64 = us.astype(np.float64)
        assert (lo[tok] - EPS <= u64).all() and (u64 < C[tok] + EPS).all()


def test_finished_rows_write_only_the_decode_input():
    V = 65536
    lg = logits_for(V)
    counts = counts_for(V, lg)
    before = counts.copy()
    done = np.array([0, 1, 0], np.uint32)
    out = library().rwkv_mi355x_selftest_sample_rows(lg, U, TEMPERATURE, TOP_P, 0.2, 0.2, counts=counts, done=done, step=4,
                                                     active=2)
    assert out['decode_tokens'][1] == 0  # an id < V for the decode step's embedding
    for k in ('tokens', 'kept', 'lengths'):
        assert out[k][1] == FILL, k
    assert bits(out['cutoff'])[1] == FILL
    assert np.array_equal(counts[1], before[1]) and list(done) == [0, 1, 0] and out['active'] == 2
    # the live rows beside it are untouched by it
    for r in (0, 2):
        row = sampling.penalize(lg[r], before[r], 0.2, 0.2)
        assert out['tokens'][r] == one_row(row, r)[0] and out['lengths'][r] == 5


def test_stop_tokens_finish_a_row():
    V = 50277
    lg = logits_for(V)
    plain = library().rwkv_mi355x_selftest_sample_rows(lg, U, TEMPERATURE, TOP_P)
    t = [int(x) for x in plain['tokens']]
    assert len(set(t)) == 3
    # 16 stop tokens; rows 0 and 2 draw one of them, row 1 does not
    others = [x for x in range(100, 200) if x not in t][:14]
    stops = others[:7] + [t[2]] + others[7:] + [t[0]]
    out = library().rwkv_mi355x_selftest_sample_rows(lg, U, TEMPERATURE, TOP_P, stop_tokens=stops, step=7)
    assert [int(x) for x in out['tokens']] == t and [int(x) for x in out['decode_tokens']] == t
    assert list(out['done']) == [1, 0, 1] and list(out['lengths']) == [8, 8, 8] and out['active'] == 1
