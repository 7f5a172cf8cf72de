"""rwkv_mi355x_generate_beam (include/rwkv_mi355x.h): one beam step on host operands and
whole calls on the tiny fixtures, against rwkv_cpp.sampling.beam_step in float64 numpy."""
import ctypes
import os

import numpy as np
import pytest

from rwkv_lib import library
from rwkv_cpp import sampling
from rwkv_cpp.rwkv_cpp_shared_library import RWKVBeam

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
P_F, P_U, P_D = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_uint32, ctypes.c_double))
RWKV_ERROR_ARGS = 1 << 8
FIXTURES = ['tiny-rwkv-4v0-660K-FP16.bin', 'tiny-rwkv-5v2-730K-FP16.bin', 'tiny-rwkv-6v0-3m-Q5_1.bin',
            'tiny-rwkv-7v0-834K-FP16.bin']
PROMPT = list(b'This is a port of [B')
FILL = 0xFFFFFFFF
SETS = ['gauss', 'equal_rows', 'const_row', 'ahead', 'mixed', 'neg_inf', 'stop_best']


def tol(V):
    """The bound tests/test_gpu_logprobs_kernel.py derives for logZ: every term of S is non-negative, so
    two associations of the sum differ by at most V * 2**-53 relative, log(S) by as much absolutely, and
    the roundings of log, of m + log(S) and of the two score operations add a few ulps of values < 100."""
    return V * 2.0 ** -52 + 1e-12


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def step_case(kind, W, V):
    """(logits [W, V], scores, finished, stop tokens) of one input set."""
    rng = np.random.default_rng(1000 * W + V + 7 * SETS.index(kind))
    logits = (rng.standard_normal((W, V)) * 4).astype(np.float32)
    scores = -rng.uniform(0.0, 5.0, W)
    finished = np.zeros(W, np.uint32)
    stop = []
    if kind == 'equal_rows':  # the cross-row ties resolve by b, then v
        logits[:] = logits[0]
        scores[:] = -1.5
    elif kind == 'const_row':  # ties within a row
        logits[W // 2] = 0.25
    elif kind == 'ahead':  # every child has the one parent
        scores = -50.0 - scores
        scores[W - 1] = 0.0
    elif kind == 'mixed':  # finished beams among the live ones' candidates
        finished[1::2] = 1  # with scores just under the live rows' median best candidate
        best = [scores[b] + sampling.logprobs(logits[b], 1)[2][0] for b in range(0, W, 2)]
        scores[1::2] = np.median(best) - rng.uniform(0.0, 1.0, finished[1::2].size)
    elif kind == 'neg_inf':
        hole = rng.random((W, V)) < 0.3
        hole[np.arange(W), np.arange(W) % V] = False
        logits[hole] = -np.inf
    elif kind == 'stop_best':
        stop = [int(logits[0].argmax()), int(rng.integers(V))]
    return logits, scores, finished, stop


@pytest.mark.parametrize('kind', SETS)
@pytest.mark.parametrize('V', ['W', 17, 1023, 1025, 65537])
@pytest.mark.parametrize('W', [1, 2, 5, 16])
def test_beam_step(W, V, kind):
    V = W if V == 'W' else V
    logits, scores, finished, stop = step_case(kind, W, V)
    parent, token, score, fin, gap = sampling.beam_step(logits, scores, finished, stop)
    print(f'W={W} V={V} {kind}: gap {gap:.3e} tol {tol(V):.3e}')
    assert gap > 2 * tol(V)
    if kind == 'ahead':
        assert (parent == W - 1).all()
    got = library().rwkv_mi355x_selftest_beam_step(logits, scores, finished, stop)
    assert np.array_equal(got[0], parent) and np.array_equal(got[1], token) and np.array_equal(got[3], fin)
    with np.errstate(invalid='ignore'):
        err = np.where(got[2] == score, 0.0, np.abs(got[2] - score))  # equal infinities are equal
    print(f'  max score error {err.max():.3e}')
    assert (err <= tol(V)).all()
    again = library().rwkv_mi355x_selftest_beam_step(logits, scores, finished, stop)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, again))


class Ctx:
    def __init__(self, name, slots=16):
        self.lib = library()
        self.L = self.lib.library
        self.ctx = self.lib.rwkv_init_from_file(os.path.join(GOLD, name), 1, 99)
        self.ptr = self.ctx.ptr
        self.V, self.S = self.L.rwkv_get_n_vocab(self.ptr), self.L.rwkv_get_state_len(self.ptr)
        self.lib.rwkv_mi355x_batch_reserve(self.ctx, slots)

    def start(self, tokens=()):
        """Fresh state, the prompt as one sequence, then `tokens` one decode step each."""
        assert self.L.rwkv_mi355x_state_upload(self.ptr, None)
        self.lib.rwkv_mi355x_eval_device(self.ctx, PROMPT)
        for t in tokens:
            self.lib.rwkv_mi355x_eval_device(self.ctx, [int(t)])

    def state(self):
        st = np.zeros(self.S, np.float32)
        assert self.L.rwkv_mi355x_state_download(self.ptr, st.ctypes.data_as(P_F))
        return st

    def logits(self):
        lg = np.zeros(self.V, np.float32)
        assert self.L.rwkv_mi355x_debug_buffer(self.ptr, b'logits', lg.ctypes.data_as(ctypes.c_void_p), lg.nbytes) == lg.nbytes
        return lg

    def host_search(self, W, n, stop, alpha):
        """Beam search on the host: sampling.beam_step over rwkv_mi355x_eval_batch with host states.
        Returns ([(tokens, score, finished)] in rank order, the smallest gap of any step)."""
        self.start()
        states, logits = np.zeros((W, self.S), np.float32), np.zeros((W, self.V), np.float32)
        states[0], logits[0] = self.state(), self.logits()
        scores, fin = np.zeros(W), np.array([0] + [2] * (W - 1), np.uint32)
        toks, gap = [[] for _ in range(W)], np.inf
        for _ in range(n):
            parent, token, scores, fin, g = sampling.beam_step(logits, scores, fin, stop)
            gap = min(gap, g)
            toks = [toks[p] + [int(t)] * bool(t != FILL) for p, t in zip(parent, token)]
            if not (fin == 0).any():
                break
            states, out = np.ascontiguousarray(states[parent]), np.zeros_like(states)
            self.lib.rwkv_mi355x_eval_batch(self.ctx, [int(t) if f == 0 else 0 for t, f in zip(token, fin)],
                                            states.ctypes.data, out.ctypes.data, logits.ctypes.data)
            states = out
        rank = sampling.beam_rank(scores, [len(t) for t in toks], alpha)
        return [(toks[r], scores[r], int(fin[r])) for r in rank], gap

    def check_against_host(self, W, n, stop, alpha):
        want, gap = self.host_search(W, n, stop, alpha)
        print(f'W={W} stop={stop} alpha={alpha}: gap {gap:.3e}, tol {n * tol(self.V):.3e}')
        assert gap > 2 * n * tol(self.V)
        self.start()
        ref_state, ref_logits = self.state(), self.logits()
        out = self.lib.rwkv_mi355x_generate_beam(self.ctx, W, n, stop, alpha, check_every=1)
        assert np.array_equal(bits(self.state()), bits(ref_state)) and np.array_equal(bits(self.logits()), bits(ref_logits))
        for j, (toks, score, fin) in enumerate(want):
            assert list(out['tokens'][j]) == toks + [FILL] * (n - len(toks)), j
            assert out['lengths'][j] == len(toks) and out['finished'][j] == fin
            assert abs(out['scores'][j] - score) <= n * tol(self.V)
        # the reorder: an unfinished beam's slot holds the state and logits of its tokens evaluated alone
        for j, (toks, _, fin) in enumerate(want):
            if fin:
                assert not self.L.rwkv_mi355x_batch_load(self.ptr, int(out['rows'][j]))
                continue
            self.lib.rwkv_mi355x_batch_load(self.ctx, int(out['rows'][j]))
            got_state, got_logits = self.state(), self.logits()
            self.start(toks)
            assert np.array_equal(bits(got_state), bits(self.state())), j
            assert np.array_equal(bits(got_logits), bits(self.logits())), j
        return want


@pytest.fixture(scope='module', params=FIXTURES)
def ctx(request):
    c = Ctx(request.param)
    yield c
    c.lib.rwkv_free(c.ctx)


def test_width_one_is_greedy(ctx):
    ctx.start()
    want = ctx.lib.rwkv_mi355x_generate(ctx.ctx, 12, temperature=0.0)
    ctx.start()
    out = ctx.lib.rwkv_mi355x_generate_beam(ctx.ctx, 1, 12)
    assert list(out['tokens'][0]) == want and out['lengths'][0] == 12 and out['steps'] == 12


@pytest.mark.parametrize('W', [4, 16])
def test_beam_equals_host_search(ctx, W):
    want = ctx.check_against_host(W, 12, [], 0.0)
    # the first token of these beams that as a stop token finishes some beams of the host search and
    # not all: finished beams ride along, and the final ranking mixes both kinds
    def mixed(beams):
        return any(f for _, _, f in beams) and not all(f for _, _, f in beams)
    stop = next([t] for toks, _, _ in want for t in toks if mixed(ctx.host_search(W, 12, [t], 0.0)[0]))
    for alpha in (0.0, 1.0):
        assert mixed(ctx.check_against_host(W, 12, stop, alpha))


def call(c, width=2, n=4, n_stop=0, stop=(0,), alpha=0.0, null=None):
    """One raw call; `null`: the index of an output pointer passed as NULL.  Returns its result."""
    stop_arr = (ctypes.c_uint32 * len(stop))(*stop)
    p = RWKVBeam(width, n_stop, stop_arr, alpha, 0)
    W = max(1, min(width, 16))
    outs = [np.zeros(W * max(1, min(n, 16)), np.uint32), np.zeros(W, np.uint32), np.zeros(W, np.float64),
            np.zeros(W, np.uint32), np.zeros(W, np.uint32)]
    args = [None if i == null else x.ctypes.data_as(P_D if x.dtype == np.float64 else P_U) for i, x in enumerate(outs)]
    return c.L.rwkv_mi355x_generate_beam(c.ptr, ctypes.byref(p), n, *args, None)


ERRORS = [dict(width=0), dict(width=17), dict(width=5), dict(n=0), dict(n=65537), dict(n_stop=17, stop=(0,) * 17),
          dict(n_stop=1, stop=(1 << 20,)), dict(alpha=-1.0), dict(alpha=float('nan')), dict(alpha=float('inf')), dict(invalid=True)] + \
         [dict(null=i) for i in range(5)]


@pytest.mark.parametrize('case', ERRORS, ids=str)
def test_argument_errors(case):
    c = Ctx('tiny-rwkv-6v0-3m-Q5_1.bin', slots=4)
    c.start()
    c.lib.rwkv_mi355x_batch_store(c.ctx, 0)
    slot = c.state(), c.logits()
    case = dict(case)
    if case.pop('invalid', False):  # the logits no longer follow the state
        assert c.L.rwkv_mi355x_state_upload(c.ptr, None)
    own = c.state(), c.logits()
    assert not call(c, **case) and c.lib.library.rwkv_get_last_error(c.ptr) == RWKV_ERROR_ARGS
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(own, (c.state(), c.logits())))
    c.lib.rwkv_mi355x_batch_load(c.ctx, 0)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(slot, (c.state(), c.logits())))
    c.lib.rwkv_free(c.ctx)
