"""rwkv_mi355x_{sample,generate,generate_batch,generate_queue}_logprobs (include/rwkv_mi355x.h): the
calls draw the tokens of their plain siblings, bit for bit, and report for every draw the
log-probabilities sampling.logprobs gives for the row the token was drawn from -- replayed on the host
from the same prefix (rwkv_mi355x_eval_device with logits_out, sampling.penalize with running counts,
the bias).

Tolerance: ids exactly; values to V * 2**-52 + 1e-12 (twice the worst-case bound on a sum of V
non-negative float64 terms in any association, plus room for the device exp / log and the final
subtraction at |values| < 100)."""
import ctypes
import os

import numpy as np
import pytest

from rwkv_lib import library, RWKVModel
from rwkv_cpp import sampling
from rwkv_cpp.rwkv_cpp_shared_library import make_batch_sampling, make_logprobs, make_sampling
from test_gpu_generate_batch import BIAS, FIXTURES, GOLD, V6, bits, row_params
from test_gpu_generate_queue import CAPS7, ROWS7, QCtx

pytestmark = pytest.mark.gpu

P_U = ctypes.POINTER(ctypes.c_uint32)
RWKV_ERROR_ARGS = 1 << 8
FILL_U32, FILL_U64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope='module')
def world_model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp('generate_logprobs') / 'world-v6.bin')
    assert library().library.rwkv_mi355x_write_synthetic_model(p.encode(), 6, 65536, 256, 3, 0, b'Q5_1', 11)
    return p


def tol(V):
    return V * 2.0 ** -52 + 1e-12


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def is_fill(lp, r, cols):
    """Columns `cols` of row r hold the library's fill: every byte 0xFF."""
    return ((bits64(lp.token_logprob[r, cols]) == FILL_U64).all() and (lp.top_ids[r, cols] == FILL_U32).all()
            and (bits64(lp.top_logprobs[r, cols]) == FILL_U64).all())


class LCtx(QCtx):
    def generate(self, r, n, q, k=None):
        """Row r's prompt, then rwkv_mi355x_generate[_logprobs]: (tokens, state, logits, Logprobs or None)."""
        self.start(r)
        out = library().rwkv_mi355x_generate(self, n, q['temperature'], q['top_p'], q['logit_bias'], q['seed'], q['offset'],
                                             None, k)
        toks, lp = (out, None) if k is None else out
        return toks, self.state(), self.logits(), lp

    def batch(self, B, n, k=None, fill=True, **kw):
        """(tokens, lengths, steps, Logprobs or None, [(state, logits) of every slot])."""
        if fill:
            self.fill(B)
        p = make_batch_sampling(B, kw.get('temperature', 1.0), kw.get('top_p', 0.8), kw.get('presence'), kw.get('frequency'),
                                kw.get('logit_bias'), kw['seeds'], kw.get('offsets', 0), kw.get('stop_tokens', ()),
                                kw.get('keep_counts', False), kw.get('check_every', 0))
        out = library().rwkv_mi355x_generate_batch(self, B, n, p, k)
        return out[0], out[1], out[2], (out[3] if k is not None else None), [self.slot(r) for r in range(B)]

    def queue_lp(self, caps, lanes, kw, k=None, n=None, stop_tokens=()):
        self.fill(len(caps))
        out = library().rwkv_mi355x_generate_queue(
            self, caps, lanes, kw.get('temperature', 1.0), kw.get('top_p', 0.8), kw.get('presence'), kw.get('frequency'),
            kw.get('logit_bias'), kw['seeds'], kw.get('offsets', 0), stop_tokens, 0, n, k)
        out['slots'] = [self.slot(s) for s in range(len(caps))]
        return out

    def replay(self, r, tokens, kw, lp, k):
        """Sequence r's draws on the host: before token i the logits of the same prefix, penalised with
        the running counts and biased; column i of lp against sampling.logprobs of that row."""
        q = row_params(kw, r)
        lg = np.zeros(self.V, np.float32)
        self.start(r, lg)
        counts = np.zeros(self.V, np.uint32)
        for i, t in enumerate(tokens):
            row = sampling.penalize(lg, counts, q['presence'], q['frequency'])
            for b, v in (q['logit_bias'] or {}).items():
                row[b] = row[b] + np.float32(v)
            logz, ids, vals = sampling.logprobs(row, k)
            assert list(lp.top_ids[i]) == list(ids), (r, i)
            assert np.abs(lp.top_logprobs[i] - vals).max(initial=0.0) <= tol(self.V), (r, i)
            assert abs(lp.token_logprob[i] - (np.float64(row[t]) - logz)) <= tol(self.V), (r, i)
            for j in range(k):
                if int(ids[j]) == t:
                    assert bits64(lp.token_logprob[i:i + 1])[0] == bits64(lp.top_logprobs[i][j:j + 1])[0], (r, i)
            counts[t] += 1
            if i + 1 < len(tokens):
                self.step([t], lg)


def same_slots(a, b):
    return all(np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1])) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. the tokens do not change
@pytest.mark.parametrize('name', FIXTURES)
def test_generate_draws_the_same_tokens(name):
    c = LCtx(os.path.join(GOLD, name))
    try:
        for q in (dict(temperature=0.0, top_p=0.5, logit_bias=None, seed=3, offset=0),
                  dict(temperature=0.8, top_p=0.5, logit_bias=BIAS, seed=5, offset=2)):
            want = c.generate(1, 9, q)
            for k in (0, 5):
                got = c.generate(1, 9, q, k)
                assert got[0] == want[0] and np.array_equal(bits(got[1]), bits(want[1])), (q, k)
                assert np.array_equal(bits(got[2]), bits(want[2])), (q, k)
                lp = got[3]
                assert lp.token_logprob.shape == (9,) and lp.top_ids.shape == (9, k)
                assert np.isfinite(lp.token_logprob).all() and (lp.token_logprob <= 0.0).all()
                assert (lp.top_ids < c.V).all() and np.isfinite(lp.top_logprobs).all()
    finally:
        c.free()


@pytest.mark.parametrize('name', FIXTURES)
def test_generate_batch_draws_the_same_tokens(name):
    c = LCtx(os.path.join(GOLD, name))
    try:
        kw = dict(temperature=[0.0, 0.9, 1.0], top_p=[0.5, 0.9, 1.0], seeds=[7, 8, 9], offsets=[0, 1, 2], presence=0.3,
                  frequency=0.2, logit_bias=BIAS)
        free = c.batch(3, 8, **kw)[0]
        stops = [int(free[1][3])]  # row 1 stops on its fourth token at the latest
        runs = []
        for k in (None, 0, 5):
            first = c.batch(3, 6, k, stop_tokens=stops, **kw)
            more = c.batch(3, 4, k, fill=False, stop_tokens=stops, keep_counts=True, **dict(kw, offsets=[6, 7, 8]))
            runs.append((first, more))
        assert runs[0][0][1][1] <= 4
        for (first, more), k in zip(runs[1:], (0, 5)):
            for got, want in ((first, runs[0][0]), (more, runs[0][1])):
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], k
                assert same_slots(got[4], want[4]), k
                for r in range(3):  # drawn columns are filled, the columns after them hold the fill
                    n = int(got[1][r])
                    assert np.isfinite(got[3].token_logprob[r, :n]).all() and (got[3].top_ids[r, :n] < c.V).all(), (k, r)
                    assert is_fill(got[3], r, slice(n, None)), (k, r)
            # row 1 was finished when the continuation began: nothing of it was written
            assert more[1][1] == 0 and is_fill(more[3], 1, slice(0, None))
    finally:
        c.free()


@pytest.mark.parametrize('name', FIXTURES)
def test_generate_queue_draws_the_same_tokens(name):
    c = LCtx(os.path.join(GOLD, name))
    try:
        free = c.queue_lp(CAPS7, 3, ROWS7, n=8)
        stops = [int(free['tokens'][4][2])]  # the longest sequence ends early
        want = c.queue_lp(CAPS7, 3, ROWS7, n=8, stop_tokens=stops)
        assert want['lengths'][4] <= 3
        for k in (0, 5):
            got = c.queue_lp(CAPS7, 3, ROWS7, k, n=8, stop_tokens=stops)
            for key in ('tokens', 'lengths', 'lane', 'start'):
                assert np.array_equal(got[key], want[key]), (k, key)
            assert got['steps'] == want['steps'] and same_slots(got['slots'], want['slots']), k
            for s in range(7):
                n = int(got['lengths'][s])
                assert np.isfinite(got['logprobs'].token_logprob[s, :n]).all(), (k, s)
                assert is_fill(got['logprobs'], s, slice(n, None)), (k, s)
    finally:
        c.free()


# ------------------------------------------------------------------ 2. the values
def test_batch_values_are_those_of_the_replayed_rows():
    c, ref = LCtx(os.path.join(GOLD, V6)), LCtx(os.path.join(GOLD, V6))
    try:
        kw = dict(temperature=[0.0, 0.9], top_p=[0.5, 0.95], seeds=[21, 22], offsets=[0, 4], presence=0.4, frequency=0.3,
                  logit_bias=BIAS)
        free = c.batch(2, 10, **kw)[0]
        stops = [int(free[1][5])]
        toks, lens, _, lp, _ = c.batch(2, 10, 5, stop_tokens=stops, **kw)
        assert lens[1] <= 6 and int(toks[1][lens[1] - 1]) in stops  # the stop token's column is reported too
        for r in range(2):
            n = int(lens[r])
            ref.replay(r, [int(t) for t in toks[r][:n]], kw, type(lp)(*(x[r, :n] for x in lp)), 5)
            assert is_fill(lp, r, slice(n, None))
    finally:
        c.free()
        ref.free()


def test_queue_values_are_those_of_the_replayed_sequences():
    c, ref = LCtx(os.path.join(GOLD, V6)), LCtx(os.path.join(GOLD, V6))
    try:
        kw = dict(ROWS7, presence=0.25, frequency=0.125)
        out = c.queue_lp(CAPS7, 3, kw, 4, n=8)
        start = [int(x) for x in out['start']]
        odd = next(s for s in range(7) if start[s] % 2 == 1 and out['lengths'][s] > 1)
        even = next(s for s in range(7) if start[s] > 0 and start[s] % 2 == 0)
        for s in (odd, even):
            n = int(out['lengths'][s])
            ref.replay(s, [int(t) for t in out['tokens'][s][:n]], kw, type(out['logprobs'])(*(x[s, :n] for x in out['logprobs'])), 4)
    finally:
        c.free()
        ref.free()


def test_token_logprobs_are_the_scores_of_the_sequence():
    """No penalties, no bias: token_logprob[i] = -loss[i] of rwkv_mi355x_score_sequence over the same
    tokens from the same start state."""
    c = LCtx(os.path.join(GOLD, V6))
    try:
        q = dict(temperature=0.9, top_p=0.9, logit_bias=None, seed=31, offset=0)
        toks, _, _, lp = c.generate(2, 12, q, 0)
        prompt = c.prompt(2)
        assert c.L.rwkv_mi355x_state_upload(c.ptr, None)
        seq = prompt + toks[:-1]
        losses, _, _ = library().rwkv_mi355x_score_sequence(c, seq, seq[1:] + toks[-1:])
        assert np.abs(lp.token_logprob + losses[len(prompt) - 1:]).max() <= tol(c.V)
    finally:
        c.free()


def test_sample_reports_the_draw():
    c = LCtx(os.path.join(GOLD, V6))
    try:
        lg = np.zeros(c.V, np.float32)
        c.start(0, lg)
        before = (c.state(), c.logits())
        tok, lp = library().rwkv_mi355x_sample(c, 0.7, 0.8, BIAS, 5, 1, logprobs=20)
        assert tok == library().rwkv_mi355x_sample(c, 0.7, 0.8, BIAS, 5, 1)
        row = lg.copy()
        for b, v in BIAS.items():
            row[b] = row[b] + np.float32(v)
        logz, ids, vals = sampling.logprobs(row, 20)
        assert list(lp.top_ids) == list(ids) and np.abs(lp.top_logprobs - vals).max() <= tol(c.V)
        assert abs(lp.token_logprob - (np.float64(row[tok]) - logz)) <= tol(c.V)
        assert same_slots([before], [(c.state(), c.logits())])
    finally:
        c.free()


# ------------------------------------------------------------------ 3. one large vocabulary
def test_world_vocabulary(world_model):
    c, ref = LCtx(world_model), LCtx(world_model)
    try:
        caps = [3, 5, 2, 4]
        kw = dict(temperature=[1.0, 0.9, 0.0, 0.8], top_p=[0.9, 1.0, 0.8, 0.5], seeds=[31, 32, 33, 34], offsets=[0, 3, 0, 7],
                  presence=[0.2, 0.0, 0.2, 0.0], frequency=[0.2, 0.0, 0.1, 0.0], logit_bias=BIAS)
        want = c.queue_lp(caps, 2, kw)
        got = c.queue_lp(caps, 2, kw, 20)
        for key in ('tokens', 'lengths', 'lane', 'start'):
            assert np.array_equal(got[key], want[key]), key
        assert same_slots(got['slots'], want['slots'])
        for s in (0, 3):  # one admitted at step 0, one later
            n = int(got['lengths'][s])
            ref.replay(s, [int(t) for t in got['tokens'][s][:n]], kw, type(got['logprobs'])(*(x[s, :n] for x in got['logprobs'])), 20)
        assert got['start'][3] > 0
    finally:
        c.free()
        ref.free()


# ------------------------------------------------------------------ 4. errors
def test_argument_errors_leave_everything_alone():
    c = LCtx(os.path.join(GOLD, V6))
    try:
        L = c.L
        c.fill(2)
        c.start(0)
        before = [c.slot(0), c.slot(1)]
        c.start(0)
        own = (c.state(), c.logits())
        p, bp = make_sampling(0.8, 0.5, None, 1, 0), make_batch_sampling(2, 0.8, 0.5, seeds=[1, 2])
        tok, lens, caps = np.zeros((2, 4), np.uint32), np.zeros(2, np.uint32), np.array([4, 4], np.uint32)
        calls = [
            lambda lp: L.rwkv_mi355x_sample_logprobs(c.ptr, ctypes.byref(p), tok.ctypes.data_as(P_U), lp),
            lambda lp: L.rwkv_mi355x_generate_logprobs(c.ptr, ctypes.byref(p), 4, tok.ctypes.data_as(P_U), None, lp),
            lambda lp: L.rwkv_mi355x_generate_batch_logprobs(c.ptr, 2, ctypes.byref(bp), 4, tok.ctypes.data_as(P_U),
                                                             lens.ctypes.data_as(P_U), None, lp),
            lambda lp: L.rwkv_mi355x_generate_queue_logprobs(c.ptr, 2, 2, ctypes.byref(bp), caps.ctypes.data_as(P_U), 4,
                                                             tok.ctypes.data_as(P_U), lens.ctypes.data_as(P_U), None, None,
                                                             None, lp)]

        def bad(kind):
            lp, _ = make_logprobs(2, 4, 5)
            if kind == 'above 20':
                lp.top_k = 21
            else:
                setattr(lp, kind, None)
            return lp

        kinds = ['above 20', 'token_logprob', 'top_ids', 'top_logprobs']
        for i, call in enumerate(calls):
            for kind in kinds:
                lp = bad(kind)
                assert not call(ctypes.byref(lp)) and c.error() == RWKV_ERROR_ARGS, (i, kind)
        assert same_slots([own], [(c.state(), c.logits())])
        assert same_slots(before, [c.slot(0), c.slot(1)])
        # top_k == 0 needs neither of the two top arrays, and lp == NULL is the plain call
        c.start(0)
        lp, arrays = make_logprobs(1, 4, 0)
        lp.top_ids, lp.top_logprobs = None, None
        a = np.zeros(4, np.uint32)
        assert L.rwkv_mi355x_generate_logprobs(c.ptr, ctypes.byref(p), 4, a.ctypes.data_as(P_U), None, ctypes.byref(lp))
        assert np.isfinite(arrays.token_logprob).all()
        c.start(0)
        b = np.zeros(4, np.uint32)
        assert L.rwkv_mi355x_generate_logprobs(c.ptr, ctypes.byref(p), 4, b.ctypes.data_as(P_U), None, None)
        st = (c.state(), c.logits())
        c.start(0)
        d = np.zeros(4, np.uint32)
        assert L.rwkv_mi355x_generate(c.ptr, ctypes.byref(p), 4, d.ctypes.data_as(P_U), None)
        assert list(a) == list(b) == list(d) and same_slots([st], [(c.state(), c.logits())])
    finally:
        c.free()


def test_top_k_above_a_small_vocabulary_is_refused(tmp_path):
    """top_k <= 20 but above n_vocab: a context of a 12-token model, on which nothing is evaluated (the
    check needs the vocabulary only and comes first)."""
    path = str(tmp_path / 'v12.bin')
    assert library().library.rwkv_mi355x_write_synthetic_model(path.encode(), 4, 12, 64, 1, 0, b'FP16', 3)
    L = library().library
    ptr = L.rwkv_init_from_file(path.encode(), 1, 99)
    assert ptr
    try:
        assert L.rwkv_get_n_vocab(ptr) == 12
        p, bp = make_sampling(0.8, 0.5, None, 1, 0), make_batch_sampling(1, 0.8, 0.5, seeds=[1])
        tok, one = np.zeros(4, np.uint32), np.array([4], np.uint32)
        lp, _ = make_logprobs(1, 4, 13)
        t, o = tok.ctypes.data_as(P_U), one.ctypes.data_as(P_U)
        for call in (lambda: L.rwkv_mi355x_sample_logprobs(ptr, ctypes.byref(p), t, ctypes.byref(lp)),
                     lambda: L.rwkv_mi355x_generate_logprobs(ptr, ctypes.byref(p), 4, t, None, ctypes.byref(lp)),
                     lambda: L.rwkv_mi355x_generate_batch_logprobs(ptr, 1, ctypes.byref(bp), 4, t, o, None, ctypes.byref(lp)),
                     lambda: L.rwkv_mi355x_generate_queue_logprobs(ptr, 1, 1, ctypes.byref(bp), o, 4, t, o, None, None, None,
                                                                   ctypes.byref(lp))):
            assert not call() and L.rwkv_get_last_error(ptr) == RWKV_ERROR_ARGS
    finally:
        L.rwkv_free(ptr)


# ------------------------------------------------------------------ 5. the Python layer
def test_python_generate_batch_returns_per_row_arrays():
    m = RWKVModel(library(), os.path.join(GOLD, V6), gpu_layer_count=99)
    try:
        prompts = [[10, 20, 30], [40, 50], [60]]
        plain = m.generate_batch(prompts, 6, temperature=[0.0, 0.9, 1.0], stop_tokens=[0], seeds=[1, 2, 3])
        assert isinstance(plain, list) and all(isinstance(x, list) for x in plain)
        lists, lps = m.generate_batch(prompts, 6, temperature=[0.0, 0.9, 1.0], stop_tokens=[0], seeds=[1, 2, 3], logprobs=3)
        assert lists == plain and len(lps) == 3
        for toks, lp in zip(lists, lps):
            assert lp.token_logprob.shape == (len(toks),) and lp.top_ids.shape == (len(toks), 3)
            assert lp.top_logprobs.shape == (len(toks), 3) and np.isfinite(lp.token_logprob).all()
        m.eval_sequence(prompts[0], None, use_numpy=True)
        tok, lp = m.sample(temperature=0.0, logprobs=2)
        assert tok == int(lp.top_ids[0]) and lp.token_logprob == lp.top_logprobs[0]
        toks, lp = m.generate(5, temperature=0.0, logprobs=1)
        assert toks == [int(i) for i in lp.top_ids[:, 0]] and np.array_equal(lp.token_logprob, lp.top_logprobs[:, 0])
    finally:
        m.free()
