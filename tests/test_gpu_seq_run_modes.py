"""No mode of one forward leaks into the next call on the same context.

The sequence program (engine_sequence.hip) serves a plain sequence, a batched decode step, a packed
prefill chunk and the head tiles of the scorer and the prefill; which of them a forward is comes as an
argument (SeqRun), and the decode program gets its token the same way.  One context runs, in this
order, a sequence of T = 33, rwkv_mi355x_eval_batch with B = 2, rwkv_mi355x_score_sequence with
T = 34, rwkv_mi355x_prefill_batch of two rows of 1 and 5 tokens and one decode token; each result must
equal, bit for bit, the same call made on a freshly created context given the same input state.
Nothing here takes a tolerance.

One test per tiny fixture: v4, v5.2 and v7 in FP16, v6 in Q5_1 (tests/golden has no FP16 file of it).
"""
import ctypes
import os

import numpy as np
import pytest
import torch  # noqa: F401  before librwkv initialises HIP (torch's own HIP runtime must come up first)

from rwkv_lib import library

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
FIXTURES = ['tiny-rwkv-4v0-660K-FP16.bin', 'tiny-rwkv-5v2-730K-FP16.bin', 'tiny-rwkv-6v0-3m-Q5_1.bin',
            'tiny-rwkv-7v0-834K-FP16.bin']
P_F = ctypes.POINTER(ctypes.c_float)


class Ctx:
    def __init__(self, path):
        self.lib = library()
        self.L = self.lib.library
        self.ctx = self.lib.rwkv_init_from_file(path, 1, 99)
        self.ptr = self.ctx.ptr
        self.V = self.L.rwkv_get_n_vocab(self.ptr)
        self.n = self.L.rwkv_get_state_len(self.ptr)

    def free(self):
        self.lib.rwkv_free(self.ctx)

    def upload(self, state):
        assert self.L.rwkv_mi355x_state_upload(self.ptr, None if state is None else state.ctypes.data_as(P_F))

    def state(self):
        st = np.zeros(self.n, np.float32)
        assert self.L.rwkv_mi355x_state_download(self.ptr, st.ctypes.data_as(P_F))
        return st

    def logits(self):
        lg = np.zeros(self.V, np.float32)
        assert self.L.rwkv_mi355x_debug_buffer(self.ptr, b'logits', lg.ctypes.data_as(ctypes.c_void_p), lg.nbytes) == lg.nbytes
        return lg

    # the five calls: each takes its input state (None: whatever the context holds) and returns arrays
    def sequence(self, state, tokens):
        if state is not None:
            self.upload(state)
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        lg = np.zeros(self.V, np.float32)
        assert self.L.rwkv_mi355x_eval_device(self.ptr, arr, len(tokens), True, lg.ctypes.data_as(P_F), True)
        return [lg, self.state()]

    def batch(self, states, tokens):
        out_states = np.zeros_like(states)
        lg = np.zeros((len(tokens), self.V), np.float32)
        self.lib.rwkv_mi355x_eval_batch(self.ctx, tokens, states.ctypes.data, out_states.ctypes.data, lg.ctypes.data)
        return [lg, out_states]

    def score(self, state, tokens, targets):
        if state is not None:
            self.upload(state)
        losses, argmax, lg = self.lib.rwkv_mi355x_score_sequence(self.ctx, tokens, targets, True)
        return [losses, argmax, lg, self.state(), self.logits()]

    def prefill(self, prompts):
        self.lib.rwkv_mi355x_batch_reserve(self.ctx, len(prompts))
        self.lib.rwkv_mi355x_prefill_batch(self.ctx, prompts, list(range(len(prompts))))
        out = []
        for slot in range(len(prompts)):
            self.lib.rwkv_mi355x_batch_load(self.ctx, slot)
            out += [self.state(), self.logits()]
        return out


def same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f'{what}: output {i} differs from a fresh context\'s'


@pytest.mark.parametrize('fixture', FIXTURES)
def test_calls_in_a_row_equal_fresh_contexts(fixture):
    path = os.path.join(GOLD, fixture)
    one = Ctx(path)
    rng = np.random.default_rng(41)

    def toks(n):
        return [int(t) for t in rng.integers(0, one.V, n)]

    seq, pair, scored, targets, rows, last = toks(33), toks(2), toks(34), toks(34), [toks(1), toks(5)], toks(1)

    def fresh(call):
        c = Ctx(path)
        try:
            return call(c)
        finally:
            c.free()

    try:
        one.upload(None)
        got = one.sequence(None, seq)
        same(got, fresh(lambda c: c.sequence(None, seq)), 'sequence T=33')
        s1 = got[1]
        # two contexts: the one the sequence left and a fresh one
        states = np.stack([s1, fresh(lambda c: c.state())])
        same(one.batch(states, pair), fresh(lambda c: c.batch(states, pair)), 'eval_batch B=2')
        # the scorer continues from the context's own state, which eval_batch does not touch
        got = one.score(None, scored, targets)
        same(got, fresh(lambda c: c.score(s1, scored, targets)), 'score_sequence T=34')
        got = one.prefill(rows)
        same(got, fresh(lambda c: c.prefill(rows)), 'prefill_batch rows (1, 5)')
        # the decode token continues from the last slot loaded
        s4 = got[-2]
        same(one.sequence(None, last), fresh(lambda c: c.sequence(s4, last)), 'decode token')
    finally:
        one.free()
