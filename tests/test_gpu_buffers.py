"""The engine's device buffers grow on demand (csrc/devbuf.hpp, Engine::grow): a context whose
buffers grew in the middle of its life -- and whose captured graphs were dropped with the buffers
they pointed at -- gives the bits of a fresh context that reached the large size directly, and goes
on giving the small size's bits afterwards."""
import ctypes
import os

import numpy as np
import pytest

from oracle_ctypes import assert_bits_equal
from rwkv_lib import RWKVModel, library
from test_gpu_batch import contexts, prefixes
from test_gpu_generate import Ctx as GenCtx
from test_gpu_generate_batch import Ctx as BatchCtx
from test_gpu_score import Ctx as ScoreCtx

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
V6 = os.path.join(GOLD, 'tiny-rwkv-6v0-3m-Q5_1.bin')
TEXT = list(b'This is a port of [BlinkDL/RWKV-LM](https://github.com/BlinkDL/RWKV-LM')
SAMPLED = dict(temperature=0.8, top_p=0.5, seed=7)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_generate_regrows_its_token_buffer():
    """gen_tokens_ starts at 64 tokens: 8, then 80 (regrown to 128), then 8 again."""
    c, ref = GenCtx(V6), GenCtx(V6)
    try:
        ref.start()
        want_lg = np.zeros(ref.V, np.float32)
        want = ref.generate(80, want_lg, **SAMPLED)
        c.start()
        assert c.generate(8, **SAMPLED) == want[:8]
        c.start()
        lg = np.zeros(c.V, np.float32)
        assert c.generate(80, lg, **SAMPLED) == want
        assert np.array_equal(bits(lg), bits(want_lg))
        assert np.array_equal(bits(c.state()), bits(ref.state()))
        c.start()
        assert c.generate(8, **SAMPLED) == want[:8]
    finally:
        c.free()
        ref.free()


def test_score_regrows_across_the_chunk_limit():
    """The score buffers start at 1024 tokens and a chunk is 1024 tokens: 1100 tokens regrow them to
    2048 and leave a second chunk of 76."""
    c, ref = ScoreCtx(V6), ScoreCtx(V6)
    try:
        tokens = [(TEXT[i % len(TEXT)] + i // len(TEXT)) % c.V for i in range(1100)]
        targets = tokens[1:] + [c.V - 1]
        want_loss, want_arg, _ = ref.score(tokens, targets)
        want_state = ref.state()
        c.fresh()
        small = c.score(tokens[:40], targets[:40])
        c.fresh()
        loss, arg, _ = c.score(tokens, targets)
        assert np.array_equal(loss, want_loss) and np.array_equal(arg, want_arg)
        assert np.array_equal(bits(c.state()), bits(want_state))
        assert np.array_equal(small[0], want_loss[:40]) and np.array_equal(small[1], want_arg[:40])
        c.fresh()
        again = c.score(tokens[:40], targets[:40])
        assert np.array_equal(again[0], small[0]) and np.array_equal(again[1], small[1])
    finally:
        c.free()
        ref.free()


def test_generate_batch_regrows_its_token_buffer():
    """gtokens_ starts at 1024 tokens: B n = 24, then 1200 (regrown to 2048)."""
    kw = dict(temperature=[0.0, 1.0, 0.7], top_p=[0.8, 1.0, 0.8], seeds=[11, 12, 13], offsets=[0, 3, 0])
    c, ref = BatchCtx(V6), BatchCtx(V6)
    try:
        want, want_len, want_steps = ref.run(3, n=400, **kw)
        assert list(want_len) == [400] * 3 and want_steps == 400
        small, small_len, _ = c.run(3, n=8, **kw)  # reserves the slots and stores the prompts
        assert np.array_equal(small, want[:, :8]) and list(small_len) == [8] * 3
        toks, lens, steps = c.run(3, n=400, **kw)  # stores the same prompts again
        assert np.array_equal(toks, want) and np.array_equal(lens, want_len) and steps == want_steps
        for r in range(3):
            (st, lg), (wst, wlg) = c.slot(r), ref.slot(r)
            assert np.array_equal(bits(st), bits(wst)) and np.array_equal(bits(lg), bits(wlg)), r
    finally:
        c.free()
        ref.free()


def test_batched_staging_regrows_under_replay():
    """eval_batch with host states at B = 5, 5, 20, 20, 5: the staging buffers go from 8 rows to 32
    between captured graphs, every second call of a size replays its graph.  Every row of every call
    is rwkv_eval of that token and state (a second context's)."""
    m, ref = RWKVModel(library(), V6), RWKVModel(library(), V6)
    try:
        states = contexts(ref, prefixes(20, ref.n_vocab))
        toks = [(97 + 13 * i) % ref.n_vocab for i in range(20)]
        want = [ref.eval(toks[i], states[i].copy(), None, None, use_numpy=True) for i in range(20)]
        want = [(lg.copy(), st.copy()) for lg, st in want]
        for call, B in enumerate([5, 5, 20, 20, 5]):
            blg, bst = m.eval_batch(toks[:B], states[:B])
            for i in range(B):
                assert_bits_equal(blg[i], want[i][0], f'call {call} context {i} logits')
                assert_bits_equal(bst[i], want[i][1], f'call {call} context {i} state')
    finally:
        m.free()
        ref.free()


def test_scratch_moves_under_captured_batched_graphs():
    """B = 16 is the first size whose quantized matmuls take the tiled GEMM (Engine::forward_range:
    batch_gemm_min_ = 16), whose scratch (gy_, part_, m2_ for Q5_1) the captured step points at.  A
    200-token sequence moves all three (and the workspace): the batched graphs must be gone."""
    m = RWKVModel(library(), V6)
    try:
        states = contexts(m, prefixes(16, m.n_vocab))
        toks = [(97 + 13 * i) % m.n_vocab for i in range(16)]
        first = m.eval_batch(toks, states)  # eager
        for what in ('capture', 'replay'):
            lg, st = m.eval_batch(toks, states)
            assert_bits_equal(lg, first[0], f'{what}: logits')
            assert_bits_equal(st, first[1], f'{what}: states')
        m.eval_sequence([TEXT[i % len(TEXT)] for i in range(200)], None, use_numpy=True)
        lg, st = m.eval_batch(toks, states)
        assert_bits_equal(lg, first[0], 'after the sequence: logits')
        assert_bits_equal(st, first[1], 'after the sequence: states')
    finally:
        m.free()


@pytest.mark.parametrize('name', ['tiny-rwkv-5v2-730K-FP16.bin', 'tiny-rwkv-6v0-3m-Q5_1.bin'])
def test_workspace_regrows_between_decode_graphs(name):
    """Two decode steps capture both parities' graphs at capacity 1; a 40-token sequence replaces
    the workspace they point at; two more decode steps.  The serial sequence path and the decode
    agree bit for bit (test_gpu_parity.py), so the result is that of 44 single steps."""
    c, ref = GenCtx(os.path.join(GOLD, name)), GenCtx(os.path.join(GOLD, name))
    try:
        tokens = [TEXT[i % len(TEXT)] % c.V for i in range(44)]
        want_lg = np.zeros(ref.V, np.float32)
        assert ref.L.rwkv_mi355x_state_upload(ref.ptr, None)
        for t in tokens:
            ref.step([t], want_lg)
        lg = np.zeros(c.V, np.float32)
        assert c.L.rwkv_mi355x_state_upload(c.ptr, None)
        for part in ([tokens[0]], [tokens[1]], tokens[2:42], [tokens[42]], [tokens[43]]):
            c.step(part, lg)
        assert np.array_equal(bits(lg), bits(want_lg))
        assert np.array_equal(bits(c.state()), bits(ref.state()))
    finally:
        c.free()
        ref.free()
