"""Byte-DFA constrained generation (csrc/constrain.hip): k_dfa_mask and k_dfa_advance through their
self-tests against rwkv_cpp.constraint (allowed_mask, walk), and the four *_constrained calls on the
tiny fixtures against the library's own unconstrained calls.  Integer logic and a select: everything
is compared exactly."""
import functools
import os

import numpy as np
import pytest

from rwkv_lib import library, RWKVModel
from rwkv_cpp import sampling
from rwkv_cpp.constraint import DEAD, Dfa, allowed_mask, from_choices, join, walk
from rwkv_cpp.rwkv_cpp_shared_library import make_batch_sampling
from test_gpu_generate_batch import GOLD, PROMPT, V6, bits

pytestmark = pytest.mark.gpu

RWKV_ERROR_ARGS = 1 << 8
V52 = 'tiny-rwkv-5v2-730K-FP16.bin'
LENGTHS = [0, 1, 2, 15, 16, 17, 40]  # the empty token and both sides of the register / tail boundary


def table(kind):
    """A seeded random DFA with ~40 % dead transitions: one state; 40 states (256 distinct byte
    classes: no compression); the most states the LDS limit admits at 256 classes."""
    n = {'one': 1, 'classes': 40, 'limit': library().rwkv_mi355x_constraint_max_entries() // 256}[kind]
    rng = np.random.default_rng(n)
    nxt = rng.integers(0, n, (n, 256)).astype(np.uint16)
    nxt[rng.random((n, 256)) < 0.4] = DEAD
    if n > 1:
        assert len({nxt[:, b].tobytes() for b in range(256)}) == 256
    return nxt, rng.integers(0, 2, n).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def mask_case(V, kind, rows):
    nxt, acc = table(kind)
    n = nxt.shape[0]
    rng = np.random.default_rng(V + rows)
    starts = [int(s) for s in rng.integers(0, n, rows)]
    acc[starts[0]] = 1  # the stop tokens are allowed in row 0 and (another state) not in the last row
    if starts[-1] != starts[0]:
        acc[starts[-1]] = 0
    vocab = []
    for t in range(V):
        size = LENGTHS[t % len(LENGTHS)] if t < 64 else int(rng.choice(LENGTHS))
        data = bytearray(rng.integers(0, 256, size).astype(np.uint8).tobytes())
        if t % 2:  # every other token lives as long as it can from one of the start states
            q = starts[t % rows]
            for i in range(size):
                alive = np.flatnonzero(nxt[q] != DEAD)
                if alive.size == 0:
                    break
                data[i] = int(rng.choice(alive))
                q = int(nxt[q][data[i]])
        vocab.append(bytes(data))
    stops = [3, V - 1]  # lengths 15 and anything
    logits = rng.standard_normal((rows, V)).astype(np.float32)
    finished = [0] * rows
    if rows > 1:
        finished[1] = 1
    want = np.stack([allowed_mask(nxt, acc, q, vocab, stops) for q in starts])
    assert any(want[0][t] and len(vocab[t]) == 40 for t in range(V))  # a long token lives through its tail
    return nxt, acc, starts, vocab, stops, logits, finished, want


@pytest.mark.parametrize('rows', [1, 3])
@pytest.mark.parametrize('kind', ['one', 'classes', 'limit'])
@pytest.mark.parametrize('V', [1000, 1025, 4099])
def test_mask_kernel_equals_allowed_mask(V, kind, rows):
    nxt, acc, starts, vocab, stops, logits, finished, want = mask_case(V, kind, rows)
    masked, n_allowed, ended = library().rwkv_mi355x_selftest_dfa_mask(logits, vocab, Dfa(nxt, acc, starts), stops, finished)
    for r in range(rows):
        if finished[r]:  # skipped: the fill is still there
            assert np.all(masked[r] == 7.0) and n_allowed[r] == 0 and ended[r] == 1
            continue
        expect = np.where(want[r], logits[r], np.float32(-np.inf))
        assert np.array_equal(bits(masked[r]), bits(expect)), r
        assert n_allowed[r] == want[r].sum()
        assert ended[r] == (2 if want[r].sum() == 0 else 0)


def test_advance_kernel_equals_walk():
    nxt, _, _, vocab, _, _, _, _ = mask_case(1025, 'classes', 3)
    rng = np.random.default_rng(5)
    tokens = np.concatenate([rng.integers(0, len(vocab), 200), [t for t, v in enumerate(vocab) if len(v) == 40][:56]])
    states = rng.integers(0, nxt.shape[0], tokens.size)
    got = library().rwkv_mi355x_selftest_dfa_advance(states, tokens, vocab, nxt)
    want = [walk(nxt, int(q), vocab[t]) for q, t in zip(states, tokens)]
    assert any(w != DEAD and len(vocab[t]) == 40 for w, t in zip(want, tokens))
    assert list(got) == [int(q) if w == DEAD else w for q, w in zip(states, want)]  # a dead walk leaves the state


# ------------------------------------------------------------------ the whole path, tiny v5.2 and v6
def synthetic_vocab(V):
    """Every token has a byte: its id's low byte, except a few multi-byte ones."""
    vocab = [bytes([t % 256]) for t in range(V)]
    for t, v in ((1, b'ye'), (2, b'or'), (4, b'north'), (5, b'4'), (6, b'\xc3\xa9t')):
        vocab[t] = v
    return vocab


@pytest.fixture(scope='module', params=[V52, V6])
def model(request):
    m = RWKVModel(library(), os.path.join(GOLD, request.param))
    m.set_vocab_bytes(synthetic_vocab(m.n_vocab))
    yield m
    m.free()


def two_automata():
    return join(from_choices([b'yes', b'no', b'north']), from_choices([b'42', b'7', 'été'.encode()]))


PROMPTS = [PROMPT[r:] + PROMPT[:r] for r in range(3)]
KW = dict(temperature=1.0, top_p=1.0, seeds=[31, 32, 33])


def run(model, call, n, dfa, **extra):
    if call == 'batch':
        return model.generate_batch(PROMPTS, n, dfa=dfa, **KW, **extra)
    return model.generate_queue(PROMPTS, n, lanes=2, dfa=dfa, **KW, **extra)


@pytest.mark.parametrize('call', ['batch', 'queue'])
def test_rows_follow_their_automata_and_end_when_complete(model, call):
    vocab = synthetic_vocab(model.n_vocab)
    dfa, (a, b) = two_automata()
    dfa.start = starts = [a, b, a]
    n = 8
    tokens = run(model, call, n, dfa)
    for r in range(3):
        spelled = b''.join(vocab[t] for t in tokens[r])
        assert len(tokens[r]) >= 1 and walk(dfa.next, starts[r], spelled) == dfa.state[r] != DEAD, (r, spelled)
        # no stop token: a row ends where nothing can follow, a leaf of its trie, before its cap
        assert dfa.ended[r] == 2 and dfa.accepting[dfa.state[r]] and len(tokens[r]) < n, (r, spelled)
        assert np.all(dfa.next[dfa.state[r]] == DEAD)
    # the slot of an ended row holds what its last token left: the same call capped at the row's length
    # (the row never meets the empty mask) leaves a slot that draws the same next token
    r = 0
    model.batch_load(r)
    ended_next = model.sample(temperature=0.0)
    again = Dfa(dfa.next, dfa.accepting, starts)
    capped = run(model, call, len(tokens[r]), again)
    assert capped[r] == tokens[r] and again.ended[r] == 0 and again.state[r] == dfa.state[r]
    model.batch_load(r)
    assert model.sample(temperature=0.0) == ended_next


@pytest.mark.parametrize('call', ['batch', 'queue'])
def test_stop_token_only_where_accepting(model, call):
    vocab = synthetic_vocab(model.n_vocab)
    dfa, (a, b) = two_automata()
    dfa.start = starts = [a, b, a]
    stop = 0
    tokens = run(model, call, 8, dfa, stop_tokens=[stop], logit_bias={stop: 60.0})  # drawn as soon as allowed
    for r in range(3):
        assert tokens[r][-1] == stop and stop not in tokens[r][:-1] and dfa.ended[r] == 1
        q = walk(dfa.next, starts[r], b''.join(vocab[t] for t in tokens[r][:-1]))
        assert q == dfa.state[r] and dfa.accepting[q]
        # and it was not allowed one token earlier
        assert len(tokens[r]) >= 2 and not dfa.accepting[walk(dfa.next, starts[r], b''.join(vocab[t] for t in tokens[r][:-2]))]


def test_accept_everything_is_the_unconstrained_call_bit_for_bit(model):
    every = lambda: Dfa(np.zeros((1, 256), np.uint16), [1])  # noqa: E731
    kw = dict(temperature=0.9, top_p=0.8, seed=11, logprobs=2, top_k=50)

    def single(dfa):
        model.eval_sequence(PROMPT, None, use_numpy=True)
        return model.sample(dfa=dfa, **kw), model.generate(6, dfa=dfa, **kw)

    (t0, lp0), (g0, glp0) = single(None)
    (t1, lp1), (g1, glp1) = single(every())
    assert t0 == t1 and g0 == g1 and lp0.token_logprob == lp1.token_logprob
    for x, y in zip(glp0, glp1):
        assert x.tobytes() == y.tobytes()
    bkw = dict(logprobs=2, stop_tokens=[PROMPT[0]], min_p=0.01, **KW)
    for plain, con in ((model.generate_batch(PROMPTS, 6, **bkw), model.generate_batch(PROMPTS, 6, dfa=every(), **bkw)),
                       (model.generate_queue(PROMPTS, [6, 4, 5], lanes=2, **bkw),
                        model.generate_queue(PROMPTS, [6, 4, 5], lanes=2, dfa=every(), **bkw))):
        assert plain[0] == con[0]
        for x, y in zip(plain[1], con[1]):
            assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))


def test_one_constrained_draw_is_the_sampler_on_host_masked_logits(model):
    vocab = synthetic_vocab(model.n_vocab)
    dfa = from_choices([b'yes', b'no', b'north', b'maybe'])
    logits, _ = model.eval_sequence(PROMPT, None, use_numpy=True)
    kw = dict(temperature=1.1, top_p=0.9)
    for seed in range(6):
        token = model.sample(seed=seed, top_k=3, dfa=dfa, **kw)
        masked = np.where(allowed_mask(dfa.next, dfa.accepting, 0, vocab), logits, np.float32(-np.inf))
        u = np.array([sampling.uniform(seed, 0)], np.float32)
        want = library().rwkv_mi355x_selftest_sample(masked, u, filters=dict(top_k=3), **kw)[0][0]
        assert token == want and vocab[token] in (b'y', b'ye', b'n', b'm')
        assert dfa.state[0] == walk(dfa.next, 0, vocab[token]) and dfa.ended[0] == 0


def test_bad_constraints_fail_before_anything_changes(model):
    L, ptr = library().library, model._ctx.ptr
    model.generate_batch(PROMPTS[:2], 2, seeds=[1, 2])  # slots 0 and 1 hold something
    model.eval_sequence(PROMPT, None, use_numpy=True)
    before = model.sample(temperature=0.0)
    good = from_choices([b'yes'])
    over = library().rwkv_mi355x_constraint_max_entries() // 256 + 1
    big = table('classes')[0]
    bad_entry = good.next.copy()
    bad_entry[1, 7] = good.next.shape[0]
    bads = [Dfa(np.zeros((0, 256), np.uint16), []), Dfa(bad_entry, good.accepting), Dfa(good.next, good.accepting, 4),
            Dfa(np.concatenate([big] * (over // 40 + 1))[:over], np.zeros(over, np.uint8))]
    params = make_batch_sampling(2, seeds=[1, 2])
    bare = RWKVModel(library(), os.path.join(GOLD, 'tiny-rwkv-6v0-3m-Q5_0.bin'))  # no vocabulary bytes
    calls = [(bare, lambda m, d: m.sample(dfa=d), good)]
    for bad in bads:
        calls += [(model, lambda m, d: m.sample(dfa=d), bad), (model, lambda m, d: m.generate(3, dfa=d), bad),
                  (model, lambda m, d: library().rwkv_mi355x_generate_batch(m._ctx, 2, 3, params, dfa=d), bad),
                  (model, lambda m, d: library().rwkv_mi355x_generate_queue(m._ctx, [3, 3], 2, seeds=[1, 2], dfa=d), bad)]
    bare.eval_sequence(PROMPT, None, use_numpy=True)
    for m, call, d in calls:
        with pytest.raises(ValueError):
            call(m, d)
        assert L.rwkv_get_last_error(m._ctx.ptr) == RWKV_ERROR_ARGS
    bare.free()
    # NULL arrays, and offsets that decrease
    from rwkv_cpp.rwkv_cpp_shared_library import make_constraint, make_sampling
    import ctypes
    for field in ('next', 'accepting', 'state'):
        c = make_constraint(1, good)
        setattr(c, field, None)
        token = ctypes.c_uint32(0)
        assert not L.rwkv_mi355x_sample_constrained(ptr, ctypes.byref(make_sampling(1.0, 0.8, None, 0, 0)), ctypes.byref(token), None, None,
                                                    ctypes.byref(c))
        assert L.rwkv_get_last_error(ptr) == RWKV_ERROR_ARGS
    offsets = np.arange(model.n_vocab + 1, dtype=np.uint32)
    offsets[5] = 9
    data = np.zeros(model.n_vocab + 16, np.uint8)
    assert not L.rwkv_mi355x_vocab_bytes(ptr, offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                         data.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    assert L.rwkv_get_last_error(ptr) == RWKV_ERROR_ARGS
    assert model.sample(temperature=0.0) == before
