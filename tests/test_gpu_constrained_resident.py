"""A resident constraint table (rwkv_mi355x_constraint_table) and the kernel that walks it from memory
(k_dfa_mask_mem, csrc/constrain.hip): the kernel through its self-test against
rwkv_cpp.constraint.allowed_mask at table sizes on both sides of the LDS limit and at the top of the
16-bit numbering, the four calls with a resident table over the limit against the same automaton passed
with the call, and the errors.  Integers and a select: everything is compared exactly."""
import functools

import numpy as np
import pytest

from rwkv_lib import library
from rwkv_cpp.constraint import DEAD, Dfa, ResidentDfa, allowed_mask, from_choices
from test_gpu_generate_batch import PROMPT, bits
from test_gpu_constrained import KW, LENGTHS, PROMPTS, RWKV_ERROR_ARGS, model, run, two_automata  # noqa: F401

pytestmark = pytest.mark.gpu

# one state; 256 distinct classes in a table that fits the LDS; the smallest table the LDS kernel
# refuses; the largest the numbering admits
SIZES = {'one': lambda: 1, 'classes': lambda: 40, 'over': lambda: library().rwkv_mi355x_constraint_max_entries() // 256 + 1,
         'top': lambda: 65534}


@functools.lru_cache(maxsize=None)
def table(n):
    """test_gpu_constrained.table at n states: seeded, ~40 % dead transitions, 256 distinct classes."""
    rng = np.random.default_rng(n)
    nxt = rng.integers(0, n, (n, 256)).astype(np.uint16)
    nxt[rng.random((n, 256)) < 0.4] = DEAD
    assert n == 1 or len({nxt[:, b].tobytes() for b in range(256)}) == 256
    return nxt, rng.integers(0, 2, n).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def mem_case(V, n, rows):
    """test_gpu_constrained.mask_case on table(n); the last row starts in the last state."""
    nxt, acc = table(n)
    acc = acc.copy()
    rng = np.random.default_rng(V + rows)
    starts = [int(s) for s in rng.integers(0, n, rows)]
    starts[-1] = n - 1
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
    stops = [3, V - 1]
    logits = rng.standard_normal((rows, V)).astype(np.float32)
    finished = [0] * rows
    if rows > 1:
        finished[1] = 1  # a skipped row inside the first group of four
    want = np.stack([allowed_mask(nxt, acc, q, vocab, stops) for q in starts])
    assert any(want[-1][t] and len(vocab[t]) == 40 for t in range(V))  # a tail walked to its end, from the last state
    return nxt, acc, starts, vocab, stops, logits, finished, want


@pytest.mark.parametrize('rows', [1, 3, 6])  # a lone row; a partial group; a full group of four and a tail of two
@pytest.mark.parametrize('kind', list(SIZES))
@pytest.mark.parametrize('V', [1025, 4099])
def test_memory_mask_kernel_equals_allowed_mask(V, kind, rows):
    nxt, acc, starts, vocab, stops, logits, finished, want = mem_case(V, SIZES[kind](), rows)
    masked, n_allowed, ended = library().rwkv_mi355x_selftest_dfa_mask_mem(logits, vocab, Dfa(nxt, acc, starts), stops, finished)
    for r in range(rows):
        if finished[r]:  # skipped: the fill is still there
            assert np.all(masked[r] == 7.0) and n_allowed[r] == 0 and ended[r] == 1
            continue
        expect = np.where(want[r], logits[r], np.float32(-np.inf))
        assert np.array_equal(bits(masked[r]), bits(expect)), r
        assert n_allowed[r] == want[r].sum()
        assert ended[r] == (2 if want[r].sum() == 0 else 0)


def padded(dfa):
    """dfa's table followed by unreachable random states, 256 distinct classes, over the LDS limit."""
    n0, n = dfa.next.shape[0], 400
    rng = np.random.default_rng(9)
    pad = rng.integers(0, n, (n - n0, 256)).astype(np.uint16)
    assert len({pad[:, b].tobytes() for b in range(256)}) == 256 and n * 256 > library().rwkv_mi355x_constraint_max_entries()
    return np.concatenate([dfa.next, pad]), np.concatenate([dfa.accepting, rng.integers(0, 2, n - n0).astype(np.uint8)])


@pytest.mark.parametrize('call', ['single', 'batch', 'queue'])
def test_resident_table_over_the_limit_gives_what_the_table_with_the_call_gives(model, call):
    given, (a, b) = two_automata()
    resident = model.set_constraint_table(*padded(given))
    assert resident.n_states == 400 == library().library.rwkv_mi355x_constraint_table_states(model._ctx.ptr)
    out = []
    for dfa in (given, resident):
        if call == 'single':
            model.eval_sequence(PROMPT, None, use_numpy=True)
            dfa.start = b
            first = model.sample(seed=5, temperature=1.0, top_p=1.0, dfa=dfa)
            got = [first, int(dfa.state[0]), int(dfa.ended[0])]
            dfa.start = a
            got.append(model.generate(8, seed=7, temperature=1.0, top_p=1.0, dfa=dfa))
        else:
            dfa.start = [a, b, a]
            got = [run(model, call, 8, dfa)]
        out.append(got + [dfa.state.tolist(), dfa.ended.tolist()])
    model.set_constraint_table(None)
    assert out[0] == out[1] and 2 in out[0][-1]  # some row ran until nothing was allowed


def test_bad_resident_tables_fail_before_anything_changes(model):
    L, ptr = library().library, model._ctx.ptr
    model.eval_sequence(PROMPT, None, use_numpy=True)
    before = model.sample(temperature=0.0)
    good = from_choices([b'yes', b'no'])
    n = good.next.shape[0]
    bad_entry = good.next.copy()
    bad_entry[1, 7] = n

    def refused(what):
        with pytest.raises(ValueError):
            what()
        assert L.rwkv_get_last_error(ptr) == RWKV_ERROR_ARGS
        assert model.sample(temperature=0.0) == before

    assert model.set_constraint_table(None) is None
    refused(lambda: model.sample(dfa=ResidentDfa(n)))  # no table set
    resident = model.set_constraint_table(good.next, good.accepting)
    refused(lambda: model.generate(3, dfa=ResidentDfa(n + 1)))  # another n_states
    refused(lambda: model.set_constraint_table(np.zeros((0xFFFF, 256), np.uint16), np.zeros(0xFFFF, np.uint8)))
    refused(lambda: model.set_constraint_table(bad_entry, good.accepting))
    # the table set before is still in place, and works
    assert L.rwkv_mi355x_constraint_table_states(ptr) == n
    assert model.sample(seed=2, dfa=resident) == model.sample(seed=2, dfa=good) and resident.state[0] == good.state[0]
    model.set_constraint_table(None)
    refused(lambda: model.sample(dfa=resident))  # after freeing
