"""The sixteen generation entry points of include/rwkv_mi355x.h -- rwkv_mi355x_{sample, generate,
generate_batch, generate_queue} and their _logprobs, _filtered and _constrained variants -- through
ctypes alone.

a. A NULL part is the call without it: with the same state and slots, every entry point of a family
   that is given the same parts returns the same tokens, lengths, lanes, starts, steps and
   log-probabilities and leaves the same state, logits and slots, bit for bit.
b. The argument checks run in one order in all of them: of two bad arguments the earlier check's message
   is the one printed, the flag is RWKV_ERROR_ARGS, and state, logits and slots are untouched.  The
   message fragments are those of the library's CTX_CHECK strings.

Shapes: n = 4 tokens, B = 2 rows, Q = 3 sequences over 2 lanes with max_tokens 4, 2, 3."""
import ctypes
import os

import numpy as np
import pytest

from rwkv_cpp.rwkv_cpp_shared_library import (RWKVConstraint, make_batch_sampling, make_filters, make_logprobs,
                                              make_sampling)
from test_gpu_generate_batch import GOLD, V6, bits
from test_gpu_generate_queue import QCtx

pytestmark = pytest.mark.gpu

P_U = ctypes.POINTER(ctypes.c_uint32)
RWKV_ERROR_ARGS = 1 << 8
N, B, Q, LANES, CAPS, SLOTS = 4, 2, 3, 2, [4, 2, 3], 3
SUFFIXES = ('', '_logprobs', '_filtered', '_constrained')
FAMILIES = ('sample', 'generate', 'generate_batch', 'generate_queue')


@pytest.fixture(scope='module')
def ctx():
    c = QCtx(os.path.join(GOLD, V6))
    c.L.rwkv_set_print_errors(c.ptr, True)
    yield c
    c.free()


def call(c, family, variant, lp=None, f=None, cons=None, **o):
    """The family's entry point SUFFIXES[variant] with its first `variant` optional parts (lp, f, cons;
    None: NULL).  o: what a bad call changes -- temperature (row 0), top_p, n, rows, caps, keep_counts,
    token_null, lengths_null.  Returns (ok, the host outputs)."""
    rows = o.get('rows', {'generate_batch': B, 'generate_queue': Q}.get(family, 1))
    n = o.get('n', N)
    tok, lens = np.zeros((rows, N), np.uint32), np.zeros(rows, np.uint32)
    lane, start, steps = np.zeros(rows, np.uint32), np.zeros(rows, np.uint32), ctypes.c_uint32(0)
    t = None if o.get('token_null') else tok.ctypes.data_as(P_U)
    if family in ('sample', 'generate'):
        p = make_sampling(o.get('temperature', 0.8), o.get('top_p', 0.5), None, 7, 0)
        args = (ctypes.byref(p), t) if family == 'sample' else (ctypes.byref(p), n, t, None)
    else:
        p = make_batch_sampling(rows, [o.get('temperature', 0.8)] + [0.9] * (rows - 1), o.get('top_p', 0.5),
                                seeds=list(range(1, rows + 1)), keep_counts=o.get('keep_counts', False))
        le = None if o.get('lengths_null') else lens.ctypes.data_as(P_U)
        if family == 'generate_batch':
            args = (rows, ctypes.byref(p), n, t, le, ctypes.byref(steps))
        else:
            caps = np.array(o.get('caps', CAPS), np.uint32)
            args = (rows, LANES, ctypes.byref(p), caps.ctypes.data_as(P_U), n, t, le, lane.ctypes.data_as(P_U),
                    start.ctypes.data_as(P_U), ctypes.byref(steps))
    parts = tuple(x and ctypes.byref(x) for x in (lp, f, cons))[:variant]
    ok = getattr(c.L, f'rwkv_mi355x_{family}{SUFFIXES[variant]}')(c.ptr, *args, *parts)
    return ok, (tok, lens, lane, start, steps.value)


def device(c):
    """The context's state and logits, then those of every slot (reading a slot loads it)."""
    return [(c.state(), c.logits())] + [c.slot(s) for s in range(SLOTS)]


def same(a, b):
    return all(np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1])) for x, y in zip(a, b))


# ------------------------------------------------------------------ a. a NULL part is the call without it
@pytest.mark.parametrize('k', [None, 3])
@pytest.mark.parametrize('family', FAMILIES)
def test_null_parts_forward(ctx, family, k):
    c = ctx
    results = []
    for variant in range(0 if k is None else 1, 4):
        c.fill(SLOTS)
        c.start(0)
        lp, arrays = make_logprobs(Q, N, k) if k is not None else (None, ())
        ok, host = call(c, family, variant, lp)
        assert ok, (family, variant)
        results.append((host, [a.tobytes() for a in arrays], device(c)))
    first = results[0]
    for variant, (host, lps, dev) in enumerate(results[1:], 1):
        assert all(np.array_equal(x, y) for x, y in zip(host, first[0])), (family, variant)
        assert lps == first[1], (family, variant)
        assert same(dev, first[2]), (family, variant)


# ------------------------------------------------------------------ b. which check wins
def bad_lp():
    lp, _ = make_logprobs(Q, N, 3)
    lp.top_k = 21
    return lp


NO_STATES = RWKVConstraint(0, None, None, None, None)

# (family, the parts and changes of a call with two bad arguments, the first check's message)
PRECEDENCE = [(family, dict(lp=bad_lp, temperature=-1.0), 'top_k') for family in FAMILIES] + [
    ('sample', dict(temperature=-1.0, token_null=True), 'Temperature'),
    ('sample', dict(f=dict(min_p=2.0), token_null=True), 'min_p'),
    ('generate', dict(n=0, cons=NO_STATES), 'Token count'),
    ('generate', dict(f=dict(typical_p=float('nan')), n=0), 'typical_p'),
    ('generate_batch', dict(rows=SLOTS + 1, lengths_null=True), 'slots reserved'),
    ('generate_batch', dict(top_p=1.5, f=dict(min_p=-1.0)), 'top_p'),
    ('generate_queue', dict(caps=[4, 0, 3], temperature=-1.0), 'max_tokens'),
    ('generate_queue', dict(f=dict(min_p=2.0), keep_counts=True), 'min_p'),
    ('generate_queue', dict(keep_counts=True, cons=NO_STATES), 'keep_counts'),
]


@pytest.mark.parametrize('family,bad,message', PRECEDENCE, ids=[f'{p[0]}-{p[2]}-{i}' for i, p in enumerate(PRECEDENCE)])
def test_the_first_check_wins(ctx, capfd, family, bad, message):
    c = ctx
    bad = dict(bad)
    rows = bad.get('rows', {'generate_batch': B, 'generate_queue': Q}.get(family, 1))
    lp = bad.pop('lp', None)
    lp = lp and lp()
    f = bad.pop('f', None)
    f = f and make_filters(rows, **f)
    cons = bad.pop('cons', None)
    first = 3 if cons is not None else 2 if f is not None else 1 if lp is not None else 0
    c.fill(SLOTS)
    slots = [c.slot(s) for s in range(SLOTS)]
    c.start(0)
    before = [(c.state(), c.logits())] + slots
    for variant in range(first, 4):
        capfd.readouterr()
        ok, _ = call(c, family, variant, lp, f, cons, **bad)
        err = capfd.readouterr().err
        assert not ok and c.error() == RWKV_ERROR_ARGS, (variant, err)
        assert message in err.splitlines()[0], (variant, err)
    assert same(before, device(c))
