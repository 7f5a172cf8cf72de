"""rwkv_mi355x_generate_batch (include/rwkv_mi355x.h): a batch of sequences generated on the device --
per-row sampling, penalties, exact stops -- gives every row the tokens, the state and the logits of
that row generated alone, bit for bit: by rwkv_mi355x_generate where that can express the row, by
the stepwise host loop (rwkv_mi355x_eval_device with logits_out, sampling.penalize, the one-row sampler
kernel) where it cannot."""
import ctypes
import os

import numpy as np
import pytest

from rwkv_lib import library
from rwkv_cpp import sampling
from rwkv_cpp.rwkv_cpp_shared_library import make_batch_sampling, make_sampling

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
P_F = ctypes.POINTER(ctypes.c_float)
P_U = ctypes.POINTER(ctypes.c_uint32)
RWKV_ERROR_ARGS, RWKV_ERROR_CTX, RWKV_ERROR_UNSUPPORTED = 1 << 8, 6 << 8, 9
FIXTURES = ['tiny-rwkv-4v0-660K-FP16.bin', 'tiny-rwkv-5v2-730K-FP16.bin', 'tiny-rwkv-6v0-3m-Q5_1.bin',
            'tiny-rwkv-7v0-834K-FP16.bin']
V6 = 'tiny-rwkv-6v0-3m-Q5_1.bin'
PROMPT = list(b'This is a port of [B')  # 20 tokens; row r starts from its rotation by r
N = 12
FILL = 0xFFFFFFFF
# five rows: greedy, top_p = 1, temperature 0.7, and two more streams
ROWS5 = dict(temperature=[0.0, 1.0, 0.7, 0.8, 1.0], top_p=[0.8, 1.0, 0.8, 0.5, 0.8], seeds=[11, 12, 13, 14, 15],
             offsets=[0, 3, 0, 7, 1])
BIAS = {5: 0.75, 32: -1.5, 101: 0.5}


@pytest.fixture(scope='module')
def world_model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp('generate_batch') / 'world-v6.bin')
    assert library().library.rwkv_mi355x_write_synthetic_model(p.encode(), 6, 65536, 256, 3, 0, b'Q5_1', 11)
    return p


def bits(a):
    return np.asarray(a).view(np.uint32)


def row_params(kw, r):
    """Row r's scalars of a per-row parameter set (scalars are shared)."""
    def pick(v):
        return v[r] if hasattr(v, '__len__') else v
    return dict(temperature=pick(kw.get('temperature', 1.0)), top_p=pick(kw.get('top_p', 0.8)),
                seed=pick(kw['seeds']), offset=pick(kw.get('offsets', 0)), presence=pick(kw.get('presence') or 0.0),
                frequency=pick(kw.get('frequency') or 0.0), logit_bias=kw.get('logit_bias'))


class Ctx:
    def __init__(self, path, knobs=None, timing=False):
        self.L = library().library
        self.ptr = self.L.rwkv_init_from_file(path.encode(), 1, 99)
        assert self.ptr
        for k, v in (knobs or {}).items():
            assert self.L.rwkv_mi355x_debug_set(self.ptr, k.encode(), v)
        if timing:
            self.L.rwkv_mi355x_set_kernel_timing(self.ptr, True)
        self.V = self.L.rwkv_get_n_vocab(self.ptr)

    def free(self):
        self.L.rwkv_free(self.ptr)

    def prompt(self, r):
        k = r % len(PROMPT)
        return [(t + r // len(PROMPT)) % self.V for t in PROMPT[k:] + PROMPT[:k]]

    def step(self, tokens, logits_out=None):
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        out = logits_out.ctypes.data_as(P_F) if logits_out is not None else None
        assert self.L.rwkv_mi355x_eval_device(self.ptr, arr, len(tokens), True, out, True)

    def start(self, r, logits_out=None):
        """Fresh state, then row r's prompt with logits."""
        assert self.L.rwkv_mi355x_state_upload(self.ptr, None)
        self.step(self.prompt(r), logits_out)

    def state(self):
        st = np.zeros(self.L.rwkv_get_state_len(self.ptr), np.float32)
        assert self.L.rwkv_mi355x_state_download(self.ptr, st.ctypes.data_as(P_F))
        return st

    def logits(self):
        lg = np.zeros(self.V, np.float32)
        assert self.L.rwkv_mi355x_debug_buffer(self.ptr, b'logits', lg.ctypes.data_as(ctypes.c_void_p), lg.nbytes) == lg.nbytes
        return lg

    def error(self):
        return self.L.rwkv_get_last_error(self.ptr)

    # ---- slots
    def fill(self, B):
        if self.L.rwkv_mi355x_batch_slots(self.ptr) != B:
            assert self.L.rwkv_mi355x_batch_reserve(self.ptr, B)
        for r in range(B):
            self.start(r)
            assert self.L.rwkv_mi355x_batch_store(self.ptr, r)

    def slot(self, r):
        """(state, logits) of slot r, through batch_load into the context."""
        assert self.L.rwkv_mi355x_batch_load(self.ptr, r)
        return self.state(), self.logits()

    def run_raw(self, B, n, p, tokens_null=False, lengths_null=False):
        toks = np.zeros((B if B else 1, max(n, 1) if n <= 65536 else 1), np.uint32)
        lens = np.zeros(max(B, 1), np.uint32)
        steps = ctypes.c_uint32(FILL)
        ok = self.L.rwkv_mi355x_generate_batch(self.ptr, B, ctypes.byref(p) if p is not None else None, n,
                                               None if tokens_null else toks.ctypes.data_as(P_U),
                                               None if lengths_null else lens.ctypes.data_as(P_U), ctypes.byref(steps))
        return ok, toks, lens, steps.value

    def run(self, B, n=N, **kw):
        """One call on freshly filled slots unless keep_counts.  Returns (tokens [B][n], lengths, steps)."""
        if not kw.get('keep_counts'):
            self.fill(B)
        p = make_batch_sampling(B, kw.get('temperature', 1.0), kw.get('top_p', 0.8), kw.get('presence'), kw.get('frequency'),
                                kw.get('logit_bias'), kw['seeds'], kw.get('offsets', 0), kw.get('stop_tokens', ()),
                                kw.get('keep_counts', False), kw.get('check_every', 0))
        ok, toks, lens, steps = self.run_raw(B, n, p)
        assert ok
        return toks, lens, steps

    # ---- the same row alone
    def single(self, r, n, kw):
        """Row r through rwkv_mi355x_generate (no penalties): tokens, state, logits."""
        q = row_params(kw, r)
        assert q['presence'] == 0.0 and q['frequency'] == 0.0
        self.start(r)
        p = make_sampling(q['temperature'], q['top_p'], q['logit_bias'], q['seed'], q['offset'])
        toks = (ctypes.c_uint32 * n)()
        lg = np.zeros(self.V, np.float32)
        assert self.L.rwkv_mi355x_generate(self.ptr, ctypes.byref(p), n, toks, lg.ctypes.data_as(P_F))
        return list(toks), self.state(), lg

    def stepwise(self, r, n, kw):
        """Row r through the host loop: eval_device with logits_out, sampling.penalize over the host's
        running counts, the one-row sampler kernel with the draw made on the host."""
        q = row_params(kw, r)
        lg = np.zeros(self.V, np.float32)
        self.start(r, lg)
        counts = np.zeros(self.V, np.uint32)
        toks = []
        for i in range(n):
            row = sampling.penalize(lg, counts, q['presence'], q['frequency'])
            tok, _, _ = library().rwkv_mi355x_selftest_sample(row, sampling.uniform(q['seed'], q['offset'] + i),
                                                              temperature=q['temperature'], top_p=q['top_p'],
                                                              logit_bias=q['logit_bias'])
            toks.append(int(tok[0]))
            counts[toks[-1]] += 1
            self.step([toks[-1]], lg)
        return toks, self.state(), lg

    def after(self, r, tokens):
        """State and logits of a context that evaluated row r's prompt and then `tokens`, one at a time."""
        self.start(r)
        for t in tokens:
            self.step([t])
        return self.state(), self.logits()


def assert_row(c, r, got_tokens, want):
    toks, st, lg = want
    assert list(got_tokens) == toks, r
    gst, glg = c.slot(r)
    assert np.array_equal(bits(gst), bits(st)), r
    assert np.array_equal(bits(glg), bits(lg)), r


# ------------------------------------------------------------------ 1. rows = the single-context generator
@pytest.mark.parametrize('name', FIXTURES)
def test_rows_equal_generate(name):
    c = Ctx(os.path.join(GOLD, name))
    try:
        kw = dict(ROWS5, logit_bias=BIAS)
        toks, lens, steps = c.run(5, **kw)
        assert list(lens) == [N] * 5 and steps == N
        for r in range(5):
            assert_row(c, r, toks[r], c.single(r, N, kw))
    finally:
        c.free()


# ------------------------------------------------------------------ 2. around the batched step's thresholds
@pytest.mark.parametrize('B', [1, 17, 33])
@pytest.mark.parametrize('which', ['v6', 'world'])
def test_batch_thresholds(which, B, world_model):
    c = Ctx(world_model if which == 'world' else os.path.join(GOLD, V6))
    try:
        kw = dict(temperature=[(0.0, 1.0, 0.7)[r % 3] for r in range(B)], top_p=[(0.8, 1.0, 0.5)[r % 3] for r in range(B)],
                  seeds=[100 + r for r in range(B)], offsets=[r % 5 for r in range(B)], logit_bias=BIAS)
        toks, lens, _ = c.run(B, **kw)
        assert list(lens) == [N] * B
        for r in sorted({0, B // 2, B - 1}):
            assert_row(c, r, toks[r], c.single(r, N, kw))
    finally:
        c.free()


# ------------------------------------------------------------------ 3. penalties
PENALISED = dict(temperature=[0.0, 0.0, 1.0, 0.8, 0.7], top_p=[0.8, 0.8, 0.8, 0.5, 1.0], seeds=[21, 22, 23, 24, 25],
                 offsets=[0, 0, 2, 0, 5], presence=[2.0, 2.0, 0.2, 0.2, 0.2], frequency=[1.0, 1.0, 0.2, 0.2, 0.2],
                 logit_bias=BIAS)


@pytest.mark.parametrize('name', FIXTURES)
def test_penalties_equal_the_stepwise_loop(name):
    """Under greedy decoding every fixture repeats a token within 12 steps of every rotation of the
    prompt (the CPU oracle, tests/oracle_ctypes.py: first repeats at steps 1 to 7), so a presence
    penalty of 2 and a frequency penalty of 1 change the greedy rows."""
    c = Ctx(os.path.join(GOLD, name))
    try:
        toks, lens, _ = c.run(5, **PENALISED)
        assert list(lens) == [N] * 5
        for r in range(5):
            assert_row(c, r, toks[r], c.stepwise(r, N, PENALISED))
        plain = dict(PENALISED, presence=None, frequency=None)
        free, _, _ = c.run(5, **plain)
        assert any(list(free[r]) != list(toks[r]) for r in (0, 1)), 'no greedy row changed: the penalties were not exercised'
        assert any(len(set(free[r])) < N for r in (0, 1))
    finally:
        c.free()


# ------------------------------------------------------------------ 4. stops, row by row
SAMPLED5 = dict(temperature=[1.0, 0.9, 0.7, 0.8, 1.0], top_p=[0.9, 1.0, 0.8, 0.9, 0.8], seeds=[31, 32, 33, 34, 35],
                offsets=[0, 3, 0, 7, 1])


def test_stops_are_exact_and_rows_independent(world_model):
    c = Ctx(world_model)
    try:
        R, _, _ = c.run(5, **SAMPLED5)
        R = [[int(t) for t in row] for row in R]
        whole = [(R[r],) + c.slot(r) for r in range(5)]
        stops = [R[3][0], R[1][3]]
        want_len = [next((i + 1 for i, t in enumerate(R[r]) if t in stops), N) for r in range(5)]
        assert 1 in want_len and N in want_len and any(1 < x < N for x in want_len), want_len
        assert any(x == N and not set(R[r]) & set(stops) for r, x in enumerate(want_len)), 'no row runs to the end'
        toks, lens, steps = c.run(5, stop_tokens=stops, **SAMPLED5)
        assert list(lens) == want_len and steps == N
        for r in range(5):
            n = want_len[r]
            assert list(toks[r]) == R[r][:n] + [FILL] * (N - n), r
            if R[r][n - 1] in stops:
                st, lg = c.after(r, R[r][:n - 1])
                assert_row(c, r, toks[r][:n], (R[r][:n], st, lg))
            else:
                assert_row(c, r, toks[r], whole[r])
    finally:
        c.free()


# ------------------------------------------------------------------ 5. check_every
def test_check_every_does_not_change_the_results(world_model):
    c = Ctx(world_model)
    try:
        R, _, _ = c.run(5, **SAMPLED5)
        stops = [int(R[3][0]), int(R[1][3])]
        runs = []
        for k in (0, 1, 4):
            toks, lens, _ = c.run(5, stop_tokens=stops, check_every=k, **SAMPLED5)
            runs.append((toks.copy(), lens.copy(), [c.slot(r) for r in range(5)]))
        for toks, lens, slots in runs[1:]:
            assert np.array_equal(toks, runs[0][0]) and np.array_equal(lens, runs[0][1])
            for (st, lg), (st0, lg0) in zip(slots, runs[0][2]):
                assert np.array_equal(bits(st), bits(st0)) and np.array_equal(bits(lg), bits(lg0))
        # every row stops at its first token: the host sees it after one step, or never looks
        first = sorted({int(R[r][0]) for r in range(5)})
        out = {}
        for k in (1, 0):
            toks, lens, steps = c.run(5, stop_tokens=first, check_every=k, **SAMPLED5)
            assert list(lens) == [1] * 5 and steps == (1 if k else N)
            assert [int(t) for t in toks[:, 0]] == [int(R[r][0]) for r in range(5)] and (toks[:, 1:] == FILL).all()
            out[k] = [c.slot(r) for r in range(5)]
        for r in range(5):
            c.start(r)  # the slot of a row that stopped at once is its prompt's state and logits
            for st, lg in (out[0][r], out[1][r]):
                assert np.array_equal(bits(st), bits(c.state())) and np.array_equal(bits(lg), bits(c.logits()))
    finally:
        c.free()


# ------------------------------------------------------------------ 6. continuation
def test_two_calls_continue_one(world_model):
    c = Ctx(world_model)
    try:
        kw = dict(SAMPLED5, presence=[0.2, 0.5, 0.2, 2.0, 0.2], frequency=[0.2, 0.1, 0.2, 1.0, 0.2], logit_bias=BIAS)
        W0, _, _ = c.run(5, **kw)
        stops = [int(W0[2][2])]  # row 2 finishes within the first call
        W, wl, _ = c.run(5, stop_tokens=stops, **kw)
        whole = [c.slot(r) for r in range(5)]
        assert wl[2] <= 3 and N in list(wl)
        for n1 in (6, 5):  # 5 + 7: both calls take an odd number of steps
            a, al, _ = c.run(5, n=n1, stop_tokens=stops, **kw)
            b, bl, _ = c.run(5, n=N - n1, stop_tokens=stops, keep_counts=True,
                             **dict(kw, offsets=[o + n1 for o in kw['offsets']]))
            for r in range(5):
                got = list(a[r][:al[r]]) + list(b[r][:bl[r]])
                assert got == list(W[r][:wl[r]]), (n1, r)
                st, lg = c.slot(r)
                assert np.array_equal(bits(st), bits(whole[r][0])) and np.array_equal(bits(lg), bits(whole[r][1])), (n1, r)
            # the row that finished in the first call stays finished
            assert al[2] == wl[2] and bl[2] == 0 and (b[2] == FILL).all()
    finally:
        c.free()


# ------------------------------------------------------------------ 7. store / load
def test_store_load_round_trip():
    c = Ctx(os.path.join(GOLD, V6))
    clone = Ctx.__new__(Ctx)
    clone.L, clone.V = c.L, c.V
    clone.ptr = c.L.rwkv_clone_context(c.ptr, 1)
    assert clone.ptr
    try:
        assert c.L.rwkv_mi355x_batch_reserve(c.ptr, 3) and c.L.rwkv_mi355x_batch_slots(c.ptr) == 3
        c.start(4)
        st, lg = c.state(), c.logits()
        assert c.L.rwkv_mi355x_batch_store(c.ptr, 2)
        c.start(1)  # the context moves on; an odd number of steps flips its state parity
        c.step([7])
        got = c.slot(2)
        assert np.array_equal(bits(got[0]), bits(st)) and np.array_equal(bits(got[1]), bits(lg))
        # generate continues from the loaded slot as the original does (here: a clone given the same prompt)
        want = clone.single(4, 8, dict(temperature=0.8, top_p=0.5, seeds=7))
        p = make_sampling(0.8, 0.5, None, 7, 0)
        toks = (ctypes.c_uint32 * 8)()
        assert c.L.rwkv_mi355x_generate(c.ptr, ctypes.byref(p), 8, toks, None)
        assert list(toks) == want[0] and np.array_equal(bits(c.state()), bits(want[1]))
        # reserve empties every slot
        assert c.L.rwkv_mi355x_batch_reserve(c.ptr, 3)
        assert not c.L.rwkv_mi355x_batch_load(c.ptr, 2) and c.error() == RWKV_ERROR_ARGS
        assert c.L.rwkv_mi355x_batch_reserve(c.ptr, 0) and c.L.rwkv_mi355x_batch_slots(c.ptr) == 0
    finally:
        clone.free()
        c.free()


# ------------------------------------------------------------------ 8. errors
def test_argument_errors_leave_the_slots_alone():
    c = Ctx(os.path.join(GOLD, V6))
    try:
        kw = dict(temperature=[0.0, 0.8], top_p=0.5, seeds=[1, 2])
        want, _, _ = c.run(2, **kw)
        assert c.L.rwkv_mi355x_batch_reserve(c.ptr, 3)
        for r in range(2):
            c.start(r)
            assert c.L.rwkv_mi355x_batch_store(c.ptr, r)
        before = [c.slot(r) for r in range(2)]

        def params(B=2, **over):
            return make_batch_sampling(B, **dict(dict(temperature=[0.0, 0.8, 0.5][:B], top_p=0.5, seeds=[1, 2, 3][:B]), **over))

        nan = float('nan')
        cases = [(0, 4, params()), (4, 4, params(4, temperature=0.5, seeds=None)), (3, 4, params(3)),  # slot 2 never stored
                 (2, 0, params()), (2, 65537, params()), (2, 4, None),
                 (2, 4, params(temperature=[0.5, -1.0])), (2, 4, params(temperature=[nan, 0.5])),
                 (2, 4, params(top_p=[0.5, 1.5])), (2, 4, params(presence=[0.0, nan])), (2, 4, params(frequency=[nan, 0.0])),
                 (2, 4, params(logit_bias={i: 0.0 for i in range(257)})), (2, 4, params(logit_bias={c.V: 1.0})),
                 (2, 4, params(stop_tokens=list(range(17)))), (2, 4, params(stop_tokens=[c.V]))]
        for B, n, p in cases:
            ok, _, _, _ = c.run_raw(B, n, p)
            assert not ok and c.error() == RWKV_ERROR_ARGS, (B, n)
        for null in ('temperature', 'top_p', 'seed', 'offset'):
            p = params()
            setattr(p, null, None)
            ok, _, _, _ = c.run_raw(2, 4, p)
            assert not ok and c.error() == RWKV_ERROR_ARGS, null
        for kwn in (dict(tokens_null=True), dict(lengths_null=True)):
            ok, _, _, _ = c.run_raw(2, 4, params(), **kwn)
            assert not ok and c.error() == RWKV_ERROR_ARGS
        assert not c.L.rwkv_mi355x_batch_reserve(c.ptr, 257) and c.error() == RWKV_ERROR_ARGS
        assert not c.L.rwkv_mi355x_batch_store(c.ptr, 3) and c.error() == RWKV_ERROR_ARGS
        assert not c.L.rwkv_mi355x_batch_load(c.ptr, 2) and c.error() == RWKV_ERROR_ARGS
        # a store needs logits that follow the state
        assert c.L.rwkv_mi355x_state_upload(c.ptr, None)
        assert not c.L.rwkv_mi355x_batch_store(c.ptr, 2) and c.error() == RWKV_ERROR_ARGS
        # nothing moved: the slots hold the same bits and generate the same tokens
        for r in range(2):
            st, lg = c.slot(r)
            assert np.array_equal(bits(st), bits(before[r][0])) and np.array_equal(bits(lg), bits(before[r][1]))
        ok, toks, lens, _ = c.run_raw(2, N, params())
        assert ok and np.array_equal(toks, want) and list(lens[:2]) == [N, N]
    finally:
        c.free()


def test_pipeline_context_is_refused():
    L = library().library
    devs = (ctypes.c_int * 2)(0, 0)
    pipe = L.rwkv_mi355x_init_pipeline(os.path.join(GOLD, V6).encode(), 1, 2, devs)
    assert pipe
    try:
        want = RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED
        assert not L.rwkv_mi355x_batch_reserve(pipe, 2) and L.rwkv_get_last_error(pipe) == want
        assert not L.rwkv_mi355x_batch_store(pipe, 0) and L.rwkv_get_last_error(pipe) == want
        assert not L.rwkv_mi355x_batch_load(pipe, 0) and L.rwkv_get_last_error(pipe) == want
        p = make_batch_sampling(2, 0.0, 0.5)
        toks, lens = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 2)()
        assert not L.rwkv_mi355x_generate_batch(pipe, 2, ctypes.byref(p), 4, toks, lens, None)
        assert L.rwkv_get_last_error(pipe) == want
    finally:
        L.rwkv_free(pipe)


# ------------------------------------------------------------------ 9. the decode arms
@pytest.mark.parametrize('arm', ['no_graphs', 'timing'])
def test_decode_arms_give_the_same_bits(arm):
    path = os.path.join(GOLD, V6)
    kw = dict(PENALISED, stop_tokens=[101])
    base = Ctx(path)
    c = Ctx(path, {'graphs': 0} if arm == 'no_graphs' else None, timing=arm == 'timing')
    try:
        want = base.run(5, **kw)
        got = c.run(5, **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        for r in range(5):
            a, b = c.slot(r), base.slot(r)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    finally:
        if arm == 'timing':
            c.L.rwkv_mi355x_set_kernel_timing(c.ptr, False)
        c.free()
        base.free()
