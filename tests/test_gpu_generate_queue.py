"""rwkv_mi355x_generate_queue (include/rwkv_mi355x.h): a queue of sequences over a few decode rows.
Everything about a sequence -- tokens, length, its slot's state and logits -- equals, bit for bit, that
sequence generated alone (rwkv_mi355x_generate_batch with B = 1 and n = its max_tokens, or the
stepwise host loop for the penalties), and the lanes, start steps and step count are the list
schedule of the lengths drawn (sampling.queue_schedule)."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from rwkv_lib import library
from rwkv_cpp import sampling
from rwkv_cpp.rwkv_cpp_shared_library import make_batch_sampling, make_sampling
from test_gpu_generate_batch import BIAS, FIXTURES, GOLD, V6, Ctx, bits, row_params

pytestmark = pytest.mark.gpu

P_U = ctypes.POINTER(ctypes.c_uint32)
RWKV_ERROR_ARGS, RWKV_ERROR_CTX, RWKV_ERROR_UNSUPPORTED = 1 << 8, 6 << 8, 9
FILL, NONE = 0xFFFFFFFF, 0xFFFFFFFF
CAPS7 = [1, 2, 5, 3, 8, 1, 4]
# seven sequences: greedy, top_p = 1, temperature 0.7, and further streams
ROWS7 = dict(temperature=[0.0, 1.0, 0.7, 0.8, 1.0, 0.9, 0.0], top_p=[0.8, 1.0, 0.8, 0.5, 0.8, 0.9, 0.3],
             seeds=[41, 42, 43, 44, 45, 46, 47], offsets=[0, 3, 0, 7, 1, 2, 0], logit_bias=BIAS)
SAMPLED8 = dict(temperature=[1.0, 0.9, 0.7, 0.8, 1.0, 1.0, 0.9, 0.8], top_p=[0.9, 1.0, 0.8, 0.9, 0.8, 0.95, 0.9, 1.0],
                seeds=[51, 52, 53, 54, 55, 56, 57, 58], offsets=[0, 3, 0, 7, 1, 0, 2, 5])


@pytest.fixture(scope='module')
def world_model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp('generate_queue') / 'world-v6.bin')
    assert library().library.rwkv_mi355x_write_synthetic_model(p.encode(), 6, 65536, 256, 3, 0, b'Q5_1', 11)
    return p


class QCtx(Ctx):
    def prompt(self, r):
        """Row r's rotation of the prompt, odd rows without its last token."""
        p = super().prompt(r)
        return p[:len(p) - r % 2]

    def alone(self, s, n, kw, stop_tokens=()):
        """Sequence s by itself: slot 0 filled as the queue's slot s, generate_batch with B = 1."""
        q = row_params(kw, s)
        if self.L.rwkv_mi355x_batch_slots(self.ptr) != 1:
            assert self.L.rwkv_mi355x_batch_reserve(self.ptr, 1)
        self.start(s)
        assert self.L.rwkv_mi355x_batch_store(self.ptr, 0)
        p = make_batch_sampling(1, q['temperature'], q['top_p'], q['presence'], q['frequency'], q['logit_bias'],
                                [q['seed']], [q['offset']], stop_tokens, False, 0)
        ok, toks, lens, _ = self.run_raw(1, n, p)
        assert ok
        st, lg = self.slot(0)
        return [int(t) for t in toks[0][:lens[0]]], st, lg

    def queue(self, caps, lanes, kw, n=None, stop_tokens=(), check_every=0, fill=True):
        if fill:
            self.fill(len(caps))
        return library().rwkv_mi355x_generate_queue(
            self, caps, lanes, kw.get('temperature', 1.0), kw.get('top_p', 0.8), kw.get('presence'), kw.get('frequency'),
            kw.get('logit_bias'), kw['seeds'], kw.get('offsets', 0), stop_tokens, check_every, n)


def assert_sequences(c, out, caps, lanes, want, n=None):
    """Every sequence against its reference (tokens, state, logits), and the schedule."""
    n = max(caps) if n is None else n
    for s, (toks, st, lg) in enumerate(want):
        k = int(out['lengths'][s])
        assert [int(t) for t in out['tokens'][s]] == toks + [FILL] * (n - len(toks)), s
        assert k == len(toks), s
        gst, glg = c.slot(s)
        assert np.array_equal(bits(gst), bits(st)), s
        assert np.array_equal(bits(glg), bits(lg)), s
    lane, start, steps = sampling.queue_schedule(out['lengths'], lanes)
    assert list(out['lane']) == lane and list(out['start']) == start and out['steps'] == steps


# ------------------------------------------------------------------ 1. every architecture
@pytest.mark.parametrize('name', FIXTURES)
def test_sequences_equal_the_sequence_alone(name):
    c, ref = QCtx(os.path.join(GOLD, name)), QCtx(os.path.join(GOLD, name))
    try:
        out = c.queue(CAPS7, 3, ROWS7, n=8)
        assert list(out['lengths']) == CAPS7
        assert_sequences(c, out, CAPS7, 3, [ref.alone(s, CAPS7[s], ROWS7) for s in range(7)], n=8)
        # admissions at odd and at even steps: into both state buffers
        assert {int(x) % 2 for x in out['start'] if x > 0} == {0, 1}, list(out['start'])
    finally:
        c.free()
        ref.free()


# ------------------------------------------------------------------ 2. stops
# twelve sampled sequences; token 0 (every other token of this model's text) is biased away, so that
# the streams differ from their first token on
SAMPLED12 = dict(temperature=[(1.0, 0.9, 1.2)[s % 3] for s in range(12)], top_p=[(1.0, 0.95)[s % 2] for s in range(12)],
                 seeds=[60 + s for s in range(12)], offsets=[s % 4 for s in range(12)], logit_bias={0: -100.0})


def choose_stops(R, lanes):
    """Stop tokens and caps such that, on the streams R the sequences draw alone, one sequence stops on
    its first token, one exactly on its cap-th token (not its first), one never stops and two
    sequences are admitted at the same step > 0.  Returns (stops, caps, lengths)."""
    Q, n = len(R), len(R[0])
    for a, b, k in itertools.product(range(Q), range(Q), range(1, n)):
        stops = {R[a][0], R[b][k]}
        first = [next((i for i, t in enumerate(row) if t in stops), None) for row in R]
        if a == b or first[b] != k or None not in first:
            continue
        for base in itertools.permutations([n, n - 1, 3, 2], 3):
            caps = [base[s % 3] for s in range(Q)]
            caps[b] = k + 1
            lengths = [c if f is None or f >= c else f + 1 for c, f in zip(caps, first)]
            _, start, _ = sampling.queue_schedule(lengths, lanes)
            if any(x > 0 and start.count(x) >= 2 for x in start):
                return sorted(stops), caps, lengths
    raise AssertionError(f'no stop tokens with the four properties among the drawn tokens: {R}')


def test_stops():
    c, ref = QCtx(os.path.join(GOLD, V6)), QCtx(os.path.join(GOLD, V6))
    try:
        Q, lanes, n = 12, 3, 8
        R = [ref.alone(s, n, SAMPLED12)[0] for s in range(Q)]
        stops, caps, lengths = choose_stops(R, lanes)
        want = [ref.alone(s, caps[s], SAMPLED12, stops) for s in range(Q)]
        got_len = [len(w[0]) for w in want]
        assert got_len == lengths
        stopped = [w[0][-1] in stops for w in want]
        assert any(stopped[s] and got_len[s] == 1 for s in range(Q)), 'no sequence stops on its first token'
        assert any(stopped[s] and got_len[s] == caps[s] and caps[s] > 1 for s in range(Q)), 'no stop on the cap-th token'
        assert any(not stopped[s] and not set(R[s]) & set(stops) for s in range(Q)), 'no sequence runs to its cap'
        _, start, _ = sampling.queue_schedule(got_len, lanes)
        assert any(x > 0 and start.count(x) >= 2 for x in start), 'no two lanes free at the same step'
        # a sequence that stops on its cap-th token ends as stopped: its state has not consumed the token
        for s in range(Q):
            if stopped[s] and got_len[s] == caps[s] and caps[s] > 1:
                st, lg = ref.after(s, want[s][0][:-1])
                assert np.array_equal(bits(st), bits(want[s][1])) and np.array_equal(bits(lg), bits(want[s][2]))
        out = c.queue(caps, lanes, SAMPLED12, n=n, stop_tokens=stops)
        assert_sequences(c, out, caps, lanes, want, n=n)
    finally:
        c.free()
        ref.free()


# ------------------------------------------------------------------ 3. penalties
def test_penalties_do_not_leak_between_the_sequences_of_a_lane():
    c, ref = QCtx(os.path.join(GOLD, V6)), QCtx(os.path.join(GOLD, V6))
    try:
        caps = [3, 6, 2, 5, 4]
        kw = dict(temperature=[0.0, 0.0, 1.0, 0.8, 0.0], top_p=[0.8, 0.8, 0.8, 0.5, 1.0], seeds=[21, 22, 23, 24, 25],
                  offsets=[0, 0, 2, 0, 5], presence=0.3, frequency=0.2, logit_bias=BIAS)
        out = c.queue(caps, 2, kw)
        assert_sequences(c, out, caps, 2, [ref.stepwise(s, caps[s], kw) for s in range(5)])
        assert max(out['start']) > 0, 'no lane was used twice'
    finally:
        c.free()
        ref.free()


# ------------------------------------------------------------------ 4. degenerate shapes
def test_full_lanes_equal_generate_batch():
    c, ref = QCtx(os.path.join(GOLD, V6)), QCtx(os.path.join(GOLD, V6))
    try:
        Q, n = 5, 6
        kw = {k: (v[:Q] if isinstance(v, list) else v) for k, v in ROWS7.items()}
        toks, lens, steps = ref.run(Q, n=n, **kw)
        want = [ref.slot(r) for r in range(Q)]
        for lanes in (Q, 8):
            out = c.queue([n] * Q, lanes, kw)
            assert np.array_equal(out['tokens'], toks) and np.array_equal(out['lengths'], lens) and out['steps'] == steps
            assert list(out['lane']) == list(range(Q)) and list(out['start']) == [0] * Q
            for r in range(Q):
                st, lg = c.slot(r)
                assert np.array_equal(bits(st), bits(want[r][0])) and np.array_equal(bits(lg), bits(want[r][1]))
    finally:
        c.free()
        ref.free()


@pytest.mark.parametrize('Q,lanes', [(1, 1), (3, 256)])
def test_one_sequence_and_the_widest_queue(Q, lanes):
    c, ref = QCtx(os.path.join(GOLD, V6)), QCtx(os.path.join(GOLD, V6))
    try:
        caps = [5, 2, 4][:Q]
        out = c.queue(caps, lanes, {k: (v[:Q] if isinstance(v, list) else v) for k, v in ROWS7.items()})
        assert_sequences(c, out, caps, lanes, [ref.alone(s, caps[s], ROWS7) for s in range(Q)])
    finally:
        c.free()
        ref.free()


# ------------------------------------------------------------------ 5. check_every
def test_check_every_does_not_change_the_results():
    c = QCtx(os.path.join(GOLD, V6))
    try:
        R = c.queue(CAPS7, 3, ROWS7)
        stops = [int(R['tokens'][4][1])]  # the longest sequence ends early: the tail of the bound is idle
        runs = []
        for k in (0, 1, 5):
            out = c.queue(CAPS7, 3, ROWS7, n=8, stop_tokens=stops, check_every=k)
            runs.append((out, [c.slot(s) for s in range(7)]))
        assert runs[0][0]['lengths'][4] <= 2
        for out, slots in runs[1:]:
            for key in ('tokens', 'lengths', 'lane', 'start'):
                assert np.array_equal(out[key], runs[0][0][key]), key
            assert out['steps'] == runs[0][0]['steps']
            for (st, lg), (st0, lg0) in zip(slots, runs[0][1]):
                assert np.array_equal(bits(st), bits(st0)) and np.array_equal(bits(lg), bits(lg0))
    finally:
        c.free()


# ------------------------------------------------------------------ 6. the world vocabulary
def test_world_vocabulary(world_model):
    c, ref = QCtx(world_model), QCtx(world_model)
    try:
        caps = [2, 5, 1, 4, 3]
        kw = dict(temperature=[1.0, 0.9, 0.0, 0.8, 1.0], top_p=[0.9, 1.0, 0.8, 0.5, 0.8], seeds=[31, 32, 33, 34, 35],
                  offsets=[0, 3, 0, 7, 1], presence=[0.2, 0.0, 0.2, 0.0, 0.2], frequency=[0.2, 0.0, 0.1, 0.0, 0.2],
                  logit_bias=BIAS)
        out = c.queue(caps, 2, kw)
        assert_sequences(c, out, caps, 2, [ref.alone(s, caps[s], kw) for s in range(5)])
    finally:
        c.free()
        ref.free()


# ------------------------------------------------------------------ 7. the turnover kernel alone
def turnover_rule(lane_seq, done, length, max_tokens, nxt, step, fill):
    """Step 1 of the rule on plain integers (what k_gen_turnover does to its words)."""
    lanes, Q = len(lane_seq), len(done)
    lane_seq, done = list(lane_seq), list(done)
    retire, admit = [NONE] * lanes, [NONE] * lanes
    lane, start = [fill] * Q, [fill] * Q
    free = []
    for r, s in enumerate(lane_seq):
        if s != NONE and not done[s] and length[s] >= max_tokens[s]:
            retire[r], done[s] = s, 1
        if s == NONE or done[s]:
            free.append(r)
            lane_seq[r] = NONE
    for r in free:
        if nxt < Q:
            admit[r], lane_seq[r], lane[nxt], start[nxt] = nxt, nxt, r, step
            nxt += 1
    active = (Q - nxt) + sum(s != NONE for s in lane_seq)
    return dict(lane_seq=lane_seq, done=done, lane=lane, start=start, retire_to=retire, admit_from=admit, next=nxt,
                active=active)


@pytest.mark.parametrize('lanes', [1, 3, 64, 65, 256])
def test_turnover_kernel_is_the_rule(lanes):
    rng = np.random.default_rng(1000 + lanes)
    fill = 0xFFFFFFFE
    # (waiting sequences, share of idle lanes, share of ended ones among the busy)
    cases = [(0, 0.3, 0.5), (max(1, lanes // 4), 0.3, 0.9), (lanes + 5, 0.0, 1.0), (lanes + 5, 1.0, 0.0), (7, 0.0, 0.0),
             (2 * lanes, 0.2, 0.5), (3, 0.5, 0.5)]
    for case, (waiting, idle, ended) in enumerate(cases):
        nxt = lanes + int(rng.integers(0, 4))  # the sequences that have been admitted so far
        Q = nxt + waiting
        max_tokens = rng.integers(1, 9, Q).astype(np.uint32)
        length, done = np.zeros(Q, np.uint32), np.zeros(Q, np.uint32)
        lane_seq = np.full(lanes, NONE, np.uint32)
        held = rng.permutation(nxt)[:lanes]
        for s in range(nxt):  # not in a lane: ended long ago
            done[s], length[s] = 1, max_tokens[s]
        for r in range(lanes):
            if rng.random() < idle:
                continue
            s = int(held[r])
            lane_seq[r] = s
            if rng.random() < ended:
                kind = int(rng.integers(0, 3))  # a stop, the cap, a stop on the cap-th token
                done[s] = 0 if kind == 1 else 1
                length[s] = max_tokens[s] if kind else int(rng.integers(1, max_tokens[s] + 1))
            else:
                done[s], length[s] = 0, int(rng.integers(0, max_tokens[s]))
        want = turnover_rule(lane_seq, done, length, max_tokens, nxt, 17 + case, fill)
        got = library().rwkv_mi355x_selftest_gen_turnover(lane_seq, done, length, max_tokens, nxt, 17 + case, fill)
        for key, val in want.items():
            assert np.array_equal(np.asarray(got[key], np.int64), np.asarray(val, np.int64)), (case, key)
        free = sum(1 for r in range(lanes) if want['lane_seq'][r] == NONE or want['admit_from'][r] != NONE)
        if case == 2:
            assert free == lanes and want['next'] == nxt + lanes
        if case == 4:
            assert free == 0 and want['next'] == nxt


# ------------------------------------------------------------------ 8. continuation
def test_a_slot_continues_as_the_sequence_alone():
    c, ref = QCtx(os.path.join(GOLD, V6)), QCtx(os.path.join(GOLD, V6))
    try:
        caps = [3, 1, 4, 2]
        kw = {k: (v[:4] if isinstance(v, list) else v) for k, v in SAMPLED8.items()}
        R = [ref.alone(s, caps[s], kw)[0] for s in range(4)]
        stops = [R[2][1]]  # sequence 2 ends by a stop unless another draws the token first
        out = c.queue(caps, 2, kw, stop_tokens=stops)
        p = make_sampling(0.8, 0.5, None, 7, 0)
        for s in range(4):
            toks = ref.alone(s, caps[s], kw, stops)[0]
            assert [int(t) for t in out['tokens'][s][:out['lengths'][s]]] == toks
            more = []
            for x in (ref, c):
                # ref: slot 0 holds the alone run's result and alone() has loaded it
                if x is c:
                    assert x.L.rwkv_mi355x_batch_load(x.ptr, s)
                buf = (ctypes.c_uint32 * 4)()
                assert x.L.rwkv_mi355x_generate(x.ptr, ctypes.byref(p), 4, buf, None)
                more.append((list(buf), x.state(), x.logits()))
            assert more[0][0] == more[1][0], s
            assert np.array_equal(bits(more[0][1]), bits(more[1][1])) and np.array_equal(bits(more[0][2]), bits(more[1][2])), s
        assert out['lengths'][2] <= 2, 'sequence 2 did not end by the stop'
    finally:
        c.free()
        ref.free()


# ------------------------------------------------------------------ 9. one context's words under both calls
def test_batch_and_queue_calls_share_one_context():
    """generate_batch and generate_queue drive the same device words (done, length, fin_step, active;
    the queue's own behind them).  One reservation of 7 slots serves a batch call, a queue call and the
    batch call again, so the second batch call starts from the words the queue left."""
    c, ref, qref = (QCtx(os.path.join(GOLD, V6)) for _ in range(3))
    try:
        B, n, n2 = 3, 6, 5
        kw = {k: v[:B] for k, v in SAMPLED8.items()}
        more = dict(kw, offsets=[o + n for o in kw['offsets']])
        R, _, _ = ref.run(B, n=n, **kw)
        stops = [int(R[1][2])]  # row 1 draws it at its third token unless it or another row draws it sooner

        def stored(rows):
            for r in range(rows):
                c.start(r)
                assert c.L.rwkv_mi355x_batch_store(c.ptr, r)

        def batch(x, keep=False):
            p = make_batch_sampling(B, kw['temperature'], kw['top_p'], None, None, None, kw['seeds'],
                                    (more if keep else kw)['offsets'], stops, keep, 0)
            ok, toks, lens, steps = x.run_raw(B, n2 if keep else n, p)
            assert ok
            return toks, lens, steps, [x.slot(r) for r in range(B)]

        def same(a, b):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
            for (st, lg), (st0, lg0) in zip(a[3], b[3]):
                assert np.array_equal(bits(st), bits(st0)) and np.array_equal(bits(lg), bits(lg0))

        assert c.L.rwkv_mi355x_batch_reserve(c.ptr, 7)
        stored(B)
        first = batch(c)
        assert first[1][1] <= 3 and first[2] == n, 'row 1 did not end by the stop'
        stored(7)
        out = c.queue(CAPS7, 2, ROWS7, fill=False)
        out_slots = [c.slot(s) for s in range(7)]
        stored(B)
        third = batch(c)
        fourth = batch(c, keep=True)

        ref.fill(B)
        want = batch(ref)
        same(first, third)
        same(first, want)
        same(fourth, batch(ref, keep=True))
        qwant = qref.queue(CAPS7, 2, ROWS7)
        for key in ('tokens', 'lengths', 'lane', 'start'):
            assert np.array_equal(out[key], qwant[key]), key
        assert out['steps'] == qwant['steps'] and list(out['lengths']) == CAPS7
        for s in range(7):
            st, lg = qref.slot(s)
            assert np.array_equal(bits(out_slots[s][0]), bits(st)) and np.array_equal(bits(out_slots[s][1]), bits(lg)), s
    finally:
        for x in (c, ref, qref):
            x.free()


# ------------------------------------------------------------------ 10. the launches of a step
def launches(c, run):
    """run()'s result and {kernel class: launches} of rwkv_mi355x_kernel_stats for it."""
    c.L.rwkv_mi355x_set_kernel_timing(c.ptr, True)  # clears the table
    out = run()
    table = {}
    for i in range(c.L.rwkv_mi355x_kernel_stats(c.ptr, -1, None, 0, None, None, None, None)):
        name = ctypes.create_string_buffer(128)
        la, ms, by, fl = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        c.L.rwkv_mi355x_kernel_stats(c.ptr, i, name, 128, ctypes.byref(la), ctypes.byref(ms), ctypes.byref(by), ctypes.byref(fl))
        table[name.value.decode()] = la.value
    return out, table


def test_launches_per_step():
    """What a step enqueues besides the batched decode, counted from the loop bounds: the batch runs n
    steps of {sampler, snapshot}; the queue ceil(sum caps / lanes) + max caps steps of {turnover,
    move, sampler, snapshot}, or as many as were needed when the host looks at `active` every step."""
    c = QCtx(os.path.join(GOLD, V6), timing=True)
    try:
        B, n, lanes = 3, 5, 3
        bound = -(-sum(CAPS7) // lanes) + max(CAPS7)
        assert bound == 16
        kw = {k: v[:B] for k, v in SAMPLED8.items()}
        p = make_batch_sampling(B, kw['temperature'], kw['top_p'], None, None, None, kw['seeds'], kw['offsets'], (), False, 0)
        per_step = ('k_gen_turnover', 'k_gen_move', 'k_sample_rows', 'k_gen_snapshot')

        def queue(check_every, logprobs=None):
            return library().rwkv_mi355x_generate_queue(c, CAPS7, lanes, ROWS7['temperature'], ROWS7['top_p'], None, None,
                                                        ROWS7['logit_bias'], ROWS7['seeds'], ROWS7['offsets'], (),
                                                        check_every, None, logprobs)

        for lp in (None, 2):
            sampler = 'k_sample_rows_lp' if lp else 'k_sample_rows'
            c.fill(B)
            (_, lens, steps, *_), t = launches(c, lambda: library().rwkv_mi355x_generate_batch(c, B, n, p, lp))
            assert list(lens) == [n] * B and steps == n
            assert t[sampler] == n and t['k_gen_snapshot'] == n
            assert 'k_gen_turnover' not in t and 'k_gen_move' not in t
            assert t.get('k_logprobs') == (n if lp else None) and ('k_sample_rows' in t) == (lp is None)
            for check_every in (0, 1):
                c.fill(7)
                out, t = launches(c, lambda: queue(check_every, lp))
                assert list(out['lengths']) == CAPS7 and out['steps'] < bound
                want = out['steps'] if check_every else bound
                assert [t[k if k != 'k_sample_rows' else sampler] for k in per_step] == [want] * 4, (lp, check_every, t)
                assert t.get('k_logprobs') == (want if lp else None) and ('k_sample_rows' in t) == (lp is None)
    finally:
        c.L.rwkv_mi355x_set_kernel_timing(c.ptr, False)
        c.free()


# ------------------------------------------------------------------ 11. errors
def test_argument_errors_leave_the_slots_alone():
    c, ref = QCtx(os.path.join(GOLD, V6)), QCtx(os.path.join(GOLD, V6))
    try:
        caps = [2, 3, 1]
        kw = dict(temperature=[0.0, 0.8, 0.5], top_p=0.5, seeds=[1, 2, 3])
        want = [ref.alone(s, caps[s], kw) for s in range(3)]
        assert c.L.rwkv_mi355x_batch_reserve(c.ptr, 4)
        for s in range(3):
            c.start(s)
            assert c.L.rwkv_mi355x_batch_store(c.ptr, s)
        before = [c.slot(s) for s in range(3)]

        def params(Q=3, **over):
            return make_batch_sampling(Q, **dict(dict(temperature=[0.0, 0.8, 0.5, 0.5][:Q], top_p=0.5, seeds=[1, 2, 3, 4][:Q]),
                                                 **over))

        def call(Q=3, lanes=2, p=None, caps=(2, 3, 1), n=4, null=()):
            cap = np.array(list(caps) + [1] * 8, np.uint32)
            toks, lens = np.zeros((max(Q, 1), 8), np.uint32), np.zeros(max(Q, 1), np.uint32)
            args = dict(max_tokens=cap.ctypes.data_as(P_U), tokens=toks.ctypes.data_as(P_U), lengths=lens.ctypes.data_as(P_U))
            for k in null:
                args[k] = None
            return c.L.rwkv_mi355x_generate_queue(c.ptr, Q, lanes, ctypes.byref(p) if p is not None else None,
                                                  args['max_tokens'], n, args['tokens'], args['lengths'], None, None, None)

        nan = float('nan')
        cases = [dict(Q=0, p=params()), dict(Q=5, p=params(4)), dict(Q=4, p=params(4), caps=(2, 3, 1, 1)),  # slot 3 never stored
                 dict(lanes=0, p=params()), dict(lanes=257, p=params()), dict(n=0, p=params()), dict(n=65537, p=params()),
                 dict(p=None), dict(p=params(), null=('max_tokens',)), dict(p=params(), null=('tokens',)),
                 dict(p=params(), null=('lengths',)), dict(p=params(), caps=(2, 0, 1)), dict(p=params(), caps=(2, 5, 1)),
                 dict(p=params(keep_counts=True)),
                 dict(p=params(temperature=[0.5, -1.0, 0.5])), dict(p=params(temperature=[nan, 0.5, 0.5])),
                 dict(p=params(top_p=[0.5, 1.5, 0.5])), dict(p=params(presence=[0.0, nan, 0.0])),
                 dict(p=params(frequency=[nan, 0.0, 0.0])), dict(p=params(logit_bias={i: 0.0 for i in range(257)})),
                 dict(p=params(logit_bias={c.V: 1.0})), dict(p=params(stop_tokens=list(range(17)))),
                 dict(p=params(stop_tokens=[c.V]))]
        for i, kwargs in enumerate(cases):
            assert not call(**kwargs) and c.error() == RWKV_ERROR_ARGS, i
        for null in ('temperature', 'top_p', 'seed', 'offset'):
            p = params()
            setattr(p, null, None)
            assert not call(p=p) and c.error() == RWKV_ERROR_ARGS, null
        # nothing moved: the slots hold the same bits, and the queue gives the reference result
        for s in range(3):
            st, lg = c.slot(s)
            assert np.array_equal(bits(st), bits(before[s][0])) and np.array_equal(bits(lg), bits(before[s][1]))
        out = c.queue(caps, 2, kw, fill=False)
        assert_sequences(c, out, caps, 2, want)
    finally:
        c.free()
        ref.free()


def test_pipeline_context_is_refused():
    L = library().library
    devs = (ctypes.c_int * 2)(0, 0)
    pipe = L.rwkv_mi355x_init_pipeline(os.path.join(GOLD, V6).encode(), 1, 2, devs)
    assert pipe
    try:
        p = make_batch_sampling(2, 0.0, 0.5)
        caps, toks, lens = (ctypes.c_uint32 * 2)(4, 4), (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 2)()
        assert not L.rwkv_mi355x_generate_queue(pipe, 2, 2, ctypes.byref(p), caps, 4, toks, lens, None, None, None)
        assert L.rwkv_get_last_error(pipe) == RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED
    finally:
        L.rwkv_free(pipe)
