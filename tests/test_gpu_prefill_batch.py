"""rwkv_mi355x_prefill_batch (include/rwkv_mi355x.h): many prompts evaluated together in packed
sequence passes land in their slots exactly as the single-sequence path leaves them.

The yardstick is that path, which the rest of the suite pins to the oracle: for row i,
state_upload(NULL), eval_device(prompt_i, logits), state_download and debug_buffer('logits') against
batch_load(slot_i) and the same two reads, np.array_equal on the uint32 views.  Nothing here takes
a tolerance."""
import ctypes
import os

import numpy as np
import pytest

from rwkv_lib import library
from rwkv_cpp import RWKVModel
from rwkv_cpp.rwkv_cpp_shared_library import make_batch_sampling, make_sampling
from synth import write_synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
P_F = ctypes.POINTER(ctypes.c_float)
P_U = ctypes.POINTER(ctypes.c_uint32)
P_SZ = ctypes.POINTER(ctypes.c_size_t)
P_B = ctypes.POINTER(ctypes.c_uint8)
RWKV_ERROR_ARGS, RWKV_ERROR_CTX, RWKV_ERROR_UNSUPPORTED = 1 << 8, 6 << 8, 9
FIXTURES = ['tiny-rwkv-4v0-660K-FP16.bin', 'tiny-rwkv-5v2-730K-FP16.bin', 'tiny-rwkv-6v0-3m-Q5_1.bin',
            'tiny-rwkv-7v0-834K-FP16.bin']
V6 = os.path.join(GOLD, 'tiny-rwkv-6v0-3m-Q5_1.bin')
TEXT = list(b'This is a port of [BlinkDL/RWKV-LM] to the MI355X; ')  # row r reads its rotation by r
# a lone token; boundaries inside a 4-token workgroup; the WKV-4 / WKV-7 chunk of 16 and 16 + 1; the
# WKV-6 chunk and GEMM tile of 64 and 64 + 1; two chunks plus a tail; two one-token rows apart
LENGTHS = [1, 3, 16, 17, 64, 65, 2, 130, 1]
ROWS5 = dict(temperature=[0.0, 1.0, 0.7, 0.8, 1.0], top_p=[0.8, 1.0, 0.8, 0.5, 0.8], seeds=[11, 12, 13, 14, 15],
             offsets=[0, 3, 0, 7, 1])
# head size 64: one quantised format per architecture (Q8_0 and Q8_1 activation tiles both) and FP16
HEAD64 = [(4, 'Q4_0'), (4, 'FP16'), (5, 'Q5_1'), (5, 'FP16'), (6, 'Q5_0'), (6, 'FP16'), (7, 'Q4_1'), (7, 'FP16')]


def bits(a):
    return np.asarray(a).view(np.uint32)


def row_tokens(V, r, length):
    return [(TEXT[(r + k) % len(TEXT)] + k // len(TEXT)) % V for k in range(length)]


@pytest.fixture(scope='module')
def synth_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp('prefill_batch'))


def head64_model(synth_dir, arch, fmt):
    p = os.path.join(synth_dir, f'v{arch}-{fmt}.bin')
    assert write_synth(p, arch, 512, 128, 2, fmt, 29, norms=1, wide_decay=1)
    return p


@pytest.fixture(scope='module')
def world_model(synth_dir):
    p = os.path.join(synth_dir, 'world-v6.bin')
    assert library().library.rwkv_mi355x_write_synthetic_model(p.encode(), 6, 65536, 256, 3, 0, b'Q5_1', 11)
    return p


_SERIAL = {}  # (model path, tokens) -> (state, logits) of the single-sequence path, computed once


class Ctx:
    def __init__(self, path, knobs=None, timing=False):
        self.L = library().library
        self.path = path
        self.ptr = self.L.rwkv_init_from_file(path.encode(), 1, 99)
        assert self.ptr
        for k, v in (knobs or {}).items():
            assert self.L.rwkv_mi355x_debug_set(self.ptr, k.encode(), v)
        self.timing = timing
        if timing:
            self.L.rwkv_mi355x_set_kernel_timing(self.ptr, True)
        self.V = self.L.rwkv_get_n_vocab(self.ptr)

    def free(self):
        if self.timing:
            self.L.rwkv_mi355x_set_kernel_timing(self.ptr, False)
        self.L.rwkv_free(self.ptr)

    def knob(self, name, value):
        assert self.L.rwkv_mi355x_debug_set(self.ptr, name.encode(), value)

    def eval(self, tokens):
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        assert self.L.rwkv_mi355x_eval_device(self.ptr, arr, len(tokens), True, None, True)

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

    def serial(self, tokens):
        """(state, logits) after the tokens from a fresh state, by the single-sequence path."""
        key = (self.path, tuple(tokens))
        if key not in _SERIAL:
            assert self.L.rwkv_mi355x_state_upload(self.ptr, None)
            self.eval(tokens)
            st, lg = self.state(), self.logits()
            st.flags.writeable = lg.flags.writeable = False
            _SERIAL[key] = (st, lg)
        return _SERIAL[key]

    def reserve(self, n):
        assert self.L.rwkv_mi355x_batch_reserve(self.ptr, n)

    def store_serial(self, slot, tokens):
        assert self.L.rwkv_mi355x_state_upload(self.ptr, None)
        self.eval(tokens)
        assert self.L.rwkv_mi355x_batch_store(self.ptr, slot)

    def slot(self, r):
        assert self.L.rwkv_mi355x_batch_load(self.ptr, r)
        return self.state(), self.logits()

    def prefill_raw(self, n_rows, slots, tokens, lengths, cont):
        def arr(t, v):
            return None if v is None else (t * max(1, len(v)))(*v)
        return self.L.rwkv_mi355x_prefill_batch(self.ptr, n_rows, arr(ctypes.c_uint32, slots), arr(ctypes.c_uint32, tokens),
                                                arr(ctypes.c_size_t, lengths), arr(ctypes.c_uint8, cont))

    def prefill(self, prompts, slots, cont=None):
        return self.prefill_raw(len(prompts), slots, [t for p in prompts for t in p], [len(p) for p in prompts], cont)

    def generate(self, B, n, kw):
        p = make_batch_sampling(B, kw['temperature'], kw['top_p'], None, None, None, kw['seeds'], kw['offsets'], (), False, 0)
        toks, lens = np.zeros((B, n), np.uint32), np.zeros(B, np.uint32)
        assert self.L.rwkv_mi355x_generate_batch(self.ptr, B, ctypes.byref(p), n, toks.ctypes.data_as(P_U),
                                                 lens.ctypes.data_as(P_U), None)
        return toks, lens


def assert_slots(c, prompts, slots, ref=None):
    for i, (p, s) in enumerate(zip(prompts, slots)):
        want = (ref or c).serial(p)
        st, lg = c.slot(s)
        assert np.array_equal(bits(st), bits(want[0])), (i, len(p), 'state')
        assert np.array_equal(bits(lg), bits(want[1])), (i, len(p), 'logits')


def plan(lengths, cap):
    count, rows, begins, lens, chunks = library().rwkv_mi355x_selftest_prefill_plan(lengths, cap)
    assert count > 0
    return rows[:count], begins[:count], lens[:count], chunks[:count]


def run_shapes(path, knobs=None, timing=False, caps=(0,), ref_path=None):
    """One prefill of the LENGTHS rows into reversed slots 1 .. B of B + 2, beside a stored slot 0 and
    a never-stored slot B + 1, under every packing cap of `caps` (0: the default)."""
    c = Ctx(path, knobs, timing)
    ref = Ctx(ref_path) if ref_path else None  # a context without the arm, for the yardstick
    try:
        B = len(LENGTHS)
        prompts = [row_tokens(c.V, r, n) for r, n in enumerate(LENGTHS)]
        slots = list(range(B, 0, -1))
        spare = row_tokens(c.V, 40, 7)
        one = dict(temperature=[0.9], top_p=[0.7], seeds=[5], offsets=[2])
        c.reserve(B + 2)
        c.store_serial(0, spare)
        # the target slots hold another sequence's state beforehand: a fresh row that read its slot
        # instead of the fresh state would show (freshly allocated slots may be all zero, as a fresh
        # v5 / v6 / v7 state is)
        for s in slots:
            assert c.L.rwkv_mi355x_batch_store(c.ptr, s)
        spare_tokens, _ = c.generate(1, 6, one)
        for cap in caps:
            c.knob('prefill_chunk', cap)
            c.store_serial(0, spare)
            before = c.slot(0)
            assert c.prefill(prompts, slots), cap
            assert_slots(c, prompts, slots, ref)
            # the stored slot beside them kept its bits and generates what it generated; the empty one is empty
            after = c.slot(0)
            assert np.array_equal(bits(after[0]), bits(before[0])) and np.array_equal(bits(after[1]), bits(before[1]))
            assert np.array_equal(c.generate(1, 6, one)[0], spare_tokens)
            assert not c.L.rwkv_mi355x_batch_load(c.ptr, B + 1) and c.error() == RWKV_ERROR_ARGS
    finally:
        if ref:
            ref.free()
        c.free()


# ------------------------------------------------------------------ 1. the generic head-size kernels
@pytest.mark.parametrize('name', FIXTURES)
def test_tiny_fixtures(name):
    run_shapes(os.path.join(GOLD, name))


# ------------------------------------------------------------------ 2. head size 64, real norms and decays
@pytest.mark.parametrize('arch,fmt', HEAD64)
def test_head_size_64(arch, fmt, synth_dir):
    run_shapes(head64_model(synth_dir, arch, fmt))


# ------------------------------------------------------------------ 3. the gathered head lands in the right slots
def test_real_vocabulary_33_rows(world_model):
    c = Ctx(world_model)
    try:
        B = 33
        prompts = [row_tokens(c.V, r, 1 + r % 5) for r in range(B)]
        slots = list(range(B - 1, -1, -1))
        c.reserve(B)
        c.store_serial(0, row_tokens(c.V, 40, 7))  # every slot holds another sequence beforehand
        for s in slots[:-1]:
            assert c.L.rwkv_mi355x_batch_store(c.ptr, s)
        assert c.prefill(prompts, slots)
        assert_slots(c, prompts, slots)
    finally:
        c.free()


# ------------------------------------------------------------------ 4. packing does not change bits
def test_the_caps_split_rows():
    rows, _, lens, chunks = plan(LENGTHS, 8)
    pieces = np.bincount(rows)
    assert pieces.max() >= 3 and (lens == 1).any()
    for cap in (64, 100):
        rows, _, lens, _ = plan(LENGTHS, cap)
        assert np.bincount(rows).max() >= 2, cap
    # a split row whose remainder in the next chunk is one token (the 64-token row at cap 100)
    rows, _, lens, _ = plan(LENGTHS, 100)
    assert ((lens == 1) & (np.bincount(rows)[rows] > 1)).any()


@pytest.mark.parametrize('which', ['tiny4', 'tiny6', 'tiny7', (4, 'Q4_0'), (5, 'Q5_1'), (6, 'Q5_0'), (7, 'Q4_1')],
                         ids=lambda w: w if isinstance(w, str) else f'v{w[0]}-{w[1]}')
def test_packing_does_not_change_bits(which, synth_dir):
    tiny = {'tiny4': FIXTURES[0], 'tiny6': FIXTURES[2], 'tiny7': FIXTURES[3]}
    path = os.path.join(GOLD, tiny[which]) if isinstance(which, str) else head64_model(synth_dir, *which)
    run_shapes(path, caps=(8, 64, 100, 0))


# ------------------------------------------------------------------ 5. continuation
@pytest.mark.parametrize('which', ['tiny6', (4, 'Q4_0'), (7, 'Q4_1')], ids=lambda w: w if isinstance(w, str) else f'v{w[0]}-{w[1]}')
@pytest.mark.parametrize('cap', [0, 8])
def test_continuation(which, cap, synth_dir):
    c = Ctx(V6 if which == 'tiny6' else head64_model(synth_dir, *which), {'prefill_chunk': cap})
    try:
        whole = [row_tokens(c.V, r, n) for r, n in enumerate([34, 21, 9, 40])]
        half = [len(p) // 2 for p in whole]
        c.reserve(4)
        for r in range(4):
            c.store_serial(r, whole[r][:half[r]])
        prompts = [whole[0][half[0]:], whole[1], whole[2][half[2]:], whole[3]]
        assert c.prefill(prompts, [0, 1, 2, 3], [1, 0, 1, 0])
        assert_slots(c, whole, [0, 1, 2, 3])
    finally:
        c.free()


# ------------------------------------------------------------------ 6. extremes
def test_one_row_of_one_token():
    c = Ctx(V6)
    try:
        c.reserve(1)
        prompts = [row_tokens(c.V, 3, 1)]
        assert c.prefill(prompts, [0])
        assert_slots(c, prompts, [0])
    finally:
        c.free()


def test_256_rows():
    c = Ctx(V6)
    try:
        B = 256
        prompts = [row_tokens(c.V, r, 1 + r % 3) for r in range(B)]
        slots = list(range(B))
        c.reserve(B)
        assert c.prefill(prompts, slots)
        assert_slots(c, prompts, slots)
    finally:
        c.free()


# ------------------------------------------------------------------ 7. generation from prefilled slots
def test_generation_from_prefilled_slots():
    c = Ctx(V6)
    try:
        prompts = [row_tokens(c.V, r, 20) for r in range(5)]
        c.reserve(5)
        for r in range(5):
            c.store_serial(r, prompts[r])
        want = c.generate(5, 12, ROWS5)
        assert c.prefill(prompts, list(range(5)))
        got = c.generate(5, 12, ROWS5)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    finally:
        c.free()


def test_model_generate_batch_with_batched_prefill():
    m = RWKVModel(library(), V6, gpu_layer_count=99)
    try:
        prompts = [row_tokens(256, r, n) for r, n in enumerate([20, 1, 7, 33, 2])]
        kw = dict(temperature=ROWS5['temperature'], top_p=ROWS5['top_p'], seeds=ROWS5['seeds'], stop_tokens=[10])
        want = m.generate_batch(prompts, 12, **kw)
        assert m.generate_batch(prompts, 12, batched_prefill=True, **kw) == want
        # the wrapper alone: slots chosen by the caller, a continuation
        m.prefill_batch([p[:1] for p in prompts[:2]], slots=[4, 2])
        m.prefill_batch([prompts[0][1:], prompts[1][1:] + [65]], slots=[4, 2], cont=True)
        m.prefill_batch([prompts[0], prompts[1] + [65]], slots=[0, 1])
        lib, ctx = m._library, m._ctx
        for a, b in ((4, 0), (2, 1)):
            got = []
            for s in (a, b):
                lib.rwkv_mi355x_batch_load(ctx, s)
                st = np.zeros(m._state_buffer_element_count, np.float32)
                assert lib.library.rwkv_mi355x_state_download(ctx.ptr, st.ctypes.data_as(P_F))
                got.append(st)
            assert np.array_equal(bits(got[0]), bits(got[1]))
    finally:
        m.free()


# ------------------------------------------------------------------ 8. the context's own state and logits
def test_context_untouched():
    c = Ctx(V6)
    try:
        c.reserve(9)
        assert c.L.rwkv_mi355x_state_upload(c.ptr, None)
        c.eval(row_tokens(c.V, 9, 11))
        p = make_sampling(0.9, 0.6, None, 21, 4)

        def look():
            tok = ctypes.c_uint32(0xFFFFFFFF)
            assert c.L.rwkv_mi355x_sample(c.ptr, ctypes.byref(p), ctypes.byref(tok))
            return c.state(), c.logits(), tok.value

        before = look()
        prompts = [row_tokens(c.V, r, n) for r, n in enumerate(LENGTHS)]
        assert c.prefill(prompts, list(range(9)))
        after = look()
        assert np.array_equal(bits(after[0]), bits(before[0])) and np.array_equal(bits(after[1]), bits(before[1]))
        assert after[2] == before[2]
        # and it goes on from there as if nothing had happened
        c.eval([65])
        mid = c.state()
        assert np.array_equal(bits(mid), bits(c.serial(row_tokens(c.V, 9, 11) + [65])[0]))
    finally:
        c.free()


# ------------------------------------------------------------------ 9. arms
@pytest.mark.parametrize('arm', ['no_graphs', 'timing'])
@pytest.mark.parametrize('which', ['tiny6', (6, 'Q5_0')], ids=lambda w: w if isinstance(w, str) else f'v{w[0]}-{w[1]}')
def test_arms_give_the_same_bits(arm, which, synth_dir):
    path = V6 if which == 'tiny6' else head64_model(synth_dir, *which)
    run_shapes(path, {'graphs': 0} if arm == 'no_graphs' else None, timing=arm == 'timing', caps=(0, 8), ref_path=path)


# ------------------------------------------------------------------ 10. errors
def test_argument_errors_leave_the_slots_alone():
    c = Ctx(V6)
    try:
        c.reserve(4)
        stored = row_tokens(c.V, 2, 9)
        c.store_serial(0, stored)
        c.store_serial(1, stored[:4])
        before = [c.slot(r) for r in range(2)]
        good = dict(n_rows=2, slots=[0, 1], tokens=[1, 2, 3, 4, 5], lengths=[2, 3], cont=None)
        cases = dict(
            no_rows=dict(n_rows=0), too_many_rows=dict(n_rows=5, slots=[0, 1, 2, 3, 0], tokens=[1] * 5, lengths=[1] * 5),
            null_slots=dict(slots=None), null_tokens=dict(tokens=None), null_lengths=dict(lengths=None),
            slot_out_of_range=dict(slots=[0, 4]), slot_twice=dict(slots=[1, 1]), zero_length=dict(lengths=[5, 0]),
            token_out_of_range=dict(tokens=[1, 2, 3, c.V, 5]), cont_on_empty_slot=dict(slots=[0, 2], cont=[1, 1]))
        for name, over in cases.items():
            assert not c.prefill_raw(**dict(good, **over)), name
            assert c.error() == RWKV_ERROR_ARGS, name
        for r in range(2):
            st, lg = c.slot(r)
            assert np.array_equal(bits(st), bits(before[r][0])) and np.array_equal(bits(lg), bits(before[r][1])), r
        assert not c.L.rwkv_mi355x_batch_load(c.ptr, 2) and c.error() == RWKV_ERROR_ARGS
        # the packing cap: 1 up to the sequence chunk
        assert not c.L.rwkv_mi355x_debug_set(c.ptr, b'prefill_chunk', 1025)
        # and the good call is good
        assert c.prefill_raw(**good)
        assert_slots(c, [[1, 2], [3, 4, 5]], [0, 1])
    finally:
        c.free()


def test_pipeline_and_stage_contexts_are_refused():
    L = library().library
    devs = (ctypes.c_int * 2)(0, 0)
    pipe = L.rwkv_mi355x_init_pipeline(V6.encode(), 1, 2, devs)
    assert pipe
    stage = L.rwkv_mi355x_init_from_file_layers(V6.encode(), 1, 0, L.rwkv_get_n_layer(pipe) - 1)
    assert stage
    try:
        slots, toks, lens = (ctypes.c_uint32 * 1)(0), (ctypes.c_uint32 * 2)(1, 2), (ctypes.c_size_t * 1)(2)
        for ptr in (pipe, stage):
            assert not L.rwkv_mi355x_prefill_batch(ptr, 1, slots, toks, lens, None)
            assert L.rwkv_get_last_error(ptr) == RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED
    finally:
        L.rwkv_free(stage)
        L.rwkv_free(pipe)
