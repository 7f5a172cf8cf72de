"""rwkv_mi355x_score_sequence (include/rwkv_mi355x.h), the whole path: the sequence evaluation with the
head on every token gives, per position, the logits of serial rwkv_eval bit for bit, the state of
the serial loop bit for bit, and losses / argmaxes that are perplexity.cross_entropy / np.argmax of
those logits (losses within 1e-9: test_gpu_xent.py derives the bound)."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest

from oracle_ctypes import VARIANT_GPU, OracleModel, set_variant
from rwkv_lib import RWKVModel, library
from rwkv_cpp import convert, perplexity
from rwkv_cpp.perplexity import cross_entropy
from rwkv_cpp.rwkv_cpp_shared_library import make_sampling

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
P_F = ctypes.POINTER(ctypes.c_float)
P_U = ctypes.POINTER(ctypes.c_uint32)
P_D = ctypes.POINTER(ctypes.c_double)
RWKV_ERROR_ARGS, RWKV_ERROR_CTX, RWKV_ERROR_UNSUPPORTED = 1 << 8, 6 << 8, 9
FIXTURES = ['tiny-rwkv-4v0-660K-FP32.bin', 'tiny-rwkv-5v2-730K-FP16.bin', 'tiny-rwkv-6v0-3m-Q5_1.bin',
            'tiny-rwkv-7v0-834K-FP16.bin']
V6 = os.path.join(GOLD, 'tiny-rwkv-6v0-3m-Q5_1.bin')
TEXT = list(b'This is a port of [BlinkDL/RWKV-LM](https://github.com/BlinkDL/RWKV-LM')  # T = 70
TOL = 1e-9
R = 128  # Engine::kScoreRows, the head tile


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Ctx:
    """A context on the device-resident state through the raw ABI."""

    def __init__(self, path=None, ptr=None):
        self.lib = library()
        self.L = self.lib.library
        self.ptr = ptr or self.L.rwkv_init_from_file(path.encode(), 1, 99)
        assert self.ptr
        self.V = self.L.rwkv_get_n_vocab(self.ptr)

    def free(self):
        self.L.rwkv_free(self.ptr)

    def fresh(self):
        assert self.L.rwkv_mi355x_state_upload(self.ptr, None)

    def state(self):
        st = np.zeros(self.L.rwkv_get_state_len(self.ptr), np.float32)
        assert self.L.rwkv_mi355x_state_download(self.ptr, st.ctypes.data_as(P_F))
        return st

    def score(self, tokens, targets=None, want_logits=False):
        return self.lib.rwkv_mi355x_score_sequence(self, tokens, targets, want_logits)

    def eval_device(self, tokens):
        """rwkv_mi355x_eval_device of the tokens; the last token's logits."""
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        lg = np.zeros(self.V, np.float32)
        assert self.L.rwkv_mi355x_eval_device(self.ptr, arr, len(tokens), True, lg.ctypes.data_as(P_F), True)
        return lg

    def device_logits(self):
        lg = np.zeros(self.V, np.float32)
        assert self.L.rwkv_mi355x_debug_buffer(self.ptr, b'logits', lg.ctypes.data_as(P_F), lg.nbytes) == lg.nbytes
        return lg

    def serial(self, tokens, keep_states=()):
        """One rwkv_eval per token from a fresh state through the host-state ABI: the logits of every
        position, the final state, and the states after the token counts in keep_states."""
        lg = np.zeros((len(tokens), self.V), np.float32)
        st = np.zeros(self.L.rwkv_get_state_len(self.ptr), np.float32)
        kept = {}
        for i, t in enumerate(tokens):
            sin = st.ctypes.data_as(P_F) if i else None
            assert self.L.rwkv_eval(self.ptr, int(t), sin, st.ctypes.data_as(P_F), lg[i].ctypes.data_as(P_F))
            if i + 1 in keep_states:
                kept[i + 1] = st.copy()
        return lg, st, kept

    def error(self):
        return self.L.rwkv_get_last_error(self.ptr)


def check_against_logits(got, ref_logits, targets):
    """(losses, argmax, logits) of a score call against the reference logits of the same positions."""
    losses, argmax, logits = got
    if logits is not None:
        assert np.array_equal(bits(logits), bits(ref_logits))
    want = np.array([cross_entropy(row, int(t)) for row, t in zip(ref_logits, targets)])
    err = np.abs(losses - want).max()
    print(f'T {len(targets)}: max |loss - ref| = {err:.3e}')
    assert err <= TOL
    assert np.array_equal(argmax, np.argmax(ref_logits, axis=1).astype(np.uint32))


def check_model(path):
    c = Ctx(path)
    try:
        tokens = [t % c.V for t in TEXT]
        targets = tokens[1:] + [c.V - 1]
        ref_logits, ref_state, _ = c.serial(tokens)
        c.fresh()
        got = c.score(tokens, targets, want_logits=True)
        check_against_logits(got, ref_logits, targets)
        assert np.array_equal(bits(c.state()), bits(ref_state))
        assert np.array_equal(bits(c.device_logits()), bits(ref_logits[-1]))
        # without targets and without the logits: the argmaxes alone
        c.fresh()
        losses, argmax, logits = c.score(tokens)
        assert losses is None and logits is None and np.array_equal(argmax, got[1])
    finally:
        c.free()


@pytest.mark.parametrize('name', FIXTURES)
def test_score_equals_serial_eval(name):
    check_model(os.path.join(GOLD, name))


def test_score_equals_serial_eval_world_vocabulary(tmp_path):
    p = str(tmp_path / 'world-v6.bin')
    assert library().library.rwkv_mi355x_write_synthetic_model(p.encode(), 6, 65536, 256, 3, 0, b'Q5_1', 11)
    check_model(p)


def test_score_equals_the_oracle():
    tokens, targets = TEXT, TEXT[1:] + [0]
    set_variant(VARIANT_GPU)
    try:
        o = OracleModel(V6)
        rows, state = [], None
        for t in tokens:
            lg, state = o.eval_sequence([t], state)
            rows.append(np.array(lg, np.float32))
    finally:
        set_variant(0)
    c = Ctx(V6)
    try:
        check_against_logits(c.score(tokens, targets, want_logits=True), np.stack(rows), targets)
        assert np.array_equal(bits(c.state()), bits(state))
    finally:
        c.free()


@pytest.mark.parametrize('ignore_first_n', [0, 8])
def test_measure_device_equals_measure(ignore_first_n):
    m = RWKVModel(library(), V6)
    try:
        loss, _, n = perplexity.measure(m, TEXT, ignore_first_n)
        for chunk in (1024, 16):
            dloss, dppl, dn = perplexity.measure_device(m, TEXT, ignore_first_n, chunk=chunk)
            assert dn == n and abs(dloss - loss) <= TOL and dppl == math.exp(dloss)
    finally:
        m.free()


# ---- boundaries (the 6v0 fixture, random tokens): one token, the k_mm / k_fmm switch at 32 rows, the
# head tile R, and an engine chunk of 1024 plus a one-token decode tail
SMALL_T = [1, 31, 32, 33, R - 1, R, R + 1]


@pytest.fixture(scope='module')
def v6_serial():
    tokens = [int(t) for t in np.random.default_rng(5).integers(0, 256, 1026)]
    c = Ctx(V6)
    try:
        logits, _, states = c.serial(tokens[:R + 1], keep_states=SMALL_T)
    finally:
        c.free()
    return tokens, logits, states


@pytest.mark.parametrize('T', SMALL_T)
def test_boundary_lengths(T, v6_serial):
    tokens, ref_logits, ref_states = v6_serial
    c = Ctx(V6)
    try:
        got = c.score(tokens[:T], tokens[1:T + 1], want_logits=True)
        check_against_logits(got, ref_logits[:T], tokens[1:T + 1])
        assert np.array_equal(bits(c.state()), bits(ref_states[T]))
        assert np.array_equal(bits(c.device_logits()), bits(ref_logits[T - 1]))
    finally:
        c.free()


def test_engine_chunk_plus_decode_tail(v6_serial):
    tokens, T = v6_serial[0], 1025
    c = Ctx(V6)
    try:
        want_last = c.eval_device(tokens[:T])
        want_state = c.state()
        c.fresh()
        losses, argmax, _ = c.score(tokens[:T], tokens[1:T + 1])
        assert np.array_equal(bits(c.device_logits()), bits(want_last))
        assert np.array_equal(bits(c.state()), bits(want_state))
        # 16 positions (both ends, the tile and chunk edges among them): the logits of a position
        # are those of its prefix evaluated as a sequence
        picks = {0, 1, R - 1, R, 1023, 1024}
        for p in np.random.default_rng(6).integers(0, T, 64):
            if len(picks) < 16:
                picks.add(int(p))
        assert len(picks) == 16
        for p in sorted(picks):
            c.fresh()
            lg = c.eval_device(tokens[:p + 1])
            assert abs(losses[p] - cross_entropy(lg, tokens[p + 1])) <= TOL, p
            assert argmax[p] == np.argmax(lg), p
    finally:
        c.free()


def test_continuation_and_sampling_after_score(v6_serial):
    tokens = v6_serial[0]
    a, b = tokens[:40], tokens[40:141]
    c = Ctx(V6)
    try:
        whole = c.score(a + b, tokens[1:142])
        whole_last, whole_state = c.device_logits(), c.state()
        c.fresh()
        la, _, _ = c.score(a, tokens[1:41])
        lb, amax_b, _ = c.score(b, tokens[41:142])
        assert np.array_equal(np.concatenate([la, lb]).view(np.uint64), whole[0].view(np.uint64))
        assert np.array_equal(bits(c.device_logits()), bits(whole_last))
        assert np.array_equal(bits(c.state()), bits(whole_state))
        p = make_sampling(temperature=0.0)
        tok = ctypes.c_uint32(0xffffffff)
        assert c.L.rwkv_mi355x_sample(c.ptr, ctypes.byref(p), ctypes.byref(tok))
        assert tok.value == amax_b[-1] == np.argmax(whole_last)
    finally:
        c.free()


# ---- errors
def raw_score(c, tokens, targets, losses=True):
    T = len(tokens)
    tok = (ctypes.c_uint32 * T)(*tokens)
    tg = (ctypes.c_uint32 * T)(*targets) if targets is not None else None
    out = (ctypes.c_double * T)() if losses else None
    return c.L.rwkv_mi355x_score_sequence(c.ptr, tok, T, tg, out, (ctypes.c_uint32 * T)(), None)


def test_argument_errors_leave_the_state_untouched():
    c = Ctx(V6)
    try:
        c.eval_device(TEXT[:10])
        before = c.state()
        assert not raw_score(c, TEXT[:8], TEXT[1:8] + [c.V])
        assert c.error() == RWKV_ERROR_ARGS
        assert not raw_score(c, TEXT[:8], TEXT[1:9], losses=False)
        assert c.error() == RWKV_ERROR_ARGS
        assert not raw_score(c, TEXT[:8], None, losses=True)
        assert c.error() == RWKV_ERROR_ARGS
        assert not raw_score(c, TEXT[:7] + [c.V], TEXT[1:9])
        assert c.error() == RWKV_ERROR_ARGS
        assert np.array_equal(bits(c.state()), bits(before))
        assert raw_score(c, TEXT[:8], TEXT[1:9]) and c.error() == 0
    finally:
        c.free()


def test_pipeline_and_headless_stage_contexts_are_refused():
    L = library().library
    devs = (ctypes.c_int * 2)(0, 0)
    pipe = L.rwkv_mi355x_init_pipeline(V6.encode(), 1, 2, devs)
    assert pipe
    stage = L.rwkv_mi355x_init_from_file_layers(V6.encode(), 1, 0, L.rwkv_get_n_layer(pipe) - 1)
    assert stage
    try:
        for ptr in (pipe, stage):
            c = Ctx(ptr=ptr)
            assert not raw_score(c, TEXT[:8], TEXT[1:9])
            assert c.error() == RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED
    finally:
        L.rwkv_free(stage)
        L.rwkv_free(pipe)


# ---- a quantised head: the library's quantiser leaves head.weight alone, the loader takes files that
# do not.  The head has no sequence-GEMM tile records, so its rows must go through the decode forms.
def q8_0_blocks(w):
    """Q8_0 (fp16 scale + 32 int8 per block) of a float32 matrix, row-major."""
    x = np.ascontiguousarray(w, np.float32).reshape(-1, 32)
    d = (np.abs(x).max(axis=1) / 127.0).astype(np.float16)
    inv = np.where(d > 0, 1.0 / np.maximum(d.astype(np.float32), 1e-30), 0.0).astype(np.float32)
    q = np.clip(np.rint(x * inv[:, None]), -127, 127).astype(np.int8)
    rec = np.zeros(len(x), np.dtype([('d', '<f2'), ('q', 'i1', 32)]))
    rec['d'], rec['q'] = d, q
    return rec.tobytes()


def test_quantised_head(tmp_path):
    header, tensors = convert.read_model_file(os.path.join(GOLD, 'tiny-rwkv-4v0-660K-FP32.bin'))
    p = str(tmp_path / 'q8-head.bin')
    with open(p, 'wb') as f:
        f.write(struct.pack('=iiiiii', *header))
        for key, t in tensors:
            if key == 'head.weight':
                k = key.encode()
                f.write(struct.pack('=iii', 2, len(k), 9) + struct.pack('=ii', *reversed(t.shape)) + k + q8_0_blocks(t))
            else:
                f.write(convert.tensor_record(key, t))
    c = Ctx(p)
    try:
        tokens = [t % c.V for t in TEXT[:40]]
        targets = tokens[1:] + [0]
        ref_logits, ref_state, _ = c.serial(tokens)
        c.fresh()
        check_against_logits(c.score(tokens, targets, want_logits=True), ref_logits, targets)
        assert np.array_equal(bits(c.state()), bits(ref_state))
    finally:
        c.free()
