"""rwkv_mi355x_generate / rwkv_mi355x_sample (include/rwkv_mi355x.h): the generation loop that stays
on the device gives the tokens, the state and the logits of the host loop it replaces --
rwkv_mi355x_eval_device with logits_out, a token chosen on the host, repeat -- bit for bit."""
import ctypes
import os

import numpy as np
import pytest

from rwkv_lib import RWKVModel, library
from rwkv_cpp import sampling
from rwkv_cpp.rwkv_cpp_shared_library import make_sampling

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
P_F = ctypes.POINTER(ctypes.c_float)
P_I = ctypes.POINTER(ctypes.c_int32)
P_U = ctypes.POINTER(ctypes.c_uint32)
RWKV_ERROR_ARGS, RWKV_ERROR_CTX, RWKV_ERROR_UNSUPPORTED = 1 << 8, 6 << 8, 9
FIXTURES = ['tiny-rwkv-4v0-660K-FP16.bin', 'tiny-rwkv-5v2-730K-FP16.bin', 'tiny-rwkv-6v0-3m-Q5_1.bin',
            'tiny-rwkv-7v0-834K-FP16.bin']
V6 = 'tiny-rwkv-6v0-3m-Q5_1.bin'
PROMPT = list(b'This is a port of [B')  # 20 tokens


@pytest.fixture(scope='module')
def world_model(tmp_path_factory):
    p = str(tmp_path_factory.mktemp('generate') / 'world-v6.bin')
    assert library().library.rwkv_mi355x_write_synthetic_model(p.encode(), 6, 65536, 256, 3, 0, b'Q5_1', 11)
    return p


class Ctx:
    def __init__(self, path, knobs=None):
        self.L = library().library
        self.ptr = self.L.rwkv_init_from_file(path.encode(), 1, 99)
        assert self.ptr
        for k, v in (knobs or {}).items():
            assert self.L.rwkv_mi355x_debug_set(self.ptr, k.encode(), v)
        self.V = self.L.rwkv_get_n_vocab(self.ptr)
        self.prompt = [t % self.V for t in PROMPT]

    def free(self):
        self.L.rwkv_free(self.ptr)

    def start(self, logits_out=None):
        """Fresh state, then the prompt with logits."""
        assert self.L.rwkv_mi355x_state_upload(self.ptr, None)
        self.step(self.prompt, logits_out)

    def step(self, tokens, logits_out=None):
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        out = logits_out.ctypes.data_as(P_F) if logits_out is not None else None
        assert self.L.rwkv_mi355x_eval_device(self.ptr, arr, len(tokens), True, out, True)

    def state(self):
        st = np.zeros(self.L.rwkv_get_state_len(self.ptr), np.float32)
        assert self.L.rwkv_mi355x_state_download(self.ptr, st.ctypes.data_as(P_F))
        return st

    def host_loop(self, n, pick):
        """The loop generate replaces; pick(logits, i) chooses token i on the host."""
        lg = np.zeros(self.V, np.float32)
        self.start(lg)
        toks = []
        for i in range(n):
            toks.append(int(pick(lg, i)))
            self.step([toks[-1]], lg)
        return toks, self.state(), lg

    def generate_raw(self, n, logits_out=None, tokens_null=False, **kw):
        p = make_sampling(**kw)
        toks = (ctypes.c_uint32 * max(n, 1))()
        out = logits_out.ctypes.data_as(P_F) if logits_out is not None else None
        ok = self.L.rwkv_mi355x_generate(self.ptr, ctypes.byref(p), n, None if tokens_null else toks, out)
        return ok, list(toks[:n])

    def generate(self, n, logits_out=None, **kw):
        ok, toks = self.generate_raw(n, logits_out, **kw)
        assert ok
        return toks

    def sample(self, **kw):
        p = make_sampling(**kw)
        t = ctypes.c_uint32(0xffffffff)
        assert self.L.rwkv_mi355x_sample(self.ptr, ctypes.byref(p), ctypes.byref(t))
        return t.value

    def error(self):
        return self.L.rwkv_get_last_error(self.ptr)


def bits(a):
    return np.asarray(a).view(np.uint32)


def greedy_pick(lg, i):
    return np.argmax(lg)


def check_greedy(path, knobs=None, n=16):
    c = Ctx(path, knobs)
    try:
        toks, st, lg = c.host_loop(n, greedy_pick)
        c.start()
        glg = np.zeros(c.V, np.float32)
        gen = c.generate(n, glg, temperature=0.0)
        assert gen == toks
        assert np.array_equal(bits(c.state()), bits(st))
        assert np.array_equal(bits(glg), bits(lg))
    finally:
        c.free()


@pytest.mark.parametrize('name', FIXTURES)
def test_greedy_equals_the_host_loop(name):
    check_greedy(os.path.join(GOLD, name))


def test_greedy_equals_the_host_loop_world_vocabulary(world_model):
    check_greedy(world_model)


@pytest.mark.parametrize('knobs', [{'co_mode': 0}, {'co_mode': 1}, {'graphs': 0}, {'generic_decode': 1}],
                         ids=['co_mode0', 'co_mode1', 'no_graphs', 'generic_decode'])
def test_greedy_equals_the_host_loop_in_every_decode_arm(knobs):
    check_greedy(os.path.join(GOLD, V6), knobs)


def test_greedy_with_kernel_timing_on():
    c = Ctx(os.path.join(GOLD, V6))
    try:
        toks, st, _ = c.host_loop(8, greedy_pick)
        c.L.rwkv_mi355x_set_kernel_timing(c.ptr, True)
        c.start()
        assert c.generate(8, temperature=0.0) == toks
        assert np.array_equal(bits(c.state()), bits(st))
        c.L.rwkv_mi355x_set_kernel_timing(c.ptr, False)
    finally:
        c.free()


SAMPLED = dict(temperature=0.8, top_p=0.5, seed=7)


def stepwise_pick(lg, i):
    tok, _, _ = library().rwkv_mi355x_selftest_sample(lg, sampling.uniform(7, i), temperature=0.8, top_p=0.5)
    return tok[0]


@pytest.mark.parametrize('which', FIXTURES + ['world'])
def test_sampled_equals_the_stepwise_loop(which, world_model):
    c = Ctx(world_model if which == 'world' else os.path.join(GOLD, which))
    try:
        toks, st, lg = c.host_loop(24, stepwise_pick)
        c.start()
        glg = np.zeros(c.V, np.float32)
        assert c.generate(24, glg, **SAMPLED) == toks
        assert np.array_equal(bits(c.state()), bits(st))
        assert np.array_equal(bits(glg), bits(lg))
    finally:
        c.free()


def test_continuation_sample_and_state_traffic(world_model):
    c = Ctx(world_model)
    try:
        c.start()
        whole = c.generate(16, **SAMPLED)
        st = c.state()
        c.start()
        io0 = library().rwkv_mi355x_state_io_bytes(c)
        # rwkv_mi355x_sample: the first token of generate, state and logits untouched
        st0 = c.state()
        first = c.sample(**SAMPLED)
        assert first == whole[0] and first == c.sample(**SAMPLED)
        assert c.sample(offset=3, **SAMPLED) == stepwise_offset(c, 3)
        assert np.array_equal(bits(c.state()), bits(st0))
        io1 = library().rwkv_mi355x_state_io_bytes(c)
        a = c.generate(8, **SAMPLED)
        b = c.generate(8, offset=8, **SAMPLED)
        assert a + b == whole
        # no state crosses PCIe in generate (the two downloads above are this test's own)
        assert library().rwkv_mi355x_state_io_bytes(c) == io1
        assert io1[0] == io0[0] and io1[1] == io0[1] + 2 * 4 * len(st0)
        assert np.array_equal(bits(c.state()), bits(st))
    finally:
        c.free()


def stepwise_offset(c, offset):
    lg = np.zeros(c.V, np.float32)
    assert c.L.rwkv_mi355x_debug_buffer(c.ptr, b'logits', lg.ctypes.data_as(ctypes.c_void_p), lg.nbytes) == lg.nbytes
    tok, _, _ = library().rwkv_mi355x_selftest_sample(lg, sampling.uniform(7, offset), temperature=0.8, top_p=0.5)
    return int(tok[0])


def test_model_generate_blocks_and_stop_tokens():
    path = os.path.join(GOLD, V6)
    m = RWKVModel(library(), path)
    L = library().library
    prompt = PROMPT

    def state():
        st = np.zeros(L.rwkv_get_state_len(m._ctx.ptr), np.float32)
        assert L.rwkv_mi355x_state_download(m._ctx.ptr, st.ctypes.data_as(P_F))
        return st

    try:
        m.eval_sequence(prompt, None, use_numpy=True)
        stream = m.generate(16, temperature=0.0)
        assert len(stream) == 16
        stop = stream[5]
        cut = stream[:stream.index(stop) + 1]
        m.eval_sequence(prompt, None, use_numpy=True)
        assert m.sample(temperature=0.0) == stream[0]
        assert m.generate(16, temperature=0.0, stop_tokens=[stop], block=1) == cut
        exact = state()
        # the stepwise state after the prompt and the tokens up to the stop token
        _, st = m.eval_sequence(prompt, None, use_numpy=True)
        for t in cut:
            _, st = m.eval(t, st, st, None, use_numpy=True)
        assert np.array_equal(bits(exact), bits(st))
        m.eval_sequence(prompt, None, use_numpy=True)
        assert m.generate(16, temperature=0.0, stop_tokens=[stop], block=16) == cut
        m.eval_sequence(prompt, None, use_numpy=True)
        assert m.generate(16, temperature=0.0, block=5) == stream
    finally:
        m.free()


def test_argument_errors_leave_the_context_usable():
    c = Ctx(os.path.join(GOLD, V6))
    try:
        c.start()
        want = c.generate(4, temperature=0.0)
        c.start()
        for n, kw in ((4, dict(temperature=-1.0)), (4, dict(temperature=float('nan'))), (4, dict(top_p=1.5)),
                      (4, dict(logit_bias={c.V: 1.0})), (0, {}), (65537, {})):
            ok, _ = c.generate_raw(n, **kw)
            assert not ok and c.error() == RWKV_ERROR_ARGS, (n, kw)
        ok, _ = c.generate_raw(4, tokens_null=True)
        assert not ok and c.error() == RWKV_ERROR_ARGS
        assert not c.L.rwkv_mi355x_generate(c.ptr, None, 4, (ctypes.c_uint32 * 4)(), None)
        assert c.error() == RWKV_ERROR_ARGS
        p = make_sampling(logit_bias={i: 0.0 for i in range(257)})
        assert not c.L.rwkv_mi355x_sample(c.ptr, ctypes.byref(p), ctypes.byref(ctypes.c_uint32()))
        assert c.error() == RWKV_ERROR_ARGS
        # none of the refused calls touched the state or the logits
        assert c.generate(4, temperature=0.0) == want
        # the logits do not follow an uploaded state
        assert c.L.rwkv_mi355x_state_upload(c.ptr, None)
        ok, _ = c.generate_raw(4, temperature=0.0)
        assert not ok and c.error() == RWKV_ERROR_ARGS
        c.step(c.prompt)
        assert c.generate(4, temperature=0.0) == want
        # nor an evaluation that did not run the head
        arr = (ctypes.c_int32 * 1)(want[0])
        c.start()
        assert c.L.rwkv_mi355x_eval_device(c.ptr, arr, 1, False, None, True)
        ok, _ = c.generate_raw(4, temperature=0.0)
        assert not ok and c.error() == RWKV_ERROR_ARGS
    finally:
        c.free()


def test_pipeline_context_is_refused():
    L = library().library
    devs = (ctypes.c_int * 2)(0, 0)
    pipe = L.rwkv_mi355x_init_pipeline(os.path.join(GOLD, V6).encode(), 1, 2, devs)
    assert pipe
    try:
        p = make_sampling(temperature=0.0)
        toks = (ctypes.c_uint32 * 4)()
        assert not L.rwkv_mi355x_generate(pipe, ctypes.byref(p), 4, toks, None)
        assert L.rwkv_get_last_error(pipe) == RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED
        assert not L.rwkv_mi355x_sample(pipe, ctypes.byref(p), toks)
        assert L.rwkv_get_last_error(pipe) == RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED
        # still usable
        lg = np.zeros(L.rwkv_get_n_vocab(pipe), np.float32)
        st = np.zeros(L.rwkv_get_state_len(pipe), np.float32)
        assert L.rwkv_eval(pipe, 5, None, st.ctypes.data_as(P_F), lg.ctypes.data_as(P_F))
    finally:
        L.rwkv_free(pipe)
