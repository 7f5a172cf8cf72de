"""rwkv_mi355x_generate_speculative (include/rwkv_mi355x.h): the tokens, the state and the
logits of rwkv_mi355x_generate, bit for bit, whatever the history offers as drafts."""
import ctypes
import os

import numpy as np
import pytest

from rwkv_lib import RWKVModel, library
from rwkv_cpp.rwkv_cpp_shared_library import RWKVSpeculation, make_sampling

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
P_F, P_U = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
RWKV_ERROR_ARGS, RWKV_ERROR_CTX, RWKV_ERROR_UNSUPPORTED = 1 << 8, 6 << 8, 9
FIXTURES = ['tiny-rwkv-4v0-660K-FP16.bin', 'tiny-rwkv-5v1-730K-FP16.bin', 'tiny-rwkv-5v2-730K-FP16.bin',
            'tiny-rwkv-6v0-3m-Q5_1.bin', 'tiny-rwkv-7v0-834K-FP16.bin']
SYNTH = [(arch, fmt) for arch in (4, 5, 6, 7) for fmt in ('Q4_0', 'FP16')]  # head size 64, k_wkv4_seq
SAMPLING = [dict(temperature=0.0), dict(temperature=1.0, top_p=0.8, seed=1234, offset=77)]
PROMPT = list(b'This is a port of [B')
N = 40


@pytest.fixture(scope='module', params=FIXTURES + SYNTH, ids=str)
def model_path(request, tmp_path_factory):
    if isinstance(request.param, str):
        return os.path.join(GOLD, request.param)
    arch, fmt = request.param
    p = str(tmp_path_factory.mktemp('spec') / f'v{arch}-{fmt}.bin')
    assert library().library.rwkv_mi355x_write_synthetic_model(p.encode(), arch, 256, 128, 2, 0, fmt.encode(), 3)
    return p


class Ctx:
    def __init__(self, path):
        self.lib, self.L = library(), library().library
        self.ctx = self.lib.rwkv_init_from_file(path, 1, 99)
        self.V = self.L.rwkv_get_n_vocab(self.ctx.ptr)
        self.prompt = [t % self.V for t in PROMPT]

    def start(self):
        arr = (ctypes.c_int32 * len(self.prompt))(*self.prompt)
        assert self.L.rwkv_mi355x_state_upload(self.ctx.ptr, None)
        assert self.L.rwkv_mi355x_eval_device(self.ctx.ptr, arr, len(self.prompt), True, None, True)

    def run(self, call, *args, **kw):
        """(tokens[, stats], state bits, logits bits) of one generation call from the prompt."""
        self.start()
        return self.more(call, *args, **kw)

    def more(self, call, *args, **kw):
        lg = np.zeros(self.V, np.float32)
        out = call(self.ctx, *args, logits_out_address=lg.ctypes.data, **kw)
        st = np.zeros(self.L.rwkv_get_state_len(self.ctx.ptr), np.float32)
        assert self.L.rwkv_mi355x_state_download(self.ctx.ptr, st.ctypes.data_as(P_F))
        return out, st.view(np.uint32), lg.view(np.uint32)


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize('kw', SAMPLING, ids=['greedy', 'sampled'])
def test_identity_with_generate(model_path, kw):
    c = Ctx(model_path)
    try:
        spec = c.lib.rwkv_mi355x_generate_speculative
        want = c.run(c.lib.rwkv_mi355x_generate, N, **kw)
        G = want[0]
        wrong = [(t + 1) % c.V if j % 7 == 3 else t for j, t in enumerate(G)]
        for name, history, k in (('prompt', c.prompt, 4), ('perfect', c.prompt + G, 15), ('flawed', c.prompt + wrong, 4)):
            (toks, st), state, logits = c.run(spec, N, history=history, draft_len=k, **kw)
            print(name, st)
            assert same((toks, state, logits), want), name
            assert st['steps'] + st['accepted'] == N
            if name == 'perfect':  # 16-row passes, trace entry 15
                assert st['steps'] < N
            if name == 'flawed':  # rejections at the first, middle and last rows
                assert 0 < st['accepted'] < st['drafted']
        # two calls continue the stream as one does
        off = kw.get('offset', 0)
        (a, _), _, _ = c.run(spec, N // 2, history=c.prompt + G, **kw)
        (b, _), state, logits = c.more(spec, N // 2, history=c.prompt + G, **dict(kw, offset=off + N // 2))
        assert same((a + b, state, logits), want)
    finally:
        c.lib.rwkv_free(c.ctx)


def test_python_model_interface():
    lib = library()
    model = RWKVModel(lib, os.path.join(GOLD, FIXTURES[3]), gpu_layer_count=99)
    try:
        model.eval_sequence(PROMPT, None, use_numpy=True)
        want = model.generate(12, temperature=0.0, block=12)
        model.eval_sequence(PROMPT, None, use_numpy=True)
        toks, st = model.generate_speculative(12, history=PROMPT + want, temperature=0.0)
        assert toks == want and st['steps'] + st['accepted'] == 12 and st['accepted'] > 0
    finally:
        model.free()


BAD = {'draft_len_0': dict(draft_len=0), 'draft_len_16': dict(draft_len=16), 'ngram_min_0': dict(ngram_min=0),
       'min_above_max': dict(ngram_min=3, ngram_max=2), 'ngram_max_9': dict(ngram_max=9), 'history_token': dict(history=[1, 1 << 20]),
       'too_long': dict(history=[1] * ((1 << 20) - 3)), 'no_logits': dict(no_logits=True)}


@pytest.mark.parametrize('name', BAD)
def test_argument_errors(name):
    c = Ctx(os.path.join(GOLD, FIXTURES[3]))
    try:
        c.start()
        want = c.more(c.lib.rwkv_mi355x_generate, 4, temperature=0.0)
        bad = dict(BAD[name])
        if bad.pop('no_logits', False):  # a step without the head
            arr = (ctypes.c_int32 * 1)(5)
            assert c.L.rwkv_mi355x_eval_device(c.ctx.ptr, arr, 1, False, None, True)
        else:
            c.start()
        hist = np.asarray(bad.pop('history', []), np.uint32)
        s = RWKVSpeculation(**dict(dict(draft_len=4, ngram_min=1, ngram_max=4), **bad), history=hist.ctypes.data_as(P_U),
                            n_history=hist.size)
        toks, p = (ctypes.c_uint32 * 4)(), make_sampling(temperature=0.0)
        assert not c.L.rwkv_mi355x_generate_speculative(c.ctx.ptr, ctypes.byref(p), ctypes.byref(s), 4, toks, None, None)
        assert c.L.rwkv_get_last_error(c.ctx.ptr) == RWKV_ERROR_ARGS
        assert same(c.run(c.lib.rwkv_mi355x_generate, 4, temperature=0.0), want)  # still usable
    finally:
        c.lib.rwkv_free(c.ctx)


def test_pipeline_context_is_refused():
    L = library().library
    pipe = L.rwkv_mi355x_init_pipeline(os.path.join(GOLD, FIXTURES[3]).encode(), 1, 2, (ctypes.c_int * 2)(0, 0))
    assert pipe
    try:
        s, p, toks = RWKVSpeculation(4, 1, 4, None, 0), make_sampling(temperature=0.0), (ctypes.c_uint32 * 4)()
        assert not L.rwkv_mi355x_generate_speculative(pipe, ctypes.byref(p), ctypes.byref(s), 4, toks, None, None)
        assert L.rwkv_get_last_error(pipe) == RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED
        lg, st = np.zeros(L.rwkv_get_n_vocab(pipe), np.float32), np.zeros(L.rwkv_get_state_len(pipe), np.float32)
        assert L.rwkv_eval(pipe, 5, None, st.ctypes.data_as(P_F), lg.ctypes.data_as(P_F))  # still usable
    finally:
        L.rwkv_free(pipe)
