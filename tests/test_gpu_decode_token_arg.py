"""A one-token step's id travels by value in the argument block of the step's first launch (TokArg:
k_v6_maa_dec4 EMB, k_v4_att_fused EMB, k_embed_ln); a graph replay with another id updates that one
kernel node (Engine::TokGraph::set_tok) and nothing is enqueued between two replays to deliver it.
Generation keeps reading the word the sampler wrote on the device.

Everything here compares bit for bit: against oracle_ctypes.gpu_variant (the GPU-association oracle,
one serial step after the other) and against rwkv_eval_sequence over the same prefix.

A stale argument block would show as the logits and state of another token: the sequences repeat
ids (A, B, A), include ids 0 and n_vocab - 1, and run long enough that both state parities and both
graph flavours (logits on / off) are replayed with a changed id -- with the steps synchronised one
by one, and enqueued without waiting in between (an update must not reach a replay already queued).
"""
import ctypes
import os

import numpy as np
import pytest
import torch  # noqa: F401  before librwkv initialises HIP (torch's own HIP runtime must come up first)

from oracle_ctypes import assert_bits_equal, gpu_variant
from rwkv_lib import library
from rwkv_cpp.rwkv_cpp_shared_library import make_sampling

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
P_F = ctypes.POINTER(ctypes.c_float)
TINY = {4: 'tiny-rwkv-4v0-660K-FP16.bin', 5: 'tiny-rwkv-5v2-730K-FP16.bin', 6: 'tiny-rwkv-6v0-3m-Q5_1.bin',
        7: 'tiny-rwkv-7v0-834K-FP16.bin'}
# Engine::FUSE_*: the defaults (v4 adds FUSE_FFNCO) and the same without FUSE_EMBMAA (512)
FUSE = {4: (959, 447), 6: (831, 319)}

_refs = {}


class Ctx:
    def __init__(self, path, knobs=None, clone_of=None):
        self.L = library().library
        self.ptr = self.L.rwkv_clone_context(clone_of.ptr, 1) if clone_of else self.L.rwkv_init_from_file(path.encode(), 1, 99)
        assert self.ptr
        for k, v in (knobs or {}).items():
            assert self.L.rwkv_mi355x_debug_set(self.ptr, k.encode(), v)
        self.V = self.L.rwkv_get_n_vocab(self.ptr)
        self.n_state = self.L.rwkv_get_state_len(self.ptr)

    def free(self):
        self.L.rwkv_free(self.ptr)

    def reset(self):
        assert self.L.rwkv_mi355x_state_upload(self.ptr, None)

    def step(self, tokens, logits=True, sync=True):
        """rwkv_mi355x_eval_device on the device-resident state; returns the logits (or None)."""
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        lg = np.zeros(self.V, np.float32) if logits and sync else None
        assert self.L.rwkv_mi355x_eval_device(self.ptr, arr, len(tokens), logits, lg.ctypes.data_as(P_F) if lg is not None else None, sync)
        return lg

    def sync(self):
        assert self.L.rwkv_mi355x_sync(self.ptr)

    def state(self):
        st = np.zeros(self.n_state, np.float32)
        assert self.L.rwkv_mi355x_state_download(self.ptr, st.ctypes.data_as(P_F))
        return st

    def sequence(self, tokens):
        """rwkv_eval_sequence from the fresh state: (logits, state)."""
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        st, lg = np.zeros(self.n_state, np.float32), np.zeros(self.V, np.float32)
        assert self.L.rwkv_eval_sequence(self.ptr, arr, len(tokens), None, st.ctypes.data_as(P_F), lg.ctypes.data_as(P_F))
        return lg, st

    def generate(self, n):
        p = make_sampling(temperature=0.0)
        toks = (ctypes.c_uint32 * n)()
        assert self.L.rwkv_mi355x_generate(self.ptr, ctypes.byref(p), n, toks, None)
        return list(toks)


def serial_reference(path, tokens):
    """[(logits, state) after token i] of the GPU-association oracle, each step from the previous
    step's state; computed once per (model, tokens) and shared."""
    key = (path, tuple(tokens))
    if key not in _refs:
        out, st = [], None
        for t in tokens:
            lg, st = gpu_variant(path, [t], state_in=st)
            out.append((lg.copy(), st.copy()))
        _refs[key] = out
    return _refs[key]


def stale_tokens(V):
    a, b = 34 % V, 105 % V
    return [a, b, a, 0, V - 1, a, b]


def check_stale(path, knobs, what):
    c = Ctx(path, knobs)
    try:
        toks = stale_tokens(c.V)
        ref = serial_reference(path, toks)
        # every step with logits, synchronised: logits and state after each, also against
        # rwkv_eval_sequence over the same prefix
        c.reset()
        got = []
        for i, t in enumerate(toks):
            lg = c.step([t])
            got.append((lg, c.state()))
        for i in range(len(toks)):
            assert_bits_equal(got[i][0], ref[i][0], f'{what}: logits after step {i} vs the oracle')
            assert_bits_equal(got[i][1], ref[i][1], f'{what}: state after step {i} vs the oracle')
            slg, sst = c.sequence(toks[:i + 1])
            assert_bits_equal(got[i][0], slg, f'{what}: logits after step {i} vs rwkv_eval_sequence')
            assert_bits_equal(got[i][1], sst, f'{what}: state after step {i} vs rwkv_eval_sequence')
        # the graphs without logits at both parities, each replayed with changed ids
        c.reset()
        for i, t in enumerate(toks):
            c.step([t], logits=False)
            assert_bits_equal(c.state(), ref[i][1], f'{what}: state after step {i} without logits')
        # nothing waited for between the steps
        c.reset()
        for t in toks[:-1]:
            c.step([t], logits=False, sync=False)
        lg = c.step(toks[-1:])
        assert_bits_equal(lg, ref[-1][0], f'{what}: logits after the steps enqueued without waiting')
        assert_bits_equal(c.state(), ref[-1][1], f'{what}: state after the steps enqueued without waiting')
    finally:
        c.free()


@pytest.fixture(scope='module')
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp('decode_token_arg')


def synthetic(model_dir, arch, C, layers, fmt='Q4_0', vocab=4096):
    p = os.path.join(str(model_dir), f'v{arch}-{C}-{layers}-{fmt}.bin')
    if not os.path.isfile(p):
        assert library().library.rwkv_mi355x_write_synthetic_model(p.encode(), arch, vocab, C, layers, 0, fmt.encode(), 29)
    return p


@pytest.mark.parametrize('arch', [4, 5, 6, 7])
def test_stale_argument_tiny_fixtures(arch):
    check_stale(os.path.join(GOLD, TINY[arch]), None, f'v{arch}')


@pytest.mark.parametrize('knobs', [{'decode_fusion': FUSE[6][0]}, {'decode_fusion': FUSE[6][1]}, {'decode_fusion': 511},
                                   {'graphs': 0}, {'generic_decode': 1}],
                         ids=['emb', 'no_emb', 'fusion511', 'no_graphs', 'generic_decode'])
def test_stale_argument_v6_arms(knobs):
    check_stale(os.path.join(GOLD, TINY[6]), knobs, f'v6 {knobs}')


@pytest.mark.parametrize('knobs', [{'decode_fusion': FUSE[4][0]}, {'decode_fusion': FUSE[4][1]}, {'graphs': 0}],
                         ids=['emb', 'no_emb', 'no_graphs'])
def test_stale_argument_v4_arms(knobs):
    check_stale(os.path.join(GOLD, TINY[4]), knobs, f'v4 {knobs}')


@pytest.mark.parametrize('fusion', [FUSE[6][0], FUSE[6][1]], ids=['emb', 'no_emb'])
@pytest.mark.parametrize('co_mode', [0, 1])
def test_stale_argument_v6_layouts(model_dir, co_mode, fusion):
    # C = 512: the smallest width of the co-resident layout (co_mode 1 forces it)
    check_stale(synthetic(model_dir, 6, 512, 2), {'co_mode': co_mode, 'decode_fusion': fusion},
                f'v6 C=512 co_mode {co_mode} fusion {fusion}')


@pytest.mark.parametrize('co_mode', [0, 1])
def test_stale_argument_v4_layouts(model_dir, co_mode):
    check_stale(synthetic(model_dir, 4, 512, 2, 'Q8_0'), {'co_mode': co_mode}, f'v4 C=512 co_mode {co_mode}')


@pytest.mark.parametrize('arch,fmt', [(6, 'Q4_0'), (4, 'Q8_0'), (7, 'Q5_1')])
def test_host_state_path(model_dir, arch, fmt):
    """rwkv_eval(ctx, t, s, s, lg): 6 layers run as two chunk graphs (4 layers each), of which only
    the first takes the id."""
    path = synthetic(model_dir, arch, 256, 6, fmt, 512)
    c = Ctx(path)
    try:
        toks = stale_tokens(c.V)
        ref = serial_reference(path, toks)
        st, lg = np.zeros(c.n_state, np.float32), np.zeros(c.V, np.float32)
        c.L.rwkv_init_state(c.ptr, st.ctypes.data_as(P_F))
        for i, t in enumerate(toks):
            assert c.L.rwkv_eval(c.ptr, t, st.ctypes.data_as(P_F), st.ctypes.data_as(P_F), lg.ctypes.data_as(P_F))
            assert_bits_equal(lg, ref[i][0], f'v{arch}: logits after rwkv_eval {i}')
            assert_bits_equal(st, ref[i][1], f'v{arch}: state after rwkv_eval {i}')
        # without logits: the other graph flavour of every chunk
        c.L.rwkv_init_state(c.ptr, st.ctypes.data_as(P_F))
        for i, t in enumerate(toks):
            assert c.L.rwkv_eval(c.ptr, t, st.ctypes.data_as(P_F), st.ctypes.data_as(P_F), None)
            assert_bits_equal(st, ref[i][1], f'v{arch}: state after rwkv_eval {i} without logits')
        slg, sst = c.sequence(toks)
        assert_bits_equal(lg, slg, f'v{arch}: logits vs rwkv_eval_sequence')
        assert_bits_equal(st, sst, f'v{arch}: state vs rwkv_eval_sequence')
    finally:
        c.free()


@pytest.mark.parametrize('arch', [4, 6])
def test_decode_step_after_a_sequence(arch):
    path = os.path.join(GOLD, TINY[arch])
    c = Ctx(path)
    try:
        prompt = [t % c.V for t in b'This is']
        tail = [0, c.V - 1, prompt[0]]
        ref = serial_reference(path, prompt + tail)
        c.reset()
        c.step(prompt)
        for i, t in enumerate(tail):
            lg = c.step([t])
            assert_bits_equal(lg, ref[len(prompt) + i][0], f'v{arch}: logits of decode step {i} after a sequence')
            assert_bits_equal(c.state(), ref[len(prompt) + i][1], f'v{arch}: state of decode step {i} after a sequence')
    finally:
        c.free()


@pytest.mark.parametrize('arch', [4, 6])
def test_host_ids_around_generate(arch):
    """Host-id steps, then generation (every step reads the id the sampler wrote), then host-id steps
    again: the same graphs switch the source of the id back and forth."""
    path = os.path.join(GOLD, TINY[arch])
    c = Ctx(path)
    try:
        a, b = 34 % c.V, 105 % c.V
        c.reset()
        c.step([a])
        c.step([b])
        gen = c.generate(4)
        after = [b, c.V - 1, a]
        for t in after[:-1]:
            c.step([t])
        lg = c.step(after[-1:])
        st = c.state()
        gen2 = c.generate(3)
        st2 = c.state()
        ref = serial_reference(path, [a, b] + gen + after)
        assert int(np.argmax(ref[1][0])) == gen[0], 'the first generated token is the greedy pick'
        assert_bits_equal(lg, ref[-1][0], f'v{arch}: logits of host-id steps after generate')
        assert_bits_equal(st, ref[-1][1], f'v{arch}: state of host-id steps after generate')
        ref2 = serial_reference(path, [a, b] + gen + after + gen2)
        assert int(np.argmax(ref[-1][0])) == gen2[0]
        assert_bits_equal(st2, ref2[-1][1], f'v{arch}: state of a generation after host-id steps')
    finally:
        c.free()


def test_two_clones_alternate(model_dir):
    path = synthetic(model_dir, 6, 512, 2)
    c1 = Ctx(path)
    c2 = Ctx(path, clone_of=c1)
    try:
        t1 = stale_tokens(c1.V)
        t2 = [(t * 7 + 3) % c1.V for t in t1]
        r1, r2 = serial_reference(path, t1), serial_reference(path, t2)
        c1.reset()
        c2.reset()
        for i in range(len(t1)):
            c1.step([t1[i]], logits=True, sync=False)
            c2.step([t2[i]], logits=True, sync=False)
        c1.sync()
        c2.sync()
        assert_bits_equal(c1.state(), r1[-1][1], 'clone 1 state')
        assert_bits_equal(c2.state(), r2[-1][1], 'clone 2 state')
        # one more step each, with logits
        assert_bits_equal(c1.step([t2[0]]), serial_reference(path, t1 + [t2[0]])[-1][0], 'clone 1 logits')
        assert_bits_equal(c2.step([t1[0]]), serial_reference(path, t2 + [t1[0]])[-1][0], 'clone 2 logits')
    finally:
        c2.free()
        c1.free()


# The co-resident attention launch against the ordered one and the oracle at H = 8 (the smallest
# width it accepts), H = 16 (H % 8 != 0 has no co-resident form -- the layout needs C % 512 == 0 -- so
# the nearest width it accepts) and H = 32 (8 H = 256 workgroups: one per compute unit).  The cases a
# regrouping of its workgroups over the XCDs has to keep: one such map (a head's eight workgroups on
# one XCD) was measured slower and is not in the tree.
@pytest.mark.parametrize('C', [512, 1024, 2048])
def test_co_resident_equals_ordered_and_oracle(model_dir, C):
    path = synthetic(model_dir, 6, C, 2)
    toks = [17, 4095, 0, 17]
    ref = serial_reference(path, toks)
    got = {}
    for co_mode in (0, 1):
        c = Ctx(path, {'co_mode': co_mode})
        try:
            c.reset()
            got[co_mode] = []
            for t in toks:
                lg = c.step([t])
                got[co_mode].append((lg, c.state()))
        finally:
            c.free()
    for i in range(len(toks)):
        for co_mode in (0, 1):
            assert_bits_equal(got[co_mode][i][0], ref[i][0], f'C={C} co_mode {co_mode}: logits after step {i}')
            assert_bits_equal(got[co_mode][i][1], ref[i][1], f'C={C} co_mode {co_mode}: state after step {i}')
        assert_bits_equal(got[1][i][0], got[0][i][0], f'C={C}: co-resident vs ordered logits after step {i}')
        assert_bits_equal(got[1][i][1], got[0][i][1], f'C={C}: co-resident vs ordered state after step {i}')
