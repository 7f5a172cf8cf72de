"""The v6 attention reducer publishes y before the decay tail and the state update (mv_att6.hpp
att6_reduce, both layouts): every bit of logits and state stays what the oracle computes.

A wrong ordering shows first in the state and in the logits only one token later, so the decode is
compared after EVERY token: 6 tokens through rwkv_eval (three at each state parity), logits and the
full state against oracle_ctypes.gpu_variant on the same prefix, bit for bit, in the ordered layout
(co_mode 0) and the co-resident one (co_mode 1); the final pair also against one eval_sequence of
the 6 tokens.  Afterwards every hand-off granule reads zero (each was cleared by its reader).  The
same tokens through rwkv_mi355x_eval_device without an intermediate sync give the same final bits:
a late state store racing the next token's launch would show there.

Shapes: arch 6, V = 1024, 2 layers; C = 512 (8 heads, the smallest width the co-resident layout
takes) and C = 1024; Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 cover the WF and WD instantiations.  The synthetic
writer accepts both widths.
"""
import ctypes
import os

import numpy as np
import pytest
import torch  # noqa: F401  before librwkv initialises HIP (torch's own HIP runtime must come up first)

from oracle_ctypes import assert_bits_equal, gpu_variant
from rwkv_lib import RWKVModel, library

pytestmark = pytest.mark.gpu

VOCAB = 1024
LAYERS = 2
WIDTHS = [512, 1024]
FORMATS = ['Q4_0', 'Q4_1', 'Q5_0', 'Q5_1', 'Q8_0']
TOKENS = [int(t) for t in np.random.default_rng(61).integers(0, VOCAB, 6)]
P_F = ctypes.POINTER(ctypes.c_float)

_refs = {}


@pytest.fixture(scope='module')
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp('att6_output_first')


def model_path(model_dir, C, fmt):
    p = os.path.join(str(model_dir), f'v6-{C}-{fmt}.bin')
    if not os.path.isfile(p):
        assert library().library.rwkv_mi355x_write_synthetic_model(p.encode(), 6, VOCAB, C, LAYERS, 0, fmt.encode(), 37)
    return p


def reference(path):
    """[(logits, state) after token i] of the oracle's GPU-association variant: gpu_variant of each
    one-token step from the previous step's state, which is gpu_variant on the prefix (its serial
    form is this chain).  Computed once per model and shared."""
    if path not in _refs:
        out, st = [], None
        for t in TOKENS:
            lg, st = gpu_variant(path, [t], state_in=st)
            out.append((lg.copy(), st.copy()))
        _refs[path] = out
    return _refs[path]


def assert_granules_cleared(m, C):
    gran = np.ones(6 * C, np.uint64)  # r, k, v, g rows + one decay-LoRA copy per head
    n = library().library.rwkv_mi355x_debug_buffer(m._ctx.ptr, b'granules', gran.ctypes.data_as(ctypes.c_void_p),
                                                   gran.nbytes)
    assert n == gran.nbytes
    assert not gran.any(), f'hand-off granules not cleared: {np.nonzero(gran)[0][:8]}'


@pytest.mark.parametrize('co_mode', [0, 1])
@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('C', WIDTHS)
def test_every_token_bit_exact(model_dir, C, fmt, co_mode):
    path = model_path(model_dir, C, fmt)
    ref = reference(path)
    L = library()
    m = RWKVModel(L, path)
    assert L.library.rwkv_mi355x_debug_set(m._ctx.ptr, b'co_mode', co_mode)
    lg, st = None, None
    for i, t in enumerate(TOKENS):
        lg, st = m.eval(t, st, None, None, use_numpy=True)
        assert_bits_equal(lg, ref[i][0], f'C={C} {fmt} co_mode {co_mode}: logits after token {i}')
        assert_bits_equal(st, ref[i][1], f'C={C} {fmt} co_mode {co_mode}: state after token {i}')
    assert_granules_cleared(m, C)
    slg, sst = m.eval_sequence(TOKENS, None, use_numpy=True)
    assert_bits_equal(lg, slg, f'C={C} {fmt} co_mode {co_mode}: decode vs sequence logits')
    assert_bits_equal(st, sst, f'C={C} {fmt} co_mode {co_mode}: decode vs sequence state')
    m.free()


@pytest.mark.parametrize('co_mode', [0, 1])
@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('C', WIDTHS)
def test_device_resident_no_intermediate_sync(model_dir, C, fmt, co_mode):
    path = model_path(model_dir, C, fmt)
    ref_lg, ref_st = reference(path)[-1]
    L = library()
    lib = L.library
    m = RWKVModel(L, path)
    ptr = m._ctx.ptr
    assert lib.rwkv_mi355x_debug_set(ptr, b'co_mode', co_mode)
    assert lib.rwkv_mi355x_state_upload(ptr, None)
    for t in TOKENS[:-1]:
        assert lib.rwkv_mi355x_eval_device(ptr, (ctypes.c_int32 * 1)(t), 1, False, None, False)
    lg = np.zeros(VOCAB, np.float32)
    assert lib.rwkv_mi355x_eval_device(ptr, (ctypes.c_int32 * 1)(TOKENS[-1]), 1, True, lg.ctypes.data_as(P_F), True)
    st = np.zeros(m._state_buffer_element_count, np.float32)
    assert lib.rwkv_mi355x_state_download(ptr, st.ctypes.data_as(P_F))
    assert_bits_equal(lg, ref_lg, f'C={C} {fmt} co_mode {co_mode}: device-resident logits')
    assert_bits_equal(st, ref_st, f'C={C} {fmt} co_mode {co_mode}: device-resident state')
    assert_granules_cleared(m, C)
    m.free()
