"""The engine's launch table, pinned against a recording (tests/golden/decode_program.json).

With kernel timing on (rwkv_mi355x_set_kernel_timing) the engine runs eagerly and
rwkv_mi355x_kernel_stats returns, per kernel class in order of first launch, the number of launches
and the algorithmic bytes and flops the host computed for them.  All of that is host arithmetic on
the model's shapes, so it is deterministic: the table says which kernels a program enqueues, how
often, in which order they first appear and with which roofline formula -- what the bit-exactness
tests cannot see (two programs of the same bits may differ in launches).

Cases, per BASELINE configuration (test_gpu_configs.CONFIGS at 2 layers, V = 4096):
  decode    4 tokens through rwkv_mi355x_eval_device (both state parities twice) under
            decode_fusion -1 (the model's default), 0, 1023 and 127, each with co_mode 0 and 1;
            v6 also on a context created with RWKV_MI355X_SPLIT_MAA=1
  batched   one rwkv_mi355x_eval_batch step at B = 2 and B = 16 (the two sides of the batched GEMM
            threshold)
  sequence  one evaluation at T = 2 and T = 33 (the two sides of the 32-token float-matmul threshold)
  prefill   one rwkv_mi355x_prefill_batch of rows of 1, 2 and 33 tokens at the default packing cap, and
            one of rows of 1 and 3 tokens with the debug knob prefill_chunk = 1 (one-token chunks)
  score     one rwkv_mi355x_score_sequence with targets at T = 1 (the decode step and k_xent), 34 (one
            head tile) and 130 (two head tiles, 128 + 2 rows)

Names, their order and the launch counts must match exactly; bytes and flops to a relative 1e-9
(the order of additions in a formula may change, nothing else).  tools/record_decode_program.py
writes the recording with collect() below.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch  # noqa: F401  before librwkv initialises HIP (torch's own HIP runtime must come up first)

from rwkv_lib import RWKVModel, library
from test_gpu_configs import CONFIGS, LAYERS, VOCAB

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(__file__), 'golden', 'decode_program.json')
MASKS = (-1, 0, 1023, 127)
DECODE_TOKENS = (17, 4000, 321, 9)
BATCHES = (2, 16)
SEQ_LENS = (2, 33)
PREFILL_ROWS = (1, 2, 33)
PREFILL_ROWS_1 = (1, 3)
SCORE_LENS = (1, 34, 130)


def model_file(model_dir, name):
    arch, C, F, fmt = CONFIGS[name]
    p = os.path.join(str(model_dir), f'{name}-L{LAYERS}.bin')
    if not os.path.isfile(p):
        assert library().library.rwkv_mi355x_write_synthetic_model(p.encode(), arch, VOCAB, C, LAYERS, F,
                                                                   fmt.encode(), 21)
    return p


def read_table(lib, ptr):
    """[[name, launches, total_bytes, total_flops], ...] in order of first launch."""
    n = lib.rwkv_mi355x_kernel_stats(ptr, -1, None, 0, None, None, None, None)
    rows = []
    for i in range(n):
        name = ctypes.create_string_buffer(128)
        la, ms, by, fl = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        lib.rwkv_mi355x_kernel_stats(ptr, i, name, 128, ctypes.byref(la), ctypes.byref(ms), ctypes.byref(by),
                                     ctypes.byref(fl))
        rows.append([name.value.decode(), la.value, by.value, fl.value])
    return rows


def timed(lib, ptr, run):
    lib.rwkv_mi355x_set_kernel_timing(ptr, True)  # clears the table
    try:
        run()
        return read_table(lib, ptr)
    finally:
        lib.rwkv_mi355x_set_kernel_timing(ptr, False)


def decode_cases(lib, m, prefix):
    ptr = m._ctx.ptr

    def run():
        for t in DECODE_TOKENS:
            arr = (ctypes.c_int32 * 1)(t)
            assert lib.rwkv_mi355x_eval_device(ptr, arr, 1, True, None, True)

    out = {}
    for mask in MASKS:
        for co in (0, 1):
            assert lib.rwkv_mi355x_debug_set(ptr, b'decode_fusion', mask)
            assert lib.rwkv_mi355x_debug_set(ptr, b'co_mode', co)
            assert lib.rwkv_mi355x_state_upload(ptr, None)
            out[f'{prefix} fusion={mask} co={co}'] = timed(lib, ptr, run)
    assert lib.rwkv_mi355x_debug_set(ptr, b'decode_fusion', -1)
    assert lib.rwkv_mi355x_debug_set(ptr, b'co_mode', -1)
    return out


def collect(name, model_dir):
    """Every case's table for one configuration: {case: rows}."""
    L = library()
    lib = L.library
    path = model_file(model_dir, name)
    m = RWKVModel(L, path)
    ptr = m._ctx.ptr
    out = decode_cases(lib, m, 'decode')
    rng = np.random.default_rng(5)
    for B in BATCHES:
        toks = [int(t) for t in rng.integers(0, VOCAB, B)]
        out[f'batch B={B}'] = timed(lib, ptr, lambda: m.eval_batch(toks, None))
    for T in SEQ_LENS:
        arr = (ctypes.c_int32 * T)(*[int(t) for t in rng.integers(0, VOCAB, T)])
        assert lib.rwkv_mi355x_state_upload(ptr, None)

        def run():
            assert lib.rwkv_mi355x_eval_device(ptr, arr, T, True, None, True)

        out[f'sequence T={T}'] = timed(lib, ptr, run)
    m.batch_reserve(len(PREFILL_ROWS))
    for rows, chunk in ((PREFILL_ROWS, 0), (PREFILL_ROWS_1, 1)):
        prompts = [[int(t) for t in rng.integers(0, VOCAB, n)] for n in rows]
        assert lib.rwkv_mi355x_debug_set(ptr, b'prefill_chunk', chunk)
        try:
            out[f'prefill rows={rows} chunk={chunk}'] = timed(lib, ptr, lambda: m.prefill_batch(prompts))
        finally:
            assert lib.rwkv_mi355x_debug_set(ptr, b'prefill_chunk', 0)
    for T in SCORE_LENS:
        toks = [int(t) for t in rng.integers(0, VOCAB, T)]
        targets = [int(t) for t in rng.integers(0, VOCAB, T)]
        m.reset_state()
        out[f'score T={T}'] = timed(lib, ptr, lambda: m.score(toks, targets))
    m.free()
    if CONFIGS[name][0] == 6:
        os.environ['RWKV_MI355X_SPLIT_MAA'] = '1'
        try:
            m = RWKVModel(L, path)
        finally:
            os.environ.pop('RWKV_MI355X_SPLIT_MAA', None)
        out.update(decode_cases(lib, m, 'decode split_maa'))
        m.free()
    return out


@pytest.fixture(scope='module')
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp('decode_program')


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_launch_table_matches_recording(model_dir, name):
    with open(GOLDEN_FILE) as f:
        want = json.load(f)['tables'][name]
    got = collect(name, model_dir)
    assert sorted(got) == sorted(want), 'the set of cases changed: record again only with the cases of the docstring'
    for case in want:
        w, g = want[case], got[case]
        assert [(r[0], r[1]) for r in g] == [(r[0], r[1]) for r in w], f'{name}, {case}: kernels / order / launches'
        assert any(r[1] > 0 for r in g), f'{name}, {case}: nothing recorded'
        for rg, rw in zip(g, w):
            for k, what in ((2, 'bytes'), (3, 'flops')):
                assert abs(rg[k] - rw[k]) <= 1e-9 * abs(rw[k]), f'{name}, {case}, {rg[0]}: {what} {rg[k]!r} != {rw[k]!r}'
