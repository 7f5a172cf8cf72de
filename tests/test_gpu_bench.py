"""bench.py's plain run: the headline line alone, and --dump-outputs writing what the last timed step
left -- the logits and the recurrent state of the device-resident decode -- from seeded tokens, so
that two builds can be compared output for output."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before librwkv initialises HIP)

from oracle_ctypes import assert_bits_equal
from rwkv_lib import library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_F = ctypes.POINTER(ctypes.c_float)
P_INT = ctypes.POINTER(ctypes.c_int32)
STEPS, WARMUP = 3, 2


def test_roofline_only_needs_full():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--roofline-only'], capture_output=True, text=True)
    assert r.returncode == 2 and '--full' in r.stderr


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup',
                        str(WARMUP), '--config', 'v4-169m-q8_0', '--model-dir', str(tmp_path), '--dump-outputs', str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line['steps'] == STEPS and line['warmup'] == WARMUP and line['unit'] == 'tokens/s' and line['higher_is_better']
    assert line['ms_per_step'] > 0 and abs(line['value'] * line['ms_per_step'] / 1e3 - 1) < 1e-2
    # the legs behind --full are neither run nor reported
    assert not {'seq_eval', 'roofline', 'cpu_baseline', 'parity', 'batched_decode'} & set(line)
    assert sorted(os.listdir(out)) == ['logits.npy', 'state.npy']
    logits, state = np.load(out / 'logits.npy'), np.load(out / 'state.npy')
    assert logits.dtype == np.float32 and state.dtype == np.float32

    # the same seeded tokens through the library from a fresh state: the dump is the last step's result
    lib = library()
    L = lib.library
    ctx = lib.rwkv_init_from_file(str(tmp_path / 'v4-169m-q8_0-seed1.bin'), 1, 99)
    n_vocab, n_state = L.rwkv_get_n_vocab(ctx.ptr), L.rwkv_get_state_len(ctx.ptr)
    assert logits.shape == (n_vocab,) and state.shape == (n_state,)
    tokens = np.random.default_rng(1234).integers(0, n_vocab, size=WARMUP + STEPS).astype(np.int32)
    want_logits, want_state = np.zeros(n_vocab, np.float32), np.zeros(n_state, np.float32)
    assert L.rwkv_mi355x_state_upload(ctx.ptr, None)
    for i in range(len(tokens)):
        assert L.rwkv_mi355x_eval_device(ctx.ptr, tokens[i:i + 1].ctypes.data_as(P_INT), 1, True,
                                         want_logits.ctypes.data_as(P_F), True)
    assert L.rwkv_mi355x_state_download(ctx.ptr, want_state.ctypes.data_as(P_F))
    lib.rwkv_free(ctx)
    assert_bits_equal(logits, want_logits, 'dumped logits')
    assert_bits_equal(state, want_state, 'dumped state')
