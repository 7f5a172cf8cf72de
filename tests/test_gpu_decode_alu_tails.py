"""The decode chain's row reductions by one wave_sums butterfly per wave (mv_common.hpp row_sums:
af_rows, rows_dot_img, maa_dec4_body, mv_body, mv_body_split, k_mva, the Wo rows of both v6
attention layouts): every bit of logits and state stays what the oracle computes.

Two-layer v6 models, V = 4096, through the ABI: 6 tokens of rwkv_eval, logits and the full state
after EVERY token against oracle_ctypes.gpu_variant (the GPU-association oracle) bit for bit, in the
ordered layout (co_mode 0) and the co-resident one (co_mode 1).

Shapes: C = 512 (partial units: lanes past K / 32 blocks contribute nothing), 2048 (one full unit
per lane) and 4096 (two units per lane, the split LayerNorm-prologue body); Q4_0 (one sum per row),
Q5_1 (two sums per row: the m * s accumulator) and Q8_0 (both 16-byte halves of a block).

Batched decode (k_mvb), one case per format: B = 1, 8 and 9 contexts against per-context rwkv_eval,
bit for bit -- 8 fills one activation ring round at one unit per lane, 9 crosses into the next.
"""
import os

import numpy as np
import pytest
import torch  # noqa: F401  before librwkv initialises HIP (torch's own HIP runtime must come up first)

from oracle_ctypes import assert_bits_equal, gpu_variant
from rwkv_lib import RWKVModel, library

pytestmark = pytest.mark.gpu

VOCAB = 4096
LAYERS = 2
WIDTHS = [512, 2048, 4096]
FORMATS = ['Q4_0', 'Q5_1', 'Q8_0']
TOKENS = [int(t) for t in np.random.default_rng(83).integers(0, VOCAB, 6)]

_refs = {}


@pytest.fixture(scope='module')
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp('decode_alu_tails')


def model_path(model_dir, C, fmt):
    p = os.path.join(str(model_dir), f'v6-{C}-{fmt}.bin')
    if not os.path.isfile(p):
        assert library().library.rwkv_mi355x_write_synthetic_model(p.encode(), 6, VOCAB, C, LAYERS, 0, fmt.encode(), 41)
    return p


def reference(path):
    """[(logits, state) after token i] of the oracle's GPU-association variant, each step from the
    previous step's state; computed once per model and shared by both layouts."""
    if path not in _refs:
        out, st = [], None
        for t in TOKENS:
            lg, st = gpu_variant(path, [t], state_in=st)
            out.append((lg.copy(), st.copy()))
        _refs[path] = out
    return _refs[path]


@pytest.mark.parametrize('co_mode', [0, 1])
@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('C', WIDTHS)
def test_decode_bit_exact_vs_oracle(model_dir, C, fmt, co_mode):
    path = model_path(model_dir, C, fmt)
    ref = reference(path)
    L = library()
    m = RWKVModel(L, path)
    assert L.library.rwkv_mi355x_debug_set(m._ctx.ptr, b'co_mode', co_mode)
    st = None
    for i, t in enumerate(TOKENS):
        lg, st = m.eval(t, st, None, None, use_numpy=True)
        assert_bits_equal(lg, ref[i][0], f'C={C} {fmt} co_mode {co_mode}: logits after token {i}')
        assert_bits_equal(st, ref[i][1], f'C={C} {fmt} co_mode {co_mode}: state after token {i}')
    m.free()


@pytest.mark.parametrize('fmt', FORMATS)
def test_batched_decode_equals_per_context(model_dir, fmt):
    path = model_path(model_dir, 512, fmt)
    m = RWKVModel(library(), path)
    n = m._state_buffer_element_count
    # 9 contexts, each one token (its own) past the fresh state, so every context's state differs
    first = [(131 * i + 17) % VOCAB for i in range(9)]
    states = np.zeros((9, n), np.float32)
    for i, t in enumerate(first):
        _, st = m.eval(t, None, None, None, use_numpy=True)
        states[i] = st
    toks = [(977 * i + 5) % VOCAB for i in range(9)]
    single = [m.eval(toks[i], states[i].copy(), None, None, use_numpy=True) for i in range(9)]
    single = [(lg.copy(), st.copy()) for lg, st in single]
    for B in (1, 8, 9):
        blg, bst = m.eval_batch(toks[:B], states[:B].copy())
        for i in range(B):
            assert_bits_equal(blg[i], single[i][0], f'{fmt} B={B}: context {i} logits')
            assert_bits_equal(bst[i], single[i][1], f'{fmt} B={B}: context {i} state')
    m.free()
