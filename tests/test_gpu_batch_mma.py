"""The batched decode's k_mvt route (debug_set "batch_mma_min"): rwkv_mi355x_eval_batch on it is bit-identical to
each context through rwkv_eval and to the route off; the kernel shows under its own name in the kernel statistics."""
import os
import types

import pytest
import torch  # noqa: F401  before librwkv initialises HIP (torch's own HIP runtime must come up first)

from oracle_ctypes import assert_bits_equal
from rwkv_lib import RWKVModel, library
from test_gpu_generate_queue import launches

pytestmark = pytest.mark.gpu
STEPS = 3


@pytest.mark.parametrize('arch,fmt', [(6, 'Q4_0'), (7, 'Q5_1'), (5, 'Q4_1')])
@pytest.mark.parametrize('B', [2, 9, 15])
def test_batch_mma_route_bit_exact(tmp_path, arch, fmt, B):
    """512-wide, 2-layer, 1024-token-vocabulary synthetic models, 3 steps."""
    L = library().library
    p = os.path.join(str(tmp_path), 'm.bin')
    assert L.rwkv_mi355x_write_synthetic_model(p.encode(), arch, 1024, 512, 2, 0, fmt.encode(), 7)
    m = RWKVModel(library(), p)
    c = types.SimpleNamespace(L=L, ptr=m._ctx.ptr)
    toks = [[(31 * i + 17 * j + 5) % 1024 for i in range(B)] for j in range(STEPS)]

    def steps():
        st, out = None, []
        for j in range(STEPS):
            lg, st = m.eval_batch(toks[j], st)
            out.append((lg.copy(), st.copy()))
        return out

    mvt = lambda table: sum(n for k, n in table.items() if k.startswith('k_mvt<'))  # classes carry the weight type
    try:
        assert L.rwkv_mi355x_debug_set(c.ptr, b'batch_mma_min', 2)
        on = steps()  # captured graphs, replayed
        on_eager, on_table = launches(c, steps)  # kernel timing on: eager
        assert L.rwkv_mi355x_debug_set(c.ptr, b'batch_mma_min', 17)
        off, off_table = launches(c, steps)
        assert mvt(on_table) > 0 and mvt(off_table) == 0, (on_table, off_table)
        for j in range(STEPS):
            for k in (0, 1):
                assert_bits_equal(on[j][k], off[j][k], f'step {j} {("logits", "states")[k]}: route on vs off')
                assert_bits_equal(on_eager[j][k], off[j][k], f'step {j} {("logits", "states")[k]}: eager, on vs off')
        for i in range(B):  # each context alone through rwkv_eval
            st = None
            for j in range(STEPS):
                lg, st = m.eval(toks[j][i], st, None, None, use_numpy=True)
                assert_bits_equal(on[j][0][i], lg, f'context {i} step {j} logits vs rwkv_eval')
                assert_bits_equal(on[j][1][i], st, f'context {i} step {j} state vs rwkv_eval')
    finally:
        L.rwkv_mi355x_set_kernel_timing(c.ptr, False)
        m.free()
