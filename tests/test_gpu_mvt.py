"""k_mvt (csrc/mv_tile.hip), the int8-MFMA tile matvec of the batched decode at 2..16 contexts, through
rwkv_mi355x_selftest_matmul_group form 4, bit for bit against the oracle (matmul_group_ref.py): its
shape space, emission, epilogues that read y0 / aux / bias, and the groups it declines."""
import numpy as np
import pytest

import matmul_group_ref as R
from oracle_ctypes import assert_bits_equal, matmul as oracle_matmul
from test_gpu_matmul_group import check_emit, run_group

pytestmark = pytest.mark.gpu

QUANT = ['Q4_0', 'Q4_1', 'Q5_0', 'Q5_1', 'Q8_0']
K_SET = [96, 2048, 2560, 7168, 14336]
T_SET = [2, 7, 15, 16]
M_SET = [1, 33, 70]


@pytest.mark.parametrize('fmt,K,T,M', [(fmt, K, T, M_SET[(fi + ki + ti) % 3]) for fi, fmt in enumerate(QUANT)
                                       for ki, K in enumerate(K_SET) for ti, T in enumerate(T_SET)])
def test_mvt_shape_space(fmt, K, T, M):
    """K: empty classes, one block per class, a ragged second round, a half-full last round, seven rounds;
    M fills no tile and rotates along the cases.  Against the GPU-association oracle, k_mvb (form 1) and
    the project's bound of the ggml-order oracle."""
    wb, wd = R.weights(fmt, K, M)
    x = R.activations(K, T)
    ok, launched, (o,) = run_group(4, 1, T, K, x, [dict(fmt=fmt, wb=wb, M=M)])
    assert ok and launched == 1
    assert_bits_equal(o['y'], R.acc_gpu(fmt, K, M, T), f'k_mvt {fmt} K {K} T {T} M {M} vs GPU-association oracle')
    ok1, launched1, (o1,) = run_group(1, 1, T, K, x, [dict(fmt=fmt, wb=wb, M=M)])
    assert ok1 and launched1 == 1
    assert_bits_equal(o['y'], o1['y'], f'k_mvt {fmt} K {K} T {T} M {M} vs k_mvb')
    ref = oracle_matmul(fmt, wb, K, M, x)
    bound = np.abs(x.astype(np.float64)) @ np.abs(wd.astype(np.float64)).T
    err = np.abs(o['y'].astype(np.float64) - ref)
    assert np.all(err <= 1e-5 * bound + 1e-6), float((err / (bound + 1e-12)).max())


@pytest.mark.parametrize('fmt,K,T', [(f, (2048, 2560)[i % 2], (3, 9, 16, 2, 15)[i]) for i, f in enumerate(QUANT)])
@pytest.mark.parametrize('q8_1', [False, True])
def test_mvt_emission(fmt, K, T, q8_1):
    group = [dict(fmt=fmt, wb=R.weights(fmt, K, 64)[0], M=64, emit=1, q8_1=q8_1),
             dict(fmt=fmt, wb=R.weights(fmt, K, 33)[0], M=33)]
    ok, launched, (o, o2) = run_group(4, 1, T, K, R.activations(K, T), group)
    assert ok and launched == 1
    check_emit(o, R.acc_gpu(fmt, K, 64, T), q8_1, f'k_mvt {fmt} K {K} T {T}')
    assert_bits_equal(o2['y'], R.acc_gpu(fmt, K, 33, T), 'second entry')


@pytest.mark.parametrize('fmt,q8_1', [('Q4_1', True), ('Q5_0', False)])
def test_mvt_emission_zero_block(fmt, q8_1):
    """EPI_RELU_SQ over the 'edge' operands: an all-zero block and one with an fp16-subnormal scale."""
    K, T, M = 2048, 5, 96
    ref = R.epilogue_f32(R.EPI_RELU_SQ, R.acc_gpu(fmt, K, M, T, 'edge'))
    _, d, _, _ = R.emit_reference(ref, q8_1)
    assert np.all(d[:, 0] == 0) and np.all((d[:, 1] > 0) & (d[:, 1] < 2.0 ** -14))
    ok, launched, (o,) = run_group(4, 1, T, K, R.activations(K, T, 'edge'),
                                   [dict(fmt=fmt, wb=R.weights(fmt, K, M, 'edge')[0], M=M, epi=R.EPI_RELU_SQ, emit=1,
                                         q8_1=q8_1)])
    assert ok and launched == 1
    check_emit(o, ref, q8_1, f'k_mvt {fmt} relu^2 edge blocks')


@pytest.mark.parametrize('epi', [R.EPI_SIGMUL_ADD, R.EPI_VMIX7], ids=['sigmul_add', 'vmix7'])
@pytest.mark.parametrize('fmt', ['Q4_1', 'Q8_0'])
def test_mvt_epilogues(epi, fmt):
    K, M, T = 2048, 70, 5
    y0, aux, bias = R.epi_operands(epi, T, M)
    kind = R.epi_kind(epi)
    ref = R.epilogue_f32(epi, R.acc_gpu(fmt, K, M, T, kind), y0, aux, bias)
    ok, launched, (o,) = run_group(4, 1, T, K, R.activations(K, T),
                                   [dict(fmt=fmt, wb=R.weights(fmt, K, M, kind)[0], M=M, epi=epi, y0=y0, aux=aux, bias=bias)])
    assert ok and launched == 1
    assert_bits_equal(o['y'], ref, f'k_mvt {R.EPI_NAMES[epi]} {fmt}')


@pytest.mark.parametrize('fmt,K,T,M,emit', [('Q4_0', 2048, 1, 33, 0), ('Q4_0', 2048, 17, 33, 0), ('FP16', 2048, 5, 33, 0),
                                            ('Q5_1', 48, 5, 33, 0), ('Q8_0', 2048, 5, 48, 1)])
def test_mvt_declines(fmt, K, T, M, emit):
    """Nothing launched, nothing written (K = 48 is already refused by the selftest entry: ok false)."""
    x = R.activations(K, T)
    ok, launched, (o,) = run_group(4, 1, T, K, x, [dict(fmt=fmt, wb=R.weights(fmt, K - K % 32 or 32, M)[0], M=M, emit=emit)])
    assert launched == 0 and np.all(np.isnan(o['y'])) and ok == (K % 32 == 0)
    if emit:
        assert np.all(o['q'] == 77) and np.all(o['qsum'] == 12345)
