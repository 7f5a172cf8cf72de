"""The reference of the matmul-group GPU tests (matmul_group_ref.py: oracle_matmul in the GPU
association, then the epilogue restated in float32) against an independent float64 statement of the
same epilogue, on the CPU.

float64 side: np.exp / np.tanh over the float64 product of the dequantized weights and the
quantized-then-dequantized input.  Tolerance, derived (matmul_group_ref.epilogue_f64):

    L * (1e-5 * |x| |W| + 1e-6) + 4 ulp(result)

The first term is the project's matmul bound (test_gpu_kernels.test_matmul_kernel) carried through
the arm's Lipschitz constant L in acc: 1/4 sigmoid, 1 tanh, 1.1 silu, 2 max|acc| relu^2, 1/e DECAY6,
0.152 DECAY7, 1/4 SIGMOID_BIAS; 1 for ADD, sigmoid(aux) for SIGMUL_ADD, |aux - y| / 4 for VMIX7.  The
second covers the arm's own float32 roundings and the <= 1.5 ulp exp / tanh.

One correction to that derivation, found here: for the _1 formats (Q4_1, Q5_1 against Q8_1 input)
the matmul adds m_w * s per block with s = fp16(d * sum q), which is NOT the product of the
dequantized operands.  That fp16 rounding moves acc by up to 2^-11 |m_w| |s| per block -- 3 to 7 times
1e-5 |x| |W| + 1e-6 at K = 2048 -- so it joins the matmul bound (min_sum_slack).  The other formats
stay inside the formula as it stands, by a factor of ten or more.
"""
import numpy as np
import pytest

import matmul_group_ref as R
import oracle_ctypes as oc


def min_sum_slack(fmt, K, M, T, kind):
    """Sum over blocks of 2^-11 |m_w| |s_x| (Q4_1 / Q5_1 against Q8_1; 0 elsewhere): how far the
    fp16 rounding of s = d * sum(q) can move acc from the product of the dequantized operands."""
    if R.ACT_FMT[fmt] != 'Q8_1':
        return 0.0
    _, wd = R.weights(fmt, K, M, kind)
    x = R.activations(K, T)
    # m_w of a _1 block is its smallest dequantized value (q = 0) or below it in magnitude
    mw = np.abs(wd.reshape(M, K // 32, 32)).max(2).astype(np.float64)
    s = np.zeros((T, K // 32))
    for t in range(T):
        s[t] = np.abs(oc.quantize_act('Q8_1', x[t])[2])
    return 2.0 ** -11 * (s @ mw.T)


@pytest.mark.parametrize('fmt,K,M,T', R.EPI_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('epi', range(11), ids=R.EPI_NAMES)
def test_epilogue_reference_against_float64(epi, fmt, K, M, T):
    kind = R.epi_kind(epi)
    ref, acc, ops = R.epi_reference(epi, fmt, K, M, T)
    acc64, bound = R.acc_f64(fmt, K, M, T, kind)
    acc_tol = 1e-5 * bound + 1e-6 + min_sum_slack(fmt, K, M, T, kind)
    assert np.all(np.abs(acc.astype(np.float64) - acc64) <= acc_tol)
    v64, tol = R.epilogue_f64(epi, acc64, acc_tol, *ops)
    err = np.abs(ref.astype(np.float64) - v64)
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(v64))
    print(f'{R.EPI_NAMES[epi]} {fmt} K {K} M {M} T {T}: max err / tol = {float((err / tol).max()):.3g}')
    assert np.all(err <= tol), float((err / tol).max())


@pytest.mark.parametrize('fmt,K,M,T', R.EPI_SHAPES, ids=lambda v: str(v))
def test_epilogue_operands_exercise_the_arms(fmt, K, M, T):
    """The operand sets reach what they are meant to: acc of both signs and on both sides of tanh's
    breakpoints, DECAY6 from 1 down to exact 0 with the inner exp at 0, subnormal and inf, and every
    arm's reference different from acc in most elements (a mis-wired epi cannot pass as STORE)."""
    wide = R.acc_gpu(fmt, K, M, T, 'wide')
    a = np.abs(wide)
    assert (wide > 0).any() and (wide < 0).any()
    assert (a < 0.625).any() and ((a >= 0.625) & (a <= 9)).any() and (a > 9).any()
    ref, acc, (_, _, bias) = R.epi_reference(R.EPI_DECAY6, fmt, K, M, T)
    inner = R.gpu_exp(acc + bias[None, :])
    assert (ref == 1).any() and (ref == 0).any() and ((ref > 0.01) & (ref < 0.99)).any()
    tiny = np.finfo(np.float32).tiny
    assert (inner == 0).any() and np.isinf(inner).any() and ((inner > 0) & (inner < tiny)).any()
    z = acc + bias[None, :]
    assert z[np.abs(z) < 50].min() < -8 and z[np.abs(z) < 50].max() > 4
    for epi in range(1, 11):
        ref, acc, _ = R.epi_reference(epi, fmt, K, M, T)
        assert np.mean(ref.view(np.uint32) != acc.view(np.uint32)) > 0.5, R.EPI_NAMES[epi]
