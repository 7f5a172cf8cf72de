"""The reference of the decode-matvec GPU tests (mv_group_ref.py) against independent float64
statements, on the CPU, over every case and every entry test_gpu_mv_group.py compares the kernels on.

a. y: float64 epilogue (np.exp / np.tanh) over the float64 product of the dequantized weights and the
   matvec's input row quantized then dequantized.  Tolerance, as test_matmul_group_cpu.py derives it:
       L * (1e-5 |v| |W| + 1e-6 [+ 2^-11 sum |m_w| |s|, the _1 formats' fp16 s]) + 4 ulp(result)
b. oracle_norm_row in the GPU-association variant against a float64 LayerNorm, within test_gpu_norms'
   8 u (|x - mean| scale |w| + |mean| scale |w| + |b|), at every K the cases use and on the hard rows
   (variance 0, |mean| >> spread).  The token-shift mix between a. and b. is three float32 numpy
   operations written as oracle.c writes them.
"""
import numpy as np
import pytest

import matmul_group_ref as R
import mv_group_ref as V
import oracle_ctypes as oc


def check_y(ref_y, ref_acc, y64, tol, acc64, acc_tol, what):
    assert np.all(np.isfinite(ref_y)) and np.all(np.isfinite(y64)), what
    ea = np.abs(ref_acc.astype(np.float64) - acc64)
    assert np.all(ea <= acc_tol), (what, 'acc', float((ea / acc_tol).max()))
    err = np.abs(ref_y.astype(np.float64) - y64)
    print(f'{what}: max err / tol = {float((err / tol).max()):.3g}')
    assert np.all(err <= tol), (what, float((err / tol).max()))


@pytest.mark.parametrize('name', V.CASE_IDS)
def test_reference_against_float64(name):
    entries, expect = V.CASE_BY_ID[name](V.CUS_DEFAULT)
    rows, grid, stride, units = expect
    assert rows in (2, 4, 8) and grid >= 1 and units == max(R.mv_units(e['fmt'], e['K']) for e in entries)
    assert stride == 0 or (len(entries) == 1 and stride == grid == 2 * V.CUS_DEFAULT)
    for i, e in enumerate(entries):
        ref = V.reference(e)
        y64, tol, acc64, acc_tol = V.reference_f64(e, ref['v'])
        check_y(ref['y'], ref['acc'], y64, tol, acc64, acc_tol, f'{name} entry {i}')
        if e['epi'] != R.EPI_STORE:
            assert np.mean(ref['y'].view(np.uint32) != ref['acc'].view(np.uint32)) > 0.5


@pytest.mark.parametrize('fmt,Fk,Ck,M', V.SIG_CASES)
def test_sigmul_reference_against_float64(fmt, Fk, Ck, M):
    """k_mvsig's reference: both products in float64, the gate's tolerance carried through sigmoid
    (Lipschitz 1/4) times |Wv . k|."""
    wv, k, wr, xr, y0 = V.sig_operands(fmt, Fk, Ck, M)
    ref, accv, accr = V.sig_reference(fmt, Fk, Ck, M)
    ev = dict(fmt=fmt, K=Fk, M=M, kind='unit', epi=R.EPI_STORE, y0=None, aux=None, bias=None)
    er = dict(fmt=fmt, K=Ck, M=M, kind='wide', epi=R.EPI_STORE, y0=None, aux=None, bias=None)
    v64, _, _, v_tol = V.reference_f64(ev, k)
    r64, _, _, r_tol = V.reference_f64(er, xr)
    assert np.all(np.abs(accv - v64) <= v_tol) and np.all(np.abs(accr - r64) <= r_tol)
    g = 1.0 / (1.0 + np.exp(-r64))
    y64 = y0 + g * v64
    tol = g * v_tol + 0.25 * r_tol * np.abs(v64) + 4 * R.ulp32(y64) + 4 * R.ulp32(g * v64)
    err = np.abs(ref.astype(np.float64) - y64)
    assert np.all(err <= tol), float((err / tol).max())
    if M == 70:  # the gate's argument reaches both sides of rk_expf's breakpoints
        assert (accr > 0.625).any() and (accr < -0.625).any()


LN_K = sorted({e['K'] for name in V.CASE_IDS if name.startswith(('ln', 'emit', 'mixed-ln', 'eight-ln', 'epi'))
               for e in V.CASE_BY_ID[name](V.CUS_DEFAULT)[0] if e['src'] == V.SRC_LNMIX})


@pytest.mark.parametrize('kind', ['unit', 'const', 'offset'])
@pytest.mark.parametrize('K', LN_K)
def test_norm_row_against_float64(K, kind):
    o = V.ln_operands(K, kind)
    xa = V.gpu_variant(oc.norm_row, o['x'], o['lnw'], o['lnb'])
    ln64, bound = V.layernorm_f64(o['x'], o['lnw'], o['lnb'])
    err = np.abs(xa.astype(np.float64) - ln64)
    print(f'K {K} {kind}: max err / bound = {float((err / (bound + 1e-300)).max()):.3f}')
    assert np.all(np.isfinite(xa)) and np.all(err <= bound), np.argwhere(err > bound)[:4]
    if kind == 'const':  # variance 0: the eps path gives exactly the bias
        assert np.array_equal(xa, o['lnb'])


def test_ln_k_cover_the_register_tiles():
    assert set(V.K_LN) <= set(LN_K) and 2560 in LN_K
