"""The decode matvec family on the MI355X, one MVGroup at a time (rwkv_mi355x_selftest_mv_group ->
launch_mv_group: k_mva, k_mv's mv_body and mv_body_split; rwkv_mi355x_selftest_mv_sigmul -> k_mvsig),
against the oracle.

Reference (mv_group_ref.py): oracle_norm_row, the token-shift mix in numpy float32, oracle_matmul in the
GPU-association variant, the epilogue restated in float32, emitted blocks = quantize_act of the reference
row.  Every output is compared bit for bit: y, the emission (codes, d, s, qsum), act2_out and carry_out.
Every case also asserts the rows per wave, grid, stride and units per lane launch_mv_group reports, so it
is known to have reached the branch it was written for (the table: DESIGN.md 2); the row-heavy cases take
their sizes from the device's compute-unit count.  Outputs start as 0xA5 bytes on the device: a row
nobody wrote cannot equal the reference.

STORE cases of SRC_ACT / SRC_F32 also stay within the project's 1e-5 |W| |x| + 1e-6 of the ggml-order
oracle, and carry_out within test_gpu_norms' bound of a float64 LayerNorm (independent of the oracle).
The shapes launch_mv_group / mv_sigmul_supported decline are refused on the host: launched = 0, outputs
untouched.
"""
import ctypes

import numpy as np
import pytest
import torch  # before librwkv initialises HIP (torch's own HIP runtime must come up first)

import matmul_group_ref as R
import mv_group_ref as V
from oracle_ctypes import TYPE_IDS, assert_bits_equal, matmul as oracle_matmul
from rwkv_lib import library

pytestmark = pytest.mark.gpu

vp, ci = ctypes.c_void_p, ctypes.c_int


class Entry(ctypes.Structure):
    _fields_ = [('wtype', ci), ('W', vp), ('M', ci), ('K', ci), ('src', ci), ('x', vp), ('carry', vp), ('lnw', vp),
                ('lnb', vp), ('mu', vp), ('mu2', vp), ('form', ci), ('epi', ci), ('y0', vp), ('aux', vp), ('bias', vp),
                ('emit', ci), ('out_q8_1', ci), ('y', vp), ('q', vp), ('d', vp), ('s', vp), ('qsum', vp),
                ('carry_out', vp), ('q2', vp), ('d2', vp), ('s2', vp), ('qsum2', vp)]


class Shape(ctypes.Structure):
    _fields_ = [('rows', ci), ('grid', ci), ('stride', ci), ('units_max', ci), ('cus', ci)]


def lib():
    L = library().library
    L.rwkv_mi355x_selftest_mv_group.argtypes = [ci, ctypes.POINTER(Entry), ctypes.POINTER(Shape), ctypes.POINTER(ci)]
    L.rwkv_mi355x_selftest_mv_group.restype = ctypes.c_bool
    L.rwkv_mi355x_selftest_mv_sigmul.argtypes = [ci, vp, ci, ci, vp, ci, vp, ci, ci, vp, vp, vp, ctypes.POINTER(ci)]
    L.rwkv_mi355x_selftest_mv_sigmul.restype = ctypes.c_bool
    return L


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


SENTINEL = {'y': np.float32(-7.5), 'q': 77, 'd': np.float32(-1), 's': np.float32(-1), 'qsum': 12345}


def run_group(entries):
    """Returns (ok, launched, shape, outputs).  The host arrays start as SENTINEL, so a declined launch
    (outputs untouched) and a launched one (every byte copied back from the poisoned device buffers)
    can be told apart."""
    n = len(entries)
    arr = (Entry * n)()
    keep, outs = [], []
    p = lambda a: None if a is None else a.ctypes.data
    for i, e in enumerate(entries):
        M, K = e['M'], e['K']
        o = {'y': np.full(M, SENTINEL['y'], np.float32)}
        if e['emit']:
            o.update(q=np.full(M, 77, np.int8), d=np.full(M // 32, -1, np.float32), s=np.full(M // 32, -1, np.float32),
                     qsum=np.full(M // 32, 12345, np.int32))
        if e.get('carry_out'):
            o['carry_out'] = np.full(K, SENTINEL['y'], np.float32)
        if e.get('mu2') is not None:
            o.update(q2=np.full(K, 77, np.int8), d2=np.full(K // 32, -1, np.float32), s2=np.full(K // 32, -1, np.float32),
                     qsum2=np.full(K // 32, 12345, np.int32))
        wb = e['wb'] if 'wb' in e else V.weights_of(e)[0]
        ops = {k: (None if e.get(k) is None else np.ascontiguousarray(e[k], np.float32))
               for k in ('x', 'carry', 'lnw', 'lnb', 'mu', 'mu2', 'y0', 'aux', 'bias')}
        ops['wb'] = np.ascontiguousarray(wb)
        keep.append(ops)
        arr[i] = Entry(TYPE_IDS[e['fmt']], p(ops['wb']), M, K, e['src'], p(ops['x']), p(ops['carry']), p(ops['lnw']),
                       p(ops['lnb']), p(ops['mu']), p(ops['mu2']), e.get('form', 0), e.get('epi', 0), p(ops['y0']),
                       p(ops['aux']), p(ops['bias']), int(bool(e['emit'])), int(bool(e.get('q8_1'))), p(o['y']),
                       p(o.get('q')), p(o.get('d')), p(o.get('s')), p(o.get('qsum')), p(o.get('carry_out')), p(o.get('q2')),
                       p(o.get('d2')), p(o.get('s2')), p(o.get('qsum2')))
        outs.append(o)
    launched, shape = ci(-1), Shape(-1, -1, -1, -1, -1)
    ok = lib().rwkv_mi355x_selftest_mv_group(n, arr, ctypes.byref(shape), ctypes.byref(launched))
    return ok, launched.value, shape, outs


def check_entry(e, o, what):
    ref = V.reference(e)
    assert_bits_equal(o['y'], ref['y'], what + ' y')
    if e['epi'] != R.EPI_STORE:  # a mis-wired epi cannot pass as STORE
        assert np.mean(ref['y'].view(np.uint32) != ref['acc'].view(np.uint32)) > 0.5
    if e['emit']:
        assert np.array_equal(o['q'], ref['q']), what + ' q'
        assert_bits_equal(o['d'], ref['d'], what + ' d')
        assert np.array_equal(o['qsum'], ref['qsum']), what + ' qsum'
        if e['q8_1']:
            assert_bits_equal(o['s'], ref['s'], what + ' s')
    if e.get('carry_out'):
        assert_bits_equal(o['carry_out'], ref['xa'], what + ' carry_out')
        # ... and the LayerNorm against float64, independent of the oracle
        ln64, bound = V.layernorm_f64(e['x'], e['lnw'], e['lnb'])
        err = np.abs(o['carry_out'].astype(np.float64) - ln64)
        print(f'{what} carry_out: max err / bound = {float((err / (bound + 1e-300)).max()):.3f}')
        assert np.all(err <= bound), np.argwhere(err > bound)[:4]
    if 'act2' in ref:
        q, d, s, qsum = ref['act2']
        assert np.array_equal(o['q2'], q), what + ' act2 q'
        assert_bits_equal(o['d2'], d, what + ' act2 d')
        assert np.array_equal(o['qsum2'], qsum), what + ' act2 qsum'
        if s is not None:
            assert_bits_equal(o['s2'], s, what + ' act2 s')
    if e['epi'] == R.EPI_STORE and e['src'] != V.SRC_LNMIX:
        # the project's matmul bound against the ggml-order oracle (test_gpu_kernels.py)
        wb, wd = V.weights_of(e)
        x = e['x'][None, :]
        ref0 = oracle_matmul(e['fmt'], wb, e['K'], e['M'], x)[0]
        bound = (np.abs(x.astype(np.float64)) @ np.abs(wd.astype(np.float64)).T)[0]
        err = np.abs(o['y'].astype(np.float64) - ref0)
        assert np.all(err <= 1e-5 * bound + 1e-6), float((err / (bound + 1e-12)).max())


@pytest.mark.parametrize('name', V.CASE_IDS)
def test_mv_group(name):
    cus = device_cus()
    entries, expect = V.CASE_BY_ID[name](cus)
    ok, launched, shape, outs = run_group(entries)
    assert ok and launched == 1
    assert shape.cus == cus
    assert (shape.rows, shape.grid, shape.stride, shape.units_max) == expect
    for i, (e, o) in enumerate(zip(entries, outs)):
        check_entry(e, o, f'{name} entry {i}')


def test_hard_operands_are_hard():
    """The default rows hold what they are meant to: a block whose Q8 scale is an fp16 subnormal and an
    all-zero block, in the plain rows and in every form's mixed LayerNorm row."""
    tiny = 2.0 ** -14
    rows = [V.x_row(2048)] + [V.source(V.entry('Q8_0', 2112, 8, V.SRC_LNMIX, form))[0] for form in (0, 1, 2)]
    for v in rows:
        q, d, _, _ = V.act_blocks('Q8_0', v)
        assert 0 < d[0] < tiny and np.all(q[64:96] == 0) and d[2] == 0 and d[1] > tiny


# ------------------------------------------------------------------------------------------- k_mvsig
def run_sigmul(fmt_v, wv, Mv, Fk, k, fmt_r, wr, Mr, Ck, xr, y0):
    y = np.full(Mv, SENTINEL['y'], np.float32)
    launched = ci(-1)
    arrs = [np.ascontiguousarray(a) for a in (wv, k, wr, xr, y0)]
    ok = lib().rwkv_mi355x_selftest_mv_sigmul(TYPE_IDS[fmt_v], arrs[0].ctypes.data, Mv, Fk, arrs[1].ctypes.data,
                                              TYPE_IDS[fmt_r], arrs[2].ctypes.data, Mr, Ck, arrs[3].ctypes.data,
                                              arrs[4].ctypes.data, y.ctypes.data, ctypes.byref(launched))
    return ok, launched.value, y


@pytest.mark.parametrize('fmt,Fk,Ck,M', V.SIG_CASES)
def test_mv_sigmul(fmt, Fk, Ck, M):
    wv, k, wr, xr, y0 = V.sig_operands(fmt, Fk, Ck, M)
    ok, launched, y = run_sigmul(fmt, wv, M, Fk, k, fmt, wr, M, Ck, xr, y0)
    assert ok and launched == 1
    ref, accv, accr = V.sig_reference(fmt, Fk, Ck, M)
    assert_bits_equal(y, ref, f'k_mvsig {fmt} F {Fk} C {Ck} M {M}')
    # ... and the same bits as the two launches it replaces
    e_r = dict(fmt=fmt, K=Ck, M=M, src=V.SRC_ACT, emit=False, x=xr, wb=wr)
    ok, launched, _, (o_r,) = run_group([e_r])
    assert ok and launched == 1
    assert_bits_equal(o_r['y'], accr, 'receptance matvec')
    e_v = dict(fmt=fmt, K=Fk, M=M, src=V.SRC_ACT, emit=False, x=k, wb=wv, epi=R.EPI_SIGMUL_ADD, y0=y0, aux=o_r['y'])
    ok, launched, _, (o_v,) = run_group([e_v])
    assert ok and launched == 1
    assert_bits_equal(y, o_v['y'], 'k_mvsig vs receptance matvec + EPI_SIGMUL_ADD')


# ----------------------------------------------------------------------------------- declined shapes
def untouched(outs):
    return all(np.all(a == SENTINEL[k.rstrip('2')]) for o in outs for k, a in o.items() if k != 'carry_out') and \
        all(np.all(o['carry_out'] == SENTINEL['y']) for o in outs if 'carry_out' in o)


def declined(entries):
    ok, launched, _, outs = run_group(entries)
    return ok and launched == 0 and untouched(outs)


def taken(entries):
    ok, launched, _, outs = run_group(entries)
    return ok and launched == 1 and not untouched(outs)


def test_declined_shapes():
    """Each obstacle alone makes launch_mv_group refuse the group on the host; the same group without
    it is taken."""
    E, A, F32, LN = V.entry, V.SRC_ACT, V.SRC_F32, V.SRC_LNMIX
    # K % 32 != 0 (float rows: the quantized formats have no such matrix)
    assert declined([E('FP32', 48, 9, F32)]) and taken([E('FP32', 64, 9, F32)])
    # LayerNorm: K % 64 != 0, K > 4096 (by launch_mv_shape's register tile), K > 8192
    assert declined([E('Q8_0', 96, 9, LN)]) and taken([E('Q8_0', 128, 9, LN)])
    assert declined([E('Q8_0', 4160, 9, LN)]) and declined([E('FP16', 8256, 9, LN)])
    # a LayerNorm group with two K; two sources; two token-shift forms
    assert declined([E('Q8_0', 128, 9, LN), E('Q8_0', 192, 9, LN)])
    assert taken([E('Q8_0', 128, 9, LN), E('Q8_0', 128, 9, LN)])
    assert declined([E('Q8_0', 128, 9, LN), E('Q8_0', 128, 9, F32)])
    assert declined([E('Q8_0', 128, 9, LN, 0), E('Q8_0', 128, 9, LN, 1)])
    # emission: no prologue source, a plain LayerNorm input, M % 32 != 0
    assert declined([E('Q8_0', 128, 32, A, emit=True)]) and declined([E('Q8_0', 128, 32, F32, emit=True)])
    assert declined([E('Q8_0', 128, 32, LN, 2, emit=True)])
    assert declined([E('Q8_0', 128, 40, LN, 1, emit=True)]) and taken([E('Q8_0', 128, 32, LN, 1, emit=True)])


def test_mv_sigmul_declines():
    """Three C units, nine F units, unequal M, float weights, two weight types: mv_sigmul_supported says
    no and nothing runs."""
    def run(fmt_v, Fk, Mv, fmt_r, Ck, Mr):
        y0 = np.zeros(Mv, np.float32)
        ok, launched, y = run_sigmul(fmt_v, R.weights(fmt_v, Fk, Mv)[0], Mv, Fk, V.x_row(Fk), fmt_r,
                                     R.weights(fmt_r, Ck, Mr)[0], Mr, Ck, V.x_row(Ck), y0)
        return ok, launched, bool(np.all(y == SENTINEL['y']))
    assert run('Q4_0', 2048, 9, 'Q4_0', 4096, 9) == (True, 1, False)
    assert run('Q4_0', 2048, 9, 'Q4_0', 4128, 9) == (True, 0, True)
    assert run('Q4_0', 16416, 9, 'Q4_0', 2048, 9) == (True, 0, True)
    assert run('Q4_0', 2048, 9, 'Q4_0', 2048, 8) == (True, 0, True)
    assert run('FP16', 512, 9, 'FP16', 512, 9) == (True, 0, True)
    assert run('FP32', 256, 9, 'FP32', 256, 9) == (True, 0, True)
    assert run('Q4_0', 2048, 9, 'Q5_0', 2048, 9) == (True, 0, True)
