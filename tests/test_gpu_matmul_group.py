"""Whole matmul groups (MMGroup, csrc/common.hpp) on the MI355X through a chosen launcher
(rwkv_mi355x_selftest_matmul_group), against the oracle.

Reference (matmul_group_ref.py): acc = oracle_matmul in the GPU-association variant, the epilogue
restated in numpy float32 with the oracle's exp / tanh, emitted blocks = quantize_act of the reference
row.  Everything is compared bit for bit (assert_bits_equal; integer arrays with array_equal).

a. k_mvb (form 1, EPI_STORE) over its shape space: every weight format, K with 1, 2, 4 and 8 units
   per lane (a full and a ragged last unit each), T around the activation ring's depth PD and the
   butterfly's G contexts, M that fills no workgroup -- against the oracle, against k_mm (form 0) and
   within the project's bound of the ggml-order oracle; the K and T it declines.
b. In-kernel Q8 emission of k_mm / k_mm_small / k_mvb / k_fmm (and k_fmm's combine), with a
   non-emitting entry behind the emitting one, an all-zero block and a block whose scale is an fp16
   subnormal.
b2. The int8-MFMA GEMM's own emission (form 2, token-tile records returned de-tiled): the epilogue of
   the direct kernel emitting instead of writing y (fuse_emit), the split-K combine writing y and
   emitting, and the entries that must not fuse.
c. Each of the ten non-STORE epilogues at each site apply_epi is applied at (matmul_group_ref.EPI_SITES).
"""
import ctypes

import numpy as np
import pytest

import matmul_group_ref as R
from oracle_ctypes import TYPE_IDS, assert_bits_equal, matmul as oracle_matmul
from rwkv_lib import library

pytestmark = pytest.mark.gpu


class Entry(ctypes.Structure):
    _fields_ = [('wtype', ctypes.c_int), ('W', ctypes.c_void_p), ('M', ctypes.c_int), ('epi', ctypes.c_int),
                ('y0', ctypes.c_void_p), ('aux', ctypes.c_void_p), ('bias', ctypes.c_void_p), ('emit', ctypes.c_int),
                ('out_q8_1', ctypes.c_int), ('out_tiled', ctypes.c_int), ('fused', ctypes.c_int), ('y', ctypes.c_void_p),
                ('q', ctypes.c_void_p), ('d', ctypes.c_void_p), ('s', ctypes.c_void_p), ('qsum', ctypes.c_void_p)]


assert ctypes.sizeof(Entry) == 104 and Entry.y.offset == 64  # the layout without `fused`: it fills former padding


def lib():
    L = library().library
    L.rwkv_mi355x_selftest_matmul_group.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Entry),
                                                    ctypes.POINTER(ctypes.c_int)]
    L.rwkv_mi355x_selftest_matmul_group.restype = ctypes.c_bool
    return L


def run_group(form, split, T, K, x, entries):
    """entries: dicts fmt, wb, M and optionally epi, y0, aux, bias, emit, q8_1, tiled.  Returns (ok,
    launched, outputs): outputs[i] = dict y [, q, d, s, qsum].  A y the epilogue does not read starts
    as NaN, the emitted arrays as a poison value: whatever the kernel leaves unwritten shows."""
    n = len(entries)
    arr = (Entry * n)()
    keep, outs = [], []
    for i, e in enumerate(entries):
        M, epi = e['M'], e.get('epi', R.EPI_STORE)
        y0 = e.get('y0')
        if y0 is None:
            y0 = np.full((T, M), np.nan, np.float32)
        o = {'y': np.full((T, M), np.nan, np.float32)}
        if e.get('emit'):
            o.update(q=np.full((T, M), 77, np.int8), d=np.full((T, M // 32), -1, np.float32),
                     s=np.full((T, M // 32), -1, np.float32), qsum=np.full((T, M // 32), 12345, np.int32))
        ops = [np.ascontiguousarray(v) if v is not None else None for v in (e['wb'], y0, e.get('aux'), e.get('bias'))]
        keep.append(ops)
        p = lambda a: None if a is None else a.ctypes.data
        arr[i] = Entry(TYPE_IDS[e['fmt']], p(ops[0]), M, epi, p(ops[1]), p(ops[2]), p(ops[3]), int(bool(e.get('emit'))),
                       int(bool(e.get('q8_1'))), int(bool(e.get('tiled'))), -1, p(o['y']), p(o.get('q')), p(o.get('d')),
                       p(o.get('s')), p(o.get('qsum')))
        outs.append(o)
    launched = ctypes.c_int(-1)
    x = np.ascontiguousarray(x, np.float32)
    ok = lib().rwkv_mi355x_selftest_matmul_group(form, split, T, K, x.ctypes.data, n, arr, ctypes.byref(launched))
    for i, o in enumerate(outs):
        o['fused'] = arr[i].fused
    return ok, launched.value, outs


# ------------------------------------------------------------------------------------- a. k_mvb shapes
# K per weight class and unit count U (a full and a ragged last unit), and one K past U = 8
K_QUANT = {1: [96, 2048], 2: [2560, 4096], 4: [5120, 7168], 8: [8224, 14336]}
K_F16 = {1: [320], 2: [768], 4: [1536, 2048], 8: [2560, 4096]}
K_F32 = {1: [64], 2: [512], 4: [768, 1024], 8: [2048]}
K_DECLINED = {'FP16': 4128, 'FP32': 2080}
T_SET = [1, 2, 3, 5, 7, 8, 9, 13, 15]
M_SET = [1, 33, 70]


def k_table(fmt):
    return K_F32 if fmt == 'FP32' else K_F16 if fmt == 'FP16' else K_QUANT


def mvb_cases():
    """Every (format, U) meets every T of T_SET; the full and the ragged K of a U alternate along T
    (starting with the other one in the next format: the unit mask and the context tails are separate
    loops of the kernel), and M rotates through M_SET."""
    cases = []
    for fi, fmt in enumerate(R.FORMATS):
        for U, ks in k_table(fmt).items():
            assert all(R.mvb_u(fmt, K) == U for K in ks)
            cases += [(fmt, ks[(ti + fi) % len(ks)], T, M_SET[(fi + ti + U) % 3]) for ti, T in enumerate(T_SET)]
            if fmt in ('FP16', 'FP32'):  # the float weights' larger context counts, one K per U
                cases += [(fmt, ks[-1], T, M_SET[(ti + U) % 3]) for ti, T in enumerate((31, 255, 256))]
    return cases


def check_store(fmt, K, T, M):
    wb, wd = R.weights(fmt, K, M)
    x = R.activations(K, T)
    ok, launched, (o,) = run_group(1, 1, T, K, x, [dict(fmt=fmt, wb=wb, M=M)])
    assert ok and launched == 1
    assert_bits_equal(o['y'], R.acc_gpu(fmt, K, M, T), f'k_mvb {fmt} K {K} T {T} M {M} vs GPU-association oracle')
    ok0, launched0, (o0,) = run_group(0, 1, T, K, x, [dict(fmt=fmt, wb=wb, M=M)])
    assert ok0 and launched0 == 1
    assert_bits_equal(o['y'], o0['y'], f'k_mvb {fmt} K {K} T {T} M {M} vs launch_mm_group')
    ref = oracle_matmul(fmt, wb, K, M, x)
    bound = np.abs(x.astype(np.float64)) @ np.abs(wd.astype(np.float64)).T
    err = np.abs(o['y'].astype(np.float64) - ref)
    assert np.all(err <= 1e-5 * bound + 1e-6), float((err / (bound + 1e-12)).max())


@pytest.mark.parametrize('fmt,K,T,M', mvb_cases())
def test_mvb_shape_space(fmt, K, T, M):
    check_store(fmt, K, T, M)


@pytest.mark.parametrize('fmt', R.FORMATS)
def test_mvb_declines(fmt):
    """Nine units per lane and 257 contexts are outside k_mvb: nothing launched, no error."""
    K9 = K_DECLINED.get(fmt, 16416)
    assert R.mvb_u(fmt, K9) == 0
    wb, _ = R.weights(fmt, K9, 33)
    ok, launched, (o,) = run_group(1, 1, 5, K9, R.activations(K9, 5), [dict(fmt=fmt, wb=wb, M=33)])
    assert ok and launched == 0 and np.all(np.isnan(o['y']))
    K = k_table(fmt)[1][0]
    wb, _ = R.weights(fmt, K, 33)
    ok, launched, (o,) = run_group(1, 1, 257, K, R.activations(K, 257), [dict(fmt=fmt, wb=wb, M=33)])
    assert ok and launched == 0 and np.all(np.isnan(o['y']))


# ---------------------------------------------------------------------------------------- b. emission
def check_emit(o, ref_y, q8_1, what):
    assert_bits_equal(o['y'], ref_y, what + ' y')
    q, d, s, qsum = R.emit_reference(ref_y, q8_1)
    assert np.array_equal(o['q'], q), what + ' q'
    assert_bits_equal(o['d'], d, what + ' d')
    assert np.array_equal(o['qsum'], qsum), what + ' qsum'
    if q8_1:
        assert_bits_equal(o['s'], s, what + ' s')


K_EMIT = {'FP32': {1: 64, 2: 512}, 'FP16': {1: 320, 2: 768}}
EMIT_T = [1, 3, 5, 9, 15]


def emit_cases():
    """Forms 0 and 1 on the same operands: each (format, U) at every T of EMIT_T (float weights, which
    stay on k_mvb past 15 contexts, also at 31), M and the output format alternating so that each
    (format, U) meets both of each."""
    return [(fmt, U, T, (32, 96)[(ti + mi) % 2], (ti + fi + U + mi) % 2 == 1)
            for fi, fmt in enumerate(R.FORMATS) for U in (1, 2)
            for ti, T in enumerate(EMIT_T + ([31] if fmt in K_EMIT else [])) for mi in (0, 1)]


@pytest.mark.parametrize('fmt,U,T,M,q8_1', emit_cases())
def test_emission_mm_and_mvb(fmt, U, T, M, q8_1):
    """An emitting entry with a non-emitting M = 33 entry behind it: the block0 search and the
    E.emit == 0 branch of an EMIT kernel both run (forms 0: k_mm<., 8, .> / k_mm_small, 1: k_mvb<., 8, U, true>)."""
    K = K_EMIT.get(fmt, {1: 2048, 2: 2560})[U]
    x = R.activations(K, T)
    group = [dict(fmt=fmt, wb=R.weights(fmt, K, M)[0], M=M, emit=1, q8_1=q8_1),
             dict(fmt=fmt, wb=R.weights(fmt, K, 33)[0], M=33)]
    for form in (0, 1):
        ok, launched, (o, o2) = run_group(form, 1, T, K, x, group)
        assert ok and launched == 1
        what = f'form {form} {fmt} K {K} T {T} M {M}'
        check_emit(o, R.acc_gpu(fmt, K, M, T), q8_1, what)
        assert_bits_equal(o2['y'], R.acc_gpu(fmt, K, 33, T), what + ' second entry')


@pytest.mark.parametrize('fmt', ['FP16', 'FP32'])
@pytest.mark.parametrize('T', [16, 70])
@pytest.mark.parametrize('split', [1, 4])
@pytest.mark.parametrize('q8_1', [False, True])
def test_emission_fmm(fmt, T, split, q8_1):
    """k_fmm's emit (split 1, with a non-emitting M = 33 entry behind) and its combine's (split 4)."""
    K, M = 768, 64
    x = R.activations(K, T)
    group = [dict(fmt=fmt, wb=R.weights(fmt, K, M)[0], M=M, emit=1, q8_1=q8_1)]
    if split == 1:
        group.append(dict(fmt=fmt, wb=R.weights(fmt, K, 33)[0], M=33))
    ok, launched, outs = run_group(3, split, T, K, x, group)
    assert ok and launched == 1
    check_emit(outs[0], R.acc_gpu(fmt, K, M, T), q8_1, f'k_fmm {fmt} T {T} split {split}')
    if split == 1:
        assert_bits_equal(outs[1]['y'], R.acc_gpu(fmt, K, 33, T), 'second entry')


@pytest.mark.parametrize('fmt,K', [('Q4_1', 2048), ('Q8_0', 2560), ('FP16', 768)])
def test_mvb_declines_emitting_shapes(fmt, K):
    """An emitting entry that is no whole number of 32-row blocks, one at a U = 4 K, and a tiled out."""
    x = R.activations(K, 5)
    ok, launched, _ = run_group(1, 1, 5, K, x, [dict(fmt=fmt, wb=R.weights(fmt, K, 40)[0], M=40, emit=1)])
    assert ok and launched == 0
    ok, launched, _ = run_group(1, 1, 5, K, x, [dict(fmt=fmt, wb=R.weights(fmt, K, 32)[0], M=32, emit=1, tiled=1)])
    assert ok and launched == 0
    K4 = k_table(fmt)[4][0]
    ok, launched, _ = run_group(1, 1, 5, K4, R.activations(K4, 5),
                                [dict(fmt=fmt, wb=R.weights(fmt, K4, 32)[0], M=32, emit=1)])
    assert ok and launched == 0
    # the same entries without the obstacle are taken
    ok, launched, _ = run_group(1, 1, 5, K, x, [dict(fmt=fmt, wb=R.weights(fmt, K, 32)[0], M=32, emit=1)])
    assert ok and launched == 1


@pytest.mark.parametrize('form,fmt,K,T', [(0, 'Q4_1', 2048, 5), (1, 'Q4_1', 2048, 5), (0, 'FP16', 768, 5),
                                          (1, 'FP16', 768, 5), (0, 'FP16', 320, 5), (1, 'Q5_0', 2560, 3),
                                          (3, 'FP16', 768, 16)])
@pytest.mark.parametrize('q8_1', [False, True])
def test_emission_edge_blocks(form, fmt, K, T, q8_1):
    """EPI_RELU_SQ over the 'edge' operands: rows 0..31 have a negative acc for every context (an
    all-zero block: d = 0, q = 0), rows 32..63 give a block scale in the fp16-subnormal range."""
    M = 96
    acc = R.acc_gpu(fmt, K, M, T, 'edge')
    ref = R.epilogue_f32(R.EPI_RELU_SQ, acc)
    q, d, _, _ = R.emit_reference(ref, q8_1)
    assert np.all(acc[:, :32] < 0) and np.all(d[:, 0] == 0) and np.all(q[:, :32] == 0)
    assert np.all((d[:, 1] > 0) & (d[:, 1] < 2.0 ** -14))
    x = R.activations(K, T, 'edge')
    ok, launched, (o,) = run_group(form, 1, T, K, x, [dict(fmt=fmt, wb=R.weights(fmt, K, M, 'edge')[0], M=M,
                                                           epi=R.EPI_RELU_SQ, emit=1, q8_1=q8_1)])
    assert ok and launched == 1
    check_emit(o, ref, q8_1, f'form {form} {fmt} K {K} T {T} relu^2 edge blocks')


# ------------------------------------------------------------- b2. the GEMM's fused tiled emission
# launch_qgemm sets fuse_emit on an entry whose epilogue can emit Q8_0 token tiles itself; the direct
# kernel (split 1) then writes the tile records INSTEAD of y.  Form 2 returns the flag and the records
# de-tiled; y starts as NaN on the device, so a fused entry must come back all NaN.
FUSABLE = [R.EPI_STORE, R.EPI_SIGMOID, R.EPI_TANH, R.EPI_SILU, R.EPI_RELU_SQ]
FUSE_T = [2, 63, 64, 65, 130]


def fused_cases():
    """Every fusable epilogue on every _0 format and on Q4_1 (the fused branch adds the m * s totals
    itself); T around the 64-token tile, M of one and three row tiles, and K = 2048 (k_qgemm_k64) / 2560
    (k_qgemm) rotate so each meets each of the others."""
    cases = []
    for ei, epi in enumerate(FUSABLE):
        for fi, fmt in enumerate(('Q4_0', 'Q5_0', 'Q8_0', 'Q4_1')):
            i = ei * 4 + fi
            cases.append((epi, fmt, (2048, 2560)[(ei + fi // 2) % 2], (64, 192)[(ei + fi) % 2], FUSE_T[i % 5]))
    return cases


def check_tiles(o, ref_y, q8_1, what):
    q, d, s, qsum = R.emit_reference(ref_y, q8_1)
    assert np.array_equal(o['q'], q), what + ' q'
    assert_bits_equal(o['d'], d, what + ' d')
    assert np.array_equal(o['qsum'], qsum), what + ' qsum'
    if q8_1:
        assert_bits_equal(o['s'], s, what + ' s')


def emission_untouched(o):
    return np.all(o['q'] == 77) and np.all(o['d'] == -1) and np.all(o['s'] == -1) and np.all(o['qsum'] == 12345)


@pytest.mark.parametrize('epi,fmt,K,M,T', fused_cases())
def test_gemm_fused_emission(epi, fmt, K, M, T):
    kind = 'wide' if epi != R.EPI_STORE else 'unit'
    ref = R.epilogue_f32(epi, R.acc_gpu(fmt, K, M, T, kind))
    ok, launched, (o,) = run_group(2, 1, T, K, R.activations(K, T),
                                   [dict(fmt=fmt, wb=R.weights(fmt, K, M, kind)[0], M=M, epi=epi, emit=1, tiled=1)])
    assert ok and launched == 1 and o['fused'] == 1
    assert np.all(np.isnan(o['y'])), 'a fused entry writes no y'
    check_tiles(o, ref, False, f'fused {R.EPI_NAMES[epi]} {fmt} K {K} M {M} T {T}')


@pytest.mark.parametrize('fmt,q8_1', [('Q4_0', False), ('Q5_0', False), ('Q8_0', False), ('Q4_1', True), ('Q5_1', False)])
@pytest.mark.parametrize('M,T', [(64, 33), (96, 65)])
def test_gemm_split_combine_emits(fmt, q8_1, M, T):
    """Split 4: k_qg_combine applies the epilogue, writes y AND emits for every emitting entry (any M
    % 32 == 0, either output format), beside a non-emitting entry."""
    K = 2048
    ref = R.epilogue_f32(R.EPI_SILU, R.acc_gpu(fmt, K, M, T, 'wide'))
    group = [dict(fmt=fmt, wb=R.weights(fmt, K, M, 'wide')[0], M=M, epi=R.EPI_SILU, emit=1, tiled=1, q8_1=q8_1),
             dict(fmt=fmt, wb=R.weights(fmt, K, 64)[0], M=64)]
    ok, launched, (o, o2) = run_group(2, 4, T, K, R.activations(K, T), group)
    assert ok and launched == 1 and o['fused'] == 1 and o2['fused'] == 0
    assert_bits_equal(o['y'], ref, 'combine y')
    check_tiles(o, ref, q8_1, f'combine {fmt} M {M} T {T}')
    assert_bits_equal(o2['y'], R.acc_gpu(fmt, K, 64, T), 'second entry')


@pytest.mark.parametrize('fmt,K,T', [('Q4_0', 2048, 65), ('Q8_0', 2560, 5)])
def test_gemm_entries_that_must_not_fuse(fmt, K, T):
    """Beside a fusing entry in the same launch: M = 96 (no whole 64-row tiles), an ADD epilogue (reads
    y) and a Q8_1 output each keep the plain store -- y written, nothing emitted."""
    x = R.activations(K, T)
    y0, _, _ = R.epi_operands(R.EPI_ADD, T, 64)
    group = [dict(fmt=fmt, wb=R.weights(fmt, K, 64)[0], M=64, emit=1, tiled=1),
             dict(fmt=fmt, wb=R.weights(fmt, K, 96)[0], M=96, emit=1, tiled=1),
             dict(fmt=fmt, wb=R.weights(fmt, K, 64, 'wide')[0], M=64, epi=R.EPI_ADD, y0=y0, emit=1, tiled=1),
             dict(fmt=fmt, wb=R.weights(fmt, K, 128)[0], M=128, emit=1, tiled=1, q8_1=True)]
    ok, launched, outs = run_group(2, 1, T, K, x, group)
    assert ok and launched == 1 and [o['fused'] for o in outs] == [1, 0, 0, 0]
    assert np.all(np.isnan(outs[0]['y']))
    check_tiles(outs[0], R.acc_gpu(fmt, K, 64, T), False, 'the fusing entry')
    refs = [R.acc_gpu(fmt, K, 96, T), R.epilogue_f32(R.EPI_ADD, R.acc_gpu(fmt, K, 64, T, 'wide'), y0),
            R.acc_gpu(fmt, K, 128, T)]
    for o, ref in zip(outs[1:], refs):
        assert_bits_equal(o['y'], ref, 'a non-fused entry')
        assert emission_untouched(o)


@pytest.mark.parametrize('fmt,K,T', [('Q4_0', 2048, 5), ('Q5_0', 2560, 65), ('Q8_0', 2048, 64)])
def test_gemm_fused_emission_edge_blocks(fmt, K, T):
    """EPI_RELU_SQ over the 'edge' operands (test_emission_edge_blocks): an all-zero block and a block
    whose scale is an fp16 subnormal, through the fused emission."""
    M = 64
    acc = R.acc_gpu(fmt, K, M, T, 'edge')
    ref = R.epilogue_f32(R.EPI_RELU_SQ, acc)
    _, d, _, _ = R.emit_reference(ref, False)
    assert np.all(acc[:, :32] < 0) and np.all(d[:, 0] == 0) and np.all((d[:, 1] > 0) & (d[:, 1] < 2.0 ** -14))
    ok, launched, (o,) = run_group(2, 1, T, K, R.activations(K, T, 'edge'),
                                   [dict(fmt=fmt, wb=R.weights(fmt, K, M, 'edge')[0], M=M, epi=R.EPI_RELU_SQ, emit=1, tiled=1)])
    assert ok and launched == 1 and o['fused'] == 1 and np.all(np.isnan(o['y']))
    check_tiles(o, ref, False, f'fused relu^2 edge blocks {fmt} K {K} T {T}')


# ------------------------------------------------------------------------ c. every epilogue, every site
@pytest.mark.parametrize('form,split,fmt,K,M,T', R.EPI_SITES)
@pytest.mark.parametrize('epi', range(1, 11), ids=R.EPI_NAMES[1:])
def test_epilogue_at_every_site(epi, form, split, fmt, K, M, T):
    ref, acc, (y0, aux, bias) = R.epi_reference(epi, fmt, K, M, T)
    assert np.mean(ref.view(np.uint32) != acc.view(np.uint32)) > 0.5  # a mis-wired epi cannot pass as STORE
    x = R.activations(K, T)
    wb, _ = R.weights(fmt, K, M, R.epi_kind(epi))
    ok, launched, (o,) = run_group(form, split, T, K, x, [dict(fmt=fmt, wb=wb, M=M, epi=epi, y0=y0, aux=aux, bias=bias)])
    assert ok and launched == 1
    assert_bits_equal(o['y'], ref, f'{R.EPI_NAMES[epi]} form {form} split {split} {fmt} K {K} M {M} T {T}')
