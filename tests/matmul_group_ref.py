"""Operands and references of the matmul-group tests (test_gpu_matmul_group.py on the MI355X,
test_matmul_group_cpu.py without one).

The reference of one MMGroup entry (csrc/common.hpp) is built in two steps: acc = oracle_matmul in
the oracle's GPU-association variant, then the entry's epilogue restated in numpy float32 with one
IEEE operation per numpy operation (both libraries build with -ffp-contract=off) and the oracle's
restated exp / tanh (oracle_gpu_expf / oracle_gpu_tanhf).  An independent float64 statement of each
epilogue (np.exp / np.tanh over the float64 product of the dequantized operands) and its derived
tolerance pin that reference on the CPU.
"""
import ctypes

import numpy as np

import oracle_ctypes as oc

FORMATS = ['FP32', 'FP16', 'Q4_0', 'Q4_1', 'Q5_0', 'Q5_1', 'Q8_0']
ACT_FMT = {'FP32': 'FP32', 'FP16': 'FP16', 'Q4_0': 'Q8_0', 'Q5_0': 'Q8_0', 'Q8_0': 'Q8_0', 'Q4_1': 'Q8_1',
           'Q5_1': 'Q8_1'}

(EPI_STORE, EPI_SIGMOID, EPI_TANH, EPI_SILU, EPI_RELU_SQ, EPI_ADD, EPI_SIGMUL_ADD, EPI_DECAY6, EPI_DECAY7,
 EPI_SIGMOID_BIAS, EPI_VMIX7) = range(11)
EPI_NAMES = ['store', 'sigmoid', 'tanh', 'silu', 'relu_sq', 'add', 'sigmul_add', 'decay6', 'decay7', 'sigmoid_bias',
             'vmix7']
READS_Y = (EPI_ADD, EPI_SIGMUL_ADD, EPI_VMIX7)
READS_AUX = (EPI_SIGMUL_ADD, EPI_VMIX7)
READS_BIAS = (EPI_DECAY6, EPI_DECAY7, EPI_SIGMOID_BIAS, EPI_VMIX7)

F1 = np.float32(1)
DECAY7_SCALE = np.float32(-0.606531)


def mv_units(fmt, K):
    """16-byte units per lane of the decode matvecs (csrc/mv_common.hpp mv_units)."""
    if fmt == 'FP32':
        return (K + 255) // 256
    if fmt == 'FP16':
        return (K + 511) // 512
    return (K // 32 + 63) // 64


def mvb_u(fmt, K):
    """k_mvb's unit count U for one K (1, 2, 4, 8), or 0 where launch_mvb_group declines."""
    u = mv_units(fmt, K)
    return 1 if u <= 1 else 2 if u <= 2 else 4 if u <= 4 else 8 if u <= 8 else 0


def _gpu_fn(name):
    f = getattr(oc.lib(), name)
    f.restype = ctypes.c_float
    f.argtypes = [ctypes.c_float]
    return f


def gpu_exp(a):
    """rk_expf elementwise (the oracle's restatement), float32 in and out."""
    f = _gpu_fn('oracle_gpu_expf')
    a = np.asarray(a, np.float32)
    return np.array([f(v) for v in a.ravel().tolist()], np.float32).reshape(a.shape)


def gpu_tanh(a):
    f = _gpu_fn('oracle_gpu_tanhf')
    a = np.asarray(a, np.float32)
    return np.array([f(v) for v in a.ravel().tolist()], np.float32).reshape(a.shape)


def gpu_sigmoid(a):
    return F1 / (F1 + gpu_exp(-a))


def epilogue_f32(epi, acc, y0=None, aux=None, bias=None):
    """apply_epi (csrc/device_common.hpp) in numpy float32, operation by operation."""
    acc = np.asarray(acc, np.float32)
    with np.errstate(over='ignore', under='ignore'):
        if epi == EPI_STORE:
            out = acc.copy()
        elif epi == EPI_SIGMOID:
            out = gpu_sigmoid(acc)
        elif epi == EPI_TANH:
            out = gpu_tanh(acc)
        elif epi == EPI_SILU:
            out = acc / (F1 + gpu_exp(-acc))
        elif epi == EPI_RELU_SQ:
            r = np.where(acc > 0, acc, np.float32(0)).astype(np.float32)
            out = r * r
        elif epi == EPI_ADD:
            out = y0 + acc
        elif epi == EPI_SIGMUL_ADD:
            out = y0 + gpu_sigmoid(aux) * acc
        elif epi == EPI_DECAY6:
            out = gpu_exp(-gpu_exp(acc + bias[None, :]))
        elif epi == EPI_DECAY7:
            out = gpu_exp(gpu_sigmoid(acc + bias[None, :]) * DECAY7_SCALE)
        elif epi == EPI_SIGMOID_BIAS:
            out = gpu_sigmoid(acc + bias[None, :])
        elif epi == EPI_VMIX7:
            out = y0 + (aux - y0) * gpu_sigmoid(acc + bias[None, :])
        else:
            raise ValueError(epi)
    assert out.dtype == np.float32
    return out


def ulp32(v):
    """The float32 spacing at |v| (float64 array)."""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def epilogue_f64(epi, acc, acc_tol, y0=None, aux=None, bias=None):
    """(value, tolerance) of an epilogue in float64 over a float64 acc whose float32 counterpart is
    known to within acc_tol (elementwise).  tolerance = L * acc_tol + 4 ulp32(value): L the arm's
    Lipschitz constant in acc over the range used (the y-reading arms: the factor acc is multiplied
    by), and 4 ulp for the arm's own roundings -- at most four float32 operations of half an ulp each
    and the <= 1.5 ulp exp / tanh."""
    a = np.asarray(acc, np.float64)
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    with np.errstate(over='ignore', under='ignore'):
        if epi == EPI_STORE:
            v, L = a, 1.0
        elif epi == EPI_SIGMOID:
            v, L = sig(a), 0.25
        elif epi == EPI_TANH:
            v, L = np.tanh(a), 1.0
        elif epi == EPI_SILU:
            v, L = a * sig(a), 1.1
        elif epi == EPI_RELU_SQ:
            v, L = np.maximum(a, 0.0) ** 2, 2.0 * np.abs(a).max()
        elif epi == EPI_ADD:
            v, L = y0 + a, 1.0
        elif epi == EPI_SIGMUL_ADD:
            g = sig(aux.astype(np.float64))
            v, L = y0 + g * a, g
        elif epi == EPI_DECAY6:
            v, L = np.exp(-np.exp(a + bias[None, :])), 1.0 / np.e
        elif epi == EPI_DECAY7:
            v, L = np.exp(sig(a + bias[None, :]) * float(DECAY7_SCALE)), 0.152
        elif epi == EPI_SIGMOID_BIAS:
            v, L = sig(a + bias[None, :]), 0.25
        elif epi == EPI_VMIX7:
            dlt = aux.astype(np.float64) - y0
            v, L = y0 + dlt * sig(a + bias[None, :]), np.abs(dlt) / 4
        else:
            raise ValueError(epi)
    return v, L * acc_tol + 4 * ulp32(v)


# ------------------------------------------------------------------------------------------ operands
def special_rows(M):
    """The rows whose bias is -105, +90 and -100 (epi_operands)."""
    return [M // 3, M // 2, (2 * M) // 3]


_weights = {}
_acts = {}
_accs = {}


def weights(fmt, K, M, kind='unit'):
    """(block bytes, dequantized float32 [M, K]) of the seeded matrix, built once per shape.
    kind 'unit': rows of norm ~1 (acc ~ N(0, 1)); 'wide': row m scaled by a factor spread
    geometrically over [0.05, 15], so |acc| lies on both sides of 0.625 and of 9; 'edge': rows 0..31 all
    negative (against a positive input: a negative acc everywhere), rows 32..63 scaled by 0.022
    (relu(acc)^2 of order 1e-3: a Q8 scale in the fp16-subnormal range), the rest as 'unit'; 'bias':
    'unit' with the rows of epi_operands' three special bias values scaled by 0.1, so acc + bias stays
    within 0.5 of them."""
    key = (fmt, K, M, kind)
    if key not in _weights:
        rng = np.random.default_rng(1000 * K + 3 * M + ('unit', 'wide', 'edge', 'bias').index(kind))
        w = (rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32)
        if kind == 'wide':
            s = np.geomspace(0.05, 15.0, M)
            w *= rng.permutation(s).astype(np.float32)[:, None]
        elif kind == 'edge':
            w[:32] = -np.abs(w[:32])
            w[32:64] *= np.float32(0.022)
        elif kind == 'bias':
            w[special_rows(M)] *= np.float32(0.1)
        wb = oc.quantize_rows(fmt, w)
        _weights[key] = (wb, oc.dequantize(fmt, wb, K, M))
    return _weights[key]


def activations(K, T, kind='unit'):
    """x [T][K] float32; 'edge': all positive."""
    key = (K, T, kind)
    if key not in _acts:
        x = np.random.default_rng(K * 3 + T).standard_normal((T, K)).astype(np.float32)
        x[0, :64] *= np.float32(1e-5)  # Q8 scales (and Q8_1 sums) in the fp16 subnormal range
        if kind == 'edge':
            x = np.abs(x)
        _acts[key] = x
    return _acts[key]


def acc_gpu(fmt, K, M, T, kind='unit'):
    """oracle_matmul in the GPU-association variant, computed once per operand set."""
    key = (fmt, K, M, T, kind)
    if key not in _accs:
        wb, _ = weights(fmt, K, M, kind)
        x = activations(K, T, 'edge' if kind == 'edge' else 'unit')
        oc.set_variant(oc.VARIANT_GPU)
        try:
            _accs[key] = oc.matmul(fmt, wb, K, M, x)
        finally:
            oc.set_variant(0)
        _accs[key].setflags(write=False)
    return _accs[key]


def act_dequant(fmt, x):
    """x as the matmul of weight format fmt sees it (quantized, then dequantized), float64."""
    a = ACT_FMT[fmt]
    if a == 'FP32':
        return x.astype(np.float64)
    if a == 'FP16':
        return x.astype(np.float16).astype(np.float64)
    out = np.zeros(x.shape, np.float64)
    for t in range(x.shape[0]):
        q, d, _ = oc.quantize_act(a, x[t])
        out[t] = q.astype(np.float64) * np.repeat(d.astype(np.float64), 32)
    return out


def acc_f64(fmt, K, M, T, kind='unit'):
    """(acc, bound): the float64 product of the dequantized operands and |x| |W| of the same."""
    _, wd = weights(fmt, K, M, kind)
    xd = act_dequant(fmt, activations(K, T, 'edge' if kind == 'edge' else 'unit'))
    w64 = wd.astype(np.float64)
    return xd @ w64.T, np.abs(xd) @ np.abs(w64).T


def epi_operands(epi, T, M):
    """(y0, aux, bias) of an epilogue at [T][M]: y0 and aux of order 1; bias spread over [-9, 5] with
    one value at -105 and one at +90 (rk_expf's cut-offs: the inner exp underflows to 0 or overflows
    to inf) and one at -100 (the inner exp a float32 subnormal)."""
    rng = np.random.default_rng(100 * epi + T + M)
    y0 = rng.standard_normal((T, M)).astype(np.float32) if epi in READS_Y else None
    aux = rng.standard_normal((T, M)).astype(np.float32) if epi in READS_AUX else None
    bias = None
    if epi in READS_BIAS:
        bias = rng.permutation(np.linspace(-9.0, 5.0, M)).astype(np.float32)
        bias[special_rows(M)] = [-105.0, 90.0, -100.0]
    return y0, aux, bias


def epi_kind(epi):
    """The weights an epilogue is tried on: the bias arms spread acc + bias through the bias."""
    return 'bias' if epi in READS_BIAS else 'wide'


def emit_reference(y, q8_1):
    """quantize_act of every reference row: (q [T][M] int8, d, s, qsum [T][M / 32])."""
    T, M = y.shape
    q = np.zeros((T, M), np.int8)
    d = np.zeros((T, M // 32), np.float32)
    s = np.zeros((T, M // 32), np.float32)
    for t in range(T):
        rq, rd, rs = oc.quantize_act('Q8_1' if q8_1 else 'Q8_0', y[t])
        q[t], d[t] = rq, rd
        if q8_1:
            s[t] = rs
    return q, d, s, q.reshape(T, M // 32, 32).astype(np.int32).sum(2).astype(np.int32)


# ------------------------------------------------------------------------ the epilogue sites' cases
# (form, split, fmt, K, M, T): every site apply_epi is applied at, one small shape each.
#   form 0: k_mm (T = 1: one token per pass, T = 5: four), k_mm_small (FP16, K <= 512, T >= 2)
#   form 1: k_mvb
#   form 2: k_qgemm's direct epilogue -- scalar at M = 70, four rows per access at M = 96 -- and, split
#           4 at M = 96, k_qg_combine (a group with an M % 32 != 0 entry is never split: M = 70 with
#           split 4 runs the direct kernel again); Q4_1 adds the m * s totals, Q5_0 does not
#   form 3: k_fmm, unsplit and (split 4) through k_qg_combine
EPI_SITES = [(form, 1, fmt, K, 70, T) for form in (0, 1) for fmt, K in (('Q4_1', 2048), ('FP16', 768)) for T in (1, 5)]
EPI_SITES += [(0, 1, 'FP16', 320, 70, 5)]
EPI_SITES += [(2, split, fmt, 2048, M, 33) for fmt in ('Q4_1', 'Q5_0') for M in (70, 96) for split in (1, 4)]
EPI_SITES += [(3, split, 'FP16', 2048, 96, 33) for split in (1, 4)]
EPI_SHAPES = sorted({(fmt, K, M, T) for _, _, fmt, K, M, T in EPI_SITES})


def epi_reference(epi, fmt, K, M, T):
    """(reference y, acc, (y0, aux, bias)) of epilogue epi at one shape of EPI_SHAPES."""
    acc = acc_gpu(fmt, K, M, T, epi_kind(epi))
    ops = epi_operands(epi, T, M)
    return epilogue_f32(epi, acc, *ops), acc, ops
