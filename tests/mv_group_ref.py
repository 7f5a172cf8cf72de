"""Cases, operands and references of the decode-matvec tests (test_gpu_mv_group.py on the MI355X,
test_mv_group_cpu.py without one).

The reference of one MVGroup entry (csrc/kernels.hpp) is built from the oracle's own pieces:
    xa  = oracle_norm_row in the GPU-association variant                      (SRC_LNMIX)
    v   = the token-shift mix in numpy float32, one IEEE operation per numpy operation, as oracle.c
          writes it: form 0 xa * mu + (xp - xp * mu), form 1 (xp - xa) * mu + xa, form 2 xa
    acc = oracle_matmul in the GPU-association variant (it quantizes v as the kernels do)
    y   = matmul_group_ref.epilogue_f32, emitted blocks = matmul_group_ref.emit_reference
k_mvsig is epilogue_f32(EPI_SIGMUL_ADD, Wv . k, y0, aux = Wr . xr).

A case is (id, build): build(cus) returns (entries, expect) for a device of `cus` compute units --
launch_mv_group's thresholds count row blocks per compute unit, so the row-heavy cases size their M
from it.  expect = (rows, grid, stride, units_max): what the launcher must report for the branch the
case was written for.  Both test files walk the same CASES, so the float64 statement on the CPU covers
every entry the GPU is compared on.
"""
import numpy as np

import matmul_group_ref as R
import oracle_ctypes as oc

F = np.float32
QUANT = ['Q4_0', 'Q4_1', 'Q5_0', 'Q5_1', 'Q8_0']
SRC_ACT, SRC_F32, SRC_LNMIX = 0, 1, 2
CUS_DEFAULT = 256  # the MI355X; the CPU test builds the cases for it


def ceil_div(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------ operands
def x_row(K, seed=0):
    """An activation row: block 0 scaled into the range where its Q8 scale is an fp16 subnormal,
    block 2 (K >= 96) all zero, the rest N(0, 1)."""
    x = np.random.default_rng(7 * K + seed).standard_normal(K).astype(F)
    x[:32] *= F(1e-5)
    if K >= 96:
        x[64:96] = 0
    return x


def ln_operands(K, kind='unit', seed=0):
    """x, carry, lnw, lnb, mu, mu2 [K] of a LayerNorm entry.  lnw in +-[0.5, 1.5] with every 17th
    channel negated, lnb in [-0.5, 0.5]; block 0 of lnw, lnb and carry scaled by 1e-5 (the mixed row's
    block 0 then has an fp16-subnormal Q8 scale), block 2 (K >= 96) of the three zero (an all-zero
    activation block in every form).  kind 'const': x constant (variance 0: the eps path); 'offset': x =
    1e4 + N(0, 1) (|mean| >> spread: cancellation in x - mean)."""
    rng = np.random.default_rng(11 * K + seed)
    x = (rng.standard_normal(K) * 2 + 0.3).astype(F)
    if kind == 'const':
        x[:] = F(3.25)
    elif kind == 'offset':
        x = (1e4 + rng.standard_normal(K)).astype(F)
    carry = rng.standard_normal(K).astype(F)
    lnw = rng.uniform(0.5, 1.5, K).astype(F)
    lnw[16::17] *= F(-1)
    lnb = rng.uniform(-0.5, 0.5, K).astype(F)
    for a in (lnw, lnb, carry):
        a[:32] *= F(1e-5)
        if K >= 96:
            a[64:96] = 0
    mu = rng.uniform(0, 1, K).astype(F)
    mu2 = rng.uniform(0, 1, K).astype(F)
    return dict(x=x, carry=carry, lnw=lnw, lnb=lnb, mu=mu, mu2=mu2)


def entry(fmt, K, M, src, form=0, epi=R.EPI_STORE, emit=False, q8_1=False, kind=None, ln=None, x=None, mu_seed=None,
          carry_out=False, mu2=False):
    """One entry: weights R.weights(fmt, K, M, kind) (kind defaults to the epilogue's), epilogue operands
    R.epi_operands(epi, 1, M)."""
    kind = kind or (R.epi_kind(epi) if epi != R.EPI_STORE else 'unit')
    e = dict(fmt=fmt, K=K, M=M, src=src, form=form, epi=epi, emit=emit, q8_1=q8_1, kind=kind, carry_out=carry_out)
    if src == SRC_LNMIX:
        o = dict(ln if ln is not None else ln_operands(K))
        if mu_seed is not None:  # an entry's own mix over the shared x and carry
            o['mu'] = np.random.default_rng(1000 + mu_seed).uniform(0, 1, K).astype(F)
        e.update(o)
        if not mu2:
            e['mu2'] = None
    else:
        e['x'] = x if x is not None else x_row(K)
    e['y0'], e['aux'], e['bias'] = R.epi_operands(epi, 1, M)
    return e


def weights_of(e):
    return R.weights(e['fmt'], e['K'], e['M'], e['kind'])


# ----------------------------------------------------------------------------------------- reference
def gpu_variant(fn, *a):
    oc.set_variant(oc.VARIANT_GPU)
    try:
        return fn(*a)
    finally:
        oc.set_variant(0)


def mix(form, xa, xp, mu):
    """The token-shift mix of oracle.c (mix_v4 / the v6 form) in float32, nothing contracted."""
    if form == 2:
        return xa.copy()
    if form == 0:
        return xa * mu + (xp - xp * mu)
    return (xp - xa) * mu + xa


def source(e):
    """(v, xa): the row the matvec consumes (float32 [K], before its quantization) and the LayerNorm
    output (None for the other sources)."""
    if e['src'] != SRC_LNMIX:
        return e['x'], None
    xa = gpu_variant(oc.norm_row, e['x'], e['lnw'], e['lnb'])
    v = mix(e['form'], xa, e['carry'], e['mu'])
    assert v.dtype == F
    return v, xa


def act_blocks(fmt, v):
    """quantize_act of v in weight format fmt's activation format: (q, d, s or None, qsum)."""
    q, d, s = oc.quantize_act(R.ACT_FMT[fmt], v)
    return q, d, s, q.reshape(-1, 32).astype(np.int32).sum(1).astype(np.int32)


def reference(e):
    """Everything the kernel writes for entry e: y [M]; emitting: q, d, s, qsum; carry_out [K]; with
    mu2: act2 = (q, d, s, qsum) of the second mix.  Also acc and v for the float64 statements."""
    v, xa = source(e)
    wb, _ = weights_of(e)
    acc = gpu_variant(oc.matmul, e['fmt'], wb, e['K'], e['M'], v[None, :])
    y = R.epilogue_f32(e['epi'], acc, e['y0'], e['aux'], e['bias'])
    out = dict(y=y[0], acc=acc[0], v=v, xa=xa)
    if e['emit']:
        q, d, s, qsum = R.emit_reference(y, e['q8_1'])
        out.update(q=q[0], d=d[0], s=s[0], qsum=qsum[0])
    if e['src'] == SRC_LNMIX and e.get('mu2') is not None:
        out['act2'] = act_blocks(e['fmt'], mix(e['form'], xa, e['carry'], e['mu2']))
    return out


def layernorm_f64(x, w, b, eps=1e-5):
    """(LayerNorm in float64, test_gpu_norms' bound 8 u (|x - mean| s |w| + |mean| s |w| + |b|))."""
    x64 = x.astype(np.float64)
    mean = x64.mean()
    d = x64 - mean
    scale = 1.0 / np.sqrt((d * d).mean() + eps)
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    terms = np.abs(d) * scale * np.abs(w64) + abs(mean) * scale * np.abs(w64) + np.abs(b64)
    return d * scale * w64 + b64, 8 * 2.0 ** -24 * terms


def min_sum_slack(e, v):
    """test_matmul_group_cpu.min_sum_slack for one row: the fp16 rounding of s = d * sum(q) against the
    blocks' mins (Q4_1 / Q5_1 only)."""
    if R.ACT_FMT[e['fmt']] != 'Q8_1':
        return 0.0
    _, wd = weights_of(e)
    mw = np.abs(wd.reshape(e['M'], e['K'] // 32, 32)).max(2).astype(np.float64)
    s = np.abs(oc.quantize_act('Q8_1', v)[2]).astype(np.float64)
    return 2.0 ** -11 * (mw @ s)


def reference_f64(e, v):
    """(y, tolerance) of entry e in float64 on the operands the kernel sees: the dequantized weights and
    v quantized then dequantized.  tolerance = L (1e-5 |v| |W| + 1e-6 [+ the _1 formats' fp16 term]) +
    4 ulp (matmul_group_ref.epilogue_f64)."""
    _, wd = weights_of(e)
    vd = R.act_dequant(e['fmt'], v[None, :])
    w64 = wd.astype(np.float64)
    acc64 = vd @ w64.T
    acc_tol = 1e-5 * (np.abs(vd) @ np.abs(w64).T) + 1e-6 + min_sum_slack(e, v)
    y, tol = R.epilogue_f64(e['epi'], acc64, acc_tol, e['y0'], e['aux'], e['bias'])
    return y[0], tol[0], acc64[0], acc_tol[0]


# --------------------------------------------------------------------------------------------- cases
# K per weight class and units per lane: a full and a ragged last unit each
K_ACT = {'quant': {1: [96, 2048], 2: [2080, 4096], 4: [6176, 8192]},
         'FP16': {1: [320, 512], 2: [768, 1024], 4: [1536, 2048]},
         'FP32': {1: [64, 256], 2: [320, 512], 4: [768, 1024]}}
K_ACT8 = [8224, 14336, 16384]  # quantized rows of 5, 7 and 8 units: k_mv<2, 8, MVK_ACT>
# SRC_F32: 1 unit (U = 1), 2 units (launched as U = 4), 5 units (the round form's second round)
K_F32SRC = {'quant': [96, 4096, 10240], 'FP16': [320, 768, 2560], 'FP32': [64, 512, 1280]}
# LayerNorm: one partial 512-element chunk; a ragged second chunk; LNP 32's limit; LNP 64 ragged and full
K_LN = [64, 576, 2048, 2112, 4096]
M_ACT = [1, 7, 8, 9, 33, 70]
M_SMALL = [1, 9, 70]


def kclass(fmt):
    return fmt if fmt in ('FP16', 'FP32') else 'quant'


def _single(e, rows=2, stride=0):
    rw = 4 * rows
    return [e], (rows, ceil_div(e['M'], rw), stride, R.mv_units(e['fmt'], e['K']))


def _group(entries, rows):
    rw = 4 * rows
    return entries, (rows, sum(ceil_div(e['M'], rw) for e in entries), 0,
                     max(R.mv_units(e['fmt'], e['K']) for e in entries))


CASES = []


def case(name, build):
    CASES.append((name, build))


# ---- a. SRC_ACT, k_mva (one type, <= 4 units; FP32 takes the same shape through the generic unit)
for fi, fmt in enumerate(R.FORMATS):
    ks = [K for U in (1, 2, 4) for K in K_ACT[kclass(fmt)][U]]
    for ki, K in enumerate(ks):
        M = M_ACT[(ki + fi) % 6]
        case(f'act-{fmt}-K{K}-M{M}', lambda cus, fmt=fmt, K=K, M=M: _single(entry(fmt, K, M, SRC_ACT)))
# ---- b. SRC_ACT, quantized rows of 5..8 units: one round of 8
for fi, fmt in enumerate(QUANT):
    for ki, K in enumerate(K_ACT8):
        M = M_SMALL[(ki + fi) % 3]
        case(f'act8-{fmt}-K{K}-M{M}', lambda cus, fmt=fmt, K=K, M=M: _single(entry(fmt, K, M, SRC_ACT)))
# ---- c. SRC_F32
for fi, fmt in enumerate(R.FORMATS):
    for ki, K in enumerate(K_F32SRC[kclass(fmt)]):
        M = M_SMALL[(ki + fi) % 3]
        case(f'f32-{fmt}-K{K}-M{M}', lambda cus, fmt=fmt, K=K, M=M: _single(entry(fmt, K, M, SRC_F32)))


def _persistent(cus, fmt, src, form=0):
    """One entry of more than 8 cus row blocks of 8: 2 cus workgroups walk them (stride = the grid)."""
    M = 64 * cus + 8 * 3 + 5
    e = entry(fmt, 64, M, src, form, carry_out=src == SRC_LNMIX)
    return [e], (2, 2 * cus, 2 * cus, R.mv_units(fmt, 64))


for fmt in ('Q8_0', 'FP16'):
    case(f'f32-walk-{fmt}', lambda cus, fmt=fmt: _persistent(cus, fmt, SRC_F32))
    case(f'ln-walk-{fmt}', lambda cus, fmt=fmt: _persistent(cus, fmt, SRC_LNMIX, 2))

# ---- d. SRC_LNMIX, not emitting, 2 rows per wave: every format x form x K; the entry writes carry_out
for fi, fmt in enumerate(R.FORMATS):
    for form in (0, 1, 2):
        for ki, K in enumerate(K_LN):
            M = [1, 9, 33, 70][(fi + form + ki) % 4]
            case(f'ln-{fmt}-form{form}-K{K}-M{M}', lambda cus, fmt=fmt, form=form, K=K, M=M: _single(
                entry(fmt, K, M, SRC_LNMIX, form, carry_out=True)))
# the F16 one-round shape of 5..8 units (K = 2560, rows 2): k_mv<1, 8, MVK_LN, ., false, W_F16, 64>
for form in (0, 1, 2):
    case(f'ln-f16u8-form{form}', lambda cus, form=form: _single(entry('FP16', 2560, 70, SRC_LNMIX, form, carry_out=True)))


def _rows_group(cus, fmt, form, K, per_cu):
    """Three entries whose 8-row blocks together just exceed per_cu * cus (carry_out on the second)."""
    m = ceil_div(8 * (per_cu * cus + 8), 3)
    Ms = [m + 5, m - 3, m + 1]
    ln = ln_operands(K)
    es = [entry(fmt, K, M, SRC_LNMIX, form, ln=ln, mu_seed=i, carry_out=i == 1) for i, M in enumerate(Ms)]
    assert sum(ceil_div(M, 8) for M in Ms) > per_cu * cus
    return _group(es, 4 if per_cu == 2 else 8)


# 4 rows per wave: more than 2 cus 8-row blocks (K = 64: the thresholds count rows, not bytes)
for fi, fmt in enumerate(R.FORMATS):
    case(f'ln-rows4-{fmt}', lambda cus, fmt=fmt, form=fi % 3: _rows_group(cus, fmt, form, 64, 2))
# 8 rows per wave: more than 4 cus blocks, K > 2048, two units taken in two round trips (U = 1)
for fi, fmt in enumerate(QUANT):
    case(f'ln-rows8-{fmt}', lambda cus, fmt=fmt, form=fi % 3: _rows_group(cus, fmt, form, 2112, 4))
# mu2 / act2_out: the entry's first workgroup emits a second mix of the same LayerNorm
for fi, fmt in enumerate(QUANT):
    K = (64, 2112, 576, 4096, 2048)[fi]
    case(f'ln-mu2-{fmt}-K{K}', lambda cus, fmt=fmt, K=K, form=fi % 2: _single(
        entry(fmt, K, 33, SRC_LNMIX, form, carry_out=True, mu2=True)))
# hard rows: variance 0 and |mean| >> spread
for kind in ('const', 'offset'):
    for fmt, K, form in (('Q4_1', 2112, 0), ('Q8_0', 576, 1), ('FP16', 2048, 2), ('FP32', 64, 1)):
        case(f'ln-{kind}-{fmt}-K{K}', lambda cus, kind=kind, fmt=fmt, K=K, form=form: _single(
            entry(fmt, K, 33, SRC_LNMIX, form, ln=ln_operands(K, kind), carry_out=True)))


# ---- e. SRC_LNMIX, emitting (8 rows per wave, a 32-row block per workgroup) beside a plain entry
def _emit_group(cus, fmt, form, K, M, q8_1, epi=R.EPI_STORE):
    ln = ln_operands(K)
    es = [entry(fmt, K, M, SRC_LNMIX, form, epi=epi, emit=True, q8_1=q8_1, ln=ln, mu_seed=0),
          entry(fmt, K, 33, SRC_LNMIX, form, ln=ln, mu_seed=1, carry_out=True)]
    return _group(es, 8)


for fi, fmt in enumerate(R.FORMATS):
    for form in (0, 1):
        for ki, K in enumerate((576, 2112)):  # quantized: U = 1 and U = 2 (at most cus row blocks)
            M, q8_1 = (32, 96)[(fi + form + ki) % 2], (fi + ki) % 2 == 1
            case(f'emit-{fmt}-form{form}-K{K}-M{M}-{"q81" if q8_1 else "q80"}',
                 lambda cus, fmt=fmt, form=form, K=K, M=M, q8_1=q8_1: _emit_group(cus, fmt, form, K, M, q8_1))
# two units per lane and more row blocks than compute units: taken at U = 1
for fi, fmt in enumerate(QUANT):
    case(f'emit-u1-{fmt}', lambda cus, fmt=fmt, form=fi % 2: _emit_group(cus, fmt, form, 2112, 32 * cus, fi % 2 == 0))

# ---- f. the generic unit (WFIX = -1): a mixed-type group per source (FP32 weights: in every family)
MIXED = ('Q4_0', 'FP16', 'Q5_1')
case('mixed-act', lambda cus: _group([entry(f, K, M, SRC_ACT) for f, K, M in zip(MIXED, (2048, 768, 4096), (9, 33, 70))], 2))
case('mixed-act-rounds', lambda cus: _group(
    [entry(f, K, M, SRC_ACT) for f, K, M in zip(MIXED, (2048, 2560, 6176), (9, 33, 70))], 2))
case('mixed-f32', lambda cus: _group([entry(f, K, M, SRC_F32) for f, K, M in zip(MIXED, (2048, 768, 4096), (9, 33, 70))], 2))
for form in (0, 1, 2):
    case(f'mixed-ln-form{form}', lambda cus, form=form: _group(
        [entry(f, 2112, M, SRC_LNMIX, form, ln=ln_operands(2112), mu_seed=i, carry_out=i == 2)
         for i, (f, M) in enumerate(zip(MIXED, (9, 33, 70)))], 2))

# ---- g. eight entries of unequal M: every b1..b7 boundary inside and at the edge of a workgroup
M_EIGHT = [1, 8, 9, 33, 16, 7, 70, 24]
for fmt in ('Q4_0', 'FP16'):
    K = 576 if fmt == 'Q4_0' else 320
    case(f'eight-act-{fmt}', lambda cus, fmt=fmt, K=K: _group(
        [entry(fmt, K, M, SRC_ACT, x=x_row(K, i % 2)) for i, M in enumerate(M_EIGHT)], 2))
    case(f'eight-f32-{fmt}', lambda cus, fmt=fmt, K=K: _group(
        [entry(fmt, K, M, SRC_F32, x=x_row(K, i)) for i, M in enumerate(M_EIGHT)], 2))
    case(f'eight-ln-{fmt}', lambda cus, fmt=fmt, K=K: _group(
        [entry(fmt, K, M, SRC_LNMIX, 1, ln=ln_operands(K), mu_seed=i, carry_out=i == 3) for i, M in enumerate(M_EIGHT)], 2))

# ---- h. every non-STORE epilogue once per kernel body
for epi in range(1, 11):
    n = R.EPI_NAMES[epi]
    case(f'epi-{n}-mva', lambda cus, epi=epi: _single(entry('Q4_1', 2048, 70, SRC_ACT, epi=epi)))
    case(f'epi-{n}-mv-act', lambda cus, epi=epi: _single(entry('Q5_0', 8224, 70, SRC_ACT, epi=epi)))
    case(f'epi-{n}-mv-f32', lambda cus, epi=epi: _single(entry('Q4_1', 2048, 70, SRC_F32, epi=epi)))
    case(f'epi-{n}-split', lambda cus, epi=epi: _single(entry('Q4_1', 2048, 70, SRC_LNMIX, epi % 3, epi=epi)))
    case(f'epi-{n}-split-emit', lambda cus, epi=epi: _emit_group(cus, 'Q4_1', epi % 2, 2048, 96, epi % 2 == 0, epi))

CASE_IDS = [c[0] for c in CASES]
CASE_BY_ID = dict(CASES)
assert len(CASE_BY_ID) == len(CASES)

# ---- k_mvsig: (fmt, F, C, M) -- F of 1, 2, 3, 4, 5, 7, 8 units (full and ragged alternating), C of 1, 2
SIG_CASES = []
for fi, fmt in enumerate(QUANT):
    for ui, u in enumerate((1, 2, 3, 4, 5, 7, 8)):
        Fk = 2048 * u if (ui + fi) % 2 else 2048 * (u - 1) + 96
        Ck = ((96, 2048), (2080, 4096))[(ui + fi) % 2][(ui // 2) % 2]
        SIG_CASES.append((fmt, Fk, Ck, (1, 8, 9, 70)[(ui + fi) % 4]))


def sig_operands(fmt, Fk, Ck, M):
    """(Wv bytes, k, Wr bytes, xr, y0) of a k_mvsig case; the receptance rows are 'wide', so sigmoid's
    argument spans both of rk_expf's ranges."""
    rng = np.random.default_rng(Fk + Ck + M)
    return (R.weights(fmt, Fk, M)[0], x_row(Fk, 1), R.weights(fmt, Ck, M, 'wide')[0], x_row(Ck, 2),
            rng.standard_normal(M).astype(F))


def sig_reference(fmt, Fk, Ck, M):
    wv, k, wr, xr, y0 = sig_operands(fmt, Fk, Ck, M)
    accv = gpu_variant(oc.matmul, fmt, wv, Fk, M, k[None, :])
    accr = gpu_variant(oc.matmul, fmt, wr, Ck, M, xr[None, :])
    return R.epilogue_f32(R.EPI_SIGMUL_ADD, accv, y0[None, :], accr)[0], accv[0], accr[0]
