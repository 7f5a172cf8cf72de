"""wave_sums<N> (device_common.hpp) against wave_sum63, bit for bit, through
rwkv_mi355x_selftest_wave_sums (one workgroup of one wave).

wave_sums folds N slots per lane with a halving butterfly; lane l must return the wave total of slot
l & (N - 1) with exactly the bits wave_sum63 gives for that slot (the balanced tree over adjacent
lanes; IEEE addition commutes bit for bit, so only the tree's shape matters).  Every lane of the wave
is checked, not only lanes < N: after the butterfly all 64 lanes hold their slot's total.

Operands: seeded normals; magnitudes spread over 2^+-30 with heavy cancellation (x, -x pairs on
adjacent lanes and across rows, so the tree's shape decides what survives); all -0 (the total must
stay -0); mixed +-0; denormals; +-inf without NaN (each slot holds infinities of one sign only).
NaN inputs are excluded: which payload a NaN + NaN addition returns may depend on the operand order,
and the matvecs never produce NaN (weights and activations are finite by construction of the
quantized formats).

The padded three-row form (row_sums<WF, 3>: a zero fourth slot) is checked for the lane -> row
mapping: lanes 0..2 hold rows 0..2, for a plain format (sum + 0.0f) and a _1 format (sum + sum2).
"""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  before librwkv initialises HIP (torch's own HIP runtime must come up first)

from rwkv_lib import library

pytestmark = pytest.mark.gpu

P_F = ctypes.POINTER(ctypes.c_float)
F = np.float32
SIZES = [2, 4, 8, 16, 32, 64]


def selftest(n, p):
    fn = library().library.rwkv_mi355x_selftest_wave_sums
    fn.argtypes = [ctypes.c_int, P_F, P_F, P_F]
    fn.restype = ctypes.c_bool
    p = np.ascontiguousarray(p, F)
    sums, ref = np.zeros(64, F), np.zeros(abs(n), F)
    assert fn(n, p.ctypes.data_as(P_F), sums.ctypes.data_as(P_F), ref.ctypes.data_as(P_F))
    return sums, ref


def operands(kind, width, seed):
    """[64 lanes][width] float32."""
    rng = np.random.default_rng(seed)
    if kind == 'normal':
        return rng.standard_normal((64, width)).astype(F)
    if kind == 'cancel':
        x = (rng.standard_normal((64, width)) * np.exp2(rng.integers(-30, 31, (64, width)))).astype(F)
        x[1::2] = -x[0::2]                      # adjacent pairs cancel exactly ...
        x[2::4] += rng.standard_normal((16, width)).astype(F) * F(2.0 ** -20)  # ... but quads do not
        x[16:32] = -x[0:16] + F(1e-3)           # rows nearly cancel against each other
        x[32:] *= F(2.0 ** 12)
        return x.astype(F)
    if kind == 'neg_zero':
        return np.full((64, width), -0.0, F)
    if kind == 'mixed_zero':
        return np.where(rng.integers(0, 2, (64, width)) == 1, F(-0.0), F(0.0)).astype(F)
    if kind == 'denormal':
        bits = rng.integers(1, 1 << 23, (64, width)).astype(np.uint32) | (rng.integers(0, 2, (64, width)).astype(np.uint32) << 31)
        return bits.view(F)
    if kind == 'inf':
        x = rng.standard_normal((64, width)).astype(F)
        sign = np.where(np.arange(width) % 2 == 0, F(1), F(-1))  # one sign of infinity per slot: no NaN
        hit = rng.integers(0, 8, (64, width)) == 0
        hit[:, : min(width, 2)] |= rng.integers(0, 2, (64, min(width, 2))) == 1
        return np.where(hit, sign * F(np.inf), x).astype(F)
    raise ValueError(kind)


KINDS = ['normal', 'cancel', 'neg_zero', 'mixed_zero', 'denormal', 'inf']


def tree63(col):
    """wave_sum63's tree in float32 numpy: adjacent pairs, quads, ... (a restatement for the zeros)."""
    v = col.astype(F)
    while v.size > 1:
        v = (v[0::2] + v[1::2]).astype(F)
    return v[0]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', SIZES)
def test_every_slot_bit_exact(n, kind):
    p = operands(kind, n, 100 * n + KINDS.index(kind))
    with np.errstate(all='ignore'):
        sums, ref = selftest(n, p)
        assert not np.isnan(ref).any(), 'operands must not produce NaN'
        want = ref[np.arange(64) & (n - 1)]
        assert np.array_equal(sums.view(np.uint32), want.view(np.uint32)), \
            f'N={n} {kind}: lanes {np.nonzero(sums.view(np.uint32) != want.view(np.uint32))[0][:8]} differ'
        if kind != 'denormal':  # numpy may flush or keep denormals by platform: the device pair is the check
            host = np.array([tree63(p[:, j]) for j in range(n)], F)
            assert np.array_equal(ref.view(np.uint32), host.view(np.uint32)), f'N={n} {kind}: wave_sum63 vs the host tree'
    if kind == 'neg_zero':
        assert (sums.view(np.uint32) == 0x80000000).all()


@pytest.mark.parametrize('kind', ['normal', 'cancel', 'neg_zero', 'mixed_zero'])
@pytest.mark.parametrize('n', [3, -3])
def test_padded_three_rows_lane_mapping(n, kind):
    p = operands(kind, 6, 7 + KINDS.index(kind) + (n < 0))
    if not kind.endswith('zero'):
        p[:, 0] += F(1.0)  # rows differ, so a wrong lane -> row mapping shows
    with np.errstate(all='ignore'):
        sums, ref = selftest(n, p)
    assert np.array_equal(sums[:3].view(np.uint32), ref.view(np.uint32)), f'n={n} {kind}: {sums[:3]} vs {ref}'
    if kind == 'normal':
        assert len({int(b) for b in ref.view(np.uint32)}) == 3
    if kind == 'neg_zero':
        # a plain format's sum + 0.0f canonicalises -0 to +0; the _1 form adds two -0 sums: -0
        assert (sums[:3].view(np.uint32) == (0 if n == 3 else 0x80000000)).all()
