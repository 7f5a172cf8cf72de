"""The norm kernels against a float64 numpy restatement, independent of the oracle: k_groupnorm
(rwkv_mi355x_selftest_groupnorm) and k_ln_emit (rwkv_mi355x_selftest_ln), with weights away from 1,
biases away from 0 and, in every case, one constant head / row (variance 0: the eps path), one with
mean 1e4 and spread 1 (cancellation in x - mean) and one all-zero.

Elementwise bound, u = 2**-24:
    8 u (|x - mean| scale |w| + |mean| scale |w| + |b|)        (* |g|, + |v * bonus| inside, per mode)
Five fp32 roundings sit on each element (x - mean, * scale, * w, + b and scale itself; modes 1 / 2 add
one or two), each at most u relative to a term of the sum; the float-rounded mean moves x - mean by at
most u |mean|, and the variance it biases moves scale by (u |mean|)^2 / 2 var, below u for these data.
A float32 numpy restatement of the same formula must meet the bound on the same inputs before the
GPU is judged by it (asserted in each test).
"""
import ctypes

import numpy as np
import pytest
import torch  # before librwkv initialises HIP (torch's own HIP runtime must come up first)

from rwkv_lib import library

pytestmark = pytest.mark.gpu

P_F = ctypes.POINTER(ctypes.c_float)
U = 2.0 ** -24
F = np.float32


def ptr(a):
    return a.ctypes.data_as(P_F)


def norm_params(rng, C):
    w = rng.uniform(0.5, 1.5, C).astype(F)
    w[16::17] *= F(-1)
    return w, rng.uniform(-0.5, 0.5, C).astype(F)


def special_rows(rng, x):
    """x [n >= 3][S]: row 0 constant, row 1 mean 1e4 spread 1, row 2 zero."""
    x[0] = F(3.25)
    x[1] = (1e4 + rng.standard_normal(x.shape[1])).astype(F)
    x[2] = 0


def normalize(x, w, b, eps, dt):
    """(x - mean) * scale * w + b over the last axis in precision dt, the statistics in float64 (as the
    kernels sum them) rounded to dt; returns the result and the bound's three terms in float64."""
    x64 = x.astype(np.float64)
    mean = x64.mean(-1, keepdims=True).astype(dt)
    d = x.astype(dt) - mean
    var = (d.astype(np.float64) ** 2).mean(-1, keepdims=True).astype(dt)
    scale = (dt(1) / np.sqrt(var + dt(eps))).astype(dt)
    o = ((d * scale).astype(dt) * w.astype(dt)).astype(dt) + b.astype(dt)
    terms = (np.abs(d) * scale * np.abs(w) + np.abs(mean) * scale * np.abs(w) + np.abs(b)).astype(np.float64)
    return o.astype(dt), terms


@pytest.mark.parametrize('mode,eps', [(0, 1e-5), (1, 64e-5), (2, 64e-5)])
@pytest.mark.parametrize('T,H,S', [(1, 8, 64), (5, 40, 64), (3, 16, 8), (2, 3, 32)])
def test_groupnorm_vs_float64(T, H, S, mode, eps):
    """Modes: 0 the v5.1 norm, 1 * g (v5.2 / v6 gate), 2 (+ v * bonus) * g (v7).  H * S = 512 and 2560
    fill two and ten 256-channel blocks; 16 heads of 8 is the v6 fixture's shape; 3 heads of 32 make
    C = 96, a last wave with half its lanes past the row."""
    rng = np.random.default_rng(T * 1000 + H * 10 + S + mode)
    C = H * S
    y = (rng.standard_normal((T, H, S)) * rng.uniform(0.1, 4, (T, H, 1)) + rng.uniform(-2, 2, (T, H, 1))).astype(F)
    special_rows(rng, y.reshape(T * H, S))
    w, b = norm_params(rng, C)
    g = rng.standard_normal((T, C)).astype(F)
    v = rng.standard_normal((T, C)).astype(F)
    bonus = rng.standard_normal((T, H)).astype(F)

    def restate(dt):
        o, terms = normalize(y, w.reshape(H, S), b.reshape(H, S), eps, dt)
        vb = v.reshape(T, H, S).astype(dt) * bonus[:, :, None].astype(dt)
        if mode == 2:
            o = (o + vb).astype(dt)
            terms = terms + np.abs(vb)
        if mode >= 1:
            o = (o * g.reshape(T, H, S).astype(dt)).astype(dt)
            terms = terms * np.abs(g.reshape(T, H, S))
        return o.astype(np.float64), terms

    ref, terms = restate(np.float64)
    bound = 8 * U * terms
    f32, _ = restate(np.float32)
    assert np.all(np.abs(f32 - ref) <= bound), 'the bound does not hold for a float32 restatement'
    out = np.full((T, C), np.nan, F)
    assert library().library.rwkv_mi355x_selftest_groupnorm(T, H, S, eps, mode, ptr(y), ptr(w), ptr(b), ptr(g), ptr(v),
                                                            ptr(bonus), ptr(out))
    err = np.abs(out.reshape(T, H, S).astype(np.float64) - ref)
    print(f'groupnorm T {T} H {H} S {S} mode {mode}: max err / bound = {float((err / (bound + 1e-300)).max()):.3f}')
    assert np.all(np.isfinite(out))
    assert np.all(err <= bound), np.argwhere(err > bound)[:4]


@pytest.mark.parametrize('C', [64, 768, 2560, 4096, 4608])
def test_ln_emit_vs_float64(C):
    """C = 64: one lane group of one chunk; 768 / 2560: a ragged last 512-element chunk; 4096: eight
    whole chunks; 4608: past the widths the register prologues hold."""
    rng = np.random.default_rng(C)
    rows = 5
    x = (rng.standard_normal((rows, C)) * 2 + 0.3).astype(F)
    special_rows(rng, x)
    w, b = norm_params(rng, C)
    ref, terms = normalize(x, w, b, 1e-5, np.float64)
    bound = 8 * U * terms
    f32, _ = normalize(x, w, b, 1e-5, np.float32)
    assert np.all(np.abs(f32.astype(np.float64) - ref) <= bound), 'the bound does not hold for a float32 restatement'
    out = np.full((rows, C), np.nan, F)
    assert library().library.rwkv_mi355x_selftest_ln(C, rows, ptr(x), ptr(w), ptr(b), ptr(out))
    err = np.abs(out.astype(np.float64) - ref)
    print(f'ln C {C}: max err / bound = {float((err / (bound + 1e-300)).max()):.3f}')
    assert np.all(np.isfinite(out))
    assert np.all(err <= bound), np.argwhere(err > bound)[:4]
