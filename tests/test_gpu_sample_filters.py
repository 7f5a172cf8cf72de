"""The filtered sampler (csrc/sample_filter.hip: top-k, min-p, typical-p in front of top-p) through
rwkv_mi355x_selftest_sample_filtered / _sample_rows_filtered against rwkv_cpp.sampling.kept_mask and a
float64 inverse CDF, and the four *_filtered calls on the tiny v6 fixture.

Inputs are test_gpu_sampling's: logits round(N(0, 3) * 64) / 64, so ties are exact, distinct logits
differ by >= 1/64 (1.6 % in e, far above float32 error), and l - m is exact in float32.  EPS is that
file's bound on the kernel's normalised float32 masses.

Every parameter is placed where float64 alone decides the kept set:
  top_k      any K: the rule is integer counts over distinct-or-tied e.
  min_p      the float32 middle of two adjacent distinct values of e.
  typical_p  the middle of a gap >= 8 EPS between the masses of two adjacent groups of equal d, where
             also the boundary group's d is more than 2 DERR from both neighbouring groups.  DERR bounds
             |d_device - d_float64|: the device's g = A / S_F is a weighted mean of x = m - l whose
             weights e carry expf's relative error (<= 2^-22: two float32 ulps, the argument being
             exact), which moves a mean by at most 2 * 2^-22 * R, R = max x - min x over F; the two fp64
             sums add at most V * 2^-52 * R; the one float32 rounding of d adds 2^-24 * R.
  top_p      the middle of a gap >= 8 EPS between two achievable masses of the set kept so far.
gap() asserts these conditions for the point it returns."""
import ctypes
import functools
import os

import numpy as np
import pytest

from rwkv_lib import library, RWKVModel
from rwkv_cpp import sampling
from rwkv_cpp.rwkv_cpp_shared_library import make_batch_sampling
from test_gpu_generate_batch import GOLD, PROMPT, V6, bits
from test_gpu_sampling import EPS, U_LAST, logits_for

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 65, 1025, 50277, 65536, 70001]
MODES = ['top_k', 'min_p', 'typical_p', 'all']
RWKV_ERROR_ARGS = 1 << 8


def gap(key, mass, target, key_err=0.0):
    """Over the tie groups of `key` in ascending order: the float32 middle of the interval of
    cumulative mass fractions that group j adds, for the usable j nearest target."""
    vals, inv = np.unique(key, return_inverse=True)
    share = np.bincount(inv, weights=mass) / mass.sum()
    hi = np.cumsum(share)
    lo = hi - share
    mid = 0.5 * (lo + hi)
    ok = (share >= 8 * EPS * 1.01) & (mid < 1.0)
    if key_err:
        far = np.diff(vals) > 2 * key_err
        ok &= np.append(far, True) & np.insert(far, 0, True)
    assert ok.any(), 'no group with a gap of 8 * EPS and a separated key'
    j = int(np.argmin(np.where(ok, np.abs(mid - target), np.inf)))
    point = float(np.float32(mid[j]))
    assert 0.0 < point < 1.0 and hi[j] - point >= 4 * EPS and point - lo[j] >= 4 * EPS
    return point


@functools.lru_cache(maxsize=None)
def case(V, mode):
    """(row, filters, top_p, temperature, kept mask) with every parameter placed as the docstring says."""
    l = logits_for(V)[0]
    x = l.astype(np.float64).max() - l.astype(np.float64)
    e = np.exp(-x)
    f, top_p, keep = {}, 0.0, np.ones(V, bool)
    if mode in ('top_k', 'all'):
        f['top_k'] = max(1, min(40, V // 3))
        keep = sampling.kept_mask(l, **f)
    if mode in ('min_p', 'all'):
        vals = np.unique(e[keep])
        j = len(vals) // 3
        f['min_p'] = float(np.float32(0.5 * (vals[j] + vals[j + 1]))) if len(vals) > 1 else 0.5
        assert len(vals) == 1 or vals[j] < f['min_p'] < vals[j + 1]
        keep = sampling.kept_mask(l, **f)
    if mode in ('typical_p', 'all'):
        spread = x[keep].max() - x[keep].min()
        derr = spread * (2 * 2.0 ** -22 + V * 2.0 ** -52 + 2.0 ** -24)
        g = (e[keep] * x[keep]).sum() / e[keep].sum()
        f['typical_p'] = gap(np.abs(x[keep] - g), e[keep], 0.6, derr)
        keep = sampling.kept_mask(l, **f)
    if mode == 'all':
        top_p = gap(-e[keep], e[keep], 0.8)
    return l, f, top_p, (0.8 if mode == 'all' else 1.0), sampling.kept_mask(l, top_p=top_p, **f)


def run(logits, u, **kw):
    return library().rwkv_mi355x_selftest_sample(logits, u, **kw)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('V', SIZES)
def test_kept_set_and_draw(V, mode):
    l, f, top_p, temperature, mask = case(V, mode)
    p = np.exp(l.astype(np.float64) - float(l.max()))
    p /= p.sum()
    w = np.where(mask, p ** (1.0 / temperature), 0.0)
    C = np.cumsum(w) / w.sum()
    lo = np.concatenate([[0.0], C[:-1]])
    # tokens heavy enough that the middle of their CDF interval is 4 * EPS from both ends
    heavy = np.flatnonzero(w / w.sum() >= 8 * EPS)[:24]
    assert len(heavy) >= 1
    us = np.concatenate([(0.5 * (lo[heavy] + C[heavy])).astype(np.float32),
                         np.random.default_rng(V).random(6, dtype=np.float32), np.array([0.0, U_LAST], np.float32)])
    tok, kept, cutoff = run(np.broadcast_to(l, (len(us), V)), us, temperature=temperature, top_p=top_p, filters=f)
    tok = tok.astype(np.int64)
    assert set(kept) == {int(mask.sum())}, (f, top_p)
    assert (tok < V).all() and mask[tok].all()
    assert list(tok[:len(heavy)]) == list(heavy)
    assert (lo[tok] - EPS <= us).all() and (us < C[tok] + EPS).all()
    assert tok[-2] == np.flatnonzero(mask)[0]  # u = 0: the first kept index
    if not (mode == 'top_k' and f['top_k'] >= V):  # nothing on: k_sample's cutoff, 0 without top_p
        assert abs(cutoff[0] - p[mask].min()) <= 1e-5 * p[mask].min()


@pytest.mark.parametrize('V', [65, 70001])
def test_rows_kernel_with_mixed_filters_is_the_plain_kernel_per_row(V):
    cases = [case(V, mode) for mode in MODES]
    u = np.float32(0.37)
    out = library().rwkv_mi355x_selftest_sample_rows(
        np.stack([c[0] for c in cases]), u, [c[3] for c in cases], [c[2] for c in cases],
        filters={k: [c[1].get(k, 0) for c in cases] for k in ('top_k', 'min_p', 'typical_p')})
    for r, (l, f, top_p, temperature, mask) in enumerate(cases):
        tok, kept, cutoff = run(l, u, temperature=temperature, top_p=top_p, filters=f)
        assert (out['tokens'][r], out['kept'][r]) == (tok[0], kept[0]) and kept[0] == mask.sum()
        assert bits(out['cutoff'][r:r + 1])[0] == bits(cutoff)[0]
        assert out['decode_tokens'][r] == tok[0] and out['lengths'][r] == 1


@pytest.mark.parametrize('V', [1025, 70001])
def test_ties_at_the_kth_value_are_all_kept(V):
    r = np.full(V, -20.0, np.float32)
    # different threads, waves and register rows; 65535 | 65536: the registers against the tail
    ties = [2, 70, 1024] if V == 1025 else [2, 70, 3272, 65535, 65536, V - 1]
    r[7] = 5.0
    r[ties] = 3.0
    us = np.linspace(0, U_LAST, 64).astype(np.float32)
    for K in (2, len(ties)):
        tok, kept, _ = run(np.broadcast_to(r, (64, V)), us, temperature=1.0, top_p=0.0, filters=dict(top_k=K))
        assert set(kept) == {1 + len(ties)}
        assert set(tok) == set(ties) | {7}


@pytest.mark.parametrize('V', [65, 65536, 70001])
def test_top_k_1_is_the_argmax_for_any_u(V):
    r = logits_for(V)[1].copy()
    r[np.argmax(r)] += 1.0  # one maximum
    us = np.linspace(0, U_LAST, 16).astype(np.float32)
    tok, kept, _ = run(np.broadcast_to(r, (16, V)), us, temperature=0.7, top_p=0.9, filters=dict(top_k=1))
    assert set(tok) == {int(np.argmax(r))} and set(kept) == {1}


@pytest.mark.parametrize('V', [65, 70001])
def test_off_values_are_the_unfiltered_kernel_bit_for_bit(V):
    lg = logits_for(V)
    us = np.array([0.1, 0.5, 0.9], np.float32)
    kw = dict(temperature=0.8, top_p=0.5, logit_bias={0: 1.5})
    plain = run(lg, us, **kw)
    for f in ({}, dict(top_k=0), dict(top_k=V), dict(top_k=V + 7), dict(min_p=0.0), dict(typical_p=0.0),
              dict(typical_p=1.0), dict(top_k=V, min_p=0.0, typical_p=1.0)):
        for x, y in zip(plain, run(lg, us, filters=f, **kw)):
            assert np.array_equal(bits(x), bits(y)), f


# ------------------------------------------------------------------ the whole path, tiny v6
@pytest.fixture(scope='module')
def model():
    m = RWKVModel(library(), os.path.join(GOLD, V6))
    yield m
    m.free()


MIXED = dict(temperature=[1.0, 0.8, 1.0, 0.9], top_p=[0.9, 0.0, 0.7, 1.0], seeds=[21, 22, 23, 24],
             top_k=[0, 12, 5, 300], min_p=[0.02, 0.0, 0.05, 0.0], typical_p=[0.0, 0.9, 0.5, 1.0])


def test_generate_top_k_1_is_greedy_with_bit_equal_logprobs(model):
    model.eval_sequence(PROMPT, None, use_numpy=True)
    greedy, glp = model.generate(12, temperature=0.0, logprobs=3)
    model.eval_sequence(PROMPT, None, use_numpy=True)
    first, flp = model.sample(temperature=1.0, seed=5, top_k=1, logprobs=3)
    tokens, lp = model.generate(12, temperature=1.0, seed=5, top_k=1, logprobs=3)
    assert tokens == greedy and first == greedy[0]
    assert flp.token_logprob == glp.token_logprob[0]
    for a, b in zip(lp, glp):
        assert a.tobytes() == b.tobytes()


def test_batch_and_queue_rows_equal_the_sequence_alone(model):
    prompts = [PROMPT[r:] + PROMPT[:r] for r in range(4)]
    n = 10
    alone = []
    for r, prompt in enumerate(prompts):
        kw = {k: [v[r]] for k, v in MIXED.items()}
        out = model.generate_batch([prompt], n, logprobs=2, **kw)
        alone.append((out[0][0], out[1][0]))
    for tokens, lps in (model.generate_batch(prompts, n, logprobs=2, **MIXED),
                        model.generate_queue(prompts, n, lanes=2, logprobs=2, **MIXED)):
        for r in range(4):
            assert tokens[r] == alone[r][0], r
            assert lps[r].token_logprob.tobytes() == alone[r][1].token_logprob.tobytes(), r
    # the filters bite: some row's tokens differ from the same call without them
    plain = model.generate_batch(prompts, n, **{k: MIXED[k] for k in ('temperature', 'top_p', 'seeds')})
    assert plain != [a[0] for a in alone]


def test_bad_filter_values_fail_before_anything_changes(model):
    L, ptr = library().library, model._ctx.ptr
    model.generate_batch([PROMPT, PROMPT[1:]], 2, seeds=[1, 2])  # slots 0 and 1 hold something

    def state():
        st = np.zeros(L.rwkv_get_state_len(ptr), np.float32)
        assert L.rwkv_mi355x_state_download(ptr, st.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        return st

    def slots():
        out = []
        for slot in (0, 1):
            model.batch_load(slot)
            out.append(state())
        return out

    slots_before = slots()
    model.eval_sequence(PROMPT, None, use_numpy=True)
    before = state()
    params = make_batch_sampling(2, seeds=[1, 2])
    for bad in (dict(min_p=1.5), dict(min_p=-0.1), dict(typical_p=float('nan')), dict(typical_p=2.0)):
        for call in (lambda: model.sample(**bad), lambda: model.generate(4, **bad),
                     lambda: library().rwkv_mi355x_generate_batch(model._ctx, 2, 3, params, **bad),
                     lambda: library().rwkv_mi355x_generate_queue(model._ctx, [3, 3], 2, seeds=[1, 2], **bad)):
            with pytest.raises(ValueError):
                call()
            assert L.rwkv_get_last_error(ptr) == RWKV_ERROR_ARGS, bad
    assert np.array_equal(bits(before), bits(state()))
    assert model.sample(temperature=0.0) == model.sample(temperature=0.0, min_p=0.5)  # the logits are still valid
    for a, b in zip(slots_before, slots()):
        assert np.array_equal(bits(a), bits(b))
