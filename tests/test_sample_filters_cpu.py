"""rwkv_cpp.sampling.kept_mask against the sort-based textbook statement of each rule at V <= 64, and
the ctypes mirror of struct rwkv_mi355x_filters against the header.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from rwkv_lib import REPO
from rwkv_cpp import sampling
from rwkv_cpp.rwkv_cpp_shared_library import RWKVFilters, make_filters


def row(V, seed):
    """test_gpu_sampling's inputs: exact ties, distinct logits >= 1/64 apart."""
    return (np.round(np.random.default_rng(seed).normal(0, 3, V) * 64) / 64).astype(np.float32)


def textbook(l, top_k, min_p, typical_p, top_p):
    """Each rule as its paper or library states it: sort, walk, cut -- then widen the cut to its ties."""
    l = l.astype(np.float64)
    p = np.exp(l - l.max())
    p /= p.sum()
    keep = np.ones(len(l), bool)
    if 0 < top_k < len(l):
        keep &= p >= sorted(p, reverse=True)[top_k - 1]
    if min_p > 0:
        keep &= p >= float(np.float32(min_p)) * p.max()
    for active, key in ((0 < typical_p < 1, 'typical'), (0 < top_p < 1, 'top_p')):
        if not active:
            continue
        idx = np.flatnonzero(keep)
        q = p[idx] / p[idx].sum()
        if key == 'typical':
            score = np.abs(-np.log(q) - (-(q * np.log(q)).sum()))  # |surprise - conditional entropy|
            want = typical_p
        else:
            score, want = -q, top_p
        acc, cut = 0.0, None
        for j in np.argsort(score, kind='stable'):
            acc += q[j]
            cut = score[j]
            if acc > want:
                break
        # ties at the cut: scores equal up to the float64 noise of the normalisation
        keep[idx] &= score <= cut + 1e-12 * max(1.0, abs(cut))
    return keep


@pytest.mark.parametrize('V', [1, 2, 7, 64])
@pytest.mark.parametrize('rule', [dict(top_k=3), dict(min_p=0.05), dict(typical_p=0.6), dict(top_p=0.7),
                                  dict(top_k=20, min_p=0.01, typical_p=0.9, top_p=0.8)])
def test_kept_mask_is_the_textbook_rule(V, rule):
    kw = dict(top_k=0, min_p=0.0, typical_p=0.0, top_p=0.0)
    kw.update(rule)
    for seed in range(8):
        l = row(V, seed)
        got = sampling.kept_mask(l, **kw)
        assert np.array_equal(got, textbook(l, **kw)), (V, seed, rule)
        assert got.any()


def test_off_values_keep_everything_and_ties_stay_together():
    l = row(64, 3)
    for kw in (dict(), dict(top_k=0), dict(top_k=64), dict(top_k=1000), dict(min_p=0.0), dict(typical_p=0.0),
               dict(typical_p=1.0), dict(top_p=0.0), dict(top_p=1.0)):
        assert sampling.kept_mask(l, **kw).all(), kw
    t = np.array([0.0, 2.0, 1.0, 2.0, 1.0, -3.0], np.float32)
    assert list(sampling.kept_mask(t, top_k=1)) == [False, True, False, True, False, False]
    assert list(sampling.kept_mask(t, top_k=3)) == [False, True, True, True, True, False]
    with pytest.raises(ValueError):
        sampling.kept_mask(t, min_p=1.5)
    with pytest.raises(ValueError):
        sampling.kept_mask(t, typical_p=float('nan'))


def test_ctypes_filters_mirror_the_header():
    text = open(os.path.join(REPO, 'include', 'rwkv_mi355x.h')).read()
    body = re.search(r'struct rwkv_mi355x_filters \{(.*?)\};', text, re.S).group(1)
    decl = re.findall(r'const\s+(\w+)\s*\*\s*(\w+);', body)
    assert decl == [('uint32_t', 'top_k'), ('float', 'min_p'), ('float', 'typical_p')]
    ctype = {'uint32_t': ctypes.c_uint32, 'float': ctypes.c_float}
    assert [(n, t) for n, t in RWKVFilters._fields_] == [(n, ctypes.POINTER(ctype[t])) for t, n in decl]
    assert ctypes.sizeof(RWKVFilters) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert make_filters(4) is None
    f = make_filters(2, top_k=5, typical_p=[0.5, 0.25])
    assert list(f.top_k[0:2]) == [5, 5] and not f.min_p and list(f.typical_p[0:2]) == [0.5, 0.25]
    with pytest.raises(ValueError):
        make_filters(3, min_p=[0.1, 0.2])
