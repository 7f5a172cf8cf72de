"""The host side of device sampling: sampling.uniform reproduces the sampler's counter-based draw
(known answers computed independently), and sampling.sample_probs_u is sample_probs with the draw
given -- the same filtering, the same errors."""
import numpy as np
import pytest

from rwkv_lib import RWKVModel  # noqa: F401  (puts the package on sys.path)
from rwkv_cpp import sampling


def test_uniform_known_answers():
    assert sampling.splitmix64(0, 0) == 0xe220a8397b1dcdaf
    assert sampling.splitmix64(0, 1) == 0x6e789e6aa1b965f4
    assert sampling.splitmix64(1234567, 0) == 0x599ed017fb08fc85
    assert [sampling.uniform(42, i) for i in range(3)] == [0.7415648698806763, 0.1599103808403015,
                                                          0.27860110998153687]
    for i in range(200):
        u = sampling.uniform(7, i)
        assert 0.0 <= u < 1.0 and u == float(np.float32(u))
    # counters and seeds wrap modulo 2^64
    assert sampling.uniform(3, (1 << 64) - 1) == sampling.uniform(3, -1)


class _Searchsorted:
    """np.random.choice with the uniform draw fixed to u."""

    def __init__(self, u):
        self.u = u

    def choice(self, a, p):
        cdf = np.cumsum(p)
        return int(cdf.searchsorted(self.u * cdf[-1], side='right'))


@pytest.mark.parametrize('temperature,top_p,bias', [(1.0, 0.8, None), (0.8, 0.5, None), (1.5, 0.95, {3: 2.0, 17: -4.0}),
                                                    (0.0, 0.8, {5: 30.0}), (1.0, 0.0, None), (1.0, 1.0, None)])
def test_sample_probs_u_is_sample_probs_with_the_draw_given(temperature, top_p, bias):
    rng = np.random.default_rng(5)
    for V in (1, 7, 300):
        probs = sampling.softmax(rng.normal(0, 3, V).astype(np.float32))
        if bias and max(bias) >= V:
            continue
        for u in [0.0, 0.25, 0.5, 0.999, float(np.float32(1 - 2.0 ** -24))] + list(rng.random(8)):
            got = sampling.sample_probs_u(probs, u, temperature, top_p, bias)
            want = sampling.sample_probs(probs, temperature, top_p, bias, _Searchsorted(u))
            assert got == want
            assert 0 <= got < V


def test_sample_probs_u_raises_like_sample_probs():
    probs = sampling.softmax(np.arange(8, dtype=np.float32))
    for kw in ({'temperature': -0.5}, {'temperature': float('nan')}, {'top_p': 1.5}, {'top_p': -0.1}):
        with pytest.raises(ValueError) as a:
            sampling.sample_probs(probs, **kw)
        with pytest.raises(ValueError) as b:
            sampling.sample_probs_u(probs, 0.5, **kw)
        assert str(a.value) == str(b.value)


def test_sample_probs_u_covers_the_kept_set():
    """Sweeping u over [0, 1) visits exactly the tokens the top-p filter keeps, in index order."""
    probs = np.array([0.05, 0.4, 0.05, 0.3, 0.2], np.float32)
    seen = [sampling.sample_probs_u(probs, u, 1.0, 0.8) for u in np.linspace(0, 0.999, 200)]
    assert sorted(set(seen)) == [1, 3, 4]
    assert seen == sorted(seen)
