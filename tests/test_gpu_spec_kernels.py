"""The kernels of rwkv_mi355x_generate_speculative (csrc/spec.hip) on host operands: the draft search
against rwkv_cpp.sampling.ngram_draft, and the accept / commit pair behind the rows' sampler."""
import numpy as np
import pytest

from rwkv_lib import library
from rwkv_cpp import sampling
from test_speculative_cpu import CASES

pytestmark = pytest.mark.gpu

BIG = (1 << 20) - 1


@pytest.mark.parametrize('name', CASES)
def test_draft_small(name):
    corpus, k, lo, hi, _ = CASES[name]
    assert library().rwkv_mi355x_selftest_spec_draft(corpus, k, lo, hi) == sampling.ngram_draft(corpus, k, lo, hi)


@pytest.mark.parametrize('plants', [[(100, 3, 777)], [(100, 3, 777), (BIG - 2000, 3, 888)], [(100, 4, 777), (BIG - 2000, 3, 888)]],
                         ids=['first_share', 'last_share_is_later', 'first_share_is_longer'])
def test_draft_largest_corpus(plants):
    """Distinct tokens but for the planted copies of the end's n-gram: (position, length, the token behind)."""
    corpus = np.arange(10, 10 + BIG, dtype=np.uint32)
    corpus[-4:] = [2, 3, 4, 5]
    for at, g, behind in plants:
        corpus[at:at + g] = corpus[BIG - g:]
        corpus[at + g] = behind
    want = sampling.ngram_draft(corpus, 4, 1, 4)[:1]  # one token is all the call still wants
    assert want == [plants[-1][2] if plants[-1][1] >= plants[0][1] else plants[0][2]]
    assert library().rwkv_mi355x_selftest_spec_draft(corpus, 4, 1, 4, limit=1) == want


def committed(trace_entry, arch, n_layer, H, S):
    """The state a trace entry stands for: WKV-6 heads are value-major in the trace."""
    if arch not in (5, 6):
        return trace_entry
    C = H * S
    e = trace_entry.reshape(n_layer, C * (2 + S)).copy()
    heads = e[:, 2 * C:].reshape(n_layer, H, S, S)
    e[:, 2 * C:] = heads.transpose(0, 1, 3, 2).reshape(n_layer, -1)
    return e.reshape(-1)


@pytest.mark.parametrize('arch, H, S', [(4, 3, 8), (6, 2, 64), (6, 3, 8), (7, 2, 16)])
@pytest.mark.parametrize('d, m', [(1, 0), (1, 1), (15, 0), (15, 7), (15, 15)])
def test_accept_commit(d, m, arch, H, S):
    V, n_layer, kw = 301, 2, dict(temperature=1.0, top_p=0.8)
    seed, offset = 5, 100
    rng = np.random.default_rng(d * 16 + m)
    logits = (rng.standard_normal((d + 1, V)) * 3).astype(np.float32)
    u = [sampling.uniform(seed, offset + r) for r in range(d + 1)]
    draws = library().rwkv_mi355x_selftest_sample(logits, u, **kw)[0]
    drafts = draws[:d].copy()
    if m < d:
        drafts[m] = (drafts[m] + 1) % V
    C = H * S
    state_len = n_layer * (5 * C if arch == 4 else C * (2 + S))
    trace = np.arange((d + 1) * state_len, dtype=np.float32).reshape(d + 1, state_len)  # distinct, exact
    got_m, appended, x0, state, row = library().rwkv_mi355x_selftest_spec_accept(
        logits, drafts, arch, n_layer, H, S, trace, seed=seed, offset=offset, **kw)
    assert got_m == m and x0 == draws[m]
    assert list(appended) == list(drafts[:m]) + [0xFFFFFFFF] * (d - m)
    assert np.array_equal(state, committed(trace[m], arch, n_layer, H, S))
    assert np.array_equal(row.view(np.uint32), logits[m].view(np.uint32))
