"""rwkv_cpp.sampling.ngram_draft, the specification of rwkv_mi355x_generate_speculative's draft rule, on
hand-written cases (tests/test_gpu_spec_kernels.py runs the device search on the same ones)."""
import pytest

from rwkv_lib import library  # noqa: F401  (puts the package on the path)
from rwkv_cpp import sampling

# (corpus, k, ngram_min, ngram_max, the draft)
CASES = {
    'length_1': ([5], 4, 1, 4, []),
    'length_2_match': ([5, 5], 4, 1, 4, [5]),
    'length_2_none': ([5, 6], 4, 1, 4, []),
    'overlaps_the_end': ([7, 7, 7], 4, 2, 2, [7]),
    'latest_of_equal': ([1, 2, 9, 1, 2, 8, 1, 2, 7, 1, 2], 4, 1, 2, [7, 1, 2]),
    'longer_earlier_wins': ([3, 1, 2, 50, 9, 2, 60, 1, 2], 4, 1, 3, [50, 9, 2, 60]),
    'short_continuation': ([4, 5, 6, 4], 8, 1, 4, [5, 6, 4]),
    'no_match': ([1, 2, 3, 4], 4, 1, 4, []),
    'below_ngram_min': ([1, 2, 3, 2], 4, 2, 4, []),
    'k_cuts': ([1, 2, 3, 4, 5, 1], 2, 1, 8, [2, 3]),
}


@pytest.mark.parametrize('name', CASES)
def test_ngram_draft(name):
    corpus, k, lo, hi, want = CASES[name]
    assert sampling.ngram_draft(corpus, k, lo, hi) == want
