"""k_xent (csrc/xent.hip) alone, through rwkv_mi355x_selftest_xent: per logits row the cross-entropy of
a target and the argmax, against perplexity.cross_entropy (float64 numpy) and np.argmax on the same
fp32 inputs.

Tolerance: argmax equal; |loss - ref| <= 1e-9 absolute.  Derived, not measured: the terms of S are
positive and each carries <= 2 ulp of fp64 exp error, summation adds <= (tree depth) * 2^-53, so S is
off by ~1e-14 relative on either side; m and l[target] enter exactly; for |values| <= 100 the
difference is ~1e-13.  1e-9 leaves four orders of margin and still catches any fp32 shortcut (~1e-6).
"""
import numpy as np
import pytest

from rwkv_lib import library
from rwkv_cpp.perplexity import cross_entropy

pytestmark = pytest.mark.gpu
TOL = 1e-9

# (V, rows): V = 1 gives loss exactly 0; 259 rows start unaligned and hold less than one pass; 1000 is
# aligned but no power of two; 65537 leaves the second row unaligned; 262144 is beyond what the
# workgroup holds in registers
SHAPES = [(1, 1), (2, 1), (2, 3), (3, 1), (3, 3), (259, 3), (1000, 3), (4096, 1), (4096, 5), (65536, 2), (65537, 2),
          (262144, 1)]


def make_logits(V, rows, seed=0):
    return (np.random.default_rng(1000 * seed + V + rows).standard_normal((rows, V)) * 4).astype(np.float32)


def reference(logits, targets):
    return (np.array([cross_entropy(row, int(t)) for row, t in zip(logits, targets)], np.float64),
            np.argmax(logits, axis=1).astype(np.uint32))


def check(logits, targets):
    loss, amax = library().rwkv_mi355x_selftest_xent(logits, targets)
    want_loss, want_amax = reference(logits, targets)
    err = np.abs(loss - want_loss).max()
    print(f'V {logits.shape[1]} rows {logits.shape[0]}: max |loss - ref| = {err:.3e}')
    assert np.array_equal(amax, want_amax)
    assert err <= TOL, (loss, want_loss)
    return loss, amax


@pytest.mark.parametrize('V,rows', SHAPES)
def test_loss_and_argmax_match_numpy(V, rows):
    logits = make_logits(V, rows)
    rng = np.random.default_rng(V)
    for targets in (np.zeros(rows), np.full(rows, V - 1), np.argmax(logits, axis=1), rng.integers(0, V, rows)):
        loss, _ = check(logits, targets.astype(np.uint32))
        if V == 1:
            assert np.array_equal(loss, np.zeros(rows))


def test_max_subtraction_with_shifted_rows():
    logits = make_logits(4096, 3, seed=1)
    logits[0] += 80.0
    logits[2] -= 80.0
    check(logits, np.array([5, 4095, 17], np.uint32))


@pytest.mark.parametrize('V', [259, 65536, 262144])
def test_lowest_index_wins_a_tied_maximum(V):
    logits = make_logits(V, 2, seed=2)
    top = np.float32(logits.max() + 1.0)
    ties = [[V // 3, V // 2 + 1, V - 1], [7, 130, V - 2]]
    for r in range(2):
        logits[r, ties[r]] = top
    _, amax = check(logits, np.array([0, V - 1], np.uint32))
    assert list(amax) == [ties[0][0], ties[1][0]]


def test_a_call_is_a_pure_function_of_its_inputs():
    logits = make_logits(65537, 2, seed=3)
    targets = np.array([1, 65536], np.uint32)
    a = library().rwkv_mi355x_selftest_xent(logits, targets)
    b = library().rwkv_mi355x_selftest_xent(logits, targets)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


def test_non_finite_rows_return_and_leave_their_neighbours_right():
    logits = make_logits(4099, 4, seed=4)
    logits[1, 77] = np.inf
    logits[2, 3000] = np.nan
    targets = np.array([3, 4, 5, 4098], np.uint32)
    loss, amax = library().rwkv_mi355x_selftest_xent(logits, targets)
    want_loss, want_amax = reference(logits[[0, 3]], targets[[0, 3]])
    assert np.array_equal(amax[[0, 3]], want_amax)
    assert np.abs(loss[[0, 3]] - want_loss).max() <= TOL
