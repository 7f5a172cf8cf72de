"""The token layouts of the serial WKV kernels against each other, bit for bit, through
rwkv_mi355x_selftest_wkv_layouts.

Every serial recurrence (WKV-4, WKV-6 with a per-channel or a per-token decay, WKV-7) is one kernel
over a token span (csrc/wkv_span.hpp): one sequence, the contexts of a batched decode step (WKV-4
only), or the segments of a packed chunk.  A span's result must be the one-sequence kernel's on the
same tokens and state, word for word, so no tolerance: the differing words are 0.

The entry point draws the operands from the seed and runs (a) one one-sequence launch per segment,
(b) one segmented launch over the packed rows, (c) for WKV-4 with every length 1, the contexts
form.  Every form's outputs start as a poison word of its own, so a row nobody wrote is a
difference, and the compared count must be every output word: sum(lens) * C plus the state words
the kernel writes per segment (WKV-4: aa, bb, pp = 3 C; otherwise H S S).

Lengths: a lone token, the 16-token chunk of WKV-4 / WKV-7 and 17, the 64-token chunk of WKV-6 and
65.  Shapes: WKV-4 at C = 128 (one wave per 64 channels, k_wkv4_seq, in the segmented launch;
k_wkv4 for the lone tokens of (a)) and C = 96 (k_wkv4, the last wave half empty); kinds 5, 6, 7 at
two heads of 8, 32 (the per-lane key-group kernels) and 64 (the staged kernels).
"""
import pytest
import torch  # noqa: F401  before librwkv initialises HIP (torch's own HIP runtime must come up first)

from rwkv_lib import library

pytestmark = pytest.mark.gpu

LENS = [1, 3, 16, 17, 64, 65, 2, 1]


def check(kind, H, S, lens, ctx=False):
    C = H * S
    state_words = 3 * C if kind == 4 else H * S * S
    total = sum(lens) * C + len(lens) * state_words
    d = library().rwkv_mi355x_selftest_wkv_layouts(kind, H, S, lens, seed=1000 * kind + S)
    print(f'kind {kind} H {H} S {S}: {d}')
    assert d['compared_seg'] == total
    assert d['y_seg'] == 0 and d['state_seg'] == 0
    assert d['compared_ctx'] == (total if ctx else 0)
    assert d['y_ctx'] == 0 and d['state_ctx'] == 0


@pytest.mark.parametrize('H,S', [(2, 64), (3, 32)], ids=['C128', 'C96'])
def test_wkv4_segments(H, S):
    check(4, H, S, LENS)


@pytest.mark.parametrize('H,S', [(2, 64), (3, 32)], ids=['C128', 'C96'])
def test_wkv4_contexts(H, S):
    check(4, H, S, [1] * len(LENS), ctx=True)


@pytest.mark.parametrize('S', [8, 32, 64])
@pytest.mark.parametrize('kind', [5, 6, 7])
def test_wkv67_segments(kind, S):
    check(kind, 2, S, LENS)
