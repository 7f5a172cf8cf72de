"""rwkv_cpp.constraint on hand-written cases: the numpy restatement the GPU tests compare against."""
import numpy as np

import rwkv_lib  # noqa: F401  (puts the package on the path)
from rwkv_cpp.constraint import DEAD, allowed_mask, from_choices, join, pack_vocab, walk


def test_from_choices_accepts_at_each_complete_choice():
    d = from_choices([b'no', b'north', 'été'.encode()])
    assert d.next.shape == (1 + 5 + 5, 256) and d.next.dtype == np.uint16
    q = walk(d.next, 0, b'no')
    assert q != DEAD and d.accepting[q]                      # a choice that is a prefix of another
    assert not d.accepting[walk(d.next, 0, b'nor')]
    assert d.accepting[walk(d.next, q, b'rth')]
    assert walk(d.next, 0, b'nope') == DEAD and walk(d.next, 0, b'') == 0
    e = 'été'.encode()                                        # c3 a9 74 c3 a9: bytes, not characters
    assert [bool(d.accepting[walk(d.next, 0, e[:i])]) for i in range(1, 6)] == [False] * 4 + [True]


def test_allowed_mask_rules():
    d = from_choices([b'no', b'north'])
    vocab = [b'', b'n', b'no', b'nor', b'x', b'north!', b'o']
    assert list(allowed_mask(d.next, d.accepting, 0, vocab)) == [False, True, True, True, False, False, False]
    q = walk(d.next, 0, b'no')
    # a stop token goes by accepting[q] alone, whatever its bytes: token 4 (b'x') and token 0 (no bytes)
    assert list(allowed_mask(d.next, d.accepting, q, vocab, stops=[4, 0])) == [True, False, False, False, True, False, False]
    assert not allowed_mask(d.next, d.accepting, 0, vocab, stops=[4])[4]
    leaf = walk(d.next, 0, b'north')
    assert not allowed_mask(d.next, d.accepting, leaf, vocab).any()


def test_join_keeps_the_automata_apart():
    a, b = from_choices([b'ab']), from_choices([b'cd', b'c'])
    both, (sa, sb) = join(a, b)
    assert (sa, sb) == (0, 3) and both.next.shape[0] == 3 + 3
    assert walk(both.next, sa, b'ab') == 2 and walk(both.next, sa, b'c') == DEAD
    assert both.accepting[walk(both.next, sb, b'c')] and walk(both.next, sb, b'ab') == DEAD


def test_pack_vocab():
    offsets, data = pack_vocab([b'ab', b'', b'c'])
    assert list(offsets) == [0, 2, 2, 3] and data.tobytes() == b'abc'
