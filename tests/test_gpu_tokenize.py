"""Tokenization on the device (rwkv_mi355x_tokenize, csrc/tokenize.hip) against
rwkv_cpp.world_tokenizer.WorldTokenizer.encode_bytes on the same vocabulary: a hand-made vocabulary on a
512-token model (fallbacks, text and tile boundaries, duplicates, no match, the argument errors) and the
World vocabulary on a 65536-token model.  Ids and offsets: everything is compared exactly."""
import ctypes
import functools
import os

import numpy as np
import pytest

from rwkv_lib import library, RWKVModel
from rwkv_cpp.rwkv_cpp_shared_library import TOKENIZE_TILE as TILE
from rwkv_cpp.world_tokenizer import WorldTokenizer

pytestmark = pytest.mark.gpu

RWKV_ERROR_ARGS = 1 << 8
WORLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rwkv_vocab_v20230424.txt')


def long_token(lmax):
    return bytes(range(1, lmax + 1))  # holds b'abcde' when lmax >= 101


def vocab(lmax, no_ff=False):
    """512 tokens: the single bytes (without 0xFF: no_ff), a few words, one token of lmax bytes, b'ab'
    twice (ids 256 and 262) and ids without bytes."""
    v = [bytes([b]) for b in range(256)] + [b'ab', b'abcd', b'abcde', b'bc', b'cdx', long_token(lmax), b'ab']
    v += [b''] * (512 - len(v))
    if no_ff:
        v[255] = b''
    return v


def seeded_text(n_bytes, seed=7):
    """ASCII words, CJK and emoji, mixed by a seeded generator and cut at n_bytes."""
    words = ['the', 'quick', 'brown', 'fox', 'tokenizer', 'of', '\n', '  ', '1234', '3.14', 'RWKV', 'Hello,', 'naïve',
             '你好', '世界', '日本語のテキスト', '한국어', '🙂', '🚀🌍', 'été', '(x + y)', '"quoted"']
    picks = np.random.default_rng(seed).integers(0, len(words), n_bytes // 2)
    return ''.join(words[i] + ' ' * int(i % 3 != 0) for i in picks).encode('utf-8')[:n_bytes]


@functools.lru_cache(maxsize=None)
def setup(kind, tmp):
    """(model, reference) for 'world' or (lmax, no_ff): a one-layer model of n_embed 64 that knows the
    vocabulary's bytes, and a WorldTokenizer filled from the same list as its __init__ fills it."""
    ref = WorldTokenizer.__new__(WorldTokenizer)
    if kind == 'world':
        ref.__init__(WORLD)
        n_vocab = 65536
    else:
        n_vocab = 512
        ref.index_to_token, ref.root = dict(enumerate(vocab(*kind))), {}
        for idx, tok in ref.index_to_token.items():
            node = ref.root
            for ch in tok:
                node = node.setdefault(ch, {})
            node[-1] = idx
    path = os.path.join(tmp, f'tok{n_vocab}.bin')
    assert library().library.rwkv_mi355x_write_synthetic_model(path.encode(), 4, n_vocab, 64, 1, 0, b'FP16', 3)
    return RWKVModel(library(), path, gpu_layer_count=99, vocab_bytes=ref), ref


@pytest.fixture(scope='module')
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp('tokenize'))


def tile_texts(lmax):
    """Repeats of the lmax-byte token from every shift, in lengths around one tile and over three."""
    run = long_token(lmax) * (4 * TILE // lmax + 3)
    return [run[s:s + n] for s in range(lmax) for n in (TILE - 1, TILE, TILE + 1, 3 * TILE + lmax)]


CASES = {
    'fallback': lambda lmax: [b'abcdx', b'abcx', b'abcdabcde'],
    'mid_path': lambda lmax: [b'abc', b'abcdabc', b'cd', long_token(lmax)[:-1], long_token(lmax) + long_token(lmax)[:1]],
    'boundaries': lambda lmax: [b'', b'a', b'bcd', b'ab', b'', b'cde', b'abc', b'dx', b'abcd', b'e', long_token(lmax)[:-1],
                                long_token(lmax)[-1:], b''],
    'duplicates': lambda lmax: [b'abab', b'xab', b'ab'],
    'tiles': tile_texts,
}


@pytest.mark.parametrize('lmax', [8, 200])
@pytest.mark.parametrize('case', list(CASES))
def test_hand_made_vocabulary_equals_encode_bytes(case, lmax, tmp):
    model, ref = setup((lmax, False), tmp)
    texts = CASES[case](lmax)
    want = [ref.encode_bytes(t) for t in texts]
    assert model.tokenize(texts) == want
    if case == 'duplicates':
        assert want[0] == [262, 262]
    if case == 'tiles':
        assert any(257 in w or 258 in w for w in want) == (lmax == 200) and all(261 in w for w in want)


def test_world_vocabulary_equals_encode_bytes(tmp):
    model, ref = setup('world', tmp)
    data = seeded_text(200_000)
    cuts = [0] + sorted(np.random.default_rng(11).integers(0, len(data), 63).tolist()) + [len(data)]
    texts = [data[a:b] for a, b in zip(cuts, cuts[1:])]
    got = model.tokenize(texts)
    for i, t in enumerate(texts):
        assert got[i] == ref.encode_bytes(t), i
    assert model.tokenize(['🙂 naïve 你好']) == [ref.encode('🙂 naïve 你好')]  # str goes as UTF-8


def raw_call(model, data, offsets, n_texts, null=None):
    """The C call with filled outputs: (ok, last error, error_at, tokens, token_offsets)."""
    L, ptr = library().library, model._ctx.ptr
    blob = np.frombuffer(data + b'\0', np.uint8)
    off = np.array(offsets, np.uint64)
    tokens, token_off = np.full(max(len(data), 1), 0xA5A5A5A5, np.uint32), np.full(len(offsets), 7, np.uint64)
    at = ctypes.c_uint64(99)
    P8, P32, P64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64))
    args = {'bytes': blob.ctypes.data_as(P8), 'offsets': off.ctypes.data_as(P64), 'tokens_out': tokens.ctypes.data_as(P32),
            'token_offsets_out': token_off.ctypes.data_as(P64)}
    if null:
        args[null] = None
    ok = L.rwkv_mi355x_tokenize(ptr, args['bytes'], args['offsets'], n_texts, args['tokens_out'], args['token_offsets_out'],
                                ctypes.byref(at))
    return ok, L.rwkv_get_last_error(ptr), at.value, tokens, token_off


@pytest.mark.parametrize('where', ['near', 'third_tile'])
def test_no_match_reports_the_reference_offset_and_writes_nothing(where, tmp):
    model, ref = setup((8, True), tmp)
    pad = long_token(8) * (2 * TILE // 8 + 1) if where == 'third_tile' else b''
    texts = [b'abc', b'', pad + b'ab\xffcd', b'\xff']
    starts = np.cumsum([0] + [len(t) for t in texts]).tolist()
    with pytest.raises(ValueError) as e:
        ref.encode_bytes(texts[2])
    want = starts[2] + int(str(e.value).rsplit(' ', 1)[1])
    assert want == starts[2] + len(pad) + 2
    ok, err, at, tokens, token_off = raw_call(model, b''.join(texts), starts, len(texts))
    assert not ok and err == RWKV_ERROR_ARGS and at == want
    assert np.all(tokens == 0xA5A5A5A5) and np.all(token_off == 7)
    with pytest.raises(ValueError) as e:
        model.tokenize(texts)
    assert (e.value.text, e.value.offset) == (2, len(pad) + 2)


@pytest.mark.parametrize('bad', ['bytes', 'offsets', 'tokens_out', 'token_offsets_out', 'decreasing', 'no_texts', 'too_many_texts',
                                 'too_many_bytes', 'no_vocabulary', 'long_token'])
def test_argument_errors(bad, tmp):
    model, _ = setup((8, False), tmp)
    offsets, n = [0, 2, 5], 2
    if bad == 'decreasing':
        offsets = [0, 3, 2]
    elif bad == 'no_texts':
        n = 0
    elif bad == 'too_many_texts':
        offsets, n = [0] * 65538, 65537
    elif bad == 'too_many_bytes':
        offsets = [0, 2, (1 << 28) + 1]
    elif bad in ('no_vocabulary', 'long_token'):
        model = RWKVModel(library(), os.path.join(tmp, 'tok512.bin'), gpu_layer_count=99)
        if bad == 'long_token':
            model.set_vocab_bytes([b'x' * 256] + [b'y'] * 511)
    ok, err, at, tokens, token_off = raw_call(model, b'abcde', offsets, n, null=bad if bad in ('bytes', 'offsets', 'tokens_out',
                                                                                               'token_offsets_out') else None)
    assert not ok and err == RWKV_ERROR_ARGS and at == 99
    assert np.all(tokens == 0xA5A5A5A5) and np.all(token_off == 7)
    if model is not setup((8, False), tmp)[0]:
        model.free()
