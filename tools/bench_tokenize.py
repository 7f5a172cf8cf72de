#!/usr/bin/env python3
"""Tokenization rates, the device (RWKVModel.tokenize) beside the Python trie
(WorldTokenizer.encode_bytes), on the World vocabulary and seeded text (ASCII words, CJK and emoji):
64 KB, 1 MB and 16 MB in one text, and 1 MB split into 256 texts.

The model is a one-layer synthetic file with 65536 tokens: tokenization reads the vocabulary only.  Per
size: one warm-up call, then --reps timed calls of RWKVModel.tokenize (a host clock around the
synchronous call, which takes Python bytes and returns Python lists) and of the C call alone on prepared
numpy arrays; encode_bytes on the same bytes in the same process (one call from 1 MB on).  Then one call
with rwkv_mi355x_set_kernel_timing on: the four kernels' own spans.  --out names the text file written.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'rwkv.cppy_amd', 'python'))
VOCAB = os.path.join(REPO, 'tests', 'golden', 'rwkv_vocab_v20230424.txt')
SIZES = (('64 KB, 1 text', 1 << 16, 1), ('1 MB, 1 text', 1 << 20, 1), ('16 MB, 1 text', 1 << 24, 1), ('1 MB, 256 texts', 1 << 20, 256))


def seeded_text(n_bytes, seed=7):
    words = ['the', 'quick', 'brown', 'fox', 'tokenizer', 'of', '\n', '  ', '1234', '3.14', 'RWKV', 'Hello,', 'naïve',
             '你好', '世界', '日本語のテキスト', '한국어', '🙂', '🚀🌍', 'été', '(x + y)', '"quoted"']
    picks = np.random.default_rng(seed).integers(0, len(words), n_bytes // 2)
    return ''.join(words[i] + ' ' * int(i % 3 != 0) for i in picks).encode('utf-8')[:n_bytes]


def kernel_ms(L, ptr):
    name = ctypes.create_string_buffer(256)
    launches, ms, by, fl = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    out = {}
    for i in range(L.rwkv_mi355x_kernel_stats(ptr, -1, None, 0, None, None, None, None)):
        L.rwkv_mi355x_kernel_stats(ptr, i, name, 256, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(by), ctypes.byref(fl))
        out[name.value.decode()] = ms.value
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lib', default=os.path.join(REPO, 'rwkv.cppy_amd', 'build', 'librwkv.so'))
    ap.add_argument('--model-dir', default=os.environ.get('RWKV_BENCH_DIR', '/tmp/rwkv_bench'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'tokenize.txt'))
    args = ap.parse_args()
    import rwkv_cpp
    from rwkv_cpp.world_tokenizer import WorldTokenizer
    lib = rwkv_cpp.RWKVSharedLibrary(args.lib)
    L = lib.library
    os.makedirs(args.model_dir, exist_ok=True)
    path = os.path.join(args.model_dir, 'v4-c64-l1-v65536-fp16-seed3.bin')
    if not os.path.isfile(path):
        assert L.rwkv_mi355x_write_synthetic_model((path + '.tmp').encode(), 4, 65536, 64, 1, 0, b'FP16', 3)
        os.replace(path + '.tmp', path)
    ref = WorldTokenizer(VOCAB)
    model = rwkv_cpp.RWKVModel(lib, path, gpu_layer_count=99, vocab_bytes=ref)
    ptr = model._ctx.ptr
    data = seeded_text(max(s for _, s, _ in SIZES))
    P8, P32, P64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64))
    text = ['Tokenization on the device: World vocabulary (65529 tokens, longest 128 bytes), seeded mixed text, one MI355X.',
            f'tools/bench_tokenize.py: 1 warm-up + {args.reps} timed calls, host clock around the synchronous call; median (min .. max).',
            '']
    for label, size, n_texts in SIZES:
        step = size // n_texts
        texts = [data[i * step:(i + 1) * step] for i in range(n_texts)]
        blob = np.frombuffer(b''.join(texts), np.uint8)
        offsets = np.arange(n_texts + 1, dtype=np.uint64) * step
        tokens, token_off = np.zeros(size, np.uint32), np.zeros(n_texts + 1, np.uint64)

        def c_call():
            t0 = time.perf_counter()
            assert L.rwkv_mi355x_tokenize(ptr, blob.ctypes.data_as(P8), offsets.ctypes.data_as(P64), n_texts,
                                          tokens.ctypes.data_as(P32), token_off.ctypes.data_as(P64), None)
            return time.perf_counter() - t0

        def py_call():
            t0 = time.perf_counter()
            model.tokenize(texts)
            return time.perf_counter() - t0

        def ref_call():
            t0 = time.perf_counter()
            out = [ref.encode_bytes(t) for t in texts]
            return time.perf_counter() - t0, out

        got = model.tokenize(texts)  # the warm-up, and the check
        ref_times, want = zip(*[ref_call() for _ in range(3 if size < (1 << 20) else 1)])
        assert got == want[0], label
        n_tok = sum(len(t) for t in got)
        rows = (('RWKVModel.tokenize', [py_call() for _ in range(args.reps)]),
                ('rwkv_mi355x_tokenize', [c_call() for _ in range(1 + args.reps)][1:]), ('encode_bytes', list(ref_times)))
        text.append(f'{label}: {n_tok} tokens')
        for name, times in rows:
            med = statistics.median(times)
            text.append(f'  {name:22s} {med * 1e3:10.3f} ms ({min(times) * 1e3:.3f} .. {max(times) * 1e3:.3f})  '
                        f'{size / med / 1e6:9.2f} MB/s  {n_tok / med:12.0f} tok/s')
        L.rwkv_mi355x_set_kernel_timing(ptr, True)  # the statistics start from nothing
        call_ms = c_call() * 1e3
        spans = {k: v for k, v in kernel_ms(L, ptr).items() if k.startswith('k_tok_')}
        L.rwkv_mi355x_set_kernel_timing(ptr, False)
        text.append(f'  kernels of one timed call ({call_ms:.3f} ms): ' +
                    ', '.join(f'{k} {v:.3f} ms ({v / call_ms * 100:.1f}%)' for k, v in sorted(spans.items())))
    model.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(text) + '\n')
    print('\n'.join(text))
    return 0


if __name__ == '__main__':
    sys.exit(main())
