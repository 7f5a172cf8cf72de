#!/usr/bin/env python3
"""What the sampler's filters cost per draw at V = 65536: rwkv_mi355x_generate[_filtered] on a small
synthetic RWKV-v6 (C 256, L 3, V 65536, Q5_1 -- the sampler's time does not depend on the layers) with
temperature 0.8 and top_p 0.5, for no filter (k_sample, the code object of the parent commit), each
filter alone and all three together (k_sample_f).

One process; per round every variant in turn, so the variants alternate.  Two numbers per variant,
medians over the rounds: the sampler kernel's own time per launch (hipEvent pairs bound to its
dispatches: rwkv_mi355x_set_kernel_timing) and the host-clocked time per generated token of an untimed
call.  Prints one JSON line and a table for profiles/sample_filters_ab.txt."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'rwkv.cppy_amd', 'python'))
import rwkv_cpp  # noqa: E402

VARIANTS = [('none', {}), ('top_k=40', dict(top_k=40)), ('min_p=0.05', dict(min_p=0.05)),
            ('typical_p=0.9', dict(typical_p=0.9)), ('all three', dict(top_k=40, min_p=0.05, typical_p=0.9))]
PROMPT = [11, 2047, 40000, 7, 65535, 300, 1234, 50000]


def sampler_stats(L, ptr):
    """{kernel: (launches, ms)} of the sampler kernels so far."""
    name = ctypes.create_string_buffer(256)
    launches, ms, by, fl = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    out = {}
    for i in range(L.rwkv_mi355x_kernel_stats(ptr, -1, None, 0, None, None, None, None)):
        L.rwkv_mi355x_kernel_stats(ptr, i, name, 256, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(by),
                                   ctypes.byref(fl))
        if name.value.startswith(b'k_sample'):
            out[name.value.decode()] = (launches.value, ms.value)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--tokens', type=int, default=256)
    ap.add_argument('--model-dir', default=os.environ.get('RWKV_BENCH_DIR', '/tmp/rwkv_bench'))
    args = ap.parse_args()
    lib = rwkv_cpp.RWKVSharedLibrary(os.path.join(REPO, 'rwkv.cppy_amd', 'build', 'librwkv.so'))
    L = lib.library
    os.makedirs(args.model_dir, exist_ok=True)
    path = os.path.join(args.model_dir, 'v6-c256-l3-v65536-q5_1-seed11.bin')
    if not os.path.isfile(path):
        assert L.rwkv_mi355x_write_synthetic_model(path.encode(), 6, 65536, 256, 3, 0, b'Q5_1', 11)
    m = rwkv_cpp.RWKVModel(lib, path, gpu_layer_count=99)
    ptr = m._ctx.ptr

    def generate(kw, n):
        m.eval_sequence(PROMPT, None, use_numpy=True)
        t0 = time.perf_counter()
        lib.rwkv_mi355x_generate(m._ctx, n, 0.8, 0.5, None, 1, 0, **kw)
        return (time.perf_counter() - t0) / n * 1e6

    kernel_us = {name: [] for name, _ in VARIANTS}
    token_us = {name: [] for name, _ in VARIANTS}
    for name, kw in VARIANTS:  # warm-up: code objects, graphs
        generate(kw, 16)
    for _ in range(args.rounds):
        for name, kw in VARIANTS:
            token_us[name].append(generate(kw, args.tokens))
            L.rwkv_mi355x_set_kernel_timing(ptr, True)
            before = sampler_stats(L, ptr)
            generate(kw, 64)
            after = sampler_stats(L, ptr)
            L.rwkv_mi355x_set_kernel_timing(ptr, False)
            kernel = 'k_sample_f' if kw else 'k_sample'
            b = before.get(kernel, (0, 0.0))
            assert after[kernel][0] - b[0] == 64, (kernel, before, after)
            kernel_us[name].append((after[kernel][1] - b[1]) * 1e3 / 64)
    m.free()
    result = {name: {'kernel_us': statistics.median(kernel_us[name]), 'kernel_us_runs': kernel_us[name],
                     'token_us': statistics.median(token_us[name]), 'token_us_runs': token_us[name]} for name, _ in VARIANTS}
    print(json.dumps(result))
    base = result['none']
    print(f"{'filters':<16}{'kernel':<14}{'us/launch':>10}{'min..max':>16}{'delta':>9}{'us/token':>10}{'delta':>9}")
    for name, kw in VARIANTS:
        r = result[name]
        runs = r['kernel_us_runs']
        print(f"{name:<16}{'k_sample_f' if kw else 'k_sample':<14}{r['kernel_us']:>10.1f}"
              f"{f'{min(runs):.1f}..{max(runs):.1f}':>16}{r['kernel_us'] - base['kernel_us']:>+9.1f}"
              f"{r['token_us']:>10.1f}{r['token_us'] - base['token_us']:>+9.1f}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
