#!/usr/bin/env python3
"""What a byte-DFA constraint costs per draw at V = 65536: k_dfa_mask + k_dfa_advance (constrain.hip)
on a small synthetic RWKV-v6 (C 256, L 3, V 65536, Q5_1 -- the kernels' time does not depend on the
layers), for rows 1 (rwkv_mi355x_generate) and 64 (rwkv_mi355x_generate_batch), a 30-state and a
near-limit table (random, 40 % dead transitions, 256 byte classes), beside the sampler's own time; and
the host-clocked time per token of rwkv_mi355x_generate with the accept-everything automaton against
the same call without a constraint.

One process; per round every variant in turn, so the variants alternate.  Kernel times are hipEvent
pairs bound to the dispatches (rwkv_mi355x_set_kernel_timing), medians over the rounds.  The
vocabulary is synthetic: sorted byte strings of 1 to 24 bytes.  Prints one JSON line and a table for
profiles/constrained_ab.txt.

--resident: the resident table (rwkv_mi355x_constraint_table) instead.  k_dfa_mask (a table
passed with the call) against k_dfa_mask_mem (the same table and one unreachable state more, resident,
which puts it over the LDS limit) and k_dfa_mask_mem at 2045 states x 40 classes and 65534 x 256, for
rows 1 and 64 and two row mixes: every row in a state that two bytes leave (most tokens die on their
first byte) or in a state that every byte leaves (every token is walked to its end).  Both states loop
to themselves, so the mix holds over the steps.  Then the host time of setting the 65534-state table
and of one constrained sample with a 319-state table passed with the call against resident.  --lib
names another build of the library to measure (a kernel variant).  For profiles/constrained_resident_ab.txt."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'rwkv.cppy_amd', 'python'))
import rwkv_cpp  # noqa: E402
from rwkv_cpp.constraint import DEAD, Dfa  # noqa: E402

PROMPT = [11, 2047, 40000, 7, 65535, 300, 1234, 50000]
KERNELS = ('k_dfa_mask', 'k_dfa_mask_mem', 'k_dfa_advance', 'k_sample_rows', 'k_sample')


def stats(L, ptr):
    name = ctypes.create_string_buffer(256)
    launches, ms, by, fl = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    out = {k: (0, 0.0) for k in KERNELS}
    for i in range(L.rwkv_mi355x_kernel_stats(ptr, -1, None, 0, None, None, None, None)):
        L.rwkv_mi355x_kernel_stats(ptr, i, name, 256, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(by),
                                   ctypes.byref(fl))
        if name.value.decode() in out:
            out[name.value.decode()] = (launches.value, ms.value)
    return out


def random_table(n, seed):
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, n, (n, 256)).astype(np.uint16)
    nxt[rng.random((n, 256)) < 0.4] = DEAD
    return nxt, np.ones(n, np.uint8)


def mix_table(n, n_cls, seed):
    """random_table with n_cls byte classes; state 0 is left by the bytes of classes 0 and 1 only (0x61 and
    0x62 among them) and state 1 by every byte, each back to itself."""
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, n, (n, n_cls)).astype(np.uint16)
    cols[rng.random((n, n_cls)) < 0.4] = DEAD
    cols[0] = DEAD
    cols[0, :2] = 0
    cols[1] = 1
    of = np.concatenate([np.arange(n_cls), rng.integers(0, n_cls, 256 - n_cls)])
    of[[0, 1, 0x61, 0x62]] = [of[0x61], of[0x62], 0, 1]
    return np.ascontiguousarray(cols[:, of]), np.ones(n, np.uint8)


def resident(args, lib, m, run, stats):
    L, ptr = lib.library, m._ctx.ptr
    limit = lib.rwkv_mi355x_constraint_max_entries() // 256
    base = mix_table(limit, 256, 2)
    extra = np.concatenate([base[0], np.full((1, 256), DEAD, np.uint16)]), np.ones(limit + 1, np.uint8)
    tables = [(f'{limit} x 256, with the call', base, False), (f'{limit + 1} x 256, resident', extra, True),
              ('2045 x 40, resident', mix_table(2045, 40, 3), True), ('65534 x 256, resident', mix_table(65534, 256, 4), True)]
    set_ms, us = [], {}
    for name, table, res in tables:
        dfa = Dfa(*table)
        if res:
            t0 = time.perf_counter()
            dfa = m.set_constraint_table(*table)
            if table[0].shape[0] == 65534:
                set_ms.append((time.perf_counter() - t0) * 1e3)
        for rows in (1, 64):
            for mix, start in (('first byte', 0), ('every byte', 1)):
                dfa.start = start
                run(rows, dfa, 8)
                samples = {k: [] for k in KERNELS}
                for _ in range(args.rounds):
                    L.rwkv_mi355x_set_kernel_timing(ptr, True)
                    before = stats(L, ptr)
                    run(rows, dfa, 32)
                    after = stats(L, ptr)
                    L.rwkv_mi355x_set_kernel_timing(ptr, False)
                    for k in KERNELS:
                        if after[k][0] - before[k][0]:
                            samples[k].append((after[k][1] - before[k][1]) * 1e3 / (after[k][0] - before[k][0]))
                us[f'{name}; rows {rows}; {mix}'] = {k: statistics.median(v) for k, v in samples.items() if v}
    # one constrained sample, host clock: the table with the call (compressed and uploaded by the call) or resident
    m.eval_sequence(PROMPT, None, use_numpy=True)
    given, res = Dfa(*base), m.set_constraint_table(*base)
    sample_us = {'with the call': [], 'resident': []}
    for i in range(10 + 50 * args.rounds):
        for k, dfa in (('with the call', given), ('resident', res)):
            t0 = time.perf_counter()
            m.sample(seed=i, dfa=dfa)
            if i >= 10:
                sample_us[k].append((time.perf_counter() - t0) * 1e6)
    m.set_constraint_table(None)
    result = {'resident_kernel_us': us, 'set_65534_states_ms': set_ms,
              'sample_us': {k: statistics.median(v) for k, v in sample_us.items()}}
    print(json.dumps(result))
    print(f"{'table; rows; mix':<52}{'k_dfa_mask':>12}{'k_dfa_mask_mem':>16}   us per launch (median of {args.rounds})")
    for name, ks in us.items():
        print(f"{name:<52}{ks.get('k_dfa_mask', float('nan')):>12.1f}{ks.get('k_dfa_mask_mem', float('nan')):>16.1f}")
    print(f'rwkv_mi355x_constraint_table, 65534 states: {set_ms[0]:.1f} ms (host)')
    for k, v in result['sample_us'].items():
        print(f'sample, {limit}-state table {k:<16}{v:>8.1f} us (host, median)')
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--tokens', type=int, default=256)
    ap.add_argument('--model-dir', default=os.environ.get('RWKV_BENCH_DIR', '/tmp/rwkv_bench'))
    ap.add_argument('--resident', action='store_true', help='the resident-table measurements instead')
    ap.add_argument('--lib', default=os.path.join(REPO, 'rwkv.cppy_amd', 'build', 'librwkv.so'))
    args = ap.parse_args()
    lib = rwkv_cpp.RWKVSharedLibrary(args.lib)
    L = lib.library
    os.makedirs(args.model_dir, exist_ok=True)
    path = os.path.join(args.model_dir, 'v6-c256-l3-v65536-q5_1-seed11.bin')
    if not os.path.isfile(path):
        assert L.rwkv_mi355x_write_synthetic_model(path.encode(), 6, 65536, 256, 3, 0, b'Q5_1', 11)
    rng = np.random.default_rng(3)
    vocab = [bytes([t]) for t in range(256)] + sorted(
        rng.integers(0, 256, int(n)).astype(np.uint8).tobytes() for n in rng.integers(2, 25, 65536 - 256))
    m = rwkv_cpp.RWKVModel(lib, path, gpu_layer_count=99, vocab_bytes=vocab)
    ptr = m._ctx.ptr
    limit = lib.rwkv_mi355x_constraint_max_entries() // 256
    tables = {'30 states': random_table(30, 1), f'{limit} states (limit)': random_table(limit, 2)}
    m.batch_reserve(64)
    prompts = [PROMPT[r % 8:] + PROMPT[:r % 8] for r in range(64)]

    def run(rows, table, n):
        dfa = Dfa(*table) if isinstance(table, tuple) else table
        if rows == 1:
            m.eval_sequence(PROMPT, None, use_numpy=True)
            t0 = time.perf_counter()
            lib.rwkv_mi355x_generate(m._ctx, n, 0.8, 0.5, None, 1, 0, dfa=dfa)
        else:
            t0 = time.perf_counter()
            m.generate_batch(prompts, n, temperature=0.8, top_p=0.5, dfa=dfa)
        return (time.perf_counter() - t0) / n * 1e6

    if args.resident:
        return resident(args, lib, m, run, stats)
    cases = [(rows, name) for rows in (1, 64) for name in tables]
    kernel_us = {c: {k: [] for k in KERNELS} for c in cases}
    every = (np.zeros((1, 256), np.uint16), [1])
    token_us = {'unconstrained': [], 'accept everything': []}
    for rows, name in cases:  # warm-up: code objects, graphs
        run(rows, tables[name], 8)
    run(1, None, 16), run(1, every, 16)
    for _ in range(args.rounds):
        token_us['unconstrained'].append(run(1, None, args.tokens))
        token_us['accept everything'].append(run(1, every, args.tokens))
        for rows, name in cases:
            L.rwkv_mi355x_set_kernel_timing(ptr, True)
            before = stats(L, ptr)
            run(rows, tables[name], 32)
            after = stats(L, ptr)
            L.rwkv_mi355x_set_kernel_timing(ptr, False)
            for k in KERNELS:
                launches = after[k][0] - before[k][0]
                if launches:
                    kernel_us[(rows, name)][k].append((after[k][1] - before[k][1]) * 1e3 / launches)
    m.free()
    med = lambda v: statistics.median(v) if v else float('nan')  # noqa: E731
    result = {'kernel_us': {f'rows {r}, {n}': {k: med(v) for k, v in ks.items() if v} for (r, n), ks in kernel_us.items()},
              'token_us': {k: med(v) for k, v in token_us.items()}, 'token_us_runs': token_us}
    print(json.dumps(result))
    print(f"{'rows':<6}{'table':<24}{'k_dfa_mask':>12}{'k_dfa_advance':>15}{'sampler':>10}   us per launch (median of {args.rounds})")
    for (r, n), ks in kernel_us.items():
        print(f"{r:<6}{n:<24}{med(ks['k_dfa_mask']):>12.1f}{med(ks['k_dfa_advance']):>15.1f}{med(ks['k_sample_rows']):>10.1f}")
    for k, v in token_us.items():
        print(f'generate, {k:<20}{med(v):>8.1f} us/token  ({1e6 / med(v):.0f} tok/s; runs {min(v):.1f}..{max(v):.1f})')
    return 0


if __name__ == '__main__':
    sys.exit(main())
