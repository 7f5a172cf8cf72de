#!/usr/bin/env python3
"""Scoring rates on the headline model (synthetic RWKV-v6 C 2048, L 24, V 65536, Q4_0, the file
bench.py writes), tokens per second from a fresh device state:

  score    rwkv_mi355x_score_sequence of T tokens with targets, no logits_out (head on every token)
  eval     rwkv_mi355x_eval_device of the same T tokens, logits on (head on the last token only)
  serial   perplexity.measure over 256 scored tokens (one rwkv_eval per token, cross-entropy in numpy)
  kernels  the matmul kernel classes of one score call of 1024 tokens (rwkv_mi355x_set_kernel_timing:
           event pairs around each matmul group; the head's tiles run under the batched decode's
           class name k_mvb<head type>)

One fresh process per arm; in it one warm-up pass per T, then --reps timed passes (a host clock around
the synchronous call); median, minimum and maximum are reported.  score - eval is the cost of the
all-token head.  --out names the text file written.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'rwkv.cppy_amd', 'python'))
DEFAULT_LIB = os.path.join(REPO, 'rwkv.cppy_amd', 'build', 'librwkv.so')
ARCH, V, C, NL, FMT = 6, 65536, 2048, 24, 'Q4_0'
LENGTHS = (1024, 4096)
SERIAL_TOKENS = 256


def arm(args):
    import rwkv_cpp
    from rwkv_cpp import perplexity
    lib = rwkv_cpp.RWKVSharedLibrary(args.lib)
    L = lib.library
    os.makedirs(args.model_dir, exist_ok=True)
    path = os.path.join(args.model_dir, 'v6-1b6-q4_0-seed1.bin')
    if not os.path.isfile(path):
        assert L.rwkv_mi355x_write_synthetic_model((path + '.tmp').encode(), ARCH, V, C, NL, 0, FMT.encode(), 1)
        os.replace(path + '.tmp', path)
    model = rwkv_cpp.RWKVModel(lib, path, gpu_layer_count=NL + 1)
    ctx = model._ctx
    tokens = [int(t) for t in np.random.default_rng(3).integers(0, V, max(LENGTHS) + 1)]

    def score(T):
        model.reset_state()
        t0 = time.perf_counter()
        lib.rwkv_mi355x_score_sequence(ctx, tokens[:T], tokens[1:T + 1])
        return time.perf_counter() - t0

    def eval_device(T):
        model.reset_state()
        arr = (ctypes.c_int32 * T)(*tokens[:T])
        t0 = time.perf_counter()
        assert L.rwkv_mi355x_eval_device(ctx.ptr, arr, T, True, None, True)
        return time.perf_counter() - t0

    def serial(T):
        t0 = time.perf_counter()
        perplexity.measure(model, tokens[:T + 1])
        return time.perf_counter() - t0

    def timed(run, T):
        run(T)
        times = [run(T) for _ in range(args.reps)]
        return {'tok_per_s': T / statistics.median(times), 'tok_per_s_min': T / max(times),
                'tok_per_s_max': T / min(times), 'ms_median': statistics.median(times) * 1e3}

    out = {}
    if args.arm == 'kernels':
        score(1024)
        L.rwkv_mi355x_set_kernel_timing(ctx.ptr, True)
        score(1024)
        name = ctypes.create_string_buffer(256)
        launches, ms, by, fl = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        count = L.rwkv_mi355x_kernel_stats(ctx.ptr, -1, None, 0, None, None, None, None)
        for i in range(count):
            L.rwkv_mi355x_kernel_stats(ctx.ptr, i, name, 256, ctypes.byref(launches), ctypes.byref(ms),
                                       ctypes.byref(by), ctypes.byref(fl))
            out[name.value.decode()] = {'launches': launches.value, 'ms': ms.value}
        L.rwkv_mi355x_set_kernel_timing(ctx.ptr, False)
    elif args.arm == 'serial':
        out[str(SERIAL_TOKENS)] = timed(serial, SERIAL_TOKENS)
    else:
        for T in LENGTHS:
            out[str(T)] = timed({'score': score, 'eval': eval_device}[args.arm], T)
    model.free()
    print('ARM ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--arms', default='score,eval,serial,kernels')
    ap.add_argument('--arm', default=None, help='(internal) run this one arm in this process')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lib', default=DEFAULT_LIB)
    ap.add_argument('--model-dir', default=os.environ.get('RWKV_BENCH_DIR', '/tmp/rwkv_bench'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'score_sequence.txt'))
    args = ap.parse_args()
    if args.arm:
        return arm(args)
    arms = {}
    for name in args.arms.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--arm', name, '--reps', str(args.reps), '--lib', args.lib,
               '--model-dir', args.model_dir]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
        lines = [l for l in p.stdout.splitlines() if l.startswith('ARM ')]
        if p.returncode or not lines:
            print(f'arm {name} failed (exit {p.returncode})', file=sys.stderr)
            return 1
        arms[name] = json.loads(lines[-1][4:])
        print(name, arms[name], file=sys.stderr, flush=True)
    text = [f'Scoring on the device: synthetic RWKV-v6 C {C} L {NL} V {V} {FMT}, one MI355X.',
            f'tools/bench_score.py: one process per arm, 1 warm-up + {args.reps} timed passes from a fresh state,',
            'host clock around the synchronous call; tokens/s median (min .. max).', '']
    for name in ('score', 'eval', 'serial'):
        for T, r in arms.get(name, {}).items():
            text.append(f'{name:7s} T {int(T):5d}: {r["tok_per_s"]:10.0f} tok/s ({r["tok_per_s_min"]:.0f} .. '
                        f'{r["tok_per_s_max"]:.0f}), {r["ms_median"]:.2f} ms per call')
    if 'score' in arms and 'eval' in arms:
        text.append('')
        for T in arms['score']:
            gap = arms['score'][T]['ms_median'] - arms['eval'][T]['ms_median']
            text.append(f'all-token head, T {int(T)}: {gap:.2f} ms per call = {gap * 1e3 / int(T):.2f} us per token '
                        f'({gap / arms["score"][T]["ms_median"] * 100:.0f}% of the score call)')
    if 'score' in arms and 'serial' in arms:
        r = arms['score'][str(LENGTHS[0])]['tok_per_s'] / arms['serial'][str(SERIAL_TOKENS)]['tok_per_s']
        text.append(f'score (T {LENGTHS[0]}) over the serial loop: {r:.1f}x')
    if 'kernels' in arms:
        text += ['', 'matmul kernel classes of one score call, T 1024 (timing on: eager launches, event pairs):']
        for k, s in sorted(arms['kernels'].items(), key=lambda kv: -kv[1]['ms']):
            text.append(f'  {k:24s} {s["launches"]:6d} launches {s["ms"]:9.3f} ms')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(text) + '\n')
    print('\n'.join(text))
    return 0


if __name__ == '__main__':
    sys.exit(main())
