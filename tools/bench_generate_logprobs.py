#!/usr/bin/env python3
"""What log-probabilities cost in device generation, on the headline model (synthetic RWKV-v6 C 2048,
L 24, V 65536, Q4_0, the file bench.py writes) with the reference's generation settings (temperature
0.8, top_p 0.5), 256 tokens a pass:

  generate          rwkv_mi355x_generate at this build and, with --parent-lib, at a build of the parent
                    commit: separate processes, alternating, the parent first, --rounds of each
  generate_lp<K>    rwkv_mi355x_generate_logprobs with top_k K = 0, 5, 20
  batch32           rwkv_mi355x_generate_batch over B = 32 rows; batch32_lp5 the same with top_k 5
  k_logprobs_<K>    k_logprobs' own time per launch (hipEvent pairs bound to its dispatches:
                    rwkv_mi355x_set_kernel_timing) inside generate_logprobs, K = 0, 5, 20, and the LP
                    sampler's beside it

One fresh process per leg; in it one warm-up pass, then --reps timed passes, the median reported.  The
entry points are bound by hand, so that the same code measures a build that lacks the new ones.
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
DEFAULT_LIB = os.path.join(REPO, 'rwkv.cppy_amd', 'build', 'librwkv.so')
ARCH, V, C, NL, FMT = 6, 65536, 2048, 24, 'Q4_0'
TEMPERATURE, TOP_P, B = 0.8, 0.5, 32
P_F, P_U, P_D = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)


class Sampling(ctypes.Structure):
    _fields_ = [('temperature', ctypes.c_float), ('top_p', ctypes.c_float), ('n_bias', ctypes.c_uint32),
                ('bias_ids', P_U), ('bias_values', P_F), ('seed', ctypes.c_uint64), ('offset', ctypes.c_uint64)]


class BatchSampling(ctypes.Structure):
    _fields_ = [('temperature', P_F), ('top_p', P_F), ('presence', P_F), ('frequency', P_F),
                ('seed', ctypes.POINTER(ctypes.c_uint64)), ('offset', ctypes.POINTER(ctypes.c_uint64)),
                ('n_bias', ctypes.c_uint32), ('bias_ids', P_U), ('bias_values', P_F), ('n_stop', ctypes.c_uint32),
                ('stop_tokens', P_U), ('keep_counts', ctypes.c_uint32), ('check_every', ctypes.c_uint32)]


class Logprobs(ctypes.Structure):
    _fields_ = [('top_k', ctypes.c_uint32), ('token_logprob', P_D), ('top_ids', P_U), ('top_logprobs', P_D)]


def bind(path):
    L = ctypes.CDLL(path)
    vp, sz, u32, P_I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)
    sig = {'rwkv_init_from_file': ([ctypes.c_char_p, u32, u32], vp), 'rwkv_free': ([vp], None),
           'rwkv_mi355x_state_upload': ([vp, P_F], ctypes.c_bool),
           'rwkv_mi355x_eval_device': ([vp, P_I, sz, ctypes.c_bool, P_F, ctypes.c_bool], ctypes.c_bool),
           'rwkv_mi355x_sync': ([vp], ctypes.c_bool),
           'rwkv_mi355x_write_synthetic_model': ([ctypes.c_char_p, ctypes.c_int, u32, u32, u32, u32, ctypes.c_char_p,
                                                  ctypes.c_uint64], ctypes.c_bool),
           'rwkv_mi355x_generate': ([vp, ctypes.POINTER(Sampling), sz, P_U, P_F], ctypes.c_bool),
           'rwkv_mi355x_batch_reserve': ([vp, sz], ctypes.c_bool), 'rwkv_mi355x_batch_store': ([vp, sz], ctypes.c_bool),
           'rwkv_mi355x_generate_batch': ([vp, sz, ctypes.POINTER(BatchSampling), sz, P_U, P_U, P_U], ctypes.c_bool),
           'rwkv_mi355x_set_kernel_timing': ([vp, ctypes.c_bool], None),
           'rwkv_mi355x_kernel_stats': ([vp, ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_longlong), P_D, P_D,
                                         P_D], ctypes.c_int)}
    for name, (argtypes, restype) in sig.items():
        getattr(L, name).argtypes, getattr(L, name).restype = argtypes, restype
    if hasattr(L, 'rwkv_mi355x_generate_logprobs'):
        P_LP = ctypes.POINTER(Logprobs)
        L.rwkv_mi355x_generate_logprobs.argtypes = sig['rwkv_mi355x_generate'][0] + [P_LP]
        L.rwkv_mi355x_generate_batch_logprobs.argtypes = sig['rwkv_mi355x_generate_batch'][0] + [P_LP]
        L.rwkv_mi355x_generate_logprobs.restype = L.rwkv_mi355x_generate_batch_logprobs.restype = ctypes.c_bool
    return L


def leg(args):
    L = bind(args.lib)
    os.makedirs(args.model_dir, exist_ok=True)
    path = os.path.join(args.model_dir, 'v6-1b6-q4_0-seed1.bin')
    if not os.path.isfile(path):
        assert L.rwkv_mi355x_write_synthetic_model((path + '.tmp').encode(), ARCH, V, C, NL, 0, FMT.encode(), 1)
        os.replace(path + '.tmp', path)
    ctx = L.rwkv_init_from_file(path.encode(), 1, NL + 1)
    assert ctx
    n = args.tokens
    prompt = (ctypes.c_int32 * 8)(*[int(t) for t in np.random.default_rng(3).integers(0, V, 8)])
    p = Sampling(TEMPERATURE, TOP_P, 0, None, None, 1, 0)
    tokens = np.zeros((B, n), np.uint32)

    def logprobs(rows, k):
        keep = (np.zeros((rows, n)), np.zeros((rows, n, max(1, k)), np.uint32), np.zeros((rows, n, max(1, k))))
        lp = Logprobs(k, keep[0].ctypes.data_as(P_D), keep[1].ctypes.data_as(P_U), keep[2].ctypes.data_as(P_D))
        lp._keep = keep
        return lp

    def start():
        assert L.rwkv_mi355x_state_upload(ctx, None)
        assert L.rwkv_mi355x_eval_device(ctx, prompt, 8, True, None, True)

    def generate(k, count=n):
        start()
        lp = logprobs(1, k) if k is not None else None
        t0 = time.perf_counter()
        if k is None:
            assert L.rwkv_mi355x_generate(ctx, ctypes.byref(p), count, tokens.ctypes.data_as(P_U), None)
        else:
            assert L.rwkv_mi355x_generate_logprobs(ctx, ctypes.byref(p), count, tokens.ctypes.data_as(P_U), None, ctypes.byref(lp))
        return time.perf_counter() - t0

    rows_f = [(ctypes.c_float * B)(*[x] * B) for x in (TEMPERATURE, TOP_P)]
    rows_u = [(ctypes.c_uint64 * B)(*range(B)), (ctypes.c_uint64 * B)()]
    bp = BatchSampling(rows_f[0], rows_f[1], None, None, rows_u[0], rows_u[1], 0, None, None, 0, None, 0, 0)
    lengths = np.zeros(B, np.uint32)

    def batch(k):
        start()
        for r in range(B):
            assert L.rwkv_mi355x_batch_store(ctx, r)
        lp = logprobs(B, k) if k is not None else None
        t0 = time.perf_counter()
        a = (ctx, B, ctypes.byref(bp), n, tokens.ctypes.data_as(P_U), lengths.ctypes.data_as(P_U), None)
        assert L.rwkv_mi355x_generate_batch(*a) if k is None else L.rwkv_mi355x_generate_batch_logprobs(*a, ctypes.byref(lp))
        return time.perf_counter() - t0

    def kernel_us(k):
        L.rwkv_mi355x_set_kernel_timing(ctx, True)
        generate(k, 64)
        L.rwkv_mi355x_sync(ctx)
        name = ctypes.create_string_buffer(256)
        launches, ms, by, fl = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        us = {}
        for i in range(L.rwkv_mi355x_kernel_stats(ctx, -1, None, 0, None, None, None, None)):
            L.rwkv_mi355x_kernel_stats(ctx, i, name, 256, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(by),
                                       ctypes.byref(fl))
            if name.value in (b'k_logprobs', b'k_sample_lp') and launches.value:
                us[name.value.decode()] = ms.value * 1e3 / launches.value
        L.rwkv_mi355x_set_kernel_timing(ctx, False)
        assert 'k_logprobs' in us, 'no k_logprobs launches in the kernel statistics'
        return us

    name = args.leg
    if name.startswith('k_logprobs_'):
        k = int(name.rsplit('_', 1)[1])
        kernel_us(k)
        runs = [kernel_us(k) for _ in range(args.reps)]
        out = {f'{key}_us': statistics.median(r[key] for r in runs) for key in runs[0]}
    else:
        k = int(name.split('_lp')[1]) if '_lp' in name else None
        if name.startswith('batch32'):
            assert L.rwkv_mi355x_batch_reserve(ctx, B)
        run = (lambda: batch(k)) if name.startswith('batch32') else (lambda: generate(k))
        run()
        times = [run() for _ in range(args.reps)]
        rows = B if name.startswith('batch32') else 1
        out = {'tok_per_s': rows * n / statistics.median(times), 'us_per_step': statistics.median(times) / n * 1e6,
               'us_per_step_runs': [t / n * 1e6 for t in times]}
    L.rwkv_free(ctx)
    print('LEG ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--leg', default=None, help='(internal) run this one leg in this process')
    ap.add_argument('--tokens', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3, help='processes of each build in the generate comparison')
    ap.add_argument('--lib', default=DEFAULT_LIB)
    ap.add_argument('--parent-lib', default=None, help='a build of the parent commit (the generate comparison)')
    ap.add_argument('--model-dir', default=os.environ.get('RWKV_BENCH_DIR', '/tmp/rwkv_bench'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'generate_logprobs_bench.json'))
    args = ap.parse_args()
    if args.leg:
        return leg(args)

    def run(name, lib):
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', name, '--tokens', str(args.tokens), '--reps',
               str(args.reps), '--lib', lib, '--model-dir', args.model_dir]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
        lines = [l for l in p.stdout.splitlines() if l.startswith('LEG ')]
        if p.returncode or not lines:
            raise SystemExit(f'leg {name} failed (exit {p.returncode})')
        out = json.loads(lines[-1][4:])
        print(name, os.path.relpath(lib, REPO), out, file=sys.stderr, flush=True)
        return out

    result = {'model': f'synthetic RWKV-v6 C {C} L {NL} V {V} {FMT}', 'temperature': TEMPERATURE, 'top_p': TOP_P,
              'tokens': args.tokens, 'reps': args.reps, 'legs': {}}
    legs = result['legs']
    legs['generate_parent'], legs['generate'] = [], []
    for _ in range(args.rounds):
        if args.parent_lib:
            legs['generate_parent'].append(run('generate', args.parent_lib))
        legs['generate'].append(run('generate', args.lib))
    for name in ('generate_lp0', 'generate_lp5', 'generate_lp20', 'batch32', 'batch32_lp5', 'k_logprobs_0', 'k_logprobs_5',
                 'k_logprobs_20'):
        legs[name] = run(name, args.lib)
    med = lambda runs: statistics.median(r['us_per_step'] for r in runs)  # noqa: E731
    result['generate_us_per_token'] = med(legs['generate'])
    if legs['generate_parent']:
        result['generate_parent_us_per_token'] = med(legs['generate_parent'])
        result['generate_parent_spread_us'] = [min(r['us_per_step'] for r in legs['generate_parent']),
                                               max(r['us_per_step'] for r in legs['generate_parent'])]
    for k in (0, 5, 20):
        result[f'logprobs_{k}_cost_us_per_token'] = legs[f'generate_lp{k}']['us_per_step'] - result['generate_us_per_token']
    result['batch32_logprobs_5_cost_us_per_step'] = legs['batch32_lp5']['us_per_step'] - legs['batch32']['us_per_step']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))
    return 0


if __name__ == '__main__':
    sys.exit(main())
