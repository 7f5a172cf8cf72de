#!/usr/bin/env python3
"""Time to fill B generation slots from B prompts on the headline model (synthetic RWKV-v6 C 2048,
L 24, V 65536, Q4_0, the file bench.py writes).

  a  the per-prompt loop -- rwkv_mi355x_state_upload(NULL), rwkv_mi355x_eval_device(prompt),
     rwkv_mi355x_batch_store(slot), one synchronisation at the end -- on a build of the PARENT commit
     (--parent-tree: a checkout of it with its library built; the leg is left out without one)
  b  the same loop on this build
  c  rwkv_mi355x_prefill_batch
  d  (B = 1 only) a bare rwkv_mi355x_eval_device of the prompt on this build

Grid: B in 1, 8, 32, 128, 256 x prompt length in 8, 64, 512; one ragged set (B = 128, lengths uniform
in [1, 256], seed 7); B = 1 with 1024 tokens.  One fresh process per (leg, point); in it one warm-up
pass, then --reps timed passes, the median reported and every pass listed.  c / a is reported at
every point, and called real only when the medians differ by more than the spread (max - min) of a's
own passes.  --out names the JSON file written.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH, V, C, NL, FMT = 6, 65536, 2048, 24, 'Q4_0'
GRID = [(B, n) for B in (1, 8, 32, 128, 256) for n in (8, 64, 512)] + [(128, 'ragged'), (1, 1024)]


def point_lengths(B, n):
    if n == 'ragged':
        return [int(x) for x in np.random.default_rng(7).integers(1, 257, B)]
    return [int(n)] * B


def leg(args):
    tree = args.parent_tree if args.leg == 'a' else REPO
    sys.path.insert(0, os.path.join(tree, 'rwkv.cppy_amd', 'python'))
    import rwkv_cpp
    lib = rwkv_cpp.RWKVSharedLibrary(os.path.join(tree, 'rwkv.cppy_amd', 'build', 'librwkv.so'))
    L = lib.library
    os.makedirs(args.model_dir, exist_ok=True)
    path = os.path.join(args.model_dir, 'v6-1b6-q4_0-seed1.bin')
    if not os.path.isfile(path):
        assert L.rwkv_mi355x_write_synthetic_model((path + '.tmp').encode(), ARCH, V, C, NL, 0, FMT.encode(), 1)
        os.replace(path + '.tmp', path)
    ctx = lib.rwkv_init_from_file(path, 1, NL + 1)
    B = args.rows
    lengths = point_lengths(B, 'ragged' if args.length < 0 else args.length)
    rng = np.random.default_rng(3)
    prompts = [[int(t) for t in rng.integers(0, V, n)] for n in lengths]
    if args.leg != 'd':
        lib.rwkv_mi355x_batch_reserve(ctx, B)

    def loop():
        t0 = time.perf_counter()
        for r in range(B):
            assert L.rwkv_mi355x_state_upload(ctx.ptr, None)
            lib.rwkv_mi355x_eval_device(ctx, prompts[r])
            lib.rwkv_mi355x_batch_store(ctx, r)
        assert L.rwkv_mi355x_sync(ctx.ptr)
        return time.perf_counter() - t0

    def prefill():
        t0 = time.perf_counter()
        lib.rwkv_mi355x_prefill_batch(ctx, prompts, list(range(B)))
        return time.perf_counter() - t0

    def bare():
        assert L.rwkv_mi355x_state_upload(ctx.ptr, None)
        t0 = time.perf_counter()
        lib.rwkv_mi355x_eval_device(ctx, prompts[0])
        assert L.rwkv_mi355x_sync(ctx.ptr)
        return time.perf_counter() - t0

    run = {'a': loop, 'b': loop, 'c': prefill, 'd': bare}[args.leg]
    run()
    times = [run() for _ in range(args.reps)]
    out = {'ms': statistics.median(times) * 1e3, 'ms_runs': [round(t * 1e3, 3) for t in times],
           'tok_per_s': sum(lengths) / statistics.median(times)}
    if args.kernel_stats:
        # one more pass with kernel timing on: the per-kernel-class times of this leg
        L.rwkv_mi355x_set_kernel_timing(ctx.ptr, True)
        run()
        import ctypes
        stats = {}
        for i in range(L.rwkv_mi355x_kernel_stats(ctx.ptr, -1, None, 0, None, None, None, None)):
            name, launches, ms = ctypes.create_string_buffer(128), ctypes.c_longlong(), ctypes.c_double()
            L.rwkv_mi355x_kernel_stats(ctx.ptr, i, name, len(name), ctypes.byref(launches), ctypes.byref(ms), None, None)
            stats[name.value.decode()] = {'launches': launches.value, 'ms': round(ms.value, 3)}
        out['kernel_stats'] = stats
        L.rwkv_mi355x_set_kernel_timing(ctx.ptr, False)
    lib.rwkv_free(ctx)
    print('LEG ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--legs', default='a,b,c')
    ap.add_argument('--points', default='', help='"B:length,..." (length "ragged" allowed); empty: the whole grid')
    ap.add_argument('--leg', default=None, help='(internal) run this one leg in this process')
    ap.add_argument('--rows', type=int, default=8, help='(internal) the point\'s B')
    ap.add_argument('--length', type=int, default=8, help='(internal) the point\'s prompt length, -1: ragged')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--kernel-stats', action='store_true', help='add a pass with kernel timing on and its per-kernel times')
    ap.add_argument('--parent-tree', default=os.environ.get('RWKV_PARENT_TREE', ''),
                    help='a checkout of the parent commit with rwkv.cppy_amd/build/librwkv.so built (leg a)')
    ap.add_argument('--model-dir', default=os.environ.get('RWKV_BENCH_DIR', '/tmp/rwkv_bench'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'prefill_batch_bench.json'))
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    grid = GRID
    if args.points:
        grid = [(int(p.split(':')[0]), p.split(':')[1] if p.split(':')[1] == 'ragged' else int(p.split(':')[1]))
                for p in args.points.split(',')]
    legs_wanted = [x for x in args.legs.split(',') if x]
    if 'a' in legs_wanted and not os.path.isfile(os.path.join(args.parent_tree, 'rwkv.cppy_amd', 'build', 'librwkv.so')):
        print('no parent build (--parent-tree): leg a is left out', file=sys.stderr)
        legs_wanted.remove('a')
    result = {'model': f'synthetic RWKV-v6 C {C} L {NL} V {V} {FMT}', 'reps': args.reps, 'unit': 'ms per fill of all B slots',
              'points': []}
    for B, n in grid:
        legs = {}
        for name in legs_wanted + (['d'] if B == 1 else []):
            cmd = [sys.executable, os.path.abspath(__file__), '--leg', name, '--rows', str(B), '--length',
                   str(-1 if n == 'ragged' else n), '--reps', str(args.reps), '--model-dir', args.model_dir,
                   '--parent-tree', args.parent_tree] + (['--kernel-stats'] if args.kernel_stats else [])
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
            lines = [x for x in p.stdout.splitlines() if x.startswith('LEG ')]
            if p.returncode or not lines:
                # nothing more is started on the GPU after a leg that did not end well
                print(f'leg {name} B={B} length={n} failed (exit {p.returncode})', file=sys.stderr)
                return 1
            legs[name] = json.loads(lines[-1][4:])
            print(B, n, name, legs[name]['ms'], legs[name]['ms_runs'], file=sys.stderr, flush=True)
        pt = {'rows': B, 'length': n, 'tokens': sum(point_lengths(B, n)), 'legs': legs}
        if 'a' in legs and 'c' in legs:
            spread = max(legs['a']['ms_runs']) - min(legs['a']['ms_runs'])
            pt['c_over_a'] = round(legs['c']['ms'] / legs['a']['ms'], 4)
            pt['a_spread_ms'] = round(spread, 3)
            pt['difference_is_real'] = abs(legs['c']['ms'] - legs['a']['ms']) > spread
        if 'b' in legs and 'a' in legs:
            pt['b_over_a'] = round(legs['b']['ms'] / legs['a']['ms'], 4)
        if 'd' in legs and 'c' in legs:
            pt['c_over_bare_eval'] = round(legs['c']['ms'] / legs['d']['ms'], 4)
        result['points'].append(pt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))
    return 0


if __name__ == '__main__':
    sys.exit(main())
