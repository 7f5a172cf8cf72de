#!/usr/bin/env python3
"""Continuous batching against waves on the headline model (synthetic RWKV-v6 C 2048, L 24, V 65536,
Q4_0, the file bench.py writes): 256 sequences whose max_tokens are uniform in [16, 256] from a fixed
seed, no stop tokens (both legs do the same useful work), temperature 0.8, top_p 0.5, presence /
frequency penalties 0.2 / 0.2, 32 decode rows.

  a  one rwkv_mi355x_generate_queue call over 32 lanes, check_every = 0
  b  the same slots through rwkv_mi355x_generate_batch in 8 waves of 32 rows, each wave with n = its
     longest max_tokens; what a row draws past its cap is ignored

Both legs start from the same prefilled slots (rwkv_mi355x_prefill_batch; leg b brings each wave's
slots to [0, 32) with batch_load / batch_store); neither is timed.  One fresh process per leg; in it
one warm-up pass, then --reps timed passes, the median reported: decode steps, us per step, useful
tokens per second.  The ratio of the two step counts is known beforehand (sampling.queue_schedule) and
is the ceiling of the speed-up; a's us/step - b's us/step is what the turnover and move launches
cost per step.  --out names the JSON file written.
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
sys.path.insert(0, os.path.join(REPO, 'rwkv.cppy_amd', 'python'))
DEFAULT_LIB = os.path.join(REPO, 'rwkv.cppy_amd', 'build', 'librwkv.so')
ARCH, V, C, NL, FMT = 6, 65536, 2048, 24, 'Q4_0'
TEMPERATURE, TOP_P, PRESENCE, FREQUENCY = 0.8, 0.5, 0.2, 0.2
LO, HI = 16, 256


def workload(Q, lanes):
    """(max_tokens, the queue's steps, the waves' steps)."""
    from rwkv_cpp import sampling
    caps = [int(x) for x in np.random.default_rng(7).integers(LO, HI + 1, Q)]
    _, _, queue_steps = sampling.queue_schedule(caps, lanes)
    wave_steps = sum(max(caps[w:w + lanes]) for w in range(0, Q, lanes))
    return caps, queue_steps, wave_steps


def leg(args):
    import rwkv_cpp
    from rwkv_cpp.rwkv_cpp_shared_library import make_batch_sampling
    lib = rwkv_cpp.RWKVSharedLibrary(args.lib)
    L = lib.library
    os.makedirs(args.model_dir, exist_ok=True)
    path = os.path.join(args.model_dir, 'v6-1b6-q4_0-seed1.bin')
    if not os.path.isfile(path):
        assert L.rwkv_mi355x_write_synthetic_model((path + '.tmp').encode(), ARCH, V, C, NL, 0, FMT.encode(), 1)
        os.replace(path + '.tmp', path)
    ctx = lib.rwkv_init_from_file(path, 1, NL + 1)
    Q, lanes = args.sequences, args.lanes
    caps, queue_steps, wave_steps = workload(Q, lanes)
    prompts = [[int(t) for t in row] for row in np.random.default_rng(3).integers(0, V, (Q, 8))]
    lib.rwkv_mi355x_batch_reserve(ctx, Q)

    def prefill():
        lib.rwkv_mi355x_prefill_batch(ctx, prompts, list(range(Q)))

    def queue():
        prefill()
        t0 = time.perf_counter()
        out = lib.rwkv_mi355x_generate_queue(ctx, caps, lanes, TEMPERATURE, TOP_P, PRESENCE, FREQUENCY,
                                             seeds=range(1, Q + 1))
        dt = time.perf_counter() - t0
        assert list(out['lengths']) == caps and out['steps'] == queue_steps, (out['steps'], queue_steps)
        return dt, out['steps']

    def waves():
        prefill()
        dt, steps = 0.0, 0
        for w in range(0, Q, lanes):
            rows = min(lanes, Q - w)
            for r in range(rows if w else 0):
                lib.rwkv_mi355x_batch_load(ctx, w + r)
                lib.rwkv_mi355x_batch_store(ctx, r)
            assert L.rwkv_mi355x_sync(ctx.ptr)
            n = max(caps[w:w + rows])
            p = make_batch_sampling(rows, TEMPERATURE, TOP_P, PRESENCE, FREQUENCY, seeds=range(1 + w, 1 + w + rows))
            t0 = time.perf_counter()
            _, lengths, ran = lib.rwkv_mi355x_generate_batch(ctx, rows, n, p)
            dt += time.perf_counter() - t0
            assert ran == n and (lengths == n).all()
            steps += ran
        return dt, steps

    run = {'a': queue, 'b': waves}[args.leg]
    run()
    passes = [run() for _ in range(args.reps)]
    steps = passes[0][1]
    med = statistics.median(t for t, _ in passes)
    out = {'sequences': Q, 'lanes': lanes, 'useful_tokens': sum(caps), 'steps': int(steps), 'reps': args.reps,
           'seconds': med, 'us_per_step': med / steps * 1e6, 'useful_tok_per_s': sum(caps) / med,
           'us_per_step_runs': [t / steps * 1e6 for t, _ in passes]}
    lib.rwkv_free(ctx)
    print('LEG ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--legs', default='a,b')
    ap.add_argument('--leg', default=None, help='(internal) run this one leg in this process')
    ap.add_argument('--sequences', type=int, default=256)
    ap.add_argument('--lanes', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lib', default=DEFAULT_LIB)
    ap.add_argument('--model-dir', default=os.environ.get('RWKV_BENCH_DIR', '/tmp/rwkv_bench'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'generate_queue_bench.json'))
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    caps, queue_steps, wave_steps = workload(args.sequences, args.lanes)
    result = {'model': f'synthetic RWKV-v6 C {C} L {NL} V {V} {FMT}', 'temperature': TEMPERATURE, 'top_p': TOP_P,
              'presence': PRESENCE, 'frequency': FREQUENCY, 'sequences': args.sequences, 'lanes': args.lanes,
              'max_tokens': f'uniform [{LO}, {HI}], numpy default_rng(7)', 'useful_tokens': sum(caps),
              'steps_queue': queue_steps, 'steps_waves': wave_steps, 'step_ratio_waves_over_queue': wave_steps / queue_steps,
              'reps': args.reps, 'legs': {}}
    for name in args.legs.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', name, '--sequences', str(args.sequences), '--lanes',
               str(args.lanes), '--reps', str(args.reps), '--lib', args.lib, '--model-dir', args.model_dir]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
        lines = [l for l in p.stdout.splitlines() if l.startswith('LEG ')]
        if p.returncode or not lines:
            # nothing more is started on the GPU after a leg that did not end well
            print(f'leg {name} failed (exit {p.returncode})', file=sys.stderr)
            return 1
        result['legs'][name] = json.loads(lines[-1][4:])
        print(name, result['legs'][name], file=sys.stderr, flush=True)
    legs = result['legs']
    if 'a' in legs and 'b' in legs:
        result['time_ratio_waves_over_queue'] = legs['b']['seconds'] / legs['a']['seconds']
        result['turnover_and_move_us_per_step'] = legs['a']['us_per_step'] - legs['b']['us_per_step']
        result['queue_is_faster'] = legs['a']['useful_tok_per_s'] > legs['b']['useful_tok_per_s']
        if not result['queue_is_faster']:
            print('rwkv_mi355x_generate_queue is NOT faster than the waves', file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))
    return 0


if __name__ == '__main__':
    sys.exit(main())
