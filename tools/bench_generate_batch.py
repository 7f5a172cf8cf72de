#!/usr/bin/env python3
"""Batched generation rates on the headline model (synthetic RWKV-v6 C 2048, L 24, V 65536, Q4_0, the
file bench.py writes): temperature 0.8, top_p 0.5, presence / frequency penalties 0.2 / 0.2,
128 tokens for each of B rows, B in 8, 32, 128.

  a  rwkv_mi355x_generate_batch, no stop tokens, check_every = 0 (nothing but the tokens comes back)
  b  the loop a caller could write before it: rwkv_mi355x_eval_batch_device on torch device tensors,
     the B x V logits brought to the host every step, per row the penalties and
     sampling.sample_logits on the host, the tokens passed back
  c  bare rwkv_mi355x_eval_batch_device steps with logits on and nothing downloaded: the ceiling

One fresh process per (leg, B); in it one warm-up pass, then --reps timed passes, the median
reported.  1/a - 1/c (per step) is what sampling, penalties and the snapshot kernel cost in the loop.
--out names the JSON file written.  What the sampler change did to single-context generation is
measured with tools/bench_generate.py legs a and c and plain bench.py, this build and a build of the
previous commit alternating (the single_context block of profiles/generate_batch_bench.json).
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


def leg(args):
    import rwkv_cpp
    from rwkv_cpp import sampling
    from rwkv_cpp.rwkv_cpp_shared_library import make_batch_sampling
    if args.leg in ('b', 'c'):
        # torch's runtime first, as in bench.py: it does not find the GPU once the library has opened it
        import torch
        torch.cuda.init()
    lib =rwkv_cpp.RWKVSharedLibrary(args.lib)
    L = lib.library
    os.makedirs(args.model_dir, exist_ok=True)
    path = os.path.join(args.model_dir, 'v6-1b6-q4_0-seed1.bin')
    if not os.path.isfile(path):
        assert L.rwkv_mi355x_write_synthetic_model((path + '.tmp').encode(), ARCH, V, C, NL, 0, FMT.encode(), 1)
        os.replace(path + '.tmp', path)
    ctx = lib.rwkv_init_from_file(path, 1, NL + 1)
    B, n = args.rows, args.tokens
    state_len = L.rwkv_get_state_len(ctx.ptr)
    prompts = np.random.default_rng(3).integers(0, V, (B, 8))

    def generate_batch():
        for r in range(B):
            assert L.rwkv_mi355x_state_upload(ctx.ptr, None)
            lib.rwkv_mi355x_eval_device(ctx, [int(t) for t in prompts[r]])
            lib.rwkv_mi355x_batch_store(ctx, r)
        p = make_batch_sampling(B, TEMPERATURE, TOP_P, PRESENCE, FREQUENCY, seeds=range(1, B + 1))
        t0 = time.perf_counter()
        _, lengths, steps = lib.rwkv_mi355x_generate_batch(ctx, B, n, p)
        dt = time.perf_counter() - t0
        assert steps == n and (lengths == n).all()
        return dt

    def device_buffers():
        import torch
        dev = torch.device('cuda', 0)
        sbuf = [torch.zeros((B, state_len), dtype=torch.float32, device=dev) for _ in range(2)]
        lbuf = torch.zeros((B, V), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        return sbuf, lbuf

    def step(sbuf, lbuf, tokens, i):
        sin = None if i == 0 else sbuf[i & 1].data_ptr()
        assert L.rwkv_mi355x_eval_batch_device(ctx.ptr, tokens.ctypes.data, B, sin, sbuf[(i & 1) ^ 1].data_ptr(),
                                               lbuf.data_ptr())

    def host_loop():
        sbuf, lbuf = device_buffers()
        rng = np.random.default_rng(1)
        counts = np.zeros((B, V), np.float32)
        tokens = np.ascontiguousarray(prompts[:, 0], dtype=np.uint32)
        step(sbuf, lbuf, tokens, 0)
        assert L.rwkv_mi355x_sync(ctx.ptr)
        t0 = time.perf_counter()
        for i in range(1, n + 1):
            lg = lbuf.cpu().numpy()
            for r in range(B):
                seen = counts[r] > 0
                lg[r][seen] -= PRESENCE + counts[r][seen] * FREQUENCY
                tokens[r] = sampling.sample_logits(lg[r], TEMPERATURE, TOP_P, rng=rng)
                counts[r, tokens[r]] += 1
            step(sbuf, lbuf, tokens, i)
            assert L.rwkv_mi355x_sync(ctx.ptr)
        return time.perf_counter() - t0

    def bare():
        sbuf, lbuf = device_buffers()
        toks = np.random.default_rng(5).integers(0, V, (n + 1, B)).astype(np.uint32)
        step(sbuf, lbuf, toks[0], 0)
        assert L.rwkv_mi355x_sync(ctx.ptr)
        t0 = time.perf_counter()
        for i in range(1, n + 1):
            step(sbuf, lbuf, toks[i], i)
        assert L.rwkv_mi355x_sync(ctx.ptr)
        return time.perf_counter() - t0

    if args.leg == 'a':
        lib.rwkv_mi355x_batch_reserve(ctx, B)
    run = {'a': generate_batch, 'b': host_loop, 'c': bare}[args.leg]
    run()
    times = [run() for _ in range(args.reps)]
    med = statistics.median(times)
    out = {'rows': B, 'tokens': n, 'reps': args.reps, 'tok_per_s': B * n / med, 'us_per_step': med / n * 1e6, 'us_per_step_runs': [t / n * 1e6 for t in times]}
    lib.rwkv_free(ctx)
    print('LEG ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--legs', default='a,b,c')
    ap.add_argument('--batch', default='8,32,128')
    ap.add_argument('--leg', default=None, help='(internal) run this one leg in this process')
    ap.add_argument('--rows', type=int, default=8, help='(internal) the leg\'s B')
    ap.add_argument('--tokens', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-tokens', type=int, default=0, help='tokens per row in leg b (0: --tokens); its rate is per step')
    ap.add_argument('--host-reps', type=int, default=0, help='timed passes of leg b (0: --reps)')
    ap.add_argument('--lib', default=DEFAULT_LIB)
    ap.add_argument('--model-dir', default=os.environ.get('RWKV_BENCH_DIR', '/tmp/rwkv_bench'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'generate_batch_bench.json'))
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    result = {'model': f'synthetic RWKV-v6 C {C} L {NL} V {V} {FMT}', 'temperature': TEMPERATURE, 'top_p': TOP_P,
              'presence': PRESENCE, 'frequency': FREQUENCY, 'tokens': args.tokens, 'reps': args.reps, 'runs': []}
    failed = 0
    for B in [int(b) for b in args.batch.split(',') if b.strip()]:
        legs = {}
        for name in args.legs.split(','):
            tokens, reps = args.tokens, args.reps
            if name == 'b':
                tokens, reps = args.host_tokens or tokens, args.host_reps or reps
            cmd = [sys.executable, os.path.abspath(__file__), '--leg', name, '--rows', str(B), '--tokens', str(tokens),
                   '--reps', str(reps), '--lib', args.lib, '--model-dir', args.model_dir]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
            lines = [l for l in p.stdout.splitlines() if l.startswith('LEG ')]
            if p.returncode or not lines:
                # nothing more is started on the GPU after a leg that did not end well
                print(f'leg {name} B={B} failed (exit {p.returncode})', file=sys.stderr)
                return 1
            legs[name] = json.loads(lines[-1][4:])
            print(B, name, legs[name], file=sys.stderr, flush=True)
        run = {'rows': B, 'legs': legs}
        if 'a' in legs and 'c' in legs:
            run['sampling_cost_us_per_step'] = legs['a']['us_per_step'] - legs['c']['us_per_step']
        if 'a' in legs and 'b' in legs:
            run['generate_batch_vs_host_loop'] = legs['a']['tok_per_s'] / legs['b']['tok_per_s']
            if not run['generate_batch_vs_host_loop'] > 1.0:
                failed += 1
                print(f'B={B}: rwkv_mi355x_generate_batch is NOT faster than the host loop', file=sys.stderr)
        result['runs'].append(run)
    result['faster_than_the_host_loop_at_every_B'] = failed == 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
