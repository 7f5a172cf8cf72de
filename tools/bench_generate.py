#!/usr/bin/env python3
"""Text generation rates on the headline model (synthetic RWKV-v6 C 2048, L 24, V 65536, Q4_0, the
file bench.py writes) with the reference's generation settings (temperature 0.8, top_p 0.5):

  a  rwkv_mi355x_generate over 256 tokens (sampling and decoding on the device)
  b  the host loop it replaces: rwkv_mi355x_eval_device with logits_out, then sampling.sample_logits
  c  leg a at temperature 0 (greedy)
  d  bare asynchronous rwkv_mi355x_eval_device steps with logits on and no download
  e  the sampler kernel's own time per call (hipEvent pairs bound to its dispatches on the
     context's stream: rwkv_mi355x_set_kernel_timing), greedy and top-p

One fresh process per leg; in it one warm-up pass, then --reps timed passes, the median reported.
1/a - 1/d is what sampling costs per generated token inside the loop.  --lib runs the legs on another
build of the library (leg b on a build of the previous commit); --out names the JSON file written.
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
TEMPERATURE, TOP_P = 0.8, 0.5
P_F = ctypes.POINTER(ctypes.c_float)


class OlderLibrary:
    """The few entry points legs b and d need, bound by hand: a build of the previous commit has no
    rwkv_mi355x_generate for the package's bindings to find."""

    class Ctx:
        def __init__(self, ptr):
            self.ptr = ptr

    def __init__(self, path):
        L = self.library = ctypes.CDLL(path)
        vp, sz, u32, P_I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)
        L.rwkv_init_from_file.argtypes, L.rwkv_init_from_file.restype = [ctypes.c_char_p, u32, u32], vp
        L.rwkv_free.argtypes, L.rwkv_free.restype = [vp], None
        L.rwkv_mi355x_state_upload.argtypes, L.rwkv_mi355x_state_upload.restype = [vp, P_F], ctypes.c_bool
        L.rwkv_mi355x_eval_device.argtypes = [vp, P_I, sz, ctypes.c_bool, P_F, ctypes.c_bool]
        L.rwkv_mi355x_eval_device.restype = ctypes.c_bool
        L.rwkv_mi355x_sync.argtypes, L.rwkv_mi355x_sync.restype = [vp], ctypes.c_bool
        L.rwkv_mi355x_write_synthetic_model.argtypes = [ctypes.c_char_p, ctypes.c_int, u32, u32, u32, u32,
                                                        ctypes.c_char_p, ctypes.c_uint64]
        L.rwkv_mi355x_write_synthetic_model.restype = ctypes.c_bool

    def rwkv_init_from_file(self, path, threads, layers):
        ptr = self.library.rwkv_init_from_file(path.encode(), threads, layers)
        assert ptr
        return self.Ctx(ptr)

    def rwkv_free(self, ctx):
        self.library.rwkv_free(ctx.ptr)


def leg(args):
    import rwkv_cpp
    from rwkv_cpp import sampling
    if hasattr(ctypes.CDLL(args.lib), 'rwkv_mi355x_generate'):
        lib = rwkv_cpp.RWKVSharedLibrary(args.lib)
    else:
        assert args.leg in ('b', 'd'), 'this build has no rwkv_mi355x_generate'
        lib = OlderLibrary(args.lib)
    L = lib.library
    os.makedirs(args.model_dir, exist_ok=True)
    path = os.path.join(args.model_dir, 'v6-1b6-q4_0-seed1.bin')
    if not os.path.isfile(path):
        assert L.rwkv_mi355x_write_synthetic_model((path + '.tmp').encode(), ARCH, V, C, NL, 0, FMT.encode(), 1)
        os.replace(path + '.tmp', path)
    ctx = lib.rwkv_init_from_file(path, 1, NL + 1)
    n = args.tokens
    prompt = (ctypes.c_int32 * 8)(*[int(t) for t in np.random.default_rng(3).integers(0, V, 8)])
    lg = np.zeros(V, np.float32)

    def start():
        assert L.rwkv_mi355x_state_upload(ctx.ptr, None)
        assert L.rwkv_mi355x_eval_device(ctx.ptr, prompt, 8, True, None, True)

    def generate(temperature):
        start()
        t0 = time.perf_counter()
        lib.rwkv_mi355x_generate(ctx, n, temperature, TOP_P, None, 1, 0)
        return time.perf_counter() - t0

    def host_loop():
        start()
        rng = np.random.default_rng(1)
        assert L.rwkv_mi355x_eval_device(ctx.ptr, prompt, 1, True, lg.ctypes.data_as(P_F), True)
        tok = (ctypes.c_int32 * 1)()
        t0 = time.perf_counter()
        for _ in range(n):
            tok[0] = sampling.sample_logits(lg, TEMPERATURE, TOP_P, rng=rng)
            assert L.rwkv_mi355x_eval_device(ctx.ptr, tok, 1, True, lg.ctypes.data_as(P_F), True)
        return time.perf_counter() - t0

    def bare():
        start()
        toks = [(ctypes.c_int32 * 1)(int(t)) for t in np.random.default_rng(5).integers(0, V, n)]
        t0 = time.perf_counter()
        for t in toks:
            assert L.rwkv_mi355x_eval_device(ctx.ptr, t, 1, True, None, False)
        assert L.rwkv_mi355x_sync(ctx.ptr)
        return time.perf_counter() - t0

    def sampler_us(temperature):
        start()
        L.rwkv_mi355x_set_kernel_timing(ctx.ptr, True)
        lib.rwkv_mi355x_generate(ctx, 64, temperature, TOP_P, None, 1, 0)
        L.rwkv_mi355x_sync(ctx.ptr)
        name = ctypes.create_string_buffer(256)
        launches, ms, by, fl = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        count = L.rwkv_mi355x_kernel_stats(ctx.ptr, -1, None, 0, None, None, None, None)
        us = None
        for i in range(count):
            L.rwkv_mi355x_kernel_stats(ctx.ptr, i, name, 256, ctypes.byref(launches), ctypes.byref(ms),
                                       ctypes.byref(by), ctypes.byref(fl))
            if b'k_sample' in name.value and launches.value:
                us = ms.value * 1e3 / launches.value
        L.rwkv_mi355x_set_kernel_timing(ctx.ptr, False)
        assert us is not None, 'no k_sample launches in the kernel statistics'
        return us

    if args.leg == 'e':
        out = {}
        for key, temperature in (('greedy', 0.0), ('top_p', TEMPERATURE)):
            sampler_us(temperature)
            out[f'sampler_us_{key}'] = statistics.median(sampler_us(temperature) for _ in range(args.reps))
    else:
        run = {'a': lambda: generate(TEMPERATURE), 'b': host_loop, 'c': lambda: generate(0.0), 'd': bare}[args.leg]
        run()
        times = [run() for _ in range(args.reps)]
        out = {'tok_per_s': n / statistics.median(times), 'us_per_token': statistics.median(times) / n * 1e6,
               'us_per_token_runs': [t / n * 1e6 for t in times]}
    lib.rwkv_free(ctx)
    print('LEG ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--legs', default='a,b,c,d,e')
    ap.add_argument('--leg', default=None, help='(internal) run this one leg in this process')
    ap.add_argument('--tokens', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lib', default=DEFAULT_LIB)
    ap.add_argument('--label', default='this build')
    ap.add_argument('--model-dir', default=os.environ.get('RWKV_BENCH_DIR', '/tmp/rwkv_bench'))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'generate_bench.json'))
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    result = {'model': f'synthetic RWKV-v6 C {C} L {NL} V {V} {FMT}', 'temperature': TEMPERATURE, 'top_p': TOP_P,
              'tokens': args.tokens, 'reps': args.reps, 'build': args.label, 'legs': {}}
    for name in args.legs.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', name, '--tokens', str(args.tokens), '--reps',
               str(args.reps), '--lib', args.lib, '--model-dir', args.model_dir]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
        lines = [l for l in p.stdout.splitlines() if l.startswith('LEG ')]
        if p.returncode or not lines:
            print(f'leg {name} failed (exit {p.returncode})', file=sys.stderr)
            return 1
        result['legs'][name] = json.loads(lines[-1][4:])
        print(name, result['legs'][name], file=sys.stderr, flush=True)
    legs = result['legs']
    if 'a' in legs and 'd' in legs:
        result['sampling_cost_us_per_token'] = legs['a']['us_per_token'] - legs['d']['us_per_token']
    if 'a' in legs and 'b' in legs:
        result['generate_vs_host_loop'] = legs['a']['tok_per_s'] / legs['b']['tok_per_s']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))
    return 0


if __name__ == '__main__':
    sys.exit(main())
