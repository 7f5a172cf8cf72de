#!/usr/bin/env python3
"""Records tests/golden/decode_program.json: the launch tables test_gpu_decode_program.py pins.

Run it on a GPU with the library built from the commit whose program is to be the reference:
    python tools/record_decode_program.py [--out FILE] [--commit ID]
The tables come from the test module's own collect(), so the recording and the test cannot drift
apart.  --commit is written into the file as the build it was recorded from.
"""
import argparse
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))

import test_gpu_decode_program as tdp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=tdp.GOLDEN_FILE)
    ap.add_argument('--commit', default='', help='the commit the library was built from')
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        tables = {name: tdp.collect(name, d) for name in sorted(tdp.CONFIGS)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    # one case per line, so a change of one program shows as one line of the file's diff
    configs = []
    for name, t in tables.items():
        cases = ',\n'.join(f'  {json.dumps(c)}: {json.dumps(rows)}' for c, rows in t.items())
        configs.append(f' {json.dumps(name)}: {{\n{cases}\n }}')
    with open(args.out, 'w') as f:
        f.write('{\n"recorded_from": %s,\n"row": ["kernel", "launches", "total_bytes", "total_flops"],\n"tables": {\n%s\n}\n}\n'
                % (json.dumps(args.commit), ',\n'.join(configs)))
    empty = [f'{n}: {c}' for n, t in tables.items() for c, rows in t.items() if not any(r[1] for r in rows)]
    print(f'wrote {args.out}: {sum(len(t) for t in tables.values())} cases; cases with no launches recorded: {empty}')


if __name__ == '__main__':
    main()
