"""Synthetic rwkv.cpp files with options (rwkv_mi355x_write_synthetic_model_ex) and a reader of the
file's tensor table, shared by test_synthetic_cpu.py, test_gpu_real_shapes.py and test_gpu_norms.py.

The file layout (reference rwkv_file_format.inc): six uint32 (magic, version, n_vocab, n_embed,
n_layer, data_type), then per tensor three uint32 (n_dims, name length, type), n_dims uint32 sizes
(ggml order: ne[0] is the row length), the name and the data.
"""
import ctypes
import os
import struct

import numpy as np

from rwkv_cpp.rwkv_cpp_shared_library import RWKVSynthOpts
from rwkv_lib import library

# file type id -> (elements per block, bytes per block)
BLOCK = {0: (1, 4), 1: (1, 2), 2: (32, 18), 3: (32, 20), 7: (32, 22), 8: (32, 24), 9: (32, 34)}
OPTS = ('norms', 'wide_decay', 'maa_d', 'decay_d', 'w_d', 'a_d', 'v_d', 'g_d')


def write_synth(path, arch, n_vocab, n_embed, n_layer, fmt, seed, ffn=0, **opts):
    """Writes the file unless it exists; opts: the fields of struct rwkv_mi355x_synth_opts.  Returns
    the library's verdict (False: the writer refused the shape)."""
    assert set(opts) <= set(OPTS), opts
    if os.path.isfile(path):
        return True
    o = RWKVSynthOpts(**opts)
    return bool(library().library.rwkv_mi355x_write_synthetic_model_ex(
        path.encode(), arch, n_vocab, n_embed, n_layer, ffn, fmt.encode(), seed, ctypes.byref(o)))


def read_tensors(path):
    """{name: (ne tuple in ggml order, type id, data offset, data bytes)} and the raw file bytes."""
    raw = open(path, 'rb').read()
    pos = 24
    out = {}
    while pos < len(raw):
        nd, nl, ty = struct.unpack_from('<3I', raw, pos)
        pos += 12
        ne = struct.unpack_from(f'<{nd}I', raw, pos)
        pos += 4 * nd
        name = raw[pos:pos + nl].decode()
        pos += nl
        per, bb = BLOCK[ty]
        nb = int(np.prod(ne)) // per * bb
        out[name] = (ne, ty, pos, nb)
        pos += nb
    assert pos == len(raw), (pos, len(raw))
    return out, raw


def f32_tensor(path, name):
    """A tensor stored as FP32 (every 1-D tensor and the time_* / r_k tensors), flat."""
    tensors, raw = read_tensors(path)
    ne, ty, off, nb = tensors[name]
    assert ty == 0, (name, ty)
    return np.frombuffer(raw, np.float32, nb // 4, off).copy()


def rewrite_f32(src, dst, changes):
    """Copies src to dst with the FP32 tensors in `changes` ({name: flat float32 array}) replaced."""
    tensors, raw = read_tensors(src)
    buf = bytearray(raw)
    for name, val in changes.items():
        ne, ty, off, nb = tensors[name]
        val = np.ascontiguousarray(val, np.float32)
        assert ty == 0 and val.nbytes == nb, (name, ty, nb)
        buf[off:off + nb] = val.tobytes()
    with open(dst, 'wb') as f:
        f.write(bytes(buf))
