"""The synthetic-model writer and its options (rwkv_mi355x_write_synthetic_model_ex), no GPU needed.

The plain writer's bytes are pinned by digest (bench.py and every real-width test read its files);
the options -- seeded norms, LoRA widths, wide decays -- are checked on the stored tensors, through
the oracle's loader and against the oracle's quantizer.  test_norms_files_see_an_index_slip shows,
on data alone, that the norms files used by test_gpu_real_shapes.py can see a one-channel slip of
att.ln_x or an ln1 / ln2 swap: the oracle's logits change in bits.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle_ctypes import OracleModel, quantize_file as oracle_quantize
from rwkv_lib import library
from synth import f32_tensor, read_tensors, rewrite_f32, write_synth

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
QUANT_TYPES = (2, 3, 7, 8, 9)


def test_plain_writer_bytes_unchanged(tmp_path):
    """The option-less writer, through both entry points (the old one and _ex with NULL / all-zero
    options), writes the bytes it wrote before the options existed."""
    kat = json.load(open(os.path.join(GOLD, 'synthetic_writer_sha256.json')))
    L = library().library
    assert len(kat) == 3
    for key, digest in kat.items():
        arch, fmt = int(key[1]), key.split('-')[4]
        assert key == f'v{arch}-C128-L2-V512-{fmt}-seed42'
        a, b, c = (str(tmp_path / f'{key}.{s}') for s in 'abc')
        assert L.rwkv_mi355x_write_synthetic_model(a.encode(), arch, 512, 128, 2, 0, fmt.encode(), 42)
        assert L.rwkv_mi355x_write_synthetic_model_ex(b.encode(), arch, 512, 128, 2, 0, fmt.encode(), 42, None)
        assert write_synth(c, arch, 512, 128, 2, fmt, 42)
        for p in (a, b, c):
            assert hashlib.sha256(open(p, 'rb').read()).hexdigest() == digest, (key, p)


NORMS = ['blocks.0.ln0', 'blocks.0.ln1', 'blocks.0.ln2', 'blocks.1.ln1', 'blocks.1.ln2', 'ln_out']


@pytest.mark.parametrize('arch,fmt', [(4, 'Q8_0'), (5, 'Q4_1'), (6, 'Q4_0'), (7, 'Q5_1'), (6, 'FP16')])
def test_norms_option(tmp_path, arch, fmt):
    """norms: weights U(0.5, 1.5) with channels c % 17 == 16 negated, biases U(-0.5, 0.5), no two
    tensors alike; everything else in the file is what the plain writer stores."""
    C = 256
    p, q = str(tmp_path / 'n.bin'), str(tmp_path / 'plain.bin')
    assert write_synth(p, arch, 512, C, 2, fmt, 9, norms=1)
    assert write_synth(q, arch, 512, C, 2, fmt, 9)
    names = NORMS + (['blocks.0.att.ln_x', 'blocks.1.att.ln_x'] if arch >= 5 else [])
    ws, bs = [], []
    neg = np.arange(C) % 17 == 16
    for n in names:
        w, b = f32_tensor(p, n + '.weight'), f32_tensor(p, n + '.bias')
        assert w.shape == (C,) and b.shape == (C,)
        assert np.all(w[neg] <= -0.5) and np.all(w[neg] >= -1.5) and np.all(w[~neg] >= 0.5) and np.all(w[~neg] <= 1.5)
        assert np.all(np.abs(b) <= 0.5) and b.min() < -0.4 and b.max() > 0.4 and np.abs(w).max() > 1.4
        assert np.all(f32_tensor(q, n + '.weight') == 1) and np.all(f32_tensor(q, n + '.bias') == 0)
        ws.append(w)
        bs.append(b)
    for i in range(len(names)):
        for j in range(i):
            # independent draws: nowhere near each other (equal seeds would give equal tensors)
            assert np.abs(ws[i] - ws[j]).max() > 0.5 and np.abs(bs[i] - bs[j]).max() > 0.5, (names[i], names[j])
            assert np.abs(np.abs(ws[i]) - 0.5 - (bs[j] + 0.5)).max() > 0.5, (names[i], names[j])
    tp, rp = read_tensors(p)
    tq, rq = read_tensors(q)
    assert list(tp) == list(tq)
    for n, (ne, ty, off, nb) in tp.items():
        assert tq[n] == (ne, ty, off, nb)
        if '.ln' not in n and not n.startswith('ln_out'):
            assert rp[off:off + nb] == rq[off:off + nb], n
    m = OracleModel(p)
    assert (m.arch_major, m.n_embed, m.n_layer, m.n_vocab) == (arch, C, 2, 512)
    lg, st = m.eval_serial([1, 2, 3])
    assert np.all(np.isfinite(lg)) and np.all(np.isfinite(st))
    lq, _ = OracleModel(q).eval_serial([1, 2, 3])
    assert not np.array_equal(lg, lq)


@pytest.mark.parametrize('fmt,maa_d,decay_d', [('Q4_0', 32, 64), ('Q4_0', 64, 128), ('Q4_0', 96, 160), ('Q4_0', 32, 96),
                                               ('FP16', 40, 72)])
def test_v6_lora_widths(tmp_path, fmt, maa_d, decay_d):
    C = 128
    p = str(tmp_path / 'w6.bin')
    assert write_synth(p, 6, 512, C, 2, fmt, 5, maa_d=maa_d, decay_d=decay_d)
    t, _ = read_tensors(p)
    for l in range(2):
        assert t[f'blocks.{l}.att.time_maa_w1'][0] == (C, 5 * maa_d)
        assert t[f'blocks.{l}.att.time_maa_w2'][0] == (maa_d, C, 5)
        assert t[f'blocks.{l}.att.time_decay_w1'][0] == (C, decay_d)
        assert t[f'blocks.{l}.att.time_decay_w2'][0] == (decay_d, C)
    lg, st = OracleModel(p).eval_serial([1, 2, 3])
    assert np.all(np.isfinite(lg)) and np.all(np.isfinite(st))


def test_v6_quantized_decay_width_needs_whole_blocks(tmp_path):
    """time_decay_w2 (K = decay_d) is quantized in 32-element blocks: the writer refuses other widths
    there, and writes them in the float formats."""
    assert not write_synth(str(tmp_path / 'bad.bin'), 6, 512, 128, 2, 'Q4_0', 5, decay_d=72)
    assert not os.path.exists(str(tmp_path / 'bad.bin'))
    assert write_synth(str(tmp_path / 'ok.bin'), 6, 512, 128, 2, 'FP32', 5, decay_d=72)


@pytest.mark.parametrize('fmt,w,a,v,g', [('Q5_1', 96, 96, 64, 320), ('Q5_1', 128, 128, 96, 512), ('FP16', 64, 64, 32, 520),
                                         ('FP32', 96, 96, 64, 264)])
def test_v7_lora_widths(tmp_path, fmt, w, a, v, g):
    C = 128
    p = str(tmp_path / 'w7.bin')
    assert write_synth(p, 7, 512, C, 2, fmt, 5, w_d=w, a_d=a, v_d=v, g_d=g)
    t, _ = read_tensors(p)
    for l in range(2):
        for n, d in (('w', w), ('a', a), ('g', g)) + ((('v', v),) if l else ()):
            assert t[f'blocks.{l}.att.{n}1'][0] == (C, d)
            assert t[f'blocks.{l}.att.{n}2'][0] == (d, C)
    assert 'blocks.0.att.v1' not in t
    lg, st = OracleModel(p).eval_serial([1, 2, 3])
    assert np.all(np.isfinite(lg)) and np.all(np.isfinite(st))


def test_zero_widths_keep_the_defaults(tmp_path):
    a, b = str(tmp_path / 'a.bin'), str(tmp_path / 'b.bin')
    assert write_synth(a, 6, 512, 128, 2, 'Q4_0', 5) and write_synth(b, 6, 512, 128, 2, 'Q4_0', 5, maa_d=32, decay_d=64)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    assert write_synth(a + '7', 7, 512, 128, 2, 'FP16', 5)
    assert write_synth(b + '7', 7, 512, 128, 2, 'FP16', 5, w_d=96, a_d=96, v_d=64, g_d=320)
    assert open(a + '7', 'rb').read() == open(b + '7', 'rb').read()


@pytest.mark.parametrize('arch', [4, 5, 6, 7])
def test_wide_decay_ranges(tmp_path, arch):
    """wide_decay: the stored decays cover the stated ranges (1024 draws per tensor: both ends are
    reached to within a tenth of the range) and nothing else changes."""
    C = 1024
    p, q = str(tmp_path / 'wd.bin'), str(tmp_path / 'plain.bin')
    assert write_synth(p, arch, 64, C, 2, 'FP16', 3, wide_decay=1)
    assert write_synth(q, arch, 64, C, 2, 'FP16', 3)

    def covers(x, lo, hi):
        assert x.shape == (C,) and np.all(x >= lo) and np.all(x <= hi), (x.min(), x.max())
        assert x.min() < lo + 0.1 * (hi - lo) and x.max() > hi - 0.1 * (hi - lo), (x.min(), x.max())

    changed = set()
    for l in range(2):
        pre = f'blocks.{l}.att.'
        if arch == 4:
            covers(f32_tensor(p, pre + 'time_first'), -4, 4)
            covers(np.log(-f32_tensor(p, pre + 'time_decay').astype(np.float64)), -3 - 1e-6, 3 + 1e-6)
            changed |= {pre + 'time_first', pre + 'time_decay'}
        elif arch == 5:
            d = f32_tensor(p, pre + 'time_decay').astype(np.float64)
            assert np.all(d > 0) and np.all(d < 1)
            covers(np.log(-np.log(d)), -8 - 1e-3, 2 + 1e-6)  # exp(-exp(-8)) is 2.7 ulp of 1 below 1
            changed.add(pre + 'time_decay')
        else:
            name = pre + ('time_decay' if arch == 6 else 'w0')
            covers(f32_tensor(p, name), -8, 2)
            changed.add(name)
    tp, rp = read_tensors(p)
    tq, rq = read_tensors(q)
    assert tp == tq
    for n, (ne, ty, off, nb) in tp.items():
        assert (rp[off:off + nb] != rq[off:off + nb]) == (n in changed), n
    lg, st = OracleModel(p).eval_serial([1, 2, 3, 4])
    assert np.all(np.isfinite(lg)) and np.all(np.isfinite(st))


@pytest.mark.parametrize('arch,fmt,opts', [(4, 'Q8_0', dict(norms=1, wide_decay=1)),
                                           (5, 'Q4_1', dict(norms=1, wide_decay=1)),
                                           (6, 'Q4_0', dict(norms=1, maa_d=64, decay_d=128)),
                                           (7, 'Q5_1', dict(norms=1, w_d=128, a_d=128, v_d=96, g_d=512))])
def test_quantized_writer_matches_oracle_quantizer(tmp_path, arch, fmt, opts):
    """Every tensor the writer quantizes holds the bytes the oracle's quantizer gives for the FP32
    file's tensor, the library's quantizer agrees on the whole file, and the FP32 tensors are equal.
    (The files differ elsewhere by design: the writer stores unquantized matrices as FP16, as the
    reference's converter does, where quantizing an FP32 file leaves them FP32.)"""
    q, f32, oq, lq = (str(tmp_path / n) for n in ('q.bin', 'f32.bin', 'oq.bin', 'lq.bin'))
    assert write_synth(q, arch, 512, 128, 2, fmt, 42, **opts)
    assert write_synth(f32, arch, 512, 128, 2, 'FP32', 42, **opts)
    oracle_quantize(f32, oq, fmt)
    library().rwkv_quantize_model_file(f32, lq, fmt)
    assert open(oq, 'rb').read() == open(lq, 'rb').read()
    tw, rw = read_tensors(q)
    to, ro = read_tensors(oq)
    assert list(tw) == list(to)
    nq = 0
    for n, (ne, ty, off, nb) in tw.items():
        one, oty, ooff, onb = to[n]
        assert one == ne
        if ty in QUANT_TYPES or ty == 0:
            assert oty == ty and rw[off:off + nb] == ro[ooff:ooff + onb], n
            nq += ty in QUANT_TYPES
        else:
            assert ty == 1 and oty == 0, n
            f = np.frombuffer(ro, np.float32, onb // 4, ooff).astype(np.float16)
            assert f.tobytes() == rw[off:off + nb], n
    assert nq >= 2 * 5


@pytest.mark.parametrize('arch,fmt', [(6, 'Q4_0'), (7, 'Q5_1')])
def test_norms_files_see_an_index_slip(tmp_path, arch, fmt):
    """Sensitivity of the C = 512 norms files of test_gpu_real_shapes.py (same writer arguments): with
    att.ln_x.weight of layer 1 rolled by one channel, or layer 1's ln1 and ln2 exchanged, the oracle's
    logits differ in bits from the original's -- a kernel reading the neighbouring channel or the
    other norm cannot equal the oracle on these files.  (On the plain writer's identity norms both
    edits leave the file unchanged.)"""
    p = str(tmp_path / 'n.bin')
    assert write_synth(p, arch, 1024, 512, 2, fmt, 61, norms=1)
    toks = [int(t) for t in np.random.default_rng(7).integers(0, 1024, 6)]
    lg0, st0 = OracleModel(p).eval_serial(toks)
    roll = str(tmp_path / 'roll.bin')
    w = f32_tensor(p, 'blocks.1.att.ln_x.weight')
    rewrite_f32(p, roll, {'blocks.1.att.ln_x.weight': np.roll(w, 1)})
    swap = str(tmp_path / 'swap.bin')
    rewrite_f32(p, swap, {f'blocks.1.ln{a}.{k}': f32_tensor(p, f'blocks.1.ln{b}.{k}')
                          for a, b in ((1, 2), (2, 1)) for k in ('weight', 'bias')})
    for name, path in (('roll', roll), ('swap', swap)):
        lg, st = OracleModel(path).eval_serial(toks)
        assert np.all(np.isfinite(lg))
        assert not np.array_equal(lg.view(np.uint32), lg0.view(np.uint32)), name
        assert np.abs(lg - lg0).max() > 1e-3, (name, float(np.abs(lg - lg0).max()))
    q = str(tmp_path / 'plain.bin')
    assert write_synth(q, arch, 1024, 512, 2, fmt, 61)
    w = f32_tensor(q, 'blocks.1.att.ln_x.weight')
    assert np.array_equal(np.roll(w, 1), w)
