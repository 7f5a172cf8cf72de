"""Real widths with data the plain synthetic writer never produces (synth.py, struct
rwkv_mi355x_synth_opts): norms that are not the identity, LoRA widths at and beyond every kernel
predicate, decays at the edges of their range, and the odd RWKV-4 vocabulary of 50277.

The plain writer stores ones and zeros for ln0 / ln1 / ln2 / ln_out / att.ln_x, so with its files a
kernel reading a norm weight of the wrong channel, head or tensor equals the oracle all the same; the
golden fixtures have one head of 64 (v5, v7) or heads of 8 (v6).  Here every norm tensor is its own
seeded draw (test_synthetic_cpu.py::test_norms_files_see_an_index_slip: the oracle's logits move when
one is shifted by a channel), at C = 512 (8 heads of 64, two per 256-channel norm block) and at the
widths where test_gpu_configs.py documents a change of code path.

Gate, as everywhere: logits and state equal the oracle's GPU-association variant bit for bit; the
distance to the ggml-order oracle is bounded by the noise band max(1e-3, 1.5 * noise) at C = 512.
All files: 2 layers (v7's v0 / v1 / v2 and v6's next-layer maa need a layer above 0), V = 1024.
"""
import os

import numpy as np
import pytest
import torch  # before librwkv initialises HIP (torch's own HIP runtime must come up first)

from oracle_ctypes import assert_bits_equal, gpu_variant, noise_band
from rwkv_lib import RWKVModel, library
from synth import write_synth
from test_gpu_batch import check_batch
from test_gpu_configs import FUSION_MASKS, gpu_serial
from test_gpu_generate import check_greedy
from test_gpu_score import Ctx as ScoreCtx, check_against_logits

pytestmark = pytest.mark.gpu

VOCAB = 1024
LAYERS = 2
RWKV_ERROR_MODEL_PARAMS, RWKV_ERROR_UNSUPPORTED, RWKV_ERROR_SHAPE = 4 << 8, 9, 10

NORM_CASES = ([(4, 'Q8_0', C) for C in (512, 768, 4096, 4608)] + [(5, 'Q4_1', C) for C in (512, 4096)] +
              [(6, 'Q4_0', C) for C in (512, 2048, 2560, 4096, 4608)] + [(7, 'Q5_1', C) for C in (512, 2560)] +
              [(6, 'FP16', 512), (7, 'FP16', 512)])
SMALL_CASES = [c for c in NORM_CASES if c[2] == 512]
DEC_TOKS = [int(t) for t in np.random.default_rng(7).integers(0, VOCAB, 6)]
SEQ_TOKS = [int(t) for t in np.random.default_rng(8).integers(0, VOCAB, 70)]


@pytest.fixture(scope='module')
def d(tmp_path_factory):
    return str(tmp_path_factory.mktemp('real'))


def synth_file(d, arch, fmt, C, vocab=VOCAB, layers=LAYERS, **opts):
    tag = '-'.join(f'{k}{v}' for k, v in sorted(opts.items()))
    p = os.path.join(d, f'v{arch}-{fmt}-C{C}-V{vocab}-L{layers}-{tag}.bin')
    assert write_synth(p, arch, vocab, C, layers, fmt, 61, **opts), p
    return p


_REF = {}


def oracle(path, toks, sequence=False):
    """The GPU-association oracle's (logits, state), computed once per file and token list."""
    key = (path, tuple(toks), sequence)
    if key not in _REF:
        lg, st = gpu_variant(path, toks, sequence=sequence)
        lg.setflags(write=False)
        st.setflags(write=False)
        _REF[key] = (lg, st)
    return _REF[key]


def check_decode(m, path, toks, what):
    lg, st = gpu_serial(m, toks)
    glg, gst = oracle(path, toks)
    assert_bits_equal(lg, glg, f'{what} decode logits')
    assert_bits_equal(st, gst, f'{what} decode state')
    return lg, st


def check_sequence(m, path, toks, what):
    lg, st = m.eval_sequence(toks, None, use_numpy=True)
    glg, gst = oracle(path, toks, sequence=True)
    assert_bits_equal(lg, glg, f'{what} sequence logits')
    assert_bits_equal(st, gst, f'{what} sequence state')
    return lg, st


def set_knob(m, name, value):
    assert library().library.rwkv_mi355x_debug_set(m._ctx.ptr, name, value), (name, value)


# ------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize('arch,fmt,C', NORM_CASES)
def test_norms_decode_bit_exact(d, arch, fmt, C):
    path = synth_file(d, arch, fmt, C, norms=1)
    m = RWKVModel(library(), path)
    lg, st = check_decode(m, path, DEC_TOKS, f'v{arch} {fmt} C={C} norms')
    m.free()
    if C == 512:
        olg, ost, noise, _ = noise_band(path, DEC_TOKS)
        tol = max(1e-3, 1.5 * noise)
        assert np.abs(lg - olg).max() <= tol, (float(np.abs(lg - olg).max()), noise)
        assert np.abs(st - ost).max() <= tol, (float(np.abs(st - ost).max()), noise)


@pytest.mark.parametrize('arch,fmt,C', NORM_CASES)
def test_norms_sequence_bit_exact(d, arch, fmt, C):
    path = synth_file(d, arch, fmt, C, norms=1)
    m = RWKVModel(library(), path)
    lg, st = check_sequence(m, path, SEQ_TOKS, f'v{arch} {fmt} C={C} norms')
    lg2, st2 = m.eval_sequence_in_chunks(SEQ_TOKS, None, chunk_size=32, use_numpy=True)
    m.free()
    assert_bits_equal(lg2, lg, 'chunks of 32 vs one call: logits')
    assert_bits_equal(st2, st, 'chunks of 32 vs one call: state')
    if C == 512:
        olg, ost, noise, _ = noise_band(path, SEQ_TOKS, sequence=True)
        tol = max(1e-3, 1.5 * noise)
        assert np.abs(lg - olg).max() <= tol, (float(np.abs(lg - olg).max()), noise)


@pytest.mark.parametrize('arch,fmt,C', SMALL_CASES + [(6, 'Q4_0', 2048)])
def test_norms_every_decode_arm(d, arch, fmt, C):
    """Every fused decode launch and its unfused arm (test_gpu_configs.py FUSION_MASKS) and both v6
    attention layouts read the norms of the right channel, head and tensor."""
    path = synth_file(d, arch, fmt, C, norms=1)
    m = RWKVModel(library(), path)
    for mask in FUSION_MASKS + [1023]:
        set_knob(m, b'decode_fusion', mask)
        check_decode(m, path, DEC_TOKS, f'v{arch} {fmt} C={C} norms, fusion mask {mask}')
    for co in (-1, 0, 1):
        set_knob(m, b'co_mode', co)
        check_decode(m, path, DEC_TOKS, f'v{arch} {fmt} C={C} norms, co_mode {co}')
    m.free()


@pytest.mark.parametrize('arch,fmt,C', SMALL_CASES)
@pytest.mark.parametrize('B', [8, 56])
def test_norms_batch(d, arch, fmt, C, B):
    """Batched decode (B = 8: the matvec over the contexts; B = 56: the GEMM on token tiles): every
    context equals its own rwkv_eval bit for bit."""
    check_batch(synth_file(d, arch, fmt, C, norms=1), B)


# ------------------------------------------------------------------------------ LoRA widths
LORA_MASKS = [1023 ^ 1, 1023 ^ 2, 1023 ^ 16, 1023 ^ 256, 1023 ^ 512, 0, 1023]


def check_lora_file(path, what, refused=0):
    """Loads, decodes under the masks that switch each LoRA-carrying fusion off and on, runs the
    sequence.  refused: the error a width the engine does not take must give at load (never a context
    that fails or returns garbage later)."""
    L = library().library
    L.rwkv_set_print_errors(None, False)
    try:
        ptr = L.rwkv_init_from_file(path.encode(), 1, 99)
        err = L.rwkv_get_last_error(None)
    finally:
        L.rwkv_set_print_errors(None, True)
    if refused:
        assert not ptr and err == refused, f'{what}: expected a refusal with {refused:#x}, got {ptr} / {err:#x}'
        return
    assert ptr, f'{what}: the loader refused the file (error {err:#x})'
    L.rwkv_free(ptr)
    m = RWKVModel(library(), path)
    for mask in LORA_MASKS:
        set_knob(m, b'decode_fusion', mask)
        check_decode(m, path, DEC_TOKS, f'{what}, fusion mask {mask}')
    check_sequence(m, path, SEQ_TOKS, what)
    m.free()


@pytest.mark.parametrize('C', [512, 2048])
@pytest.mark.parametrize('maa_d,decay_d', [(32, 64), (64, 128), (96, 160), (32, 96), (64, 160)])
def test_v6_lora_widths(d, C, maa_d, decay_d):
    """v6 maa / decay LoRA widths at and beyond each predicate: maa D = 32 is the limit of
    sig_maa_supported / v6_maa_emb_supported, 64 that of v6_maa_dec_supported, of the second k_v6_mix5
    instantiation and of the loader; decay D = 64 / 96 / 128 are v6_decay_seq_supported's widths and
    160 is past it.  maa D = 96 has no kernel (k_v6_mix5 holds D <= 64): the loader refuses it with
    RWKV_ERROR_MODEL_PARAMS | RWKV_ERROR_SHAPE, so decay 160 also runs beside maa 64."""
    path = synth_file(d, 6, 'Q4_0', C, norms=1, maa_d=maa_d, decay_d=decay_d)
    check_lora_file(path, f'v6 C={C} maa_d={maa_d} decay_d={decay_d}',
                    refused=RWKV_ERROR_MODEL_PARAMS | RWKV_ERROR_SHAPE if maa_d > 64 else 0)


@pytest.mark.parametrize('fmt,w,a,v,g', [(f, *wd) for f in ('Q5_1', 'FP16')
                                         for wd in ((96, 96, 64, 320), (128, 128, 96, 512), (64, 64, 32, 520),
                                                    (64, 64, 32, 544))] +
                         [('FP32', 0, 0, 0, 256), ('FP32', 0, 0, 0, 264), ('FP32', 0, 0, 0, 288)])
def test_v7_lora_widths(d, fmt, w, a, v, g):
    """v7 LoRA widths around att7_lora_supported: K % 8 == 0 and K <= 512 (F16) / 256 (F32).  g = 512
    and 256 sit at the register tile's edge; 544 (F16) and 288 (F32) are past it and take the matvec
    arm.  520 and 264 are no whole 32-element blocks, which every matvec outside the fused launch
    needs: the loader refuses them with RWKV_ERROR_MODEL_PARAMS | RWKV_ERROR_UNSUPPORTED (before, the
    context loaded and rwkv_eval failed)."""
    path = synth_file(d, 7, fmt, 512, norms=1, w_d=w, a_d=a, v_d=v, g_d=g)
    check_lora_file(path, f'v7 {fmt} w={w} a={a} v={v} g={g}',
                    refused=RWKV_ERROR_MODEL_PARAMS | RWKV_ERROR_UNSUPPORTED if g % 32 else 0)


# ------------------------------------------------------------------------------ wide decays
@pytest.mark.parametrize('arch,fmt', [(4, 'Q8_0'), (5, 'Q4_1'), (6, 'Q4_0'), (7, 'Q5_1')])
def test_wide_decays(d, arch, fmt):
    """Decays over their whole range (v6 / v7: w = exp(-exp(U(-8, 2))), from 1 - 3e-4 down to 6e-4;
    v4: time_first in +-4 and decays down to -20 per token, where the pp stabiliser decides): finite,
    serial == sequence, and both equal the oracle."""
    path = synth_file(d, arch, fmt, 512, norms=1, wide_decay=1)
    toks12 = SEQ_TOKS[:12]
    m = RWKVModel(library(), path)
    lg, st = check_decode(m, path, toks12, f'v{arch} wide decay')
    assert np.all(np.isfinite(lg)) and np.all(np.isfinite(st))
    slg, sst = check_sequence(m, path, SEQ_TOKS, f'v{arch} wide decay')
    assert np.all(np.isfinite(slg)) and np.all(np.isfinite(sst))
    lg70, st70 = gpu_serial(m, SEQ_TOKS)
    m.free()
    assert_bits_equal(lg70, slg, 'serial vs sequence logits')
    assert_bits_equal(st70, sst, 'serial vs sequence state')


# --------------------------------------------------------------------------- odd vocabulary
ODD_V = 50277
ODD_TOKS = [int(t) for t in np.random.default_rng(9).integers(0, ODD_V, 150)]


def odd_file(d, fmt):
    return synth_file(d, 4, fmt, 768, vocab=ODD_V, layers=1)


@pytest.mark.parametrize('fmt', ['Q8_0', 'FP16'])
def test_odd_vocabulary_decode_and_sequence(d, fmt):
    """The RWKV-4 vocabulary of 50277 (odd: logits rows only 4-byte aligned, M % 32 == 5) through the
    decode head (k_mv) and the sequence evaluation."""
    path = odd_file(d, fmt)
    m = RWKVModel(library(), path)
    check_decode(m, path, ODD_TOKS[:4], f'V={ODD_V} {fmt}')
    check_sequence(m, path, ODD_TOKS[:40], f'V={ODD_V} {fmt}')
    m.free()


@pytest.mark.parametrize('fmt', ['Q8_0', 'FP16'])
def test_odd_vocabulary_score(d, fmt):
    """150 tokens cross the 128-row head tile with ldy = 50277: every logits row equals serial
    rwkv_eval bit for bit, losses within 1e-9 of float64 numpy, argmaxes equal."""
    c = ScoreCtx(odd_file(d, fmt))
    try:
        targets = ODD_TOKS[1:] + [ODD_V - 1]
        ref_logits, ref_state, _ = c.serial(ODD_TOKS)
        c.fresh()
        got = c.score(ODD_TOKS, targets, want_logits=True)
        assert got[2] is not None and got[2].shape == (150, ODD_V)
        check_against_logits(got, ref_logits, targets)
        assert_bits_equal(c.state(), ref_state, 'state after scoring')
    finally:
        c.free()


@pytest.mark.parametrize('fmt', ['Q8_0', 'FP16'])
@pytest.mark.parametrize('B', [5, 56])
def test_odd_vocabulary_batch(d, fmt, B):
    check_batch(odd_file(d, fmt), B)


@pytest.mark.parametrize('fmt', ['Q8_0', 'FP16'])
def test_odd_vocabulary_greedy_generate(d, fmt):
    check_greedy(odd_file(d, fmt), n=8)
