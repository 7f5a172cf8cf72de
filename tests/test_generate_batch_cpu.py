"""Batched generation without a GPU: sampling.penalize (the float32 restatement of the sampler
kernel's penalty) against the float64 formula, make_batch_sampling, and RWKVModel.generate_batch
against a fake library object that records what it is asked to do."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'rwkv.cppy_amd', 'python'))

from rwkv_cpp import sampling  # noqa: E402
from rwkv_cpp.rwkv_cpp_model import RWKVModel  # noqa: E402
from rwkv_cpp.rwkv_cpp_shared_library import make_batch_sampling  # noqa: E402


# ------------------------------------------------------------------------------------ penalize
@pytest.mark.parametrize('presence,frequency', [(0.2, 0.2), (2.0, 1.0), (0.0, 0.3), (0.4, 0.0), (0.0, 0.0)])
def test_penalize_is_the_float64_formula_to_one_rounding(presence, frequency):
    rng = np.random.default_rng(5)
    logits = (rng.normal(0, 4, 4096)).astype(np.float32)
    counts = np.where(rng.random(4096) < 0.2, rng.integers(1, 40, 4096), 0).astype(np.uint32)
    before = logits.copy()
    out = sampling.penalize(logits, counts, presence, frequency)
    assert out.dtype == np.float32 and out.shape == logits.shape
    assert np.array_equal(logits, before), 'the input was modified'
    untouched = counts == 0
    assert untouched.any() and (~untouched).any()
    assert np.array_equal(out[untouched].view(np.uint32), logits[untouched].view(np.uint32))
    exact = logits.astype(np.float64) - (presence + counts.astype(np.float64) * frequency)
    # the roundings, each at most 2^-24 relative: presence and frequency to float32 and the product
    # and the sum (together <= 3 * 2^-24 of the penalty), the difference (2^-24 of the result); with
    # m the largest magnitude among logit, penalty and result that is <= 4 * 2^-24 * m: one ulp of m
    # at the top of its binade, two at the bottom
    scale = np.maximum(np.abs(exact), np.maximum(np.abs(logits), presence + counts * frequency)).astype(np.float64)
    assert (np.abs(out.astype(np.float64) - exact)[~untouched] <= scale[~untouched] * 2.0 ** -22).all()
    if presence == 0.0 and frequency == 0.0:
        assert np.array_equal(out.view(np.uint32), logits.view(np.uint32))


def test_penalize_is_the_pinned_float32_sequence():
    f = np.float32
    logits = np.array([1.1, -2.3, 0.7, 5.0], f)
    counts = np.array([3, 0, 1, 7], np.uint32)
    out = sampling.penalize(logits, counts, 0.2, 0.3)
    for i in range(4):
        want = logits[i] if counts[i] == 0 else f(logits[i] - f(f(0.2) + f(f(counts[i]) * f(0.3))))
        assert out[i].view(np.uint32) == f(want).view(np.uint32)
    with pytest.raises(ValueError):
        sampling.penalize(logits, counts[:3], 0.2, 0.3)


# ------------------------------------------------------------------------------------ make_batch_sampling
def test_make_batch_sampling_broadcasts_and_keeps_its_arrays():
    p = make_batch_sampling(3, 0.5, [0.1, 0.2, 0.3], None, 0.25, {7: 1.5}, None, [4, 5, 6], [9, 8], True, 4)
    assert [p.temperature[i] for i in range(3)] == [0.5] * 3
    assert [round(p.top_p[i], 6) for i in range(3)] == [0.1, 0.2, 0.3]
    assert not p.presence and [p.frequency[i] for i in range(3)] == [0.25] * 3
    assert [p.seed[i] for i in range(3)] == [0, 1, 2] and [p.offset[i] for i in range(3)] == [4, 5, 6]
    assert p.n_bias == 1 and p.bias_ids[0] == 7 and p.bias_values[0] == 1.5
    assert p.n_stop == 2 and [p.stop_tokens[i] for i in range(2)] == [9, 8]
    assert p.keep_counts == 1 and p.check_every == 4
    with pytest.raises(ValueError):
        make_batch_sampling(3, [0.5, 0.5])
    with pytest.raises(ValueError):
        make_batch_sampling(0)


# ------------------------------------------------------------------------------------ RWKVModel.generate_batch
class FakeCtx:
    ptr = 1234


class FakeRaw:
    """What reset_state reaches for: library.library.rwkv_mi355x_state_upload."""

    def __init__(self, log):
        self.log = log

    def rwkv_mi355x_state_upload(self, ptr, state):
        assert ptr == FakeCtx.ptr and state is None
        self.log.append(('reset',))
        return True


class FakeLibrary:
    def __init__(self, slots=0):
        self.log = []
        self.library = FakeRaw(self.log)
        self.slots = slots
        self.params = None

    def rwkv_init_from_file(self, path, threads, layers):
        return FakeCtx()

    def rwkv_get_state_buffer_element_count(self, ctx):
        return 8

    def rwkv_get_logits_buffer_element_count(self, ctx):
        return 300

    def rwkv_free(self, ctx):
        pass

    def rwkv_mi355x_batch_slots(self, ctx):
        return self.slots

    def rwkv_mi355x_batch_reserve(self, ctx, n):
        self.log.append(('reserve', n))
        self.slots = n

    def rwkv_mi355x_eval_device(self, ctx, tokens, compute_logits=True):
        assert compute_logits
        self.log.append(('eval', tuple(tokens)))

    def rwkv_mi355x_batch_store(self, ctx, slot):
        self.log.append(('store', slot))

    def rwkv_mi355x_batch_load(self, ctx, slot):
        self.log.append(('load', slot))

    def rwkv_mi355x_generate_batch(self, ctx, rows, n, params):
        self.log.append(('generate', rows, n))
        self.params = params
        tokens = np.full((rows, n), 0xFFFFFFFF, np.uint32)
        lengths = np.zeros(rows, np.uint32)
        for r in range(rows):
            lengths[r] = min(n, r + 1)
            tokens[r, :lengths[r]] = np.arange(lengths[r]) + 10 * r
        return tokens, lengths, n


@pytest.fixture
def model(tmp_path):
    path = tmp_path / 'model.bin'
    path.write_bytes(b'x')
    lib = FakeLibrary()
    m = RWKVModel(lib, str(path))
    yield m, lib
    m.free()


def test_generate_batch_prepares_each_row_in_order(model):
    m, lib = model
    prompts = [[1, 2, 3], [4, 5], [6]]
    out = m.generate_batch(prompts, 4)
    assert lib.log == [('reserve', 3),
                       ('reset',), ('eval', (1, 2, 3)), ('store', 0),
                       ('reset',), ('eval', (4, 5)), ('store', 1),
                       ('reset',), ('eval', (6,)), ('store', 2),
                       ('generate', 3, 4)]
    # cut to the lengths
    assert out == [[0], [10, 11], [20, 21, 22]]
    assert all(type(t) is int for row in out for t in row)
    # enough slots already: no second reservation
    lib.log.clear()
    m.generate_batch(prompts[:2], 4)
    assert ('reserve', 2) not in lib.log and lib.log[-1] == ('generate', 2, 4)


def test_generate_batch_parameters(model):
    m, lib = model
    m.generate_batch([[1], [2], [3]], 5)
    p = lib.params
    # the defaults: temperature 1, top_p 0.8, no penalty, row r draws from stream r, a look every 16 steps
    assert [p.temperature[i] for i in range(3)] == [1.0] * 3
    assert [p.top_p[i] for i in range(3)] == [np.float32(0.8)] * 3
    assert [p.presence[i] for i in range(3)] == [0.0] * 3 and [p.frequency[i] for i in range(3)] == [0.0] * 3
    assert [p.seed[i] for i in range(3)] == [0, 1, 2] and [p.offset[i] for i in range(3)] == [0, 0, 0]
    assert p.n_bias == 0 and p.n_stop == 0 and p.keep_counts == 0 and p.check_every == 16
    m.generate_batch([[1], [2], [3]], 5, temperature=[0.0, 0.5, 1.5], top_p=0.25, presence_penalty=0.5,
                     frequency_penalty=[0.0, 0.25, 0.5], logit_bias={3: -1.0}, seeds=[7, 8, 9], stop_tokens=[0, 261],
                     check_every=0)
    p = lib.params
    assert [p.temperature[i] for i in range(3)] == [0.0, 0.5, 1.5] and [p.top_p[i] for i in range(3)] == [0.25] * 3
    assert [p.presence[i] for i in range(3)] == [0.5] * 3 and [p.frequency[i] for i in range(3)] == [0.0, 0.25, 0.5]
    assert [p.seed[i] for i in range(3)] == [7, 8, 9]
    assert p.n_bias == 1 and p.bias_ids[0] == 3 and p.bias_values[0] == -1.0
    assert p.n_stop == 2 and [p.stop_tokens[i] for i in range(2)] == [0, 261] and p.check_every == 0


def test_generate_batch_argument_checks(model):
    m, lib = model
    for bad in (dict(prompts=[], n=4), dict(prompts=[[1]] * 257, n=4), dict(prompts=[[1], []], n=4),
                dict(prompts=[[1]], n=0), dict(prompts=[[1], [2]], n=4, temperature=[1.0]),
                dict(prompts=[[1], [2]], n=4, seeds=[1, 2, 3])):
        with pytest.raises(ValueError):
            m.generate_batch(**bad)
    assert lib.log == [], 'a refused call reached the library'


def test_slot_methods_pass_through(model):
    m, lib = model
    m.batch_reserve(4)
    m.batch_store(2)
    m.batch_load(2)
    assert lib.log == [('reserve', 4), ('store', 2), ('load', 2)]
