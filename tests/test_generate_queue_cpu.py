"""The queue of rwkv_mi355x_generate_queue without a GPU: sampling.queue_schedule (the rule of the
turnover on plain integers) on cases worked by hand, and RWKVModel.generate_queue against a fake
library object that records what it is asked to do."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'rwkv.cppy_amd', 'python'))

from rwkv_cpp import sampling  # noqa: E402
from rwkv_cpp.rwkv_cpp_model import RWKVModel  # noqa: E402


# ------------------------------------------------------------------------------------ queue_schedule
def test_seven_sequences_on_three_lanes():
    """By hand.  Step 0: 0, 1, 2 enter lanes 0, 1, 2 and hold them until steps 1, 2, 5.  Step 1: lane 0
    is free, 3 enters (until 4).  Step 2: lane 1, 4 enters (until 10).  Step 3: nothing is free.
    Step 4: lane 0, 5 enters (until 5).  Step 5: lanes 0 and 2 are free, 6 enters lane 0 (until 9) and
    nothing waits for lane 2.  The last decode step is step 9: 10 steps."""
    lane, start, steps = sampling.queue_schedule([1, 2, 5, 3, 8, 1, 4], 3)
    assert lane == [0, 1, 2, 0, 1, 0, 0]
    assert start == [0, 0, 0, 1, 2, 4, 5]
    assert steps == 10


def test_lanes_freed_at_the_same_step_fill_in_lane_order():
    """Lanes 0 and 2 are both free before step 2 (lane 1 until step 3): sequence 3 takes lane 0,
    sequence 4 lane 2, and 5 waits for lane 1."""
    lane, start, steps = sampling.queue_schedule([2, 3, 2, 1, 4, 1], 3)
    assert lane == [0, 1, 2, 0, 2, 0]
    assert start == [0, 0, 0, 2, 2, 3]
    assert steps == 6


def test_more_lanes_than_sequences():
    for lanes in (3, 4, 256):
        assert sampling.queue_schedule([3, 1, 2], lanes) == ([0, 1, 2], [0, 0, 0], 3)


def test_one_lane_runs_them_one_after_the_other():
    lengths = [3, 1, 2, 5]
    lane, start, steps = sampling.queue_schedule(lengths, 1)
    assert lane == [0] * 4 and start == [0, 3, 4, 6] and steps == sum(lengths)


def test_schedule_stays_within_the_list_scheduling_bound():
    rng = np.random.default_rng(3)
    for _ in range(50):
        Q, lanes = int(rng.integers(1, 40)), int(rng.integers(1, 9))
        lengths = [int(x) for x in rng.integers(1, 20, Q)]
        lane, start, steps = sampling.queue_schedule(lengths, lanes)
        L = min(lanes, Q)
        assert steps <= -(-sum(lengths) // L) + max(lengths)
        assert steps == max(s + n for s, n in zip(start, lengths))
        # no two sequences share a lane at a step
        busy = set()
        for s in range(Q):
            for i in range(start[s], start[s] + lengths[s]):
                assert (lane[s], i) not in busy
                busy.add((lane[s], i))


def test_schedule_argument_checks():
    for lengths, lanes in (([], 2), ([1, 0], 2), ([1, 2], 0)):
        with pytest.raises(ValueError):
            sampling.queue_schedule(lengths, lanes)


# ------------------------------------------------------------------------------------ RWKVModel.generate_queue
class FakeCtx:
    ptr = 1234


class FakeLibrary:
    def __init__(self, slots=0):
        self.log = []
        self.slots = slots
        self.kw = None

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

    def rwkv_mi355x_prefill_batch(self, ctx, prompts, slots, cont=None):
        self.log.append(('prefill', tuple(tuple(p) for p in prompts), tuple(slots), cont))

    def rwkv_mi355x_generate_queue(self, ctx, max_tokens, lanes, temperature, top_p, presence, frequency, logit_bias,
                                   seeds, offsets, stop_tokens, check_every):
        self.log.append(('queue', tuple(max_tokens), lanes))
        self.kw = dict(temperature=temperature, top_p=top_p, presence=presence, frequency=frequency, logit_bias=logit_bias,
                       seeds=seeds, offsets=offsets, stop_tokens=stop_tokens, check_every=check_every)
        Q, n = len(max_tokens), max(max_tokens)
        tokens = np.full((Q, n), 0xFFFFFFFF, np.uint32)
        lengths = np.array([min(c, s + 1) for s, c in enumerate(max_tokens)], np.uint32)
        for s in range(Q):
            tokens[s, :lengths[s]] = np.arange(lengths[s]) + 10 * s
        return dict(tokens=tokens, lengths=lengths, lane=np.zeros(Q, np.uint32), start=np.zeros(Q, np.uint32), steps=n)


@pytest.fixture
def model(tmp_path):
    path = tmp_path / 'model.bin'
    path.write_bytes(b'x')
    lib = FakeLibrary()
    m = RWKVModel(lib, str(path))
    yield m, lib
    m.free()


def test_generate_queue_prefills_then_queues(model):
    m, lib = model
    prompts = [[1, 2, 3], [4, 5], [6]]
    out = m.generate_queue(prompts, [4, 1, 3], lanes=2)
    assert lib.log == [('reserve', 3), ('prefill', ((1, 2, 3), (4, 5), (6,)), (0, 1, 2), None), ('queue', (4, 1, 3), 2)]
    assert out == [[0], [10], [20, 21, 22]]
    assert all(type(t) is int for row in out for t in row)
    # the defaults: 32 lanes, temperature 1, top_p 0.8, no penalty, a look every 16 steps; a scalar cap
    lib.log.clear()
    m.generate_queue(prompts, 5)
    assert lib.log == [('prefill', ((1, 2, 3), (4, 5), (6,)), (0, 1, 2), None), ('queue', (5, 5, 5), 32)]
    assert lib.kw == dict(temperature=1.0, top_p=0.8, presence=0.0, frequency=0.0, logit_bias=None, seeds=None, offsets=0,
                          stop_tokens=(), check_every=16)
    m.generate_queue(prompts, 5, temperature=[0.0, 0.5, 1.5], presence_penalty=0.5, frequency_penalty=[0.0, 0.25, 0.5],
                     logit_bias={3: -1.0}, seeds=[7, 8, 9], stop_tokens=[0, 261], check_every=0)
    assert lib.kw == dict(temperature=[0.0, 0.5, 1.5], top_p=0.8, presence=0.5, frequency=[0.0, 0.25, 0.5],
                          logit_bias={3: -1.0}, seeds=[7, 8, 9], offsets=0, stop_tokens=[0, 261], check_every=0)


def test_generate_queue_argument_checks(model):
    m, lib = model
    for bad in (dict(prompts=[], max_tokens=4), dict(prompts=[[1]] * 257, max_tokens=4), dict(prompts=[[1], []], max_tokens=4),
                dict(prompts=[[1]], max_tokens=0), dict(prompts=[[1], [2]], max_tokens=[4, 0]),
                dict(prompts=[[1], [2]], max_tokens=[4]), dict(prompts=[[1]], max_tokens=65537),
                dict(prompts=[[1]], max_tokens=4, lanes=0), dict(prompts=[[1]], max_tokens=4, lanes=257),
                dict(prompts=[[1], [2]], max_tokens=4, temperature=[1.0]),
                dict(prompts=[[1], [2]], max_tokens=4, seeds=[1, 2, 3])):
        with pytest.raises(ValueError):
            m.generate_queue(**bad)
    assert lib.log == [], 'a refused call reached the library'
