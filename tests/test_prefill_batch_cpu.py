"""Batched prefill without a GPU: the host planner through the library's export and, as a stand-alone
program, under the host sanitizers; the Python binding and RWKVModel.prefill_batch /
generate_batch(batched_prefill=True) against a fake library object that records what it is asked
to do."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'rwkv.cppy_amd', 'python'))

from rwkv_cpp.rwkv_cpp_model import RWKVModel  # noqa: E402
from rwkv_cpp.rwkv_cpp_shared_library import RWKVSharedLibrary  # noqa: E402

FILL = 0xFFFFFFFF
CAPS = [1, 8, 1024]


# ------------------------------------------------------------------------------------ the planner
def planner():
    from rwkv_lib import library
    return library().rwkv_mi355x_selftest_prefill_plan


def hand_cases(cap):
    return [[1], [cap], [cap + 1], [3 * cap + 1], [1] * 256]


def random_cases(cap):
    rng = np.random.default_rng(1000 + cap)
    out = []
    for it in range(12):
        n = int(rng.integers(1, 257))
        top = 3 * cap + 2 if it % 2 else 9
        out.append([int(x) for x in rng.integers(1, top + 1, n)])
    return out


def check_plan(lengths, cap):
    plan = planner()
    total = sum(lengths)
    n_chunks = -(-total // cap)
    bound = len(lengths) + n_chunks - 1
    count, rows, begins, lens, chunks = plan(lengths, cap, bound)
    assert 0 < count <= bound, (lengths[:8], cap)
    rows, begins, lens, chunks = (a[:count].astype(np.int64) for a in (rows, begins, lens, chunks))
    # every row's tokens exactly once and in order: the rows never go back, and a row's pieces add up
    assert (np.diff(rows) >= 0).all() and (lens >= 1).all()
    assert np.array_equal(np.bincount(rows, weights=lens, minlength=len(lengths)).astype(np.int64), np.array(lengths))
    # the segments tile the chunks in order: a chunk holds at most cap tokens, every one but the last is full
    assert (np.diff(chunks) >= 0).all() and chunks[0] == 0 and chunks[-1] == n_chunks - 1
    for c in range(n_chunks):
        sel = chunks == c
        assert begins[sel][0] == 0 and np.array_equal(begins[sel][1:], np.cumsum(lens[sel])[:-1]), c
        filled = int(lens[sel].sum())
        assert filled == (cap if c < n_chunks - 1 else total - cap * (n_chunks - 1)) and filled <= cap, c
    # a split row's pieces sit in consecutive chunks
    for r in np.flatnonzero(np.bincount(rows) > 1):
        assert np.array_equal(np.diff(chunks[rows == r]), np.ones((rows == r).sum() - 1)), r
    # a table that is too small is reported and not overrun
    if count > 1:
        short = plan(lengths, cap, count - 1)
        assert short[0] == -1
    wide = plan(lengths, cap, count + 3)
    assert wide[0] == count and all((a[count:] == FILL).all() for a in wide[1:])
    return count


@pytest.mark.parametrize('cap', CAPS)
def test_planner_hand_cases(cap):
    counts = [check_plan(lengths, cap) for lengths in hand_cases(cap)]
    # [1], [cap]: one piece; [cap + 1]: two; [3 cap + 1]: four; 256 ones: 256
    assert counts == [1, 1, 2, 4, 256]


@pytest.mark.parametrize('cap', CAPS)
def test_planner_random_cases(cap):
    for lengths in random_cases(cap):
        check_plan(lengths, cap)


def test_planner_refuses_bad_arguments():
    plan = planner()
    assert plan([3, 0, 2], 8)[0] == -2
    assert plan([], 8, 4)[0] == -2
    assert plan([3], 0, 4)[0] == -2


def test_planner_under_host_sanitizers(tmp_path):
    """The same cases from a stand-alone program (tests/prefill_plan_host.cpp) built with
    -fsanitize=address,undefined: host code only, run directly."""
    cxx = next((c for c in ('g++', 'clang++', 'c++') if shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler (g++, clang++ or c++) on PATH')
    exe = str(tmp_path / 'prefill_plan_host')
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-I', os.path.join(REPO, 'rwkv.cppy_amd', 'csrc'), os.path.join(REPO, 'tests', 'prefill_plan_host.cpp'),
                            '-o', exe], capture_output=True, text=True)
    if build.returncode != 0 and ('asan' in build.stderr or 'ubsan' in build.stderr or 'sanitize' in build.stderr):
        pytest.skip(f'{cxx} has no sanitizer runtime here: {build.stderr.strip().splitlines()[-1]}')
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'prefill_plan: ok' in run.stdout


# ------------------------------------------------------------------------------------ the binding
class RawLibrary:
    """The ctypes library as the binding sees it: records the arrays of one prefill call."""

    def __init__(self, ok=True):
        self.ok = ok
        self.calls = []

    def rwkv_mi355x_prefill_batch(self, ptr, n_rows, slots, tokens, lengths, cont):
        total = sum(lengths[i] for i in range(n_rows))
        self.calls.append(dict(ptr=ptr, n_rows=n_rows, slots=[slots[i] for i in range(n_rows)],
                               tokens=[tokens[i] for i in range(total)], lengths=[lengths[i] for i in range(n_rows)],
                               cont=None if cont is None else [cont[i] for i in range(n_rows)]))
        return self.ok


class FakeCtx:
    ptr = 1234


def binding(raw):
    lib = RWKVSharedLibrary.__new__(RWKVSharedLibrary)
    lib.library = raw
    return lib


def test_binding_concatenates_the_prompts():
    raw = RawLibrary()
    lib = binding(raw)
    lib.rwkv_mi355x_prefill_batch(FakeCtx(), [[1, 2, 3], [4], [5, 6]], [2, 0, 1])
    lib.rwkv_mi355x_prefill_batch(FakeCtx(), [[7], [8, 9]], [1, 3], [True, False])
    assert raw.calls == [dict(ptr=1234, n_rows=3, slots=[2, 0, 1], tokens=[1, 2, 3, 4, 5, 6], lengths=[3, 1, 2], cont=None),
                         dict(ptr=1234, n_rows=2, slots=[1, 3], tokens=[7, 8, 9], lengths=[1, 2], cont=[1, 0])]
    assert isinstance(raw.calls[0]['lengths'][0], int)
    with pytest.raises(ValueError):
        lib.rwkv_mi355x_prefill_batch(FakeCtx(), [[1], [2]], [0])
    with pytest.raises(ValueError):
        lib.rwkv_mi355x_prefill_batch(FakeCtx(), [[1], [2]], [0, 1], [True])
    assert len(raw.calls) == 2
    with pytest.raises(ValueError):
        binding(RawLibrary(ok=False)).rwkv_mi355x_prefill_batch(FakeCtx(), [[1]], [0])


# ------------------------------------------------------------------------------------ RWKVModel
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

    def rwkv_mi355x_prefill_batch(self, ctx, prompts, slots, cont=None):
        self.log.append(('prefill', tuple(tuple(p) for p in prompts), tuple(slots), None if cont is None else tuple(cont)))

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


def test_generate_batch_with_batched_prefill(model):
    m, lib = model
    prompts = [[1, 2, 3], [4, 5], [6]]
    out = m.generate_batch(prompts, 4, batched_prefill=True)
    assert lib.log == [('reserve', 3), ('prefill', ((1, 2, 3), (4, 5), (6,)), (0, 1, 2), None), ('generate', 3, 4)]
    assert out == [[0], [10, 11], [20, 21, 22]]
    # the default is the per-row loop, call for call
    lib.log.clear()
    assert m.generate_batch(prompts[:2], 4) == out[:2]
    assert lib.log == [('reset',), ('eval', (1, 2, 3)), ('store', 0), ('reset',), ('eval', (4, 5)), ('store', 1),
                       ('generate', 2, 4)]


def test_prefill_batch_slots_and_cont(model):
    m, lib = model
    m.prefill_batch([[1, 2], [3]])
    assert lib.log == [('reserve', 2), ('prefill', ((1, 2), (3,)), (0, 1), (False, False))]
    # enough slots: no second reservation, whatever the slots
    lib.log.clear()
    m.prefill_batch([(4,), (5, 6)], slots=[1, 0], cont=[True, False])
    assert lib.log == [('prefill', ((4,), (5, 6)), (1, 0), (True, False))]
    # too few: reserved up to the highest slot named
    lib.log.clear()
    m.prefill_batch([[7]], slots=[5])
    assert lib.log == [('reserve', 6), ('prefill', ((7,),), (5,), (False,))]
    lib.log.clear()
    m.prefill_batch([[7], [8]], cont=True)
    assert lib.log == [('prefill', ((7,), (8,)), (0, 1), (True, True))]


def test_prefill_batch_argument_checks(model):
    m, lib = model
    for bad in (dict(prompts=[]), dict(prompts=[[1]] * 257), dict(prompts=[[1], []]), dict(prompts=[[1], [2]], slots=[0, 0]),
                dict(prompts=[[1], [2]], slots=[0]), dict(prompts=[[1], [2]], slots=[0, 256]),
                dict(prompts=[[1], [2]], cont=[True]), dict(prompts=[[1]], slots=[3], cont=True)):
        with pytest.raises(ValueError):
            m.prefill_batch(**bad)
    with pytest.raises(ValueError):
        m.generate_batch([[1], []], 4, batched_prefill=True)
    assert lib.log == [], 'a refused call reached the library'
