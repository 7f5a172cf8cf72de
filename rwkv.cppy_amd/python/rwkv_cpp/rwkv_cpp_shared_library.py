"""ctypes binding of librwkv.so (the MI355X build).

Mirrors the reference's python/rwkv_cpp/rwkv_cpp_shared_library.py interface
(RWKVSharedLibrary, RWKVContext, load_rwkv_shared_library) -- same method names,
argument meaning and error behaviour (ValueError on failure) -- so callers written
against the reference run unchanged.  Argument types match the reference bindings
(rwkv_cpp_shared_library.py:49-107): tokens are passed as int32 (same bits as uint32).
The additive rwkv_mi355x_* entry points (include/rwkv_mi355x.h) are bound too.
"""
import collections
import ctypes
import os
import pathlib
import sys
from typing import Tuple, List, Optional

QUANTIZED_FORMAT_NAMES = ('Q4_0', 'Q4_1', 'Q5_0', 'Q5_1', 'Q8_0')

P_FLOAT = ctypes.POINTER(ctypes.c_float)
P_INT = ctypes.POINTER(ctypes.c_int32)


class RWKVContext:
    def __init__(self, ptr):
        self.ptr = ptr


class RWKVSampling(ctypes.Structure):
    """struct rwkv_mi355x_sampling (include/rwkv_mi355x.h)."""
    _fields_ = [('temperature', ctypes.c_float), ('top_p', ctypes.c_float), ('n_bias', ctypes.c_uint32),
                ('bias_ids', ctypes.POINTER(ctypes.c_uint32)), ('bias_values', P_FLOAT),
                ('seed', ctypes.c_uint64), ('offset', ctypes.c_uint64)]


class RWKVSynthOpts(ctypes.Structure):
    """struct rwkv_mi355x_synth_opts (include/rwkv_mi355x.h); all zero = the plain synthetic writer."""
    _fields_ = [(n, ctypes.c_uint32) for n in ('norms', 'wide_decay', 'maa_d', 'decay_d', 'w_d', 'a_d', 'v_d', 'g_d')]


def make_sampling(temperature: float = 1.0, top_p: float = 0.8, logit_bias=None, seed: int = 0,
                  offset: int = 0) -> RWKVSampling:
    """Fills an RWKVSampling; logit_bias: {token id: value}.  The bias arrays stay referenced by the
    returned structure."""
    bias = dict(logit_bias or {})
    ids = (ctypes.c_uint32 * max(1, len(bias)))(*bias.keys())
    values = (ctypes.c_float * max(1, len(bias)))(*bias.values())
    p = RWKVSampling(temperature, top_p, len(bias), ctypes.cast(ids, ctypes.POINTER(ctypes.c_uint32)),
                     ctypes.cast(values, P_FLOAT), seed & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFFFFFFFFFF)
    p._keep = (ids, values)
    return p


class RWKVBatchSampling(ctypes.Structure):
    """struct rwkv_mi355x_batch_sampling (include/rwkv_mi355x.h)."""
    _fields_ = [('temperature', P_FLOAT), ('top_p', P_FLOAT), ('presence', P_FLOAT), ('frequency', P_FLOAT),
                ('seed', ctypes.POINTER(ctypes.c_uint64)), ('offset', ctypes.POINTER(ctypes.c_uint64)),
                ('n_bias', ctypes.c_uint32), ('bias_ids', ctypes.POINTER(ctypes.c_uint32)), ('bias_values', P_FLOAT),
                ('n_stop', ctypes.c_uint32), ('stop_tokens', ctypes.POINTER(ctypes.c_uint32)),
                ('keep_counts', ctypes.c_uint32), ('check_every', ctypes.c_uint32)]


class RWKVLogprobs(ctypes.Structure):
    """struct rwkv_mi355x_logprobs (include/rwkv_mi355x.h)."""
    _fields_ = [('top_k', ctypes.c_uint32), ('token_logprob', ctypes.POINTER(ctypes.c_double)),
                ('top_ids', ctypes.POINTER(ctypes.c_uint32)), ('top_logprobs', ctypes.POINTER(ctypes.c_double))]


# What a call with logprobs=K returns besides its tokens: the drawn tokens' log-probabilities
# (float64 [n]) and the K most likely alternatives of every draw (uint32 / float64 [n, K]).
Logprobs = collections.namedtuple('Logprobs', ('token_logprob', 'top_ids', 'top_logprobs'))

MAX_TOP_LOGPROBS = 20


def make_logprobs(rows: int, n: int, top_k: int):
    """Host arrays [rows, n] (and [rows, n, top_k]) for a call with log-probabilities and the
    RWKVLogprobs pointing at them.  The arrays start as a pattern the library never writes (0xA5
    bytes); the library fills every column: drawn values, or its own fill (0xFF bytes) elsewhere."""
    import numpy as np
    top_k = int(top_k)
    if not 0 <= top_k <= MAX_TOP_LOGPROBS:
        raise ValueError(f'logprobs must be in [0, {MAX_TOP_LOGPROBS}]')
    arrays = Logprobs(np.full((rows, n), 0xA5A5A5A5A5A5A5A5, np.uint64).view(np.float64),
                      np.full((rows, n, top_k), 0xA5A5A5A5, np.uint32),
                      np.full((rows, n, top_k), 0xA5A5A5A5A5A5A5A5, np.uint64).view(np.float64))
    lp = RWKVLogprobs(top_k, arrays.token_logprob.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                      arrays.top_ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                      arrays.top_logprobs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    lp._keep = arrays
    return lp, arrays


def _per_row(value, rows: int, name: str) -> list:
    """A scalar repeated for every row, or a sequence of exactly `rows` values."""
    if hasattr(value, '__len__'):
        if len(value) != rows:
            raise ValueError(f'{name}: {len(value)} values for {rows} rows')
        return list(value)
    return [value] * rows


def make_batch_sampling(rows: int, temperature=1.0, top_p=0.8, presence=None, frequency=None, logit_bias=None,
                        seeds=None, offsets=0, stop_tokens=(), keep_counts: bool = False,
                        check_every: int = 0) -> RWKVBatchSampling:
    """Fills an RWKVBatchSampling for `rows` rows.  temperature, top_p, presence, frequency, seeds and
    offsets are scalars (the same for every row) or sequences of `rows` values; presence / frequency
    None leave the structure's pointer NULL (no penalty); seeds None gives row r the seed r.
    logit_bias: {token id: value}, shared by the rows.  The arrays stay referenced by the returned
    structure."""
    if not rows > 0:
        raise ValueError('rows must be > 0')
    P_U32, P_U64 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    keep = []

    def floats(value, name):
        if value is None:
            return ctypes.cast(None, P_FLOAT)
        arr = (ctypes.c_float * rows)(*[float(v) for v in _per_row(value, rows, name)])
        keep.append(arr)
        return ctypes.cast(arr, P_FLOAT)

    def words(value, name):
        arr = (ctypes.c_uint64 * rows)(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in _per_row(value, rows, name)])
        keep.append(arr)
        return ctypes.cast(arr, P_U64)

    bias = dict(logit_bias or {})
    ids = (ctypes.c_uint32 * max(1, len(bias)))(*bias.keys())
    values = (ctypes.c_float * max(1, len(bias)))(*bias.values())
    stops = list(stop_tokens)
    stop_arr = (ctypes.c_uint32 * max(1, len(stops)))(*stops)
    keep += [ids, values, stop_arr]
    p = RWKVBatchSampling(floats(temperature, 'temperature'), floats(top_p, 'top_p'), floats(presence, 'presence'),
                          floats(frequency, 'frequency'), words(range(rows) if seeds is None else seeds, 'seeds'),
                          words(offsets, 'offsets'), len(bias), ctypes.cast(ids, P_U32), ctypes.cast(values, P_FLOAT),
                          len(stops), ctypes.cast(stop_arr, P_U32), 1 if keep_counts else 0, int(check_every))
    p._keep = keep
    return p


class RWKVSharedLibrary:
    """Python wrapper around librwkv.so."""

    def __init__(self, shared_library_path: str) -> None:
        self.library = ctypes.cdll.LoadLibrary(shared_library_path)
        L = self.library
        vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32

        L.rwkv_init_from_file.argtypes = [ctypes.c_char_p, u32, u32]
        L.rwkv_init_from_file.restype = vp
        L.rwkv_clone_context.argtypes = [vp, u32]
        L.rwkv_clone_context.restype = vp
        L.rwkv_eval.argtypes = [vp, ctypes.c_int32, P_FLOAT, P_FLOAT, P_FLOAT]
        L.rwkv_eval.restype = ctypes.c_bool
        L.rwkv_eval_sequence.argtypes = [vp, P_INT, sz, P_FLOAT, P_FLOAT, P_FLOAT]
        L.rwkv_eval_sequence.restype = ctypes.c_bool
        L.rwkv_eval_sequence_in_chunks.argtypes = [vp, P_INT, sz, sz, P_FLOAT, P_FLOAT, P_FLOAT]
        L.rwkv_eval_sequence_in_chunks.restype = ctypes.c_bool
        for name in ('rwkv_get_n_vocab', 'rwkv_get_n_embed', 'rwkv_get_n_layer', 'rwkv_get_state_len',
                     'rwkv_get_logits_len'):
            getattr(L, name).argtypes = [vp]
            getattr(L, name).restype = sz
        L.rwkv_get_state_buffer_element_count.argtypes = [vp]
        L.rwkv_get_state_buffer_element_count.restype = u32
        L.rwkv_get_logits_buffer_element_count.argtypes = [vp]
        L.rwkv_get_logits_buffer_element_count.restype = u32
        L.rwkv_init_state.argtypes = [vp, P_FLOAT]
        L.rwkv_init_state.restype = None
        L.rwkv_free.argtypes = [vp]
        L.rwkv_free.restype = None
        L.rwkv_quantize_model_file.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
        L.rwkv_quantize_model_file.restype = ctypes.c_bool
        L.rwkv_get_system_info_string.argtypes = []
        L.rwkv_get_system_info_string.restype = ctypes.c_char_p
        L.rwkv_set_print_errors.argtypes = [vp, ctypes.c_bool]
        L.rwkv_set_print_errors.restype = None
        L.rwkv_get_print_errors.argtypes = [vp]
        L.rwkv_get_print_errors.restype = ctypes.c_bool
        L.rwkv_get_last_error.argtypes = [vp]
        L.rwkv_get_last_error.restype = ctypes.c_int

        # additive MI355X extensions
        L.rwkv_mi355x_state_upload.argtypes = [vp, P_FLOAT]
        L.rwkv_mi355x_state_upload.restype = ctypes.c_bool
        L.rwkv_mi355x_state_download.argtypes = [vp, P_FLOAT]
        L.rwkv_mi355x_state_download.restype = ctypes.c_bool
        L.rwkv_mi355x_eval_device.argtypes = [vp, P_INT, sz, ctypes.c_bool, P_FLOAT, ctypes.c_bool]
        L.rwkv_mi355x_eval_device.restype = ctypes.c_bool
        L.rwkv_mi355x_eval_layers.argtypes = [vp, vp, sz, u32, u32, vp, vp, ctypes.c_bool, P_FLOAT]
        L.rwkv_mi355x_eval_layers.restype = ctypes.c_bool
        L.rwkv_mi355x_eval_layers_async.argtypes = [vp, vp, sz, u32, u32, vp, vp, ctypes.c_bool]
        L.rwkv_mi355x_eval_layers_async.restype = ctypes.c_bool
        L.rwkv_mi355x_logits_device.argtypes = [vp]
        L.rwkv_mi355x_logits_device.restype = vp
        L.rwkv_mi355x_init_from_file_layers.argtypes = [ctypes.c_char_p, u32, u32, u32]
        L.rwkv_mi355x_init_from_file_layers.restype = vp
        L.rwkv_mi355x_debug_buffer.argtypes = [vp, ctypes.c_char_p, vp, sz]
        L.rwkv_mi355x_debug_buffer.restype = ctypes.c_longlong
        L.rwkv_mi355x_sync.argtypes = [vp]
        L.rwkv_mi355x_sync.restype = ctypes.c_bool
        L.rwkv_mi355x_stream.argtypes = [vp]
        L.rwkv_mi355x_stream.restype = vp
        L.rwkv_mi355x_device_state.argtypes = [vp]
        L.rwkv_mi355x_device_state.restype = vp
        L.rwkv_mi355x_decode_bytes.argtypes = [vp, ctypes.c_bool]
        L.rwkv_mi355x_decode_bytes.restype = ctypes.c_double
        L.rwkv_mi355x_weight_bytes.argtypes = [vp, ctypes.c_bool]
        L.rwkv_mi355x_weight_bytes.restype = ctypes.c_double
        L.rwkv_mi355x_matmul_flops_per_token.argtypes = [vp, ctypes.c_bool]
        L.rwkv_mi355x_matmul_flops_per_token.restype = ctypes.c_double
        L.rwkv_mi355x_arch.argtypes = [vp, ctypes.POINTER(ctypes.c_int64)]
        L.rwkv_mi355x_arch.restype = None
        L.rwkv_mi355x_write_synthetic_model.argtypes = [ctypes.c_char_p, ctypes.c_int, u32, u32, u32, u32,
                                                        ctypes.c_char_p, ctypes.c_uint64]
        L.rwkv_mi355x_write_synthetic_model.restype = ctypes.c_bool
        L.rwkv_mi355x_write_synthetic_model_ex.argtypes = [ctypes.c_char_p, ctypes.c_int, u32, u32, u32, u32,
                                                           ctypes.c_char_p, ctypes.c_uint64,
                                                           ctypes.POINTER(RWKVSynthOpts)]
        L.rwkv_mi355x_write_synthetic_model_ex.restype = ctypes.c_bool
        L.rwkv_mi355x_selftest_groupnorm.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                     ctypes.c_int] + [P_FLOAT] * 7
        L.rwkv_mi355x_selftest_groupnorm.restype = ctypes.c_bool
        L.rwkv_mi355x_selftest_ln.argtypes = [ctypes.c_int, ctypes.c_int] + [P_FLOAT] * 4
        L.rwkv_mi355x_selftest_ln.restype = ctypes.c_bool
        L.rwkv_mi355x_eval_batch.argtypes = [vp, vp, sz, vp, vp, vp]
        L.rwkv_mi355x_eval_batch.restype = ctypes.c_bool
        L.rwkv_mi355x_eval_batch_device.argtypes = [vp, vp, sz, vp, vp, vp]
        L.rwkv_mi355x_eval_batch_device.restype = ctypes.c_bool
        L.rwkv_mi355x_set_kernel_timing.argtypes = [vp, ctypes.c_bool]
        L.rwkv_mi355x_set_kernel_timing.restype = None
        L.rwkv_mi355x_kernel_stats.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_longlong),
                                               ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(ctypes.c_double)]
        L.rwkv_mi355x_kernel_stats.restype = ctypes.c_int
        L.rwkv_mi355x_layer_state_len.argtypes = [vp]
        L.rwkv_mi355x_layer_state_len.restype = sz
        L.rwkv_mi355x_state_upload_layers.argtypes = [vp, vp, u32, u32]
        L.rwkv_mi355x_state_upload_layers.restype = ctypes.c_bool
        L.rwkv_mi355x_state_download_layers.argtypes = [vp, vp, u32, u32]
        L.rwkv_mi355x_state_download_layers.restype = ctypes.c_bool
        L.rwkv_mi355x_state_io_bytes.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.rwkv_mi355x_state_io_bytes.restype = None
        L.rwkv_mi355x_clone_context_on.argtypes = [vp, u32, ctypes.c_int]
        L.rwkv_mi355x_clone_context_on.restype = vp
        L.rwkv_mi355x_context_device.argtypes = [vp]
        L.rwkv_mi355x_context_device.restype = ctypes.c_int
        L.rwkv_mi355x_init_pipeline.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        L.rwkv_mi355x_init_pipeline.restype = vp
        L.rwkv_mi355x_pipeline_stages.argtypes = [vp]
        L.rwkv_mi355x_pipeline_stages.restype = ctypes.c_int
        L.rwkv_mi355x_pipeline_peer_pairs.argtypes = [vp]
        L.rwkv_mi355x_pipeline_peer_pairs.restype = ctypes.c_int
        L.rwkv_mi355x_debug_set.argtypes = [vp, ctypes.c_char_p, ctypes.c_longlong]
        L.rwkv_mi355x_debug_set.restype = ctypes.c_bool
        P_SAMPLING, P_U32 = ctypes.POINTER(RWKVSampling), ctypes.POINTER(ctypes.c_uint32)
        L.rwkv_mi355x_sample.argtypes = [vp, P_SAMPLING, P_U32]
        L.rwkv_mi355x_sample.restype = ctypes.c_bool
        L.rwkv_mi355x_generate.argtypes = [vp, P_SAMPLING, sz, P_U32, P_FLOAT]
        L.rwkv_mi355x_generate.restype = ctypes.c_bool
        L.rwkv_mi355x_selftest_sample.argtypes = [P_FLOAT, ctypes.c_int, ctypes.c_int, P_SAMPLING, P_FLOAT, P_U32, P_U32,
                                                  P_FLOAT]
        L.rwkv_mi355x_selftest_sample.restype = ctypes.c_bool
        P_BATCH = ctypes.POINTER(RWKVBatchSampling)
        L.rwkv_mi355x_batch_reserve.argtypes = [vp, sz]
        L.rwkv_mi355x_batch_reserve.restype = ctypes.c_bool
        L.rwkv_mi355x_batch_slots.argtypes = [vp]
        L.rwkv_mi355x_batch_slots.restype = sz
        L.rwkv_mi355x_batch_store.argtypes = [vp, sz]
        L.rwkv_mi355x_batch_store.restype = ctypes.c_bool
        L.rwkv_mi355x_batch_load.argtypes = [vp, sz]
        L.rwkv_mi355x_batch_load.restype = ctypes.c_bool
        L.rwkv_mi355x_generate_batch.argtypes = [vp, sz, P_BATCH, sz, P_U32, P_U32, P_U32]
        L.rwkv_mi355x_generate_batch.restype = ctypes.c_bool
        L.rwkv_mi355x_generate_queue.argtypes = [vp, sz, sz, P_BATCH, P_U32, sz, P_U32, P_U32, P_U32, P_U32, P_U32]
        L.rwkv_mi355x_generate_queue.restype = ctypes.c_bool
        L.rwkv_mi355x_selftest_gen_turnover.argtypes = [ctypes.c_int, ctypes.c_int, u32] + [P_U32] * 10
        L.rwkv_mi355x_selftest_gen_turnover.restype = ctypes.c_bool
        P_SIZE = ctypes.POINTER(sz)
        L.rwkv_mi355x_prefill_batch.argtypes = [vp, sz, P_U32, P_U32, P_SIZE, ctypes.POINTER(ctypes.c_uint8)]
        L.rwkv_mi355x_prefill_batch.restype = ctypes.c_bool
        L.rwkv_mi355x_selftest_prefill_plan.argtypes = [P_SIZE, sz, sz, P_U32, P_U32, P_U32, P_U32, sz]
        L.rwkv_mi355x_selftest_prefill_plan.restype = ctypes.c_longlong
        L.rwkv_mi355x_selftest_sample_rows.argtypes = [P_FLOAT, ctypes.c_int, ctypes.c_int, P_BATCH, P_FLOAT, u32, P_U32,
                                                       P_U32, P_U32, P_U32, P_U32, P_FLOAT, P_U32, P_U32]
        L.rwkv_mi355x_selftest_sample_rows.restype = ctypes.c_bool
        P_DOUBLE, P_LP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(RWKVLogprobs)
        L.rwkv_mi355x_sample_logprobs.argtypes = L.rwkv_mi355x_sample.argtypes + [P_LP]
        L.rwkv_mi355x_generate_logprobs.argtypes = L.rwkv_mi355x_generate.argtypes + [P_LP]
        L.rwkv_mi355x_generate_batch_logprobs.argtypes = L.rwkv_mi355x_generate_batch.argtypes + [P_LP]
        L.rwkv_mi355x_generate_queue_logprobs.argtypes = L.rwkv_mi355x_generate_queue.argtypes + [P_LP]
        L.rwkv_mi355x_selftest_sample_logprobs.argtypes = L.rwkv_mi355x_selftest_sample.argtypes + [
            u32, P_DOUBLE, P_U32, P_DOUBLE]
        L.rwkv_mi355x_selftest_sample_rows_logprobs.argtypes = L.rwkv_mi355x_selftest_sample_rows.argtypes + [
            u32, P_DOUBLE, P_U32, P_DOUBLE]
        for name in ('sample', 'generate', 'generate_batch', 'generate_queue', 'selftest_sample', 'selftest_sample_rows'):
            getattr(L, f'rwkv_mi355x_{name}_logprobs').restype = ctypes.c_bool
        L.rwkv_mi355x_score_sequence.argtypes = [vp, P_U32, sz, P_U32, P_DOUBLE, P_U32, P_FLOAT]
        L.rwkv_mi355x_score_sequence.restype = ctypes.c_bool
        L.rwkv_mi355x_selftest_xent.argtypes = [P_FLOAT, ctypes.c_int, ctypes.c_int, P_U32, P_DOUBLE, P_U32]
        L.rwkv_mi355x_selftest_xent.restype = ctypes.c_bool
        L.rwkv_mi355x_selftest_wkv_layouts.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, P_U32, ctypes.c_int,
                                                       ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        L.rwkv_mi355x_selftest_wkv_layouts.restype = ctypes.c_bool

        self.nullptr = ctypes.cast(0, ctypes.c_void_p)

    # ---- reference interface ----------------------------------------------------------
    def rwkv_init_from_file(self, model_file_path: str, thread_count: int, offload_layers: int) -> RWKVContext:
        ptr = self.library.rwkv_init_from_file(model_file_path.encode('utf-8'), ctypes.c_uint32(thread_count),
                                               ctypes.c_uint32(offload_layers))
        if ptr is None:
            raise ValueError('rwkv_init_from_file failed, check stderr')
        return RWKVContext(ptr)

    def rwkv_eval(self, ctx: RWKVContext, token: int, state_in_address: Optional[int], state_out_address: int,
                  logits_out_address: int) -> None:
        if not self.library.rwkv_eval(ctx.ptr, ctypes.c_int32(token),
                                      ctypes.cast(0 if state_in_address is None else state_in_address, P_FLOAT),
                                      ctypes.cast(state_out_address, P_FLOAT),
                                      ctypes.cast(logits_out_address, P_FLOAT)):
            raise ValueError('rwkv_eval failed, check stderr')

    def rwkv_eval_sequence(self, ctx: RWKVContext, tokens: List[int], state_in_address: Optional[int],
                           state_out_address: int, logits_out_address: int) -> None:
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        if not self.library.rwkv_eval_sequence(ctx.ptr, ctypes.cast(arr, P_INT), ctypes.c_size_t(len(tokens)),
                                               ctypes.cast(0 if state_in_address is None else state_in_address, P_FLOAT),
                                               ctypes.cast(state_out_address, P_FLOAT),
                                               ctypes.cast(logits_out_address, P_FLOAT)):
            raise ValueError('rwkv_eval_sequence failed, check stderr')

    def rwkv_eval_sequence_in_chunks(self, ctx: RWKVContext, tokens: List[int], chunk_size: int,
                                     state_in_address: Optional[int], state_out_address: int,
                                     logits_out_address: int) -> None:
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        if not self.library.rwkv_eval_sequence_in_chunks(
                ctx.ptr, ctypes.cast(arr, P_INT), ctypes.c_size_t(len(tokens)), ctypes.c_size_t(chunk_size),
                ctypes.cast(0 if state_in_address is None else state_in_address, P_FLOAT),
                ctypes.cast(state_out_address, P_FLOAT), ctypes.cast(logits_out_address, P_FLOAT)):
            raise ValueError('rwkv_eval_sequence_in_chunks failed, check stderr')

    def rwkv_get_n_vocab(self, ctx: RWKVContext) -> int:
        return self.library.rwkv_get_n_vocab(ctx.ptr)

    def rwkv_get_n_embed(self, ctx: RWKVContext) -> int:
        return self.library.rwkv_get_n_embed(ctx.ptr)

    def rwkv_get_n_layer(self, ctx: RWKVContext) -> int:
        return self.library.rwkv_get_n_layer(ctx.ptr)

    def rwkv_get_state_buffer_element_count(self, ctx: RWKVContext) -> int:
        return self.library.rwkv_get_state_buffer_element_count(ctx.ptr)

    def rwkv_get_logits_buffer_element_count(self, ctx: RWKVContext) -> int:
        return self.library.rwkv_get_logits_buffer_element_count(ctx.ptr)

    def rwkv_free(self, ctx: RWKVContext) -> None:
        self.library.rwkv_free(ctx.ptr)
        ctx.ptr = self.nullptr

    def rwkv_quantize_model_file(self, model_file_path_in: str, model_file_path_out: str, format_name: str) -> None:
        if format_name not in QUANTIZED_FORMAT_NAMES:
            raise ValueError(f'Unknown format name {format_name}, use one of {QUANTIZED_FORMAT_NAMES}')
        if not self.library.rwkv_quantize_model_file(model_file_path_in.encode('utf-8'),
                                                     model_file_path_out.encode('utf-8'),
                                                     format_name.encode('utf-8')):
            raise ValueError('rwkv_quantize_model_file failed, check stderr')

    # ---- additive: batched decode (include/rwkv_mi355x.h) ------------------------------------
    def rwkv_mi355x_eval_batch(self, ctx: RWKVContext, tokens: List[int], state_in_address: Optional[int],
                               state_out_address: Optional[int], logits_out_address: Optional[int]) -> None:
        """len(tokens) contexts advance one token each; states [n][state_len], logits [n][n_vocab]
        (host addresses, None = fresh states / not returned).  Bit-identical to rwkv_eval per context."""
        arr = (ctypes.c_uint32 * len(tokens))(*tokens)
        if not self.library.rwkv_mi355x_eval_batch(ctx.ptr, ctypes.cast(arr, ctypes.c_void_p), len(tokens),
                                                   state_in_address, state_out_address, logits_out_address):
            raise ValueError('rwkv_mi355x_eval_batch failed, check stderr')

    # ---- additive: replicas on other GPUs and per-layer state slices ------------------------
    def rwkv_mi355x_clone_context_on(self, ctx: RWKVContext, thread_count: int, device: int) -> RWKVContext:
        """rwkv_clone_context onto GPU `device` (the model is uploaded once per GPU)."""
        ptr = self.library.rwkv_mi355x_clone_context_on(ctx.ptr, thread_count, device)
        if ptr is None:
            raise ValueError(f'rwkv_mi355x_clone_context_on(device={device}) failed, check stderr')
        return RWKVContext(ptr)

    def rwkv_mi355x_state_io_bytes(self, ctx: RWKVContext) -> Tuple[float, float]:
        """State bytes this context moved so far: (host->device, device->host)."""
        out = (ctypes.c_double * 2)()
        self.library.rwkv_mi355x_state_io_bytes(ctx.ptr, out)
        return out[0], out[1]

    # ---- additive: sampling and the generation loop on the device ---------------------------
    def rwkv_mi355x_sample(self, ctx: RWKVContext, temperature: float = 1.0, top_p: float = 0.8, logit_bias=None,
                           seed: int = 0, offset: int = 0, logprobs: Optional[int] = None):
        """One token drawn on the device from the context's logits (draw `offset` of stream `seed`);
        the state is untouched.  logprobs=K (rwkv_mi355x_sample_logprobs): returns (token, Logprobs)
        with the token's log-probability (a float) and the K most likely alternatives ([K] arrays)."""
        token = ctypes.c_uint32(0)
        p = make_sampling(temperature, top_p, logit_bias, seed, offset)
        if logprobs is None:
            if not self.library.rwkv_mi355x_sample(ctx.ptr, ctypes.byref(p), ctypes.byref(token)):
                raise ValueError('rwkv_mi355x_sample failed, check stderr')
            return token.value
        lp, out = make_logprobs(1, 1, logprobs)
        if not self.library.rwkv_mi355x_sample_logprobs(ctx.ptr, ctypes.byref(p), ctypes.byref(token), ctypes.byref(lp)):
            raise ValueError('rwkv_mi355x_sample_logprobs failed, check stderr')
        return token.value, Logprobs(float(out.token_logprob[0, 0]), out.top_ids[0, 0], out.top_logprobs[0, 0])

    def rwkv_mi355x_generate(self, ctx: RWKVContext, n: int, temperature: float = 1.0, top_p: float = 0.8,
                             logit_bias=None, seed: int = 0, offset: int = 0,
                             logits_out_address: Optional[int] = None, logprobs: Optional[int] = None):
        """n times (draw a token on the device, evaluate it) without a host round trip; returns the
        tokens.  Draw i uses counter offset + i, so a call with offset + n continues the stream.
        logprobs=K (rwkv_mi355x_generate_logprobs): returns (tokens, Logprobs of [n] / [n, K] arrays)."""
        tokens = (ctypes.c_uint32 * max(1, n))()
        p = make_sampling(temperature, top_p, logit_bias, seed, offset)
        logits_out = ctypes.cast(logits_out_address or 0, P_FLOAT)
        if logprobs is None:
            if not self.library.rwkv_mi355x_generate(ctx.ptr, ctypes.byref(p), n, tokens, logits_out):
                raise ValueError('rwkv_mi355x_generate failed, check stderr')
            return list(tokens[:n])
        lp, out = make_logprobs(1, max(1, n), logprobs)
        if not self.library.rwkv_mi355x_generate_logprobs(ctx.ptr, ctypes.byref(p), n, tokens, logits_out,
                                                          ctypes.byref(lp)):
            raise ValueError('rwkv_mi355x_generate_logprobs failed, check stderr')
        return list(tokens[:n]), Logprobs(*(x[0, :n] for x in out))

    def rwkv_mi355x_selftest_sample(self, logits, u, temperature: float = 1.0, top_p: float = 0.8, logit_bias=None,
                                    logprobs: Optional[int] = None, fill: int = 0xA5):
        """The sampler kernel on host logits [rows][V] (float32 numpy) with the draws u [rows] given.
        Returns (tokens, kept, cutoff) numpy arrays [rows].  logprobs=K
        (rwkv_mi355x_selftest_sample_logprobs): a fourth element, Logprobs of [rows] / [rows, K] arrays
        that start as bytes of `fill`, so an entry the kernels do not write keeps them."""
        import numpy as np
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        if logits.ndim == 1:
            logits = logits[None, :]
        rows, V = logits.shape
        u = np.ascontiguousarray(np.broadcast_to(np.asarray(u, dtype=np.float32), (rows,)))
        tokens, kept, cutoff = np.zeros(rows, np.uint32), np.zeros(rows, np.uint32), np.zeros(rows, np.float32)
        p = make_sampling(temperature, top_p, logit_bias)
        P_U32 = ctypes.POINTER(ctypes.c_uint32)
        args = (logits.ctypes.data_as(P_FLOAT), rows, V, ctypes.byref(p), u.ctypes.data_as(P_FLOAT),
                tokens.ctypes.data_as(P_U32), kept.ctypes.data_as(P_U32), cutoff.ctypes.data_as(P_FLOAT))
        if logprobs is None:
            if not self.library.rwkv_mi355x_selftest_sample(*args):
                raise ValueError('rwkv_mi355x_selftest_sample failed')
            return tokens, kept, cutoff
        lp = self._selftest_logprobs(rows, logprobs, fill)
        if not self.library.rwkv_mi355x_selftest_sample_logprobs(*args, *lp[0]):
            raise ValueError('rwkv_mi355x_selftest_sample_logprobs failed')
        return tokens, kept, cutoff, lp[1]

    @staticmethod
    def _selftest_logprobs(rows: int, top_k: int, fill: int):
        """The four trailing arguments of the *_logprobs self-tests and the Logprobs they fill."""
        import numpy as np
        out = Logprobs(np.full(rows * 8, fill, np.uint8).view(np.float64),
                       np.full(rows * max(1, top_k) * 4, fill, np.uint8).view(np.uint32).reshape(rows, -1),
                       np.full(rows * max(1, top_k) * 8, fill, np.uint8).view(np.float64).reshape(rows, -1))
        P_U32, P_DOUBLE = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
        args = (top_k, out.token_logprob.ctypes.data_as(P_DOUBLE), out.top_ids.ctypes.data_as(P_U32),
                out.top_logprobs.ctypes.data_as(P_DOUBLE))
        return args, Logprobs(out.token_logprob, out.top_ids[:, :top_k], out.top_logprobs[:, :top_k])

    def rwkv_mi355x_eval_device(self, ctx: RWKVContext, tokens: List[int], compute_logits: bool = True) -> None:
        """Evaluates the tokens on the device-resident state (the logits stay on the device);
        synchronous."""
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        if not self.library.rwkv_mi355x_eval_device(ctx.ptr, ctypes.cast(arr, P_INT), len(tokens), compute_logits,
                                                    None, True):
            raise ValueError('rwkv_mi355x_eval_device failed, check stderr')

    # ---- additive: batched generation on the device ------------------------------------------
    def rwkv_mi355x_batch_reserve(self, ctx: RWKVContext, n_slots: int) -> None:
        """Gives the context n_slots <= 256 generation slots (0 frees them); every slot is empty."""
        if not self.library.rwkv_mi355x_batch_reserve(ctx.ptr, n_slots):
            raise ValueError('rwkv_mi355x_batch_reserve failed, check stderr')

    def rwkv_mi355x_batch_slots(self, ctx: RWKVContext) -> int:
        return self.library.rwkv_mi355x_batch_slots(ctx.ptr)

    def rwkv_mi355x_batch_store(self, ctx: RWKVContext, slot: int) -> None:
        """The context's device state and logits go into the slot, which starts a new sequence."""
        if not self.library.rwkv_mi355x_batch_store(ctx.ptr, slot):
            raise ValueError('rwkv_mi355x_batch_store failed, check stderr')

    def rwkv_mi355x_batch_load(self, ctx: RWKVContext, slot: int) -> None:
        """The context continues from the slot's state and logits."""
        if not self.library.rwkv_mi355x_batch_load(ctx.ptr, slot):
            raise ValueError('rwkv_mi355x_batch_load failed, check stderr')

    def _generate_slots(self, name: str, ctx: RWKVContext, rows: int, n: int, logprobs: Optional[int], head: tuple,
                        extra: tuple = ()):
        """What rwkv_mi355x_generate_batch and rwkv_mi355x_generate_queue share: the output arrays of
        `rows` sequences and the plain / _logprobs entry point `name`, called with (ctx, *head, n,
        tokens, lengths, *extra, steps[, logprobs]).  Returns (tokens [rows, n], lengths [rows], steps,
        Logprobs of [rows, n] / [rows, n, K] arrays or None)."""
        import numpy as np
        tokens = np.zeros((rows, max(1, n)), np.uint32)
        lengths = np.zeros(rows, np.uint32)
        steps = ctypes.c_uint32(0)
        P_U32 = ctypes.POINTER(ctypes.c_uint32)
        args = (ctx.ptr, *head, n, tokens.ctypes.data_as(P_U32), lengths.ctypes.data_as(P_U32),
                *(x.ctypes.data_as(P_U32) for x in extra), ctypes.byref(steps))
        out = None
        if logprobs is not None:
            name += '_logprobs'
            lp, out = make_logprobs(rows, max(1, n), logprobs)
            args += (ctypes.byref(lp),)
        if not getattr(self.library, name)(*args):
            raise ValueError(f'{name} failed, check stderr')
        return tokens[:, :n], lengths, steps.value, out and Logprobs(*(x[:, :n] for x in out))

    def rwkv_mi355x_generate_batch(self, ctx: RWKVContext, rows: int, n: int, params: RWKVBatchSampling,
                                   logprobs: Optional[int] = None):
        """Up to n tokens for each of slots [0, rows) (make_batch_sampling).  Returns (tokens uint32
        [rows, n], 0xFFFFFFFF after a row's last token; lengths uint32 [rows]; the decode steps run).
        logprobs=K (rwkv_mi355x_generate_batch_logprobs): a fourth element, Logprobs of [rows, n] /
        [rows, n, K] arrays whose columns past a row's length hold the fill (NaN, 0xFFFFFFFF)."""
        out = self._generate_slots('rwkv_mi355x_generate_batch', ctx, rows, n, logprobs, (rows, ctypes.byref(params)))
        return out if logprobs is not None else out[:3]

    def rwkv_mi355x_generate_queue(self, ctx: RWKVContext, max_tokens, lanes: int, temperature=1.0, top_p=0.8,
                                   presence=None, frequency=None, logit_bias=None, seeds=None, offsets=0,
                                   stop_tokens=(), check_every: int = 0, n: Optional[int] = None,
                                   logprobs: Optional[int] = None):
        """The sequences in slots [0, len(max_tokens)) through a queue over `lanes` decode rows, at most
        max_tokens[s] tokens each (make_batch_sampling over the sequences, keep_counts false).  Returns
        a dict: tokens uint32 [Q, n] (n: max(max_tokens) unless given; 0xFFFFFFFF after a sequence's
        last token), lengths, lane, start uint32 [Q] and steps, the decode steps that were needed.
        logprobs=K (rwkv_mi355x_generate_queue_logprobs) adds 'logprobs': Logprobs of [Q, n] / [Q, n, K]
        arrays."""
        import numpy as np
        caps = np.ascontiguousarray(max_tokens, dtype=np.uint32)
        Q = int(caps.size)
        params = make_batch_sampling(Q, temperature, top_p, presence, frequency, logit_bias, seeds, offsets,
                                     stop_tokens, False, check_every)
        n = int(caps.max()) if n is None else int(n)
        out = {k: np.zeros(Q, np.uint32) for k in ('lane', 'start')}
        head = (Q, lanes, ctypes.byref(params), caps.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        out['tokens'], out['lengths'], out['steps'], lp = self._generate_slots(
            'rwkv_mi355x_generate_queue', ctx, Q, n, logprobs, head, (out['lane'], out['start']))
        if logprobs is not None:
            out['logprobs'] = lp
        return out

    def rwkv_mi355x_selftest_gen_turnover(self, lane_seq, done, length, max_tokens, next_seq: int, step: int = 0,
                                          fill: int = 0xFFFFFFFE):
        """The queue's turnover kernel on host operands: lane_seq [lanes] (0xFFFFFFFF: idle), done,
        length, max_tokens [Q], the first waiting sequence.  Returns a dict of the words afterwards:
        lane_seq, retire_to, admit_from [lanes]; done, lane, start [Q] (lane and start keep `fill`
        where no sequence was admitted); next, active."""
        import numpy as np
        u32 = lambda a: np.array(a, dtype=np.uint32, copy=True)  # noqa: E731
        out = dict(lane_seq=u32(lane_seq), done=u32(done))
        lanes, Q = out['lane_seq'].size, out['done'].size
        length, max_tokens = u32(length), u32(max_tokens)
        assert length.size == Q and max_tokens.size == Q
        out.update(lane=np.full(Q, fill, np.uint32), start=np.full(Q, fill, np.uint32),
                   retire_to=np.full(lanes, fill, np.uint32), admit_from=np.full(lanes, fill, np.uint32))
        nxt, act = np.array([next_seq], np.uint32), np.array([fill], np.uint32)
        P_U32 = ctypes.POINTER(ctypes.c_uint32)
        ptr = lambda a: a.ctypes.data_as(P_U32)  # noqa: E731
        if not self.library.rwkv_mi355x_selftest_gen_turnover(
                lanes, Q, step, ptr(out['lane_seq']), ptr(out['done']), ptr(length), ptr(max_tokens), ptr(out['lane']),
                ptr(out['start']), ptr(nxt), ptr(act), ptr(out['retire_to']), ptr(out['admit_from'])):
            raise ValueError('rwkv_mi355x_selftest_gen_turnover failed')
        out.update(next=int(nxt[0]), active=int(act[0]))
        return out

    def rwkv_mi355x_prefill_batch(self, ctx: RWKVContext, prompts, slots, cont=None) -> None:
        """Evaluates the prompts (token lists, none empty) together in packed sequence passes; prompt i
        lands in slots[i] as reset / rwkv_mi355x_eval_device / rwkv_mi355x_batch_store would leave it,
        bit for bit.  cont: None, or one flag per prompt -- true continues from the slot's state."""
        rows = len(prompts)
        if len(slots) != rows or (cont is not None and len(cont) != rows):
            raise ValueError('one slot (and one cont flag) per prompt')
        flat = [int(t) for p in prompts for t in p]
        tokens = (ctypes.c_uint32 * max(1, len(flat)))(*flat)
        lengths = (ctypes.c_size_t * max(1, rows))(*[len(p) for p in prompts])
        slot_arr = (ctypes.c_uint32 * max(1, rows))(*[int(s) for s in slots])
        cont_arr = None if cont is None else (ctypes.c_uint8 * max(1, rows))(*[1 if c else 0 for c in cont])
        if not self.library.rwkv_mi355x_prefill_batch(ctx.ptr, rows, slot_arr, tokens, lengths, cont_arr):
            raise ValueError('rwkv_mi355x_prefill_batch failed, check stderr')

    def rwkv_mi355x_selftest_prefill_plan(self, lengths, cap: int, max_segs: Optional[int] = None):
        """The host planner of rwkv_mi355x_prefill_batch (no GPU).  Returns (count, rows, begins, lens,
        chunks): count as the library returns it (negative: max_segs too small, or bad arguments) and
        the four uint32 arrays of max_segs entries, entries past count untouched (0xFFFFFFFF)."""
        import numpy as np
        n = len(lengths)
        if max_segs is None:
            max_segs = n + sum(lengths) // max(1, cap) + 1
        arrs = [np.full(max_segs, 0xFFFFFFFF, np.uint32) for _ in range(4)]
        larr = (ctypes.c_size_t * max(1, n))(*[int(x) for x in lengths])
        count = self.library.rwkv_mi355x_selftest_prefill_plan(
            larr, n, cap, *[a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) for a in arrs], max_segs)
        return (int(count), *arrs)

    def rwkv_mi355x_selftest_sample_rows(self, logits, u, temperature, top_p, presence=None, frequency=None,
                                         counts=None, done=None, logit_bias=None, stop_tokens=(), step: int = 0,
                                         fill: int = 0xFFFFFFFF, active: Optional[int] = None,
                                         logprobs: Optional[int] = None, lp_fill: int = 0xA5):
        """The batched sampler kernel on host logits [rows][V] with the draws u [rows] given and
        per-row parameters (scalars or [rows]).  counts (uint32 [rows][V]) and done (uint32 [rows]) are
        updated in place when given.  Every output starts as `fill` (cutoff: its bits), so an entry
        the kernel does not write keeps it.  Returns a dict: tokens, decode_tokens, kept, cutoff,
        lengths, done [rows] and active (the live rows, starting from `active`, default rows).
        logprobs=K (rwkv_mi355x_selftest_sample_rows_logprobs) adds 'logprobs': Logprobs of [rows] /
        [rows, K] arrays that start as bytes of `lp_fill`."""
        import numpy as np
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        rows, V = logits.shape
        u = np.ascontiguousarray(np.broadcast_to(np.asarray(u, dtype=np.float32), (rows,)))
        p = make_batch_sampling(rows, temperature, top_p, presence, frequency, logit_bias, stop_tokens=stop_tokens)
        if counts is not None:
            assert counts.dtype == np.uint32 and counts.shape == (rows, V) and counts.flags['C_CONTIGUOUS']
        if done is None:
            done = np.zeros(rows, np.uint32)
        assert done.dtype == np.uint32 and done.shape == (rows,)
        out = {k: np.full(rows, fill, np.uint32) for k in ('tokens', 'decode_tokens', 'kept', 'cutoff', 'lengths')}
        act = np.array([rows if active is None else active], np.uint32)
        P_U32 = ctypes.POINTER(ctypes.c_uint32)
        args = (logits.ctypes.data_as(P_FLOAT), rows, V, ctypes.byref(p), u.ctypes.data_as(P_FLOAT), step,
                counts.ctypes.data_as(P_U32) if counts is not None else None, done.ctypes.data_as(P_U32),
                out['tokens'].ctypes.data_as(P_U32), out['decode_tokens'].ctypes.data_as(P_U32),
                out['kept'].ctypes.data_as(P_U32), out['cutoff'].ctypes.data_as(P_FLOAT),
                out['lengths'].ctypes.data_as(P_U32), act.ctypes.data_as(P_U32))
        if logprobs is None:
            if not self.library.rwkv_mi355x_selftest_sample_rows(*args):
                raise ValueError('rwkv_mi355x_selftest_sample_rows failed')
        else:
            lp = self._selftest_logprobs(rows, logprobs, lp_fill)
            if not self.library.rwkv_mi355x_selftest_sample_rows_logprobs(*args, *lp[0]):
                raise ValueError('rwkv_mi355x_selftest_sample_rows_logprobs failed')
            out['logprobs'] = lp[1]
        out['cutoff'] = out['cutoff'].view(np.float32)
        out['done'] = done
        out['active'] = int(act[0])
        return out

    # ---- additive: scoring a sequence on the device ------------------------------------------
    def rwkv_mi355x_score_sequence(self, ctx: RWKVContext, tokens, targets=None, want_logits: bool = False):
        """Evaluates the tokens on the device-resident state with the head on every token.  Returns
        (losses float64 [T] or None without targets, argmax uint32 [T], logits float32 [T, n_vocab] or
        None): losses[t] = -log softmax(logits[t])[targets[t]]."""
        import numpy as np
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        T = int(tokens.size)
        P_U32, P_DOUBLE = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
        losses = None
        if targets is not None:
            targets = np.ascontiguousarray(targets, dtype=np.uint32)
            if targets.shape != tokens.shape:
                raise ValueError(f'{targets.size} targets for {T} tokens')
            losses = np.zeros(T, np.float64)
        argmax = np.zeros(T, np.uint32)
        logits = np.zeros((T, self.rwkv_get_n_vocab(ctx)), np.float32) if want_logits else None
        if not self.library.rwkv_mi355x_score_sequence(
                ctx.ptr, tokens.ctypes.data_as(P_U32), T,
                targets.ctypes.data_as(P_U32) if targets is not None else None,
                losses.ctypes.data_as(P_DOUBLE) if losses is not None else None,
                argmax.ctypes.data_as(P_U32), logits.ctypes.data_as(P_FLOAT) if want_logits else None):
            raise ValueError('rwkv_mi355x_score_sequence failed, check stderr')
        return losses, argmax, logits

    def rwkv_mi355x_selftest_xent(self, logits, targets):
        """The scoring kernel on host logits [rows][V] (float32 numpy) and targets [rows].  Returns
        (losses float64 [rows], argmax uint32 [rows])."""
        import numpy as np
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        rows, V = logits.shape
        targets = np.ascontiguousarray(targets, dtype=np.uint32)
        assert targets.shape == (rows,)
        losses, argmax = np.zeros(rows, np.float64), np.zeros(rows, np.uint32)
        P_U32 = ctypes.POINTER(ctypes.c_uint32)
        if not self.library.rwkv_mi355x_selftest_xent(
                logits.ctypes.data_as(P_FLOAT), rows, V, targets.ctypes.data_as(P_U32),
                losses.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), argmax.ctypes.data_as(P_U32)):
            raise ValueError('rwkv_mi355x_selftest_xent failed')
        return losses, argmax

    def rwkv_mi355x_selftest_wkv_layouts(self, kind: int, H: int, S: int, lens, seed: int):
        """The serial WKV kernels' token layouts against each other on seeded operands (kind 4, 5, 6, 7;
        segment lengths lens).  Returns a dict of word counts: y_seg / state_seg (one launch per
        segment vs the segmented launch), y_ctx / state_ctx (vs the contexts form; kind 4, all
        lengths 1) and compared_seg / compared_ctx (0: that form did not run)."""
        arr = (ctypes.c_uint32 * len(lens))(*lens)
        out = (ctypes.c_uint64 * 6)()
        if not self.library.rwkv_mi355x_selftest_wkv_layouts(kind, H, S, arr, len(lens), seed, out):
            raise ValueError('rwkv_mi355x_selftest_wkv_layouts failed')
        return dict(zip(('y_seg', 'state_seg', 'y_ctx', 'state_ctx', 'compared_seg', 'compared_ctx'), map(int, out)))

    def rwkv_get_system_info_string(self) -> str:
        return self.library.rwkv_get_system_info_string().decode('utf-8')


def load_rwkv_shared_library() -> RWKVSharedLibrary:
    """Finds librwkv.so: $RWKV_CPP_SHARED_LIBRARY, then <repo>/{bin,build,...}/librwkv.so
    relative to the working directory and to this file (reference search order,
    rwkv_cpp_shared_library.py:375-426), plus rwkv.cppy_amd/build/."""
    env = os.environ.get('RWKV_CPP_SHARED_LIBRARY')
    if env and os.path.isfile(env):
        return RWKVSharedLibrary(env)
    file_name = 'librwkv.so'
    children = [
        lambda p: p / 'bin' / 'Release' / file_name,
        lambda p: p / 'bin' / file_name,
        lambda p: p / 'build' / 'bin' / 'Release' / file_name,
        lambda p: p / 'build' / 'bin' / file_name,
        lambda p: p / 'build' / file_name,
        lambda p: p / file_name,
    ]
    here = pathlib.Path(os.path.abspath(__file__)).parent
    cwd = pathlib.Path(os.path.abspath(os.getcwd()))
    parents = [cwd.parent.parent, cwd.parent, cwd, here.parent.parent, here.parent.parent / 'rwkv.cppy_amd']
    for parent in parents:
        for child in children:
            full = child(parent)
            if os.path.isfile(full):
                return RWKVSharedLibrary(str(full))
    raise ValueError(f'Failed to find {file_name} automatically; '
                     f'you need to find the library and create RWKVSharedLibrary specifying the path to it')
