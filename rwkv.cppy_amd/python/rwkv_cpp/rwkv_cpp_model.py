"""RWKVModel over librwkv.so (MI355X build).

Same constructor, properties, eval / eval_sequence / eval_sequence_in_chunks / free
methods, buffer validation and return convention as the reference's
python/rwkv_cpp/rwkv_cpp_model.py:22-364: buffers are float32, contiguous, on the CPU,
shape (state_len,) / (n_vocab,); missing outputs are allocated (numpy or torch, by the
type of the inputs given); returns (logits, state).
"""
import multiprocessing
import os
from typing import List, Optional, Tuple, Any

try:
    from . import rwkv_cpp_shared_library
except ImportError:  # imported as a top-level module
    import rwkv_cpp_shared_library

Tensor = Any  # numpy.ndarray or torch.Tensor


def _is_torch(t) -> bool:
    return type(t).__module__.startswith('torch')


class RWKVModel:
    def __init__(self, shared_library: 'rwkv_cpp_shared_library.RWKVSharedLibrary', model_path: str,
                 thread_count: int = max(1, multiprocessing.cpu_count() // 2), gpu_layer_count: int = 0,
                 **kwargs) -> None:
        if 'gpu_layers_count' in kwargs:
            gpu_layer_count = kwargs['gpu_layers_count']
        if not os.path.isfile(model_path):
            raise ValueError(f'{model_path} is not a file')
        if not thread_count > 0:
            raise ValueError('Thread count must be > 0')
        if not gpu_layer_count >= 0:
            raise ValueError('GPU layer count must be >= 0')
        self._library = shared_library
        self._ctx = self._library.rwkv_init_from_file(model_path, thread_count, gpu_layer_count)
        self._state_buffer_element_count = self._library.rwkv_get_state_buffer_element_count(self._ctx)
        self._logits_buffer_element_count = self._library.rwkv_get_logits_buffer_element_count(self._ctx)
        self._valid = True

    @property
    def n_vocab(self) -> int:
        return self._library.rwkv_get_n_vocab(self._ctx)

    @property
    def n_embed(self) -> int:
        return self._library.rwkv_get_n_embed(self._ctx)

    @property
    def n_layer(self) -> int:
        return self._library.rwkv_get_n_layer(self._ctx)

    # ---- buffer handling --------------------------------------------------------------
    def _prepare(self, state_in, state_out, logits_out, use_numpy):
        if not self._valid:
            raise ValueError('Model was freed')
        for t in (state_in, state_out, logits_out):
            if t is not None:
                use_numpy = not _is_torch(t)
                break
        if state_in is not None:
            self._validate(state_in, 'state_in', self._state_buffer_element_count)
            state_in_ptr = self._ptr(state_in)
        else:
            state_in_ptr = 0
        if state_out is not None:
            self._validate(state_out, 'state_out', self._state_buffer_element_count)
        else:
            state_out = self._zeros(self._state_buffer_element_count, use_numpy)
        if logits_out is not None:
            self._validate(logits_out, 'logits_out', self._logits_buffer_element_count)
        else:
            logits_out = self._zeros(self._logits_buffer_element_count, use_numpy)
        return state_in_ptr, state_out, logits_out

    @staticmethod
    def _validate(t, name: str, size: int) -> None:
        if _is_torch(t):
            import torch
            if t.device != torch.device('cpu'):
                raise ValueError(f'{name} is not on CPU')
            if t.dtype != torch.float32:
                raise ValueError(f'{name} is not of type float32')
            if tuple(t.shape) != (size,):
                raise ValueError(f'{name} has invalid shape {tuple(t.shape)}, expected ({size})')
            if not t.is_contiguous():
                raise ValueError(f'{name} is not contiguous')
        else:
            import numpy as np
            if t.dtype != np.float32:
                raise ValueError(f'{name} is not of type float32')
            if t.shape != (size,):
                raise ValueError(f'{name} has invalid shape {t.shape}, expected ({size})')
            if not t.flags['C_CONTIGUOUS']:
                raise ValueError(f'{name} is not contiguous')

    @staticmethod
    def _ptr(t) -> int:
        return t.data_ptr() if _is_torch(t) else t.ctypes.data

    @staticmethod
    def _zeros(n: int, use_numpy: bool):
        if use_numpy:
            import numpy as np
            return np.zeros(n, dtype=np.float32)
        import torch
        return torch.zeros(n, dtype=torch.float32, device='cpu')

    # ---- evaluation -------------------------------------------------------------------
    def eval(self, token: int, state_in: Optional[Tensor], state_out: Optional[Tensor] = None,
             logits_out: Optional[Tensor] = None, use_numpy: bool = False) -> Tuple[Tensor, Tensor]:
        sin, state_out, logits_out = self._prepare(state_in, state_out, logits_out, use_numpy)
        self._library.rwkv_eval(self._ctx, token, sin, self._ptr(state_out), self._ptr(logits_out))
        return logits_out, state_out

    def eval_sequence(self, tokens: List[int], state_in: Optional[Tensor], state_out: Optional[Tensor] = None,
                      logits_out: Optional[Tensor] = None, use_numpy: bool = False) -> Tuple[Tensor, Tensor]:
        sin, state_out, logits_out = self._prepare(state_in, state_out, logits_out, use_numpy)
        self._library.rwkv_eval_sequence(self._ctx, tokens, sin, self._ptr(state_out), self._ptr(logits_out))
        return logits_out, state_out

    def eval_sequence_in_chunks(self, tokens: List[int], state_in: Optional[Tensor], state_out: Optional[Tensor] = None,
                                logits_out: Optional[Tensor] = None, chunk_size: int = 16,
                                use_numpy: bool = False) -> Tuple[Tensor, Tensor]:
        sin, state_out, logits_out = self._prepare(state_in, state_out, logits_out, use_numpy)
        self._library.rwkv_eval_sequence_in_chunks(self._ctx, tokens, chunk_size, sin, self._ptr(state_out),
                                                   self._ptr(logits_out))
        return logits_out, state_out

    def eval_batch(self, tokens: List[int], states_in=None):
        """MI355X extension (rwkv_mi355x_eval_batch): len(tokens) independent contexts advance one token
        each in one pass over the weights.  states_in: float32 [n, state_len] numpy array, or None for
        fresh states.  Returns (logits [n, n_vocab], states [n, state_len]); row i equals
        eval(tokens[i], states_in[i]) bit for bit."""
        import numpy as np
        if not self._valid:
            raise ValueError('Model was freed')
        n = len(tokens)
        if states_in is not None:
            states_in = np.ascontiguousarray(states_in, dtype=np.float32)
            if states_in.shape != (n, self._state_buffer_element_count):
                raise ValueError(f'states_in must be [{n}, {self._state_buffer_element_count}]')
        states = np.zeros((n, self._state_buffer_element_count), np.float32)
        logits = np.zeros((n, self._logits_buffer_element_count), np.float32)
        self._library.rwkv_mi355x_eval_batch(self._ctx, list(tokens), None if states_in is None else states_in.ctypes.data,
                                             states.ctypes.data, logits.ctypes.data)
        return logits, states

    def sample(self, temperature: float = 1.0, top_p: float = 0.8, logit_bias=None, seed: int = 0,
               offset: int = 0, logprobs: Optional[int] = None):
        """MI355X extension (rwkv_mi355x_sample): draws one token on the device from the logits of the
        last evaluation on this model (sampling.sample_logits semantics; draw `offset` of the stream
        `seed`, sampling.uniform).  The state is untouched.

        logprobs=K (0 <= K <= 20): returns (token, Logprobs(token_logprob, top_ids, top_logprobs)), the
        token's log-probability under softmax(logits + bias) and the K most likely tokens with theirs
        (sampling.logprobs), taken on the device inside the sampling step."""
        if not self._valid:
            raise ValueError('Model was freed')
        if logprobs is None:
            return self._library.rwkv_mi355x_sample(self._ctx, temperature, top_p, logit_bias, seed, offset)
        return self._library.rwkv_mi355x_sample(self._ctx, temperature, top_p, logit_bias, seed, offset, logprobs=logprobs)

    def generate(self, n: int, temperature: float = 1.0, top_p: float = 0.8, logit_bias=None, seed: int = 0,
                 offset: int = 0, stop_tokens=(), block: int = 16, logprobs: Optional[int] = None):
        """MI355X extension (rwkv_mi355x_generate): generates up to n tokens on the device, continuing
        from the state and logits the last evaluation on this model left there (eval, eval_sequence, or
        an earlier generate).  Sampling and decoding run back to back on the GPU in blocks of `block`
        tokens; only the tokens come back.  Draw i uses sampling.uniform(seed, offset + i).

        Generation stops after a block that contains one of stop_tokens, and the tokens up to and
        including the first stop token are returned.  The device state has then consumed the whole
        block: it may have run up to block - 1 tokens past the stop token.  block=1 stops exactly.

        logprobs=K (0 <= K <= 20): returns (tokens, Logprobs) with one entry per returned token, cut
        where the tokens are cut: token_logprob float64 [len], top_ids uint32 and top_logprobs float64
        [len, K] (sampling.logprobs of every draw, taken on the device)."""
        if not self._valid:
            raise ValueError('Model was freed')
        if not block > 0:
            raise ValueError('block must be > 0')
        stop = set(stop_tokens)
        out: List[int] = []
        parts = []

        def result(tokens, last):
            if logprobs is None:
                return tokens
            import numpy as np
            # an empty block in front, so that n == 0 gives empty arrays of the right shapes
            empty = rwkv_cpp_shared_library.make_logprobs(1, 1, logprobs)[1]
            kept = [[x[0, :0] for x in empty]] + parts + ([last] if last is not None else [])
            return tokens, rwkv_cpp_shared_library.Logprobs(*(np.concatenate(x) for x in zip(*kept)))

        while len(out) < n:
            m = min(block, n - len(out))
            lp = None
            if logprobs is None:  # the call as it always was
                tokens = self._library.rwkv_mi355x_generate(self._ctx, m, temperature, top_p, logit_bias, seed,
                                                            offset + len(out))
            else:
                tokens, lp = self._library.rwkv_mi355x_generate(self._ctx, m, temperature, top_p, logit_bias, seed,
                                                                offset + len(out), logprobs=logprobs)
            for i, t in enumerate(tokens):
                if t in stop:
                    cut = None if lp is None else rwkv_cpp_shared_library.Logprobs(*(x[:i + 1] for x in lp))
                    return result(out + tokens[:i + 1], cut)
            out += tokens
            if lp is not None:
                parts.append(lp)
        return result(out, None)

    # ---- batched generation (rwkv_mi355x_generate_batch) --------------------------------------
    def batch_reserve(self, n_slots: int) -> None:
        """MI355X extension: gives the model n_slots <= 256 generation slots (0 frees them).  Every
        slot is empty afterwards."""
        if not self._valid:
            raise ValueError('Model was freed')
        self._library.rwkv_mi355x_batch_reserve(self._ctx, n_slots)

    def batch_store(self, slot: int) -> None:
        """MI355X extension: the device state and logits of the last evaluation on this model go into
        the slot, on the device.  The slot starts a new sequence (no token counted, not finished)."""
        if not self._valid:
            raise ValueError('Model was freed')
        self._library.rwkv_mi355x_batch_store(self._ctx, slot)

    def batch_load(self, slot: int) -> None:
        """MI355X extension: the model continues from the slot's state and logits; score, sample and
        generate go on from there."""
        if not self._valid:
            raise ValueError('Model was freed')
        self._library.rwkv_mi355x_batch_load(self._ctx, slot)

    def prefill_batch(self, prompts: List[List[int]], slots=None, cont=False) -> None:
        """MI355X extension (rwkv_mi355x_prefill_batch): evaluates the prompts together, packed into
        sequence passes of up to 1024 tokens, so the weights are read once per pass instead of once per
        prompt.  Prompt i lands in slots[i] (None: slot i; slots are reserved when there are too few)
        exactly as reset_state / eval / batch_store would leave it.  cont: a bool or one per prompt;
        true continues from the slot's state instead of a fresh one.  The model's own state and logits
        are untouched."""
        if not self._valid:
            raise ValueError('Model was freed')
        rows = len(prompts)
        if not 0 < rows <= 256:
            raise ValueError(f'{rows} prompts (1 to 256)')
        if any(len(p) == 0 for p in prompts):
            raise ValueError('empty prompt')
        slots = list(range(rows)) if slots is None else [int(s) for s in slots]
        if len(slots) != rows:
            raise ValueError(f'{len(slots)} slots for {rows} prompts')
        if len(set(slots)) != rows or any(not 0 <= s < 256 for s in slots):
            raise ValueError('slots must be distinct and in [0, 256)')
        cont = [bool(cont)] * rows if isinstance(cont, (bool, int)) else [bool(c) for c in cont]
        if len(cont) != rows:
            raise ValueError(f'{len(cont)} cont flags for {rows} prompts')
        need = max(slots) + 1
        if self._library.rwkv_mi355x_batch_slots(self._ctx) < need:
            if any(cont):
                raise ValueError(f'slot {need - 1} is not reserved: nothing to continue from')
            self._library.rwkv_mi355x_batch_reserve(self._ctx, need)
        self._library.rwkv_mi355x_prefill_batch(self._ctx, [list(p) for p in prompts], slots, cont)

    def generate_batch(self, prompts: List[List[int]], n: int, temperature=1.0, top_p=0.8, presence_penalty=0.0,
                       frequency_penalty=0.0, logit_bias=None, seeds=None, stop_tokens=(),
                       check_every: int = 16, batched_prefill: bool = False, logprobs: Optional[int] = None):
        """MI355X extension (rwkv_mi355x_generate_batch): generates up to n tokens for every prompt, all
        rows together on the device: sampling, penalties over the tokens a row has drawn, exact stops
        and one batched decode step per token, with only the tokens coming back.  temperature, top_p,
        the penalties and seeds are scalars or one value per prompt (seeds None: row r uses seed r);
        logit_bias and stop_tokens are shared.  Each prompt is evaluated from a fresh state on the
        device and stored into slot i (slots are reserved as needed); batched_prefill evaluates the
        prompts together (prefill_batch) instead of one after the other, with the same bits.  Returns one token list per
        prompt; a list that ends early ends with a stop token, which is not evaluated: slot i then
        holds the state before it, and batch_load(i) continues from there.

        logprobs=K (0 <= K <= 20): returns (token lists, [Logprobs per prompt]); prompt i's Logprobs
        has one entry per token of its list, the stop token included: token_logprob float64 [len],
        top_ids uint32 and top_logprobs float64 [len, K], of the penalised and biased distribution each
        token was drawn from (sampling.logprobs)."""
        if not self._valid:
            raise ValueError('Model was freed')
        rows = len(prompts)
        if not 0 < rows <= 256:
            raise ValueError(f'{rows} prompts (1 to 256)')
        if not n > 0:
            raise ValueError('n must be > 0')
        if any(len(p) == 0 for p in prompts):
            raise ValueError('empty prompt')
        params = rwkv_cpp_shared_library.make_batch_sampling(
            rows, temperature, top_p, presence_penalty, frequency_penalty, logit_bias, seeds, 0, stop_tokens,
            False, check_every)
        if self._library.rwkv_mi355x_batch_slots(self._ctx) < rows:
            self._library.rwkv_mi355x_batch_reserve(self._ctx, rows)
        if batched_prefill:
            self._library.rwkv_mi355x_prefill_batch(self._ctx, [list(p) for p in prompts], list(range(rows)), None)
        for slot, prompt in ([] if batched_prefill else enumerate(prompts)):
            self.reset_state()
            self._library.rwkv_mi355x_eval_device(self._ctx, list(prompt))
            self._library.rwkv_mi355x_batch_store(self._ctx, slot)
        if logprobs is None:  # the call as it always was
            out = self._library.rwkv_mi355x_generate_batch(self._ctx, rows, n, params)
        else:
            out = self._library.rwkv_mi355x_generate_batch(self._ctx, rows, n, params, logprobs=logprobs)
        tokens, lengths = out[0], out[1]
        lists = [[int(t) for t in tokens[r][:int(lengths[r])]] for r in range(rows)]
        if logprobs is None:
            return lists
        return lists, [rwkv_cpp_shared_library.Logprobs(*(x[r, :int(lengths[r])] for x in out[3])) for r in range(rows)]

    def generate_queue(self, prompts: List[List[int]], max_tokens, lanes: int = 32, temperature=1.0, top_p=0.8,
                       presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, seeds=None, stop_tokens=(),
                       check_every: int = 16, logprobs: Optional[int] = None):
        """MI355X extension (rwkv_mi355x_generate_queue): continuous batching.  Up to 256 prompts are
        evaluated together (prefill_batch) into slots 0 .. Q-1 and generated through a queue over
        `lanes` decode rows: a row whose sequence has ended -- a stop token, or its max_tokens (a scalar
        or one value per prompt) -- takes the next waiting prompt between two decode steps, so the rows
        stay full.  The other parameters are those of generate_batch, per prompt.  Returns one token
        list per prompt, each exactly what that prompt generates alone; slot i holds its final state
        and logits, and batch_load(i) continues from there.  logprobs=K: as generate_batch, (token
        lists, [Logprobs per prompt])."""
        if not self._valid:
            raise ValueError('Model was freed')
        rows = len(prompts)
        if not 0 < rows <= 256:
            raise ValueError(f'{rows} prompts (1 to 256)')
        if any(len(p) == 0 for p in prompts):
            raise ValueError('empty prompt')
        if not 0 < lanes <= 256:
            raise ValueError(f'{lanes} lanes (1 to 256)')
        caps = [int(c) for c in rwkv_cpp_shared_library._per_row(max_tokens, rows, 'max_tokens')]
        if any(not 0 < c <= 65536 for c in caps):
            raise ValueError('max_tokens must be in [1, 65536]')
        # the per-prompt parameters are checked before anything reaches the device
        rwkv_cpp_shared_library.make_batch_sampling(rows, temperature, top_p, presence_penalty, frequency_penalty,
                                                    logit_bias, seeds, 0, stop_tokens, False, check_every)
        if self._library.rwkv_mi355x_batch_slots(self._ctx) < rows:
            self._library.rwkv_mi355x_batch_reserve(self._ctx, rows)
        self._library.rwkv_mi355x_prefill_batch(self._ctx, [list(p) for p in prompts], list(range(rows)), None)
        extra = {} if logprobs is None else {'logprobs': logprobs}
        out = self._library.rwkv_mi355x_generate_queue(
            self._ctx, caps, lanes, temperature, top_p, presence_penalty, frequency_penalty, logit_bias, seeds, 0,
            stop_tokens, check_every, **extra)
        lists = [[int(t) for t in out['tokens'][r][:int(out['lengths'][r])]] for r in range(rows)]
        if logprobs is None:
            return lists
        return lists, [rwkv_cpp_shared_library.Logprobs(*(x[r, :len(lists[r])] for x in out['logprobs']))
                       for r in range(rows)]

    def reset_state(self) -> None:
        """MI355X extension (rwkv_mi355x_state_upload with NULL): the device-resident state becomes the
        fresh state, as before the first token."""
        if not self._valid:
            raise ValueError('Model was freed')
        if not self._library.library.rwkv_mi355x_state_upload(self._ctx.ptr, None):
            raise ValueError('rwkv_mi355x_state_upload failed, check stderr')

    def score(self, tokens: List[int], targets: Optional[List[int]] = None, want_logits: bool = False):
        """MI355X extension (rwkv_mi355x_score_sequence): evaluates the tokens on the device-resident
        state (continuing from wherever the last evaluation on this model left it) with the head on
        every token.  Returns (losses, argmax, logits): losses float64 [T], the cross-entropy of
        targets[t] under the logits following tokens[t] (None without targets); argmax uint32 [T];
        logits float32 [T, n_vocab] when want_logits, else None.  Only the losses and argmaxes cross
        PCIe unless the logits are asked for.  sample / generate continue from the last token."""
        if not self._valid:
            raise ValueError('Model was freed')
        return self._library.rwkv_mi355x_score_sequence(self._ctx, tokens, targets, want_logits)

    def free(self) -> None:
        if not self._valid:
            raise ValueError('Already freed')
        self._valid = False
        self._library.rwkv_free(self._ctx)

    def __del__(self) -> None:
        if getattr(self, '_valid', False):
            self.free()
