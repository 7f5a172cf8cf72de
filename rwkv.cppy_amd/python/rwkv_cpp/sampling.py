"""Token sampling over the logits rwkv_eval returns: the semantics of the reference's
python/sampling.py:6-52 (softmax, logit bias, greedy at temperature 0, top-p cutoff, temperature),
numpy only.  rng: an optional numpy Generator (the reference draws from np.random's global state)."""
from typing import Dict, Optional

import numpy as np


def softmax(x: np.ndarray, axis: int = -1) -> np.ndarray:
    x = x - x.max(axis=axis, keepdims=True)
    e = np.exp(x)
    return e / e.sum(axis=axis, keepdims=True)


def sample_logits(out, temperature: float = 1.0, top_p: float = 0.8, logit_bias: Optional[Dict[int, float]] = None,
                  rng: Optional[np.random.Generator] = None) -> int:
    if hasattr(out, 'detach'):
        out = out.detach().cpu().numpy()
    return sample_probs(softmax(np.asarray(out, dtype=np.float32), axis=-1), temperature, top_p, logit_bias, rng)


def sample_probs(probs: np.ndarray, temperature: float = 1.0, top_p: float = 0.8,
                 logit_bias: Optional[Dict[int, float]] = None, rng: Optional[np.random.Generator] = None) -> int:
    if not 0.0 <= temperature:
        raise ValueError('temperature')
    if not 0.0 <= top_p <= 1.0:
        raise ValueError('top_p')
    probs = np.array(probs, copy=True)
    if top_p == 0.0:
        top_p = 1.0
    if logit_bias:
        logits = np.log(probs)
        ids, values = zip(*logit_bias.items())
        logits[list(ids)] += values
        logits -= logits.max(axis=-1, keepdims=True)
        probs = np.exp(logits) / np.sum(np.exp(logits))
    if temperature == 0.0:
        return int(np.argmax(probs))
    if top_p < 1.0:
        sorted_probs = np.sort(probs)[::-1]
        cumulative = np.cumsum(sorted_probs)
        cutoff = float(sorted_probs[np.argmax(cumulative > top_p)])
        probs[probs < cutoff] = 0
    if temperature != 1.0:
        probs = np.power(probs, 1.0 / temperature)
    probs = probs / np.sum(probs)
    choice = rng.choice if rng is not None else np.random.choice
    return int(choice(a=len(probs), p=probs))


def uniform(seed: int, counter: int) -> float:
    """Draw `counter` of the stream `seed` as librwkv.so's sampler makes it (rwkv_mi355x_sampling):
    splitmix64 of the pair, the top 24 bits as a float32 in [0, 1)."""
    return float(np.float32(splitmix64(seed, counter) >> 40) * np.float32(2.0 ** -24))


def splitmix64(seed: int, counter: int) -> int:
    """The 64-bit word behind uniform(seed, counter)."""
    mask = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (counter + 1)) & mask
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
    return z ^ (z >> 31)


def penalize(logits, counts, presence: float, frequency: float) -> np.ndarray:
    """The presence / frequency penalty of librwkv.so's batched sampler (rwkv_mi355x_generate_batch),
    bit for bit: for every token with counts > 0, in float32 and in this order,
    logits - (presence + float32(counts) * frequency) -- one multiply, one add, one subtract, each
    rounded to float32; tokens never drawn are untouched.  Returns a new float32 array.  (The
    reference's chat loop, chat_with_bot.py:245-274, forms the penalty in double precision: its
    result can differ from this one by one float32 rounding of the logit.)"""
    l = np.array(logits, dtype=np.float32, copy=True)
    c = np.asarray(counts)
    if c.shape != l.shape:
        raise ValueError(f'counts {c.shape} for logits {l.shape}')
    hit = c > 0
    product = np.multiply(c[hit].astype(np.float32), np.float32(frequency), dtype=np.float32)
    penalty = np.add(np.float32(presence), product, dtype=np.float32)
    l[hit] = np.subtract(l[hit], penalty, dtype=np.float32)
    return l


def logprobs(l, top_k: int):
    """The log-probabilities librwkv.so reports for one draw (rwkv_mi355x_logprobs), in float64 numpy;
    the specification the device kernels are measured against.

    l is the float32 row the sampler samples from: the logits, then penalize() with the counts before
    this draw's increment, then the bias.  Temperature and top-p do not enter: this is softmax(l).
      m      = max l, exact in float32 (a NaN never wins)
      S      = sum_i exp(float64(l_i) - float64(m)), exponentials and sum in float64
      logZ   = float64(m) + log(S)
      token_logprob   = float64(l[token]) - logZ         (the caller subtracts: it knows the token)
      top_ids[0 .. K) = the K first indices in the order "larger l first, lower index first among
                        equal l", exact float32 compares; NaN elements are never listed, so fewer
                        than K come back when fewer than K elements are not NaN
      top_logprobs[j] = float64(l[top_ids[j]]) - logZ, with the same logZ: where the drawn token is
                        top_ids[j] the two values are bit-equal.
    Non-finite elements may make the values NaN or infinite.  The device fixes the association of the
    sum (it is a pure function of its inputs); this one is numpy's, and the two differ by at most
    V * 2**-53 relative in S, whatever the association, since every term is non-negative.
    Returns (logZ float64, top_ids uint32 [<= top_k], top_logprobs float64 [<= top_k])."""
    l32 = np.asarray(l, dtype=np.float32)
    if l32.ndim != 1 or not 0 <= top_k <= l32.size:
        raise ValueError('one row of logits and 0 <= top_k <= its length')
    ld = l32.astype(np.float64)
    listed = np.flatnonzero(~np.isnan(l32))
    with np.errstate(all='ignore'):
        m = ld[listed].max() if listed.size else -np.inf
        log_z = m + np.log(np.exp(ld - m).sum())
        top = listed[np.argsort(-l32[listed], kind='stable')][:top_k]
        return float(log_z), top.astype(np.uint32), ld[top] - log_z


def queue_schedule(lengths, lanes: int):
    """The schedule of librwkv.so's queue (rwkv_mi355x_generate_queue) on plain integers: sequence s
    occupies a lane for lengths[s] >= 1 steps.  Before step i the lanes whose sequence has had its
    steps are freed, and the free lanes, in increasing lane order, take the waiting sequences in
    increasing sequence order; at step 0 every lane is free.  Returns (lane, start, steps): the lane
    and the step of every sequence's admission, and the number of steps up to the one after which
    no lane was busy."""
    lengths = [int(x) for x in lengths]
    if lanes < 1 or not lengths or any(x < 1 for x in lengths):
        raise ValueError('lanes >= 1 and at least one length, each >= 1')
    L = min(int(lanes), len(lengths))
    lane, start = [0] * len(lengths), [0] * len(lengths)
    free_at = [0] * L  # the step at whose turnover the lane is free
    nxt, step = 0, 0
    while nxt < len(lengths):
        for r in range(L):
            if free_at[r] <= step and nxt < len(lengths):
                lane[nxt], start[nxt] = r, step
                free_at[r] = step + lengths[nxt]
                nxt += 1
        step += 1
    return lane, start, max(free_at)


def sample_probs_u(probs: np.ndarray, u: float, temperature: float = 1.0, top_p: float = 0.8,
                   logit_bias: Optional[Dict[int, float]] = None) -> int:
    """sample_probs with the uniform draw u in [0, 1) given instead of an rng: the same bias, top-p
    and temperature filtering, then the first index whose cumulative weight exceeds u times the total
    (what np.random.choice does with its draw)."""

    class _Fixed:
        @staticmethod
        def choice(a, p):
            cdf = np.cumsum(p)
            return min(int(cdf.searchsorted(u * cdf[-1], side='right')), a - 1)

    return sample_probs(probs, temperature, top_p, logit_bias, _Fixed)
