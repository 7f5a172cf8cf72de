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


def beam_step(logits, scores, finished, stop_tokens=()):
    """One step of librwkv.so's beam search (rwkv_mi355x_generate_beam) in float64 numpy; the
    specification the device kernels are measured against.

    logits float32 [W, V]; scores float64 [W]; finished [W]: 0 a live beam, 1 a finished one, 2 an empty
    one (beams 1 .. W-1 before step 0), which has no candidate.
      live beam b:      logZ_b = logprobs(logits[b], 0)[0]; candidate (b, v) scores
                        scores[b] + (float64(logits[b, v]) - logZ_b); a NaN element is no candidate
      finished beam b:  one candidate, (b, v = 0), with scores[b] unchanged
    The new beams are the W first candidates in the order: larger score first (float64, compared
    exactly), then lower b, then lower v.  New beam j continues beam parent[j] and appends token[j]
    (0xFFFFFFFF for a beam that was finished already); it is finished when it was, or when its token is
    one of stop_tokens.  A new beam that no candidate reaches (NaN rows only) is empty.
    Returns (parent uint32 [W], token uint32 [W], score float64 [W], finished uint32 [W], gap): gap is
    the smallest nonzero score difference between neighbours among the first W + 1 candidates (inf
    without one): the W-th against the (W+1)-th, and the selected ones against each other.  Where it
    exceeds the error of the device's logZ, the device selects exactly these beams in this order
    (equal scores are exact ties on both sides: equal logits under one logZ word)."""
    l32 = np.asarray(logits, dtype=np.float32)
    W, V = l32.shape
    scores = np.asarray(scores, dtype=np.float64)
    stop = {int(t) for t in stop_tokens}
    cands = []  # (-score, b, v): only the rows' W best can be among the W best of all
    for b in range(W):
        if int(finished[b]) == 1:
            cands.append((-float(scores[b]), b, 0))
        elif int(finished[b]) == 0:
            log_z, ids, lp = logprobs(l32[b], min(W + 1, V))
            cands += [(-float(scores[b] + x), b, int(v)) for v, x in zip(ids, lp)]
    cands.sort()
    parent, token = np.arange(W, dtype=np.uint32), np.full(W, 0xFFFFFFFF, np.uint32)
    score, fin = np.full(W, -np.inf), np.full(W, 2, np.uint32)
    for j, (s, b, v) in enumerate(cands[:W]):
        was = int(finished[b]) == 1
        parent[j], score[j] = b, -s
        token[j] = 0xFFFFFFFF if was else v
        fin[j] = 1 if was or v in stop else 0
    with np.errstate(all='ignore'):
        steps = np.diff([c[0] for c in cands[:W + 1]])
    gap = steps[steps > 0].min() if (steps > 0).any() else np.inf
    return parent, token, score, fin, float(gap)


def beam_rank(scores, lengths, length_penalty: float = 0.0):
    """The order in which rwkv_mi355x_generate_beam returns its beams: score / max(len, 1) **
    length_penalty descending, ties to the lower working row.  Returns the working rows, best first."""
    key = np.asarray(scores, np.float64) / np.maximum(np.asarray(lengths, np.float64), 1.0) ** float(length_penalty)
    return np.argsort(-key, kind='stable')


def _cutoff(key, mass, target: float) -> float:
    """The first key, in ascending order, at which the mass of all elements with a key <= it exceeds
    target (ties are one step)."""
    order = np.argsort(key, kind='stable')
    k, cum = key[order], np.cumsum(mass[order])
    step_end = np.append(k[1:] != k[:-1], True)
    return float(k[np.argmax((cum > target) & step_end)])


def kept_mask(l, top_k: int = 0, min_p: float = 0.0, typical_p: float = 0.0, top_p: float = 0.0) -> np.ndarray:
    """The tokens librwkv.so's sampler keeps for one draw (rwkv_mi355x_filters, then top_p), in float64
    numpy; the specification the device kernels are measured against.

    l is the float32 row the sampler samples from (logits, penalize(), bias).  With m = max l and
    e = exp(l - m), in this order and every rule keeping all ties at its cutoff:
      top_k      keep e >= the top_k-th largest e                       (0 or >= len(l): off)
      min_p      among those, keep e >= min_p, i.e. p >= min_p * p_max  (0: off)
      typical_p  over the set F kept so far: g = sum_F e (m - l) / sum_F e, d = |(m - l) - g|; keep
                 d <= d_c, the smallest d with sum{e in F, d <= d_c} > typical_p * sum_F e  (0, 1: off)
      top_p      over the set G kept so far: keep e >= e_c, the largest e with
                 sum{e in G, e >= e_c} > top_p * sum_G e                 (0, 1: off)
    Returns a bool array.  The device forms e in float32 and d as one float32 rounding of a float64
    value, and sums the masses in float32: where a cutoff falls between two tie groups whose masses (and,
    for typical_p, distances) differ by more than those errors, it keeps exactly this set."""
    ld = np.asarray(l, dtype=np.float32).astype(np.float64)
    if ld.ndim != 1 or ld.size == 0:
        raise ValueError('one row of logits')
    if not 0.0 <= min_p <= 1.0 or not 0.0 <= typical_p <= 1.0 or not 0.0 <= top_p <= 1.0:
        raise ValueError('min_p, typical_p and top_p are in [0, 1]')
    x = ld.max() - ld
    e = np.exp(-x)
    keep = np.ones(ld.size, bool)
    if 0 < top_k < ld.size:
        keep &= e >= np.sort(e)[-int(top_k)]
    if min_p > 0.0:
        keep &= e >= float(np.float32(min_p))
    if 0.0 < typical_p < 1.0:
        f = np.flatnonzero(keep)
        total = e[f].sum()
        d = np.abs(x - (e[f] * x[f]).sum() / total)
        keep &= d <= _cutoff(d[f], e[f], typical_p * total)
    if 0.0 < top_p < 1.0:
        g = np.flatnonzero(keep)
        keep &= -e <= _cutoff(-e[g], e[g], top_p * e[g].sum())
    return keep


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


def ngram_draft(corpus, k: int, ngram_min: int, ngram_max: int):
    """The draft rule of rwkv_mi355x_generate_speculative over a token corpus of length L (history, the
    emitted tokens and the step's drawn token): for g = ngram_max down to ngram_min with g < L, the
    largest p < L - g with corpus[p:p + g] == corpus[L - g:]; the first g that matches gives
    corpus[p + g:min(p + g + k, L)], a list (the match may overlap the end); no match: []."""
    c = np.asarray(corpus, dtype=np.int64)
    L = len(c)
    for g in range(ngram_max, ngram_min - 1, -1):
        if g >= L:
            continue
        hit = np.ones(L - g, dtype=bool)  # hit[p]: a match at p
        for i in range(g):
            hit &= c[i:L - g + i] == c[L - g + i]
        at = np.flatnonzero(hit)
        if at.size:
            p = int(at[-1])
            return [int(t) for t in c[p + g:min(p + g + k, L)]]
    return []
