/*
 * rwkv_mi355x.h -- ADDITIVE extensions of librwkv.so (nothing in rwkv.h changes).
 *
 * The reference ABI hands the recurrent state over as host float buffers on every call
 * (rwkv_eval.inc:2-22).  For RWKV-v6-1B6 that is 13 MB each way per token, more than the
 * weights' HBM time, so these entry points let a caller keep the state resident in HBM.
 * They are the path bench.py measures as "device-resident"; ABI-level rates are reported
 * beside them.
 */
#ifndef RWKV_MI355X_H
#define RWKV_MI355X_H

#include "rwkv.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Copies a host state into the context's device-resident state (NULL => fresh state). */
RWKV_API bool rwkv_mi355x_state_upload(struct rwkv_context * ctx, const float * state);
/* Copies the device-resident state out to host memory. */
RWKV_API bool rwkv_mi355x_state_download(struct rwkv_context * ctx, float * state);

/* The state of layers [layer_begin, layer_end) only: `slice` holds those layers in the host layout
 * (rwkv_mi355x_layer_state_len(ctx) floats per layer, layer_begin's first), so a pipeline stage or a
 * caller that owns part of the layers moves just its part over PCIe.  Upload with slice == NULL
 * resets those layers to the fresh state.  Layer ranges outside [0, n_layer) fail with
 * RWKV_ERROR_ARGS. */
RWKV_API size_t rwkv_mi355x_layer_state_len(const struct rwkv_context * ctx);
RWKV_API bool rwkv_mi355x_state_upload_layers(struct rwkv_context * ctx, const float * slice, uint32_t layer_begin,
                                              uint32_t layer_end);
RWKV_API bool rwkv_mi355x_state_download_layers(struct rwkv_context * ctx, float * slice, uint32_t layer_begin,
                                                uint32_t layer_end);
/* State bytes this context has moved so far: out[0] host->device, out[1] device->host (the state
 * entry points above and rwkv_eval's host state buffers). */
RWKV_API void rwkv_mi355x_state_io_bytes(const struct rwkv_context * ctx, double out[2]);

/* rwkv_clone_context onto GPU `device` (reference clone semantics, rwkv.h:93-99, rwkv.cpp:123-139:
 * a new context with a fresh state sharing the parent's model).  The model is uploaded once per
 * GPU -- the first clone on a GPU re-reads the parent's file (same layer range), later clones and
 * their parent-device siblings share that copy -- so a server runs one replica per GPU of a node
 * from one process.  device == the parent's GPU is rwkv_clone_context.  A device outside
 * [0, device count) fails with RWKV_ERROR_ARGS (on the parent's error flags) and returns NULL. */
RWKV_API struct rwkv_context * rwkv_mi355x_clone_context_on(struct rwkv_context * ctx, uint32_t n_threads,
                                                            int device);
/* The GPU a context evaluates on (-1 for NULL). */
RWKV_API int rwkv_mi355x_context_device(const struct rwkv_context * ctx);

/* rwkv_eval_sequence semantics on the device-resident state: tokens host array, T >= 1.
 * compute_logits: run the head on the last token (logits stay in HBM); logits_out (host, may be
 * NULL) additionally receives them.  No state crosses PCIe.  sync=false returns after
 * enqueueing (the caller later calls rwkv_mi355x_sync). */
RWKV_API bool rwkv_mi355x_eval_device(struct rwkv_context * ctx, const uint32_t * tokens, size_t T,
                                      bool compute_logits, float * logits_out, bool sync);
RWKV_API bool rwkv_mi355x_sync(struct rwkv_context * ctx);

/* Token sampling on the device (the reference samples on the host from downloaded logits:
 * sampling.py:18-52).  Per draw: l = logits + bias; temperature == 0 returns the lowest index holding
 * the maximum l (np.argmax); otherwise p = softmax(l), the top_p filter keeps every p_i >= c where c
 * is the largest p_i with sum{p >= c} > top_p (ties at the cutoff are all kept; top_p == 0 means 1),
 * w_i = p_i^(1/temperature) for kept i, and the draw returns the smallest index t with
 * sum_{i<=t} w_i > u * sum w, in vocabulary order.  The uniform draw is stateless, so a caller can
 * reproduce it: draw number `counter` of stream `seed` is
 *   z = seed + 0x9E3779B97F4A7C15 * (counter + 1);  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31;  u = (z >> 40) * 2^-24   (mod 2^64).
 * bias_ids / bias_values are host arrays of n_bias <= 256 entries, each id < n_vocab, values added
 * to the logits. */
struct rwkv_mi355x_sampling {
    float temperature, top_p;            /* reference defaults: 1.0, 0.8 */
    uint32_t n_bias;                     /* <= 256 */
    const uint32_t * bias_ids;           /* host; each id < n_vocab */
    const float * bias_values;           /* host */
    uint64_t seed, offset;               /* draw i uses counter offset + i */
};
/* Draws one token from the context's device logits with counter `offset`; the state and the logits
 * are untouched.  Synchronous (4 bytes cross PCIe).  The device logits must follow the device state:
 * the last evaluation on the context computed them and no state was uploaded since; otherwise, and
 * for temperature < 0 or NaN, top_p outside [0, 1], n_bias > 256, a bias id >= n_vocab or a NULL
 * pointer, the call fails with RWKV_ERROR_ARGS.  A pipeline context fails with
 * RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED. */
RWKV_API bool rwkv_mi355x_sample(struct rwkv_context * ctx, const struct rwkv_mi355x_sampling * params,
                                 uint32_t * token_out);
/* The generation loop on the device: for i in [0, n): draw token i from the device logits with
 * counter offset + i, then evaluate it (rwkv_mi355x_eval_device of that one token with logits).
 * Nothing crosses PCIe and the host does not wait inside the loop; at the end the n tokens (and, when
 * logits_out != NULL, the final logits) are copied out and the stream is synchronised.  1 <= n <=
 * 65536 (else RWKV_ERROR_ARGS; the other argument errors as rwkv_mi355x_sample).  On return the
 * state has consumed all n tokens and the device logits are those following the last one, so a
 * second call with offset + n continues the same stream.  An in-launch hand-off timeout anywhere in
 * the chain fails the call with RWKV_ERROR_CTX, as rwkv_mi355x_eval_device(sync = false) followed by
 * rwkv_mi355x_sync does: nothing is re-run and the state is unspecified until it is uploaded again. */
RWKV_API bool rwkv_mi355x_generate(struct rwkv_context * ctx, const struct rwkv_mi355x_sampling * params, size_t n,
                                   uint32_t * tokens_out, float * logits_out);

/* Batched generation on the device: up to 256 sequences of one context sample, are penalised, stop
 * and decode together, one pass over the weights per step, nothing but the tokens crossing PCIe.
 *
 * Slots.  rwkv_mi355x_batch_reserve gives the context n_slots <= 256 generation slots (each a state
 * and its logits in HBM, apart from the context's own state; 0 frees them) and invalidates every
 * slot it had.  rwkv_mi355x_batch_store copies the context's device state and device logits into a
 * slot, device to device (the logits must follow the state, as for rwkv_mi355x_sample), and starts a
 * new sequence there: its token counts are zero and it is not finished.  rwkv_mi355x_batch_load is
 * the reverse: the context continues from the slot (rwkv_mi355x_sample / _generate /
 * _score_sequence / _eval_device).  A slot >= n_slots, a store without valid device logits and a load
 * of a slot that was never stored fail with RWKV_ERROR_ARGS.
 *
 * rwkv_mi355x_generate_batch runs rows = slots [0, B) for up to n steps.  Step i of a live row r:
 *   l = logits_r; for every token t with c = counts_r[t] > 0, in float32 and in this order,
 *     l_t = l_t - (presence[r] + (float)c * frequency[r])       (one multiply, one add, one subtract,
 *   none fused: rwkv_cpp.sampling.penalize restates it bit for bit.  The reference's chat loop,
 *   chat_with_bot.py:245-274, forms the penalty in double, so its l_t can differ by one rounding);
 *   l += bias; the draw of rwkv_mi355x_sample with temperature[r], top_p[r] and
 *   u = uniform(seed[r], offset[r] + i); counts_r[token] += 1.
 * If the token is one of stop_tokens the row is finished: the stop token is the last of its tokens
 * and is not evaluated.  Otherwise the token is evaluated (one batched decode step for all rows,
 * bit-identical to rwkv_mi355x_eval_device per row).  On return tokens_out[r][0 .. lengths_out[r]) are
 * the tokens row r drew in this call and the entries after them are 0xFFFFFFFF.  Slot r holds, for a
 * finished row, the state that has consumed every token before the stop token and the logits that
 * produced the stop token; for a row that never stopped (lengths_out[r] == n) the state that has
 * consumed all n tokens and the logits after the last, as rwkv_mi355x_generate leaves a context.
 * keep_counts != 0 continues the previous call on these slots: the counts go on, rows that finished
 * stay finished (lengths_out[r] == 0, slot unchanged), and with offset[r] + n the draws continue the
 * same streams, so two calls of n equal one of 2 n.  keep_counts == 0 starts every row afresh.
 * check_every = k > 0: every k steps the host reads the number of live rows (4 bytes, one
 * synchronisation) and leaves the loop when it is 0; the results do not depend on it.  steps_out
 * (may be NULL) receives the number of decode steps that ran.
 * Errors, all before anything is enqueued (RWKV_ERROR_ARGS; state and slots untouched): B == 0 or
 * B > the reserved slots, a slot in [0, B) never stored, n == 0 or n > 65536, a NULL required
 * pointer, a temperature < 0 or NaN, a top_p outside [0, 1], a NaN penalty, n_bias > 256, a bias id
 * >= n_vocab, n_stop > 16, a stop id >= n_vocab.  A pipeline context or a stage context fails with
 * RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED.  An in-launch hand-off timeout fails the call with
 * RWKV_ERROR_CTX and leaves slots [0, B) invalid (store them again). */
RWKV_API bool rwkv_mi355x_batch_reserve(struct rwkv_context * ctx, size_t n_slots);
RWKV_API size_t rwkv_mi355x_batch_slots(const struct rwkv_context * ctx);
RWKV_API bool rwkv_mi355x_batch_store(struct rwkv_context * ctx, size_t slot);
RWKV_API bool rwkv_mi355x_batch_load(struct rwkv_context * ctx, size_t slot);
struct rwkv_mi355x_batch_sampling {
    const float * temperature, * top_p;  /* host [B] */
    const float * presence, * frequency; /* host [B], or NULL: 0 */
    const uint64_t * seed, * offset;     /* host [B]; row r draw i: uniform(seed[r], offset[r] + i) */
    uint32_t n_bias;                     /* shared by the rows, <= 256 */
    const uint32_t * bias_ids;
    const float * bias_values;
    uint32_t n_stop;                     /* <= 16, each < n_vocab */
    const uint32_t * stop_tokens;
    uint32_t keep_counts;                /* 0: counts and finished rows start from zero; else continue the last call's */
    uint32_t check_every;                /* 0: never look; k: the host looks every k steps and leaves when no row is live */
};
RWKV_API bool rwkv_mi355x_generate_batch(struct rwkv_context * ctx, size_t B,
                                         const struct rwkv_mi355x_batch_sampling * params, size_t n,
                                         uint32_t * tokens_out /* [B][n] */, uint32_t * lengths_out /* [B] */,
                                         uint32_t * steps_out);

/* Continuous batching: a queue of Q sequences over L = min(lanes, Q) decode rows ("lanes").  The
 * sequences are slots [0, Q), filled as for rwkv_mi355x_generate_batch (batch_store or prefill_batch);
 * every per-row array of params is [Q], indexed by sequence; sequence s wants at most max_tokens[s]
 * tokens (host [Q], each in [1, n]; n <= 65536 is the row stride of tokens_out).  A lane whose
 * sequence has ended is given to the next waiting sequence between two decode steps, so the L rows
 * of a step stay full while sequences wait.  Step i = 0, 1, ...:
 *   1. Turnover, lanes in increasing order.  A lane whose sequence s is ended -- it drew a stop token
 *      at step i - 1, or length[s] == max_tokens[s] -- is freed.  Ended by its cap, s takes the lane's
 *      live state and logits as its result (the state after its last token, the logits following it:
 *      what generate_batch leaves for a row that never stopped); ended by a stop it has the state
 *      before the stop token and the logits that produced it, as in generate_batch.  The free lanes,
 *      in increasing order, take the waiting sequences in increasing order: state and logits from the
 *      slot, counts zero, lane_out[s] = the lane, start_out[s] = i.  At i = 0 sequences 0 .. L-1
 *      enter lanes 0 .. L-1.
 *   2. If no lane holds a sequence the call is over.
 *   3. Every busy lane samples with the parameters and counts of its sequence s and the draw
 *      uniform(seed[s], offset[s] + length[s]); the token goes to tokens_out[s][length[s]++]; a stop
 *      token ends s and is not evaluated.
 *   4. One batched decode step over the L lanes (idle lanes decode token 0).
 * Everything about sequence s -- tokens, length, slot s's state and logits on return -- equals, bit
 * for bit, rwkv_mi355x_generate_batch with B = 1, n = max_tokens[s], s's parameters and keep_counts
 * 0 on a slot filled the same way.  tokens_out[s] is 0xFFFFFFFF past lengths_out[s]; slot s is valid
 * and rwkv_mi355x_batch_load(s) continues it.  lane_out / start_out (may be NULL) are the list
 * schedule of the lengths drawn (rwkv_cpp.sampling.queue_schedule); steps_out (may be NULL) is the
 * number of decode steps up to the one after which no lane was busy.
 * keep_counts must be 0: a capped sequence that should go on with its counts is a job for
 * rwkv_mi355x_generate_batch on its slot.  check_every = k > 0: every k steps the host reads the
 * number of sequences not yet ended (4 bytes) and leaves when it is 0; with 0 it runs
 * ceil(sum(max_tokens) / L) + max(max_tokens) steps, which list scheduling cannot exceed, the steps
 * after the end decoding token 0 in idle lanes.  The results, steps_out included, do not depend on it.
 * Errors before anything is enqueued (RWKV_ERROR_ARGS; slots, state and logits untouched): Q == 0 or
 * above the reserved slots, lanes == 0 or > 256, a slot in [0, Q) never stored, n == 0 or > 65536, a
 * NULL required pointer, a max_tokens[s] of 0 or above n, keep_counts != 0, and the parameter errors
 * of generate_batch.  A pipeline or stage context: RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED.  A failure
 * after that (RWKV_ERROR_CTX) leaves slots [0, Q) invalid. */
RWKV_API bool rwkv_mi355x_generate_queue(struct rwkv_context * ctx, size_t Q, size_t lanes,
                                         const struct rwkv_mi355x_batch_sampling * params,
                                         const uint32_t * max_tokens /* host [Q] */, size_t n,
                                         uint32_t * tokens_out /* [Q][n] */, uint32_t * lengths_out /* [Q] */,
                                         uint32_t * lane_out /* [Q] */, uint32_t * start_out /* [Q] */,
                                         uint32_t * steps_out);

/* Log-probabilities of the tokens the four calls above draw: the drawn token's, and the top_k most
 * likely alternatives (what OpenAI-style APIs return as logprobs / top_logprobs).  They are taken
 * inside the sampling step, of the distribution the token was drawn from, so nothing but the results
 * crosses PCIe and no second pass over the weights is needed.
 *
 * For one draw of a live row let l be the float32 row the sampler samples from: the logits, then the
 * presence / frequency penalty over the counts before this draw's increment, then the bias, in the
 * order and roundings stated above (rwkv_cpp.sampling.penalize).  Temperature and top_p do not enter:
 * this is the p = softmax(l) of rwkv_mi355x_sample.
 *   m    = max l, exact in float32
 *   S    = sum_i exp((double)l_i - (double)m), exponentials and sum in double, one fixed association
 *   logZ = (double)m + log(S)
 *   token_logprob   = (double)l[token] - logZ
 *   top_ids[0 .. K) = the K first indices in the order "larger l first, lower index first among equal
 *                     l" (exact float32 compares).  A NaN element is never listed; with fewer than K
 *                     elements that are not NaN the remaining entries keep the fill (below).
 *   top_logprobs[j] = (double)l[top_ids[j]] - logZ, with the same logZ word: where the drawn token is
 *                     top_ids[j], token_logprob and top_logprobs[j] are bit-equal.
 * rwkv_cpp.sampling.logprobs restates this in float64 numpy.  A call is a pure function of its inputs.
 * Non-finite logits may give NaN or infinite values; they cannot hang or fault a call.
 *
 * Layout: rows = 1 for sample and generate, B for generate_batch, Q for generate_queue; n is the call's
 * n (1 for sample); the rows are n columns apart, as in tokens_out.  Draw i of row r fills column i of
 * row r (for the queue: the column the token goes to).  A column no draw filled -- past lengths_out[r],
 * or any column of a row that was already finished under keep_counts -- and a top entry left unlisted
 * hold the fill: every byte 0xFF, so an id of 0xFFFFFFFF and a NaN.  A row that stops reports the stop
 * token's own log-probability and alternatives: the stop token is a drawn token. */
#define RWKV_MI355X_MAX_TOP_LOGPROBS 20
struct rwkv_mi355x_logprobs {
    uint32_t top_k;          /* 0 .. 20 and <= n_vocab */
    double   * token_logprob;/* host [rows][n]; required */
    uint32_t * top_ids;      /* host [rows][n][top_k]; required iff top_k > 0 */
    double   * top_logprobs; /* host [rows][n][top_k]; required iff top_k > 0 */
};
/* Each is its sibling above plus lp; with lp == NULL it is that call (which forwards here).  Tokens,
 * lengths, states, logits and every other result are, bit for bit, those of the call without lp.
 * Besides the sibling's errors: top_k > 20, top_k > n_vocab, a NULL token_logprob, or top_k > 0 with a
 * NULL top_ids / top_logprobs fail with RWKV_ERROR_ARGS, and a failed allocation of the device arrays
 * (rows * n * (8 + 12 top_k) bytes and a word per row, grown before the loop) with RWKV_ERROR_ALLOC;
 * both before anything is enqueued: slots, state and logits are untouched. */
RWKV_API bool rwkv_mi355x_sample_logprobs(struct rwkv_context * ctx, const struct rwkv_mi355x_sampling * params,
                                          uint32_t * token_out, const struct rwkv_mi355x_logprobs * lp);
RWKV_API bool rwkv_mi355x_generate_logprobs(struct rwkv_context * ctx, const struct rwkv_mi355x_sampling * params,
                                            size_t n, uint32_t * tokens_out, float * logits_out,
                                            const struct rwkv_mi355x_logprobs * lp);
RWKV_API bool rwkv_mi355x_generate_batch_logprobs(struct rwkv_context * ctx, size_t B,
                                                  const struct rwkv_mi355x_batch_sampling * params, size_t n,
                                                  uint32_t * tokens_out /* [B][n] */, uint32_t * lengths_out /* [B] */,
                                                  uint32_t * steps_out, const struct rwkv_mi355x_logprobs * lp);
RWKV_API bool rwkv_mi355x_generate_queue_logprobs(struct rwkv_context * ctx, size_t Q, size_t lanes,
                                                  const struct rwkv_mi355x_batch_sampling * params,
                                                  const uint32_t * max_tokens /* host [Q] */, size_t n,
                                                  uint32_t * tokens_out /* [Q][n] */, uint32_t * lengths_out /* [Q] */,
                                                  uint32_t * lane_out /* [Q] */, uint32_t * start_out /* [Q] */,
                                                  uint32_t * steps_out, const struct rwkv_mi355x_logprobs * lp);

/* Batched prefill: n_rows prompts, concatenated in `tokens` (lengths[i] >= 1 tokens each), are
 * evaluated together in packed sequence passes and land in slots[i] (distinct, each < the reserved
 * slots).  cont == NULL or cont[i] == 0: row i starts from the fresh state (the slot need not have
 * been stored); cont[i] != 0: it continues from the slot's state (the slot must be valid).  The head
 * runs on each row's last token.  On return slot slots[i] is what state_upload(NULL) [or batch_load],
 * rwkv_mi355x_eval_device(row i, logits) and rwkv_mi355x_batch_store(slots[i]) leave there, bit for
 * bit: state, logits, zero counts, not finished.  Other slots, the context's device state and its
 * device logits are untouched.  Synchronous; only the tokens cross PCIe.
 *
 * The rows are packed, in order, into passes of at most 1024 tokens; a row that crosses a pass is
 * split and its next piece continues from the state the previous one wrote, so the packing never
 * shows in the results.  The weights are read once per pass instead of once per prompt.
 *
 * n_rows == 0 or above the reserved slots, a NULL slots / tokens / lengths, a slot at or above the
 * reserved count or named twice, a zero length, a token >= n_vocab and cont[i] != 0 on a slot that
 * was never stored fail with RWKV_ERROR_ARGS before anything is enqueued: every slot is as it was.
 * A failure after that (RWKV_ERROR_CTX) leaves the slots of the call invalid.  A pipeline or stage
 * context fails with RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED. */
RWKV_API bool rwkv_mi355x_prefill_batch(struct rwkv_context * ctx, size_t n_rows, const uint32_t * slots,
                                        const uint32_t * tokens, const size_t * lengths, const uint8_t * cont);

/* Scoring: rwkv_mi355x_eval_device over T >= 1 tokens with the head on EVERY token.  Position t's
 * logits row (the logits serial rwkv_eval of tokens[0..t] gives, bit for bit) is reduced on the device
 * to losses_out[t] = -log softmax(row t)[targets[t]] (the exponentials and their sum in fp64) and
 * argmax_out[t] = the lowest index holding the row's maximum; only those cross PCIe, plus the rows
 * themselves when logits_out != NULL.  targets [T] and losses_out [T] are both NULL or both set (else
 * RWKV_ERROR_ARGS), every target must be < n_vocab (else RWKV_ERROR_ARGS, checked with the tokens
 * before anything is enqueued: the state is untouched); argmax_out [T] and logits_out [T][n_vocab]
 * (host) may each be NULL.  Synchronous.  On return the device state has consumed all T tokens and
 * the device logits are those of the last one, as after rwkv_mi355x_eval_device(compute_logits =
 * true), so rwkv_mi355x_sample / _generate or another score call continue from there.  A pipeline
 * context or a stage context without the head fails with RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED; an
 * in-launch hand-off timeout in a one-token chunk fails the call with RWKV_ERROR_CTX. */
RWKV_API bool rwkv_mi355x_score_sequence(struct rwkv_context * ctx, const uint32_t * tokens, size_t T,
                                         const uint32_t * targets, double * losses_out,
                                         uint32_t * argmax_out, float * logits_out);

/* Debugging aid: copies `bytes` of the named workspace buffer of the last evaluation to host `out`
 * (names: x xa sx r k v g w y a nb bb vfirst fr lora bonus logits, slot<i>.<q|d|s|qsum|h|f>).
 * Returns the bytes copied, or -1 (unknown name / copy failure).  Not part of rwkv.h. */
RWKV_API long long rwkv_mi355x_debug_buffer(struct rwkv_context * ctx, const char * name, void * out, size_t bytes);
/* Test hooks (not part of rwkv.h): "skip_granule" = index of a k_v6_att_fused producer workgroup that
 * publishes nothing (-1: off), so the in-launch hand-off times out and the next synchronising call
 * fails with RWKV_ERROR_CTX; "spin_max" = the hand-off sweep bound in passes (<= 0: the default
 * 2^20).  Returns false for an unknown name or a NULL context. */
RWKV_API bool rwkv_mi355x_debug_set(struct rwkv_context * ctx, const char * name, long long value);

/* One stage of the layer pipeline (the reference has no such entry point -- it is
 * the unit the multi-GPU sequence evaluation is built from, rwkv.cppy_amd/python/rwkv_cpp/pipeline.py).
 * Runs layers [layer_begin, layer_end) over T tokens on the device-resident state; only those
 * layers' state slices change.  x_dev / vfirst_dev: device buffers [T][n_embed] fp32 on the
 * context's GPU with the residual stream (and, v7 only, the layer-0 values v_first) entering
 * layer_begin; on return they hold the ones leaving layer_end - 1.  layer_begin == 0 embeds
 * `tokens` instead of reading x_dev (which may then be NULL).  When layer_end == n_layer and
 * compute_logits, the head runs on the last token (logits_out host, may be NULL).  Synchronous.
 * The same tensors, chunked along T, give results bit-identical to rwkv_eval_sequence. */
RWKV_API bool rwkv_mi355x_eval_layers(struct rwkv_context * ctx, const uint32_t * tokens, size_t T,
                                      uint32_t layer_begin, uint32_t layer_end, float * x_dev, float * vfirst_dev,
                                      bool compute_logits, float * logits_out);

/* The same stage, enqueued on the context's stream (rwkv_mi355x_stream) without waiting for it:
 * the caller orders its own work (e.g. an RCCL send of x_dev) on that stream.  Logits, when
 * computed, stay on the device (rwkv_mi355x_logits_device). */
RWKV_API bool rwkv_mi355x_eval_layers_async(struct rwkv_context * ctx, const uint32_t * tokens, size_t T,
                                            uint32_t layer_begin, uint32_t layer_end, float * x_dev, float * vfirst_dev,
                                            bool compute_logits);
/* The context's device logits buffer [n_vocab] (NULL for a NULL context).  It holds valid logits
 * only after an evaluation that computed them: on the context holding the head (the last stage)
 * with compute_logits / a logits request; otherwise its contents are stale. */
RWKV_API float * rwkv_mi355x_logits_device(struct rwkv_context * ctx);

/* A pipeline stage's context: only layers [layer_begin, layer_end) are uploaded (plus the
 * embedding when layer_begin == 0 and the head when layer_end == n_layer), so a stage's HBM holds
 * ~1/P of the weights (reference placement by layer range: rwkv_model_loading.inc:128-142).  The
 * state keeps the full layout.  Whole-model calls (rwkv_eval, ...) fail with
 * RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED on such a context; rwkv_mi355x_eval_layers accepts
 * ranges inside [layer_begin, layer_end). */
RWKV_API struct rwkv_context * rwkv_mi355x_init_from_file_layers(const char * path, uint32_t n_threads,
                                                                 uint32_t layer_begin, uint32_t layer_end);

/* The layer pipeline behind the reference entry points: n_stages stage contexts in
 * this process, stage i on GPU devices[i] (NULL: i modulo the device count) holding the contiguous
 * layers [i*L/P .. (i+1)*L/P) (earlier stages take the extra layers; the embedding on stage 0, the
 * head on the last).  rwkv_eval / rwkv_eval_sequence[_in_chunks] on the returned context (stage 0)
 * run every stage: the sequence is cut into chunks of >= 256 tokens, chunk c's residual stream
 * (and v7's v_first) crosses from stage s to s+1 by a peer copy over xGMI while stage s starts
 * chunk c+1; results are bit-identical to a single-GPU context.  rwkv_clone_context clones the
 * pipeline (same stages and GPUs, weights shared).  The same context is what rwkv_init_from_file
 * returns when RWKV_MI355X_PIPELINE=P (P >= 2) is set (devices: RWKV_MI355X_PIPELINE_DEVICES, a
 * comma list).  Adjacent stages on different GPUs get peer access enabled at init (a GPU pair
 * without it fails the init).  rwkv_eval_sequence_in_chunks passes chunk_size to the pipeline as
 * its chunk (the results do not depend on it).  rwkv_mi355x_state_upload / _download / sync act on
 * every stage; the other device-resident entry points (eval_device, eval_batch*, stream,
 * device_state, clone_context_on) refuse a pipeline context with RWKV_ERROR_UNSUPPORTED. */
RWKV_API struct rwkv_context * rwkv_mi355x_init_pipeline(const char * path, uint32_t n_threads, int n_stages,
                                                         const int * devices);
/* Stages of a context: P for a pipeline context, 1 otherwise (0 for NULL). */
RWKV_API int rwkv_mi355x_pipeline_stages(const struct rwkv_context * ctx);
/* Adjacent stage pairs of a pipeline context that sit on different GPUs (their hop is a peer copy
 * over xGMI, peer access enabled at init); 0 when every stage shares one GPU or for a non-pipeline. */
RWKV_API int rwkv_mi355x_pipeline_peer_pairs(const struct rwkv_context * ctx);

/* Batched decode (multi-context serving): n_contexts independent sequences of this
 * model advance ONE token each in one pass -- the rwkv_eval of each context, with every weight byte
 * read once per step for all of them (the reference runs clones side by side instead:
 * rwkv_clone_context, rwkv.h:93-99, rwkv.cpp:123-139).  Results are bit-identical to
 * rwkv_eval(ctx, tokens[i], state_in + i * state_len, ...) for every i.
 * tokens: host [n_contexts]; state_in / state_out: [n_contexts][state_len] (state_in NULL = fresh
 * states, state_out NULL = not returned); logits_out: [n_contexts][logits_len] or NULL.
 * n_contexts <= 256.  Host buffers; synchronous. */
RWKV_API bool rwkv_mi355x_eval_batch(struct rwkv_context * ctx, const uint32_t * tokens, size_t n_contexts,
                                     const float * state_in, float * state_out, float * logits_out);
/* The same with state_in / state_out / logits_out in device memory of the context's GPU (no PCIe
 * traffic; state_in != state_out; NULL state_out / logits_out: kept in library buffers).
 * Enqueued on the context's stream (rwkv_mi355x_stream); returns without waiting. */
RWKV_API bool rwkv_mi355x_eval_batch_device(struct rwkv_context * ctx, const uint32_t * tokens, size_t n_contexts,
                                            const float * state_in, float * state_out, float * logits_out);

/* The context's HIP stream (hipStream_t), so callers can time kernels with events on it. */
RWKV_API void * rwkv_mi355x_stream(struct rwkv_context * ctx);

/* Device pointer of the current device-resident state (state_len floats). */
RWKV_API float * rwkv_mi355x_device_state(struct rwkv_context * ctx);

/* Per-token algorithmic HBM bytes of one decode step (weights read + state read/written),
 * counted from the original block sizes (Q4_0 18 B / 32 weights ...), see DESIGN.md. */
RWKV_API double rwkv_mi355x_decode_bytes(const struct rwkv_context * ctx, bool with_logits);

/* Algorithmic bytes of the model's weight matrices only (all layers, + head if asked). */
RWKV_API double rwkv_mi355x_weight_bytes(const struct rwkv_context * ctx, bool with_head);

/* 2*M*K summed over every matmul of one token (head included if asked). */
RWKV_API double rwkv_mi355x_matmul_flops_per_token(const struct rwkv_context * ctx, bool with_head);

/* Architecture info: out[0..3] = arch_major, arch_minor, head_count, head_size. */
RWKV_API void rwkv_mi355x_arch(const struct rwkv_context * ctx, int64_t out[4]);

/* Writes a synthetic rwkv.cpp model file with the exact tensor shapes of a real checkpoint,
 * seeded random weights (N(0, 1/sqrt(fan_in)) for matrices), quantized with this library's
 * quantizer.  arch: 4, 5 (v5.2), 6, 7.  fmt: "FP32" "FP16" "Q4_0" "Q4_1" "Q5_0" "Q5_1" "Q8_0".
 * ffn = 0 picks the architecture's default FFN width; head_size 64 for v5+; lora dims of
 * the real checkpoints.  Used by bench.py (no checkpoints are downloadable). */
RWKV_API bool rwkv_mi355x_write_synthetic_model(const char * path, int arch, uint32_t n_vocab,
                                                uint32_t n_embed, uint32_t n_layer, uint32_t ffn,
                                                const char * fmt, uint64_t seed);

/* Options of rwkv_mi355x_write_synthetic_model_ex (test infrastructure: data the plain writer never
 * produces).  All zero = the plain writer.
 *   norms       nonzero: the weights of ln0 / ln1 / ln2 / ln_out / att.ln_x are U(0.5, 1.5) with every
 *               17th channel (c % 17 == 16) negated, the biases U(-0.5, 0.5), each tensor from its own
 *               seed (the plain writer stores ones and zeros: every norm the identity).
 *   wide_decay  nonzero: v6 time_decay and v7 w0 are U(-8, 2); v5 time_decay is exp(-exp(U(-8, 2)));
 *               v4 time_first is U(-4, 4) and time_decay -exp(U(-3, 3)).
 *   maa_d, decay_d            v6 LoRA widths (time_maa_w1 is C x 5 maa_d, time_decay_w1 C x decay_d)
 *   w_d, a_d, v_d, g_d        v7 LoRA widths (w1 / a1 / v1 / g1 are C x width)
 *               0 keeps the plain writer's width.  A width whose matrix the file format quantizes
 *               (v6 time_decay_w2, K = decay_d) must be a multiple of 32 there; the call fails otherwise.
 *               The writer stores any other width; rwkv_init_from_file refuses maa_d > 64 and decay /
 *               v7 widths that are no multiple of 32 (the CPU oracle of tests/ takes them all). */
struct rwkv_mi355x_synth_opts {
    uint32_t norms;
    uint32_t wide_decay;
    uint32_t maa_d, decay_d;
    uint32_t w_d, a_d, v_d, g_d;
};

/* rwkv_mi355x_write_synthetic_model with options; opts == NULL writes the same bytes as the plain
 * entry, which calls this one. */
RWKV_API bool rwkv_mi355x_write_synthetic_model_ex(const char * path, int arch, uint32_t n_vocab,
                                                   uint32_t n_embed, uint32_t n_layer, uint32_t ffn,
                                                   const char * fmt, uint64_t seed,
                                                   const struct rwkv_mi355x_synth_opts * opts);

/* Kernel timing: while on, every matmul launch on the context stream is bracketed by hipEvents
 * (decode runs eagerly, not from the captured graph) and accumulated per kernel class -- the
 * template instantiation name rocprofv3 reports, e.g. "k_mm<2, 2, 1>" (weight type, rows per
 * wave, columns per pass).  Turning it on clears the counters. */
RWKV_API void rwkv_mi355x_set_kernel_timing(struct rwkv_context * ctx, bool on);
/* Reads counter `index`; returns the number of kernel classes (call with index -1 to count).
 * total_bytes: algorithmic bytes (weights at original block sizes + activations in/out). */
RWKV_API int rwkv_mi355x_kernel_stats(struct rwkv_context * ctx, int index, char * name, size_t name_len,
                                      long long * launches, double * total_ms, double * total_bytes,
                                      double * total_flops);

/* ---- kernel self-tests (used by tests/ for per-kernel parity; not on the eval path) ----
 * Runs the library's activation quantizer (the emit stage every producer kernel uses) on
 * x [T][K] (host) for the activation format of weight type `wtype` (rwkv file type id) and
 * returns the int8 codes, fp16-rounded scales d and (Q8_1) s, as fp32.  q/d/s may be NULL. */
RWKV_API bool rwkv_mi355x_selftest_quantize_act(int wtype, const float * x, int T, int K, int8_t * q, float * d,
                                                float * s);
/* Runs the decode/sequence matmul kernel on W (ggml block bytes of type wtype, ne=[K, M],
 * host) and x [T][K] (host): y [T][M] = W x with the library's activation quantization. */
RWKV_API bool rwkv_mi355x_selftest_matmul(int wtype, const void * W, int K, int M, const float * x, int T, float * y);

// Self-test of the sequence GEMM: the same product as rwkv_mi355x_selftest_matmul computed by
// the int8-MFMA kernel (quantized weight types only; T >= 2).
RWKV_API bool rwkv_mi355x_selftest_gemm(int wtype, const void * W, int K, int M, const float * x, int T, float * y);
/* The same with the GEMM's split-K form forced: split 1 = one workgroup per tile, 4 / 8 = the class
 * tree in that many subtrees on as many workgroups plus the combine kernel (same bits). */
RWKV_API bool rwkv_mi355x_selftest_gemm_split(int wtype, const void * W, int K, int M, const float * x, int T,
                                              float * y, int split);

/* One entry of a matmul group (MMGroup, csrc/common.hpp) on host operands: y [T][M] = epi(W x).
 * W: ggml block bytes of type wtype, ne = [K, M]; epi: the Epi value 0..10.  y0 (initial y), aux:
 * [T][M], bias: [M]; NULL where the epilogue does not read them (y then starts as zeros).  emit != 0:
 * the post-epilogue values are also emitted as the next matmul's input, Q8_0 blocks or (out_q8_1)
 * Q8_1, returned row-major: q [T][M], d / s / qsum [T][M / 32] (any may be NULL; s is written for
 * Q8_1 only).  out_tiled: emit into token-tile records instead.  Forms 0, 1, 3 do not return those (a
 * shape the launchers' coverage rules must tell apart).  Form 2 (the GEMM) takes emitting entries with
 * out_tiled only and reports in `fused` whether launch_qgemm emitted inside the launch (fuse_emit):
 * fused = 1: the tile records come back de-tiled into q / d / s / qsum (qsum = the sums of the returned
 * codes), and y is NOT written by the direct kernel (it keeps what the caller's y held; the split-K
 * combine writes both); fused = 0: y is written and nothing is emitted (that pass is the caller's). */
struct rwkv_mi355x_selftest_mm_entry {
    int wtype;
    const void * W;
    int M;
    int epi;
    const float * y0;
    const float * aux;
    const float * bias;
    int emit;
    int out_q8_1;
    int out_tiled;
    /* out, form 2: MMEntry::fuse_emit as launch_qgemm set it (0 from the other forms).  It is the last
     * of the int fields and not the struct's last member on purpose: here it fills what was alignment
     * padding in front of y, so sizeof (104 on LP64) and every older field's offset are what they were
     * and a caller built against the struct without it still walks an array of entries correctly. */
    int fused;
    float * y;
    int8_t * q;
    float * d;
    float * s;
    int32_t * qsum;
};
/* Runs a whole group of n <= 8 entries over x [T][K] (host, shared by the entries, in entry 0's
 * activation format) through one launcher: form 0 = launch_mm_group (k_mm / k_mm_small, or k_fmm where
 * it applies), 1 = launch_mvb_group (k_mvb), 2 = launch_qgemm (token-tile input; emitting entries with
 * out_tiled), 3 = launch_fmm_group.  split (0, 1, 4, 8) is MMGroup::split.  *launched = 1 when the
 * launcher took the group, 0 when forms 1 / 3 declined it (the outputs are then untouched).  false only
 * on an error. */
RWKV_API bool rwkv_mi355x_selftest_matmul_group(int form, int split, int T, int K, const float * x, int n,
                                                struct rwkv_mi355x_selftest_mm_entry * entries, int * launched);

/* One entry of a decode matvec group (MVGroup, csrc/kernels.hpp) on host operands: y [M] = epi(W v),
 * v the entry's input row.  W: ggml block bytes of type wtype, ne = [K, M].  src 0 (SRC_ACT): v = x [K]
 * quantized on the device into wtype's activation format (entries of one format, K and x share the
 * buffer); 1 (SRC_F32): v = x [K], quantized by the kernel; 2 (SRC_LNMIX): v = the token-shift mix of
 * xa = LayerNorm(x; lnw, lnb) with carry [K] and mu [K] -- form 0: xa * mu + (carry - carry * mu),
 * 1: (carry - xa) * mu + xa, 2: xa (carry and mu unused).  carry_out [K] (optional) receives xa.  mu2
 * (optional, forms 0 / 1, quantized wtype): the same mix with mu2, quantized, comes back in q2 [K],
 * d2 / s2 / qsum2 [K / 32].  epi, y0, aux [M], bias [M], emit / out_q8_1 and q [M], d / s / qsum
 * [M / 32]: as in rwkv_mi355x_selftest_mm_entry with T = 1.  Every output starts on the device as
 * 0xA5 bytes (y: as y0 where given), so what the kernel leaves unwritten shows. */
struct rwkv_mi355x_selftest_mv_entry {
    int wtype;
    const void * W;
    int M, K;
    int src;
    const float * x;
    const float * carry;
    const float * lnw;
    const float * lnb;
    const float * mu;
    const float * mu2;
    int form;
    int epi;
    const float * y0;
    const float * aux;
    const float * bias;
    int emit;
    int out_q8_1;
    float * y;
    int8_t * q;
    float * d;
    float * s;
    int32_t * qsum;
    float * carry_out;
    int8_t * q2;
    float * d2;
    float * s2;
    int32_t * qsum2;
};
/* What launch_mv_group decided: MVGroup::rows, grid, stride, units_max, and the compute-unit count its
 * thresholds used. */
struct rwkv_mi355x_selftest_mv_shape {
    int rows, grid, stride, units_max, cus;
};
/* Runs one MVGroup of n <= 8 entries through launch_mv_group.  *launched = 0 when the launcher refused
 * the group (nothing enqueued, the outputs untouched; shape is then not written either), else 1 with the
 * outputs and *shape filled.  false only on an error of the harness itself (bad arguments, allocation,
 * a HIP error). */
RWKV_API bool rwkv_mi355x_selftest_mv_group(int n, const struct rwkv_mi355x_selftest_mv_entry * entries,
                                            struct rwkv_mi355x_selftest_mv_shape * shape, int * launched);
/* launch_mv_sigmul (k_mvsig): y [M] = y0 + sigmoid(Wr xr) * (Wv k).  Wv: ggml block bytes of type
 * wtype_v, ne = [F, Mv], k [F]; Wr: type wtype_r, ne = [C, Mr], xr [C].  *launched =
 * mv_sigmul_supported's answer; 0 leaves y untouched. */
RWKV_API bool rwkv_mi355x_selftest_mv_sigmul(int wtype_v, const void * Wv, int Mv, int F, const float * k, int wtype_r,
                                             const void * Wr, int Mr, int C, const float * xr, const float * y0,
                                             float * y, int * launched);

/* WKV-6 (v5 / v6 time mixing, head size 64) over T tokens of one context on host operands:
 * chunked = 0 runs the serial kernel (bit-exact with decode), 1 the chunk-parallel form
 * (RWKV_MI355X_WKV_CHUNK; re-associated sums).  k, v, r: [T][H*64]; w: [T][H*64] (w_per_token = 1,
 * v6) or [H*64] (v5); u: [H*64]; state_in / state_out: [H][64 key][64 value]; y: [T][H*64]. */
RWKV_API bool rwkv_mi355x_selftest_wkv6(int T, int H, int chunked, int w_per_token, const float * k, const float * v,
                                       const float * r, const float * u, const float * w, const float * state_in,
                                       float * state_out, float * y);

/* WKV-7 (v7 time mixing, head size 64) over T tokens of one context on host operands: chunked = 0 the
 * serial kernel (bit-exact with decode), 1 the chunk-parallel form (RWKV_MI355X_WKV_CHUNK; re-associated
 * sums).  r, w, k, v, a, b: [T][H*64] (a, b: the transition's rank-one factors, -kk and kk * a in
 * rwkv_operators_wkv_v7.inc:37-107); state_in / state_out: [H][64 value][64 key]; y: [T][H*64]. */
RWKV_API bool rwkv_mi355x_selftest_wkv7(int T, int H, int chunked, const float * r, const float * w, const float * k,
                                       const float * v, const float * a, const float * b, const float * state_in,
                                       float * state_out, float * y);

/* The token layouts of the serial WKV kernels against each other, bit for bit.  kind 4: WKV-4 over
 * C = H * S channels; 5 / 6: WKV-6 with a per-channel (v5) / per-token (v6) decay; 7: WKV-7 (5 - 7: H
 * heads of S, a power of two <= 64).  The n_seg segments of lens[s] >= 1 tokens tile a packed chunk;
 * operands and one input state per segment are drawn from the seed (sample_uniform: k, v, r, a, b
 * and the states in [-0.5, 0.5), WKV-6 / -7 decays in [0.9, 1), WKV-4: decay in (-1, -0.9], bb in
 * [0.5, 1.5), pp = 0).  Runs (a) one one-sequence launch per segment on its rows and state, (b) one
 * segmented launch over the chunk, (c) for kind 4 with every length 1, the contexts form of batched
 * decode; each form's outputs start as a poison word of its own.  out[0], out[1]: 32-bit words of the
 * output rows / of the written output state that differ between (a) and (b); out[2], out[3]: the same
 * between (a) and (c); out[4], out[5]: words compared for each pair (0 when (c) did not run). */
RWKV_API bool rwkv_mi355x_selftest_wkv_layouts(int kind, int H, int S, const uint32_t * lens, int n_seg, uint64_t seed,
                                               uint64_t * out);

/* The sampler kernel of rwkv_mi355x_sample on host operands: logits [rows][V] (V <= 262144), one
 * uniform draw u[r] in [0, 1) per row, params' seed / offset unused.  tokens [rows]; kept [rows] (the
 * tokens that passed the top-p filter; 1 for greedy) and cutoff [rows] (the smallest kept
 * probability) may be NULL. */
RWKV_API bool rwkv_mi355x_selftest_sample(const float * logits, int rows, int V,
                                          const struct rwkv_mi355x_sampling * params, const float * u,
                                          uint32_t * tokens, uint32_t * kept, float * cutoff);

/* The sampler kernel of rwkv_mi355x_generate_batch (k_sample_rows) on host operands, as step `step`
 * of a call: logits [rows][V]; params' temperature, top_p, presence, frequency (host [rows]; the
 * penalties may be NULL), bias and stop tokens (seed, offset, keep_counts, check_every unused); one
 * draw u[r] per row.  counts [rows][V] (may be NULL: no penalties) and done [rows] are read and
 * written.  tokens, decode_tokens (what the decode step would embed), kept, cutoff, lengths [rows]
 * and active (one word) are uploaded first and downloaded afterwards, so an entry the kernel does
 * not write keeps the caller's value; none of them may be NULL. */
RWKV_API bool rwkv_mi355x_selftest_sample_rows(const float * logits, int rows, int V,
                                               const struct rwkv_mi355x_batch_sampling * params, const float * u,
                                               uint32_t step, uint32_t * counts, uint32_t * done, uint32_t * tokens,
                                               uint32_t * decode_tokens, uint32_t * kept, float * cutoff,
                                               uint32_t * lengths, uint32_t * active);

/* The two self-tests above with log-probabilities: k_logprobs in front of the sampler's LP form, as
 * the rwkv_mi355x_*_logprobs calls launch them.  top_k in [0, 20] and <= V; token_logprob [rows],
 * top_ids and top_logprobs [rows][top_k] (not NULL, also for top_k == 0) are uploaded first and
 * downloaded afterwards, so an entry the kernels do not write keeps the caller's value.  Everything
 * else is the argument of the same name above. */
RWKV_API bool rwkv_mi355x_selftest_sample_logprobs(const float * logits, int rows, int V,
                                                   const struct rwkv_mi355x_sampling * params, const float * u,
                                                   uint32_t * tokens, uint32_t * kept, float * cutoff, uint32_t top_k,
                                                   double * token_logprob, uint32_t * top_ids, double * top_logprobs);
RWKV_API bool rwkv_mi355x_selftest_sample_rows_logprobs(const float * logits, int rows, int V,
                                                        const struct rwkv_mi355x_batch_sampling * params,
                                                        const float * u, uint32_t step, uint32_t * counts,
                                                        uint32_t * done, uint32_t * tokens, uint32_t * decode_tokens,
                                                        uint32_t * kept, float * cutoff, uint32_t * lengths,
                                                        uint32_t * active, uint32_t top_k, double * token_logprob,
                                                        uint32_t * top_ids, double * top_logprobs);

/* The turnover kernel of rwkv_mi355x_generate_queue (k_gen_turnover) on host operands, as before step
 * `step`: lane_seq [lanes] (a sequence id < Q or 0xFFFFFFFF: idle), done / lane / start [Q], *next
 * (<= Q) and *active are uploaded, updated and downloaded; length and max_tokens [Q] are read;
 * retire_to and admit_from [lanes] are uploaded, written and downloaded.  lanes in [1, 256]. */
RWKV_API bool rwkv_mi355x_selftest_gen_turnover(int lanes, int Q, uint32_t step, uint32_t * lane_seq, uint32_t * done,
                                                const uint32_t * length, const uint32_t * max_tokens, uint32_t * lane,
                                                uint32_t * start, uint32_t * next, uint32_t * active,
                                                uint32_t * retire_to, uint32_t * admit_from);

/* The host planner of rwkv_mi355x_prefill_batch (no GPU call): packs n_rows rows of lengths[i] >= 1
 * tokens, in order, into chunks of at most cap tokens.  Segment j is seg_len[j] tokens of row
 * seg_row[j], from token seg_begin[j] of chunk seg_chunk[j] on.  Returns the number of segments, -1
 * when max_segs is too small (nothing past it is written), -2 for n_rows == 0, cap == 0 or a zero length. */
RWKV_API long long rwkv_mi355x_selftest_prefill_plan(const size_t * lengths, size_t n_rows, size_t cap, uint32_t * seg_row,
                                                     uint32_t * seg_begin, uint32_t * seg_len, uint32_t * seg_chunk,
                                                     size_t max_segs);

/* k_xent on host operands (tests): logits [rows][V], targets [rows]; losses / argmax may be NULL */
RWKV_API bool rwkv_mi355x_selftest_xent(const float * logits, int rows, int V, const uint32_t * targets,
                                        double * losses, uint32_t * argmax);

/* k_groupnorm (the sequence path's per-head norm after WKV) on host operands, fp32 output:
 * out = ((y - mean_head) / sqrt(var_head + eps) * w + b [+ v * bonus, mode 2]) [* g, modes 1 and 2].
 * y, g, v, out: [T][H*S]; w, b: [H*S]; bonus: [T][H].  S: a power of two <= 64; H*S % 32 == 0.
 * g is unused in mode 0, v and bonus unless mode 2 (may be NULL then). */
RWKV_API bool rwkv_mi355x_selftest_groupnorm(int T, int H, int S, float eps, int mode, const float * y,
                                             const float * w, const float * b, const float * g, const float * v,
                                             const float * bonus, float * out);

/* k_ln_emit (the LayerNorm in front of the head, eps 1e-5) on host operands, fp32 output:
 * x, out: [rows][C]; w, b: [C]; C % 64 == 0. */
RWKV_API bool rwkv_mi355x_selftest_ln(int C, int rows, const float * x, const float * w, const float * b, float * out);

/* The decode matvecs' multi-row wave reduction (wave_sums) against the single-row tree (wave_sum63),
 * one wave on host operands.  n = 2, 4, ..., 64: p [64 lanes][n]; sums[l] = the result of lane l
 * (slot l & (n - 1)); ref[j] = the single-row tree of slot j.  n = 3 / -3: the padded three-row
 * form on p [64][6] (acc then acc2 per lane) for a plain / a _1 format; ref[j] = the per-row
 * expression (sum + 0.0f / sum + sum2).  sums: 64 floats, ref: |n| floats. */
RWKV_API bool rwkv_mi355x_selftest_wave_sums(int n, const float * p, float * sums, float * ref);

#if defined(__cplusplus)
}
#endif

#endif
