// engine_batch.hip -- batched decode (eval_batch), the generation slots and batched generation.
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "engine.hpp"
#include "kernels.hpp"

namespace rwkvmi {

// B independent contexts of this model advance one token each in one pass: the layer matmuls
// run the decode matvec kernel (k_mm) over the B activation rows, so every weight byte is read
// once per step for all B contexts, and each context's arithmetic is exactly its single-token
// decode (same lane/block association, same kernels' per-token math); token shift and the wkv
// recurrences take context t's state at t * state_len (LnMixArgs::bs, launch_wkv* bs).
// states: [B][state_len] contiguous.  dev: pointers are device memory (else host).
bool Engine::eval_batch(const uint32_t * tokens, size_t B, const float * state_in, float * state_out,
                        float * logits_out, bool dev) {
    HIP_OK(hipSetDevice(m_->device));
    co_ = false;  // batched decode: the ordered layouts only
    if (B == 0) return true;
    if (B > (size_t)kBatchMax) {
        fprintf(stderr, "rwkv: batched decode takes at most %d contexts (got %zu)\n", kBatchMax, B);
        return false;
    }
    if (!ensure_workspace((int)B)) return false;
    const size_t n = m_->state_len, V = m_->n_vocab;
    // tokens == NULL (generate_batch): the tokens are already in dtokens_[0 .. B) (the sampler wrote
    // them), every buffer is the caller's device memory and nothing is staged
    if (!tokens && !(dev && state_in && state_out && logits_out)) return false;
    if (tokens) {
        const size_t cap = doubled(1, B);
        if (!grow(bstate_[0], B * n, cap * n, GRAPHS_BATCH) || !grow(bstate_[1], B * n, cap * n, GRAPHS_BATCH) ||
            !grow(blogits_, B * V, cap * V, GRAPHS_BATCH))
            return false;
    }
    if (tokens && !stage_tokens(tokens, B)) return false;
    // input states: device pointer as given, else staged into bstate_[0] (NULL = fresh states)
    const float * sin = state_in;
    if (!state_in) {
        if (!init_state(bstate_[0], B * n)) return false;
        sin = bstate_[0];
    } else if (!dev) {
        HIP_OK(hipMemcpyAsync(bstate_[0], state_in, B * n * 4, hipMemcpyHostToDevice, stream_));
        sin = bstate_[0];
    }
    float * sout = (dev && state_out) ? state_out : bstate_[1].get();
    float * lout = (dev && logits_out) ? logits_out : blogits_.get();
    const bool lg = logits_out != nullptr;
    // the batched forward: the eager step and the captured one enqueue from the same value
    const SeqRun run = rows_run((int)B, n, sin, sout, lg ? lout : nullptr);
    auto step = [&] { return forward_range(run); };
    bool ok;
    if (use_graphs_ && !timing_) {
        // one graph per (B, state pointers, logits pointer): a decode loop alternating two state
        // buffers replays two graphs
        hipGraphExec_t ge = nullptr;
        for (const BatchGraph & g : bgraphs_)
            if (g.B == B && g.sin == sin && g.sout == sout && g.lout == (lg ? lout : nullptr)) ge = g.ge;
        if (!ge) {
            // first step with these buffers: run it eagerly (lazy GEMM scratch allocations happen
            // here, outside any capture), then capture the graph the next steps replay
            if (!step()) {
                (void)hipStreamSynchronize(stream_);
                return false;
            }
            if (bgraphs_.size() >= 8) drop_batch_graphs();
            if (!capture(ge, step)) return false;
            bgraphs_.push_back(BatchGraph{B, sin, sout, lg ? lout : nullptr, ge});
        } else {
            HIP_OK(hipGraphLaunch(ge, stream_));
        }
        ok = true;
    } else {
        ok = step();
    }
    if (!ok) {
        (void)hipStreamSynchronize(stream_);
        return false;
    }
    if (!dev) {
        if (logits_out) HIP_OK(hipMemcpyAsync(logits_out, lout, B * V * 4, hipMemcpyDeviceToHost, stream_));
        if (state_out) HIP_OK(hipMemcpyAsync(state_out, sout, B * n * 4, hipMemcpyDeviceToHost, stream_));
        HIP_OK(hipStreamSynchronize(stream_));
        return handoff_check();
    }
    return true;
}

void Engine::drop_batch_graphs() {
    for (BatchGraph & g : bgraphs_) (void)hipGraphExecDestroy(g.ge);
    bgraphs_.clear();
}

void Engine::free_slots() {
    static_cast<GenSlots &>(*this) = GenSlots{};
    gslots_ = 0;
    gvalid_.clear();
}

bool GenSlots::alloc(size_t n_slots, size_t state_len, size_t n_vocab, size_t batch_max) {
    if (!gstates_.alloc((2 * n_slots + 1) * state_len)) return false;
    gstate_[0] = gstates_;
    gstate_[1] = gstates_ + n_slots * state_len;
    gfresh_ = gstates_ + 2 * n_slots * state_len;
    if (!(gsnap_state_.alloc(n_slots * state_len) && glogits_.alloc(n_slots * n_vocab) &&
          gsnap_logits_.alloc(n_slots * n_vocab) && gcounts_.alloc(n_slots * n_vocab) && gparams_.alloc(4 * batch_max) &&
          gstreams_.alloc(2 * batch_max) && gwords_.alloc(GenWords().bind(nullptr, batch_max))))
        return false;
    gw_.bind(gwords_, batch_max);
    return true;
}

bool Engine::batch_reserve(size_t n_slots) {
    HIP_OK(hipSetDevice(m_->device));
    if (n_slots > (size_t)kBatchMax) return false;
    if (!settle(GRAPHS_BATCH)) return false;  // they hold the old slots' addresses
    free_slots();
    if (n_slots == 0) return true;
    GenSlots gs;
    if (!gs.alloc(n_slots, m_->state_len, m_->n_vocab, (size_t)kBatchMax) ||
        hipMemsetAsync(gs.gwords_, 0, gs.gwords_.size() * 4, stream_) != hipSuccess || !init_state(gs.gfresh_)) {
        (void)hipGetLastError();
        fprintf(stderr, "rwkv: allocation of %zu generation slots failed\n", n_slots);
        return false;
    }
    static_cast<GenSlots &>(*this) = std::move(gs);
    gslots_ = n_slots;
    gvalid_.assign(n_slots, 0);
    return true;
}

bool Engine::batch_store(size_t slot) {
    HIP_OK(hipSetDevice(m_->device));
    if (slot >= gslots_ || !logits_valid_) return false;
    const size_t n = m_->state_len, V = m_->n_vocab;
    gvalid_[slot] = 0;
    HIP_OK(hipMemcpyAsync(gstate_[0] + slot * n, dstate_[cur_], n * 4, hipMemcpyDeviceToDevice, stream_));
    HIP_OK(hipMemcpyAsync(glogits_ + slot * V, logits_, V * 4, hipMemcpyDeviceToDevice, stream_));
    // a new sequence in the slot: no token counted yet, not finished
    HIP_OK(hipMemsetAsync(gcounts_ + slot * V, 0, V * 4, stream_));
    HIP_OK(hipMemsetAsync(gw_.done + slot, 0, 4, stream_));
    gvalid_[slot] = 1;
    return true;
}

bool Engine::batch_load(size_t slot) {
    HIP_OK(hipSetDevice(m_->device));
    if (!batch_slot_valid(slot)) return false;
    const size_t n = m_->state_len, V = m_->n_vocab;
    logits_valid_ = false;
    HIP_OK(hipMemcpyAsync(dstate_[cur_], gstate_[0] + slot * n, n * 4, hipMemcpyDeviceToDevice, stream_));
    HIP_OK(hipMemcpyAsync(logits_, glogits_ + slot * V, V * 4, hipMemcpyDeviceToDevice, stream_));
    logits_valid_ = true;
    return true;
}

bool Engine::slots_fail(size_t n, const uint32_t * slots) {
    (void)hipStreamSynchronize(stream_);
    (void)handoff_check();
    for (size_t i = 0; i < n; i++) gvalid_[slots ? slots[i] : i] = 0;
    return false;
}

bool Engine::gen_upload(size_t Q, const BatchSamplingParams & p, size_t n) {
    const size_t K = (size_t)kBatchMax;
    gparams_h_.assign(4 * K, 0.0f);
    gstreams_h_.assign(2 * K, 0);
    for (size_t s = 0; s < Q; s++) {
        gparams_h_[s] = p.temperature[s];
        gparams_h_[K + s] = p.top_p[s];
        gparams_h_[2 * K + s] = p.presence ? p.presence[s] : 0.0f;
        gparams_h_[3 * K + s] = p.frequency ? p.frequency[s] : 0.0f;
        gstreams_h_[s] = p.seed[s];
        gstreams_h_[K + s] = p.offset[s];
    }
    return hipMemcpyAsync(gparams_, gparams_h_.data(), 4 * K * 4, hipMemcpyHostToDevice, stream_) == hipSuccess &&
           hipMemcpyAsync(gstreams_, gstreams_h_.data(), 2 * K * 8, hipMemcpyHostToDevice, stream_) == hipSuccess &&
           hipMemsetAsync(gtokens_, 0xff, Q * n * 4, stream_) == hipSuccess;
}

SampleArgs Engine::gen_sample_args(size_t rows, const BatchSamplingParams & p, size_t n) {
    const size_t K = (size_t)kBatchMax;
    SampleArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = glogits_;
    a.rows = (int)rows;
    a.V = (int)m_->n_vocab;
    a.n_bias = (int)p.n_bias;
    a.bias_ids = bias_ids_;
    a.bias_vals = bias_vals_;
    a.temperature_r = gparams_;
    a.top_p_r = gparams_ + K;
    a.presence_r = gparams_ + 2 * K;
    a.frequency_r = gparams_ + 3 * K;
    a.counts = gcounts_;
    a.seed_r = gstreams_;
    a.counter_r = gstreams_ + K;
    a.n_stop = (int)p.n_stop;
    for (uint32_t j = 0; j < p.n_stop; j++) a.stop[j] = p.stop_tokens[j];
    a.done = gw_.done;
    a.length = gw_.length;
    a.fin_step = gw_.fin_step;
    a.active = gw_.active;
    a.tok = gtokens_;
    a.tok_stride = (uint32_t)n;
    a.tok2 = dtokens_;
    return a;
}

bool Engine::generate_batch(size_t B, const BatchSamplingParams & p, size_t n, uint32_t * tokens_out,
                            uint32_t * lengths_out, uint32_t * steps_out, const LogprobsOut * lp) {
    return generate_slots(B, p, n, tokens_out, lengths_out, steps_out, lp, nullptr);
}

bool Engine::generate_queue(size_t Q, size_t lanes, const BatchSamplingParams & p, const uint32_t * max_tokens, size_t n,
                            uint32_t * tokens_out, uint32_t * lengths_out, uint32_t * lane_out, uint32_t * start_out,
                            uint32_t * steps_out, const LogprobsOut * lp) {
    const QueueCall qc{lanes, max_tokens, lane_out, start_out};
    return generate_slots(Q, p, n, tokens_out, lengths_out, steps_out, lp, &qc);
}

// The driver of both calls.  Per step one sampler launch over the rows' logits (per-sequence
// parameters, penalties, stops), k_gen_snapshot of the rows that just stopped, and one batched decode
// step (eval_batch, tokens already in dtokens_) from gstate_[p] to gstate_[p ^ 1].  A finished row
// keeps being decoded on token 0 -- the batched kernels take row t's state at t * state_len, so
// leaving a row out would need a per-row offset through every one of them -- and its live state and
// logits are garbage from then on; what the caller sees is the snapshot, which k_gen_restore puts
// back into gstate_[0] / glogits_ at the end of the call.
// Batch (qc == NULL): row r is sequence r throughout, no table (lane_seq == NULL), Q rows, n steps.
// Queue: the rows are L = min(lanes, Q) lanes, and what changes between two steps is which sequence
// a lane holds.  Sequence s waits in its slot (row s of gstate_[0] / glogits_, s >= L: a step over L
// lanes writes rows [0, L) of the state buffers and of glogits_ only), runs in a lane, and ends in its
// snapshot (row s of gsnap_*), taken by k_gen_snapshot at a stop and by k_gen_move at its cap.
// done[s] == 1 from then on, so the restore needs no table.  What the queue adds is under `qc`.
bool Engine::generate_slots(size_t Q, const BatchSamplingParams & p, size_t n, uint32_t * tokens_out, uint32_t * lengths_out,
                            uint32_t * steps_out, const LogprobsOut * lp, const QueueCall * qc) {
    HIP_OK(hipSetDevice(m_->device));
    // ---- the arguments; the per-sequence values of p are the caller's to check (BatchSamplingParams)
    if (Q == 0 || Q > gslots_ || n == 0 || !tokens_out || !lengths_out || !p.temperature || !p.top_p || !p.seed ||
        !p.offset || p.n_bias > (uint32_t)SAMPLE_MAX_BIAS || p.n_stop > (uint32_t)SAMPLE_MAX_STOP)
        return false;
    for (size_t s = 0; s < Q; s++)
        if (!gvalid_[s]) return false;
    size_t rows = Q, bound = n;
    if (qc) {
        if (qc->lanes == 0 || qc->lanes > (size_t)kBatchMax || !qc->max_tokens || p.keep_counts) return false;
        size_t total = 0, longest = 0;
        for (size_t s = 0; s < Q; s++) {
            const size_t cap = qc->max_tokens[s];
            if (cap == 0 || cap > n) return false;
            total += cap;
            longest = std::max(longest, cap);
        }
        rows = std::min(qc->lanes, Q);
        // list scheduling ends within sum / L + max steps (Graham), whatever the lengths drawn
        bound = (total + rows - 1) / rows + longest;
    }
    const size_t S = m_->state_len, V = m_->n_vocab;
    // ---- everything that allocates, before anything is enqueued: dtokens_ moves when the workspace
    // grows (and the batch graphs are dropped with it), the token buffer grows with Q * n
    if (!ensure_workspace((int)rows) || (lp && !lp_reserve(Q, n, lp->top_k))) return false;
    if (!grow(gtokens_, Q * n, doubled(1024, Q * n), GRAPHS_NONE) || !upload_bias(p.n_bias, p.bias_ids, p.bias_values))
        return false;
    // from here on a failure leaves the slots of the call undefined
    auto fail = [&] { return slots_fail(Q); };

    // ---- the start of the call: uploads and fills that do not depend on one another
    SampleArgs a = gen_sample_args(rows, p, n);
    bool ok = gen_upload(Q, p, n) && (p.keep_counts || hipMemsetAsync(gcounts_, 0, Q * V * 4, stream_) == hipSuccess);
    // the queue's argument block, in the order of GenQueue's members (launched under qc only)
    const GenQueue q{(int)rows,  (int)Q,    gw_.lane_seq,  gw_.done,       gw_.length, gw_.max_tokens,
                     gw_.lane,   gw_.start, gw_.retire_to, gw_.admit_from, gw_.next,   gw_.active};
    if (qc) {
        a.lane_seq = gw_.lane_seq;
        a.max_tokens = gw_.max_tokens;
        gqueue_h_.assign(qc->max_tokens, qc->max_tokens + Q);
        // every lane idle, nothing admitted, the first waiting sequence is 0: GEN_NONE in lane_seq, lane,
        // start, retire_to and admit_from, the arrays from lane_seq up to next (GenWords::bind)
        ok = ok && hipMemcpyAsync(gw_.max_tokens, gqueue_h_.data(), Q * 4, hipMemcpyHostToDevice, stream_) == hipSuccess &&
             hipMemsetAsync(gw_.lane_seq, 0xff, (size_t)(gw_.next - gw_.lane_seq) * 4, stream_) == hipSuccess &&
             hipMemsetAsync(gw_.next, 0, 4, stream_) == hipSuccess;
    }
    ok = ok && lp_begin(lp, Q, n, a) &&
         launch_gen_begin(stream_, (int)Q, p.keep_counts ? 1 : 0, a.done, a.length, a.fin_step, a.active);
    if (!ok) return fail();
    const GenRows g{(int)rows, S, V, a.done, a.fin_step, a.lane_seq};
    // the queue's turnover and move in front of step `step`, on the live rows that step reads
    auto turnover = [&](size_t step, float * cur) {
        return launch_gen_turnover(stream_, q, (uint32_t)step) &&
               launch_gen_move(stream_, q, S, V, cur, glogits_, gstate_[0], gsnap_state_, gsnap_logits_);
    };

    // ---- the steps
    size_t steps = 0;
    uint32_t live = 1;
    for (size_t i = 0; i < bound && live; i++) {
        float * cur = gstate_[steps & 1];
        // the step is a kernel argument of eager launches between the decode graph's replays; a row
        // without a table draws at counter_r + counter, a lane at counter_r + its sequence's length
        a.counter = i;
        a.step = (uint32_t)i;
        {
            const LaunchTimerScope timed(this, timing_);
            ok = (!qc || turnover(i, cur)) && (!lp || launch_logprobs(stream_, a)) && launch_sample(stream_, a) &&
                 launch_gen_snapshot(stream_, g, (uint32_t)i, cur, glogits_, gsnap_state_, gsnap_logits_);
        }
        ok = ok && eval_batch(nullptr, rows, cur, gstate_[(steps & 1) ^ 1], glogits_, true);
        if (!ok) return fail();
        steps++;
        if (p.check_every && (i + 1) % p.check_every == 0 && i + 1 < bound &&
            (hipMemcpyAsync(&live, a.active, 4, hipMemcpyDeviceToHost, stream_) != hipSuccess ||
             hipStreamSynchronize(stream_) != hipSuccess))
            return fail();
    }

    // ---- the end.  Queue: every sequence has ended; those whose cap ended them at the last step are
    // still in their lanes, and one more turnover and move takes them out: every row is then a
    // snapshot, restored in place.  Batch: a live row's state is in the buffer the last step wrote.
    ok = !qc || turnover(steps, gstate_[steps & 1]);
    const GenRows all{(int)Q, S, V, a.done, a.fin_step};
    ok = ok && launch_gen_restore(stream_, all, gsnap_state_, gsnap_logits_, qc ? gstate_[0] : gstate_[steps & 1], gstate_[0],
                                  glogits_);
    // [Q][n] tokens with the rows n apart, as the caller's
    ok = ok && hipMemcpyAsync(tokens_out, gtokens_, Q * n * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
         hipMemcpyAsync(lengths_out, a.length, Q * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess;
    uint32_t * start_h = nullptr;
    if (qc) {
        gqueue_h_.assign(2 * Q, 0);
        start_h = gqueue_h_.data() + Q;
        ok = ok &&
             hipMemcpyAsync(qc->lane_out ? qc->lane_out : gqueue_h_.data(), gw_.lane, Q * 4, hipMemcpyDeviceToHost, stream_) ==
                 hipSuccess &&
             hipMemcpyAsync(start_h, gw_.start, Q * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess;
    }
    ok = ok && lp_copy_out(lp, Q, n);
    if (!ok || hipStreamSynchronize(stream_) != hipSuccess || !handoff_check()) return fail();
    size_t used = steps;
    if (qc) {
        // the steps up to the one after which nothing was busy; the loop may have run more of them
        // (check_every looks only now and then), all on token 0 in idle lanes
        used = 0;
        for (size_t s = 0; s < Q; s++) used = std::max<size_t>(used, (size_t)start_h[s] + lengths_out[s]);
        if (used > steps) return fail();  // a sequence that never ended: the bound does not allow it
        if (qc->start_out) memcpy(qc->start_out, start_h, Q * 4);
    }
    if (steps_out) *steps_out = (uint32_t)used;
    return true;
}

}  // namespace rwkvmi
