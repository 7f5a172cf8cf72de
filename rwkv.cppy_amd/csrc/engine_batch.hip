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
    // the batched forward: bs_ / head_out_ are set only while it is being enqueued
    auto step = [&] {
        bs_ = n;
        head_out_ = lout;
        const bool ok = forward_range((int)B, sin, sout, 0, m_->n_layer, lg);
        bs_ = 0;
        head_out_ = nullptr;
        return ok;
    };
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

// Slots [0, B) of the context generate together: per step one k_sample_rows launch over the slots'
// logits (per-row parameters, penalties, stops), k_gen_snapshot of the rows that just stopped, and
// one batched decode step (eval_batch, tokens already in dtokens_) from gstate_[p] to gstate_[p ^ 1].
// A finished row keeps being decoded on token 0 -- the batched kernels take row t's state at
// t * state_len, so leaving a row out would need a per-row offset through every one of them -- and
// its live state and logits are garbage from then on; what the caller sees is the snapshot, which
// k_gen_restore puts back into gstate_[0] / glogits_ at the end of the call.
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
    return gsnap_state_.alloc(n_slots * state_len) && glogits_.alloc(n_slots * n_vocab) &&
           gsnap_logits_.alloc(n_slots * n_vocab) && gcounts_.alloc(n_slots * n_vocab) && gparams_.alloc(4 * batch_max) &&
           gstreams_.alloc(2 * batch_max) && gwords_.alloc(kWordRows * batch_max + 2);
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
    HIP_OK(hipMemsetAsync(gwords_ + slot, 0, 4, stream_));
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

bool Engine::gen_upload(size_t rows, const BatchSamplingParams & p, size_t n) {
    const size_t K = (size_t)kBatchMax;
    gparams_h_.assign(4 * K, 0.0f);
    gstreams_h_.assign(2 * K, 0);
    for (size_t r = 0; r < rows; r++) {
        gparams_h_[r] = p.temperature[r];
        gparams_h_[K + r] = p.top_p[r];
        gparams_h_[2 * K + r] = p.presence ? p.presence[r] : 0.0f;
        gparams_h_[3 * K + r] = p.frequency ? p.frequency[r] : 0.0f;
        gstreams_h_[r] = p.seed[r];
        gstreams_h_[K + r] = p.offset[r];
    }
    return hipMemcpyAsync(gparams_, gparams_h_.data(), 4 * K * 4, hipMemcpyHostToDevice, stream_) == hipSuccess &&
           hipMemcpyAsync(gstreams_, gstreams_h_.data(), 2 * K * 8, hipMemcpyHostToDevice, stream_) == hipSuccess &&
           hipMemsetAsync(gtokens_, 0xff, rows * n * 4, stream_) == hipSuccess;
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
    a.done = gwords_;
    a.length = gwords_ + K;
    a.fin_step = gwords_ + 2 * K;
    a.active = gwords_ + 3 * K;
    a.tok = gtokens_;
    a.tok_stride = (uint32_t)n;
    a.tok2 = dtokens_;
    return a;
}

bool Engine::gen_fail(size_t rows) {
    (void)hipStreamSynchronize(stream_);
    (void)handoff_check();
    for (size_t r = 0; r < rows; r++) gvalid_[r] = 0;
    return false;
}

bool Engine::generate_batch(size_t B, const BatchSamplingParams & p, size_t n, uint32_t * tokens_out,
                            uint32_t * lengths_out, uint32_t * steps_out, const LogprobsOut * lp) {
    HIP_OK(hipSetDevice(m_->device));
    if (B == 0 || B > gslots_ || n == 0 || !tokens_out || !lengths_out || !p.temperature || !p.top_p || !p.seed ||
        !p.offset || p.n_bias > (uint32_t)SAMPLE_MAX_BIAS || p.n_stop > (uint32_t)SAMPLE_MAX_STOP)
        return false;
    for (size_t r = 0; r < B; r++)
        if (!gvalid_[r]) return false;
    const size_t S = m_->state_len, V = m_->n_vocab;
    // everything that allocates, before anything is enqueued: dtokens_ moves when the workspace
    // grows (and the batch graphs are dropped with it), the token buffer grows with B * n
    if (!ensure_workspace((int)B) || (lp && !lp_reserve(B, n, lp->top_k))) return false;
    if (!grow(gtokens_, B * n, doubled(1024, B * n), GRAPHS_NONE) || !upload_bias(p.n_bias, p.bias_ids, p.bias_values))
        return false;
    // from here on a failure leaves the slots of the call undefined
    auto fail = [&] { return gen_fail(B); };
    bool ok = gen_upload(B, p, n);
    if (ok && !p.keep_counts) ok = hipMemsetAsync(gcounts_, 0, B * V * 4, stream_) == hipSuccess;
    SampleArgs a = gen_sample_args(B, p, n);
    ok = ok && lp_begin(lp, B, n, a);
    ok = ok && launch_gen_begin(stream_, (int)B, p.keep_counts ? 1 : 0, a.done, a.length, a.fin_step, a.active);
    if (!ok) return fail();
    GenRows g{(int)B, S, V, a.done, a.fin_step};

    size_t steps = 0;
    uint32_t live = 1;
    for (size_t i = 0; ok && i < n && live; i++) {
        // the step is a kernel argument of eager launches between the decode graph's replays
        a.counter = i;
        a.step = (uint32_t)i;
        if (timing_) g_klt = this;
        ok = (!lp || launch_logprobs(stream_, a)) && launch_sample(stream_, a) &&
             launch_gen_snapshot(stream_, g, (uint32_t)i, gstate_[steps & 1], glogits_, gsnap_state_, gsnap_logits_);
        g_klt = nullptr;
        ok = ok && eval_batch(nullptr, B, gstate_[steps & 1], gstate_[(steps & 1) ^ 1], glogits_, true);
        if (!ok) break;
        steps++;
        if (p.check_every && (i + 1) % p.check_every == 0 && i + 1 < n) {
            ok = hipMemcpyAsync(&live, a.active, 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
                 hipStreamSynchronize(stream_) == hipSuccess;
        }
    }
    if (!ok) return fail();
    ok = launch_gen_restore(stream_, g, gsnap_state_, gsnap_logits_, gstate_[steps & 1], gstate_[0], glogits_);
    // [B][n] tokens with the rows n apart, as the caller's
    ok = ok && hipMemcpyAsync(tokens_out, gtokens_, B * n * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
         hipMemcpyAsync(lengths_out, a.length, B * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
         lp_copy_out(lp, B, n);
    if (!ok) return fail();
    if (hipStreamSynchronize(stream_) != hipSuccess) return fail();
    if (!handoff_check()) {
        for (size_t r = 0; r < B; r++) gvalid_[r] = 0;
        return false;
    }
    if (steps_out) *steps_out = (uint32_t)steps;
    return true;
}

// The queue.  Lanes [0, L) are the rows of the batched step, densely, as in generate_batch; what
// changes between two steps is which sequence a lane holds.  Sequence s waits in its slot (row s of
// gstate_[0] / glogits_, s >= L: a step over L lanes writes rows [0, L) of the state buffers and of
// glogits_ only), runs in a lane, and ends in its snapshot (row s of gsnap_*), taken by
// k_gen_snapshot at a stop and by k_gen_move at its cap; k_gen_restore puts every snapshot into its
// slot at the end.  done[s] == 1 from then on, so the restore needs no table.
bool Engine::generate_queue(size_t Q, size_t lanes, const BatchSamplingParams & p, const uint32_t * max_tokens, size_t n,
                            uint32_t * tokens_out, uint32_t * lengths_out, uint32_t * lane_out, uint32_t * start_out,
                            uint32_t * steps_out, const LogprobsOut * lp) {
    HIP_OK(hipSetDevice(m_->device));
    const size_t K = (size_t)kBatchMax;
    if (Q == 0 || Q > gslots_ || lanes == 0 || lanes > K || n == 0 || !max_tokens || !tokens_out || !lengths_out ||
        !p.temperature || !p.top_p || !p.seed || !p.offset || p.keep_counts || p.n_bias > (uint32_t)SAMPLE_MAX_BIAS ||
        p.n_stop > (uint32_t)SAMPLE_MAX_STOP)
        return false;
    size_t total = 0, longest = 0;
    for (size_t s = 0; s < Q; s++) {
        if (!gvalid_[s] || max_tokens[s] == 0 || max_tokens[s] > n) return false;
        total += max_tokens[s];
        longest = std::max<size_t>(longest, max_tokens[s]);
    }
    const size_t L = std::min(lanes, Q), S = m_->state_len, V = m_->n_vocab;
    // list scheduling ends within sum / L + max steps (Graham), whatever the lengths drawn
    const size_t bound = (total + L - 1) / L + longest;
    if (!ensure_workspace((int)L) || (lp && !lp_reserve(Q, n, lp->top_k))) return false;
    if (!grow(gtokens_, Q * n, doubled(1024, Q * n), GRAPHS_NONE) || !upload_bias(p.n_bias, p.bias_ids, p.bias_values))
        return false;
    auto fail = [&] { return gen_fail(Q); };
    gqueue_h_.assign(max_tokens, max_tokens + Q);
    SampleArgs a = gen_sample_args(L, p, n);
    GenQueue q;
    q.lanes = (int)L;
    q.Q = (int)Q;
    q.done = a.done;
    q.length = a.length;
    q.active = a.active;
    uint32_t * w = gwords_ + 3 * K + 1;
    uint32_t * maxtok = w;
    q.max_tokens = maxtok;
    q.lane_seq = w + K;
    q.lane = w + 2 * K;
    q.start = w + 3 * K;
    q.retire_to = w + 4 * K;
    q.admit_from = w + 5 * K;
    q.next = w + 6 * K;
    a.lane_seq = q.lane_seq;
    a.max_tokens = q.max_tokens;
    // every lane idle, nothing admitted, the first waiting sequence is 0
    bool ok = gen_upload(Q, p, n) && hipMemsetAsync(gcounts_, 0, Q * V * 4, stream_) == hipSuccess &&
              hipMemcpyAsync(maxtok, gqueue_h_.data(), Q * 4, hipMemcpyHostToDevice, stream_) == hipSuccess &&
              hipMemsetAsync(q.lane_seq, 0xff, 5 * K * 4, stream_) == hipSuccess &&
              hipMemsetAsync(q.next, 0, 4, stream_) == hipSuccess &&
              launch_gen_begin(stream_, (int)Q, 0, a.done, a.length, a.fin_step, a.active) && lp_begin(lp, Q, n, a);
    if (!ok) return fail();
    GenRows g{(int)L, S, V, a.done, a.fin_step, q.lane_seq};

    size_t steps = 0;
    uint32_t live = 1;
    for (size_t i = 0; ok && i < bound && live; i++) {
        float * cur = gstate_[steps & 1];
        a.step = (uint32_t)i;
        if (timing_) g_klt = this;
        ok = launch_gen_turnover(stream_, q, (uint32_t)i) &&
             launch_gen_move(stream_, q, S, V, cur, glogits_, gstate_[0], gsnap_state_, gsnap_logits_) &&
             (!lp || launch_logprobs(stream_, a)) && launch_sample(stream_, a) &&
             launch_gen_snapshot(stream_, g, (uint32_t)i, cur, glogits_, gsnap_state_, gsnap_logits_);
        g_klt = nullptr;
        ok = ok && eval_batch(nullptr, L, cur, gstate_[(steps & 1) ^ 1], glogits_, true);
        if (!ok) break;
        steps++;
        if (p.check_every && (i + 1) % p.check_every == 0 && i + 1 < bound) {
            ok = hipMemcpyAsync(&live, a.active, 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
                 hipStreamSynchronize(stream_) == hipSuccess;
        }
    }
    if (!ok) return fail();
    // every sequence has ended; those whose cap ended them at the last step are still in their lanes
    ok = launch_gen_turnover(stream_, q, (uint32_t)steps) &&
         launch_gen_move(stream_, q, S, V, gstate_[steps & 1], glogits_, gstate_[0], gsnap_state_, gsnap_logits_);
    GenRows all{(int)Q, S, V, a.done, a.fin_step};
    ok = ok && launch_gen_restore(stream_, all, gsnap_state_, gsnap_logits_, gstate_[0], gstate_[0], glogits_);
    gqueue_h_.assign(2 * Q, 0);
    uint32_t * lane_h = lane_out ? lane_out : gqueue_h_.data();
    uint32_t * start_h = gqueue_h_.data() + Q;
    ok = ok && hipMemcpyAsync(tokens_out, gtokens_, Q * n * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
         hipMemcpyAsync(lengths_out, a.length, Q * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
         hipMemcpyAsync(lane_h, q.lane, Q * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
         hipMemcpyAsync(start_h, q.start, Q * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
         lp_copy_out(lp, Q, n);
    if (!ok) return fail();
    if (hipStreamSynchronize(stream_) != hipSuccess) return fail();
    if (!handoff_check()) {
        for (size_t s = 0; s < Q; s++) gvalid_[s] = 0;
        return false;
    }
    // the steps up to the one after which nothing was busy; the loop may have run more of them
    // (check_every looks only now and then), all on token 0 in idle lanes
    size_t used = 0;
    for (size_t s = 0; s < Q; s++) used = std::max<size_t>(used, (size_t)start_h[s] + lengths_out[s]);
    if (used > steps) return fail();  // a sequence that never ended: the bound does not allow it
    if (start_out) memcpy(start_out, start_h, Q * 4);
    if (steps_out) *steps_out = (uint32_t)used;
    return true;
}

}  // namespace rwkvmi
