// engine_generate.hip -- token sampling, the device-resident generation loop and sequence scoring
// on the context's own state.
#include <stdio.h>
#include <string.h>

#include "engine.hpp"
#include "kernels.hpp"

namespace rwkvmi {

// The sampler's device buffers, allocated or grown before anything is enqueued (never inside the
// loop): n token slots and the bias arrays, which are uploaded in stream order.
bool Engine::sampler_buffers(const SamplingParams & p, size_t n, SampleArgs & a) {
    if (p.n_bias > (uint32_t)SAMPLE_MAX_BIAS) return false;
    if (!grow(gen_tokens_, n, doubled(64, n), GRAPHS_NONE) || !upload_bias(p.n_bias, p.bias_ids, p.bias_values))
        return false;
    memset(&a, 0, sizeof(a));
    a.logits = logits_;
    a.rows = 1;
    a.V = (int)m_->n_vocab;
    a.temperature = p.temperature;
    a.top_p = p.top_p;
    a.n_bias = (int)p.n_bias;
    a.bias_ids = bias_ids_;
    a.bias_vals = bias_vals_;
    a.seed = p.seed;
    a.counter = p.offset;
    a.tok = gen_tokens_;
    return true;
}

bool Engine::upload_bias(uint32_t n_bias, const uint32_t * ids, const float * values) {
    if (!grow(bias_ids_, SAMPLE_MAX_BIAS, SAMPLE_MAX_BIAS, GRAPHS_NONE) ||
        !grow(bias_vals_, SAMPLE_MAX_BIAS, SAMPLE_MAX_BIAS, GRAPHS_NONE))
        return false;
    if (n_bias) {
        HIP_OK(hipMemcpyAsync(bias_ids_, ids, n_bias * 4, hipMemcpyHostToDevice, stream_));
        HIP_OK(hipMemcpyAsync(bias_vals_, values, n_bias * 4, hipMemcpyHostToDevice, stream_));
    }
    return true;
}

bool Engine::lp_reserve(size_t rows, size_t n, uint32_t top_k) {
    HIP_OK(hipSetDevice(m_->device));
    const size_t cols = rows * n, tops = cols * top_k;
    return grow(lp_token_, cols, doubled(1024, cols), GRAPHS_NONE) && grow(lp_top_, tops, doubled(1024, tops), GRAPHS_NONE) &&
           grow(lp_ids_, tops, doubled(1024, tops), GRAPHS_NONE) &&
           grow(lp_logz_, (size_t)kBatchMax, (size_t)kBatchMax, GRAPHS_NONE);
}

bool Engine::lp_begin(const LogprobsOut * lp, size_t rows, size_t n, SampleArgs & a) {
    if (!lp) return true;
    if (lp->top_k > (uint32_t)LOGPROBS_MAX_TOP || lp->top_k > m_->n_vocab || !lp->token_logprob ||
        (lp->top_k && (!lp->top_ids || !lp->top_logprobs)) || !lp_reserve(rows, n, lp->top_k))
        return false;
    const size_t cols = rows * n, tops = cols * lp->top_k;
    // one fill per array: 0xFFFFFFFF ids, NaN doubles
    HIP_OK(hipMemsetAsync(lp_token_, 0xff, cols * 8, stream_));
    if (tops) {
        HIP_OK(hipMemsetAsync(lp_top_, 0xff, tops * 8, stream_));
        HIP_OK(hipMemsetAsync(lp_ids_, 0xff, tops * 4, stream_));
    }
    a.lp_logz = lp_logz_;
    a.lp_token = lp_token_;
    a.lp_top_ids = lp_ids_;
    a.lp_top = lp_top_;
    a.lp_k = (int)lp->top_k;
    return true;
}

bool Engine::lp_copy_out(const LogprobsOut * lp, size_t rows, size_t n) {
    if (!lp) return true;
    const size_t cols = rows * n, tops = cols * lp->top_k;
    HIP_OK(hipMemcpyAsync(lp->token_logprob, lp_token_, cols * 8, hipMemcpyDeviceToHost, stream_));
    if (tops) {
        HIP_OK(hipMemcpyAsync(lp->top_ids, lp_ids_, tops * 4, hipMemcpyDeviceToHost, stream_));
        HIP_OK(hipMemcpyAsync(lp->top_logprobs, lp_top_, tops * 8, hipMemcpyDeviceToHost, stream_));
    }
    return true;
}

bool Engine::filters_begin(const FilterParams * f, size_t rows, bool upload, SampleFilters & sf) {
    memset(&sf, 0, sizeof(sf));
    if (!f) return true;
    const size_t K = (size_t)kBatchMax;
    if (rows > K || (!upload && rows != 1)) return false;
    gfilters_h_.assign(3 * K, 0);
    bool on = false;
    for (size_t r = 0; r < rows; r++) {
        const uint32_t k = f->top_k && f->top_k[r] < m_->n_vocab ? f->top_k[r] : 0u;
        const float q = f->min_p ? f->min_p[r] : 0.0f;
        const float t = f->typical_p && f->typical_p[r] < 1.0f ? f->typical_p[r] : 0.0f;
        gfilters_h_[r] = k;
        memcpy(&gfilters_h_[K + r], &q, 4);
        memcpy(&gfilters_h_[2 * K + r], &t, 4);
        on = on || k != 0u || q != 0.0f || t != 0.0f;
    }
    if (!on) return true;
    if (!upload) {
        sf.top_k = gfilters_h_[0];
        memcpy(&sf.min_p, &gfilters_h_[K], 4);
        memcpy(&sf.typical_p, &gfilters_h_[2 * K], 4);
        return true;
    }
    HIP_OK(hipMemcpyAsync(gfilters_, gfilters_h_.data(), 3 * K * 4, hipMemcpyHostToDevice, stream_));
    sf.top_k_r = gfilters_;
    sf.min_p_r = (const float *)(gfilters_ + K);
    sf.typical_p_r = (const float *)(gfilters_ + 2 * K);
    return true;
}

int Engine::vocab_bytes(const uint32_t * offsets, const uint8_t * bytes) {
    if (hipSetDevice(m_->device) != hipSuccess) return 2;
    std::vector<uint8_t> head, tail;
    std::vector<uint32_t> meta;
    if (!dfa_pack_vocab(offsets, bytes, m_->n_vocab, head, meta, tail)) return 1;
    // queued work of this context may still read the old copy
    if (hipStreamSynchronize(stream_) != hipSuccess) return 2;
    DevBuf<uint8_t> dh, dt;
    DevBuf<uint32_t> dm;
    if (!dh.alloc(head.size()) || !dt.alloc(tail.size()) || !dm.alloc(meta.size())) return 2;
    if (hipMemcpy(dh, head.data(), head.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dm, meta.data(), meta.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        (!tail.empty() && hipMemcpy(dt, tail.data(), tail.size(), hipMemcpyHostToDevice) != hipSuccess))
        return 2;
    m_->vocab_head = std::move(dh);
    m_->vocab_tail = std::move(dt);
    m_->vocab_meta = std::move(dm);
    // the tokenizer's trie is rebuilt from these on its next call
    m_->vocab_offsets_h.assign(offsets, offsets + m_->n_vocab + 1);
    m_->vocab_bytes_h.assign(bytes, bytes + offsets[m_->n_vocab]);
    m_->tok_trie.reset();
    m_->tok_state = DeviceModel::TOK_UNBUILT;
    return 0;
}

int Engine::constraint_table(uint32_t n_states, const uint16_t * next, const uint8_t * accepting) {
    if (hipSetDevice(m_->device) != hipSuccess) return 2;
    DfaTable t;
    DevBuf<uint8_t> blob, accept;
    if (n_states != 0) {
        if (!next || !accepting || !dfa_compress(next, n_states, t)) return 1;
        if (!blob.alloc(t.blob.size()) || !accept.alloc(n_states)) return 2;
        if (hipMemcpy(blob, t.blob.data(), t.blob.size(), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(accept, accepting, n_states, hipMemcpyHostToDevice) != hipSuccess)
            return 2;
    }
    // queued work of this context may still read the old table
    if (hipStreamSynchronize(stream_) != hipSuccess) return 2;
    res_blob_ = std::move(blob);
    res_accept_ = std::move(accept);
    res_states_ = n_states;
    res_cls_ = n_states ? t.n_cls : 0;
    return 0;
}

int Engine::constraint_reserve(const ConstraintParams & c, size_t Q, size_t rows) {
    if (hipSetDevice(m_->device) != hipSuccess) return 2;
    const size_t K = (size_t)kBatchMax, V = m_->n_vocab;
    dfa_resident_ = !c.next && !c.accepting;
    if (!m_->vocab_head.get() || (!dfa_resident_ && (!c.next || !c.accepting)) || !c.state || Q == 0 || Q > K || rows == 0 || rows > Q)
        return 1;
    if (dfa_resident_) {
        if (res_states_ == 0 || c.n_states != res_states_) return 1;
    } else if (!dfa_compress(c.next, c.n_states, dfa_tab_)) {
        return 1;
    }
    for (size_t s = 0; s < Q; s++)
        if (c.state[s] >= c.n_states) return 1;
    const size_t tile = rows * V;
    if (!dfa_resident_) {
        if (dfa_lds_bytes(dfa_tab_.n_states, dfa_tab_.n_cls) > constraint_lds_limit()) return 1;
        const size_t blob = dfa_tab_.blob.size();
        if (!grow(dfa_blob_, blob, doubled(4096, blob), GRAPHS_NONE) ||
            !grow(dfa_accept_, c.n_states, doubled(256, c.n_states), GRAPHS_NONE))
            return 2;
    }
    if (!grow(dfa_masked_, tile, doubled(V, tile), GRAPHS_NONE) || !grow(dfa_words_, 3 * K + 3, 3 * K + 3, GRAPHS_NONE) ||
        !grow(dfa_snap_, m_->state_len + V, m_->state_len + V, GRAPHS_NONE))
        return 2;
    return 0;
}

bool Engine::dfa_begin(const ConstraintParams & c, size_t Q, size_t rows, DfaArgs & d) {
    const size_t K = (size_t)kBatchMax;
    if (dfa_resident_ != (!c.next && !c.accepting) || dfa_masked_.size() < rows * m_->n_vocab) return false;
    if (dfa_resident_ ? res_states_ != c.n_states || res_states_ == 0 : dfa_tab_.n_states != c.n_states || dfa_tab_.blob.empty())
        return false;
    dfa_h_.assign(3 * K + 3, 0);
    for (size_t s = 0; s < Q; s++) dfa_h_[s] = c.state[s];
    if (!dfa_resident_) {
        HIP_OK(hipMemcpyAsync(dfa_blob_, dfa_tab_.blob.data(), dfa_tab_.blob.size(), hipMemcpyHostToDevice, stream_));
        HIP_OK(hipMemcpyAsync(dfa_accept_, c.accepting, c.n_states, hipMemcpyHostToDevice, stream_));
    }
    HIP_OK(hipMemcpyAsync(dfa_words_, dfa_h_.data(), (3 * K + 3) * 4, hipMemcpyHostToDevice, stream_));
    memset(&d, 0, sizeof(d));
    d.head = (const uint4 *)m_->vocab_head.get();
    d.meta = (const uint2 *)m_->vocab_meta.get();
    d.tail = m_->vocab_tail;
    d.V = (int)m_->n_vocab;
    d.tab = (const uint16_t *)(dfa_resident_ ? res_blob_ : dfa_blob_).get();
    d.accepting = dfa_resident_ ? res_accept_ : dfa_accept_;
    d.n_states = c.n_states;
    d.n_cls = dfa_resident_ ? res_cls_ : dfa_tab_.n_cls;
    d.rows = (int)rows;
    d.masked = dfa_masked_;
    d.state = dfa_words_;
    d.ended = dfa_words_ + K;
    d.n_allowed = dfa_words_ + 2 * K;
    d.ticket = dfa_words_ + 3 * K;
    // a table passed with the call, or a resident one that fits the LDS: k_dfa_mask; else k_dfa_mask_mem
    dfa_mem_ = dfa_resident_ && dfa_lds_bytes(d.n_states, d.n_cls) > constraint_lds_limit();
    return true;
}

bool Engine::dfa_mask(const DfaArgs & d) {
    return dfa_mem_ ? launch_dfa_mask_mem(stream_, d) : launch_dfa_mask(stream_, d, constraint_lds_limit());
}

bool Engine::dfa_copy_out(const ConstraintParams & c, size_t Q) {
    const size_t K = (size_t)kBatchMax;
    HIP_OK(hipMemcpyAsync(c.state, dfa_words_, Q * 4, hipMemcpyDeviceToHost, stream_));
    if (c.ended) HIP_OK(hipMemcpyAsync(c.ended, dfa_words_ + K, Q * 4, hipMemcpyDeviceToHost, stream_));
    return true;
}

bool Engine::sample(const SamplingParams & p, uint32_t * token_out, const GenExtras & x) {
    const auto [lp, f, c] = x;
    HIP_OK(hipSetDevice(m_->device));
    if (!logits_valid_ || !token_out) return false;
    SampleArgs a;
    SampleFilters sf;
    DfaArgs d{};
    if (lp && !lp_reserve(1, 1, lp->top_k)) return false;
    if (!sampler_buffers(p, 1, a) || !filters_begin(f, 1, false, sf) || !lp_begin(lp, 1, 1, a)) return false;
    if (c) {
        // no draw (no token allowed): the token stays 0xFFFFFFFF
        if (!dfa_begin(*c, 1, 1, d) || hipMemsetAsync(gen_tokens_, 0xff, 4, stream_) != hipSuccess) return false;
        d.logits = a.logits;
        d.done = a.done = dfa_words_ + 3 * (size_t)kBatchMax + 1;
        d.fin_step = a.fin_step = d.done + 1;
        d.tokens = a.tok;
        a.logits = d.masked;
        if (!dfa_mask(d)) return false;
    }
    if (lp && !launch_logprobs(stream_, a)) return false;
    if (!launch_sample(stream_, a, &sf)) return false;
    if (c && !(launch_dfa_advance(stream_, d) && dfa_copy_out(*c, 1))) return false;
    HIP_OK(hipMemcpyAsync(token_out, gen_tokens_, 4, hipMemcpyDeviceToHost, stream_));
    if (!lp_copy_out(lp, 1, 1)) return false;
    HIP_OK(hipStreamSynchronize(stream_));
    return handoff_check();
}

bool Engine::generate(const SamplingParams & p, size_t n, uint32_t * tokens_out, float * logits_out, const GenExtras & x) {
    const auto [lp, f, c] = x;
    HIP_OK(hipSetDevice(m_->device));
    if (!logits_valid_ || !tokens_out || n == 0) return false;
    SampleArgs a;
    SampleFilters sf;
    // dtokens_ moves when the workspace grows (the graphs are dropped with it): settle it first
    if (!ensure_workspace(1) || (lp && !lp_reserve(1, n, lp->top_k)) || !sampler_buffers(p, n, a) ||
        !filters_begin(f, 1, false, sf))
        return false;
    const int cur0 = cur_;
    co_retry_ = false;
    bool ok = lp_begin(lp, 1, n, a);
    const size_t K = lp ? lp->top_k : 0;
    DfaArgs d{};
    DfaSnap snap{};
    const float * const lg = a.logits;
    if (c) {
        // a draw that does not happen (no token allowed) leaves 0xFFFFFFFF, as do the draws after it
        ok = ok && dfa_begin(*c, 1, 1, d) && hipMemsetAsync(gen_tokens_, 0xff, n * 4, stream_) == hipSuccess;
        d.logits = lg;
        d.done = a.done = dfa_words_ + 3 * (size_t)kBatchMax + 1;
        d.fin_step = a.fin_step = d.done + 1;
        d.tokens = dtokens_;
        a.logits = d.masked;
        snap = DfaSnap{nullptr, lg, dfa_snap_, dfa_snap_ + m_->state_len, m_->state_len};
    }
    for (size_t i = 0; ok && i < n; i++) {
        // the counter is a kernel argument of an eager launch between the decode graphs' replays:
        // nothing per step is baked into a captured node
        a.counter = p.offset + i;
        a.tok = gen_tokens_ + i;
        a.tok2 = dtokens_;
        if (lp) {  // column i
            a.lp_token = lp_token_ + i;
            a.lp_top_ids = lp_ids_ + i * K;
            a.lp_top = lp_top_ + i * K;
        }
        {
            const LaunchTimerScope timed(this, timing_);
            if (c) {
                a.step = d.step = (uint32_t)i;
                snap.state_from = dstate_[cur_];
                ok = dfa_mask(d);
            }
            ok = ok && (!lp || launch_logprobs(stream_, a)) && launch_sample(stream_, a, &sf) &&
                 (!c || launch_dfa_advance(stream_, d, &snap));
        }
        ok = ok && run_tokens(nullptr, 1, true);
    }
    if (ok && c) {
        // a sequence that ended without a draw: the state and logits it ended with come back
        uint32_t ended = 0;
        ok = dfa_copy_out(*c, 1) &&
             hipMemcpyAsync(&ended, d.ended, 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
             hipStreamSynchronize(stream_) == hipSuccess;
        if (ok && ended == 2u)
            ok = hipMemcpyAsync(dstate_[cur_], snap.state_to, m_->state_len * 4, hipMemcpyDeviceToDevice, stream_) == hipSuccess &&
                 hipMemcpyAsync(logits_, snap.logits_to, (size_t)m_->n_vocab * 4, hipMemcpyDeviceToDevice, stream_) == hipSuccess;
    }
    if (ok) {
        ok = hipMemcpyAsync(tokens_out, gen_tokens_, n * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess;
        if (ok && logits_out) ok = copy_logits(logits_out);
        ok = ok && lp_copy_out(lp, 1, n);
    }
    ok = (hipStreamSynchronize(stream_) == hipSuccess) && ok;
    ok = handoff_check() && ok;
    if (!ok) {
        // as run_tokens: the parity the call started with; state and logits are unspecified
        cur_ = cur0;
        logits_valid_ = false;
    }
    return ok;
}

// The scorer's device buffers, allocated or grown before anything is enqueued: T targets, losses
// and argmaxes, and (T > 1: some chunk has more than one token) the head tile.
bool Engine::score_buffers(size_t T) {
    const size_t cap = doubled(1024, T);
    if (!grow(score_targets_, T, cap, GRAPHS_NONE) || !grow(score_loss_, T, cap, GRAPHS_NONE) ||
        !grow(score_argmax_, T, cap, GRAPHS_NONE))
        return false;
    const size_t tile = (size_t)kScoreRows * m_->n_vocab;
    if (T > 1 && !grow(score_tile_, tile, tile, GRAPHS_NONE)) return false;
    return true;
}

// After the layers of tokens [done, done + n) of a score() call: x_ holds their n final residual
// rows (n > 1), or the decode program's head has written logits_ (n == 1).
bool Engine::score_chunk(const ScoreRun & score, size_t done, size_t n, bool last) {
    const size_t C = m_->n_embed, V = m_->n_vocab;
    const bool want_loss = score.targets != nullptr;
    if (want_loss)
        HIP_OK(hipMemcpyAsync(score_targets_ + done, score.targets + done, n * 4, hipMemcpyHostToDevice, stream_));
    auto reduce = [&](const float * lg, size_t row0, int rows) {
        const size_t at = done + row0;
        if (!launch_xent(stream_, lg, rows, (int)V, want_loss ? score_targets_ + at : nullptr,
                         want_loss ? score_loss_ + at : nullptr, score_argmax_ + at))
            return false;
        if (score.logits_out) {
            // the next tile (or step) overwrites lg: the copy has landed before it is enqueued
            HIP_OK(hipMemcpyAsync(score.logits_out + at * V, lg, (size_t)rows * V * 4, hipMemcpyDeviceToHost, stream_));
            HIP_OK(hipStreamSynchronize(stream_));
        }
        return true;
    };
    if (n == 1) return reduce(logits_, 0, 1);
    for (size_t row0 = 0; row0 < n; row0 += (size_t)kScoreRows) {
        const int rows = (int)std::min(n - row0, (size_t)kScoreRows);
        // the head over `rows` rows as batched decode runs it over that many contexts (mm_dispatch:
        // k_fmm, k_mvb or k_mm, each row the bits of its one-token head); never the sequence GEMM,
        // for which the head has no tile records (upload_mat)
        if (!head_rows(rows_run(rows, 0, nullptr, nullptr, score_tile_), x_ + row0 * C) || !reduce(score_tile_, row0, rows))
            return false;
        if (last && row0 + rows == n)
            HIP_OK(hipMemcpyAsync(logits_, score_tile_ + (size_t)(rows - 1) * V, V * 4, hipMemcpyDeviceToDevice, stream_));
    }
    return true;
}

bool Engine::score(const uint32_t * tokens, size_t T, const uint32_t * targets, double * losses_out,
                   uint32_t * argmax_out, float * logits_out) {
    HIP_OK(hipSetDevice(m_->device));
    if (!tokens || T == 0 || (targets != nullptr) != (losses_out != nullptr) || !score_buffers(T)) return false;
    const ScoreRun run{targets, logits_out};
    co_retry_ = false;
    if (!run_tokens(tokens, T, true, &run)) return false;
    if (losses_out) HIP_OK(hipMemcpyAsync(losses_out, score_loss_, T * 8, hipMemcpyDeviceToHost, stream_));
    if (argmax_out) HIP_OK(hipMemcpyAsync(argmax_out, score_argmax_, T * 4, hipMemcpyDeviceToHost, stream_));
    HIP_OK(hipStreamSynchronize(stream_));
    // a hand-off timeout in a one-token chunk: nothing is re-run (the state has moved on)
    return handoff_check();
}

}  // namespace rwkvmi
