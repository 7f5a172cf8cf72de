// engine_spec.hip -- speculative generation on the device (rwkv_mi355x_generate_speculative).
#include <string.h>

#include "engine.hpp"
#include "kernels.hpp"

namespace rwkvmi {

// One sequence pass over the T rows in dtokens_ with the trace on, and the head over all T rows as
// score_chunk runs it (rows as contexts: each row the bits of its one-token head).  What run_tokens_impl
// does around a chunk of more than one token.
bool Engine::spec_traced_step(int T) {
    last_decode_ = false;
    co_ = false;
    logits_valid_ = false;
    SeqRun s = seq_run(T, dstate_[cur_], dstate_[cur_ ^ 1], 0, m_->n_layer, dtok(), nullptr);
    s.trace = spec_trace_;
    if (!forward_range(s) || !head_rows(rows_run(T, 0, nullptr, nullptr, spec_tile_), x_)) return false;
    HIP_OK(gran_.clear_tagged(stream_));  // a step without the fused decode flips the parity
    cur_ ^= 1;
    return true;
}

bool Engine::generate_speculative(const SamplingParams & p, const SpecParams & sp, size_t n, uint32_t * tokens_out,
                                  float * logits_out, SpecStats * stats) {
    HIP_OK(hipSetDevice(m_->device));
    const size_t S = m_->state_len, V = m_->n_vocab, C = m_->n_embed, nh = sp.n_history, R = (size_t)SPEC_ROWS;
    if (!logits_valid_ || !tokens_out || n == 0 || nh + n > (size_t)SPEC_MAX_CORPUS || (nh && !sp.history)) return false;
    // ---- everything that allocates, before anything is enqueued; dtokens_ moves when the workspace
    // grows (the graphs are dropped with it), so that comes first
    SampleArgs a;
    if (!ensure_workspace(SPEC_ROWS) || !sampler_buffers(p, 1, a) || !grow(spec_trace_, R * S, R * S, GRAPHS_NONE) ||
        !grow(spec_tile_, R * V, R * V, GRAPHS_NONE) || !grow(spec_corpus_, nh + n, doubled(1024, nh + n), GRAPHS_NONE) ||
        !grow(spec_draws_, R + 1, R + 1, GRAPHS_NONE) || !grow(spec_words_, 4, 4, GRAPHS_NONE))
        return false;
    if (!spec_h_) HIP_OK(hipHostMalloc((void **)&spec_h_, 64, hipHostMallocDefault));
    uint32_t * words = (uint32_t *)(spec_words_.get() + 1);
    SpecDraft sd;
    sd.corpus = spec_corpus_;
    sd.nh = (uint32_t)nh, sd.n = (uint32_t)n;
    sd.k = sp.draft_len, sd.gmin = sp.ngram_min, sd.gmax = sp.ngram_max;
    sd.rows = dtokens_;
    sd.w = SpecWords{words, words + 1, words + 2, spec_words_.get(), words + 3};
    SpecGeom g;
    g.n_layer = m_->n_layer;
    g.H = m_->major == 4 ? 0u : (uint32_t)m_->H, g.S = m_->major == 4 ? 0u : (uint32_t)m_->S;
    g.per_layer = layer_state_len(), g.state_len = S;
    g.shift = m_->major == 4 ? g.per_layer : 2 * C;
    g.transposed = m_->major == 5 || m_->major == 6;

    const int cur0 = cur_;
    co_retry_ = false;
    bool ok = hipMemsetAsync(spec_words_, 0, 4 * 8, stream_) == hipSuccess &&
              (!nh || hipMemcpyAsync(spec_corpus_, sp.history, nh * 4, hipMemcpyHostToDevice, stream_) == hipSuccess);
    // ---- the steps.  e: the tokens emitted, exact whenever the host decides something by it -- after a
    // traced step it lacks that step's accepted count until the next step's read
    SpecStats st;
    size_t e = 0;
    bool traced = false;  // the last step was a traced one: x0 is in place, its accepted count is due
    while (ok && e < n) {
        {
            const LaunchTimerScope timed(this, timing_);
            if (!traced) {
                a.logits = logits_, a.rows = 1;
                a.counter = p.offset + e;
                a.tok = spec_draws_ + R, a.tok2 = dtokens_;
                ok = launch_sample(stream_, a);
            }
            ok = ok && launch_spec_draft(stream_, sd);
        }
        // the step's one host wait: its draft count and the last step's accepted count
        ok = ok && hipMemcpyAsync(spec_h_, sd.w.d, 8, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
             hipStreamSynchronize(stream_) == hipSuccess;
        if (!ok) break;
        const uint32_t d = spec_h_[0];
        if (traced) {
            e += spec_h_[1];
            st.accepted += spec_h_[1];
            if (e >= n) break;  // the search saw that too and did nothing
        }
        if (d >= (uint32_t)SPEC_ROWS || e + 1 + d > n) {
            ok = false;
            break;
        }
        e += 1;  // x0
        st.steps++;
        st.drafted += d;
        traced = d != 0;
        if (!traced) {
            ok = run_tokens(nullptr, 1, true);
            const LaunchTimerScope timed(this, timing_);
            ok = ok && launch_spec_accept(stream_, sd, spec_draws_);
            continue;
        }
        ok = spec_traced_step((int)d + 1);
        const LaunchTimerScope timed(this, timing_);
        a.logits = spec_tile_, a.rows = (int)d + 1;
        a.counter = p.offset + e;  // row r: draw offset + e + r, e counting x0
        a.tok = spec_draws_, a.tok2 = nullptr;
        ok = ok && launch_sample(stream_, a) && launch_spec_accept(stream_, sd, spec_draws_) &&
             launch_spec_commit(stream_, g, spec_trace_, dstate_[cur_], spec_tile_, logits_, V, sd.w.m);
        logits_valid_ = ok;
    }
    ok = ok && e == n;
    if (ok) {
        ok = hipMemcpyAsync(tokens_out, spec_corpus_ + nh, n * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess;
        if (ok && logits_out) ok = copy_logits(logits_out);
    }
    ok = (hipStreamSynchronize(stream_) == hipSuccess) && ok;
    ok = handoff_check() && ok;
    if (!ok) {
        // as generate: the parity the call started with; state and logits are unspecified
        (void)gran_.clear_tagged(stream_);
        (void)hipStreamSynchronize(stream_);
        cur_ = cur0;
        logits_valid_ = false;
        return false;
    }
    if (stats) *stats = st;
    return true;
}

}  // namespace rwkvmi
