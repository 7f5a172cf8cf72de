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

bool Engine::sample(const SamplingParams & p, uint32_t * token_out, const LogprobsOut * lp) {
    HIP_OK(hipSetDevice(m_->device));
    if (!logits_valid_ || !token_out) return false;
    SampleArgs a;
    if (lp && !lp_reserve(1, 1, lp->top_k)) return false;
    if (!sampler_buffers(p, 1, a) || !lp_begin(lp, 1, 1, a)) return false;
    if (lp && !launch_logprobs(stream_, a)) return false;
    if (!launch_sample(stream_, a)) return false;
    HIP_OK(hipMemcpyAsync(token_out, gen_tokens_, 4, hipMemcpyDeviceToHost, stream_));
    if (!lp_copy_out(lp, 1, 1)) return false;
    HIP_OK(hipStreamSynchronize(stream_));
    return handoff_check();
}

bool Engine::generate(const SamplingParams & p, size_t n, uint32_t * tokens_out, float * logits_out,
                      const LogprobsOut * lp) {
    HIP_OK(hipSetDevice(m_->device));
    if (!logits_valid_ || !tokens_out || n == 0) return false;
    SampleArgs a;
    // dtokens_ moves when the workspace grows (the graphs are dropped with it): settle it first
    if (!ensure_workspace(1) || (lp && !lp_reserve(1, n, lp->top_k)) || !sampler_buffers(p, n, a)) return false;
    const int cur0 = cur_;
    co_retry_ = false;
    bool ok = lp_begin(lp, 1, n, a);
    const size_t K = lp ? lp->top_k : 0;
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
            ok = (!lp || launch_logprobs(stream_, a)) && launch_sample(stream_, a);
        }
        ok = ok && run_tokens(nullptr, 1, true);
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
