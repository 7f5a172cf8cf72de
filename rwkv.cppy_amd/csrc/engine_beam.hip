// engine_beam.hip -- beam search on the device (rwkv_mi355x_generate_beam).
#include <math.h>
#include <string.h>

#include <algorithm>

#include "engine.hpp"
#include "kernels.hpp"

namespace rwkvmi {

// The driver, shaped like generate_slots (engine_batch.hip).  The beams are rows [0, W) of the slots'
// buffers.  A batched step reads its rows contiguously from one state buffer and writes the other, so
// the reorder is a gather in front of it: per step k_beam_rows and k_beam_select on glogits_, then
// k_beam_gather gstate_[0][parent[j]] -> gstate_[1][j] and the step gstate_[1] -> gstate_[0], which
// also rewrites the logits rows (they need no gather).  Every step has the same buffers, so one
// captured graph serves them all, and the states end where batch_load reads them.  A finished beam's
// row is not gathered and decodes token 0 on whatever its row holds, as an idle queue lane does.
bool Engine::generate_beam(const BeamParams & p, size_t n, const BeamOut & out) {
    HIP_OK(hipSetDevice(m_->device));
    const size_t W = p.width, S = m_->state_len, V = m_->n_vocab;
    if (W == 0 || W > (size_t)BEAM_MAX_WIDTH || W > gslots_ || W > V || n == 0 || !logits_valid_ || !out.tokens ||
        !out.lengths || !out.scores || !out.finished || !out.rows || p.n_stop > 16u || (p.n_stop && !p.stop_tokens))
        return false;
    // ---- everything that allocates, before anything is enqueued (dtokens_ moves with the workspace)
    constexpr size_t K = BEAM_MAX_WIDTH, kWordDoubles = K + 2 * K * K + (5 * K + K) / 2;
    if (!ensure_workspace((int)W) || !grow(beam_words_, kWordDoubles, kWordDoubles, GRAPHS_NONE) ||
        !grow(beam_hist_, 2 * W * n, doubled(1024, 2 * W * n), GRAPHS_NONE) ||
        !grow(gtokens_, W * n, doubled(1024, W * n), GRAPHS_NONE))
        return false;
    beam_h_.assign(W * n + 2 * W, 0);
    BeamArgs a;
    memset(&a, 0, sizeof(a));
    a.logits = glogits_;
    a.W = (int)W;
    a.V = (int)V;
    double * score = beam_words_;
    a.rec = (BeamRec *)(score + K);
    uint32_t * words = (uint32_t *)(score + K + 2 * K * K);
    uint32_t *finished = words, *length = words + K;
    a.nrec = words + 2 * K, a.parent = words + 3 * K, a.token = words + 4 * K, a.live = words + 5 * K;
    a.score = a.score_out = score;
    a.finished = a.finished_out = finished;
    a.length = a.length_out = length;
    a.hist = (uint2 *)beam_hist_.get();
    a.dtok = dtokens_;
    a.n_stop = (int)p.n_stop;
    for (uint32_t j = 0; j < p.n_stop; j++) a.stop[j] = p.stop_tokens[j];

    // from here on a failure leaves slots [0, W) undefined
    auto fail = [&] { return slots_fail(W); };
    for (size_t j = 0; j < W; j++) gvalid_[j] = 0;
    float *A = gstate_[0], *B = gstate_[1];
    bool ok = hipMemcpyAsync(A, dstate_[cur_], S * 4, hipMemcpyDeviceToDevice, stream_) == hipSuccess &&
              hipMemcpyAsync(glogits_, logits_, V * 4, hipMemcpyDeviceToDevice, stream_) == hipSuccess &&
              launch_beam_begin(stream_, a);
    if (!ok) return fail();

    // ---- the steps
    size_t steps = 0;
    uint32_t live = 1;
    for (size_t i = 0; i < n && live; i++) {
        a.step = (uint32_t)i;
        {
            const LaunchTimerScope timed(this, timing_);
            ok = launch_beam_rows(stream_, a) && launch_beam_select(stream_, a) && launch_beam_gather(stream_, a, A, B, S);
        }
        ok = ok && eval_batch(nullptr, W, B, A, glogits_, true);
        if (!ok) return fail();
        steps++;
        if (p.check_every && (i + 1) % p.check_every == 0 && i + 1 < n &&
            (hipMemcpyAsync(&live, a.live, 4, hipMemcpyDeviceToHost, stream_) != hipSuccess ||
             hipStreamSynchronize(stream_) != hipSuccess))
            return fail();
    }

    // ---- the end: the token rows, then one copy of each array, unranked
    uint32_t *tok_h = beam_h_.data(), *len_h = tok_h + W * n, *fin_h = len_h + W;
    double score_h[BEAM_MAX_WIDTH];
    ok = launch_beam_finish(stream_, a, (uint32_t)steps, gtokens_, n) &&
         hipMemcpyAsync(tok_h, gtokens_, W * n * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
         hipMemcpyAsync(len_h, length, W * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
         hipMemcpyAsync(fin_h, finished, W * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
         hipMemcpyAsync(score_h, score, W * 8, hipMemcpyDeviceToHost, stream_) == hipSuccess;
    if (!ok || hipStreamSynchronize(stream_) != hipSuccess || !handoff_check()) return fail();

    // the ranking: score / max(len, 1)^alpha, descending, ties to the lower working row.  W values, in
    // double, on the host.  A beam that is not live reports finished; only a live beam's slot is valid.
    double key[BEAM_MAX_WIDTH];
    uint32_t order[BEAM_MAX_WIDTH];
    for (size_t r = 0; r < W; r++) {
        key[r] = score_h[r] / pow((double)std::max<uint32_t>(len_h[r], 1u), p.length_penalty);
    }
    // an insertion sort: stable, and bounded whatever a NaN key answers
    for (size_t r = 0; r < W; r++) {
        size_t at = r;
        for (; at > 0 && key[r] > key[order[at - 1]]; at--) order[at] = order[at - 1];
        order[at] = (uint32_t)r;
    }
    for (size_t j = 0; j < W; j++) {
        const uint32_t r = order[j];
        memcpy(out.tokens + j * n, tok_h + (size_t)r * n, n * 4);
        out.lengths[j] = len_h[r];
        out.scores[j] = score_h[r];
        out.finished[j] = fin_h[r] != BEAM_LIVE ? 1u : 0u;
        out.rows[j] = r;
        gvalid_[r] = fin_h[r] == BEAM_LIVE ? 1 : 0;
    }
    if (out.steps) *out.steps = (uint32_t)steps;
    return true;
}

}  // namespace rwkvmi
