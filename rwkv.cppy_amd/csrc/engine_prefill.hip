// engine_prefill.hip -- batched prefill: many prompts through packed sequence passes into the
// generation slots.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "engine.hpp"
#include "kernels.hpp"
#include "prefill_plan.hpp"

namespace rwkvmi {

// What batch_store does to a slot's sampling words, for the n rows of a prefill in one launch:
// counts[slot[i]][0 .. V) = 0 and words[slot[i]] (the done flag) = 0.
__global__ __launch_bounds__(256) void k_prefill_clear(const uint32_t * slot, size_t V, uint32_t * counts, uint32_t * words) {
    const size_t s = slot[blockIdx.y];
    uint32_t * c = counts + s * V;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < V; e += (size_t)gridDim.x * 256) c[e] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) words[s] = 0;
}

// The sequence path runs every per-token stage position-independently, so a chunk of tokens packed
// from several prompts is one forward_range call; only the token shift (k_ln_mix) and the WKV
// recurrences see that it is cut into segments, through SeqRun::seg.  States: every segment reads and
// writes a state in gstates_ -- [2][slots] and the fresh state -- at offsets from gstates_ itself, so
// the layer functions get gstates_ as both state pointers.  A segment never writes the state it
// reads (k_ln_mix: the workgroup of a segment's last token writes the carry its first token's
// workgroup reads).  Row i of P pieces in slot s:
//   fresh      piece p reads the fresh state (p == 0) or buffer (P - p) & 1, writes buffer (P - 1 - p) & 1:
//              the last piece writes gstate_[0]
//   continued  piece p reads buffer p & 1, writes buffer (p + 1) & 1: starts from gstate_[0]; with P odd
//              the result is in gstate_[1] and one launch copies those rows back at the end
bool Engine::prefill_batch(size_t n_rows, const uint32_t * slots, const uint32_t * tokens, const size_t * lengths,
                           const uint8_t * cont) {
    HIP_OK(hipSetDevice(m_->device));
    if (n_rows == 0 || n_rows > gslots_ || !slots || !tokens || !lengths) return false;
    const size_t n = m_->state_len, V = m_->n_vocab, C = m_->n_embed, cap = prefill_chunk_;
    size_t N = 0;
    for (size_t i = 0; i < n_rows; i++) {
        if (slots[i] >= gslots_ || lengths[i] == 0 || (cont && cont[i] && !gvalid_[slots[i]])) return false;
        N += lengths[i];
    }
    // ---- the plan and its tables, on the host
    const size_t max_segs = n_rows + N / cap + 1;
    std::vector<uint32_t> srow(max_segs), sbegin(max_segs), slen(max_segs), schunk(max_segs);
    const long long planned = prefill_plan(lengths, n_rows, cap, srow.data(), sbegin.data(), slen.data(), schunk.data(), max_segs);
    if (planned <= 0) return false;
    const size_t nseg = (size_t)planned, n_chunks = (size_t)schunk[nseg - 1] + 1;
    // one upload: [sin_off | sout_off] (8 bytes each) then begin, len, seg_of, end_src, slot, back (4 bytes each)
    const size_t w32 = 2 * nseg + N + 3 * n_rows;
    std::vector<uint64_t> tab(2 * nseg + (w32 + 1) / 2);
    uint64_t *sin_off = tab.data(), *sout_off = sin_off + nseg;
    uint32_t *begin = (uint32_t *)(sout_off + nseg), *len = begin + nseg, *seg_of = len + nseg, *end_src = seg_of + N,
             *slot = end_src + n_rows, *back = slot + n_rows;
    std::vector<uint32_t> pieces(n_rows, 0), chunk_seg0(n_chunks + 1, 0), chunk_tok0(n_chunks + 1, 0);
    for (size_t j = 0; j < nseg; j++) pieces[srow[j]]++;
    auto state_off = [&](unsigned buf, size_t s) { return (uint64_t)((buf * gslots_ + s) * n); };
    const uint64_t fresh_off = (uint64_t)(2 * gslots_ * n);
    size_t n_back = 0, tok = 0, row_tok = 0;
    uint32_t piece = 0;
    for (size_t j = 0; j < nseg; j++) {
        const uint32_t i = srow[j], P = pieces[i], c = schunk[j];
        if (j == 0 || srow[j - 1] != i) piece = 0, row_tok = 0;
        const bool ct = cont && cont[i];
        const unsigned wb = ct ? (piece + 1) & 1 : (P - 1 - piece) & 1;
        sin_off[j] = (!ct && piece == 0) ? fresh_off : state_off(wb ^ 1, slots[i]);
        sout_off[j] = state_off(wb, slots[i]);
        begin[j] = sbegin[j];
        len[j] = slen[j];
        if (j == 0 || schunk[j - 1] != c) chunk_seg0[c] = (uint32_t)j, chunk_tok0[c] = (uint32_t)tok;
        for (uint32_t t = 0; t < slen[j]; t++) seg_of[tok + t] = (uint32_t)j - chunk_seg0[c];
        tok += slen[j];
        row_tok += slen[j];
        // every table entry is checked here, before anything is enqueued: the segments tile their chunk
        // in order, stay inside it, and belong to the row whose tokens they cover
        if (slen[j] == 0 || sbegin[j] + slen[j] > cap || tok - chunk_tok0[c] != sbegin[j] + slen[j] || row_tok > lengths[i] ||
            sin_off[j] == sout_off[j] || sout_off[j] >= fresh_off)
            return false;
        if (piece + 1 == P) {
            if (row_tok != lengths[i]) return false;
            end_src[i] = sbegin[j] + slen[j] - 1;  // the row's last token, in chunk c
            if (wb == 1) back[n_back++] = slots[i];
        }
        piece++;
    }
    if (tok != N) return false;
    chunk_seg0[n_chunks] = (uint32_t)nseg;
    chunk_tok0[n_chunks] = (uint32_t)N;
    // rows ending in chunk c: [chunk_end0[c], chunk_end0[c + 1])
    std::vector<uint32_t> chunk_end0(n_chunks + 1, 0);
    {
        size_t j = 0;
        uint32_t ended = 0;
        for (size_t c = 0; c < n_chunks; c++) {
            chunk_end0[c] = ended;
            for (; j < chunk_seg0[c + 1]; j++)
                if (j + 1 == nseg || srow[j + 1] != srow[j]) ended++;
        }
        chunk_end0[n_chunks] = ended;
        if (ended != n_rows) return false;
    }
    for (size_t i = 0; i < n_rows; i++) slot[i] = slots[i];

    // ---- everything that allocates, before anything is enqueued
    co_ = false;  // sequence passes: the ordered layouts only
    if (!ensure_workspace((int)std::max(std::min(N, cap), n_rows))) return false;
    if (!grow(ptokens_, N, doubled(1024, N), GRAPHS_NONE) || !grow(ptab_, tab.size(), doubled(1024, tab.size()), GRAPHS_NONE) ||
        !grow(pend_x_, (size_t)kBatchMax * C, (size_t)kBatchMax * C, GRAPHS_NONE))
        return false;
    // from here on a failure leaves the slots of the call undefined
    auto fail = [&] { return slots_fail(n_rows, slots); };
    for (size_t i = 0; i < n_rows; i++)
        if (!(cont && cont[i])) gvalid_[slots[i]] = 0;
    if (hipMemcpyAsync(ptokens_, tokens, N * 4, hipMemcpyHostToDevice, stream_) != hipSuccess ||
        hipMemcpyAsync(ptab_, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream_) != hipSuccess)
        return fail();
    const uint64_t * d_sin = ptab_;
    const uint32_t * d32 = (const uint32_t *)(ptab_ + 2 * nseg);
    const uint32_t *d_begin = d32, *d_len = d32 + nseg, *d_seg_of = d32 + 2 * nseg, *d_end_src = d_seg_of + N,
                   *d_slot = d_end_src + n_rows, *d_back = d_slot + n_rows;

    for (size_t c = 0; c < n_chunks; c++) {
        const size_t s0 = chunk_seg0[c], t0 = chunk_tok0[c], T = chunk_tok0[c + 1] - t0;
        // in the order of SegTab's members: n, begin, len, sin_off, sout_off, seg_of
        const SegTab sg{(int)(chunk_seg0[c + 1] - s0), d_begin + s0, d_len + s0, d_sin + s0, d_sin + nseg + s0, d_seg_of + t0};
        if (hipMemcpyAsync(dtokens_, ptokens_ + t0, T * 4, hipMemcpyDeviceToDevice, stream_) != hipSuccess) return fail();
        // eager, as the sequence path: with kernel timing on, a one-token chunk's launches carry their
        // event pairs and the matmul groups theirs (mm_launch)
        {
            const LaunchTimerScope timed(this, timing_ && T == 1);
            if (!forward_range(packed_run((int)T, &sg, gstates_))) return fail();
        }
        // the residual rows of the tokens that end a row in this chunk, to the rows' places in pend_x_
        const uint32_t e0 = chunk_end0[c], ne = chunk_end0[c + 1] - e0;
        if (!launch_copy_rows(stream_, x_, d_end_src + e0, pend_x_ + (size_t)e0 * C, nullptr, (int)ne, C)) return fail();
    }
    // the head over the rows' last tokens as batched decode runs it over that many contexts (each row
    // the bits of its one-token head, as score_chunk), into the snapshot area -- free between
    // generate_batch calls -- and from there to the rows' slots
    if (!head_rows(rows_run((int)n_rows, 0, nullptr, nullptr, gsnap_logits_), pend_x_) ||
        !launch_copy_rows(stream_, gsnap_logits_, nullptr, glogits_, d_slot, (int)n_rows, V))
        return fail();
    if (!launch_copy_rows(stream_, gstate_[1], d_back, gstate_[0], d_back, (int)n_back, n)) return fail();
    // a new sequence in every slot: no token counted yet, not finished
    RK_LAUNCH(k_prefill_clear, dim3((unsigned)std::min<size_t>((V + 255) / 256, 256), (unsigned)n_rows), dim3(256), 0, stream_,
              d_slot, V, gcounts_.get(), gw_.done);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess || !handoff_check()) return fail();
    for (size_t i = 0; i < n_rows; i++) gvalid_[slots[i]] = 1;
    return true;
}

}  // namespace rwkvmi
