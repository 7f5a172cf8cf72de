// engine_tokenize.hip -- rwkv_mi355x_tokenize: the model's byte trie and the four launches of tokenize.hip.
#include <stdio.h>
#include <string.h>

#include "engine.hpp"
#include "kernels.hpp"

namespace rwkvmi {

int Engine::tokenize(const uint8_t * bytes, const uint64_t * offsets, size_t n_texts, uint32_t * tokens_out,
                     uint64_t * token_offsets_out, uint64_t * no_match) {
    if (hipSetDevice(m_->device) != hipSuccess) return 4;
    if (m_->vocab_offsets_h.empty()) return 1;
    if (m_->tok_state == DeviceModel::TOK_UNBUILT) {
        TokTrie t;
        if (!tok_build_trie(m_->vocab_offsets_h.data(), m_->vocab_bytes_h.data(), m_->n_vocab, t)) {
            m_->tok_state = DeviceModel::TOK_REFUSED;
        } else {
            DevBuf<uint32_t> d;
            if (!d.alloc(t.blob.size())) return 2;
            if (hipMemcpy(d, t.blob.data(), t.blob.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return 4;
            m_->tok_trie = std::move(d);
            m_->tok_nodes = t.n_nodes;
            m_->tok_lds = t.n_lds;
            m_->tok_lmax = t.lmax;
            m_->tok_state = DeviceModel::TOK_BUILT;
        }
    }
    if (m_->tok_state != DeviceModel::TOK_BUILT) return 1;

    const uint64_t first = offsets[0];
    const size_t total = (size_t)(offsets[n_texts] - first), n_tiles = (total + TOK_TILE - 1) / TOK_TILE;
    if (total == 0) {
        for (size_t i = 0; i <= n_texts; i++) token_offsets_out[i] = 0;
        return 0;
    }
    const size_t E = m_->tok_lmax ? m_->tok_lmax : 1, words = total / 4 + 1;
    if (!grow(tok_text_, words, doubled(4096, words), GRAPHS_NONE) || !grow(tok_len_, words * 4, doubled(16384, words * 4), GRAPHS_NONE) ||
        !grow(tok_id_, words * 4, doubled(16384, words * 4), GRAPHS_NONE) || !grow(tok_out_, total, doubled(16384, total), GRAPHS_NONE) ||
        !grow(tok_off_, n_texts + 1, doubled(64, n_texts + 1), GRAPHS_NONE) ||
        !grow(tok_text_out_, n_texts + 1, doubled(64, n_texts + 1), GRAPHS_NONE) ||
        !grow(tok_tiles_, 2 * n_tiles, doubled(64, 2 * n_tiles), GRAPHS_NONE) ||
        !grow(tok_tile_in_, 2 * n_tiles, doubled(64, 2 * n_tiles), GRAPHS_NONE) ||
        !grow(tok_table_, n_tiles * E, doubled(1024, n_tiles * E), GRAPHS_NONE) || !grow(tok_words_, 4, 4, GRAPHS_NONE))
        return 2;

    // the offsets from the first text's first byte; per tile the first text that ends behind its first
    // byte and the first (n_texts: the end of the last) that starts at or behind it
    tok_h_.resize(n_texts + 1 + 2 * n_tiles);
    uint32_t * off = tok_h_.data(), * end0 = off + n_texts + 1, * start0 = end0 + n_tiles;
    for (size_t i = 0; i <= n_texts; i++) off[i] = (uint32_t)(offsets[i] - first);
    for (size_t t = 0, ie = 0, is = 0; t < n_tiles; t++) {
        while (ie < n_texts && off[ie + 1] <= t * TOK_TILE) ie++;
        while (is < n_texts && off[is] < t * TOK_TILE) is++;
        end0[t] = (uint32_t)ie;
        start0[t] = (uint32_t)is;
    }

    TokArgs a;
    memset(&a, 0, sizeof(a));
    a.trie = m_->tok_trie;
    a.n_nodes = m_->tok_nodes;
    a.n_lds = m_->tok_lds;
    a.lmax = m_->tok_lmax;
    a.text = tok_text_;
    a.total = (uint32_t)total;
    a.off = tok_off_;
    a.n_texts = (uint32_t)n_texts;
    a.n_tiles = (uint32_t)n_tiles;
    a.tile_end0 = tok_tiles_;
    a.tile_start0 = tok_tiles_ + n_tiles;
    a.len = tok_len_;
    a.id = tok_id_;
    a.table = tok_table_;
    a.tile_in = tok_tile_in_;
    a.words = tok_words_;
    a.out = tok_out_;
    a.text_out = tok_text_out_;
    uint32_t w[3] = {1u, 0u, 0u};
    auto run = [&]() -> bool {
        HIP_OK(hipMemcpyAsync(tok_text_, bytes + first, total, hipMemcpyHostToDevice, stream_));
        HIP_OK(hipMemcpyAsync(tok_off_, off, (n_texts + 1) * 4, hipMemcpyHostToDevice, stream_));
        HIP_OK(hipMemcpyAsync(tok_tiles_, end0, 2 * n_tiles * 4, hipMemcpyHostToDevice, stream_));
        {
            const LaunchTimerScope timed(this, timing_);
            if (!launch_tok_match(stream_, a) || !launch_tok_tile(stream_, a) || !launch_tok_scan(stream_, a) ||
                !launch_tok_emit(stream_, a))
                return false;
        }
        HIP_OK(hipMemcpyAsync(w, tok_words_, sizeof(w), hipMemcpyDeviceToHost, stream_));
        HIP_OK(hipStreamSynchronize(stream_));
        return true;
    };
    if (!run()) {
        (void)hipStreamSynchronize(stream_);
        return 4;
    }
    if (w[0]) {
        if (no_match) *no_match = first + w[1];
        return 3;
    }
    if (w[2] > total) return 4;
    // the first output indices come back through the words the offsets went up in
    if (hipMemcpyAsync(off, tok_text_out_, (n_texts + 1) * 4, hipMemcpyDeviceToHost, stream_) != hipSuccess ||
        hipStreamSynchronize(stream_) != hipSuccess || off[n_texts] != w[2] ||
        (w[2] && hipMemcpy(tokens_out, tok_out_, (size_t)w[2] * 4, hipMemcpyDeviceToHost) != hipSuccess))
        return 4;
    for (size_t i = 0; i <= n_texts; i++) token_offsets_out[i] = off[i];
    return 0;
}

}  // namespace rwkvmi
