// tokenize.hip -- greedy longest-match tokenization over the vocabulary's byte trie (rwkv_mi355x_tokenize,
// DESIGN 4y): text in, ids out, the inverse of the walk the constraint kernels do.
//
// Greedy matching is serial along a text: where a token starts depends on where the one before it
// ended.  Four launches take that apart:
//   k_tok_match  one walk of the trie from every byte, as if a token started there: len[p], id[p]
//   k_tok_tile   next(p) = p + len[p] is now a table; a chain can enter a tile of TOK_TILE bytes at
//                one of lmax offsets only, and one lane per offset walks it to the tile's end
//   k_tok_scan   the tiles' maps composed in order: every tile's true entry and first output index
//   k_tok_emit   every tile walks its one true chain and stores the ids
// A walk stops at the end of its text, so no match crosses into the next text and every chain lands
// on every text boundary: a boundary restarts the chain by itself.  No workgroup waits for another
// inside a launch, and every loop is bounded by lmax, a tile's bytes or a count from the arguments.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "kernels.hpp"

namespace rwkvmi {

constexpr int TOK_MATCH_THREADS = TOK_TILE / 4;  // four consecutive bytes per lane: dword and uint4 stores
constexpr int TOK_THREADS = 256;                 // the other three kernels; >= TOK_LMAX entry offsets
constexpr int TOK_SPAN = TOK_TILE + 256;         // a tile and its halo of lmax - 1 bytes
constexpr int TOK_SCAN_LDS = 48 * 1024;          // k_tok_scan: the tile maps staged per pass
constexpr int TOK_SCAN_THREADS = 1024;
constexpr int TOK_SCAN_VEC = TOK_SCAN_LDS / 16 / TOK_SCAN_THREADS;  // uint4 per lane and pass
constexpr uint32_t TOK_FAIL = 0x80000000u;
static_assert(TOK_LMAX <= TOK_THREADS && TOK_LMAX <= TOK_SPAN - TOK_TILE, "one lane per entry offset; the halo holds a token");
static_assert((TOK_SPAN / 4 + TOK_SPAN / 32 + 256) % 2 == 0, "the nodes in the LDS are 8-byte aligned");

__host__ __device__ inline uint32_t tok_entries(uint32_t lmax) { return lmax ? lmax : 1u; }
static size_t tok_match_lds(uint32_t n_lds) {
    return ((size_t)TOK_SPAN / 4 + TOK_SPAN / 32 + 256 + 2 * (size_t)n_lds + (n_lds + 3) / 4) * 4;
}

// grid: n_tiles workgroups; dynamic LDS: tok_match_lds(n_lds) -- the tile's bytes and halo, one bit per
// byte that ends a text, the root table, and the first n_lds nodes with their labels
__global__ __launch_bounds__(TOK_MATCH_THREADS) void k_tok_match(const TokArgs a) {
    extern __shared__ uint32_t lds[];
    uint32_t * text = lds;                     // [TOK_SPAN / 4]
    uint32_t * mark = text + TOK_SPAN / 4;     // [TOK_SPAN / 32]
    uint32_t * root = mark + TOK_SPAN / 32;    // [256]
    uint2 * node = (uint2 *)(root + 256);      // [n_lds]
    uint32_t * label4 = (uint32_t *)(node + a.n_lds);
    const uint2 * gnode = (const uint2 *)(a.trie + 256);
    const uint32_t * glabel4 = a.trie + 256 + 2 * (size_t)a.n_nodes;
    const uint32_t tid = threadIdx.x, t0 = blockIdx.x * (uint32_t)TOK_TILE;
    const uint32_t text_dwords = (a.total + 3) / 4;
    for (uint32_t i = tid; i < TOK_SPAN / 4; i += TOK_MATCH_THREADS) text[i] = t0 / 4 + i < text_dwords ? a.text[t0 / 4 + i] : 0u;
    for (uint32_t i = tid; i < TOK_SPAN / 32; i += TOK_MATCH_THREADS) mark[i] = 0u;
    for (uint32_t i = tid; i < 256; i += TOK_MATCH_THREADS) root[i] = a.trie[i];
    for (uint32_t i = tid; i < 2 * a.n_lds; i += TOK_MATCH_THREADS) ((uint32_t *)node)[i] = a.trie[256 + i];
    for (uint32_t i = tid; i < (a.n_lds + 3) / 4; i += TOK_MATCH_THREADS) label4[i] = glabel4[i];
    __syncthreads();
    // the texts that end inside the span: their last bytes
    const uint32_t span_end = min(a.total, t0 + (uint32_t)TOK_SPAN);
    for (uint32_t i = a.tile_end0[blockIdx.x] + tid; i < a.n_texts; i += TOK_MATCH_THREADS) {
        const uint32_t end = a.off[i + 1];
        if (end > span_end) break;
        if (end > t0) atomicOr(&mark[(end - 1 - t0) >> 5], 1u << ((end - 1 - t0) & 31));
    }
    __syncthreads();

    const uint8_t * tb = (const uint8_t *)text;
    const uint8_t * label = (const uint8_t *)label4;
    auto label_at = [&](uint32_t c) -> uint32_t {
        return c < a.n_lds ? label[c] : (glabel4[c >> 2] >> ((c & 3) * 8)) & 255u;
    };
    uint32_t lens = 0, ids[4];
    for (int k = 0; k < 4; k++) {
        const uint32_t p = tid * 4 + k;
        uint32_t best = 0, best_id = TOK_NONE;
        if (t0 + p < a.total) {
            uint32_t c = root[tb[p]];
            for (uint32_t j = 1; j <= a.lmax && c != 0; j++) {  // c: the node after j bytes
                const uint2 nd = c < a.n_lds ? node[c] : gnode[c];
                if (nd.x != TOK_NONE) best = j, best_id = nd.x;
                const uint32_t q = p + j - 1;  // the byte just taken: the last of its text?
                if (j == a.lmax || t0 + p + j >= a.total || ((mark[q >> 5] >> (q & 31)) & 1u)) break;
                const uint32_t b = tb[p + j];
                uint32_t lo = nd.y & (TOK_MAX_NODES - 1);
                const uint32_t end = min(lo + (nd.y >> 23), a.n_nodes);
                uint32_t hi = end;
                for (int it = 0; it < 9 && lo < hi; it++) {  // a range holds at most 256 children
                    const uint32_t mid = (lo + hi) >> 1;
                    if (label_at(mid) < b) lo = mid + 1;
                    else hi = mid;
                }
                c = lo < end && label_at(lo) == b ? lo : 0u;
            }
        }
        lens |= best << (8 * k);
        ids[k] = best_id;
    }
    if (t0 + tid * 4 < a.total) {  // the buffers end on a whole vector
        ((uint32_t *)a.len)[t0 / 4 + tid] = lens;
        ((uint4 *)a.id)[t0 / 4 + tid] = make_uint4(ids[0], ids[1], ids[2], ids[3]);
    }
}

// the tile's len[] into the LDS as dwords; returns the tile's bytes
__device__ __forceinline__ uint32_t tok_stage_len(const TokArgs & a, uint32_t * len4) {
    const uint32_t t0 = blockIdx.x * (uint32_t)TOK_TILE;
    for (uint32_t i = threadIdx.x; i < TOK_TILE / 4; i += TOK_THREADS)
        len4[i] = t0 + 4 * i < a.total ? ((const uint32_t *)a.len)[t0 / 4 + i] : 0u;
    __syncthreads();
    return min((uint32_t)TOK_TILE, a.total - t0);
}

// grid: n_tiles workgroups.  Lane e < lmax: the chain that enters the tile at offset e.
__global__ __launch_bounds__(TOK_THREADS) void k_tok_tile(const TokArgs a) {
    __shared__ uint32_t len4[TOK_TILE / 4];
    const uint32_t n = tok_stage_len(a, len4), E = tok_entries(a.lmax);
    const uint8_t * len = (const uint8_t *)len4;
    if (threadIdx.x >= E) return;
    uint32_t p = threadIdx.x, count = 0;
    bool fail = false;
    for (uint32_t it = 0; it < n && p < n; it++) {
        const uint32_t l = len[p];
        if (l == 0) {
            fail = true;
            break;
        }
        p += l;
        count++;
    }
    a.table[blockIdx.x * E + threadIdx.x] = fail ? TOK_FAIL | p : min(p - min(p, n), E - 1) | count << 8;
}

// grid: one workgroup of TOK_SCAN_THREADS; dynamic LDS: chunk * (max(lmax, 1) + 2) + 1057 words, chunk % 4 == 0.  The maps
// of `chunk` tiles are staged by all lanes as uint4 (at most TOK_SCAN_VEC a lane) while the next chunk's
// loads are in flight.  A step along the chain is one dependent LDS read, so the chunk is cut into G runs of
// S tiles, one per group of max(lmax, 1) lanes: every group composes its run's maps (S steps), lane 0
// follows the chain through the G composed maps (G steps), and one lane per group walks its run again from
// its true entry and notes every tile's entry and base (S steps): 2 S + G steps instead of G S.
__global__ __launch_bounds__(TOK_SCAN_THREADS) void k_tok_scan(const TokArgs a, uint32_t chunk) {
    extern __shared__ uint4 lds4[];
    const uint32_t E = tok_entries(a.lmax), W = (E + 63) & ~63u, G = TOK_SCAN_THREADS / W;
    uint32_t * lds = (uint32_t *)lds4;           // [chunk][E] the tiles' maps
    uint32_t * stage = lds + chunk * E;          // [chunk][2] the tiles' entries and bases, before they go out
    uint32_t * sub = stage + 2 * chunk;          // [G][E] the runs' composed maps
    uint32_t * gin = sub + TOK_SCAN_THREADS;     // [G][2] the runs' entries and bases; [2 G]: the runs that stand
    const uint32_t g = threadIdx.x / W, ge = threadIdx.x % W;
    uint4 next[TOK_SCAN_VEC];
    // the vectors of the tiles from c0 on; the last one may end in the table's slack
    auto load = [&](uint32_t c0) {
        const uint32_t n4 = c0 < a.n_tiles ? (min(chunk, a.n_tiles - c0) * E + 3) / 4 : 0u;
        const uint4 * from = (const uint4 *)(a.table + (size_t)c0 * E);
#pragma unroll
        for (int k = 0; k < TOK_SCAN_VEC; k++)
            if (threadIdx.x + k * TOK_SCAN_THREADS < n4) next[k] = from[threadIdx.x + k * TOK_SCAN_THREADS];
    };
    load(0);
    uint32_t e = 0, base = 0, failed = 0, at = 0;  // lane 0's
    for (uint32_t c0 = 0; c0 < a.n_tiles; c0 += chunk) {
        const uint32_t nt = min(chunk, a.n_tiles - c0), n4 = (nt * E + 3) / 4;
#pragma unroll
        for (int k = 0; k < TOK_SCAN_VEC; k++)
            if (threadIdx.x + k * TOK_SCAN_THREADS < n4) lds4[threadIdx.x + k * TOK_SCAN_THREADS] = next[k];
        __syncthreads();
        load(c0 + chunk);
        const uint32_t S = (nt + G - 1) / G, t_lo = min(g * S, nt), t_hi = min(t_lo + S, nt);
        if (g < G && ge < E) {  // the run's map from entry ge; TOK_FAIL: no match on that chain
            uint32_t x = ge, count = 0;
            bool bad = false;
            for (uint32_t t = t_lo; t < t_hi; t++) {
                const uint32_t w = lds[t * E + x];
                if (w & TOK_FAIL) {
                    bad = true;
                    break;
                }
                count += w >> 8;
                x = w & 255u;
            }
            sub[g * E + ge] = bad ? TOK_FAIL : x | count << 8;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t stand = 0;
            for (uint32_t k = 0; k < G && !failed; k++) {
                gin[2 * k] = e;
                gin[2 * k + 1] = base;
                const uint32_t w = sub[k * E + e];
                if (w & TOK_FAIL) {  // where in run k: its tiles once more
                    failed = 1;
                    for (uint32_t t = min(k * S, nt); t < min(k * S + S, nt); t++) {
                        const uint32_t v = lds[t * E + e];
                        if (v & TOK_FAIL) {
                            at = (c0 + t) * (uint32_t)TOK_TILE + (v & ~TOK_FAIL);
                            break;
                        }
                        e = v & 255u;
                    }
                    break;
                }
                base += w >> 8;
                e = w & 255u;
                stand = k + 1;
            }
            gin[2 * G] = stand;
        }
        __syncthreads();
        if (g < gin[2 * G] && ge == 0) {
            uint32_t x = gin[2 * g], b = gin[2 * g + 1];
            for (uint32_t t = t_lo; t < t_hi; t++) {
                stage[2 * t] = x;
                stage[2 * t + 1] = b;
                const uint32_t w = lds[t * E + x];
                b += w >> 8;
                x = w & 255u;
            }
        }
        __syncthreads();
        // after a failure k_tok_emit reads none of this
        for (uint32_t i = threadIdx.x; i < 2 * nt; i += TOK_SCAN_THREADS) a.tile_in[2 * c0 + i] = stage[i];
    }
    if (threadIdx.x == 0) {
        a.words[0] = failed;
        a.words[1] = at;
        a.words[2] = base;
    }
}

// grid: n_tiles workgroups.  Lane 0 lists the positions of the tile's true chain, all lanes store their
// ids; then the texts that start in the tile find their first output index among the positions.
__global__ __launch_bounds__(TOK_THREADS) void k_tok_emit(const TokArgs a) {
    __shared__ uint32_t len4[TOK_TILE / 4];
    __shared__ uint16_t pos[TOK_TILE];
    __shared__ uint32_t n_pos;
    if (a.words[0]) return;  // no match somewhere: the tiles behind it have no entry
    const uint32_t n = tok_stage_len(a, len4), t0 = blockIdx.x * (uint32_t)TOK_TILE;
    const uint8_t * len = (const uint8_t *)len4;
    if (threadIdx.x == 0) {
        uint32_t p = a.tile_in[2 * blockIdx.x], k = 0;
        for (uint32_t it = 0; it < n && p < n; it++) {
            pos[k++] = (uint16_t)p;
            if (len[p] == 0) break;
            p += len[p];
        }
        n_pos = k;
    }
    __syncthreads();
    const uint32_t base = a.tile_in[2 * blockIdx.x + 1], cnt = n_pos;
    if (base + cnt > a.total) return;  // never after a scan that succeeded: a token has a byte
    for (uint32_t k = threadIdx.x; k < cnt; k += TOK_THREADS) a.out[base + k] = a.id[t0 + pos[k]];
    // text i (and i == n_texts, the end of the last one) starts at a chain position or at the tile's end
    const bool last = blockIdx.x + 1 == a.n_tiles;
    for (uint32_t i = a.tile_start0[blockIdx.x] + threadIdx.x; i <= a.n_texts; i += TOK_THREADS) {
        const uint32_t s = a.off[i] - t0;
        if (!last && s >= (uint32_t)TOK_TILE) break;
        uint32_t lo = 0, hi = cnt;
        for (int it = 0; it < 13 && lo < hi; it++) {  // cnt <= TOK_TILE
            const uint32_t mid = (lo + hi) >> 1;
            if (pos[mid] < s) lo = mid + 1;
            else hi = mid;
        }
        a.text_out[i] = base + lo;
    }
}

// --------------------------------------------------------------------------------------------- host
bool tok_build_trie(const uint32_t * off, const uint8_t * bytes, size_t V, TokTrie & out) {
    if (!off) return false;
    std::vector<uint32_t> order;
    uint32_t lmax = 0;
    for (size_t t = 0; t < V; t++) {
        if (off[t + 1] < off[t]) return false;
        const uint32_t n = off[t + 1] - off[t];
        if (n == 0) continue;  // a token without bytes never matches
        if (!bytes || n > (uint32_t)TOK_LMAX) return false;
        lmax = std::max(lmax, n);
        order.push_back((uint32_t)t);
    }
    auto size = [&](uint32_t t) { return off[t + 1] - off[t]; };
    // by bytes, a prefix before its extensions, equal tokens by id
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const int c = memcmp(bytes + off[x], bytes + off[y], std::min(size(x), size(y)));
        return c != 0 ? c < 0 : size(x) != size(y) ? size(x) < size(y) : x < y;
    });
    // breadth first: node i is the tokens order[lo .. hi), which share their first `depth` bytes
    struct Range {
        uint32_t lo, hi, depth;
    };
    std::vector<Range> q{{0u, (uint32_t)order.size(), 0u}};
    std::vector<uint32_t> ids, kids, root(256, 0u), level_ends;
    std::vector<uint8_t> label{0};
    for (size_t i = 0; i < q.size(); i++) {
        if (i > 0 && q[i].depth != q[i - 1].depth) level_ends.push_back((uint32_t)i);
        uint32_t lo = q[i].lo;
        const uint32_t hi = q[i].hi, d = q[i].depth, first = (uint32_t)q.size();
        uint32_t id = TOK_NONE;
        while (lo < hi && size(order[lo]) == d) id = order[lo++];  // the highest id last
        while (lo < hi) {
            const uint8_t b = bytes[off[order[lo]] + d];
            uint32_t e = lo;
            while (e < hi && bytes[off[order[e]] + d] == b) e++;
            if (i == 0) root[b] = (uint32_t)q.size();
            q.push_back({lo, e, d + 1});
            label.push_back(b);
            lo = e;
        }
        if (q.size() >= TOK_MAX_NODES) return false;
        ids.push_back(id);
        kids.push_back(first | ((uint32_t)q.size() - first) << 23);
    }
    level_ends.push_back((uint32_t)q.size());
    const uint32_t n = (uint32_t)q.size();
    out.n_nodes = n;
    out.lmax = lmax;
    out.n_lds = 1;
    for (uint32_t e : level_ends)
        if (1024 + 8 * (size_t)e + (e + 3) / 4 * 4 <= (size_t)TOK_TRIE_LDS) out.n_lds = e;
    out.blob.assign(256 + 2 * (size_t)n + (n + 3) / 4, 0u);
    memcpy(out.blob.data(), root.data(), 1024);
    for (uint32_t i = 0; i < n; i++) {
        out.blob[256 + 2 * (size_t)i] = ids[i];
        out.blob[256 + 2 * (size_t)i + 1] = kids[i];
    }
    memcpy(out.blob.data() + 256 + 2 * (size_t)n, label.data(), n);
    return true;
}

static bool tok_args_ok(const TokArgs & a) {
    return a.trie && a.n_nodes >= 1 && a.n_nodes < TOK_MAX_NODES && a.n_lds >= 1 && a.n_lds <= a.n_nodes &&
           tok_match_lds(a.n_lds) <= 5920 + (size_t)TOK_TRIE_LDS && a.lmax <= (uint32_t)TOK_LMAX && a.text && a.total >= 1 &&
           a.total <= (1u << 28) && a.off && a.n_texts >= 1 && a.n_tiles == (a.total + TOK_TILE - 1) / TOK_TILE && a.tile_end0 &&
           a.tile_start0 && a.len && a.id && a.table && a.tile_in && a.words && a.out && a.text_out;
}

bool launch_tok_match(hipStream_t st, const TokArgs & a) {
    if (!tok_args_ok(a)) return false;
    RK_LAUNCH(k_tok_match, dim3(a.n_tiles), dim3(TOK_MATCH_THREADS), (unsigned)tok_match_lds(a.n_lds), st, a);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_tok_tile(hipStream_t st, const TokArgs & a) {
    if (!tok_args_ok(a)) return false;
    RK_LAUNCH(k_tok_tile, dim3(a.n_tiles), dim3(TOK_THREADS), 0, st, a);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_tok_scan(hipStream_t st, const TokArgs & a) {
    if (!tok_args_ok(a)) return false;
    // whole vectors per pass: a multiple of four tiles, 48 to 1024 of them
    const uint32_t E = tok_entries(a.lmax), chunk = std::min(std::min((uint32_t)(TOK_SCAN_LDS / 4) / E & ~3u, 1024u), (a.n_tiles + 3) & ~3u);
    // the maps, the tiles' entries and bases, the runs' maps, their entries and bases and one word
    RK_LAUNCH(k_tok_scan, dim3(1), dim3(TOK_SCAN_THREADS), (chunk * (E + 2) + TOK_SCAN_THREADS + 33) * 4, st, a, chunk);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_tok_emit(hipStream_t st, const TokArgs & a) {
    if (!tok_args_ok(a)) return false;
    RK_LAUNCH(k_tok_emit, dim3(a.n_tiles), dim3(TOK_THREADS), 0, st, a);
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi
