// spec.hip -- the kernels of speculative generation around the traced sequence pass
// (rwkv_mi355x_generate_speculative; engine_spec.hip): the n-gram draft search over the
// token corpus, the accept step, the commit of a trace entry into the live state, and the copy of a
// layer's token-shift rows into the trace.
#include "device_common.hpp"
#include "kernels.hpp"

namespace rwkvmi {

namespace {

constexpr int SD_THREADS = 256, SD_MAX_GRID = 256;

// The draft search.  A candidate is the position q behind a match: with len(q) = the number of tokens
// in front of q that equal the tokens in front of the corpus' end L (at most gmax, at most q), a match
// of length g at p = q - g exists exactly when len(q) >= g.  So the rule "the longest g that matches
// anywhere, at its latest position" is one maximum over the key (len(q), q), q in [1, L - 1]: a thread
// keeps the best key of its positions (the first compare, against the corpus' last token, is a
// coalesced read of the whole corpus and ends almost every position), a wave and a workgroup reduce
// theirs, and the workgroups meet in one 64-bit atomic maximum.  The workgroup that takes the last
// ticket reads the result, writes the draft and re-arms both words.  Workgroup b owns the positions
// [1 + b span, 1 + (b + 1) span).
__global__ __launch_bounds__(SD_THREADS) void k_spec_draft(const SpecDraft a, uint32_t span) {
    __shared__ uint32_t s_suf[SPEC_MAX_NGRAM];
    __shared__ unsigned long long s_best[SD_THREADS / 64];
    __shared__ uint32_t s_last;
    const uint32_t tid = threadIdx.x, e = *a.w.e;  // no workgroup of this launch writes *e
    if (e >= a.n) {  // the call has its tokens: a step enqueued before the host knew
        if (blockIdx.x == 0 && tid == 0) *a.w.d = 0u;
        return;
    }
    // the corpus of this step: nh + e tokens in memory and x0, which nothing below reads from memory
    const uint32_t L = a.nh + e + 1u, x0 = a.rows[0];
    auto cget = [&](uint32_t i) -> uint32_t { return i == L - 1u ? x0 : a.corpus[i]; };
    const uint32_t gcap = min(a.gmax, L - 1u);  // g < L
    if (tid < SPEC_MAX_NGRAM) s_suf[tid] = tid < gcap ? cget(L - 1u - tid) : 0u;  // the end, last token first
    __syncthreads();
    unsigned long long best = 0ull;
    const uint32_t q0 = 1u + blockIdx.x * span, q1 = min(q0 + span, L);
    for (uint32_t q = q0 + tid; q < q1; q += SD_THREADS) {
        if (a.corpus[q - 1u] != s_suf[0]) continue;  // q - 1 <= L - 2
        const uint32_t cap = min(gcap, q);
        uint32_t len = 1u;
        while (len < cap && a.corpus[q - 1u - len] == s_suf[len]) len++;
        if (len >= a.gmin) best = max(best, ((unsigned long long)len << 32) | q);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), o), lo = __shfl_xor((uint32_t)best, o);
        best = max(best, ((unsigned long long)hi << 32) | lo);
    }
    if ((tid & 63u) == 0u) s_best[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < SD_THREADS / 64; w++) best = max(best, s_best[w]);
        if (best) atomicMax(a.w.key, best);
        __threadfence();
        s_last = atomicAdd(a.w.ticket, 1u) == gridDim.x - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last || tid != 0) return;
    __threadfence();
    const unsigned long long key = atomicMax(a.w.key, 0ull);  // every workgroup's maximum is in
    uint32_t d = 0u;
    if (key) {
        const uint32_t q = (uint32_t)key;
        d = min(min(a.k, L - q), a.n - e - 1u);  // what follows the match; the call's n tokens
        for (uint32_t i = 0; i < d; i++) a.rows[1u + i] = cget(q + i);
    }
    a.corpus[L - 1u] = x0;  // nh + e < nh + n
    *a.w.d = d;
    *a.w.key = 0ull;
    *a.w.ticket = 0u;
}

// one wave; lane r = row r
__global__ __launch_bounds__(64) void k_spec_accept(const SpecDraft a, const uint32_t * draws) {
    const uint32_t r = threadIdx.x, d = *a.w.d, e = *a.w.e;
    const uint32_t tok = r < d ? a.rows[1u + r] : 0u;
    const unsigned long long miss = __ballot(r < d && draws[r] != tok);
    const uint32_t m = miss ? (uint32_t)(__ffsll((long long)miss) - 1) : d;
    if (r < m) a.corpus[a.nh + e + 1u + r] = tok;  // <= nh + e + d <= nh + n - 1 (the draft's cut)
    if (r == 0) {
        *a.w.m = m;
        *a.w.e = e + 1u + m;
        if (d) a.rows[0] = draws[m];
    }
}

constexpr int SC_THREADS = 256, SC_S = 64;

// grid (H + 2, n_layer): workgroup (x, l) restores head x of layer l (x < H), the layer's shift rows
// (x == H) or part l of the logits row (x == H + 1).  *mp is read on the device, as k_beam_gather
// reads its parents.  A value-major head goes through an LDS tile, so that the reads and the writes are
// both contiguous.
__global__ __launch_bounds__(SC_THREADS) void k_spec_commit(const SpecGeom g, const float * trace, float * state,
                                                            const float * tile, float * logits, size_t V,
                                                            const uint32_t * mp) {
    __shared__ float t[SC_S][SC_S + 1];
    const uint32_t m = *mp, x = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
    if (m >= (uint32_t)SPEC_ROWS) return;
    if (x == g.H + 1u) {
        const float * src = tile + (size_t)m * V;
        for (size_t i = (size_t)l * SC_THREADS + tid; i < V; i += (size_t)g.n_layer * SC_THREADS) logits[i] = src[i];
        return;
    }
    const float * src = trace + (size_t)m * g.state_len + (size_t)l * g.per_layer;
    float * dst = state + (size_t)l * g.per_layer;
    if (x == g.H) {
        for (size_t i = tid; i < g.shift; i += SC_THREADS) dst[i] = src[i];
        return;
    }
    const uint32_t S = g.S, SS = S * S;
    src += g.shift + (size_t)x * SS;
    dst += g.shift + (size_t)x * SS;
    if (!g.transposed) {
        for (uint32_t i = tid; i < SS; i += SC_THREADS) dst[i] = src[i];
        return;
    }
    for (uint32_t i = tid; i < SS; i += SC_THREADS) t[i / S][i % S] = src[i];  // trace [j][i]
    __syncthreads();
    for (uint32_t i = tid; i < SS; i += SC_THREADS) dst[i] = t[i % S][i / S];  // state [i][j]
}

// grid (C / 256 rounded up, T)
__global__ __launch_bounds__(256) void k_spec_shift_trace(const float * xa, int C, float * trace_at, size_t stride) {
    const int c = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (c < C) trace_at[(size_t)t * stride + c] = xa[(size_t)t * C + c];
}

bool spec_draft_ok(const SpecDraft & a) {
    return a.corpus && a.rows && a.w.d && a.w.m && a.w.e && a.w.key && a.w.ticket && a.n >= 1 && a.k >= 1 &&
           a.k < (uint32_t)SPEC_ROWS && a.gmin >= 1 && a.gmin <= a.gmax && a.gmax <= SPEC_MAX_NGRAM &&
           (size_t)a.nh + a.n <= (size_t)SPEC_MAX_CORPUS;
}

}  // namespace

bool launch_spec_draft(hipStream_t st, const SpecDraft & a) {
    if (!spec_draft_ok(a)) return false;
    // the longest corpus of the call decides the shares, so that every step has the same grid
    const uint32_t lmax = a.nh + a.n, per = 4u * SD_THREADS;
    const uint32_t grid = std::min<uint32_t>(SD_MAX_GRID, (lmax + per - 1u) / per);
    const uint32_t span = (lmax + grid - 1u) / grid;
    RK_LAUNCH(k_spec_draft, dim3(grid), dim3(SD_THREADS), 0, st, a, span);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_spec_accept(hipStream_t st, const SpecDraft & a, const uint32_t * draws) {
    if (!spec_draft_ok(a) || !draws) return false;
    RK_LAUNCH(k_spec_accept, dim3(1), dim3(64), 0, st, a, draws);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_spec_commit(hipStream_t st, const SpecGeom & g, const float * trace, float * state, const float * tile,
                        float * logits, size_t V, const uint32_t * m) {
    if (!trace || !state || !tile || !logits || !m || V == 0 || g.n_layer == 0 || g.n_layer > 65535u ||
        (g.H && (g.S == 0 || g.S > (uint32_t)SC_S)) || g.shift + (size_t)g.H * g.S * g.S != g.per_layer ||
        g.per_layer * g.n_layer != g.state_len)
        return false;
    RK_LAUNCH(k_spec_commit, dim3(g.H + 2u, g.n_layer), dim3(SC_THREADS), 0, st, g, trace, state, tile, logits, V, m);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_spec_shift_trace(hipStream_t st, const float * xa, int T, int C, float * trace_at, size_t stride) {
    if (!xa || !trace_at || T < 1 || T > SPEC_ROWS || C < 1) return false;
    RK_LAUNCH(k_spec_shift_trace, dim3((unsigned)(C + 255) / 256, (unsigned)T), dim3(256), 0, st, xa, C, trace_at, stride);
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi
