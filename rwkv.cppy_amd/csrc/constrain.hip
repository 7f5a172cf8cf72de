// constrain.hip -- grammar-constrained generation: byte-DFA token masks (rwkv_mi355x_constraint,
// DESIGN 4u).  A constraint is a DFA over bytes; a token is allowed in state q when walking its bytes
// from q never reaches the dead state.  k_dfa_mask writes the masked copy l' of every live row's
// logits that the sampler, the filters and k_logprobs then read instead of the logits themselves;
// k_dfa_advance, behind the sampler, walks the drawn tokens.  sample.hip is not touched.
//
// The split is by token, not by row: a workgroup owns DFA_THREADS consecutive tokens, one a thread.
// It copies the class-compressed table into LDS once, reads its tokens' bytes once, translates the 16
// head bytes into byte classes once (they do not depend on the row), and then streams over the rows:
// per row the walk is one LDS lookup per byte, tab[s * n_cls + class].  The vocabulary is sorted by
// bytes, so the 64 tokens of a wave mostly share their first byte and a wave whose tokens are all dead
// leaves the walk after one lookup.
#include <string.h>

#include <vector>

#include "device_common.hpp"
#include "kernels.hpp"

namespace rwkvmi {

namespace {

constexpr uint32_t DFA_DEAD = 0xffffu;

__device__ __forceinline__ uint32_t dfa_pad16(uint32_t bytes) { return (bytes + 15u) & ~15u; }

// the row's sequence, or GEN_NONE when the row draws nothing (an idle lane, a finished sequence)
__device__ __forceinline__ uint32_t dfa_row_seq(const DfaArgs & a, int r) {
    const uint32_t seq = a.lane_seq ? a.lane_seq[r] : (uint32_t)r;
    if (seq == GEN_NONE || (a.done && a.done[seq] != 0)) return GEN_NONE;
    return seq;
}

// The end of both mask kernels.  The workgroup that finishes last sees every count: a live row with no
// allowed token is finished before its draw, as the sampler finishes a row at a stop token (done,
// fin_step, *active).  `last` is one LDS word.
__device__ __forceinline__ void dfa_finish_rows(const DfaArgs & a, uint32_t * last, int tid) {
    if (!a.ticket) return;
    __threadfence();
    __syncthreads();
    if (tid == 0) *last = atomicAdd(a.ticket, 1u) == gridDim.x - 1u ? 1u : 0u;
    __syncthreads();
    if (*last == 0u) return;
    __threadfence();
    for (int r = tid; r < a.rows; r += DFA_THREADS) {
        const uint32_t seq = dfa_row_seq(a, r);
        if (seq == GEN_NONE || atomicAdd(a.n_allowed + r, 0u) != 0u) continue;
        if (a.done) a.done[seq] = 1u;
        if (a.fin_step) a.fin_step[seq] = a.step;
        if (a.active) atomicSub(a.active, 1u);
        if (a.ended) a.ended[seq] = 2u;
    }
    if (tid == 0) *a.ticket = 0u;
}

// grid: ceil(V / DFA_THREADS) workgroups; dynamic LDS: dfa_lds_bytes(n_states, n_cls)
__global__ __launch_bounds__(DFA_THREADS) void k_dfa_mask(const DfaArgs a) {
    extern __shared__ uint4 lds4[];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t n_cls = a.n_cls, tab_bytes = dfa_pad16(a.n_states * n_cls * 2u);
    const uint16_t * tab = (const uint16_t *)lds4;
    const uint8_t * cls = (const uint8_t *)lds4 + tab_bytes;
    uint32_t * last = (uint32_t *)(cls + 256);

    // the table and the class map: one blob, whole 16-byte vectors
    const uint4 * src = (const uint4 *)a.tab;
    for (uint32_t i = tid; i < (tab_bytes + 256u) / 16u; i += DFA_THREADS) lds4[i] = src[i];

    // this thread's token: its length and head bytes stay in registers for every row
    const int t = blockIdx.x * DFA_THREADS + tid;
    const bool in = t < a.V;
    const int tc = min(t, a.V - 1);
    const uint4 h = a.head[tc];
    const uint2 m = a.meta[tc];  // length, offset of byte 16 in tail
    const int len = in ? (int)m.x : 0;
    bool is_stop = false;
#pragma unroll
    for (int j = 0; j < SAMPLE_MAX_STOP; j++) is_stop = is_stop || (j < a.n_stop && a.stop[j] == (uint32_t)t);
    __syncthreads();

    // the classes of the head bytes, packed as the bytes were
    const uint32_t hw[4] = {h.x, h.y, h.z, h.w};
    uint32_t c[4];
#pragma unroll
    for (int w = 0; w < 4; w++)
        c[w] = (uint32_t)cls[hw[w] & 255u] | (uint32_t)cls[(hw[w] >> 8) & 255u] << 8 |
               (uint32_t)cls[(hw[w] >> 16) & 255u] << 16 | (uint32_t)cls[hw[w] >> 24] << 24;

    const float NEG_INF = __int_as_float(0xff800000);
    for (int r = 0; r < a.rows; r++) {
        const uint32_t seq = dfa_row_seq(a, r);  // uniform
        if (seq == GEN_NONE) continue;
        const uint32_t q = a.state[seq];
        uint32_t s = q;
        bool alive = len > 0;
        // four bytes a group; a wave whose tokens are all through (mostly after one byte) skips the
        // rest group by group, without a lookup
#pragma unroll
        for (int g = 0; g < 4; g++) {
            if (__ballot(alive && 4 * g < len) == 0ull) continue;
#pragma unroll
            for (int i = 4 * g; i < 4 * g + 4; i++) {
                const bool go = alive && i < len;
                if (i > 4 * g && __ballot(go) == 0ull) continue;
                if (go) {
                    s = tab[s * n_cls + ((c[g] >> (8 * (i & 3))) & 255u)];
                    alive = s != DFA_DEAD;
                }
            }
        }
        if (alive && len > 16) {  // a long token: its tail comes from memory
            const uint8_t * tl = a.tail + m.y;
            for (int i = 16; i < len && alive; i++) {
                s = tab[s * n_cls + cls[tl[i - 16]]];
                alive = s != DFA_DEAD;
            }
        }
        const bool allowed = in && (is_stop ? a.accepting[q] != 0 : alive);
        if (in) {
            const size_t at = (size_t)r * (size_t)a.V + (size_t)t;
            a.masked[at] = allowed ? a.logits[at] : NEG_INF;
        }
        const unsigned long long b = __ballot(allowed);
        if (lane == 0 && b != 0ull) atomicAdd(a.n_allowed + r, (uint32_t)__popcll(b));
    }

    dfa_finish_rows(a, last, tid);
}

// ---- a resident table that does not fit the LDS (rwkv_mi355x_constraint_table) ---------
// k_dfa_mask_mem has k_dfa_mask's contract and split, and reads the table from memory.  Its LDS holds
// what the walks need beside it: the class map; one word per row, resolved by thread r in parallel
// (lane_seq -> done -> state -> accepting happen once per workgroup, not once per row in series); and
// the compacted list of the live rows.  The walks of four rows run in lockstep: the four loads of a
// byte are independent and in flight together.  (Staging the table rows of the rows' states in LDS for
// the first byte was measured and not kept: DESIGN 4v.)
constexpr uint32_t DFA_ROW_SKIP = 0xffffffffu;  // a row's word: state | accepting << 16, or no draw
constexpr uint32_t DFA_MEM_FIXED = 256 + 4 * DFA_THREADS + DFA_THREADS + 32;  // cls, words, live list, counts

// One byte (class ci) of up to four walks.  A walk that is not going reads entry 0 and keeps its state,
// so the four loads are unconditional and the compiler waits for them once.
__device__ __forceinline__ void dfa_step4(const uint16_t * __restrict__ tab, uint32_t n_cls, uint32_t ci, const bool (&go)[4],
                                          uint32_t (&s)[4], bool (&alive)[4]) {
    uint32_t x[4];
#pragma unroll
    for (int j = 0; j < 4; j++) x[j] = tab[go[j] ? s[j] * n_cls + ci : 0u];
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (go[j]) {
            s[j] = x[j];
            alive[j] = x[j] != DFA_DEAD;
        }
}

// grid: ceil(V / DFA_THREADS) workgroups; dynamic LDS: DFA_MEM_FIXED bytes; rows <= DFA_THREADS
__global__ __launch_bounds__(DFA_THREADS) void k_dfa_mask_mem(const DfaArgs a) {
    extern __shared__ uint4 lds4[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n_cls = a.n_cls;
    uint8_t * cls = (uint8_t *)lds4;
    uint32_t * word = (uint32_t *)(cls + 256);             // [DFA_THREADS]
    uint8_t * live = (uint8_t *)(word + DFA_THREADS);      // [DFA_THREADS]: the live rows, in order
    uint32_t * wave_n = (uint32_t *)(live + DFA_THREADS);  // [4], then the epilogue's word
    uint32_t * last = wave_n + 4;
    const uint16_t * __restrict__ tab = a.tab;

    // the class map behind the table, and row tid's word
    if (tid < 16) ((uint4 *)cls)[tid] = ((const uint4 *)((const uint8_t *)a.tab + dfa_pad16(a.n_states * n_cls * 2u)))[tid];
    uint32_t w = DFA_ROW_SKIP;
    if (tid < a.rows) {
        const uint32_t seq = dfa_row_seq(a, tid);
        if (seq != GEN_NONE) {
            const uint32_t q = a.state[seq];
            if (q < a.n_states) w = q | (a.accepting[q] != 0 ? 0x10000u : 0u);
        }
    }
    word[tid] = w;
    const unsigned long long mine = __ballot(w != DFA_ROW_SKIP);
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(mine);

    // this thread's token, as in k_dfa_mask
    const int t = blockIdx.x * DFA_THREADS + tid;
    const bool in = t < a.V;
    const int tc = min(t, a.V - 1);
    const uint4 h = a.head[tc];
    const uint2 m = a.meta[tc];
    const int len = in ? (int)m.x : 0;
    bool is_stop = false;
#pragma unroll
    for (int j = 0; j < SAMPLE_MAX_STOP; j++) is_stop = is_stop || (j < a.n_stop && a.stop[j] == (uint32_t)t);
    __syncthreads();

    uint32_t at = (uint32_t)__popcll(mine & ((1ull << lane) - 1ull)), n = 0;
#pragma unroll
    for (int v = 0; v < DFA_THREADS / 64; v++) {
        if (v < wave) at += wave_n[v];
        n += wave_n[v];
    }
    if (w != DFA_ROW_SKIP) live[at] = (uint8_t)tid;
    const uint32_t hw[4] = {h.x, h.y, h.z, h.w};
    uint32_t c[4];
#pragma unroll
    for (int v = 0; v < 4; v++)
        c[v] = (uint32_t)cls[hw[v] & 255u] | (uint32_t)cls[(hw[v] >> 8) & 255u] << 8 |
               (uint32_t)cls[(hw[v] >> 16) & 255u] << 16 | (uint32_t)cls[hw[v] >> 24] << 24;
    __syncthreads();

    const float NEG_INF = __int_as_float(0xff800000);
    const uint8_t * tl = a.tail + m.y;
    for (uint32_t j0 = 0; j0 < n; j0 += 4) {
        uint32_t row[4], s[4];
        bool acc[4], alive[4], go[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {  // uniform; a slot past the last live row repeats it and stays idle
            row[j] = __builtin_amdgcn_readfirstlane((uint32_t)live[min(j0 + j, n - 1u)]);
            const uint32_t wj = __builtin_amdgcn_readfirstlane(word[row[j]]);
            s[j] = wj & 0xffffu;
            acc[j] = (wj & 0x10000u) != 0u;
            alive[j] = len > 0 && j0 + j < n;
        }
        // a wave with no walk still going in any of the four rows leaves, mostly after the first byte:
        // the vocabulary is sorted by bytes, so its 64 tokens tend to die together
#pragma unroll
        for (int i = 0; i < 16; i++) {
            bool any = false;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                go[j] = alive[j] && i < len;
                any = any || go[j];
            }
            if (__ballot(any) == 0ull) break;
            dfa_step4(tab, n_cls, (c[i >> 2] >> (8 * (i & 3))) & 255u, go, s, alive);
        }
        if (len > 16) {  // a long token: its tail comes from memory
            for (int i = 16; i < len && (alive[0] || alive[1] || alive[2] || alive[3]); i++) {
#pragma unroll
                for (int j = 0; j < 4; j++) go[j] = alive[j];
                dfa_step4(tab, n_cls, cls[tl[i - 16]], go, s, alive);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j0 + j >= n) break;
            const bool allowed = in && (is_stop ? acc[j] : alive[j]);
            if (in) {
                const size_t o = (size_t)row[j] * (size_t)a.V + (size_t)t;
                a.masked[o] = allowed ? a.logits[o] : NEG_INF;
            }
            const unsigned long long b = __ballot(allowed);
            if (lane == 0 && b != 0ull) atomicAdd(a.n_allowed + row[j], (uint32_t)__popcll(b));
        }
    }
    dfa_finish_rows(a, last, tid);
}

// Behind the sampler.  Workgroup 0, thread r = row r: the row's count is cleared for the next mask; a
// row that drew a non-stop token walks it (table and class map from memory: one lane, a few bytes); a
// row the sampler stopped at this step records ended = 1.  Every workgroup: when `snap` is set and row
// 0 ended without a draw at this step, the state and logits it ended with are copied aside (the
// single-sequence loop decodes on regardless, as the batched loop does).
__global__ __launch_bounds__(DFA_THREADS) void k_dfa_advance(const DfaArgs a, const DfaSnap snap) {
    const int tid = threadIdx.x;
    if (snap.state_to && a.done[0] != 0 && a.fin_step[0] == a.step && a.ended[0] == 2u) {
        for (size_t i = (size_t)blockIdx.x * DFA_THREADS + tid; i < snap.state_len; i += (size_t)gridDim.x * DFA_THREADS)
            snap.state_to[i] = snap.state_from[i];
        for (size_t i = (size_t)blockIdx.x * DFA_THREADS + tid; i < (size_t)a.V; i += (size_t)gridDim.x * DFA_THREADS)
            snap.logits_to[i] = snap.logits_from[i];
    }
    if (blockIdx.x != 0 || tid >= a.rows) return;
    const int r = tid;
    if (a.n_allowed) a.n_allowed[r] = 0u;
    const uint32_t seq = a.lane_seq ? a.lane_seq[r] : (uint32_t)r;
    if (seq == GEN_NONE) return;
    if (a.done && a.done[seq] != 0) {
        if (a.ended && a.fin_step && a.fin_step[seq] == a.step && a.ended[seq] == 0u) a.ended[seq] = 1u;
        return;
    }
    const uint32_t t = a.tokens[r];
    if (t >= (uint32_t)a.V) return;
    const uint32_t n_cls = a.n_cls;
    const uint8_t * cls = (const uint8_t *)a.tab + dfa_pad16(a.n_states * n_cls * 2u);
    const uint8_t * hd = (const uint8_t *)(a.head + t);
    const uint2 m = a.meta[t];
    uint32_t s = a.state[seq];
    for (uint32_t i = 0; i < m.x && s != DFA_DEAD; i++) {
        const uint8_t b = i < 16u ? hd[i] : a.tail[m.y + i - 16u];
        s = a.tab[s * n_cls + cls[b]];
    }
    if (s != DFA_DEAD) a.state[seq] = s;  // an allowed token never dies; a state is always < n_states
}

}  // namespace

size_t dfa_lds_bytes(uint32_t n_states, uint32_t n_cls) {
    return (((size_t)n_states * n_cls * 2 + 15) & ~(size_t)15) + 256 + 16;
}

size_t dfa_lds_limit(int device) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || v < 0) {
        (void)hipGetLastError();
        return 0;
    }
    return (size_t)v;
}

bool dfa_compress(const uint16_t * next, uint32_t n_states, DfaTable & out) {
    if (!next || n_states == 0 || n_states >= DFA_DEAD) return false;
    for (size_t i = 0; i < (size_t)n_states * 256; i++)
        if (next[i] != DFA_DEAD && next[i] >= n_states) return false;
    // two bytes are one class when their columns are equal; the classes are numbered by first byte
    std::vector<uint32_t> rep;
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t k = 0;
        for (; k < rep.size(); k++) {
            const uint32_t o = rep[k];
            uint32_t s = 0;
            while (s < n_states && next[(size_t)s * 256 + b] == next[(size_t)s * 256 + o]) s++;
            if (s == n_states) break;
        }
        if (k == rep.size()) rep.push_back(b);
        out.cls[b] = (uint8_t)k;
    }
    out.n_states = n_states;
    out.n_cls = (uint32_t)rep.size();
    // the blob the kernels read: the table, padded to 16 bytes, then the class map
    const size_t tab_bytes = ((size_t)n_states * out.n_cls * 2 + 15) & ~(size_t)15;
    out.blob.assign(tab_bytes + 256, 0);
    uint16_t * tab = (uint16_t *)out.blob.data();
    for (uint32_t s = 0; s < n_states; s++)
        for (uint32_t k = 0; k < out.n_cls; k++) tab[(size_t)s * out.n_cls + k] = next[(size_t)s * 256 + rep[k]];
    memcpy(out.blob.data() + tab_bytes, out.cls, 256);
    return true;
}

bool dfa_pack_vocab(const uint32_t * offsets, const uint8_t * bytes, size_t V, std::vector<uint8_t> & head,
                    std::vector<uint32_t> & meta, std::vector<uint8_t> & tail) {
    if (!offsets || V == 0) return false;
    for (size_t t = 0; t < V; t++)
        if (offsets[t + 1] < offsets[t]) return false;
    if (offsets[V] > offsets[0] && !bytes) return false;
    head.assign(V * 16, 0);
    meta.assign(V * 2, 0);
    tail.clear();
    for (size_t t = 0; t < V; t++) {
        const uint32_t len = offsets[t + 1] - offsets[t];
        const uint8_t * b = bytes + offsets[t];
        if (len) memcpy(&head[t * 16], b, len < 16 ? len : 16);
        meta[2 * t] = len;
        meta[2 * t + 1] = (uint32_t)tail.size();
        if (len > 16) tail.insert(tail.end(), b + 16, b + len);
    }
    return true;
}

static bool dfa_args_ok(const DfaArgs & a) {
    return a.head && a.meta && a.tail && a.V >= 1 && a.tab && a.accepting && a.n_states >= 1 && a.n_cls >= 1 &&
           a.n_cls <= 256 && a.rows >= 1 && a.state && a.n_stop >= 0 && a.n_stop <= SAMPLE_MAX_STOP;
}

bool launch_dfa_mask(hipStream_t st, const DfaArgs & a, size_t lds_limit) {
    if (!dfa_args_ok(a) || !a.logits || !a.masked || !a.n_allowed) return false;
    const size_t lds = dfa_lds_bytes(a.n_states, a.n_cls);
    if (lds > lds_limit) return false;
    if (lds > 48 * 1024)
        HIP_OK(hipFuncSetAttribute((const void *)k_dfa_mask, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    RK_LAUNCH(k_dfa_mask, dim3((unsigned)((a.V + DFA_THREADS - 1) / DFA_THREADS)), dim3(DFA_THREADS), (unsigned)lds, st, a);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_dfa_mask_mem(hipStream_t st, const DfaArgs & a) {
    if (!dfa_args_ok(a) || !a.logits || !a.masked || !a.n_allowed || a.rows > DFA_THREADS || a.n_states >= DFA_DEAD) return false;
    RK_LAUNCH(k_dfa_mask_mem, dim3((unsigned)((a.V + DFA_THREADS - 1) / DFA_THREADS)), dim3(DFA_THREADS), DFA_MEM_FIXED, st, a);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_dfa_advance(hipStream_t st, const DfaArgs & a, const DfaSnap * snap) {
    if (!dfa_args_ok(a) || !a.tokens || a.rows > DFA_THREADS) return false;
    DfaSnap sn;
    memset(&sn, 0, sizeof(sn));
    unsigned parts = 1;
    if (snap) {
        if (!snap->state_to || !snap->state_from || !snap->logits_to || !snap->logits_from || a.rows != 1 || !a.done ||
            !a.fin_step || !a.ended)
            return false;
        sn = *snap;
        parts = 16;
    }
    RK_LAUNCH(k_dfa_advance, dim3(parts), dim3(DFA_THREADS), 0, st, a, sn);
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi
