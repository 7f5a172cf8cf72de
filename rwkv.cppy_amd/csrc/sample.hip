// sample.hip -- token sampling on the device (rwkv_mi355x_sample / _generate): logit bias, greedy
// or top-p + temperature sampling of one logits row per workgroup, the semantics of the
// reference's sampling.py:18-52 with the uniform draw made explicit.
//
// One workgroup of 1024 threads per row; thread t holds elements k * 1024 + t (k < 64) in
// registers, so a row of up to 65536 logits is read from memory once (every wave load is 256
// contiguous bytes).  Rows beyond 65536 are recomputed from memory where they are needed.
//
//   1. l = logits + bias; m = max l with the lowest index holding it (greedy returns that index)
//   2. e = expf(l - m), S = sum e            (p = e / S is never formed: every test is on e)
//   3. top-p: the cutoff is the largest e_c with sum{e >= e_c} > top_p * S, found by bisection on
//      the bit pattern of e (non-negative floats order like their bits): 30 masked sums, no sort.
//      Every e >= e_c is kept, so ties at the cutoff are all kept.
//   4. w = expf((l - m) / temperature) for kept elements (e itself at temperature 1), else 0
//   5. the draw: smallest index t with cdf(t) > u * Z in vocabulary order
//
// Every sum has one fixed association (no atomics on floats, nothing depends on scheduling), so a
// call is a pure function of its inputs.  Chains: 64 serial adds per thread, 6 DPP levels per wave,
// a 4-level tree over the 16 waves (sums); 6 DPP levels, 6 scan levels, 15 wave offsets (the cdf).
// Non-finite logits cannot hang or fault it: every loop has a fixed bound and the token is clamped.
//
// k_sample_rows is the same arithmetic for a batch of rows that each have their own parameters
// (rwkv_mi355x_generate_batch): per-row temperature, top_p and draw stream, presence / frequency
// penalties over a count table, stop tokens and finished rows (SampleArgs in kernels.hpp).
// k_gen_snapshot / k_gen_restore / k_gen_begin keep the finished rows' states (engine_batch.hip,
// generate_batch).  k_gen_turnover / k_gen_move give the rows of ended sequences to waiting ones
// (generate_queue).
#include "device_common.hpp"
#include "kernels.hpp"
#include "sample_row.hpp"

namespace rwkvmi {

namespace {

struct SampleShared {
    uint32_t bid[SAMPLE_MAX_BIAS];
    float bval[SAMPLE_MAX_BIAS];
    float red[2][SM_WAVES];            // block sums, double-buffered (one barrier per sum)
    float amax_v[SM_WAVES];
    int amax_i[SM_WAVES];
    int cnt[SM_WAVES], last[SM_WAVES];
    float wtot[SM_WAVES];
    float tab[SM_MAX_ROWS * SM_WAVES];  // (row k, wave) totals of w in vocabulary order -> their prefix sums
    int sel;
};

// Sum over the workgroup, every thread gets it: 6 DPP levels, then a fixed tree over the waves.
__device__ __forceinline__ float sm_block_sum(float part, SampleShared & sh, int & phase) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float * buf = sh.red[phase & 1];
    phase++;
    part = wave_sum63(part);
    if (lane == 63) buf[wave] = part;
    __syncthreads();
    float t[SM_WAVES];
#pragma unroll
    for (int i = 0; i < SM_WAVES; i++) t[i] = buf[i];
#pragma unroll
    for (int s = 1; s < SM_WAVES; s *= 2)
#pragma unroll
        for (int i = 0; i < SM_WAVES; i += 2 * s) t[i] += t[i + s];
    return t[0];
}

// The sampler of one row.  ROWS = false is k_sample: one set of parameters for every row.  ROWS =
// true is k_sample_rows: per-row parameters, penalties, stops and finished rows (SampleArgs); every
// addition is behind `if constexpr (ROWS)`, so the two kernels share one copy of the arithmetic and
// k_sample keeps the registers, LDS and occupancy it had before its sibling existed.
// LP = true (k_sample_lp, k_sample_rows_lp; launch_sample picks them when SampleArgs::lp_token is
// set) adds one store to emit: the drawn token's log-probability, l_t - logZ, with the logZ that
// k_logprobs (logprobs.hip) left for the row.  Nothing else differs, and the LP = false kernels are
// the kernels they were before the flag existed.
template <bool ROWS, bool LP>
__device__ __forceinline__ void sample_row(const SampleArgs & a, SampleShared & sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V, nb = a.n_bias;
    const int nrows = (V + SM_THREADS - 1) / SM_THREADS;  // <= SM_MAX_ROWS (launch_sample)
    const float * lg = a.logits + (size_t)blockIdx.x * (size_t)V;
    const float NEG_INF = __int_as_float(0xff800000);
    int phase = 0;
    float temperature = a.temperature, top_p = a.top_p;
    SmPenalty pen;
    // the sequence of this row and the index of its draw (a queue: SampleArgs::lane_seq); uniform
    uint32_t seq = blockIdx.x, at = a.step;
    if constexpr (ROWS) {
        bool idle = false;
        if (a.lane_seq) {
            seq = a.lane_seq[blockIdx.x];
            idle = seq == GEN_NONE;
            if (!idle) at = a.length[seq];
        }
        const uint32_t r = seq;
        if (idle || (a.done && a.done[r] != 0)) {
            // a finished row: the decode step still embeds tok2[row], so it gets an id < V
            if (tid == 0 && a.tok2) a.tok2[blockIdx.x] = 0;
            return;
        }
        if (a.temperature_r) temperature = a.temperature_r[r];
        if (a.top_p_r) top_p = a.top_p_r[r];
        sm_row_penalty(a, r, pen);
    }
    // l_i of an element outside the registers (and of kept elements at a temperature other than 1):
    // the same additions in the same order as the register copy below
    auto biased = [&](int i) -> float { return sm_biased<ROWS>(lg, pen, nb, sh.bid, sh.bval, i); };
    // the one thread that holds the drawn token publishes it
    auto emit = [&](uint32_t t) {
        if constexpr (LP) {
            // before the count of t grows: the l the token was drawn from
            const size_t col = !ROWS ? (size_t)blockIdx.x : a.tok_stride ? (size_t)seq * a.tok_stride + at : (size_t)seq;
            a.lp_token[col] = (double)biased((int)t) - a.lp_logz[blockIdx.x];
        }
        if constexpr (!ROWS) {
            a.tok[blockIdx.x] = t;
            if (a.tok2) a.tok2[blockIdx.x] = t;
        } else {
            const uint32_t r = seq;
            a.tok[a.tok_stride ? (size_t)r * a.tok_stride + at : (size_t)r] = t;
            if (a.tok2) a.tok2[blockIdx.x] = t;
            if (a.length) a.length[r] = at + 1u;
            if (a.counts) {
                uint32_t * c = a.counts + (size_t)r * (size_t)V + t;
                *c = *c + 1u;  // no other workgroup touches row r
            }
            bool stop = false;
#pragma unroll
            for (int j = 0; j < SAMPLE_MAX_STOP; j++) stop = stop || (j < a.n_stop && a.stop[j] == t);
            if (stop && a.done) {
                a.done[r] = 1u;
                if (a.fin_step) a.fin_step[r] = a.step;
                if (a.active) atomicSub(a.active, 1u);
            } else if (a.lane_seq && a.max_tokens && a.active && at + 1u >= a.max_tokens[r]) {
                atomicSub(a.active, 1u);  // ended by its cap: the next turnover retires it
            }
        }
    };
    for (int j = tid; j < nb; j += SM_THREADS) {
        sh.bid[j] = a.bias_ids[j];
        sh.bval[j] = a.bias_vals[j];
    }
    if (tid == 0) sh.sel = 0x7fffffff;
    __syncthreads();

    float v[SM_REGS];
#pragma unroll
    for (int k = 0; k < SM_REGS; k++) {
        const int i = k * SM_THREADS + tid;
        const float x = lg[min(i, V - 1)];  // a clamped load and a select: no branch per element
        v[k] = i < V ? x : NEG_INF;
    }
    if constexpr (ROWS) {
        if (pen.pen) {
#pragma unroll
            for (int k = 0; k < SM_REGS; k++) {
                const int i = k * SM_THREADS + tid;
                if (i < V) v[k] = sm_penalized(pen, v[k], i);
            }
        }
    }
    for (int j = 0; j < nb; j++) {
        const uint32_t id = sh.bid[j];
        if ((id & (SM_THREADS - 1)) == (uint32_t)tid && id < (uint32_t)(SM_REGS * SM_THREADS)) {
            const int kk = (int)(id >> 10);
            const float b = sh.bval[j];
#pragma unroll
            for (int k = 0; k < SM_REGS; k++) v[k] = k == kk ? v[k] + b : v[k];
        }
    }

    // ---- 1. maximum and the lowest index holding it (np.argmax; NaN never wins)
    float bv = NEG_INF;
    int bi = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < SM_REGS; k++) {
        const int i = k * SM_THREADS + tid;
        if (v[k] > bv) bv = v[k], bi = i;
    }
    for (int i = SM_REGS * SM_THREADS + tid; i < V; i += SM_THREADS) {
        const float x = biased(i);
        if (x > bv) bv = x, bi = i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    if (lane == 0) sh.amax_v[wave] = bv, sh.amax_i[wave] = bi;
    __syncthreads();
    bv = sh.amax_v[0], bi = sh.amax_i[0];
#pragma unroll
    for (int w = 1; w < SM_WAVES; w++) {
        const float ov = sh.amax_v[w];
        const int oi = sh.amax_i[w];
        if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    const float m = bv;
    if (temperature == 0.0f) {
        if (tid == 0) {
            const uint32_t t = (uint32_t)min(max(bi == 0x7fffffff ? 0 : bi, 0), V - 1);
            emit(t);
            if (a.kept) a.kept[blockIdx.x] = 1;
            if (a.cutoff) a.cutoff[blockIdx.x] = 0.0f;
        }
        return;
    }

    // ---- 2. e = exp(l - m) (0 outside the row), S = sum e
#pragma unroll
    for (int k = 0; k < SM_REGS; k++) {
        const int i = k * SM_THREADS + tid;
        v[k] = i < V ? expf(v[k] - m) : 0.0f;
    }
    // sum of the e whose bit pattern is >= cb, over this thread's elements: 64 serial adds, then
    // one more per further 64 rows
    auto thread_mass = [&](uint32_t cb) -> float {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < SM_REGS; k++) acc += __float_as_uint(v[k]) >= cb ? v[k] : 0.0f;
        for (int k0 = SM_REGS; k0 < nrows; k0 += SM_REGS) {
            float p = 0.0f;
            const int k1 = min(k0 + SM_REGS, nrows);
            for (int k = k0; k < k1; k++) {
                const int i = k * SM_THREADS + tid;
                if (i < V) {
                    const float e = expf(biased(i) - m);
                    p += __float_as_uint(e) >= cb ? e : 0.0f;
                }
            }
            acc += p;
        }
        return acc;
    };
    const float S = sm_block_sum(thread_mass(0u), sh, phase);

    // ---- 3. the top-p cutoff: the largest bit pattern cb with mass(cb) > top_p * S.  mass() is a
    // fixed-association sum of non-negative terms, so it is monotone in cb and the search is exact;
    // the result is the bit pattern of an element (mass only changes there).
    uint32_t cb = 0u;
    if (top_p > 0.0f && top_p < 1.0f) {
        const float target = top_p * S;
        uint32_t lo = 0u, hi = 0x3f800001u;  // e <= 1: mass(hi) = 0
        for (int it = 0; it < 31 && hi - lo > 1u; it++) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const float mass = sm_block_sum(thread_mass(mid), sh, phase);
            if (mass > target) lo = mid;
            else hi = mid;
        }
        cb = lo;
    }

    // ---- 4. weights of the kept elements; their count and the largest kept index
    const bool t1 = temperature == 1.0f;
    int cnt = 0, last = -1;
#pragma unroll
    for (int k = 0; k < SM_REGS; k++) {
        const int i = k * SM_THREADS + tid;
        float w = 0.0f;
        if (i < V && __float_as_uint(v[k]) >= cb) {
            cnt++;
            last = i;
            w = t1 ? v[k] : expf((biased(i) - m) / temperature);
        }
        v[k] = w;
    }
    auto tail_w = [&](int i, bool count) -> float {
        if (i >= V) return 0.0f;
        const float d = biased(i) - m, e = expf(d);
        if (__float_as_uint(e) < cb) return 0.0f;
        if (count) cnt++, last = i;
        return t1 ? e : expf(d / temperature);
    };
    // (row, wave) totals in vocabulary order: entry k * 16 + wave covers indices k * 1024 + wave * 64 + lane
#pragma unroll
    for (int k = 0; k < SM_REGS; k++) {
        const float t = wave_sum63(v[k]);
        if (lane == 63) sh.tab[k * SM_WAVES + wave] = t;
    }
    for (int k = SM_REGS; k < nrows; k++) {
        const float t = wave_sum63(tail_w(k * SM_THREADS + tid, true));
        if (lane == 63) sh.tab[k * SM_WAVES + wave] = t;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        last = max(last, __shfl_xor(last, o));
    }
    if (lane == 0) sh.cnt[wave] = cnt, sh.last[wave] = last;
    __syncthreads();
    cnt = 0, last = -1;
#pragma unroll
    for (int w = 0; w < SM_WAVES; w++) cnt += sh.cnt[w], last = max(last, sh.last[w]);

    // inclusive prefix sums of the table, 1024 entries a pass (one pass up to 65536 logits)
    const int E = nrows * SM_WAVES;
    float carry = 0.0f;
    for (int e0 = 0; e0 < E; e0 += SM_THREADS) {
        const int e = e0 + tid;
        float x = e < E ? sh.tab[e] : 0.0f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float t = __shfl_up(x, o);
            if (lane >= o) x += t;
        }
        if (lane == 63) sh.wtot[wave] = x;
        __syncthreads();
        float off = carry, tot = carry;
#pragma unroll
        for (int w = 0; w < SM_WAVES; w++) {
            tot += sh.wtot[w];
            if (w + 1 == wave) off = tot;
        }
        if (e < E) sh.tab[e] = off + x;
        carry = tot;
        __syncthreads();
    }
    const float Z = carry;

    // ---- 5. the draw
    float u;
    if (a.u) u = a.u[blockIdx.x];
    else if (ROWS && a.seed_r && a.counter_r) u = sample_uniform(a.seed_r[seq], a.counter_r[seq] + (a.lane_seq ? at : a.counter));
    else u = sample_uniform(a.seed, a.counter + blockIdx.x);
    const float target = u * Z;
    for (int e = tid; e < E; e += SM_THREADS)
        if (sh.tab[e] > target) atomicMin(&sh.sel, e);
    __syncthreads();
    const int sel = sh.sel;
    if (a.kept && tid == 0) a.kept[blockIdx.x] = (uint32_t)cnt;
    if (a.cutoff && tid == 0) a.cutoff[blockIdx.x] = __uint_as_float(cb) / S;
    int token = last;  // rounding left no index past u * Z: the largest kept index
    if (sel != 0x7fffffff) {
        if (wave != (sel & (SM_WAVES - 1))) return;
        const int ks = sel / SM_WAVES;
        float x = 0.0f;
        if (ks < SM_REGS) {
#pragma unroll
            for (int k = 0; k < SM_REGS; k++)
                if (k == ks) x = v[k];
        } else {
            x = tail_w(ks * SM_THREADS + tid, false);
        }
        const float base = sel > 0 ? sh.tab[sel - 1] : 0.0f;
        float c = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float t = __shfl_up(c, o);
            if (lane >= o) c += t;
        }
        // only elements with weight can be drawn, whatever the rounding of the prefix sums
        const unsigned long long pos = __ballot(x > 0.0f), hit = __ballot(x > 0.0f && base + c > target);
        const int first = ks * SM_THREADS + (sel & (SM_WAVES - 1)) * 64;
        if (hit) token = first + (__ffsll((long long)hit) - 1);
        else if (pos) token = first + (63 - __clzll((long long)pos));
        if (lane != 0) return;
    } else if (tid != 0) {
        return;
    }
    emit((uint32_t)min(max(token, 0), V - 1));
}

__global__ __launch_bounds__(SM_THREADS) void k_sample(const SampleArgs a) {
    __shared__ SampleShared sh;
    sample_row<false, false>(a, sh);
}

__global__ __launch_bounds__(SM_THREADS) void k_sample_rows(const SampleArgs a) {
    __shared__ SampleShared sh;
    sample_row<true, false>(a, sh);
}

__global__ __launch_bounds__(SM_THREADS) void k_sample_lp(const SampleArgs a) {
    __shared__ SampleShared sh;
    sample_row<false, true>(a, sh);
}

__global__ __launch_bounds__(SM_THREADS) void k_sample_rows_lp(const SampleArgs a) {
    __shared__ SampleShared sh;
    sample_row<true, true>(a, sh);
}

// ---- batched generation: the rows' snapshots ------------------------------------------------
// Copies n floats from src to dst with 16-byte loads and stores; the workgroup takes part `part` of
// `parts`.  src and dst are at the same offset from 16-byte aligned buffers (row r of [rows][n]
// arrays), so one scalar head aligns both; n need not be a multiple of 4 (odd vocabularies).
__device__ __forceinline__ void gen_copy_row(float * dst, const float * src, size_t n, int part, int parts) {
    const size_t head = min(n, (size_t)((4 - (((uintptr_t)src >> 2) & 3)) & 3));
    const size_t nvec = (n - head) / 4, tail = head + nvec * 4;
    if (part == 0) {
        for (size_t i = threadIdx.x; i < head; i += blockDim.x) dst[i] = src[i];
        for (size_t i = tail + threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
    }
    const float4 * s4 = (const float4 *)(src + head);
    float4 * d4 = (float4 *)(dst + head);
    for (size_t i = (size_t)part * blockDim.x + threadIdx.x; i < nvec; i += (size_t)parts * blockDim.x) d4[i] = s4[i];
}

// The same between rows of different indices (a queue's lane r and sequence s).  With n a multiple of
// 4 every row of a [rows][n] array starts on 16 bytes and gen_copy_row's head and tail are empty;
// otherwise (an odd vocabulary) the two rows need not share an alignment and the floats go one by one.
// Either way element i of a row belongs to the same thread of the same part in every call with this
// n, which is what lets k_gen_move read a lane's row and then write over it without a barrier.
__device__ __forceinline__ void gen_move_row(float * dst, const float * src, size_t n, int part, int parts) {
    if ((n & 3) == 0) {
        gen_copy_row(dst, src, n, part, parts);
    } else {
        for (size_t i = (size_t)part * blockDim.x + threadIdx.x; i < n; i += (size_t)parts * blockDim.x) dst[i] = src[i];
    }
}

constexpr int GEN_THREADS = 256;

// grid (parts, rows)
__global__ __launch_bounds__(GEN_THREADS) void k_gen_snapshot(const GenRows g, uint32_t step, const float * state,
                                                              const float * logits, float * snap_state,
                                                              float * snap_logits) {
    const int r = blockIdx.y;
    if (g.lane_seq) {
        const uint32_t s = g.lane_seq[r];
        if (s == GEN_NONE || g.done[s] == 0 || g.fin_step[s] != step) return;
        gen_move_row(snap_state + (size_t)s * g.state_len, state + (size_t)r * g.state_len, g.state_len, blockIdx.x, gridDim.x);
        gen_move_row(snap_logits + (size_t)s * g.V, logits + (size_t)r * g.V, g.V, blockIdx.x, gridDim.x);
        return;
    }
    if (g.done[r] == 0 || g.fin_step[r] != step) return;
    gen_copy_row(snap_state + (size_t)r * g.state_len, state + (size_t)r * g.state_len, g.state_len, blockIdx.x, gridDim.x);
    gen_copy_row(snap_logits + (size_t)r * g.V, logits + (size_t)r * g.V, g.V, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(GEN_THREADS) void k_gen_restore(const GenRows g, const float * snap_state,
                                                             const float * snap_logits, const float * state_live,
                                                             float * state_final, float * logits) {
    const int r = blockIdx.y;
    if (g.done[r] != 0) {
        gen_copy_row(state_final + (size_t)r * g.state_len, snap_state + (size_t)r * g.state_len, g.state_len, blockIdx.x,
                     gridDim.x);
        gen_copy_row(logits + (size_t)r * g.V, snap_logits + (size_t)r * g.V, g.V, blockIdx.x, gridDim.x);
    } else if (state_live != state_final) {
        gen_copy_row(state_final + (size_t)r * g.state_len, state_live + (size_t)r * g.state_len, g.state_len, blockIdx.x,
                     gridDim.x);
    }
}

// one workgroup of GEN_THREADS >= rows threads
__global__ __launch_bounds__(GEN_THREADS) void k_gen_begin(int rows, int keep, uint32_t * done, uint32_t * length,
                                                           uint32_t * fin_step, uint32_t * active) {
    __shared__ unsigned live;
    const int r = threadIdx.x;
    if (r == 0) live = 0u;
    __syncthreads();
    if (r < rows) {
        if (!keep) done[r] = 0u;
        length[r] = 0u;
        fin_step[r] = 0xffffffffu;
        if (keep == 0 || done[r] == 0u) atomicAdd(&live, 1u);
    }
    __syncthreads();
    if (r == 0) *active = live;
}

// ---- a queue of sequences over the lanes (rwkv_mi355x_generate_queue) ---------------
// One workgroup, thread r = lane r.  Rank of a free lane among the free lanes = a ballot's popcount
// below the lane plus the free lanes of the waves before it; the rank-th waiting sequence enters.
__global__ __launch_bounds__(GEN_THREADS) void k_gen_turnover(const GenQueue q, uint32_t step) {
    __shared__ unsigned wave_free[GEN_THREADS / 64], wave_busy[GEN_THREADS / 64];
    const int r = threadIdx.x, lane = r & 63, wave = r >> 6;
    const bool in = r < q.lanes;
    const uint32_t first = *q.next;  // read by every thread before the barrier, written after it
    uint32_t s = GEN_NONE;
    bool capped = false, ended = false;
    if (in) s = q.lane_seq[r];
    if (s != GEN_NONE) {
        const bool stopped = q.done[s] != 0;
        capped = !stopped && q.length[s] >= q.max_tokens[s];
        ended = stopped || capped;
    }
    const bool is_free = in && (s == GEN_NONE || ended);
    const unsigned long long fb = __ballot(is_free), bb = __ballot(in && !is_free);
    if (lane == 0) wave_free[wave] = (unsigned)__popcll(fb), wave_busy[wave] = (unsigned)__popcll(bb);
    __syncthreads();
    unsigned rank = (unsigned)__popcll(fb & ((1ull << lane) - 1ull)), n_free = 0, n_busy = 0;
#pragma unroll
    for (int w = 0; w < GEN_THREADS / 64; w++) {
        if (w < wave) rank += wave_free[w];
        n_free += wave_free[w];
        n_busy += wave_busy[w];
    }
    const uint32_t waiting = first < (uint32_t)q.Q ? (uint32_t)q.Q - first : 0u;
    const bool admit = is_free && rank < waiting;
    const uint32_t from = admit ? first + rank : GEN_NONE;
    if (in) {
        q.retire_to[r] = capped ? s : GEN_NONE;
        q.admit_from[r] = from;
        if (capped) q.done[s] = 1u;
        if (is_free) q.lane_seq[r] = from;
        if (admit) {
            q.lane[from] = (uint32_t)r;
            q.start[from] = step;
        }
    }
    if (r == 0) {
        const uint32_t admitted = min(n_free, waiting);
        *q.next = first + admitted;
        *q.active = waiting + n_busy;  // waiting - admitted still wait, n_busy + admitted are in lanes
    }
}

// grid (parts, lanes).  Both copies of a lane give element i of its row to the same thread
// (gen_move_row), so the admission's stores follow the retirement's loads in program order.
__global__ __launch_bounds__(GEN_THREADS) void k_gen_move(const GenQueue q, size_t state_len, size_t V, float * state,
                                                          float * logits, const float * slot_state, float * snap_state,
                                                          float * snap_logits) {
    const int r = blockIdx.y;
    const uint32_t to = q.retire_to[r], from = q.admit_from[r];
    float * st = state + (size_t)r * state_len;
    float * lg = logits + (size_t)r * V;
    if (to != GEN_NONE) {
        gen_move_row(snap_state + (size_t)to * state_len, st, state_len, blockIdx.x, gridDim.x);
        gen_move_row(snap_logits + (size_t)to * V, lg, V, blockIdx.x, gridDim.x);
    }
    if (from != GEN_NONE) {
        const float * sst = slot_state + (size_t)from * state_len;
        const float * slg = logits + (size_t)from * V;
        if (sst != st) gen_move_row(st, sst, state_len, blockIdx.x, gridDim.x);
        if (slg != lg) gen_move_row(lg, slg, V, blockIdx.x, gridDim.x);
    }
}

}  // namespace

bool launch_sample(hipStream_t st, const SampleArgs & a) {
    if (!a.logits || !a.tok || a.rows < 1 || a.V < 1 || a.V > SAMPLE_MAX_VOCAB) return false;
    if (a.n_bias < 0 || a.n_bias > SAMPLE_MAX_BIAS || (a.n_bias && (!a.bias_ids || !a.bias_vals))) return false;
    if (a.n_stop < 0 || a.n_stop > SAMPLE_MAX_STOP) return false;
    const bool rows = a.temperature_r || a.top_p_r || a.seed_r || a.counter_r || a.presence_r || a.frequency_r ||
                      a.counts || a.n_stop || a.done || a.length || a.fin_step || a.active || a.tok_stride || a.lane_seq;
    const bool lp = a.lp_token != nullptr;
    if (lp && !a.lp_logz) return false;  // k_logprobs leaves the row's logZ there
    if (rows) {
        if ((a.seed_r == nullptr) != (a.counter_r == nullptr)) return false;
        if (a.lane_seq && !a.length) return false;  // a queue's draw index is the sequence's length
        if (lp) RK_LAUNCH(k_sample_rows_lp, dim3((unsigned)a.rows), dim3(SM_THREADS), 0, st, a);
        else RK_LAUNCH(k_sample_rows, dim3((unsigned)a.rows), dim3(SM_THREADS), 0, st, a);
    } else {
        if (lp) RK_LAUNCH(k_sample_lp, dim3((unsigned)a.rows), dim3(SM_THREADS), 0, st, a);
        else RK_LAUNCH(k_sample, dim3((unsigned)a.rows), dim3(SM_THREADS), 0, st, a);
    }
    HIP_OK(hipGetLastError());
    return true;
}

// parts of a row: about 8 vectors a thread, at most 32 workgroups
static unsigned gen_parts(size_t state_len, size_t V) {
    const size_t vec = (state_len + V) / 4 + 1;
    return (unsigned)std::min<size_t>(32, std::max<size_t>(1, vec / (GEN_THREADS * 8)));
}

static bool gen_rows_ok(const GenRows & g) {
    return g.rows >= 1 && g.rows <= 65535 && g.done && g.fin_step && g.state_len >= 1 && g.V >= 1;
}

bool launch_gen_snapshot(hipStream_t st, const GenRows & g, uint32_t step, const float * state, const float * logits,
                         float * snap_state, float * snap_logits) {
    if (!gen_rows_ok(g) || !state || !logits || !snap_state || !snap_logits) return false;
    RK_LAUNCH(k_gen_snapshot, dim3(gen_parts(g.state_len, g.V), (unsigned)g.rows), dim3(GEN_THREADS), 0, st, g, step, state, logits,
              snap_state, snap_logits);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_gen_restore(hipStream_t st, const GenRows & g, const float * snap_state, const float * snap_logits,
                        const float * state_live, float * state_final, float * logits) {
    if (!gen_rows_ok(g) || !snap_state || !snap_logits || !state_live || !state_final || !logits) return false;
    RK_LAUNCH(k_gen_restore, dim3(gen_parts(g.state_len, g.V), (unsigned)g.rows), dim3(GEN_THREADS), 0, st, g, snap_state, snap_logits,
              state_live, state_final, logits);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_gen_begin(hipStream_t st, int rows, int keep, uint32_t * done, uint32_t * length, uint32_t * fin_step,
                      uint32_t * active) {
    if (rows < 1 || rows > GEN_THREADS || !done || !length || !fin_step || !active) return false;
    RK_LAUNCH(k_gen_begin, dim3(1), dim3(GEN_THREADS), 0, st, rows, keep, done, length, fin_step, active);
    HIP_OK(hipGetLastError());
    return true;
}

static bool gen_queue_ok(const GenQueue & q) {
    return q.lanes >= 1 && q.lanes <= GEN_THREADS && q.Q >= 1 && q.lane_seq && q.done && q.length && q.max_tokens &&
           q.lane && q.start && q.retire_to && q.admit_from && q.next && q.active;
}

bool launch_gen_turnover(hipStream_t st, const GenQueue & q, uint32_t step) {
    if (!gen_queue_ok(q)) return false;
    RK_LAUNCH(k_gen_turnover, dim3(1), dim3(GEN_THREADS), 0, st, q, step);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_gen_move(hipStream_t st, const GenQueue & q, size_t state_len, size_t V, float * state, float * logits,
                     const float * slot_state, float * snap_state, float * snap_logits) {
    if (!gen_queue_ok(q) || state_len < 1 || V < 1 || !state || !logits || !slot_state || !snap_state || !snap_logits)
        return false;
    RK_LAUNCH(k_gen_move, dim3(gen_parts(state_len, V), (unsigned)q.lanes), dim3(GEN_THREADS), 0, st, q, state_len, V, state, logits,
              slot_state, snap_state, snap_logits);
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi
