// beam.hip -- beam search on the device (rwkv_mi355x_generate_beam): what runs between two
// batched decode steps over the W <= 16 beams of a call.
//
//   k_beam_rows    one workgroup per beam: logZ of its logits row and the row's W best elements, as
//                  W candidate records (score, beam, token).  The W best of all W x V candidates lie in
//                  the union of the rows' W best, so nothing ever compares W x V values.
//   k_beam_select  one workgroup: the exact rank of each of the <= W^2 records; the W first are the new
//                  beams (parent, token, score, finished, length), one line of history, the token row
//                  of the decode step and the number of live beams.
//   k_beam_gather  the state reorder: row j of the step's input buffer = row parent[j] of the buffer
//                  the last step wrote, 16 bytes a lane, finished beams left out.
//   k_beam_finish  one thread per beam walks the history back into its token row.
//
// A candidate (b, v) of a live beam b with float32 logits row l scores s_b + ((double)l_v - logZ_b),
//   m = max l (exact, a NaN never wins), S = sum_i exp((double)l_i - (double)m), logZ = (double)m + log(S)
// with k_logprobs' association of S (logprobs.hip: per thread a serial chain, k ascending;
// wave_sum63_d; a 4-level tree over the 16 waves), so a beam's score is the sum of the words
// rwkv_mi355x_*_logprobs reports for its tokens.  A finished beam has one candidate, itself.  Order:
// larger score first (doubles, compared exactly), then lower b, then lower v (a finished beam: v = 0).
//
// k_beam_rows is k_logprobs without penalties, bias and the sampler's words; its load, reductions and
// arg-max rounds are restated here, not shared, as sample_filter.hip restates sample_row: k_logprobs'
// register allocation is not to move, and a 1024-thread workgroup that keeps 64 elements a
// thread has no registers to spare for a shared helper's options (profiles/beam_resources.txt).
//
// A call is a pure function of its inputs.  Non-finite logits give unspecified beams and cannot hang,
// fault or index outside a row: every loop has a fixed bound, every token written is < V, every parent
// < W.
#include "device_common.hpp"
#include "kernels.hpp"

namespace rwkvmi {

namespace {

constexpr int BM_THREADS = 1024, BM_REGS = 64, BM_WAVES = 16;
constexpr int BM_NONE = 0x7fffffff;  // no candidate; as an index it loses every tie
constexpr int BM_W = BEAM_MAX_WIDTH, BM_RECS = BM_W * BM_W;

struct BeamRowShared {
    float mx[BM_WAVES];
    double red[BM_WAVES];
    float best_v[2][BM_WAVES];  // a round's wave winners, double-buffered (one barrier per round)
    int best_i[2][BM_WAVES];
};

// (x, i) comes before (y, j): larger l first, lower index first among equal l.  False for a NaN x.
__device__ __forceinline__ bool bm_before(float x, int i, float y, int j) { return x > y || (x == y && i < j); }

__global__ __launch_bounds__(BM_THREADS) void k_beam_rows(const BeamArgs a) {
    __shared__ BeamRowShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V, W = a.W, b = blockIdx.x;
    const float NEG_INF = __int_as_float(0xff800000), POS_INF = __int_as_float(0x7f800000);
    BeamRec * rec = a.rec + (size_t)b * BM_W;
    const uint32_t flag = a.finished[b];  // uniform
    if (flag != BEAM_LIVE) {
        // a finished beam is its own single candidate; an empty one has none.  The logits are not read.
        if (tid == 0) {
            if (flag == BEAM_FINISHED) rec[0] = BeamRec{a.score[b], (uint32_t)b, 0u};
            a.nrec[b] = flag == BEAM_FINISHED ? 1u : 0u;
        }
        return;
    }
    if (tid == 0) a.nrec[b] = 0u;
    const float * lg = a.logits + (size_t)b * (size_t)V;
    float v[BM_REGS];
#pragma unroll
    for (int k = 0; k < BM_REGS; k++) {
        const int i = k * BM_THREADS + tid;
        const float x = lg[min(i, V - 1)];  // a clamped load and a select: no branch per element
        v[k] = i < V ? x : NEG_INF;
    }

    // ---- m
    float mv = NEG_INF;
#pragma unroll
    for (int k = 0; k < BM_REGS; k++)
        if (v[k] > mv) mv = v[k];
    for (int i = BM_REGS * BM_THREADS + tid; i < V; i += BM_THREADS) {
        const float x = lg[i];
        if (x > mv) mv = x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(mv, o);
        if (ov > mv) mv = ov;
    }
    if (lane == 0) sh.mx[wave] = mv;
    __syncthreads();
    mv = sh.mx[0];
#pragma unroll
    for (int w = 1; w < BM_WAVES; w++)
        if (sh.mx[w] > mv) mv = sh.mx[w];
    const double m = (double)mv;

    // ---- S and logZ (thread 0 has it: it writes the records)
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < BM_REGS; k++)
        if (k * BM_THREADS + tid < V) acc += exp((double)v[k] - m);
    for (int i = BM_REGS * BM_THREADS + tid; i < V; i += BM_THREADS) acc += exp((double)lg[i] - m);
    acc = wave_sum63_d(acc);
    if (lane == 63) sh.red[wave] = acc;
    __syncthreads();
    double logZ = 0.0;
    if (tid == 0) {
        double t[BM_WAVES];
#pragma unroll
        for (int i = 0; i < BM_WAVES; i++) t[i] = sh.red[i];
#pragma unroll
        for (int s = 1; s < BM_WAVES; s *= 2)
#pragma unroll
            for (int i = 0; i < BM_WAVES; i += 2 * s) t[i] += t[i + s];
        logZ = m + log(t[0]);
    }

    // ---- the W leading elements: round j is a block arg-max over the elements after winner j - 1
    float pv = POS_INF;  // the previous winner: everything that is not a NaN comes after (+inf, -1)
    int pi = -1;
    float cv;  // this thread's candidate: its first element after the previous winner
    int ci;
    // One wave runs this while fifteen wait at the round's barrier, so it is straight-line code: two
    // selects per element, no branch.  The indices ascend with k, so among equal values the first one
    // met is the one to keep: `x > cv`, and `ci == BM_NONE` lets a -inf element in while there is none.
    auto rescan = [&] {
        cv = NEG_INF, ci = BM_NONE;
#pragma unroll
        for (int k = 0; k < BM_REGS; k++) {
            const int i = k * BM_THREADS + tid;
            const float x = v[k];
            const bool after = (pv > x) | ((pv == x) & (pi < i));
            const bool take = (i < V) & after & ((x > cv) | (ci == BM_NONE));
            cv = take ? x : cv;
            ci = take ? i : ci;
        }
        for (int i = BM_REGS * BM_THREADS + tid; i < V; i += BM_THREADS) {
            const float x = lg[i];
            if (bm_before(pv, pi, x, i) && bm_before(x, i, cv, ci)) cv = x, ci = i;
        }
    };
    rescan();
    for (int j = 0; j < W; j++) {
        float bv = cv;
        int bi = ci;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (bm_before(ov, oi, bv, bi)) bv = ov, bi = oi;
        }
        if (lane == 0) sh.best_v[j & 1][wave] = bv, sh.best_i[j & 1][wave] = bi;
        __syncthreads();
        bv = sh.best_v[j & 1][0], bi = sh.best_i[j & 1][0];
#pragma unroll
        for (int w = 1; w < BM_WAVES; w++) {
            const float ov = sh.best_v[j & 1][w];
            const int oi = sh.best_i[j & 1][w];
            if (bm_before(ov, oi, bv, bi)) bv = ov, bi = oi;
        }
        if (bi == BM_NONE) return;  // uniform: nothing but NaNs is left
        if (tid == 0) {
            rec[j] = BeamRec{a.score[b] + ((double)bv - logZ), (uint32_t)b, (uint32_t)bi};
            a.nrec[b] = (uint32_t)j + 1u;
        }
        pv = bv, pi = bi;
        if ((bi & (BM_THREADS - 1)) == tid) rescan();
    }
}

// Record x comes before record y: larger score, then lower beam, then lower token.  Exact compares; two
// records never share (b, v), so over records without a NaN score this is a strict total order.
__device__ __forceinline__ bool rec_before(double xs, uint32_t xb, uint32_t xv, double ys, uint32_t yb, uint32_t yv) {
    return xs > ys || (xs == ys && (xb < yb || (xb == yb && xv < yv)));
}

struct BeamSelectShared {
    double sc[BM_RECS];
    uint32_t rb[BM_RECS], rv[BM_RECS], valid[BM_RECS];
    // the beams before the step, and the new ones
    double old_score[BM_W], new_score[BM_W];
    uint32_t old_fin[BM_W], old_len[BM_W];
    uint32_t new_parent[BM_W], new_token[BM_W], new_fin[BM_W], new_len[BM_W];
};

// Thread t owns record slot t = b * 16 + k (row b's k-th best).  Its rank is the number of records that
// come before it: integers counted over LDS broadcasts, no sort, no arithmetic on the scores.
__global__ __launch_bounds__(BM_RECS) void k_beam_select(const BeamArgs a) {
    __shared__ BeamSelectShared sh;
    const int t = threadIdx.x, W = a.W;
    const int b = t / BM_W, k = t % BM_W;
    const bool valid = b < W && (uint32_t)k < min(a.nrec[b < W ? b : 0], (uint32_t)W);
    BeamRec r{0.0, 0u, 0u};
    if (valid) r = a.rec[t];
    sh.sc[t] = r.score, sh.rb[t] = r.b, sh.rv[t] = r.v, sh.valid[t] = valid ? 1u : 0u;
    if (t < W) {
        sh.old_score[t] = a.score[t], sh.old_fin[t] = a.finished[t], sh.old_len[t] = a.length[t];
        // a new beam no record reaches (fewer than W candidates: NaN rows only) is empty
        sh.new_parent[t] = (uint32_t)t, sh.new_token[t] = GEN_NONE, sh.new_fin[t] = BEAM_EMPTY, sh.new_len[t] = 0u;
        sh.new_score[t] = -__longlong_as_double(0x7ff0000000000000ll);
    }
    __syncthreads();
    int rank = 0;
    for (int u = 0; u < W * BM_W; u++)
        rank += (int)(sh.valid[u] && rec_before(sh.sc[u], sh.rb[u], sh.rv[u], r.score, r.b, r.v));
    if (valid && rank < W && r.b < (uint32_t)W) {
        const bool was_fin = sh.old_fin[r.b] == BEAM_FINISHED;
        bool stop = false;
        for (int s = 0; s < a.n_stop; s++) stop |= a.stop[s] == r.v;
        sh.new_parent[rank] = r.b;
        sh.new_token[rank] = was_fin ? GEN_NONE : r.v;
        sh.new_fin[rank] = (was_fin || stop) ? BEAM_FINISHED : BEAM_LIVE;
        sh.new_len[rank] = sh.old_len[r.b] + (was_fin ? 0u : 1u);
        sh.new_score[rank] = r.score;
    }
    __syncthreads();
    if (t < W) {
        const bool live = sh.new_fin[t] == BEAM_LIVE;
        a.parent[t] = sh.new_parent[t];
        a.token[t] = sh.new_token[t];
        a.score_out[t] = sh.new_score[t];
        a.finished_out[t] = sh.new_fin[t];
        a.length_out[t] = sh.new_len[t];
        a.hist[(size_t)a.step * (size_t)W + t] = make_uint2(sh.new_parent[t], sh.new_token[t]);
        a.dtok[t] = live ? sh.new_token[t] : 0u;  // a finished beam's row decodes token 0, as an idle lane
    }
    if (t == 0) {
        uint32_t n = 0;
        for (int j = 0; j < W; j++) n += sh.new_fin[j] == BEAM_LIVE ? 1u : 0u;
        *a.live = n;
    }
}

constexpr int BG_THREADS = 256, BG_UNROLL = 4;

// grid (chunks, W): row j of dst = row parent[j] of src, len floats.  The rows are 16-byte aligned when
// len % 4 == 0 (the launcher checks the bases); the floats past the last whole vector go one by one.
__global__ __launch_bounds__(BG_THREADS) void k_beam_gather(const float * src, float * dst, size_t len, int W,
                                                            const uint32_t * parent, const uint32_t * finished, int vec) {
    const int j = blockIdx.y;
    if (finished[j] != BEAM_LIVE) return;  // nothing reads a finished beam's state again
    const uint32_t p = parent[j];
    if (p >= (uint32_t)W) return;
    const float * s = src + (size_t)p * len;
    float * d = dst + (size_t)j * len;
    const size_t n4 = vec ? len / 4 : 0;
    const size_t stride = (size_t)gridDim.x * BG_THREADS;
    const float4 * s4 = (const float4 *)s;
    float4 * d4 = (float4 *)d;
    size_t i = (size_t)blockIdx.x * BG_THREADS + threadIdx.x;
    // BG_UNROLL loads in flight per lane before the first store
    for (; i + (BG_UNROLL - 1) * stride < n4; i += BG_UNROLL * stride) {
        const float4 x0 = s4[i], x1 = s4[i + stride], x2 = s4[i + 2 * stride], x3 = s4[i + 3 * stride];
        d4[i] = x0, d4[i + stride] = x1, d4[i + 2 * stride] = x2, d4[i + 3 * stride] = x3;
    }
    for (; i < n4; i += stride) d4[i] = s4[i];
    for (size_t e = n4 * 4 + (size_t)blockIdx.x * BG_THREADS + threadIdx.x; e < len; e += stride) d[e] = s[e];
}

// Thread j rebuilds tokens[j][0 .. length[j]) from the history, last step first, and fills the rest.
__global__ __launch_bounds__(64) void k_beam_finish(const BeamArgs a, uint32_t steps, uint32_t * tokens, size_t n) {
    const int j = threadIdx.x, W = a.W;
    if (j >= W) return;
    uint32_t * row = tokens + (size_t)j * n;
    const size_t len = min((size_t)a.length_out[j], n);
    for (size_t i = len; i < n; i++) row[i] = GEN_NONE;
    size_t pos = len;
    uint32_t cur = (uint32_t)j;
    for (uint32_t s = steps; s-- > 0;) {
        const uint2 h = a.hist[(size_t)s * (size_t)W + cur];
        if (h.y != GEN_NONE && pos > 0) row[--pos] = h.y;
        if (h.x >= (uint32_t)W) break;
        cur = h.x;
    }
    for (size_t i = 0; i < pos; i++) row[i] = GEN_NONE;  // unreachable for a history this call wrote
}

// score[0] = 0, beam 0 live; beams 1 .. W - 1 empty; every length 0
__global__ void k_beam_begin(double * score, uint32_t * finished, uint32_t * length, int W) {
    const int j = threadIdx.x;
    if (j >= W) return;
    score[j] = 0.0;
    finished[j] = j == 0 ? BEAM_LIVE : BEAM_EMPTY;
    length[j] = 0u;
}

bool beam_args_ok(const BeamArgs & a) {
    return a.W >= 1 && a.W <= BM_W && a.V >= 1 && a.n_stop >= 0 && a.n_stop <= 16 && a.score && a.finished && a.length &&
           a.rec && a.nrec;
}

}  // namespace

bool launch_beam_begin(hipStream_t st, const BeamArgs & a) {
    if (!beam_args_ok(a) || !a.score_out || !a.finished_out || !a.length_out) return false;
    RK_LAUNCH(k_beam_begin, dim3(1), dim3(64), 0, st, a.score_out, a.finished_out, a.length_out, a.W);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_beam_rows(hipStream_t st, const BeamArgs & a) {
    if (!beam_args_ok(a) || !a.logits) return false;
    RK_LAUNCH(k_beam_rows, dim3((unsigned)a.W), dim3(BM_THREADS), 0, st, a);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_beam_select(hipStream_t st, const BeamArgs & a) {
    if (!beam_args_ok(a) || !a.parent || !a.token || !a.score_out || !a.finished_out || !a.length_out || !a.hist ||
        !a.dtok || !a.live)
        return false;
    RK_LAUNCH(k_beam_select, dim3(1), dim3(BM_RECS), 0, st, a);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_beam_gather(hipStream_t st, const BeamArgs & a, const float * src, float * dst, size_t state_len) {
    if (!beam_args_ok(a) || !src || !dst || src == dst || state_len == 0 || !a.parent || !a.finished_out) return false;
    const int vec = state_len % 4 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0;
    // enough workgroups a row to fill the device at W = 1, each lane with BG_UNROLL vectors at least
    const size_t per = (size_t)BG_THREADS * BG_UNROLL * 4;
    const unsigned chunks = (unsigned)std::min<size_t>(256, (state_len + per - 1) / per);
    RK_LAUNCH(k_beam_gather, dim3(chunks, (unsigned)a.W), dim3(BG_THREADS), 0, st, src, dst, state_len, a.W, a.parent,
              a.finished_out, vec);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_beam_finish(hipStream_t st, const BeamArgs & a, uint32_t steps, uint32_t * tokens, size_t n) {
    if (!beam_args_ok(a) || !a.hist || !a.length_out || !tokens || n == 0) return false;
    RK_LAUNCH(k_beam_finish, dim3(1), dim3(64), 0, st, a, steps, tokens, n);
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi
