// logprobs.hip -- log-probabilities of a draw (rwkv_mi355x_*_logprobs): k_logprobs runs directly in
// front of the sampler, on the sampler's own arguments, and sees what the sampler is about to see:
// the logits, the counts before the draw's increment, done, the idle lanes and length[s].  Per live
// row, with l the float32 row the sampler draws from (sample_row.hpp: penalties, then bias; the same
// code, so the same bits):
//
//   m      = max l, exact in fp32 (NaN never wins)
//   S      = sum_i exp((double)l_i - (double)m), exponentials and sum in fp64
//   logZ   = (double)m + log(S)                     -> lp_logz[row]: the sampler's LP form subtracts
//                                                      this word from l[token] (sample.hip, emit)
//   top j  = the j-th element in the order "larger l first, lower index first among equal l", exact
//            fp32 compares; a NaN is never listed     -> lp_top_ids, lp_top = (double)l - logZ
//
// One workgroup of 1024 threads per row in the sampler's layout: thread t holds elements k * 1024 + t
// (k < 64) in registers, the elements from 65536 on are re-formed from memory in each pass.
//
// The sum has one fixed association and no atomics (k_xent's): per thread a serial chain over its
// elements, k ascending; wave_sum63_d's 6 DPP levels; a 4-level tree over the 16 waves.
//
// Selection: round j is a block arg-max over the elements strictly after winner j - 1 in the order
// above.  Every thread keeps its own best such element as a candidate; a round reduces the 1024
// candidates (6 shuffle levels, one 16-entry LDS line, double-buffered: one barrier a round), and only
// the thread that held the winner looks for its next candidate -- the others' candidates lost to the
// winner, so they are after it already.  A round that finds no candidate (fewer non-NaN elements than
// lp_k) ends the kernel, and the entries left keep what the caller put there.
//
// A call is a pure function of its inputs.  Non-finite logits give NaN or inf values and cannot hang,
// fault or index outside the row: every loop has a fixed bound and every index listed is < V.
#include "device_common.hpp"
#include "kernels.hpp"
#include "sample_row.hpp"

namespace rwkvmi {

namespace {

struct LogprobsShared {
    uint32_t bid[SAMPLE_MAX_BIAS];
    float bval[SAMPLE_MAX_BIAS];
    float mx[SM_WAVES];
    double red[SM_WAVES];
    float best_v[2][SM_WAVES];  // a round's wave winners, double-buffered (one barrier per round)
    int best_i[2][SM_WAVES];
};

constexpr int LP_NONE = 0x7fffffff;  // no candidate; as an index it loses every tie

// (x, i) comes before (y, j): larger l first, lower index first among equal l.  False for a NaN x.
__device__ __forceinline__ bool lp_before(float x, int i, float y, int j) { return x > y || (x == y && i < j); }

__global__ __launch_bounds__(SM_THREADS) void k_logprobs(const SampleArgs a) {
    __shared__ LogprobsShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V, nb = a.n_bias;
    const float NEG_INF = __int_as_float(0xff800000), POS_INF = __int_as_float(0x7f800000);
    uint32_t seq = blockIdx.x, at = a.step;
    if (!sm_row_live(a, seq, at)) return;  // the sampler draws nothing for this row
    SmPenalty pen;
    sm_row_penalty(a, seq, pen);
    const float * lg = a.logits + (size_t)blockIdx.x * (size_t)V;
    for (int j = tid; j < nb; j += SM_THREADS) {
        sh.bid[j] = a.bias_ids[j];
        sh.bval[j] = a.bias_vals[j];
    }
    __syncthreads();
    auto biased = [&](int i) -> float { return sm_biased<true>(lg, pen, nb, sh.bid, sh.bval, i); };
    float v[SM_REGS];
    sm_load_row<true>(v, lg, V, pen, nb, sh.bid, sh.bval);

    // ---- m
    float mv = NEG_INF;
#pragma unroll
    for (int k = 0; k < SM_REGS; k++)
        if (v[k] > mv) mv = v[k];
    for (int i = SM_REGS * SM_THREADS + tid; i < V; i += SM_THREADS) {
        const float x = biased(i);
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
    for (int w = 1; w < SM_WAVES; w++)
        if (sh.mx[w] > mv) mv = sh.mx[w];
    const double m = (double)mv;

    // ---- S and logZ (thread 0 has it)
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < SM_REGS; k++)
        if (k * SM_THREADS + tid < V) acc += exp((double)v[k] - m);
    for (int i = SM_REGS * SM_THREADS + tid; i < V; i += SM_THREADS) acc += exp((double)biased(i) - m);
    acc = wave_sum63_d(acc);
    if (lane == 63) sh.red[wave] = acc;
    __syncthreads();
    double logZ = 0.0;
    if (tid == 0) {
        double t[SM_WAVES];
#pragma unroll
        for (int i = 0; i < SM_WAVES; i++) t[i] = sh.red[i];
#pragma unroll
        for (int s = 1; s < SM_WAVES; s *= 2)
#pragma unroll
            for (int i = 0; i < SM_WAVES; i += 2 * s) t[i] += t[i + s];
        logZ = m + log(t[0]);
        a.lp_logz[blockIdx.x] = logZ;
    }

    // ---- the lp_k leading elements
    const int K = min(a.lp_k, LOGPROBS_MAX_TOP);
    if (K <= 0) return;
    const size_t col = a.tok_stride ? (size_t)seq * a.tok_stride + at : (size_t)seq;
    float pv = POS_INF;  // the previous winner: everything that is not a NaN comes after (+inf, -1)
    int pi = -1;
    float cv;  // this thread's candidate: its first element after the previous winner
    int ci;
    // One wave runs this while fifteen wait at the round's barrier, so it is straight-line code: the
    // tests are combined with & and | (no short-circuit, no branch per element) into two selects.  The
    // indices ascend with k, so among equal values the first one met is the one to keep: `x > cv`, and
    // `ci == LP_NONE` lets a -inf element in while there is no candidate yet.
    auto rescan = [&] {
        cv = NEG_INF, ci = LP_NONE;
#pragma unroll
        for (int k = 0; k < SM_REGS; k++) {
            const int i = k * SM_THREADS + tid;
            const float x = v[k];
            const bool after = (pv > x) | ((pv == x) & (pi < i));
            const bool take = (i < V) & after & ((x > cv) | (ci == LP_NONE));
            cv = take ? x : cv;
            ci = take ? i : ci;
        }
        for (int i = SM_REGS * SM_THREADS + tid; i < V; i += SM_THREADS) {
            const float x = biased(i);
            if (lp_before(pv, pi, x, i) && lp_before(x, i, cv, ci)) cv = x, ci = i;
        }
    };
    rescan();
    for (int j = 0; j < K; j++) {
        float bv = cv;
        int bi = ci;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (lp_before(ov, oi, bv, bi)) bv = ov, bi = oi;
        }
        if (lane == 0) sh.best_v[j & 1][wave] = bv, sh.best_i[j & 1][wave] = bi;
        __syncthreads();
        bv = sh.best_v[j & 1][0], bi = sh.best_i[j & 1][0];
#pragma unroll
        for (int w = 1; w < SM_WAVES; w++) {
            const float ov = sh.best_v[j & 1][w];
            const int oi = sh.best_i[j & 1][w];
            if (lp_before(ov, oi, bv, bi)) bv = ov, bi = oi;
        }
        if (bi == LP_NONE) return;  // uniform: nothing but NaNs is left
        if (tid == 0) {
            a.lp_top_ids[col * (size_t)K + j] = (uint32_t)bi;
            a.lp_top[col * (size_t)K + j] = (double)bv - logZ;
        }
        pv = bv, pi = bi;
        if ((bi & (SM_THREADS - 1)) == tid) rescan();
    }
}

}  // namespace

bool launch_logprobs(hipStream_t st, const SampleArgs & a) {
    if (!a.logits || !a.lp_logz || a.rows < 1 || a.V < 1 || a.V > SAMPLE_MAX_VOCAB) return false;
    if (a.n_bias < 0 || a.n_bias > SAMPLE_MAX_BIAS || (a.n_bias && (!a.bias_ids || !a.bias_vals))) return false;
    if (a.lp_k < 0 || a.lp_k > LOGPROBS_MAX_TOP || a.lp_k > a.V || (a.lp_k && (!a.lp_top_ids || !a.lp_top))) return false;
    if (a.lane_seq && !a.length) return false;
    RK_LAUNCH(k_logprobs, dim3((unsigned)a.rows), dim3(SM_THREADS), 0, st, a);
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi
