// sample_row.hpp -- what the sampler (sample.hip) and the log-probability kernel (logprobs.hip) share:
// the row a workgroup works on and the float32 row l it samples from,
//
//   l_i = (logit_i - (presence + (float)c_i * frequency), where c_i > 0) + bias_i
//
// in the roundings of SampleArgs (kernels.hpp).  The penalty (sm_penalized) and l_i from memory
// (sm_biased) have this one copy, so the l a log-probability is taken of is, bit for bit, the l the
// token was drawn from.  sm_row_live and sm_load_row restate, for k_logprobs, what sample_row does in
// its own body (the finished-row test, and the register copy of l: the same penalty function, the same
// additions in the same order): called from sample_row they compile to the same arithmetic, but the
// register allocation of k_sample and k_sample_rows moves (one more spilled VGPR, six more spilled
// SGPRs), and those two kernels are not to move.
//
// One workgroup of SM_THREADS threads per row; thread t holds elements k * SM_THREADS + t (k <
// SM_REGS) in registers; the elements beyond them are re-formed from memory where they are needed.
#pragma once

#include "device_common.hpp"
#include "kernels.hpp"

namespace rwkvmi {

constexpr int SM_THREADS = 1024, SM_REGS = 64, SM_WAVES = 16;
constexpr int SM_MAX_ROWS = SAMPLE_MAX_VOCAB / SM_THREADS;

// The sequence of this workgroup's row and the index of its draw (a queue: SampleArgs::lane_seq).
// seq and at come in as the row and the step.  false: an idle lane or a finished row, which draws
// nothing.  Uniform over the workgroup.
__device__ __forceinline__ bool sm_row_live(const SampleArgs & a, uint32_t & seq, uint32_t & at) {
    bool idle = false;
    if (a.lane_seq) {
        seq = a.lane_seq[blockIdx.x];
        idle = seq == GEN_NONE;
        if (!idle) at = a.length[seq];
    }
    return !(idle || (a.done && a.done[seq] != 0));
}

// The penalties of sequence r over its count row; pen is uniform over the workgroup
struct SmPenalty {
    bool pen = false;
    float presence = 0.0f, frequency = 0.0f;
    const uint32_t * cnt_row = nullptr;
};

__device__ __forceinline__ void sm_row_penalty(const SampleArgs & a, uint32_t r, SmPenalty & p) {
    if (a.counts) {
        if (a.presence_r) p.presence = a.presence_r[r];
        if (a.frequency_r) p.frequency = a.frequency_r[r];
        p.pen = p.presence != 0.0f || p.frequency != 0.0f;
        p.cnt_row = a.counts + (size_t)r * (size_t)a.V;
    }
}

// the penalty of SampleArgs::counts: exactly one multiply, one add, one subtract in float32
__device__ __forceinline__ float sm_penalized(const SmPenalty & p, float x, int i) {
    const uint32_t c = p.cnt_row[i];
    return c > 0u ? __fsub_rn(x, __fadd_rn(p.presence, __fmul_rn((float)c, p.frequency))) : x;
}

// l_i from memory: the same operations in the same order as the register copy of sm_load_row
// (bid / bval: the nb bias entries, in LDS)
template <bool ROWS>
__device__ __forceinline__ float sm_biased(const float * lg, const SmPenalty & p, int nb, const uint32_t * bid,
                                           const float * bval, int i) {
    float x = lg[i];
    if constexpr (ROWS) {
        if (p.pen) x = sm_penalized(p, x, i);
    }
    for (int j = 0; j < nb; j++)
        if (bid[j] == (uint32_t)i) x += bval[j];
    return x;
}

// v[k] = l_i of element i = k * SM_THREADS + tid, -inf beyond the row
template <bool ROWS>
__device__ __forceinline__ void sm_load_row(float (&v)[SM_REGS], const float * lg, int V, const SmPenalty & p, int nb,
                                            const uint32_t * bid, const float * bval) {
    const int tid = threadIdx.x;
    const float NEG_INF = __int_as_float(0xff800000);
#pragma unroll
    for (int k = 0; k < SM_REGS; k++) {
        const int i = k * SM_THREADS + tid;
        const float x = lg[min(i, V - 1)];  // a clamped load and a select: no branch per element
        v[k] = i < V ? x : NEG_INF;
    }
    if constexpr (ROWS) {
        if (p.pen) {
#pragma unroll
            for (int k = 0; k < SM_REGS; k++) {
                const int i = k * SM_THREADS + tid;
                if (i < V) v[k] = sm_penalized(p, v[k], i);
            }
        }
    }
    for (int j = 0; j < nb; j++) {
        const uint32_t id = bid[j];
        if ((id & (SM_THREADS - 1)) == (uint32_t)tid && id < (uint32_t)(SM_REGS * SM_THREADS)) {
            const int kk = (int)(id >> 10);
            const float b = bval[j];
#pragma unroll
            for (int k = 0; k < SM_REGS; k++) v[k] = k == kk ? v[k] + b : v[k];
        }
    }
}

}  // namespace rwkvmi
