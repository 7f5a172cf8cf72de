// xent.hip -- cross-entropy and argmax of logits rows on the device (rwkv_mi355x_score_sequence):
// per row r of logits [rows][V] (fp32, row stride V)
//
//   m      = max l, exact in fp32
//   argmax = the lowest index holding m (np.argmax; NaN never wins), the tie rule of k_sample
//   S      = sum_i exp((double)l_i - (double)m), exponential and sum in fp64
//   loss   = (double)m + log(S) - (double)l[target]     (perplexity.cross_entropy)
//
// One workgroup of 1024 threads per row.  A row starts at any dword (V need not be a multiple of
// 4): up to 3 leading elements are peeled so that the body is 16-byte loads, thread t holding the
// float4s k * 1024 + t (k < 16: 65536 elements, every wave load 1 KiB contiguous) in registers for
// both passes; the float4s beyond them are read again in the second pass (the row then sits in
// L2), and up to 3 trailing elements follow as dwords.
//
// The sum has one fixed association and no atomics, so a call is a pure function of its inputs:
// per thread the serial chain peel element, register float4s (x, y, z, w; k ascending), streamed
// float4s, trailing element; then wave_sum63_d's 6 DPP levels; then a 4-level tree over the 16
// waves.  Non-finite logits give a NaN or inf loss and cannot hang or fault: every loop has a
// fixed bound, and argmax and target are clamped to the row.
#include "device_common.hpp"
#include "kernels.hpp"

namespace rwkvmi {

namespace {

constexpr int XE_THREADS = 1024, XE_VEC = 16, XE_WAVES = 16;

struct XentShared {
    float mv[XE_WAVES];
    int mi[XE_WAVES];
    double red[XE_WAVES];
};

__device__ __forceinline__ void xe_best(float x, int i, float & bv, int & bi) {
    if (x > bv || (x == bv && i < bi)) bv = x, bi = i;
}

__global__ __launch_bounds__(XE_THREADS) void k_xent(const float * __restrict__ logits, int V,
                                                     const uint32_t * __restrict__ targets,
                                                     double * __restrict__ loss, uint32_t * __restrict__ argmax) {
    __shared__ XentShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float * lg = logits + (size_t)blockIdx.x * (size_t)V;
    // [0, pre) peeled dwords, [pre, pre + 4 nvec) aligned float4s, [tail0, V) trailing dwords
    const int pre = min((int)(((16u - (unsigned)((uintptr_t)lg & 15u)) & 15u) >> 2), V);
    const int nvec = (V - pre) >> 2, tail0 = pre + 4 * nvec;
    const float4 * lv = reinterpret_cast<const float4 *>(lg + pre);
    const float NEG_INF = __int_as_float(0xff800000);

    // ---- 1. the maximum and the lowest index holding it
    float4 v[XE_VEC];
    float bv = NEG_INF;
    int bi = 0x7fffffff;
    if (tid < pre) xe_best(lg[tid], tid, bv, bi);
#pragma unroll
    for (int k = 0; k < XE_VEC; k++) {
        const int j = k * XE_THREADS + tid;
        v[k] = make_float4(NEG_INF, NEG_INF, NEG_INF, NEG_INF);
        if (j < nvec) {
            v[k] = lv[j];
            const int i = pre + 4 * j;
            xe_best(v[k].x, i, bv, bi);
            xe_best(v[k].y, i + 1, bv, bi);
            xe_best(v[k].z, i + 2, bv, bi);
            xe_best(v[k].w, i + 3, bv, bi);
        }
    }
    for (int j = XE_VEC * XE_THREADS + tid; j < nvec; j += XE_THREADS) {
        const float4 x = lv[j];
        const int i = pre + 4 * j;
        xe_best(x.x, i, bv, bi);
        xe_best(x.y, i + 1, bv, bi);
        xe_best(x.z, i + 2, bv, bi);
        xe_best(x.w, i + 3, bv, bi);
    }
    if (tid < V - tail0) xe_best(lg[tail0 + tid], tail0 + tid, bv, bi);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        xe_best(ov, oi, bv, bi);
    }
    if (lane == 0) sh.mv[wave] = bv, sh.mi[wave] = bi;
    __syncthreads();
    bv = sh.mv[0], bi = sh.mi[0];
#pragma unroll
    for (int w = 1; w < XE_WAVES; w++) xe_best(sh.mv[w], sh.mi[w], bv, bi);
    const double m = (double)bv;

    // ---- 2. S = sum exp(l - m) in fp64
    double acc = 0.0;
    if (tid < pre) acc += exp((double)lg[tid] - m);
#pragma unroll
    for (int k = 0; k < XE_VEC; k++) {
        const int j = k * XE_THREADS + tid;
        if (j < nvec) {
            acc += exp((double)v[k].x - m);
            acc += exp((double)v[k].y - m);
            acc += exp((double)v[k].z - m);
            acc += exp((double)v[k].w - m);
        }
    }
    for (int j = XE_VEC * XE_THREADS + tid; j < nvec; j += XE_THREADS) {
        const float4 x = lv[j];
        acc += exp((double)x.x - m);
        acc += exp((double)x.y - m);
        acc += exp((double)x.z - m);
        acc += exp((double)x.w - m);
    }
    if (tid < V - tail0) acc += exp((double)lg[tail0 + tid] - m);
    acc = wave_sum63_d(acc);
    if (lane == 63) sh.red[wave] = acc;
    __syncthreads();
    if (tid != 0) return;
    double t[XE_WAVES];
#pragma unroll
    for (int i = 0; i < XE_WAVES; i++) t[i] = sh.red[i];
#pragma unroll
    for (int s = 1; s < XE_WAVES; s *= 2)
#pragma unroll
        for (int i = 0; i < XE_WAVES; i += 2 * s) t[i] += t[i + s];
    if (argmax) argmax[blockIdx.x] = (uint32_t)min(max(bi == 0x7fffffff ? 0 : bi, 0), V - 1);
    if (loss) {
        const uint32_t tg = min(targets[blockIdx.x], (uint32_t)(V - 1));
        loss[blockIdx.x] = m + log(t[0]) - (double)lg[tg];
    }
}

}  // namespace

bool launch_xent(hipStream_t st, const float * logits, int rows, int V, const uint32_t * targets, double * loss,
                 uint32_t * argmax) {
    if (!logits || rows < 1 || V < 1 || (loss && !targets)) return false;
    RK_LAUNCH(k_xent, dim3((unsigned)rows), dim3(XE_THREADS), 0, st, logits, V, targets, loss, argmax);
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi
