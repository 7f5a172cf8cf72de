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
#include "device_common.hpp"
#include "kernels.hpp"

namespace rwkvmi {

namespace {

constexpr int SM_THREADS = 1024, SM_REGS = 64, SM_WAVES = 16;
constexpr int SM_MAX_ROWS = SAMPLE_MAX_VOCAB / SM_THREADS;

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

__global__ __launch_bounds__(SM_THREADS) void k_sample(const SampleArgs a) {
    __shared__ SampleShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V, nb = a.n_bias;
    const int nrows = (V + SM_THREADS - 1) / SM_THREADS;  // <= SM_MAX_ROWS (launch_sample)
    const float * lg = a.logits + (size_t)blockIdx.x * (size_t)V;
    const float NEG_INF = __int_as_float(0xff800000);
    int phase = 0;

    for (int j = tid; j < nb; j += SM_THREADS) {
        sh.bid[j] = a.bias_ids[j];
        sh.bval[j] = a.bias_vals[j];
    }
    if (tid == 0) sh.sel = 0x7fffffff;
    __syncthreads();

    // l_i of an element outside the registers (and of kept elements at a temperature other than 1):
    // the same additions in the same order as the register copy below
    auto biased = [&](int i) -> float {
        float x = lg[i];
        for (int j = 0; j < nb; j++)
            if (sh.bid[j] == (uint32_t)i) x += sh.bval[j];
        return x;
    };

    float v[SM_REGS];
#pragma unroll
    for (int k = 0; k < SM_REGS; k++) {
        const int i = k * SM_THREADS + tid;
        const float x = lg[min(i, V - 1)];  // a clamped load and a select: no branch per element
        v[k] = i < V ? x : NEG_INF;
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
    if (a.temperature == 0.0f) {
        if (tid == 0) {
            const uint32_t t = (uint32_t)min(max(bi == 0x7fffffff ? 0 : bi, 0), V - 1);
            a.tok[blockIdx.x] = t;
            if (a.tok2) a.tok2[blockIdx.x] = t;
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
    if (a.top_p > 0.0f && a.top_p < 1.0f) {
        const float target = a.top_p * S;
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
    const bool t1 = a.temperature == 1.0f;
    int cnt = 0, last = -1;
#pragma unroll
    for (int k = 0; k < SM_REGS; k++) {
        const int i = k * SM_THREADS + tid;
        float w = 0.0f;
        if (i < V && __float_as_uint(v[k]) >= cb) {
            cnt++;
            last = i;
            w = t1 ? v[k] : expf((biased(i) - m) / a.temperature);
        }
        v[k] = w;
    }
    auto tail_w = [&](int i, bool count) -> float {
        if (i >= V) return 0.0f;
        const float d = biased(i) - m, e = expf(d);
        if (__float_as_uint(e) < cb) return 0.0f;
        if (count) cnt++, last = i;
        return t1 ? e : expf(d / a.temperature);
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
    const float u = a.u ? a.u[blockIdx.x] : sample_uniform(a.seed, a.counter + blockIdx.x);
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
    const uint32_t t = (uint32_t)min(max(token, 0), V - 1);
    a.tok[blockIdx.x] = t;
    if (a.tok2) a.tok2[blockIdx.x] = t;
}

}  // namespace

bool launch_sample(hipStream_t st, const SampleArgs & a) {
    if (!a.logits || !a.tok || a.rows < 1 || a.V < 1 || a.V > SAMPLE_MAX_VOCAB) return false;
    if (a.n_bias < 0 || a.n_bias > SAMPLE_MAX_BIAS || (a.n_bias && (!a.bias_ids || !a.bias_vals))) return false;
    RK_LAUNCH(k_sample, dim3((unsigned)a.rows), dim3(SM_THREADS), 0, st, a);
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi
