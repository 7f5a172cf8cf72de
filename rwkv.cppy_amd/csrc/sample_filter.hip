// sample_filter.hip -- the sampler with the truncation rules in front of top-p: top-k, min-p and
// locally typical sampling (rwkv_mi355x_filters; the definition is in include/rwkv_mi355x.h and, in
// float64 numpy, rwkv_cpp.sampling.kept_mask).  launch_sample comes here only when a filter is set; a
// call without one runs the kernels of sample.hip, which this file does not touch.
//
// The layout is sample.hip's: one workgroup of 1024 threads per row, thread t holds elements
// k * 1024 + t (k < 64) in registers, the elements from 65536 on are re-formed from memory wherever
// they are needed.  l, m = max l, e = expf(l - m), S, the weights, the prefix sums, the draw and emit
// are sample_row's, statement for statement: that function is register-sensitive, so
// it is restated here and not shared.  What is new, per draw:
//
//   top-k    the bit pattern kb of the K-th largest e: the largest kb with #{e >= kb} >= K, by
//            bisection over integer counts (one barrier a probe, no float association at all)
//   min-p    e >= q, the same compare on the bit patterns (e_max == 1.0f): eb = max(kb, bits(q))
//   typical  over F = {e >= eb}: S_F = sum e and A = sum e (m - l) in fp64 (every product and sum in
//            double, k_logprobs' association), g = A / S_F, d = (float)|((double)m - (double)l) - g|;
//            the cutoff dc is the smallest bit pattern with mass{F, d <= dc} > typical_p * mass{F},
//            by bisection over the sampler's float32 block sums
//   top-p    sample_row's bisection over the masses of the set kept so far
//
// Where d lives.  A thread has 128 VGPRs (1024 threads: 4 waves per SIMD) and the row takes 64, so e
// and d cannot both stay.  For the typical phase the registers are loaded with l again (the row is in
// L2: the kernel read it a moment ago) and a probe is a function of v[k] = l alone: it recomputes
// e = expf(l - m) and d, and no second register row is declared.  Both are the same in every probe,
// and the compiler hoists them out of the bisection: it forms e (0 outside F) and d once, keeps most
// of the 128 values in VGPRs and reloads some 40 dwords a probe from scratch (1.2 KB of scratch a
// lane, against 68 to 80 bytes in sample.hip's kernels; profiles/sample_filters_resources.txt).  The
// occupancy is what it was: one 1024-thread workgroup, 4 waves per SIMD.  The phase ends with
// v[k] = e again, bit for bit what it was, where the element is kept and 0 where it is not: top-p's
// probes and the weights are sample_row's from there.
//
// Every loop has a fixed bound, no float is added atomically and nothing depends on scheduling: a call
// is a pure function of its inputs.  Non-finite logits may keep anything or nothing (a NaN d is never
// <= dc); the token is clamped to the row.
#include "device_common.hpp"
#include "kernels.hpp"
#include "sample_row.hpp"

namespace rwkvmi {

namespace {

struct FilterShared {
    uint32_t bid[SAMPLE_MAX_BIAS];
    float bval[SAMPLE_MAX_BIAS];
    float red[2][SM_WAVES];      // block sums, double-buffered (one barrier per sum)
    uint32_t redc[2][SM_WAVES];  // the counts of a top-k probe
    double redd[2][SM_WAVES];    // S_F and A
    float amax_v[SM_WAVES];
    int amax_i[SM_WAVES];
    int cnt[SM_WAVES], last[SM_WAVES];
    uint32_t emin[SM_WAVES];
    float wtot[SM_WAVES];
    float tab[SM_MAX_ROWS * SM_WAVES];  // (row k, wave) totals of w in vocabulary order -> their prefix sums
    int sel;
};

// sample.hip's sm_block_sum: 6 DPP levels, then a fixed tree over the waves; every thread gets it
__device__ __forceinline__ float sf_block_sum(float part, FilterShared & sh, int & phase) {
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

// Integers: any order gives the same count
__device__ __forceinline__ uint32_t sf_block_count(uint32_t part, FilterShared & sh, int & phase) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t * buf = sh.redc[phase & 1];
    phase++;
    part = wave_sum(part);
    if (lane == 0) buf[wave] = part;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < SM_WAVES; i++) t += buf[i];
    return t;
}

// Two fp64 sums behind one barrier, in k_logprobs' association (wave_sum63_d, the tree over the waves)
__device__ __forceinline__ void sf_block_sums_d(double & x, double & y, FilterShared & sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = wave_sum63_d(x);
    y = wave_sum63_d(y);
    if (lane == 63) sh.redd[0][wave] = x, sh.redd[1][wave] = y;
    __syncthreads();
    double t[2][SM_WAVES];
#pragma unroll
    for (int i = 0; i < SM_WAVES; i++) t[0][i] = sh.redd[0][i], t[1][i] = sh.redd[1][i];
#pragma unroll
    for (int s = 1; s < SM_WAVES; s *= 2)
#pragma unroll
        for (int i = 0; i < SM_WAVES; i += 2 * s) t[0][i] += t[0][i + s], t[1][i] += t[1][i + s];
    x = t[0][0], y = t[1][0];
}

// a double every lane holds alike, in scalar registers
__device__ __forceinline__ double sf_uniform_d(double x) {
    const long long b = __builtin_bit_cast(long long, x);
    const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll)), hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}

// sample_row (sample.hip) with the filters of f in front of top-p.  ROWS and LP mean what they mean
// there; the statements outside the blocks marked "filters" are that function's.
template <bool ROWS, bool LP>
__device__ __forceinline__ void sample_row_filtered(const SampleArgs & a, const SampleFilters & f, FilterShared & sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = a.V, nb = a.n_bias;
    const int nrows = (V + SM_THREADS - 1) / SM_THREADS;  // <= SM_MAX_ROWS (launch_sample)
    const float * lg = a.logits + (size_t)blockIdx.x * (size_t)V;
    const float NEG_INF = __int_as_float(0xff800000);
    int phase = 0;
    float temperature = a.temperature, top_p = a.top_p;
    uint32_t top_k = f.top_k;
    float min_p = f.min_p, typical_p = f.typical_p;
    SmPenalty pen;
    uint32_t seq = blockIdx.x, at = a.step;
    if constexpr (ROWS) {
        if (!sm_row_live(a, seq, at)) {
            // a finished row: the decode step still embeds tok2[row], so it gets an id < V
            if (tid == 0 && a.tok2) a.tok2[blockIdx.x] = 0;
            return;
        }
        const uint32_t r = seq;
        if (a.temperature_r) temperature = a.temperature_r[r];
        if (a.top_p_r) top_p = a.top_p_r[r];
        if (f.top_k_r) top_k = f.top_k_r[r];
        if (f.min_p_r) min_p = f.min_p_r[r];
        if (f.typical_p_r) typical_p = f.typical_p_r[r];
        sm_row_penalty(a, r, pen);
    }
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
    sm_load_row<ROWS>(v, lg, V, pen, nb, sh.bid, sh.bval);

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
    if (temperature == 0.0f) {  // the argmax, whatever the filters
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
    // ---- filters: the set kept so far.  A register element that is out has v[k] = 0 from then on: a
    // zero adds nothing to a mass and is below every probe, so the sums below are sample_row's, and
    // step 4 keeps no zero in a filtered draw (an e that underflowed to 0 could not be drawn at
    // temperature 1 anyway).  An element from memory: in_set(l, e), from the three words the phases
    // below leave -- eb (top-k and min-p: e >= eb), and under typ the mean g and the cutoff dc
    // (d <= dc).  They are the same in every thread and live to the end of the kernel, so they are
    // moved to scalar registers: the 64 row registers leave no VGPR for them.  All of the row at first.
    const double md = (double)m;
    uint32_t eb = 0u, dc = 0xffffffffu;
    double g = 0.0;
    bool typ = false;
    auto dist = [&](float l) -> float { return (float)fabs((md - (double)l) - g); };
    auto in_set = [&](float l, float e) -> bool {
        return __float_as_uint(e) >= eb && (!typ || __float_as_uint(dist(l)) <= dc);
    };
    // sum of the kept e whose bit pattern is >= cb, over this thread's elements: 64 serial adds, then
    // one more per further 64 rows (sample_row's thread_mass: with everything kept, its bits)
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
                    const float l = biased(i), e = expf(l - m);
                    p += __float_as_uint(e) >= cb && in_set(l, e) ? e : 0.0f;
                }
            }
            acc += p;
        }
        return acc;
    };
    const float S = sf_block_sum(thread_mass(0u), sh, phase);

    // ---- filters, top-k: the largest kb with count(kb) >= K is the bit pattern of the K-th largest e
    // (non-negative floats order like their bits).  count() is monotone, count(0) = V > K; no probe
    // is at 0, so the zeros outside the row are never counted.
    const bool k_on = top_k > 0u && top_k < (uint32_t)V;
    if (k_on) {
        uint32_t lo = 0u, hi = 0x3f800001u;  // e <= 1: count(hi) = 0
        for (int it = 0; it < 31 && hi - lo > 1u; it++) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            uint32_t c = 0u;
#pragma unroll
            for (int k = 0; k < SM_REGS; k++) c += __float_as_uint(v[k]) >= mid ? 1u : 0u;
            for (int i = SM_REGS * SM_THREADS + tid; i < V; i += SM_THREADS)
                c += __float_as_uint(expf(biased(i) - m)) >= mid ? 1u : 0u;
            if (sf_block_count(c, sh, phase) >= top_k) lo = mid;
            else hi = mid;
        }
        eb = __builtin_amdgcn_readfirstlane(lo);
    }
    // ---- filters, min-p: e >= q on the bit patterns (q > 0 here)
    const bool q_on = min_p > 0.0f;
    if (q_on) eb = max(eb, __float_as_uint(min_p));

    // ---- filters, typical-p over F = {e >= eb}
    const bool t_on = typical_p > 0.0f && typical_p < 1.0f;
    if (t_on) {
        sm_load_row<ROWS>(v, lg, V, pen, nb, sh.bid, sh.bval);  // v = l for this phase
        double s = 0.0, sa = 0.0;  // every product and every sum in fp64, k ascending
#pragma unroll
        for (int k = 0; k < SM_REGS; k++) {
            const float e = expf(v[k] - m);
            if (k * SM_THREADS + tid < V && __float_as_uint(e) >= eb) {
                const double ed = (double)e;
                s += ed;
                sa += ed * (md - (double)v[k]);
            }
        }
        for (int i = SM_REGS * SM_THREADS + tid; i < V; i += SM_THREADS) {
            const float l = biased(i), e = expf(l - m);
            if (__float_as_uint(e) >= eb) {
                const double ed = (double)e;
                s += ed;
                sa += ed * (md - (double)l);
            }
        }
        sf_block_sums_d(s, sa, sh);
        g = sf_uniform_d(sa / s);
        // sum of the e of F whose d has a bit pattern <= db, in thread_mass's association.  Outside
        // the row l = -inf, so e = 0 and the term is 0 whatever its d.
        auto thread_mass_d = [&](uint32_t db) -> float {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < SM_REGS; k++) {
                const float e = expf(v[k] - m);
                acc += __float_as_uint(e) >= eb && __float_as_uint(dist(v[k])) <= db ? e : 0.0f;
            }
            for (int k0 = SM_REGS; k0 < nrows; k0 += SM_REGS) {
                float p = 0.0f;
                const int k1 = min(k0 + SM_REGS, nrows);
                for (int k = k0; k < k1; k++) {
                    const int i = k * SM_THREADS + tid;
                    if (i < V) {
                        const float l = biased(i), e = expf(l - m);
                        p += __float_as_uint(e) >= eb && __float_as_uint(dist(l)) <= db ? e : 0.0f;
                    }
                }
                acc += p;
            }
            return acc;
        };
        // the smallest db with mass(db) > target: mass() is monotone, and all of F is below +inf
        const float target = typical_p * sf_block_sum(thread_mass_d(0xffffffffu), sh, phase);
        uint32_t lo = 0u, hi = 0x7f800000u;
        for (int it = 0; it < 32 && lo < hi; it++) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (sf_block_sum(thread_mass_d(mid), sh, phase) > target) hi = mid;
            else lo = mid + 1u;
        }
        dc = __builtin_amdgcn_readfirstlane(hi);
        typ = true;
    }
    const bool filtered = k_on || q_on || t_on;
    if (filtered) {
        // v = e again where the element is kept, else 0
#pragma unroll
        for (int k = 0; k < SM_REGS; k++) {
            const float l = v[k], e = t_on ? expf(l - m) : v[k];
            v[k] = k * SM_THREADS + tid < V && in_set(l, e) ? e : 0.0f;
        }
    }

    // ---- 3. the top-p cutoff over the set kept so far: the largest bit pattern cb with mass(cb) >
    // top_p * mass(0).  Unfiltered, mass(0) is S, bit for bit.
    uint32_t cb = 0u;
    if (top_p > 0.0f && top_p < 1.0f) {
        const float target = top_p * (filtered ? sf_block_sum(thread_mass(0u), sh, phase) : S);
        uint32_t lo = 0u, hi = 0x3f800001u;  // e <= 1: mass(hi) = 0
        for (int it = 0; it < 31 && hi - lo > 1u; it++) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const float mass = sf_block_sum(thread_mass(mid), sh, phase);
            if (mass > target) lo = mid;
            else hi = mid;
        }
        cb = lo;
    }

    // ---- 4. weights of the kept elements; their count, the largest kept index, the smallest kept e
    const bool t1 = temperature == 1.0f;
    const uint32_t cbk = filtered ? max(cb, 1u) : cb;  // filtered: the zeros are out
    int cnt = 0, last = -1;
    uint32_t emin = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < SM_REGS; k++) {
        const int i = k * SM_THREADS + tid;
        float w = 0.0f;
        if (i < V && __float_as_uint(v[k]) >= cbk) {
            cnt++;
            last = i;
            emin = min(emin, __float_as_uint(v[k]));
            w = t1 ? v[k] : expf((biased(i) - m) / temperature);
        }
        v[k] = w;
    }
    auto tail_w = [&](int i, bool count) -> float {
        if (i >= V) return 0.0f;
        const float l = biased(i), d = l - m, e = expf(d);
        if (__float_as_uint(e) < cbk || !in_set(l, e)) return 0.0f;
        if (count) cnt++, last = i, emin = min(emin, __float_as_uint(e));
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
        emin = min(emin, (uint32_t)__shfl_xor((int)emin, o));
    }
    if (lane == 0) sh.cnt[wave] = cnt, sh.last[wave] = last, sh.emin[wave] = emin;
    __syncthreads();
    cnt = 0, last = -1, emin = 0xffffffffu;
#pragma unroll
    for (int w = 0; w < SM_WAVES; w++) cnt += sh.cnt[w], last = max(last, sh.last[w]), emin = min(emin, sh.emin[w]);

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
    // the smallest kept e / S; a row with every filter off reports what k_sample reports
    if (a.cutoff && tid == 0) a.cutoff[blockIdx.x] = __uint_as_float(filtered && cnt > 0 ? emin : cb) / S;
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

__global__ __launch_bounds__(SM_THREADS) void k_sample_f(const SampleArgs a, const SampleFilters f) {
    __shared__ FilterShared sh;
    sample_row_filtered<false, false>(a, f, sh);
}

__global__ __launch_bounds__(SM_THREADS) void k_sample_rows_f(const SampleArgs a, const SampleFilters f) {
    __shared__ FilterShared sh;
    sample_row_filtered<true, false>(a, f, sh);
}

__global__ __launch_bounds__(SM_THREADS) void k_sample_f_lp(const SampleArgs a, const SampleFilters f) {
    __shared__ FilterShared sh;
    sample_row_filtered<false, true>(a, f, sh);
}

__global__ __launch_bounds__(SM_THREADS) void k_sample_rows_f_lp(const SampleArgs a, const SampleFilters f) {
    __shared__ FilterShared sh;
    sample_row_filtered<true, true>(a, f, sh);
}

}  // namespace

bool launch_sample_filtered(hipStream_t st, const SampleArgs & a, const SampleFilters & f, bool rows, bool lp) {
    // the scalars as the ABI checks them; the per-row values are the caller's to check
    if (!(f.min_p >= 0.0f && f.min_p <= 1.0f) || !(f.typical_p >= 0.0f && f.typical_p <= 1.0f)) return false;
    if (f.per_row() && !rows) return false;
    const dim3 grid((unsigned)a.rows), block(SM_THREADS);
    if (rows) {
        if (lp) RK_LAUNCH(k_sample_rows_f_lp, grid, block, 0, st, a, f);
        else RK_LAUNCH(k_sample_rows_f, grid, block, 0, st, a, f);
    } else {
        if (lp) RK_LAUNCH(k_sample_f_lp, grid, block, 0, st, a, f);
        else RK_LAUNCH(k_sample_f, grid, block, 0, st, a, f);
    }
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi
