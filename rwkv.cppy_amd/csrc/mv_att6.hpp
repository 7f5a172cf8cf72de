// mv_att6.hpp -- pieces shared by the two v6 fused attention decode launches (mv_att6f.hip, the
// ordered layout that needs no co-residency; mv_att6c.hip, the co-resident layout): the producer
// rows (k_mva's arithmetic) and the head reducer both layouts call (att6_reduce: y first, state
// last).  r / k / v / g / decay-LoRA are handed over as handoff.hpp's cleared granules.
#pragma once
#include "mv_common.hpp"

namespace rwkvmi {

constexpr int AF_P = 8;   // workgroups per head
constexpr int AF_R = 8;   // rows per wave (4 waves x 8 rows x 8 workgroups = 4 x 64 rows)

// R rows of one matrix by one wave: k_mva's loads, dots, tree and epilogue (lane r: row r) -- the
// row block of mv_common.hpp, select form, written out: with this site and maa_dec4_body through the
// helpers v6-1B6 decode sat at the lower edge of the parent's spread (mv_maa.hpp has the figures)
template <int WF, int R, int U>
__device__ __forceinline__ float af_rows(const DMat & W, const ActBuf & x, int row0, int epi, int lane) {
    const int M = W.M, K = W.K;
    int rows[R];
#pragma unroll
    for (int r = 0; r < R; r++) rows[r] = min(row0 + r, M - 1);
    WBlk w[R][U];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
        for (int r = 0; r < R; r++) w[r][u] = load_unit<WF>(W, rows[r], u, lane);
    AUnit xu[U];
#pragma unroll
    for (int u = 0; u < U; u++) xu[u] = load_act_unit<WF, false>(x, u, lane);
    __builtin_amdgcn_sched_barrier(0);
    float acc[R], acc2[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = acc2[r] = 0.0f;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const bool valid = unit_valid<WF>(K, u, lane);
#pragma unroll
        for (int r = 0; r < R; r++) {
            float t = acc[r], t2 = acc2[r];
            dot_unit<WF>(w[r][u], xu[u], t, t2);
            acc[r] = valid ? t : acc[r];
            acc2[r] = valid ? t2 : acc2[r];
        }
    }
    const float s = row_sums<WF, R>(acc, acc2, lane);
    return epi == EPI_SILU ? siluf_(s) : epi == EPI_TANH ? rk_tanhf(s) : s;
}

// ---------------------------------------------------------------------------------------------
// The head reducer of both layouts: one 5-wave workgroup per head runs k_att6_dec's arithmetic on
// the granules of its head.  Schedule (output first):
//
//   waves 0..3                                          wave 4
//   sweep r / k / v / g (lane = channel), clear         sweep the D decay-LoRA values, clear
//   -- LDS rendezvous of waves 0..3 --                  Q8 image, Wd2 row, w = exp(-exp(.)) -> sw
//   output half of wkv6: p[c] += (kv u + prev) r
//   -- LDS rendezvous of waves 0..3 --
//   wave 0: GroupNorm, gate, publish y
//   ------------------------- __syncthreads (sw visible) -------------------------
//   state half of wkv6: prev w + kv -> sout
//
// y depends on r, k, v, g, u and the old state only; this token's decay enters the new state
// alone.  The decay path is the longest input chain of the launch (a single-row matvec + tanh per
// granule, then the Wd2 row and two exps), so wave 4 stays out of the two meetings before the
// publish -- s_barrier would count it -- and the 16 KB of state stores per head leave after y.
// Every expression and every summation order is k_att6_dec's: only independent work moved.
struct __attribute__((aligned(16))) Att6Lds {
    float sr[64], sk[64], sv[64], sg[64], sw[64], su[64];
    float part[16][64];
    unsigned rdv;  // arrivals of waves 0..3 (att6_red_begin zeroes it)
};

// what a reducer loads at kernel start, under its (or the producers') weight streams
struct Att6RedOps {
    float4 st[4];  // waves 0..3: state rows 16 wave + 4 kk + q, columns 4 jq .. 4 jq + 3
    WBlk wp[4];    // wave 4: the first units of Wd2 row c0 + lane
    float lnw_c, lnb_c, dec_c, u_c;
};

#ifdef RWKV_STAMP
#define ATT6_STAMP_PARAMS , unsigned long long * stamp_x_, unsigned long long & stamp_t1_
#define ATT6_STAMP_ARGS , stamp_x_, stamp_t1_
#else
#define ATT6_STAMP_PARAMS
#define ATT6_STAMP_ARGS
#endif

template <int WD>
__device__ __forceinline__ void att6_red_begin(const Att6Dec & at, Att6Lds & L, Att6RedOps & o, int h, int lane, int wave) {
    constexpr int S = 64;
    const int c0 = h * S, jq = lane & 15, kk = lane >> 4;
    const size_t hb = (size_t)h * S * S;
    // the zeroed arrival counter ordered before every wave's first arrival: a bare s_barrier as the
    // reducer's first instructions, BEFORE any load is issued -- after them the barrier would hold
    // all five waves (and the reducer's own r / k rows in the co-resident layout) behind the waits
    // the compiler places inside the operand loads (fp16 scale conversions: a memory round trip)
    if (threadIdx.x == 0) L.rdv = 0;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wave < 4) {
#pragma unroll
        for (int q = 0; q < 4; q++)
            o.st[q] = *(const float4 *)(at.sin + hb + (size_t)(16 * wave + 4 * kk + q) * S + 4 * jq);
    }
    if (wave == 0) {
        o.lnw_c = at.lnx_w[c0 + lane];
        o.lnb_c = at.lnx_b[c0 + lane];
        o.u_c = at.u[c0 + lane];
    }
    if (wave == 4) {
        o.dec_c = at.decay[c0 + lane];
        const int nb = at.wd2.K >> 5;
#pragma unroll
        for (int l = 0; l < 4; l++) o.wp[l] = load_wblk<WD>(at.wd2, (size_t)(c0 + lane) * nb + min(l, nb - 1));
    }
}

// Meeting of waves 0..3 only: this wave's LDS stores are done (lgkmcnt), one ds_add per wave, then
// poll until `target` arrivals.  LDS executes a CU's operations in order, so a wave that reads the
// count also reads everything the arrived waves stored before their add.
__device__ __forceinline__ void att6_rdv(unsigned * ctr, unsigned target, int lane) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while ((unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) <
           target)
        __builtin_amdgcn_s_sleep(0);
    asm volatile("" ::: "memory");
}

// WO: y published as Q8 granule blocks for the Wo rows of the same launch; otherwise emitted as
// the Wo launch's input record yq
template <int WD, bool WO>
__device__ __forceinline__ void att6_reduce(const Att6Fused & a, Att6Lds & L, const Att6RedOps & o, char * smem, int h,
                                            int lane, int wave, const ActBuf & yq, unsigned * err, unsigned spin_max,
                                            float eps ATT6_STAMP_PARAMS) {
    constexpr int S = 64;
    const int C = a.C, D = a.D, c0 = h * S, jq = lane & 15, kk = lane >> 4;
    const Att6Dec & at = a.att;
    const size_t hb = (size_t)h * S * S;
    const int i0 = 16 * wave + 4 * kk;  // waves 0..3: keys i0 + q, value columns 4 jq + c
    float kq[4], vj[4];
    if (wave < 4) {
        // sweep r, k, v, g of the head's channels (lane = channel)
        unsigned long long * g = a.gran + (size_t)wave * C + c0 + lane;
        bool live[1] = {true};
        float v[1];
        gran_sweep<1>(g, 0, live, v, err, spin_max);
        float * dst = wave == 0 ? L.sr : wave == 1 ? L.sk : wave == 2 ? L.sv : L.sg;
        dst[lane] = v[0];
        gran_clear(g);
        if (wave == 0) {
            L.su[lane] = o.u_c;
            STAMP_MID();
        }
        att6_rdv(&L.rdv, 4, lane);
        // wkv6 (ggml_rwkv_wkv6), the output half: it needs no decay
        const float4 k4 = *(const float4 *)(L.sk + i0), u4 = *(const float4 *)(L.su + i0);
        const float4 r4 = *(const float4 *)(L.sr + i0);
        const float4 v4 = *(const float4 *)(L.sv + 4 * jq);
        const float uq[4] = {u4.x, u4.y, u4.z, u4.w}, rq[4] = {r4.x, r4.y, r4.z, r4.w};
        kq[0] = k4.x, kq[1] = k4.y, kq[2] = k4.z, kq[3] = k4.w;
        vj[0] = v4.x, vj[1] = v4.y, vj[2] = v4.z, vj[3] = v4.w;
        float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float prev[4] = {o.st[q].x, o.st[q].y, o.st[q].z, o.st[q].w};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const float kv = vj[c] * kq[q];
                const float temp = kv * uq[q] + prev[c];
                const float t = temp * rq[q];
                p[c] += t;
            }
        }
        *(float4 *)&L.part[4 * wave + kk][4 * jq] = make_float4(p[0], p[1], p[2], p[3]);
        att6_rdv(&L.rdv, 8, lane);
        // GroupNorm over the head (ggml_norm, fp64 sums) * ln_x + b, * g; emitted as Wo's input
        if (wave == 0) {
            STAMP_X(1);
            float sgp[4];
#pragma unroll
            for (int gg = 0; gg < 4; gg++)
                sgp[gg] = (L.part[4 * gg][lane] + L.part[4 * gg + 1][lane]) +
                          (L.part[4 * gg + 2][lane] + L.part[4 * gg + 3][lane]);
            const float x = (sgp[0] + sgp[2]) + (sgp[1] + sgp[3]);
            const double s = group_tree_sum_d((double)x, S);
            const float mean = (float)div_count(s, S);
            const float d = x - mean;
            const double s2 = group_tree_sum_d((double)(d * d), S);
            const float var = (float)div_count(s2, S);
            const float scale = 1.0f / sqrtf(var + eps);
            float y = d * scale;
            y = y * o.lnw_c;
            y = y + o.lnb_c;
            y = y * L.sg[lane];
            if constexpr (WO) pub_q8(a.ygran, (c0 >> 5) + (lane >> 5), y, a.h.tag, lane);  // the head's 2 blocks
            else emit32(yq, 0, c0 + lane, y);
            STAMP_X(2);  // y published (the ordered layout's Wo workgroups stamp x2 / x3 too)
        }
    } else {
        // wave 4 sweeps the decay LoRA values and runs the decay tail meanwhile
        unsigned long long * const gdl = a.gran + 4 * (size_t)C;
        bool live[2] = {lane < D, lane + 64 < D};
        float v[2];
        unsigned long long * const own = gdl + (size_t)h * D + lane;  // this head's copy
        gran_sweep<2>(own, 64, live, v, err, spin_max);
        if (live[0]) gran_clear(own);
        if (live[1]) gran_clear(own + 64);
        const ActBuf act = lds_act(smem, act_fmt_for(WD), D);
        if (lane < D) emit32(act, 0, lane, v[0]);  // lanes 0..31 / 32..63: whole quantization blocks
        if (lane + 64 < D) emit32(act, 0, lane + 64, v[1]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        // decay tail of channel c0 + lane: w = exp(-exp(Wd2 . dl + decay)), rwkv_graph.inc:357-367
        const float s = decay_row_thread<WD, 4, 4>(at.wd2, c0 + lane, act, at.wd2.K >> 5, o.wp);
        L.sw[lane] = rk_expf(-rk_expf(s + o.dec_c));
    }
    __syncthreads();  // the one meeting with wave 4: sw
    STAMP_X(0);
    // wkv6, the state half: S' = S w + kv (kv by the same multiply as above)
    if (wave < 4) {
        const float4 w4 = *(const float4 *)(L.sw + i0);
        const float wq[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float prev[4] = {o.st[q].x, o.st[q].y, o.st[q].z, o.st[q].w};
            float nw[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const float kv = vj[c] * kq[q];
                nw[c] = prev[c] * wq[q] + kv;
            }
            *(float4 *)(at.sout + hb + (size_t)(i0 + q) * S + 4 * jq) = make_float4(nw[0], nw[1], nw[2], nw[3]);
        }
    }
}

}  // namespace rwkvmi
