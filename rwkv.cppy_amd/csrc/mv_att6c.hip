// mv_att6c.hip -- v6 decode attention launch, CO-RESIDENT layout (rwkv_graph.inc:349-384): the
// r, k, v, g and decay-LoRA-first-stage rows, the per-head attention core and the output
// projection Wo in one launch of 8 H workgroups -- the same bits as mv_att6f.hip's ordered layout.
//
// Workgroup (h, s) = blockIdx h * 8 + s computes 32 of head h's 256 r / k / v / g rows (4 waves x 8
// rows, k_mva's lane/unit order, wave_sum63 tree and epilogues) and, on a fifth wave, the
// decay-LoRA rows of its slot, each published as a single-reader granule (handoff.hpp).  (h, 0) --
// which loads the head's state, decay-tail weights and per-channel operands while its own rows
// stream -- sweeps its head's granules and runs k_att6_dec's arithmetic (decay tail, wkv6,
// GroupNorm, gate), publishing the head's 64 outputs y as two Q8 blocks of granules tagged (layer,
// state parity) -- pub_q8: the bits Wo's fp32-input prologue would produce.  The 7 H other
// workgroups then own Wo: wave gw's rows gw, gw + 28 H, gw + 56 H, whose units it loaded at kernel
// start; it waits for every head's y, gathers the blocks into LDS and adds its rows' dots to x.
//
// The reducer (mv_att6.hpp att6_reduce, shared with the ordered layout) publishes y FIRST: waves
// 0..3 meet among themselves (an LDS arrival counter, not s_barrier) once r, k, v, g have arrived,
// run the output half of wkv6, GroupNorm and pub_q8; the decay path on wave 4 -- the launch's longest
// input chain -- joins at one __syncthreads afterwards, and only then the new state (S w + kv, 16 KB
// of stores per head) is written.  The 224 Wo workgroups wait that much less.  What remains of the
// Wo tail after the head inputs are in: the two LDS meetings and the output half (~0.45 us), the
// GroupNorm's two fp64 tree sums and the Q8 publish (~1.1 us to the stores' completion), then on
// the Wo side the pre-poll, the gather of C / 32 blocks into LDS, the qsum pass and one dot per row.
//
// Every workgroup waits on workgroups of both lower and higher index, so this layout needs all
// 8 H workgroups resident at once.  One context alone on an idle device has that (8 H <= the 256
// compute units, one workgroup each -- v6_att_co_supported); the engine uses this layout only
// while no other context of the process has work queued on the device (Engine::co_mode) and
// falls back to the ordered layout for good after a hand-off timeout (another process's launches
// holding the compute units).  Bounded spins as in mv_att6f.hip: a timeout sets *err, never a hang.
//
// Measured against the ordered layout (v6-1B6, one context): 665.6 vs 694.7 us/token -- 96 fewer
// workgroups and the Wo rows spread 3 per wave over 224 workgroups instead of 8 per wave over 64.
// y as Q8 blocks instead of fp32 granules (a third of the gather traffic over 224 gatherers, no
// quantization in them): 655.6-656.7 vs 667.1-669.3 us/token.
#include "mv_att6.hpp"

#include <algorithm>

namespace rwkvmi {

__device__ __forceinline__ int af_slot(int sidx, int h, int H) { return sidx > 0 ? (sidx - 1) * H + h : (AF_P - 1) * H + h; }

constexpr int AF_WOR = 3;  // Wo rows per non-reducer wave: ceil(C / (28 H)) with C = 64 H

template <int WF, int U, int WD>
__global__ __launch_bounds__(320) void k_v6_att_co(Att6Fused a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // Q8 image of dl (decay tail input)
    __shared__ Att6Lds L;
    constexpr int S = 64;
    const int wg = (int)blockIdx.x, h = wg / AF_P, sidx = wg % AF_P, H = a.H, C = a.C, D = a.D;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform branches
    const bool red = sidx == 0;
    const int c0 = h * S;
    const Att6Dec & at = a.att;
    unsigned long long * const gdl = a.gran + 4 * (size_t)C;
    STAMP_BEGIN();
    // the reducer's late scalars (Wo input record, hand-off words, eps) in SGPRs now
    const ActBuf yq = at.yq;
    unsigned * const err = a.h.err;
    const unsigned spin_max = a.h.spin_max;
    const float eps = at.eps;
    if (red) {
        pin_act(yq);
        asm volatile("" ::"s"(err), "s"(eps), "s"(spin_max));
    }
    const bool publish = wg != a.skip_wg;  // test hook (Engine debug knob "skip_granule")
    // ---- the reducer's head operands first (state rows, per-channel vectors, decay-tail weights):
    // they stream in with this workgroup's own weight rows
    Att6RedOps ops;
    if (red) att6_red_begin<WD>(at, L, ops, h, lane, wave);
    // ---- this workgroup's rows, each published as a granule: wave w -> matrix (4 s + w) / 8
    // (r, k, v, g), rows of head h; wave 4 -> decay LoRA rows (EPI_TANH) of its slot, the
    // non-reducer workgroups' slots first (slot = (s - 1) H + h for s > 0, 7H + h for the reducers)
    if (wave < 4) {
        const int wh = sidx * 4 + wave, m = wh >> 3, row0 = c0 + (wh & 7) * AF_R;
        const DMat W = m == 0 ? a.W[0] : m == 1 ? a.W[1] : m == 2 ? a.W[2] : a.W[3];
        const ActBuf x = m == 0 ? a.x[0] : m == 1 ? a.x[1] : m == 2 ? a.x[2] : a.x[3];
        const float v = af_rows<WF, AF_R, U>(W, x, row0, m == 3 ? EPI_SILU : EPI_STORE, lane);
        if (lane < AF_R && publish) gran_store(a.gran + (size_t)m * C + row0 + lane, GRAN_ONCE, v);
    } else {
        for (int d = af_slot(sidx, h, H); d < D; d += AF_P * H) {
            const float v = af_rows<WF, 1, U>(a.wd1, a.xw, d, EPI_TANH, lane);  // in lane 0
            const float v0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
            if (lane < H && publish) gran_store(gdl + (size_t)lane * D + d, GRAN_ONCE, v0);  // one copy per head
        }
    }
    if (!red) {
        // ---- Wo (rwkv_graph.inc:382-384, x += Wo . y) on the 7 H non-reducer workgroups: wave
        // gw owns rows gw, gw + 28 H, gw + 56 H (k_mva's per-row arithmetic does not depend on
        // which wave computes a row).  Its units are loaded now, under the reducers' attention.
        // (Strided rows: the row block of mv_common.hpp written out, measured with af_rows.)
        const int nwo = 28 * H, gw = ((sidx - 1) * H + h) * 4 + wave;
        WBlk wo[AF_WOR][U];
        float xr = 0.0f;
        if (wave < 4) {
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int j = 0; j < AF_WOR; j++) wo[j][u] = load_unit<WF>(a.wo, min(gw + nwo * j, C - 1), u, lane);
            xr = a.xres[min(gw + nwo * min(lane, AF_WOR - 1), C - 1)];
        }
        // Wait for every head: wave 0 polls the d granule of every y block (handoff.hpp
        // q8_prepoll) -- the other waves park at the barrier, so the 7 H waiting workgroups add
        // little traffic beside the reducers' own sweeps; then all five waves gather y's Q8 blocks
        // (pub_q8 in the reducers: the bits Wo's fp32-input prologue would produce) into LDS
        const ActBuf xq = lds_act(smem, act_fmt_for(WF), C);
        const int nb = C >> 5;
        if (wave == 0) q8_prepoll(a.ygran, nb, a.h.tag, err, spin_max, lane);
        __syncthreads();
        q8_gather_image<(U > 1 ? 4 : 2)>(a.ygran, nb, a.h.tag, xq, tid, 320, err, spin_max);
        __syncthreads();
        q8_image_qsum(xq, nb, tid, 320);
        __syncthreads();
        if (wave < 4) {
            float acc[AF_WOR], acc2[AF_WOR];
#pragma unroll
            for (int j = 0; j < AF_WOR; j++) acc[j] = acc2[j] = 0.0f;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const AUnit xu = load_act_unit<WF, true>(xq, u, lane);
                const bool uv = unit_valid<WF>(C, u, lane);
#pragma unroll
                for (int j = 0; j < AF_WOR; j++) {
                    float t = acc[j], t2 = acc2[j];
                    dot_unit<WF>(wo[j][u], xu, t, t2);
                    acc[j] = uv ? t : acc[j];
                    acc2[j] = uv ? t2 : acc2[j];
                }
            }
            const float s = row_sums<WF, AF_WOR>(acc, acc2, lane);
            const int row = gw + nwo * lane;
            if (lane < AF_WOR && row < C) a.xres[row] = xr + s;  // EPI_ADD
        }
        STAMP_END_NS(6);
        return;
    }
    // ---- reducer (mv_att6.hpp att6_reduce: y first, then the decay tail's w and the state)
    att6_reduce<WD, true>(a, L, ops, smem, h, lane, wave, yq, err, spin_max, eps ATT6_STAMP_ARGS);
    STAMP_END(6);
}

bool v6_att_co_supported(const Att6Fused & a) {
    // the ordered layout's shapes, Wo fused, rows spread over the 28 H non-reducer waves; and the
    // whole grid resident at one workgroup per CU (the C > 2048 forms hold up to 223 VGPRs: one
    // 5-wave workgroup per CU), so 8 H <= the device's compute units
    if (!v6_att_fused_supported(a) || !a.wo.qs || a.C % 512 || AF_P * a.H > kQgCUs) return false;
    return (a.C + 28 * a.H - 1) / (28 * a.H) <= AF_WOR;
}

template <int WF, int U>
static void launch_co_wd(hipStream_t st, const Att6Fused & a, int lds) {
    const dim3 grid(AF_P * a.H), block(320);
    switch (a.att.wd2.type) {
        case W_Q4_0: RK_LAUNCH((k_v6_att_co<WF, U, W_Q4_0>), grid, block, lds, st, a); break;
        case W_Q4_1: RK_LAUNCH((k_v6_att_co<WF, U, W_Q4_1>), grid, block, lds, st, a); break;
        case W_Q5_0: RK_LAUNCH((k_v6_att_co<WF, U, W_Q5_0>), grid, block, lds, st, a); break;
        case W_Q5_1: RK_LAUNCH((k_v6_att_co<WF, U, W_Q5_1>), grid, block, lds, st, a); break;
        default: RK_LAUNCH((k_v6_att_co<WF, U, W_Q8_0>), grid, block, lds, st, a); break;
    }
}

bool launch_v6_att_co(hipStream_t st, const Att6Fused & a) {
    if (!v6_att_co_supported(a)) {
        fprintf(stderr, "rwkv: co-resident v6 attention decode: unsupported shape\n");
        return false;
    }
    const int lds = std::max(lds_bytes_for(act_fmt_for(a.att.wd2.type), a.D), lds_bytes_for(act_fmt_for(a.W[0].type), a.C));
    const bool u1 = mv_units(a.W[0].type, a.C) <= 1;
#define AC_T(WFv)                                   \
    do {                                            \
        if (u1) launch_co_wd<WFv, 1>(st, a, lds);   \
        else launch_co_wd<WFv, 2>(st, a, lds);      \
    } while (0)
    switch (a.W[0].type) {
        case W_Q4_0: AC_T(W_Q4_0); break;
        case W_Q4_1: AC_T(W_Q4_1); break;
        case W_Q5_0: AC_T(W_Q5_0); break;
        case W_Q5_1: AC_T(W_Q5_1); break;
        default: AC_T(W_Q8_0); break;
    }
#undef AC_T
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi
