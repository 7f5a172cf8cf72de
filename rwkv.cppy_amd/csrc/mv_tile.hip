// mv_tile.hip -- the batched decode matvec for 2..16 contexts on the int8 MFMA (k_mvt).
//
// y[t][m] = W[m] . x[t] for the T <= 16 activation rows of T contexts (MMGroup, T = B), quantized
// weights only.  k_mvb pays the nibble unpack and eight sdot4 once per (context, row, block); here
// one v_mfma_i32_16x16x32_i8 yields the exact integer block dots of 16 rows x 16 contexts, the
// weights are unpacked once per (row, block), and only the fp32 block epilogue is per context.  The
// weights stream once from the decode structure-of-arrays (no tile records, no LDS copy).
//
// Association contract (mv_common.hpp "the row block"; the only thing that makes a context's row
// bit-identical to its single-context decode):
//  - block b belongs to class l = b mod 64;
//  - a class chains its blocks in ascending b from +0.0f: acc = fmaf(dw * dx, (float)sumi, acc) for
//    every format, acc2 = fmaf(mw, sx, acc2) for the _1 formats;
//  - a class with no block contributes +0.0f (K < 2048, ragged last rounds);
//  - the 64 class sums fold by wave_sum63's balanced adjacent-pair tree;
//  - the result is tree(acc) + 0.0f, or tree(acc) + tree(acc2) for the _1 formats.
// sumi is the exact integer block dot with the format's offset (-8, -16, 5th bit) applied.  An MFMA
// over one quantization block yields it exactly in whatever order k runs, so ggml's nibble order
// (byte j = elements j and j + 16) is never unscrambled: the activation operand takes the same
// permutation.
//
// Split of the work.  A workgroup is 4 waves; wave s owns the 16 classes [16 s, 16 s + 16) -- a
// complete subtree of the class tree, the subtrees split-K uses -- of a 16-row tile.  Non-emitting
// groups: one tile per workgroup; emitting groups: two, one after the other, so a workgroup holds a
// whole 32-row emission block.  (16 classes x 4 rows of chain sums per lane, twice for the _1
// formats: 32 classes per wave, or 8 waves under a 256-register cap, spill.)  A round is 64 blocks of K; per round a wave's classes are 256 contiguous bytes of a row:
//  - lane (row r = lane & 15, group g = lane >> 4) loads the whole block 4 q + g of quad q as one
//    non-temporal dwordx4 (all four quads of the round, and the next round's, before anything
//    waits) and unpacks it to 8 dwords of int8 -- once per (row, block);
//  - a 4 x 4 exchange over the groups (v_permlane32_swap, then v_permlane16_swap, per dword
//    quadruple) leaves lane (r, g) with dwords g and 4 + g of blocks 4 q + 0..3: the MFMA A operand
//    (8 k-elements per lane) of four blocks.  Lane (context n, g) does the same with the Q8
//    activation block it loaded, so both operands carry the same k permutation;
//  - the D layout gives lane (n, g) rows 4 g + 0..3 of context n.  The scales come from their
//    loading lanes by ds_bpermute (no memory): dw / mw already widened to f32 by the lane that
//    loaded them, dx / sx and the _0 offset (folded into the float bias below) likewise;
//  - (float)sumi without a conversion: the MFMA accumulates onto the integer 0x4B400000, whose
//    float reading is 1.5 * 2^23 + sumi exactly; one subtraction of (1.5 * 2^23 + offset * qsum),
//    exact as well, leaves (float)(sumi - offset * qsum).
// A block past K enters with dx = sx = +0: fmaf(+-0, finite, acc) returns acc bit for bit, since a
// chain from +0 never holds -0 (round-to-nearest gives +0 for every exact zero sum).  Contexts >= T
// clamp to T - 1 and rows >= M to M - 1; neither is stored.
// After the rounds a wave folds its 16 classes (tree16: the subtree), the subtree totals meet in LDS,
// and the workgroup adds the tree's top two levels and applies apply_epi / emit32 to every (context,
// row) exactly as k_mvb's second phase does.
#include "mv_common.hpp"

namespace rwkvmi {

typedef int mvt_v4i __attribute__((ext_vector_type(4)));

constexpr int MVT_BIAS = 0x4B400000;  // the int whose float reading is 1.5 * 2^23
constexpr float MVT_BIAS_F = 12582912.0f;

// The 32 integers of a block as 8 dwords of int8 in dot_wblk's order: v[0..3] elements 0..15,
// v[4..7] elements 16..31; the nibble formats unsigned (offset: mvt_off), the 5th bit merged.
template <int WF>
__device__ __forceinline__ void mvt_unpack(const WBlk & w, int (&v)[8]) {
    if constexpr (WF == W_Q8_0) {
        v[0] = w.q0.x, v[1] = w.q0.y, v[2] = w.q0.z, v[3] = w.q0.w;
        v[4] = w.q1.x, v[5] = w.q1.y, v[6] = w.q1.z, v[7] = w.q1.w;
    } else {
        const uint32_t n[4] = {(uint32_t)w.q0.x, (uint32_t)w.q0.y, (uint32_t)w.q0.z, (uint32_t)w.q0.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t lo = n[j] & 0x0F0F0F0Fu, hi = (n[j] >> 4) & 0x0F0F0F0Fu;
            if constexpr (WF == W_Q5_0 || WF == W_Q5_1) {
                lo |= spread4((w.qh >> (4 * j)) & 0xF);
                hi |= spread4((w.qh >> (16 + 4 * j)) & 0xF);
            }
            v[j] = (int)lo;
            v[4 + j] = (int)hi;
        }
    }
}
template <int WF>
constexpr int mvt_off() {
    return WF == W_Q4_0 ? 8 : WF == W_Q5_0 ? 16 : 0;
}

// 4 x 4 exchange over the lane groups g = lane >> 4.  In: x[i] = dword i of the block group g
// loaded.  Out: x[i] = dword g of the block group i loaded.
__device__ __forceinline__ void mvt_xpose(int & x0, int & x1, int & x2, int & x3) {
    const auto a = __builtin_amdgcn_permlane32_swap(x0, x2, false, false);  // x0 groups 2, 3 <-> x2 groups 0, 1
    const auto b = __builtin_amdgcn_permlane32_swap(x1, x3, false, false);
    const auto c = __builtin_amdgcn_permlane16_swap((int)a[0], (int)b[0], false, false);  // odd groups <-> even groups
    const auto d = __builtin_amdgcn_permlane16_swap((int)a[1], (int)b[1], false, false);
    x0 = (int)c[0], x1 = (int)c[1], x2 = (int)d[0], x3 = (int)d[1];
}

__device__ __forceinline__ float mvt_from(int src_lane, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src_lane * 4, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ long mvt_pack(int lo, int hi) {
    return (long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}

// one lane's Q8 activation block with its scales
struct MvtX {
    int4 lo, hi;
    float d, s;
    int qs;
};

template <int WF, bool EMIT>
__global__ __launch_bounds__(256) void k_mvt(MMGroup g) {
    constexpr bool one = WF == W_Q4_1 || WF == W_Q5_1;
    constexpr int OFF = mvt_off<WF>();
    constexpr int RW = EMIT ? 32 : 16;       // rows per workgroup
    constexpr int TILES = RW / 16;           // 16-row tiles a wave walks, one after the other
    __shared__ float red[one ? 2 : 1][4][16][RW];  // [acc / acc2][subtree][context][row]
    int e = 0;
#pragma unroll 1
    while (e + 1 < g.n && (int)blockIdx.x >= g.e[e + 1].block0) e++;
    const MMEntry & E = g.e[e];
    const int T = g.T, M = E.W.M, K = E.W.K, nb = K >> 5;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = wave;  // the wave's class subtree
    const int l15 = lane & 15, grp = lane >> 4;
    const int rowwg = ((int)blockIdx.x - E.block0) * RW;
    const int ctx = min(l15, T - 1);                      // B operand: this lane's context
    const size_t xrow = (size_t)ctx * nb;
    const int cls0 = sub * 16 + grp;  // this lane's class in quad 0
    const mvt_v4i bias = {MVT_BIAS, MVT_BIAS, MVT_BIAS, MVT_BIAS};
    const int rounds = (nb + 63) >> 6;
#pragma unroll 1
    for (int tile = 0; tile < TILES; tile++) {
    const int row = min(rowwg + tile * 16 + l15, M - 1);  // A operand: this lane's weight row
    const uint32_t wrow = (uint32_t)row * (uint32_t)nb;

    // block 64 u + cls0 + 4 q: the weights of (row, block) and the activations of (context, block)
    auto load_w = [&](int u, WBlk (&w)[4]) {
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = load_wblk<WF, true>(E.W, wrow + (uint32_t)min(u * 64 + cls0 + 4 * q, nb - 1));
    };
    auto load_x = [&](int u, int q) {
        const size_t b = xrow + (size_t)min(u * 64 + cls0 + 4 * q, nb - 1);
        MvtX x;
        x.lo = *(const int4 *)(E.in.q + b * 32);
        x.hi = *(const int4 *)(E.in.q + b * 32 + 16);
        x.d = E.in.d[b];
        x.s = one ? E.in.s[b] : 0.0f;
        x.qs = OFF ? E.in.qsum[b] : 0;
        return x;
    };

    float acc[4][4][4], acc2[one ? 4 : 1][4][4];  // [quad][block of the quad][row 4 g + i]
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                acc[q][i][j] = 0.0f;
                if constexpr (one) acc2[q][i][j] = 0.0f;
            }
    WBlk wc[4];
    load_w(0, wc);
#pragma unroll 1
    for (int u = 0; u < rounds; u++) {
        // the next round's stream, in flight during this round's arithmetic (past K: the last block
        // again, never used)
        WBlk wn[4];
        load_w(u + 1, wn);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const bool valid = u * 64 + cls0 + 4 * q < nb;
            const MvtX x = load_x(u, q);
            int wv[8], xv[8] = {x.lo.x, x.lo.y, x.lo.z, x.lo.w, x.hi.x, x.hi.y, x.hi.z, x.hi.w};
            mvt_unpack<WF>(wc[q], wv);
            mvt_xpose(wv[0], wv[1], wv[2], wv[3]);
            mvt_xpose(wv[4], wv[5], wv[6], wv[7]);
            mvt_xpose(xv[0], xv[1], xv[2], xv[3]);
            mvt_xpose(xv[4], xv[5], xv[6], xv[7]);
            // this lane's own scales, widened once; the other lanes fetch them below
            const float dwf = h2f((uint16_t)(wc[q].sc & 0xFFFF));
            const float mwf = one ? h2f((uint16_t)(wc[q].sc >> 16)) : 0.0f;
            const float dxf = valid ? x.d : 0.0f;
            const float sxf = valid ? x.s : 0.0f;
            const float bqf = MVT_BIAS_F + (float)(OFF * x.qs);
#pragma unroll
            for (int i = 0; i < 4; i++) {  // block 4 q + i of the wave's classes, loaded by group i
                const mvt_v4i sv =
                    __builtin_amdgcn_mfma_i32_16x16x32_i8(mvt_pack(wv[i], wv[4 + i]), mvt_pack(xv[i], xv[4 + i]), bias, 0, 0, 0);
                const float dx = mvt_from(16 * i + l15, dxf);
                const float bq = OFF ? mvt_from(16 * i + l15, bqf) : MVT_BIAS_F;
                float sx = 0.0f;
                if constexpr (one) sx = mvt_from(16 * i + l15, sxf);
#pragma unroll
                for (int j = 0; j < 4; j++) {  // row 4 g + j of context l15
                    const float dw = mvt_from(16 * i + 4 * grp + j, dwf);
                    const float sf = __builtin_bit_cast(float, (int)sv[j]) - bq;
                    acc[q][i][j] = fmaf(dw * dx, sf, acc[q][i][j]);
                    if constexpr (one) acc2[q][i][j] = fmaf(mvt_from(16 * i + 4 * grp + j, mwf), sx, acc2[q][i][j]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) wc[q] = wn[q];
    }
    // the wave's subtree: its 16 classes folded (class 4 q + i of the subtree = acc[q][i])
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float p[16];
#pragma unroll
        for (int c = 0; c < 16; c++) p[c] = acc[c >> 2][c & 3][j];
        red[0][sub][l15][tile * 16 + 4 * grp + j] = tree16(p);
        if constexpr (one) {
#pragma unroll
            for (int c = 0; c < 16; c++) p[c] = acc2[c >> 2][c & 3][j];
            red[1][sub][l15][tile * 16 + 4 * grp + j] = tree16(p);
        }
    }
    }
    __syncthreads();
    // the tree's top two levels and the epilogue over every (context, row) of the workgroup; RW = 32
    // when emitting, so each half-wave holds one context's 32-row block
    for (int i = threadIdx.x; i < T * RW; i += 256) {
        const int t = i / RW, rl = i % RW, r = rowwg + rl;
        float s = (red[0][0][t][rl] + red[0][1][t][rl]) + (red[0][2][t][rl] + red[0][3][t][rl]);
        if constexpr (one) s = s + ((red[1][0][t][rl] + red[1][1][t][rl]) + (red[1][2][t][rl] + red[1][3][t][rl]));
        else s = s + 0.0f;
        float v = 0.0f;
        if (r < M) {
            v = apply_epi(E, t, r, s);
            if (E.y) E.y[(size_t)t * E.ldy + r] = v;
        }
        if constexpr (EMIT) {
            if (E.emit) emit32(E.out, t, r, v);
        }
    }
}

template <int WF>
static bool launch_mvt_wf(hipStream_t st, MMGroup & g, bool emit) {
    const int RW = emit ? 32 : 16;
    int blocks = 0;
    for (int i = 0; i < g.n; i++) {
        g.e[i].block0 = blocks;
        blocks += (g.e[i].W.M + RW - 1) / RW;
    }
    if (!blocks) return true;
    if (emit) RK_LAUNCH((k_mvt<WF, true>), dim3(blocks), dim3(256), 0, st, g);
    else RK_LAUNCH((k_mvt<WF, false>), dim3(blocks), dim3(256), 0, st, g);
    HIP_OK(hipGetLastError());
    return true;
}

// What k_mvt covers: 2..16 contexts, quantized weights of one type, row-major Q8 input, K in whole
// blocks, emitting entries in whole 32-row blocks into row-major outputs (launch_mvb_group's rules).
bool mvt_covers(const MMGroup & g, int wtype) {
    if (g.T < 2 || g.T > 16 || !wtype_quantized(wtype)) return false;
    for (int i = 0; i < g.n; i++) {
        const MMEntry & e = g.e[i];
        if (e.W.type != wtype || e.W.K % 32 || e.in.tiled || e.in.fmt != act_fmt_for(wtype) || e.in.K != e.W.K)
            return false;
        if (e.emit && (e.W.M % 32 || e.out.tiled)) return false;
    }
    return true;
}

// false in *launched (nothing launched, nothing written) when the group is outside what k_mvt
// covers; the caller then uses k_mvb or k_mm, which compute the same bits.
bool launch_mvt_group(hipStream_t st, MMGroup & g, int wtype, bool * launched) {
    *launched = false;
    if (!mvt_covers(g, wtype)) return true;
    bool emit = false;
    for (int i = 0; i < g.n; i++) emit |= g.e[i].emit != 0;
    bool ok = false;
    switch (wtype) {
        case W_Q4_0: ok = launch_mvt_wf<W_Q4_0>(st, g, emit); break;
        case W_Q4_1: ok = launch_mvt_wf<W_Q4_1>(st, g, emit); break;
        case W_Q5_0: ok = launch_mvt_wf<W_Q5_0>(st, g, emit); break;
        case W_Q5_1: ok = launch_mvt_wf<W_Q5_1>(st, g, emit); break;
        case W_Q8_0: ok = launch_mvt_wf<W_Q8_0>(st, g, emit); break;
        default: return true;
    }
    *launched = ok;
    return ok;
}

}  // namespace rwkvmi
