// qg_msum.hip -- the _1 formats' m*s pass of the sequence GEMM (qgemm.hip).
//
// The m*s chains in the matvec's association: for class l (= b mod 64) the chain
// acc = acc + m_w[b] * s_x[b] over b = l + 64 u ascending, from 0; the 64 class sums folded by
// wave_sum63's tree (the binary counter of the GEMM).  Independent of the int8 dot, so it runs as
// its own VALU pass ahead of the GEMM -- whose tiles then carry one chain, 64 rows, like _0 -- and
// the GEMM epilogue (or k_qg_combine) adds these totals: the same y bits.
// Output m2[row][token] (row-major over rows).
//
// Two kernels over 64-row tiles, built from the same pieces: k_qg_msum (4 x 4 register tiles over 64
// tokens) and k_qg_msum_rows (one row x 8 tokens over 32).  Stages of 8 classes: all their blocks'
// m_w (64 rows) and s_x (the tile's tokens) are copied to LDS with coalesced loads -- the next
// stage's in flight while this one is accumulated.
#include "device_common.hpp"
#include "kernels.hpp"

#include <stdio.h>
#include <algorithm>

namespace rwkvmi {

typedef float qf2_t __attribute__((ext_vector_type(2)));

// The pass's arithmetic in packed f32 (v_pk_mul_f32 / v_pk_add_f32: per element the scalar
// operations' bits, tools/pk_probe.hip; this file builds without the SLP vectorizer, so the packing
// is spelled out): acc[j] = acc[j] + w * x[j] over pairs of outputs, and the class-tree folds.
// m_w and s_x are fp16 values, so w * x is exact in f32 and acc + w * x IS fmaf(w, x, acc): one
// v_pk_fma_f32 per pair instead of a v_pk_mul_f32 and a v_pk_add_f32 (the same bits).
template <int N>
__device__ __forceinline__ void qm_mac_row(float * acc, float w, const float (&x)[N]) {
    const qf2_t w2 = {w, w};
#pragma unroll
    for (int j = 0; j < N; j += 2) {
        qf2_t a = {acc[j], acc[j + 1]};
        const qf2_t x2 = {x[j], x[j + 1]};
        a = __builtin_elementwise_fma(w2, x2, a);  // = a + w * x bit for bit: m_w * s_x is exact
        acc[j] = a.x;
        acc[j + 1] = a.y;
    }
}

// One block's operands for a lane and its multiply-adds onto the lane's NO outputs
struct QMTileOps {  // k_qg_msum: m_w of 4 rows, s_x of 4 tokens
    static constexpr int NO = 16;
    float4 w, x;
    __device__ __forceinline__ void mac(float (&a)[NO]) const {
        const float wv[4] = {w.x, w.y, w.z, w.w};
        const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int r = 0; r < 4; r++) qm_mac_row<4>(a + 4 * r, wv[r], xv);
    }
};
struct QMRowOps {  // k_qg_msum_rows: m_w of the lane's row, s_x of the wave's 8 tokens
    static constexpr int NO = 8;
    float w;
    float4 s0, s1;
    __device__ __forceinline__ void mac(float (&a)[NO]) const {
        const float sx[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        qm_mac_row<8>(a, w, sx);
    }
};

// The blocks o[u], u < n, chained onto a in ascending order (n is wave-uniform); first: block 0 is
// there whatever n says, so a chain that starts on a literal 0 needs no zeroed accumulator
template <class Ops, int N>
__device__ __forceinline__ void qm_chain(float (&a)[Ops::NO], const Ops (&o)[N], int n, bool first) {
#pragma unroll
    for (int u = 0; u < N; u++) {
        if (!(first && u == 0) && u >= n) break;
        o[u].mac(a);
    }
}

// 4 blocks of a class at a time, u0 .. u0 + 3 of its n: their reads (rd(o, lc, u): slot (u, lc))
// issued together, then the chain.  Registers stay bounded for any NMAX.
template <int NMAX, class Ops, class Rd>
__device__ __forceinline__ void qm_mac4(float (&a)[Ops::NO], Rd && rd, int lc, int u0, int n, bool first) {
    Ops o[4];
#pragma unroll
    for (int q = 0; q < 4; q++) rd(o[q], lc, min(u0 + q, NMAX - 1));
    qm_chain(a, o, n - u0, first);
}

template <int NO>
__device__ __forceinline__ void qm_zero(float (&a)[NO]) {
#pragma unroll
    for (int k = 0; k < NO; k++) a[k] = 0.0f;
}

// The binary counter over the class sums (wave_sum63's tree): v = acc, then v = st[kk] + v for
// kk < NL, into st[NL] (NL < 6) or st[0] (NL = 6: the total); pairs of outputs
template <int NL, int NO>
__device__ __forceinline__ void qm_close(float (&st)[6][NO], const float (&acc)[NO]) {
#pragma unroll
    for (int k = 0; k < NO; k += 2) {
        qf2_t v = {acc[k], acc[k + 1]};
#pragma unroll
        for (int kk = 0; kk < NL; kk++) v = qf2_t{st[kk][k], st[kk][k + 1]} + v;
        st[NL < 6 ? NL : 0][k] = v.x;
        st[NL < 6 ? NL : 0][k + 1] = v.y;
    }
}
// qm_close of a runtime n in [1, 6] levels
template <int NO>
__device__ __forceinline__ void qm_close_n(int n, float (&st)[6][NO], const float (&acc)[NO]) {
    switch (n) {
        case 1: qm_close<1, NO>(st, acc); break;
        case 2: qm_close<2, NO>(st, acc); break;
        case 3: qm_close<3, NO>(st, acc); break;
        case 4: qm_close<4, NO>(st, acc); break;
        case 5: qm_close<5, NO>(st, acc); break;
        default: qm_close<6, NO>(st, acc); break;
    }
}
// Class l's sum (acc) into the counter -- an even class is level 0, an odd one closes ctz(~l)
// levels -- and acc = 0 for the next class
template <int NO>
__device__ __forceinline__ void qm_fold(int l, float (&st)[6][NO], float (&acc)[NO]) {
    if ((l & 1) == 0) {
#pragma unroll
        for (int k = 0; k < NO; k++) st[0][k] = acc[k];
    } else {
        qm_close_n<NO>(__builtin_ctz(~l), st, acc);
    }
    qm_zero(acc);
}

constexpr int QM_CLS = 8;  // classes per stage

// Stage sg's 8 classes as a static 3-level subtree (class pairs in two accumulator sets, the binary
// counter's levels 1 and 2 in named registers), then levels 3.. by the stage's own counter: the same
// additions as qm_fold, without its copies and branches.  cls(a, lc): class 8 sg + lc's chain, from
// 0, into a; called for lc = 0 .. 7 in order.
// The accumulators are members, owned by the caller's stage: as locals of an inlined function their
// scope ends right behind the switch, its arms then meet in one block, and the counter's loop-carried
// levels are copied there once per stage (32 v_mov_b64 at 16 outputs).
template <int NO>
struct QMSubtree {
    float aA[NO], aB[NO], p1[NO], p2[NO];

    static __device__ __forceinline__ void addl(float (&v)[NO], const float (&t)[NO]) {  // v = t + v
#pragma unroll
        for (int k = 0; k < NO; k += 2) {
            const qf2_t r = qf2_t{t[k], t[k + 1]} + qf2_t{v[k], v[k + 1]};
            v[k] = r.x;
            v[k + 1] = r.y;
        }
    }
    static __device__ __forceinline__ void put(float (&d)[NO], const float (&v)[NO]) {
#pragma unroll
        for (int k = 0; k < NO; k++) d[k] = v[k];
    }
    template <class Cls>
    __device__ __forceinline__ void run(int sg, float (&st)[6][NO], Cls && cls) {
#pragma unroll
        for (int lc = 0; lc < QM_CLS; lc += 2) {
            cls(aA, lc);
            cls(aB, lc + 1);
            addl(aB, aA);  // the odd class: st[0] + acc
            if (lc == 0 || lc == 4) {
                put(p1, aB);  // level 1
            } else if (lc == 2) {
                addl(aB, p1);
                put(p2, aB);  // level 2
            } else {
                addl(aB, p1);
                addl(aB, p2);
                // levels 3.. : class 8 sg + 7's counter.  Not qm_close_n: its stores through a runtime
                // level leave part of the counter in scratch here.
                switch (__builtin_ctz(~sg)) {
                    case 0: put(st[3], aB); break;
                    case 1: addl(aB, st[3]); put(st[4], aB); break;
                    case 2: addl(aB, st[3]); addl(aB, st[4]); put(st[5], aB); break;
                    default: addl(aB, st[3]); addl(aB, st[4]); addl(aB, st[5]); put(st[0], aB); break;
                }
            }
        }
    }
};

// This workgroup's entry, 64-row tile and TT-token tile: the grid is every entry's tiles in order
struct QMTile {
    int e, rt, tg;
};
template <int TT>
__device__ __forceinline__ QMTile qm_tile(const MMGroup & g) {
    const int tgs = (g.T + TT - 1) / TT;
    int e = 0, base = 0;
#pragma unroll 1
    for (; e + 1 < g.n; e++) {
        const int n_e = (g.e[e].W.M + 63) / 64 * tgs;
        if ((int)blockIdx.x < base + n_e) break;
        base += n_e;
    }
    const int local = (int)blockIdx.x - base;
    return {e, local / tgs, local % tgs};
}

// Class l of a row of nb blocks holds blocks l + 64 u, u < size(l).  A stage's LDS slot (u, lc), at
// u * 8 + lc, holds m_w and s_x of block 8 sg + lc + 64 u; blk: the block loaded into it -- a slot
// past its class's count is clamped to a block that exists (loaded, never read).
struct QMClasses {
    int nb, cq, crem;
    __device__ __forceinline__ explicit QMClasses(int nb_) : nb(nb_), cq(nb_ >> 6), crem(nb_ & 63) {}
    __device__ __forceinline__ int size(int l) const { return cq + (l < crem ? 1 : 0); }
    __device__ __forceinline__ int blk(int sg, int sl) const {
        const int lc = sl & 7, u = sl >> 3, l = sg * QM_CLS + lc;
        return min(u < size(l) ? l + 64 * u : l, nb - 1);
    }
};

// The stage loop of a 64-row x TT-token workgroup: stage sg + 1's operands are loaded (row tid % 64
// of slots tid / 64 + 4 k, token tid % TT of slots tid / TT + 256 / TT k) while stage(sg, qw[buf],
// qx[buf]) accumulates stage sg, then stored to the other buffer.
template <int NMAX, int TT, class Stage>
__device__ __forceinline__ void qm_stages(const MMEntry & E, const QMClasses & cls, int T, int r0, int tok0,
                                          float (&qw)[2][QM_CLS * NMAX][64], float (&qx)[2][QM_CLS * NMAX][TT],
                                          Stage && stage) {
    constexpr int NSLOT = QM_CLS * NMAX, LW = NSLOT / 4, XS = 256 / TT, LX = NSLOT / XS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, xt = tid & (TT - 1), xs = tid / TT;
    const int MS = qm_stride(E.W.M);
    const size_t AB = qg_a_bytes(true);
    const float * wrow = E.W.mt + min(r0 + lane, MS - 1);
    const int tx = min(tok0 + xt, T - 1);
    const float * xrow = (const float *)(E.in.tq + (size_t)(tx / QG_TOK) * cls.nb * AB + QG_A_S) + tx % QG_TOK;
    float lw[LW], lx[LX];
    auto gload = [&](int sg) {
#pragma unroll
        for (int k = 0; k < LW; k++) lw[k] = wrow[(size_t)cls.blk(sg, wave + 4 * k) * MS];
#pragma unroll
        for (int k = 0; k < LX; k++) lx[k] = xrow[(size_t)cls.blk(sg, xs + XS * k) * (AB / 4)];
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int k = 0; k < LW; k++) qw[buf][wave + 4 * k][lane] = lw[k];
#pragma unroll
        for (int k = 0; k < LX; k++) qx[buf][xs + XS * k][xt] = lx[k];
    };
    gload(0);
    lstore(0);
    __syncthreads();
#pragma unroll 1
    for (int sg = 0; sg < 64 / QM_CLS; sg++) {
        if (sg + 1 < 64 / QM_CLS) gload(sg + 1);  // in flight under this stage
        stage(sg, qw[sg & 1], qx[sg & 1]);
        if (sg + 1 < 64 / QM_CLS) lstore((sg + 1) & 1);
        __syncthreads();
    }
}

// Workgroup = 64 rows x 64 tokens (lane: 4 rows x 4 tokens; wave w: tokens 16w..16w+15): a block costs
// a lane two b128 reads (4 rows' m_w, 4 tokens' s_x) for 16 multiply-adds.
// NMAX = blocks per class rounded up to 1 / 2 / 4 (K <= 8192).
// FULL: every class has at least one block (K >= 2048): a class's chain starts with its first
// multiply-add on a literal 0 -- no zeroed accumulators.
template <int NMAX, bool FULL>
__global__ __launch_bounds__(256) void k_qg_msum(MMGroup g) {
    constexpr int NSLOT = QM_CLS * NMAX;
    __shared__ __attribute__((aligned(16))) float qw[2][NSLOT][64];
    __shared__ __attribute__((aligned(16))) float qx[2][NSLOT][64];
    const QMTile t = qm_tile<64>(g);
    const MMEntry & E = g.e[t.e];
    const int M = E.W.M, T = g.T, r0 = t.rt * 64, tok0 = t.tg * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rq = lane & 15, tq = lane >> 4;  // this lane: rows 4 rq + r, tokens 16 wave + 4 tq + c
    const QMClasses cls(E.W.K >> 5);
    float st[6][16], acc[16];
    qm_zero(acc);
    qm_stages<NMAX, 64>(E, cls, T, r0, tok0, qw, qx, [&](int sg, const float (&bw)[NSLOT][64], const float (&bx)[NSLOT][64]) {
        auto rd = [&](QMTileOps & o, int lc, int u) {
            o.w = *(const float4 *)&bw[u * 8 + lc][4 * rq];
            o.x = *(const float4 *)&bx[u * 8 + lc][16 * wave + 4 * tq];
        };
        if constexpr (NMAX <= 2) {
            // a class's operands (all NMAX slots; slots past its block count hold stale values, never
            // used) are read before the previous class's arithmetic: double-buffered registers
            QMTileOps o0[NMAX], o1[NMAX];
            auto rdc = [&](QMTileOps (&o)[NMAX], int lc) {
#pragma unroll
                for (int u = 0; u < NMAX; u++) rd(o[u], lc, u);
            };
            rdc(o0, 0);
            QMSubtree<16> tree;
            tree.run(sg, st, [&](float (&a)[16], int lc) {
                const int n = cls.size(sg * QM_CLS + lc);
                qm_zero(a);
                if (lc & 1) {
                    if (lc + 1 < QM_CLS) rdc(o0, lc + 1);
                    qm_chain(a, o1, n, FULL);
                } else {
                    rdc(o1, lc + 1);
                    qm_chain(a, o0, n, FULL);
                }
            });
        } else {
#pragma unroll 1
            for (int lc = 0; lc < QM_CLS; lc++) {
                const int l = sg * QM_CLS + lc;
                qm_mac4<NMAX, QMTileOps>(acc, rd, lc, 0, cls.size(l), false);
                qm_fold(l, st, acc);
            }
        }
    });
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = r0 + 4 * rq + r;
        if (row >= M) continue;
        float * out = g.m2 + E.moff + (size_t)row * T;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int tk = tok0 + 16 * wave + 4 * tq + c;
            if (tk < T) out[tk] = st[0][4 * r + c];
        }
    }
}

// The row form (32 or fewer tokens, and 5-16 blocks per class: K > 8192): lane = row, wave = 8
// tokens, workgroup = 64 rows x 32 tokens; a lane's m_w is one b32 read and the wave's 8 s_x two
// broadcast b128 reads per block (the 4 x 4 register tiles of k_qg_msum need 260 VGPRs at 8 blocks
// per class: one wave per SIMD).  NMAX = 1 / 2 / 4 / 8 / 16 (K <= 32768, e.g. a 20480-wide FFN value).
template <int NMAX, bool FULL>
__global__ __launch_bounds__(256) void k_qg_msum_rows(MMGroup g) {
    constexpr int NSLOT = QM_CLS * NMAX;
    __shared__ __attribute__((aligned(16))) float qw[2][NSLOT][64];
    __shared__ __attribute__((aligned(16))) float qx[2][NSLOT][32];
    const QMTile t = qm_tile<32>(g);
    const MMEntry & E = g.e[t.e];
    const int M = E.W.M, T = g.T, r0 = t.rt * 64, tok0 = t.tg * 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const QMClasses cls(E.W.K >> 5);
    float st[6][8], acc[8];
    qm_zero(acc);
    qm_stages<NMAX, 32>(E, cls, T, r0, tok0, qw, qx, [&](int sg, const float (&bw)[NSLOT][64], const float (&bx)[NSLOT][32]) {
        auto rd = [&](QMRowOps & o, int lc, int u) {
            o.w = bw[u * 8 + lc][lane];
            o.s0 = *(const float4 *)&bx[u * 8 + lc][8 * wave];
            o.s1 = *(const float4 *)&bx[u * 8 + lc][8 * wave + 4];
        };
        if constexpr (NMAX <= 2) {
            // as k_qg_msum's double-buffered operands, folded by the runtime counter
            QMRowOps o0[NMAX], o1[NMAX];
            auto rdc = [&](QMRowOps (&o)[NMAX], int lc) {
#pragma unroll
                for (int u = 0; u < NMAX; u++) rd(o[u], lc, u);
            };
            rdc(o0, 0);
#pragma unroll
            for (int lc = 0; lc < QM_CLS; lc += 2) {
                const int l = sg * QM_CLS + lc;
                rdc(o1, lc + 1);
                qm_chain(acc, o0, cls.size(l), false);
                qm_fold(l, st, acc);
                if (lc + 2 < QM_CLS) rdc(o0, lc + 2);
                qm_chain(acc, o1, cls.size(l + 1), false);
                qm_fold(l + 1, st, acc);
            }
        } else if constexpr (FULL) {
            // each class's first 4 blocks peeled so its chain starts on a literal 0
            QMSubtree<8> tree;
            tree.run(sg, st, [&](float (&a)[8], int lc) {
                const int n = cls.size(sg * QM_CLS + lc);
                qm_zero(a);
                qm_mac4<NMAX, QMRowOps>(a, rd, lc, 0, n, true);
#pragma unroll 1
                for (int u0 = 4; u0 < n; u0 += 4) qm_mac4<NMAX, QMRowOps>(a, rd, lc, u0, n, false);
            });
        } else {
#pragma unroll 1
            for (int lc = 0; lc < QM_CLS; lc++) {
                const int l = sg * QM_CLS + lc, n = cls.size(l);
#pragma unroll 1
                for (int u0 = 0; u0 < n; u0 += 4) qm_mac4<NMAX, QMRowOps>(acc, rd, lc, u0, n, false);
                qm_fold(l, st, acc);
            }
        }
    });
    const int r = r0 + lane;
    if (r >= M) return;
    float * out = g.m2 + E.moff + (size_t)r * T + tok0 + 8 * wave;
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (tok0 + 8 * wave + k < T) out[k] = st[0][k];
}

// One instantiation's launch, and the instantiations in the order they are tried: the first whose
// form matches, whose NMAX holds the group's longest class and whose FULL the group satisfies
template <bool ROWS, int NMAX, bool FULL>
static void qm_launch(hipStream_t st, MMGroup & g, int blocks) {
    if constexpr (ROWS) RK_LAUNCH((k_qg_msum_rows<NMAX, FULL>), dim3(blocks), dim3(256), 0, st, g);
    else RK_LAUNCH((k_qg_msum<NMAX, FULL>), dim3(blocks), dim3(256), 0, st, g);
}
struct QMForm {
    bool rows;
    int nmax;
    bool full;
    void (*launch)(hipStream_t, MMGroup &, int);
};
template <bool ROWS, int NMAX, bool FULL>
static constexpr QMForm qm_form() {
    return {ROWS, NMAX, FULL, qm_launch<ROWS, NMAX, FULL>};
}
static const QMForm kQMForms[] = {
    qm_form<true, 1, false>(),  qm_form<true, 2, false>(),  qm_form<true, 4, false>(),  qm_form<true, 8, true>(),
    qm_form<true, 8, false>(),  qm_form<true, 16, false>(), qm_form<false, 1, true>(),  qm_form<false, 1, false>(),
    qm_form<false, 2, true>(),  qm_form<false, 2, false>(), qm_form<false, 4, false>(),
};

// The m*s totals of a _1 group into g.m2 (every entry's moff set here), ahead of its GEMM; nothing
// for the _0 formats
bool launch_qg_msum(hipStream_t st, MMGroup & g, int wtype) {
    if (!qg_one(wtype)) return true;
    size_t mfl = 0;
    int mtiles = 0, nmax = 0;
    bool full = true;  // every entry's classes hold >= 1 block
    for (int i = 0; i < g.n; i++) {
        if (!g.e[i].W.mt) {
            fprintf(stderr, "rwkv: qgemm _1 entry %d without mins\n", i);
            return false;
        }
        g.e[i].moff = mfl;
        mfl += (size_t)g.T * g.e[i].W.M;
        mtiles += (g.e[i].W.M + 63) / 64;
        const int nbi = g.e[i].W.K / 32;
        nmax = std::max(nmax, (nbi + 63) / 64);
        full = full && nbi >= 64;
    }
    if (!g.m2 || g.m2_floats < mfl) {
        fprintf(stderr, "rwkv: qgemm _1 group needs %zu m*s floats, has %zu\n", mfl, g.m2 ? g.m2_floats : (size_t)0);
        return false;
    }
    // the 4 x 4 register-tile form over 64-token tiles; the row form (32-token tiles) for 32 or
    // fewer tokens (contexts) and for classes of more than 4 blocks
    const bool rows = g.T <= 32 || nmax > 4;
    const int blocks = mtiles * (rows ? (g.T + 31) / 32 : (g.T + 63) / 64);
    for (const QMForm & f : kQMForms) {
        if (f.rows != rows || nmax > f.nmax || (f.full && !full)) continue;
        f.launch(st, g, blocks);
        HIP_OK(hipGetLastError());
        return true;
    }
    fprintf(stderr, "rwkv: qgemm _1 group: K above the m*s pass's 32768\n");
    return false;
}

}  // namespace rwkvmi
