// qgemm.hip -- token-batched dequant GEMM for the sequence path (T > 1) on int8 MFMA.
//
// Y[t][m] = sum_b d_w[m,b] d_x[t,b] sumi(m,t,b) (+ m_w s_x for the _1 formats), the ggml block
// arithmetic of rwkv_graph.inc's ggml_mul_mat calls with Q8_0/Q8_1 activations.  One
// v_mfma_i32_16x16x32_i8 is exactly one 32-weight quantization block, so the MFMA produces the
// exact integer block dot sumi for a 16x16 (rows x tokens) tile; the fp32 scale arithmetic
// runs in the epilogue of every block and reproduces the decode matvec's association bit for
// bit: the blocks of class l = b mod 64 (lane l of k_mv / k_mm) are chained with fmaf in
// ascending b, and the 64 class sums are folded with wave_sum63's perfect binary tree (a binary
// counter over the classes).  So serial decode and sequence evaluation stay bit-identical.
//
// Operands come as tile records (common.hpp qg_*): per (row tile, block) one contiguous weight
// record, per (64-token tile, block) one contiguous activation record, so every copy
// instruction moves 1 KiB of consecutive bytes.  Workgroup = 4 waves as 2 (rows) x 2 (tokens)
// over a 32*TI-row x 64-token tile; a wave owns TI 16-row tiles x 2 16-token tiles.  Blocks are
// consumed in class-major order in chunks of 8 steps; each chunk's records are copied
// global->LDS (LDS DMA) by the four waves while the previous chunk is computed from the other
// LDS buffer, and within a chunk the LDS operands of step k+1 are read while step k's epilogue
// runs.
#include "device_common.hpp"
#include "kernels.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

// m0 in the copy asm's clobber list is a reserved register: the compiler re-sets m0 before each of
// its own uses (none in this file besides these copies)
#pragma clang diagnostic ignored "-Winline-asm"

namespace rwkvmi {

typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;

// Global->LDS copy (LDS DMA) of one 1-KiB piece: buffer_load_dwordx4 ... lds puts lane i's 16
// bytes from base + soff + voff + OFF at LDS m0 + OFF + 16 i (tools/bufdma_check.hip).  Issued as
// inline asm on purpose: the compiler cannot tell a copy into one LDS buffer from reads of the
// other and would drain vmcnt before every LDS read; the kernel orders the copies itself
// (s_waitcnt vmcnt(0) + barrier per chunk, qg_chunk_done).  M0 is written in the same statement
// (the compiler does not preserve it) and needs one wait state before the load.
template <int OFF>
__device__ __forceinline__ void qg_bdma(v4i_t rsrc, unsigned soff, unsigned m0, unsigned voff) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %2, %3 offen offset:%4 lds" ::"v"(voff),
                 "s"(m0), "s"(rsrc), "s"(soff), "i"(OFF)
                 : "m0");
}

// raw buffer descriptor over [base, base + 4 GiB) (gfx9 dword3 0x00020000)
__device__ __forceinline__ v4i_t qg_rsrc(const void * base) {
    v4i_t r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned long)base);
    r.y = __builtin_amdgcn_readfirstlane((int)((unsigned long)base >> 32));
    r.z = -1;
    r.w = 0x00020000;
    return r;
}

// One record of BYTES into LDS at m0: full 1-KiB pieces plus a partial last piece
template <int BYTES, int P = 0>
__device__ __forceinline__ void qg_record(v4i_t rsrc, unsigned soff, unsigned m0, int lane) {
    if constexpr (P * 1024 < BYTES) {
        if constexpr ((P + 1) * 1024 <= BYTES) {
            qg_bdma<P * 1024>(rsrc, soff, m0, lane * 16);
        } else if (lane * 16 < BYTES - P * 1024) {
            qg_bdma<P * 1024>(rsrc, soff, m0, lane * 16);
        }
        qg_record<BYTES, P + 1>(rsrc, soff, m0, lane);
    }
}

// All of this wave's copies have landed; the barrier then publishes every wave's copies.
__device__ __forceinline__ void qg_chunk_done() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

constexpr int QG_STEPS = 8;  // blocks per chunk

template <int WF>
struct QGLayout {
    static constexpr bool ONE = qg_one(WF);
    static constexpr int TI = 2;
    static constexpr int ROWS = qg_rows(WF);        // = 32 * TI
    static constexpr int WB = qg_w_bytes(WF);       // weight record
    static constexpr int AB = qg_a_bytes(ONE);      // activation record (stride)
    static constexpr int AC = QG_A_S;               // of which copied: the int8 values and d (Q8_1's s
                                                    // feeds k_qg_msum, not this kernel)
    static constexpr int STEP = WB + AC;            // LDS bytes per step: [weight rec][act rec]
    static constexpr int BUF = STEP * QG_STEPS;
    static constexpr int WP = (WB + 1023) / 1024;   // copy instructions per record
    static constexpr int AP = (AC + 1023) / 1024;
    static constexpr int JOBS = WP + AP;
    static_assert(ROWS == 32 * TI && WB % 16 == 0 && AB % 16 == 0 && AC % 16 == 0, "qgemm layout");
};

// Class-major walk over the blocks: class l (= b mod 64) has n = q + (l < rem) blocks, q = nb/64,
// rem = nb%64; step s of the walk is block l + 64 u.  Scalar state, advanced one step at a time.
struct QGWalk {
    int q, rem, l, u, n;
    __device__ __forceinline__ void init(int nb, int l0 = 0) {
        q = nb >> 6;
        rem = nb & 63;
        l = l0;
        u = 0;
        n = q + (l0 < rem ? 1 : 0);
    }
    __device__ __forceinline__ int block() const { return l + 64 * u; }
    __device__ __forceinline__ void next() {
        if (++u == n) {
            l++;
            u = 0;
            n = q + (l < rem ? 1 : 0);
        }
    }
};

// Where a workgroup works and what each lane of it holds
template <int WF>
struct QGTile {
    int e, nb, sidx;         // the entry whose workgroup range holds blockIdx.x, its blocks per row, the split
    int lane, wave, r16, h;  // lane = r16 + 16 h: D-layout rows 4h..4h+3 of token r16 of a 16 x 16 tile
    int row0, tok0, wr, wt;  // the tile's first row / token; this wave's tile-local row / token
    v4i_t rw, ra;            // the row tile's weight records, the token tile's activation records
    unsigned lds0;           // LDS address of smem
};
// NB: the blocks per row where the kernel fixes them (k_qgemm_k64), 0: the entry's K / 32
template <int WF, int SPLIT, int NB>
__device__ __forceinline__ QGTile<WF> qg_tile(const MMGroup & g, const void * smem) {
    using Lt = QGLayout<WF>;
    QGTile<WF> t;
    t.e = 0;
#pragma unroll 1
    while (t.e + 1 < g.n && (int)blockIdx.x >= g.e[t.e + 1].block0) t.e++;
    const MMEntry & E = g.e[t.e];
    t.nb = NB ? NB : E.W.K >> 5;
    const int tilesT = (g.T + QG_TOK - 1) / QG_TOK;
    const int local0 = (int)blockIdx.x - E.block0;
    const int local = local0 / SPLIT, mtile = local / tilesT, ttile = local % tilesT;
    t.sidx = local0 % SPLIT;
    t.lane = threadIdx.x & 63;
    t.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    t.r16 = t.lane & 15;
    t.h = t.lane >> 4;
    t.row0 = mtile * Lt::ROWS;
    t.tok0 = ttile * QG_TOK;
    t.wr = (t.wave & 1) * 16 * Lt::TI;
    t.wt = (t.wave >> 1) * 32;
    t.rw = qg_rsrc(E.W.gt + (size_t)mtile * t.nb * Lt::WB);
    t.ra = qg_rsrc(E.in.tq + (size_t)ttile * t.nb * Lt::AB);
    t.lds0 = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(lds_void_t *)smem);
    return t;
}

// This wave's share of chunk c: steps 8c + wave and 8c + wave + 4 (the walk is at the first of
// them and is left at 8(c+1) + wave).
template <int WF>
__device__ __forceinline__ void qg_load_chunk(const QGTile<WF> & t, unsigned lds_buf, int c, QGWalk & wk, int nsteps) {
    using Lt = QGLayout<WF>;
#pragma unroll
    for (int h2 = 0; h2 < 2; h2++) {
        const int k = t.wave + 4 * h2;
        if (c * QG_STEPS + k < nsteps) {
            const int b = wk.block();
            const unsigned m = lds_buf + k * Lt::STEP;
            qg_record<Lt::WB>(t.rw, (unsigned)(b * Lt::WB), m, t.lane);
            qg_record<Lt::AC>(t.ra, (unsigned)(b * Lt::AB), m + Lt::WB, t.lane);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) wk.next();
    }
}

// LDS operands of one step for one wave
template <int TI>
struct QGOps {
    long af[TI], xf[2];
    float4 sd[TI];  // d of the 4 D-layout rows 4h..4h+3 of each 16-row tile
    float dx[2];
};

// The 8-byte operand reads stay single ds_read_b64 (2 LDS cycles, 64 banks): the compiler would
// otherwise pair reads of consecutive steps into ds_read2st64_b64, which the LDS serves as two
// 16-lane-group accesses over 32 banks (8 cycles per pair, and tokens t / t + 8 of the activation
// record then share banks).  QG_MERGED_READS restores the compiler's pairing (A/B builds).
#ifdef QG_MERGED_READS
typedef const long qg_op_t;
#else
typedef __attribute__((address_space(3))) const volatile long qg_op_t;
#endif

template <int WF>
__device__ __forceinline__ void qg_read_ops(const char * sp, QGOps<QGLayout<WF>::TI> & o, const QGTile<WF> & t) {
    using Lt = QGLayout<WF>;
    const int wr = t.wr, wt = t.wt, r16 = t.r16, h = t.h;
#pragma unroll
    for (int i = 0; i < Lt::TI; i++) {
        o.af[i] = *(qg_op_t *)(sp + qg_w_off(wr + 16 * i + r16, h * 8));  // int8 row, k = 8h..8h+7
        const int ro = wr + 16 * i + 4 * h;
        o.sd[i] = *(const float4 *)(sp + qg_w_d(WF) + ro * 4);
    }
    const char * ap = sp + Lt::WB;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int tl = wt + 16 * j + r16;
        o.xf[j] = *(qg_op_t *)(ap + (h >> 1) * QG_TOK * 16 + tl * 16 + (h & 1) * 8);
        o.dx[j] = *(const float *)(ap + QG_A_D + tl * 4);
    }
}

typedef float qf2_t __attribute__((ext_vector_type(2)));

// The MFMA accumulates each block's integer dot onto QG_BIAS = 0x4B400000 (1.5 * 2^23 as a float),
// so the result read as a float is 12582912 + sumi exactly (|sumi| < 2^22), and one packed
// subtraction recovers (float)sumi for two outputs: no per-output int->float conversion.
constexpr int QG_BIAS = 0x4B400000;
constexpr float QG_BIAS_F = 12582912.0f;

// The TI x 2 MFMAs of one step (one quantization block) from this step's LDS operands
template <int TI>
__device__ __forceinline__ void qg_mfma(const QGOps<TI> & cur, v4i_t (&sv)[TI][2]) {
    const v4i_t bias = {QG_BIAS, QG_BIAS, QG_BIAS, QG_BIAS};
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) sv[i][j] = __builtin_amdgcn_mfma_i32_16x16x32_i8(cur.af[i], cur.xf[j], bias, 0, 0, 0);
}

// The fp32 block epilogue: acc = fma(d_w * d_x, sumi, acc), rows in pairs (packed f32: bitwise the
// scalar operations, tools/pk_probe.hip); FIRST: the class's first block (its chain starts from 0)
template <bool FIRST, int TI>
__device__ __forceinline__ void qg_epi(const QGOps<TI> & cur, const v4i_t (&sv)[TI][2], float (&acc)[TI][2][4]) {
    const qf2_t nbias = {-QG_BIAS_F, -QG_BIAS_F};
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int qp = 0; qp < 2; qp++) {
            const qf2_t dw = qp ? qf2_t{cur.sd[i].z, cur.sd[i].w} : qf2_t{cur.sd[i].x, cur.sd[i].y};
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const qf2_t dx = {cur.dx[j], cur.dx[j]};
                const qf2_t si = qf2_t{__int_as_float(sv[i][j][2 * qp]), __int_as_float(sv[i][j][2 * qp + 1])} + nbias;
                const qf2_t a0 = FIRST ? qf2_t{0.0f, 0.0f} : qf2_t{acc[i][j][2 * qp], acc[i][j][2 * qp + 1]};
                const qf2_t a = __builtin_elementwise_fma(dw * dx, si, a0);
                acc[i][j][2 * qp] = a.x;
                acc[i][j][2 * qp + 1] = a.y;
            }
        }
}

// y[t][m] = epi(total + t2), t2 = the m*s total (m2, _1 formats; k_qg_msum) or +0.0f, as k_mm's
// red + red2.  A lane holds rows 4h..4h+3 of one token: one 16-byte access per (token, 4 rows)
// when aligned.
template <int WF, int TI>
__device__ __forceinline__ void qg_store(const MMEntry & E, const float * m2, int T, const QGTile<WF> & tile,
                                         const float (&tot)[TI][2][4]) {
    const int M = E.W.M, tok0 = tile.tok0, row0 = tile.row0, wt = tile.wt, wr = tile.wr, r16 = tile.r16, h = tile.h;
    if constexpr (TI == 2) {
        if (E.fuse_emit) {
            // The wave's 32 rows (wr % 32 == 0) of a token are one quantization block of the next
            // matmul's input: lanes r16 + 16 h hold rows 16 i + 4 h + q.  quant32 / store32's values:
            // amax and sum over the block by xor-16/32 lane exchanges (order-free), ggml rounding.
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int t = tok0 + wt + 16 * j + r16;
                const int tc = min(t, T - 1);
                float v[2][4];
                float am = 0.0f;
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int mb = row0 + wr + 16 * i + 4 * h;
                    float t2q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (m2)
#pragma unroll
                        for (int q = 0; q < 4; q++) t2q[q] = m2[(size_t)(mb + q) * T + tc];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        v[i][q] = apply_epi_v(E, mb + q, tot[i][j][q] + t2q[q], 0.0f, 0.0f);
                        am = fmaxf(am, fabsf(v[i][q]));
                    }
                }
                am = fmaxf(am, __shfl_xor(am, 16));
                am = fmaxf(am, __shfl_xor(am, 32));
                const float d = am / 127.f;
                const float id = (am != 0.0f) ? 127.f / am : 0.0f;
                uint32_t packed[2];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    packed[i] = 0;
#pragma unroll
                    for (int q = 0; q < 4; q++) packed[i] |= ((uint32_t)(int)rintf(v[i][q] * id) & 0xffu) << (8 * q);
                }
                if (t < T) {
                    uint8_t * rec = E.out.tq + ((size_t)(t / QG_TOK) * (M >> 5) + ((row0 + wr) >> 5)) * qg_a_bytes(false);
                    const int tl = t % QG_TOK;
#pragma unroll
                    for (int i = 0; i < 2; i++) *(uint32_t *)(rec + i * QG_TOK * 16 + tl * 16 + 4 * h) = packed[i];
                    if (h == 0) ((float *)(rec + QG_A_D))[tl] = f16_round(d);
                }
            }
            return;
        }
    }
    const bool vec = ((E.ldy | M) & 3) == 0 && (((uintptr_t)E.y | (uintptr_t)E.aux) & 15) == 0;
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int t = tok0 + wt + 16 * j + r16;
            const int m0 = row0 + wr + 16 * i + 4 * h;
            if (t >= T || m0 >= M) continue;
            float acc[4];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = tot[i][j][q] + (m2 && m0 + q < M ? m2[(size_t)(m0 + q) * T + t] : 0.0f);
            float * yp = E.y + (size_t)t * E.ldy + m0;
            if (vec) {
                float4 yv = make_float4(0.f, 0.f, 0.f, 0.f), av = yv;
                if (epi_reads_y(E.epi)) yv = *(const float4 *)yp;
                if (epi_reads_aux(E.epi)) av = *(const float4 *)(E.aux + (size_t)t * E.ldy + m0);
                float4 o;
                o.x = apply_epi_v(E, m0, acc[0], yv.x, av.x);
                o.y = apply_epi_v(E, m0 + 1, acc[1], yv.y, av.y);
                o.z = apply_epi_v(E, m0 + 2, acc[2], yv.z, av.z);
                o.w = apply_epi_v(E, m0 + 3, acc[3], yv.w, av.w);
                *(float4 *)yp = o;
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (m0 + q < M) yp[q] = apply_epi(E, t, m0 + q, acc[q]);
            }
        }
}

// Split-K: one split's subtree sums to its entry's partials [S][T][M]
template <int WF, int TI>
__device__ __forceinline__ void qg_store_part(float * part, int T, int M, const QGTile<WF> & tile,
                                              const float (&sub)[TI][2][4]) {
    const int sidx = tile.sidx, tok0 = tile.tok0, row0 = tile.row0, wt = tile.wt, wr = tile.wr, r16 = tile.r16, h = tile.h;
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int t = tok0 + wt + 16 * j + r16;
            const int m0 = row0 + wr + 16 * i + 4 * h;
            if (t >= T) continue;
            float * pp = part + ((size_t)sidx * T + t) * M + m0;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (m0 + q < M) pp[q] = sub[i][j][q];
        }
}

// Class-pair fold: the odd class (in c) closes N >= 1 levels of the binary counter: v = c, then
// v = st[k] + v for k < N, into st[N] (N < 6) or the total (N = 6).  Packed f32 over output pairs
// (v_pk_add_f32: per element the scalar add's bits; this file builds without the SLP vectorizer).
template <int TI, int N>
__device__ __forceinline__ void qg_fold(float (&st)[6][TI][2][4], const float (&c)[TI][2][4], float (&tot)[TI][2][4]) {
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int q = 0; q < 4; q += 2) {
                qf2_t v = {c[i][j][q], c[i][j][q + 1]};
#pragma unroll
                for (int kk = 0; kk < N; kk++) v = qf2_t{st[kk][i][j][q], st[kk][i][j][q + 1]} + v;
                if constexpr (N < 6) {
                    st[N][i][j][q] = v.x;
                    st[N][i][j][q + 1] = v.y;
                } else {
                    tot[i][j][q] = v.x;
                    tot[i][j][q + 1] = v.y;
                }
            }
}
// qg_fold for a runtime n in [1, 6]: the odd class l closes n = ctz(~l) levels
template <int TI>
__device__ __forceinline__ void qg_close(int n, float (&st)[6][TI][2][4], const float (&c)[TI][2][4],
                                         float (&tot)[TI][2][4]) {
    switch (n) {
        case 1: qg_fold<TI, 1>(st, c, tot); break;
        case 2: qg_fold<TI, 2>(st, c, tot); break;
        case 3: qg_fold<TI, 3>(st, c, tot); break;
        case 4: qg_fold<TI, 4>(st, c, tot); break;
        case 5: qg_fold<TI, 5>(st, c, tot); break;
        default: qg_fold<TI, 6>(st, c, tot); break;
    }
}

// K = 2048 (64 blocks: every class is one block, the walk is block order): the same arithmetic
// as k_qgemm with the step bookkeeping resolved at compile time -- each 8-step chunk is
// straight-line code (the class-pair folds after steps 1, 3, 5 close 1, 2, 1 levels; after step
// 7, 3 + ctz(~chunk) levels), and the copy walk is blocks 8c + wave, 8c + wave + 4.
// SPLIT > 1 (split-K when a group has few tiles): workgroup s of a tile runs chunks
// [s * NCHL, (s + 1) * NCHL) -- a complete subtree of the perfect binary tree over the 64 classes --
// and stores that subtree sum (and, _1 formats, the m*s subtree) to its entry's partials;
// k_qg_combine adds the SPLIT subtrees with the tree's top levels and applies the epilogue (and
// the emission), so results equal the unsplit kernel bit for bit.
template <int WF, int SPLIT = 1>
__global__ __launch_bounds__(256) void k_qgemm_k64(MMGroup g) {
    using Lt = QGLayout<WF>;
    constexpr bool ONE = Lt::ONE;
    constexpr int TI = Lt::TI;
    constexpr int NB = 64, NCH = NB / QG_STEPS, NCHL = NCH / SPLIT;
    __shared__ __attribute__((aligned(16))) char smem[2][Lt::BUF];
    const QGTile<WF> t = qg_tile<WF, SPLIT, NB>(g, smem);
    const MMEntry & E = g.e[t.e];
    const int ch0 = t.sidx * NCHL;
    auto load = [&](int c, unsigned buf) {
#pragma unroll
        for (int h2 = 0; h2 < 2; h2++) {
            const int k = t.wave + 4 * h2, b = c * QG_STEPS + k;
            const unsigned m = buf + k * Lt::STEP;
            qg_record<Lt::WB>(t.rw, (unsigned)(b * Lt::WB), m, t.lane);
            qg_record<Lt::AC>(t.ra, (unsigned)(b * Lt::AB), m + Lt::WB, t.lane);
        }
    };
    float st[6][TI][2][4];
    float tot[TI][2][4];
    float c[TI][2][4];
    load(ch0, t.lds0);
    qg_chunk_done();
    if (NCHL > 1) load(ch0 + 1, t.lds0 + Lt::BUF);
    QGOps<TI> cur;
    qg_read_ops<WF>(smem[0], cur, t);
#pragma unroll 1
    for (int ch = 0; ch < NCHL; ch++) {  // local chunk index (the subtree's own tree)
        const char * buf = smem[ch & 1];
#pragma unroll
        for (int k = 0; k < QG_STEPS; k++) {
            v4i_t sv[TI][2];
            qg_mfma<TI>(cur, sv);
            QGOps<TI> nxt = cur;
            if (k + 1 < QG_STEPS) qg_read_ops<WF>(buf + (k + 1) * Lt::STEP, nxt, t);
            if (k & 1) {
                qg_epi<true, TI>(cur, sv, c);
                qg_close<TI>(k == 1 || k == 5 ? 1 : k == 3 ? 2 : 3 + __builtin_ctz(~ch), st, c, tot);
            } else {
                qg_epi<true, TI>(cur, sv, st[0]);
            }
            cur = nxt;
        }
        if (ch + 1 < NCHL) {
            qg_chunk_done();  // chunk ch+1 has landed and buffer ch&1 is free
            if (ch + 2 < NCHL) load(ch0 + ch + 2, t.lds0 + (ch & 1) * Lt::BUF);
            qg_read_ops<WF>(smem[(ch + 1) & 1], cur, t);
        }
    }
    if constexpr (SPLIT == 1) {
        qg_store(E, ONE ? g.m2 + E.moff : nullptr, g.T, t, tot);
    } else {
        // the subtree over this split's 8 * NCHL classes sits at level 3 + log2(NCHL)
        constexpr int LEV = NCHL == 1 ? 3 : NCHL == 2 ? 4 : 5;
        qg_store_part(g.part + E.poff, g.T, E.W.M, t, st[LEV]);
    }
}

// Split-K combine for a whole group: the top of the class tree over the SPLIT subtrees (8: three
// levels, 4: two), then qg_store's total (+ 0.0f, or + the m*s total for the _1 formats), the
// entry's epilogue, y, and -- for emitting entries -- the next matmul's input (emit32: one
// quantization block per 32 consecutive rows of a token, one half-wave).
template <int SPLIT, bool ONE>
__global__ __launch_bounds__(256) void k_qg_combine(MMGroup g) {
    int e = 0;
#pragma unroll 1
    while (e + 1 < g.n && (int)blockIdx.x >= g.e[e + 1].cblock0) e++;
    const MMEntry & E = g.e[e];
    const int M = E.W.M, T = g.T;
    const size_t i = (size_t)((int)blockIdx.x - E.cblock0) * 256 + threadIdx.x;
    if (i >= (size_t)T * M) return;  // T * M % 32 == 0: half-waves stay whole
    const int t = (int)(i / M), m = (int)(i % M);
    const float * pp = g.part + E.poff + (size_t)t * M + m;
    const size_t ss = (size_t)T * M;
    auto tree = [&](const float * p) {
        float v[SPLIT];
#pragma unroll
        for (int s = 0; s < SPLIT; s++) v[s] = p[s * ss];
        if constexpr (SPLIT == 8) return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        else if constexpr (SPLIT == 2) return v[0] + v[1];
        else return (v[0] + v[1]) + (v[2] + v[3]);
    };
    const float tot = tree(pp);
    float acc;
    if constexpr (ONE) acc = tot + g.m2[E.moff + (size_t)m * T + t];
    else acc = tot + 0.0f;
    const float v = apply_epi(E, t, m, acc);
    if (E.y) E.y[(size_t)t * E.ldy + m] = v;  // (k_fmm's emit-only entries have none)
    if (E.emit) emit32(E.out, t, m, v);
}

// SPLIT > 1: workgroup s of a tile walks classes [s * 64 / SPLIT, (s + 1) * 64 / SPLIT) only -- a
// complete subtree of the class tree -- and stores the subtree sums (qg_store_part) for k_qg_combine.
template <int WF, int SPLIT = 1>
__global__ __launch_bounds__(256) void k_qgemm(MMGroup g) {
    using Lt = QGLayout<WF>;
    constexpr bool ONE = Lt::ONE;
    constexpr int TI = Lt::TI;
    constexpr int CPS = 64 / SPLIT;  // classes per split
    __shared__ __attribute__((aligned(16))) char smem[2][Lt::BUF];
    const QGTile<WF> t = qg_tile<WF, SPLIT, 0>(g, smem);
    const MMEntry & E = g.e[t.e];
    const int nb = t.nb, l0 = t.sidx * CPS;
    const int cq = nb >> 6, crem = nb & 63;  // class sizes for the consumer
    // this split's steps: the blocks of classes [l0, l0 + CPS)
    const int nsteps = CPS * cq + min(max(crem - l0, 0), CPS);
    QGWalk ld;  // the loader's walk (this wave's steps)
    ld.init(nb, l0);
    for (int i = 0; i < t.wave; i++) ld.next();

    // Per output: class sums in a binary counter (wave_sum63's tree).  Classes are walked in
    // pairs: the even class accumulates straight into level 0 (st[0]), the odd one into c, and
    // the pair then folds upward -- no copies or resets of accumulators between classes (each
    // class's first block starts its chain from 0 in a peeled step).
    float st[6][TI][2][4];
    float tot[TI][2][4];
    float c[TI][2][4];
    const int nchunks = (nsteps + QG_STEPS - 1) / QG_STEPS;

    int k = 0, cb = 0, cn = 1;  // step within the chunk, its buffer, next chunk to issue
    // one block: MFMAs from this step's LDS operands, then the fp32 block epilogue into acc
    // LDS operands of the current step live in registers (cur); the next step's are read while
    // this step's epilogue runs, except across a chunk boundary (its buffer is not ready yet).
    QGOps<TI> cur;
    auto step = [&](auto first, float (&acc)[TI][2][4]) {
        constexpr bool FIRST = decltype(first)::value;
        // Chunk consumed: switch buffers (wave-uniform).  Done before this step's MFMAs, not
        // after them, so no branch separates an MFMA from the reads of its result.
        if (k == QG_STEPS) {
            k = 0;
            qg_chunk_done();  // the next chunk has landed and this buffer is free
#if defined(QG_PROBE) && QG_PROBE == 2
            if (cn < nchunks && cn < 2)  // tools/gemm_probe: compute only
#else
            if (cn < nchunks)
#endif
                qg_load_chunk(t, t.lds0 + cb * Lt::BUF, cn, ld, nsteps);
            cn++;
            cb ^= 1;
            qg_read_ops<WF>(smem[cb], cur, t);
        }
#if defined(QG_PROBE) && QG_PROBE == 1
        if (0)  // tools/gemm_probe: copies only
#endif
        {
            v4i_t sv[TI][2];
            qg_mfma<TI>(cur, sv);
            QGOps<TI> nxt = cur;
            if (k + 1 < QG_STEPS) qg_read_ops<WF>(smem[cb] + (k + 1) * Lt::STEP, nxt, t);
            qg_epi<FIRST, TI>(cur, sv, acc);
            cur = nxt;
        }
        k++;
    };
    using T1 = std::integral_constant<bool, true>;
    using T0 = std::integral_constant<bool, false>;
    auto zero_acc = [&](float (&acc)[TI][2][4]) {
#pragma unroll
        for (int i = 0; i < TI; i++)
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[i][j][q] = 0.0f;
    };
    // all blocks of class l into acc (a class without blocks, nb < 64, is a zero leaf)
    auto run_class = [&](int l, float (&acc)[TI][2][4]) {
        const int n = cq + (l < crem ? 1 : 0);
        if (n == 0) {
            zero_acc(acc);
            return;
        }
        step(T1{}, acc);
        for (int u = 1; u < n; u++) step(T0{}, acc);
    };

    if (nchunks > 0) qg_load_chunk(t, t.lds0, 0, ld, nsteps);
    qg_chunk_done();
    if (nchunks > 1) qg_load_chunk(t, t.lds0 + Lt::BUF, 1, ld, nsteps);
    cn = 2;
    qg_read_ops<WF>(smem[0], cur, t);
    for (int pr = 0; pr < CPS / 2; pr++) {  // pairs of this split's classes; folds by the relative index
        run_class(l0 + 2 * pr, st[0]);
        run_class(l0 + 2 * pr + 1, c);
        qg_close<TI>(__builtin_ctz(~(2 * pr + 1)), st, c, tot);
    }
    // copies of a partial last chunk (or of none) were never waited for: drain before exit
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    if constexpr (SPLIT == 1) {
        qg_store(E, ONE ? g.m2 + E.moff : nullptr, g.T, t, tot);
    } else {
        constexpr int LEV = SPLIT == 8 ? 3 : SPLIT == 4 ? 4 : 5;  // the subtree of CPS classes
        qg_store_part(g.part + E.poff, g.T, E.W.M, t, st[LEV]);
    }
}

// Runtime value -> template argument: f(std::integral_constant<int, V>) for the V among Vs that
// equals v; false when none does
template <int... Vs, class F>
static bool qg_dispatch(int v, F && f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// The combine of a split group whose entries' partials sit at g.part + poff (launch_qgemm's and
// k_fmm's split forms); one: the _1 formats' m*s totals at g.m2 + moff are added
bool launch_qg_combine(hipStream_t st, MMGroup & g, int split, bool one) {
    int cblocks = 0;
    for (int i = 0; i < g.n; i++) {
        g.e[i].cblock0 = cblocks;
        cblocks += (int)(((size_t)g.T * g.e[i].W.M + 255) / 256);
    }
    const bool known = qg_dispatch<2, 4, 8>(split, [&](auto sp) {
        constexpr int SP = decltype(sp)::value;
        if (one) RK_LAUNCH((k_qg_combine<SP, true>), dim3(cblocks), dim3(256), 0, st, g);
        else RK_LAUNCH((k_qg_combine<SP, false>), dim3(cblocks), dim3(256), 0, st, g);
    });
    if (!known) return false;
    HIP_OK(hipGetLastError());
    return true;
}

int g_qgemm_generic = 0;  // 1: K = 2048 through the generic kernel too (tools, comparison)
int kQgCUs = 256;          // compute units of the device (set_mv_device_cus): the split-K threshold

// Every entry's block0 (its first workgroup at one workgroup per tile); the group's tiles, or -1 for
// an entry the GEMM does not take
static int qg_validate(MMGroup & g, int wtype) {
    const int rows = qg_rows(wtype);
    const int tilesT = (g.T + QG_TOK - 1) / QG_TOK;
    int tiles = 0;
    for (int i = 0; i < g.n; i++) {
        MMEntry & e = g.e[i];
        if (e.W.type != wtype || !e.W.gt || e.W.K % 32 || !e.y || e.in.fmt != act_fmt_for(wtype) || !e.in.tiled ||
            !e.in.tq) {
            fprintf(stderr, "rwkv: qgemm entry %d not supported (type %d)\n", i, e.W.type);
            return -1;
        }
        e.block0 = tiles;
        tiles += (e.W.M + rows - 1) / rows * tilesT;
    }
    return tiles;
}

// Q8_0 emission fused into the direct kernel's epilogue (the Q4_0 / Q5_0 / Q8_0 GEMMs: a wave holds
// 32 rows, one block of the next matmul's input)
static bool qg_fuses_emit(const MMEntry & e) {
    return e.emit && e.out.tiled && e.out.fmt == A_Q8_0 && e.out.tq && e.out.K == e.W.M && e.W.M % 64 == 0 &&
           e.ldy == e.W.M && e.epi != EPI_ADD && e.epi != EPI_SIGMUL_ADD && e.epi != EPI_VMIX7 &&
           e.epi != EPI_DECAY6 && e.epi != EPI_DECAY7 && e.epi != EPI_SIGMOID_BIAS;
}

// Split-K when the group has few tiles (batched decode's 64-context tiles, small-M entries such as
// the v6 maa LoRA W1): every tile's class tree in 2, 4 or 8 subtrees on as many workgroups,
// combined (epilogue, emission) by k_qg_combine -- the same bits as the unsplit kernel.  Sets every
// entry's poff.
static int qg_choose_split(MMGroup & g, int tiles) {
    int split = g.split;
    if (split == 0) split = tiles >= 2 * kQgCUs ? 1 : tiles * 4 >= 2 * kQgCUs ? 4 : 8;
    if (split != 2 && split != 4 && split != 8) return 1;
    size_t pfl = 0;
    for (int i = 0; i < g.n; i++) {
        g.e[i].poff = pfl;
        pfl += (size_t)split * g.T * g.e[i].W.M;
    }
    if (!g.part || g.part_floats < pfl || g_qgemm_generic) return 1;
    for (int i = 0; i < g.n; i++)
        if (g.e[i].W.M % 32) return 1;  // combine: one emission block per half-wave
    return split;
}

// Every entry must have y (the engine gives emitting entries a scratch y).  Emission into the next
// matmul's activation format: the launch sets MMEntry::fuse_emit where it emits itself -- the direct
// kernel's epilogue writes Q8_0 token tiles INSTEAD of y (qg_fuses_emit), the split-K combine
// writes y and emits any format -- and an emitting entry left with fuse_emit == 0 is a separate
// launch_act_from_f32 pass by the caller.  The weights need their tile records (upload_mat) and the
// activations must be token tiles.
bool launch_qgemm(hipStream_t st, MMGroup & g, int wtype) {
    const int tiles = qg_validate(g, wtype);
    if (tiles <= 0) return tiles == 0;
    if (!launch_qg_msum(st, g, wtype)) return false;  // the m*s totals the epilogue / the combine reads
    for (int i = 0; i < g.n; i++) g.e[i].fuse_emit = qg_fuses_emit(g.e[i]);
    const int split = qg_choose_split(g, tiles);
    bool k64 = !g_qgemm_generic;
    for (int i = 0; i < g.n; i++) {
        k64 = k64 && g.e[i].W.K == 2048;
        g.e[i].block0 *= split;  // split workgroups per tile
    }
    const bool known = qg_dispatch<W_Q4_0, W_Q4_1, W_Q5_0, W_Q5_1, W_Q8_0>(wtype, [&](auto wf) {
        qg_dispatch<1, 2, 4, 8>(split, [&](auto sp) {
            constexpr int WF = decltype(wf)::value, SP = decltype(sp)::value;
            if (k64) RK_LAUNCH((k_qgemm_k64<WF, SP>), dim3(tiles * split), dim3(256), 0, st, g);
            else RK_LAUNCH((k_qgemm<WF, SP>), dim3(tiles * split), dim3(256), 0, st, g);
        });
    });
    if (!known) {
        fprintf(stderr, "rwkv: qgemm type %d unsupported\n", wtype);
        return false;
    }
    HIP_OK(hipGetLastError());
    if (split == 1) return true;
    for (int i = 0; i < g.n; i++) g.e[i].fuse_emit = g.e[i].emit;  // the combine emits
    return launch_qg_combine(st, g, split, qg_one(wtype));
}

}  // namespace rwkvmi
