// kernels.hip -- gfx950 kernels for the RWKV eval hot path.
//
// Numerics mirror the reference's CPU path (rwkv_graph.inc + ggml CPU ops), restated in
// oracle/oracle.c, and are compiled with -ffp-contract=off so every multiply/add rounds
// where the reference rounds; fused multiply-adds appear only where ggml's x86 kernels use
// them (the quantized block accumulation).
#include "kernels.hpp"

#include <algorithm>
#include "device_common.hpp"

#include <stdio.h>

namespace rwkvmi {



template <int WF, int RPW, int NT>
__device__ __forceinline__ void mm_accumulate(const MMEntry & E, int row0, int t0, int T, int lane,
                                              float (&acc)[RPW][NT], float (&acc2)[RPW][NT]) {
    const DMat & W = E.W;
    const int K = W.K, M = W.M;
    if constexpr (WF == W_F32) {
        for (int k = lane * 4; k < K; k += 256) {
            float4 x[NT];
#pragma unroll
            for (int n = 0; n < NT; n++)
                x[n] = (t0 + n < T) ? *(const float4 *)(E.in.f + (size_t)(t0 + n) * K + k) : make_float4(0, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < RPW; r++) {
                const int row = row0 + r;
                if (row < M) {
                    const float4 w = *(const float4 *)((const float *)W.qs + (size_t)row * K + k);
#pragma unroll
                    for (int n = 0; n < NT; n++) {
                        float a = acc[r][n];
                        a = fmaf(w.x, x[n].x, a);
                        a = fmaf(w.y, x[n].y, a);
                        a = fmaf(w.z, x[n].z, a);
                        a = fmaf(w.w, x[n].w, a);
                        acc[r][n] = a;
                    }
                }
            }
        }
    } else if constexpr (WF == W_F16) {
        for (int k = lane * 8; k < K; k += 512) {
            int4 x[NT];
#pragma unroll
            for (int n = 0; n < NT; n++)
                x[n] = (t0 + n < T) ? *(const int4 *)(E.in.h + (size_t)(t0 + n) * K + k) : make_int4(0, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < RPW; r++) {
                const int row = row0 + r;
                if (row < M) {
                    const int4 w = *(const int4 *)((const __half *)W.qs + (size_t)row * K + k);
#pragma unroll
                    for (int n = 0; n < NT; n++) {
                        acc[r][n] = dot8_f16(w, x[n], acc[r][n]);
                    }
                }
            }
        }
    } else {
        const int nb = K >> 5;
        for (int b = lane; b < nb; b += 64) {
            int4 alo[NT], ahi[NT];
            float dx[NT], sx[NT];
            int qs[NT];
#pragma unroll
            for (int n = 0; n < NT; n++) {
                if (t0 + n < T) {
                    const int4 * ap = (const int4 *)(E.in.q + (size_t)(t0 + n) * K + (size_t)b * 32);
                    alo[n] = ap[0];
                    ahi[n] = ap[1];
                    const size_t bi = (size_t)(t0 + n) * nb + b;
                    dx[n] = E.in.d[bi];
                    qs[n] = E.in.qsum[bi];
                    sx[n] = (WF == W_Q4_1 || WF == W_Q5_1) ? E.in.s[bi] : 0.0f;
                } else {
                    alo[n] = make_int4(0, 0, 0, 0);
                    ahi[n] = alo[n];
                    dx[n] = 0.0f;
                    qs[n] = 0;
                    sx[n] = 0.0f;
                }
            }
#pragma unroll
            for (int r = 0; r < RPW; r++) {
                const int row = row0 + r;
                if (row < M) {
#pragma unroll
                    for (int n = 0; n < NT; n++) {
                        float dw, mw;
                        const int sumi = block_dot<WF>(W, row, b, nb, alo[n], ahi[n], qs[n], dw, mw);
                        acc[r][n] = fmaf(dw * dx[n], (float)sumi, acc[r][n]);
                        if constexpr (WF == W_Q4_1 || WF == W_Q5_1) acc2[r][n] = fmaf(mw, sx[n], acc2[r][n]);  // exact product
                    }
                }
            }
        }
    }
}

template <int WF, int RPW, int NT>
__global__ __launch_bounds__(256) void k_mm(MMGroup g) {
    constexpr int RW = 4 * RPW;  // rows per workgroup
    __shared__ float red[NT][RW];
    __shared__ float red2[NT][RW];
    int e = 0;
#pragma unroll 1
    while (e + 1 < g.n && (int)blockIdx.x >= g.e[e + 1].block0) e++;
    const MMEntry & E = g.e[e];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rowwg = ((int)blockIdx.x - E.block0) * RW;
    const int row0 = rowwg + wave * RPW;
    const int T = g.T;
    // grid.y splits the tokens into spans (a multiple of NT each): every output keeps its own
    // arithmetic, the small-M groups (LoRA first stages, 18 row blocks) just get more workgroups
    const int span = ((T + (int)gridDim.y - 1) / (int)gridDim.y + NT - 1) / NT * NT;
    const int tb = (int)blockIdx.y * span, te = min(T, tb + span);
    for (int t0 = tb; t0 < te; t0 += NT) {
        float acc[RPW][NT], acc2[RPW][NT];
#pragma unroll
        for (int r = 0; r < RPW; r++)
#pragma unroll
            for (int n = 0; n < NT; n++) acc[r][n] = acc2[r][n] = 0.0f;
        mm_accumulate<WF, RPW, NT>(E, row0, t0, T, lane, acc, acc2);
#pragma unroll
        for (int r = 0; r < RPW; r++)
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const float s = wave_sum63(acc[r][n]);
                float s2 = 0.0f;
                if constexpr (WF == W_Q4_1 || WF == W_Q5_1) s2 = wave_sum63(acc2[r][n]);
                if (lane == 63) {
                    red[n][wave * RPW + r] = s;
                    red2[n][wave * RPW + r] = s2;
                }
            }
        __syncthreads();
        const int tid = threadIdx.x;
        if (tid < RW * NT) {
            const int n = tid / RW, r = tid % RW;
            const int t = t0 + n, row = rowwg + r;
            // (t < T) is uniform across each 32-lane half-wave since RW is a multiple of 32
            // whenever emission is used (RPW == 8).
            if (t < T) {
                const float acc_v = red[n][r] + red2[n][r];
                float v = 0.0f;
                if (row < E.W.M) {
                    v = apply_epi(E, t, row, acc_v);
                    if (E.y) E.y[(size_t)t * E.ldy + row] = v;
                }
                if (E.emit) emit32(E.out, t, row, v);
            }
        }
        __syncthreads();
    }
}

template <int WF>
static bool launch_mm_wf(hipStream_t st, MMGroup & g) {
    bool emit = false;
    for (int i = 0; i < g.n; i++) emit |= g.e[i].emit != 0;
    const int T = g.T;
    // Emission needs 32 rows per workgroup (one quantization block per half-wave).
    const int rpw = emit ? 8 : 2;
    const int rw = 4 * rpw;
    int blocks = 0;
    for (int i = 0; i < g.n; i++) {
        if (g.e[i].emit && (g.e[i].W.M % 32 != 0)) {
            fprintf(stderr, "rwkv: emitting matmul needs M %% 32 == 0 (M=%d)\n", g.e[i].W.M);
            return false;
        }
        if (g.e[i].W.K % 32 != 0) {
            fprintf(stderr, "rwkv: matmul needs K %% 32 == 0 (K=%d)\n", g.e[i].W.K);
            return false;
        }
        g.e[i].block0 = blocks;
        blocks += (g.e[i].W.M + rw - 1) / rw;
    }
    if (blocks == 0) return true;
    dim3 grid(blocks), block(256);
    if (T == 1) {
        if (emit) RK_LAUNCH((k_mm<WF, 8, 1>), grid, block, 0, st, g);
        else RK_LAUNCH((k_mm<WF, 2, 1>), grid, block, 0, st, g);
    } else {
        // token spans so that the grid has ~4096 workgroups (at most one span per 4 tokens)
        // (batched decode, T <= 16 over >= 256 row blocks: one span, every weight read once)
        const int gy = (T <= 16 && blocks >= 256) ? 1 : std::max(1, std::min((T + 3) / 4, 4096 / blocks));
        const dim3 grid2(blocks, gy);
        if (emit) RK_LAUNCH((k_mm<WF, 8, 4>), grid2, block, 0, st, g);
        else RK_LAUNCH((k_mm<WF, 2, 4>), grid2, block, 0, st, g);
    }
    HIP_OK(hipGetLastError());
    return true;
}

// --------------------------------------------------------------------------- small-K matmul
// F16 / F32 weights whose rows fit one unit per lane of k_mm (K <= 512 halves / 256 floats: the v7
// LoRA second stages, K = 64..480), T >= 2.  k_mm gives each output a whole wave, most of whose
// lanes hold no unit (K = 96: 12 of 64) and then a 6-step DPP reduction.  Here one THREAD computes
// one output: the lane partials p[l] = dot over unit l (k_mm's per-lane arithmetic, from 0) and
// wave_sum63's perfect binary tree over them.  Lanes without a unit contribute +0, and a partial
// is never -0 (every chain starts from +0), so the zero leaves change no bit and the tree is
// folded only over the NL leading leaves (NL = the next power of two): results equal k_mm's.
// Workgroup = 64 rows (one per lane) x MMS_TB tokens (waves take every 4th token); the rows'
// weights and the tokens' activations are staged in LDS.
constexpr int MMS_TB = 16;

template <int WF>
__device__ __forceinline__ float small_leaf(const char * wrow, const char * xrow, int l, int nl) {
    float p = 0.0f;
    if (l < nl) {
        const int4 w = *(const int4 *)(wrow + 16 * l), x = *(const int4 *)(xrow + 16 * l);
        if constexpr (WF == W_F16) {
            p = dot8_f16(w, x, 0.0f);
        } else {
            p = fmaf(__int_as_float(w.x), __int_as_float(x.x), p);
            p = fmaf(__int_as_float(w.y), __int_as_float(x.y), p);
            p = fmaf(__int_as_float(w.z), __int_as_float(x.z), p);
            p = fmaf(__int_as_float(w.w), __int_as_float(x.w), p);
        }
    }
    return p;
}

// Leaves in groups of 8 (a perfect 8-leaf tree each), the groups folded as they are produced (a
// binary counter: lv[k] holds the pending left subtree of 8 * 2^k leaves) -- the same perfect
// binary tree over NL leaves with few live registers.
template <int WF, int NL>
__device__ __forceinline__ float small_row_dot(const char * wrow, const char * xrow, int nl) {
    float lv[3];
    float v = 0.0f;
#pragma unroll 1
    for (int g = 0; g < NL / 8; g++) {
        float p[8];
#pragma unroll
        for (int l = 0; l < 8; l++) p[l] = small_leaf<WF>(wrow, xrow, 8 * g + l, nl);
        v = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
#pragma unroll
        for (int k = 0; (8 << k) < NL; k++) {
            if (g & (1 << k)) {
                v = lv[k] + v;
            } else {
                lv[k] = v;
                break;
            }
        }
    }
    return v;  // the last group closed every level: the root
}

template <int WF>
__global__ __launch_bounds__(256) void k_mm_small(MMGroup g, int wstride) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    int e = 0;
#pragma unroll 1
    while (e + 1 < g.n && (int)blockIdx.x >= g.e[e + 1].block0) e++;
    const MMEntry & E = g.e[e];
    const int M = E.W.M, K = E.W.K, T = g.T;
    constexpr int ES = WF == W_F16 ? 2 : 4;       // element bytes
    const int rowb = K * ES, nl = rowb / 16;       // bytes per row, units (lanes of k_mm)
    const int row0 = ((int)blockIdx.x - E.block0) * 64, t0 = (int)blockIdx.y * MMS_TB;
    char * ws = sm;                                // [64][wstride]
    char * xs = sm + 64 * wstride;                 // [MMS_TB][rowb]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const char * wg = (const char *)E.W.qs;
    const char * xg = (const char *)(WF == W_F16 ? (const void *)E.in.h : (const void *)E.in.f);
    // (row, unit) of flat index i: i / nl through a float reciprocal (exact: i < 2^12, nl <= 64)
    const float rnl = 1.0f / (float)nl;
    for (int i = tid; i < 64 * nl; i += 256) {
        const int r = (int)(((float)i + 0.5f) * rnl), u = i - r * nl;
        const int row = min(row0 + r, M - 1);
        *(int4 *)(ws + r * wstride + 16 * u) = *(const int4 *)(wg + (size_t)row * rowb + 16 * u);
    }
    for (int i = tid; i < MMS_TB * nl; i += 256) {
        const int t = (int)(((float)i + 0.5f) * rnl), u = i - t * nl;
        const int tt = min(t0 + t, T - 1);
        *(int4 *)(xs + t * rowb + 16 * u) = *(const int4 *)(xg + (size_t)tt * rowb + 16 * u);
    }
    __syncthreads();
    const int row = row0 + lane;
    const char * wrow = ws + lane * wstride;
    for (int tl = wave; tl < MMS_TB; tl += 4) {
        const int t = t0 + tl;
        if (t >= T) break;  // wave-uniform
        const char * xrow = xs + tl * rowb;
        float s;
        if (nl <= 8) s = small_row_dot<WF, 8>(wrow, xrow, nl);
        else if (nl <= 16) s = small_row_dot<WF, 16>(wrow, xrow, nl);
        else if (nl <= 32) s = small_row_dot<WF, 32>(wrow, xrow, nl);
        else s = small_row_dot<WF, 64>(wrow, xrow, nl);
        // k_mm: red + red2 (red2 = 0 for float weights)
        const float acc = s + 0.0f;
        float v = 0.0f;
        if (row < M) {
            v = apply_epi(E, t, row, acc);
            if (E.y) E.y[(size_t)t * E.ldy + row] = v;
        }
        // a half-wave = 32 consecutive rows of token t (M % 32 == 0 when emitting)
        if (E.emit && row0 + (lane & 32) < M) emit32(E.out, t, row, v);
    }
}

// true (and launched) when every entry is an F16 / F32 matrix with one unit per k_mm lane
static bool launch_mm_small(hipStream_t st, MMGroup & g, int wtype) {
    if (g.T < 2 || (wtype != W_F16 && wtype != W_F32)) return false;
    const int ES = wtype == W_F16 ? 2 : 4;
    int blocks = 0, kmax = 0;
    for (int i = 0; i < g.n; i++) {
        const MMEntry & e = g.e[i];
        if (e.W.type != wtype || e.W.K * ES > 1024 || (e.W.K * ES) % 16 || e.in.fmt != act_fmt_for(wtype) ||
            (e.emit && e.W.M % 32))
            return false;
        kmax = std::max(kmax, e.W.K);
    }
    for (int i = 0; i < g.n; i++) {
        g.e[i].block0 = blocks;
        blocks += (g.e[i].W.M + 63) / 64;
    }
    const int wstride = kmax * ES + 16;  // padded row: 16-byte reads of 16 lanes spread over banks
    const size_t lds = (size_t)64 * wstride + (size_t)MMS_TB * kmax * ES;
    const dim3 grid(blocks, (g.T + MMS_TB - 1) / MMS_TB);
    if (wtype == W_F16) RK_LAUNCH(k_mm_small<W_F16>, grid, dim3(256), lds, st, g, wstride);
    else RK_LAUNCH(k_mm_small<W_F32>, grid, dim3(256), lds, st, g, wstride);
    return hipGetLastError() == hipSuccess;
}

bool launch_mm_group(hipStream_t st, MMGroup & g, int wtype) {
    bool fmm = false;
    if (!launch_fmm_group(st, g, wtype, &fmm)) return false;
    if (fmm) return true;
    if (launch_mm_small(st, g, wtype)) return true;
    switch (wtype) {
        case W_F32: return launch_mm_wf<W_F32>(st, g);
        case W_F16: return launch_mm_wf<W_F16>(st, g);
        case W_Q4_0: return launch_mm_wf<W_Q4_0>(st, g);
        case W_Q4_1: return launch_mm_wf<W_Q4_1>(st, g);
        case W_Q5_0: return launch_mm_wf<W_Q5_0>(st, g);
        case W_Q5_1: return launch_mm_wf<W_Q5_1>(st, g);
        case W_Q8_0: return launch_mm_wf<W_Q8_0>(st, g);
        default:
            fprintf(stderr, "rwkv: unsupported weight type %d\n", wtype);
            return false;
    }
}

// --------------------------------------------------------------------------- timing helper
__global__ void k_delay(unsigned long long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(10);
}

bool launch_delay(hipStream_t st, int us) {
    RK_LAUNCH(k_delay, dim3(1), dim3(64), 0, st, (unsigned long long)us * 100ull);  // 100 MHz clock
    HIP_OK(hipGetLastError());
    return true;
}

// --------------------------------------------------------------------------- LayerNorm family

// One token row per workgroup.  Every wave loads the embedding row straight into registers in the
// LayerNorm chunk layout (lane l: elements 512 c + 8 l .. + 7) and computes the statistics itself
// (ln_stats_regs: ln_stats_wave's association, the same bits as the sequence kernels); wave w then
// normalizes and stores chunks w, w + 4, ...  The LayerNorm weights are loaded at kernel start, before
// the token id returns: two dependent memory round trips (token, row) instead of a store / reload of
// the row through L2 between them -- one, the row's, when the id comes with the launch (TokArg::imm).
constexpr int EMB_NC = 8;  // chunks held per lane: n_embed <= 4096
// the one parameter of both kernels (Engine::capture_tok updates tokens in a captured node)
struct EmbedLn {
    TokArg tokens;
    DMat emb;
    const float * w, * b;
    float * x;
};
__global__ __launch_bounds__(256) void k_embed_ln(EmbedLn a) {
    const TokArg & tokens = a.tokens;
    const DMat & emb = a.emb;
    const float * w = a.w, * b = a.b;
    float * x = a.x;
    STAMP_BEGIN();
    const int t = blockIdx.x, C = emb.K, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nc = (C + LN_CHUNK - 1) / LN_CHUNK;
    float wv[2][8], bv[2][8];  // this wave's chunks w and w + 4
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int c = wave + 4 * q;
        if (c < nc) {
            ln_load8(wv[q], w, c * LN_CHUNK + lane * 8, C);
            ln_load8(bv[q], b, c * LN_CHUNK + lane * 8, C);
        }
    }
    const size_t tok = tok_get(tokens, t);
    if (threadIdx.x == 0) tok_keep(tokens);
    float v[EMB_NC][8];
#pragma unroll
    for (int c = 0; c < EMB_NC; c++) {
        if (c >= nc) break;
        const int k = min(c * LN_CHUNK + lane * 8, C - 8);
        if (emb.type == W_F16) {
            const __half * p = (const __half *)emb.qs + tok * C + k;
            const int4 raw = *(const int4 *)p;
            const __half * h = (const __half *)&raw;
#pragma unroll
            for (int j = 0; j < 8; j++) v[c][j] = __half2float(h[j]);
        } else {
            ln_load8(v[c], (const float *)emb.qs + tok * C, k, C);
        }
    }
    float mean, scale;
    ln_stats_regs<EMB_NC>(v, nc, C, 1e-5f, mean, scale);
    float * xr = x + (size_t)t * C;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int c = wave + 4 * q;
        if (c >= nc) continue;
        const int k = c * LN_CHUNK + lane * 8;
        if (k >= C) continue;
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = ln_apply(v[c][j], mean, scale, wv[q][j], bv[q][j]);
        *(float4 *)(xr + k) = make_float4(o[0], o[1], o[2], o[3]);
        *(float4 *)(xr + k + 4) = make_float4(o[4], o[5], o[6], o[7]);
    }
    STAMP_END(5);
}

// Rows wider than EMB_NC chunks (n_embed > 4096, e.g. RWKV-4 14B at 5120): the same statistics
// association (ln_stats_wave's chunk order, 4 chunks in flight) with the row re-read from HBM per
// group of chunks, every wave on its own (no exchange), then wave w normalizes chunks w, w + 4, ...
__device__ __forceinline__ void emb_load8(float (&v)[8], const DMat & emb, size_t tok, int k) {
    const int C = emb.K;
    if (emb.type == W_F16) {
        const int4 raw = *(const int4 *)((const __half *)emb.qs + tok * C + min(k, C - 8));
        const __half * h = (const __half *)&raw;
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = __half2float(h[j]);
    } else {
        ln_load8(v, (const float *)emb.qs + tok * C, k, C);
    }
}
__global__ __launch_bounds__(256) void k_embed_ln_wide(EmbedLn a) {
    const TokArg & tokens = a.tokens;
    const DMat & emb = a.emb;
    const float * w = a.w, * b = a.b;
    float * x = a.x;
    const int t = blockIdx.x, C = emb.K, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nc = (C + LN_CHUNK - 1) / LN_CHUNK;
    const size_t tok = tok_get(tokens, t);
    if (threadIdx.x == 0) tok_keep(tokens);
    double s1 = 0.0, s2 = 0.0;
    for (int c0 = 0; c0 < nc; c0 += 4) {
        float v[4][8];
#pragma unroll
        for (int c = 0; c < 4; c++) emb_load8(v[c], emb, tok, min(c0 + c, nc - 1) * LN_CHUNK + lane * 8);
        double c1[4], c2[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            c1[c] = c2[c] = 0.0;
            if (c0 + c < nc) ln_chunk_sums(v[c], (c0 + c) * LN_CHUNK + lane * 8 < C, c1[c], c2[c]);
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (c0 + c < nc) s1 += c1[c], s2 += c2[c];
    }
    float mean, scale;
    ln_finish(s1, s2, C, 1e-5f, mean, scale);
    float * xr = x + (size_t)t * C;
    for (int c = wave; c < nc; c += 4) {
        const int k = c * LN_CHUNK + lane * 8;
        if (k >= C) continue;
        float v[8], wv[8], bv[8], o[8];
        emb_load8(v, emb, tok, k);
        ln_load8(wv, w, k, C);
        ln_load8(bv, b, k, C);
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = ln_apply(v[j], mean, scale, wv[j], bv[j]);
        *(float4 *)(xr + k) = make_float4(o[0], o[1], o[2], o[3]);
        *(float4 *)(xr + k + 4) = make_float4(o[4], o[5], o[6], o[7]);
    }
}

bool launch_embed_ln(hipStream_t st, const TokArg & tokens, int T, const DMat & emb, const float * w,
                     const float * b, float * x) {
    if (emb.K % 8 || (emb.type != W_F16 && emb.type != W_F32)) {
        fprintf(stderr, "rwkv: embedding row of %d elements (type %d) unsupported\n", emb.K, emb.type);
        return false;
    }
    if (tokens.imm && T != 1) {
        fprintf(stderr, "rwkv: a token id passed by value with %d tokens\n", T);
        return false;
    }
    const EmbedLn a{tokens, emb, w, b, x};
    tok_launch_note(a, offsetof(EmbedLn, tokens));
    if (emb.K > EMB_NC * LN_CHUNK) RK_LAUNCH(k_embed_ln_wide, dim3(T), dim3(256), 0, st, a);
    else RK_LAUNCH(k_embed_ln, dim3(T), dim3(256), 0, st, a);
    HIP_OK(hipGetLastError());
    return true;
}

// Token-row kernels that emit Q8 activations into sequence-GEMM token tiles run TOKS_PER_WG
// consecutive tokens per workgroup (one 256-thread group each): a tile record's 64-byte sectors
// hold 16-byte pieces of 4 consecutive tokens, so the four partial writes of a sector meet in one
// XCD's L2 instead of leaving four L2s as four partial-line write-backs.
constexpr int TOKS_PER_WG = 4;

// emit32 for an output known at compile time to be Q8 sequence-GEMM token tiles (TQ 1: Q8_0,
// 2: Q8_1) of row length K: store32's tiled values, no runtime format dispatch
template <int TQ>
__device__ __forceinline__ void emit32_tile(uint8_t * tq, int K, int t, int k, float v) {
    const Q32 r = quant32(v);
    uint8_t * rec = tq + ((size_t)(t / QG_TOK) * (K >> 5) + (k >> 5)) * qg_a_bytes(TQ == 2);
    const int tl = t % QG_TOK;
    rec[((k >> 4) & 1) * QG_TOK * 16 + tl * 16 + (k & 15)] = (uint8_t)(int8_t)r.q;
    if ((k & 31) == 0) {
        ((float *)(rec + QG_A_D))[tl] = f16_round(r.d);
        if constexpr (TQ == 2) ((float *)(rec + QG_A_S))[tl] = f16_round(r.d * (float)r.sum);
    }
}

// TQ of a set of outputs: 1 / 2 when all are Q8_0 / Q8_1 token tiles of row length K, else 0
static int tile_q(const ActBuf * outs, int n, int K) {
    if (n < 1) return 0;
    for (int i = 0; i < n; i++)
        if (!outs[i].tiled || outs[i].fmt != outs[0].fmt || outs[i].K != K ||
            (outs[i].fmt != A_Q8_0 && outs[i].fmt != A_Q8_1))
            return 0;
    return outs[0].fmt == A_Q8_1 ? 2 : 1;
}

// rwkv_carry_x (rwkv_graph.inc:56-82) + the token-shift mixes of each version.
// SEG (batched prefill): the T tokens are a packed chunk cut into segments (SegTab); a segment's first
// token is shifted against the segment's input carry, its last token writes the output carry.  The
// statistics and the per-token arithmetic are the unsegmented form's.
template <int TQ, bool SEG>
__device__ __forceinline__ void ln_mix_body(const LnMixArgs & a, const SegTab & sg) {
    // LayerNorm statistics of the workgroup's TOKS_PER_WG + 1 rows (its tokens and the one before),
    // one wave per row (the canonical one-wave association), shared through LDS
    __shared__ float s_mean[TOKS_PER_WG + 1], s_scale[TOKS_PER_WG + 1];
    const int tg = threadIdx.x >> 8, t = blockIdx.x * TOKS_PER_WG + tg, C = a.C, tid = threadIdx.x & 255;
    const int wave = threadIdx.x >> 6;
    if (wave <= TOKS_PER_WG) {
        const int rt = (int)blockIdx.x * TOKS_PER_WG - 1 + wave;
        if (rt >= 0 && rt < a.T) {
            float m, sc;
            ln_stats_any(a.x + (size_t)rt * C, C, 1e-5f, m, sc);
            if ((threadIdx.x & 63) == 0) {
                s_mean[wave] = m;
                s_scale[wave] = sc;
            }
        }
    }
    __syncthreads();
    if (t >= a.T) return;  // whole 256-thread token groups
    const float * xt = a.x + (size_t)t * C;
    const float mean = s_mean[tg + 1], scale = s_scale[tg + 1];
    // the token opens a sequence (its shift partner is a carry) / closes one (it writes the carry)
    bool first = t == 0, last = t == a.T - 1;
    const float * cin = a.carry_in;
    float * cout = a.carry_out;
    if constexpr (SEG) {
        const uint32_t s = sg.seg_of[t], b = sg.begin[s];
        first = (uint32_t)t == b;
        last = (uint32_t)t == b + sg.len[s] - 1;
        cin += sg.sin_off[s];
        if (cout) cout += sg.sout_off[s];
    }
    const float pmean = !first ? s_mean[tg] : 0.0f, pscale = !first ? s_scale[tg] : 0.0f;
    // channel blocks of 256 split over grid.y (short sequences / batched decode: more workgroups);
    // LNM_CB blocks at a time: all their loads are issued before the first store
    constexpr int LNM_CB = TQ > 0 ? 4 : 2;  // (4 spills in the runtime-format emit)
    const int cstride = (int)gridDim.y * 256;
    const int nmu = min(a.n_out, 6);
    for (int cb0 = (int)blockIdx.y * 256; cb0 < C; cb0 += LNM_CB * cstride) {
        float xv[LNM_CB], pv[LNM_CB], wv[LNM_CB], bv[LNM_CB], muv[LNM_CB][6];
#pragma unroll
        for (int j = 0; j < LNM_CB; j++) {
            const int c = min(cb0 + j * cstride + tid, C - 1);
            xv[j] = xt[c];
            wv[j] = a.lnw[c];
            bv[j] = a.lnb[c];
            // batch (a.bs > 0): every token is its own context, shifted against its own carry
            if constexpr (SEG) pv[j] = first ? cin[c] : xt[c - C];
            else pv[j] = a.bs ? a.carry_in[(size_t)t * a.bs + c] : (t > 0) ? xt[c - C] : a.carry_in[c];
#pragma unroll
            for (int n = 0; n < 6; n++) muv[j][n] = n < nmu ? a.mu[n][c] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < LNM_CB; j++) {
            const int c0 = cb0 + j * cstride, c = c0 + tid;
            if (c0 + (tid & ~63) >= C) continue;  // whole wave out of range (C % 64 == 0)
            const float xa = ln_apply(xv[j], mean, scale, wv[j], bv[j]);
            const float xp = ((!SEG && a.bs) || first) ? pv[j] : ln_apply(pv[j], pmean, pscale, wv[j], bv[j]);
            if constexpr (SEG) {
                if (last && cout) cout[c] = xa;
            } else {
                if (a.bs && a.carry_out) a.carry_out[(size_t)t * a.bs + c] = xa;
                else if (last && a.carry_out) a.carry_out[c] = xa;
            }
            if (a.out_xa) a.out_xa[(size_t)t * C + c] = xa;
            if (a.out_sx) a.out_sx[(size_t)t * C + c] = xp - xa;
#pragma unroll
            for (int n = 0; n < 6; n++) {
                if (n >= nmu) break;
                const float mu = muv[j][n];
                float v;
                if (a.form == 0) {
                    v = xa * mu + (xp - xp * mu);
                } else {
                    v = (xp - xa) * mu + xa;
                }
                if constexpr (TQ > 0) emit32_tile<TQ>(a.out[n].tq, C, t, c, v);
                else emit32(a.out[n], t, c, v);
            }
        }
    }
}

template <int TQ>
__global__ __launch_bounds__(1024) void k_ln_mix(LnMixArgs a) {
    ln_mix_body<TQ, false>(a, SegTab{});
}

template <int TQ>
__global__ __launch_bounds__(1024) void k_ln_mix_seg(LnMixArgs a, SegTab sg) {
    ln_mix_body<TQ, true>(a, sg);
}

bool launch_ln_mix(hipStream_t st, const LnMixArgs & a, const SegTab * seg) {
    // long sequences: one channel block row (grid.y = 1; each workgroup computes its rows' LayerNorm
    // statistics itself, so splitting the channels repeats that work: y = 2 / 4 / 8 measured slower)
    // fewer token groups than ~2 per CU (short sequences, batched decode): the channel blocks over
    // grid.y until the grid holds about 512 workgroups
    const int tgs = (a.T + TOKS_PER_WG - 1) / TOKS_PER_WG, cbs = (a.C + 255) / 256;
    const int gy = a.T <= 64 ? cbs : tgs < 256 ? std::min(cbs, (512 + tgs - 1) / tgs) : 1;
    const dim3 grid((a.T + TOKS_PER_WG - 1) / TOKS_PER_WG, gy), block(256 * TOKS_PER_WG);
    const int tq = tile_q(a.out, a.n_out, a.C);
    if (seg) {
        if (a.bs) return false;  // segments or contexts, not both
        if (tq == 1) RK_LAUNCH(k_ln_mix_seg<1>, grid, block, 0, st, a, *seg);
        else if (tq == 2) RK_LAUNCH(k_ln_mix_seg<2>, grid, block, 0, st, a, *seg);
        else RK_LAUNCH(k_ln_mix_seg<0>, grid, block, 0, st, a, *seg);
        HIP_OK(hipGetLastError());
        return true;
    }
    if (tq == 1) RK_LAUNCH(k_ln_mix<1>, grid, block, 0, st, a);
    else if (tq == 2) RK_LAUNCH(k_ln_mix<2>, grid, block, 0, st, a);
    else RK_LAUNCH(k_ln_mix<0>, grid, block, 0, st, a);
    HIP_OK(hipGetLastError());
    return true;
}

__global__ __launch_bounds__(256) void k_ln_emit(int C, const float * x, const float * w, const float * b, ActBuf out) {
    __shared__ double sh[8];
    const int t = blockIdx.x;  // row t of x -> row t of out
    x += (size_t)t * C;
    float mean, scale;
    ln_stats(x, C, 1e-5f, mean, scale, sh);
    for (int c0 = 0; c0 < C; c0 += blockDim.x) {
        const int c = c0 + threadIdx.x;
        if (c0 + (int)(threadIdx.x & ~63) >= C) continue;
        emit32(out, t, c, ln_apply(x[c], mean, scale, w[c], b[c]));
    }
}

bool launch_ln_emit(hipStream_t st, int C, const float * x, const float * w, const float * b, const ActBuf & out,
                    int rows) {
    RK_LAUNCH(k_ln_emit, dim3(rows), dim3(256), 0, st, C, x, w, b, out);
    HIP_OK(hipGetLastError());
    return true;
}

// --------------------------------------------------------------------------- v6 mix5
struct Mix5Args {
    int T, C, D;
    const float * lora;
    const float * w2;
    const float * maa[5];
    const float * xa;
    const float * sx;
    ActBuf out[5];
};

// Workgroup = 64 channels x 5 mixes x MIX_TT tokens (32: the per-wave setup over more tokens, 78 -> 76 us
// per v6-1B6 layer), wave n = mixed vector n (w, k, v, r, g):
// each lane holds its channel's W2 column of that mix in registers (D floats, read once per token
// tile); the tile's lora rows sit in LDS as [mix][i][token], so one 16-byte broadcast read gives
// the i-th lora value of 4 tokens.  Per token the D-long fp32 fma chain runs in k_v6_mix5_dec's
// order (sequential over i); 4 tokens' chains run side by side (168 VGPRs: 3 waves per SIMD).
constexpr int MIX_TT = 32;  // (64: 76.8 us)

// TQ > 0: all five outputs are Q8 sequence-GEMM token tiles (TQ = 2: Q8_1); each lane's record
// address is formed once (a workgroup's MIX_TT tokens lie in one QG_TOK-token tile) and the
// per-output emission is quant32 + store (store32's tiled values), no runtime format dispatch.
template <int DM, int TQ, bool EXACT>
__global__ __launch_bounds__(320) void k_v6_mix5(Mix5Args a) {
    static_assert(QG_TOK % MIX_TT == 0 && MIX_TT % 4 == 0, "mix5 token tile");
    __shared__ __attribute__((aligned(16))) float sl[5][DM][MIX_TT];
    const int C = a.C, D = EXACT ? DM : a.D, T = a.T;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = __builtin_amdgcn_readfirstlane(tid >> 6);
    // this wave's mix: operands selected with compile-time indices (no dynamic kernarg indexing)
    const float * maa_n = a.maa[0];
    ActBuf out_n = a.out[0];
#pragma unroll
    for (int m = 1; m < 5; m++)
        if (n == m) {
            maa_n = a.maa[m];
            out_n = a.out[m];
        }
    const int c = blockIdx.x * 64 + lane;
    const bool cval = (int)(blockIdx.x * 64 + (lane & ~31)) < C;  // half-wave uniform
    const int cc = min(c, C - 1);
    const int t0 = blockIdx.y * MIX_TT, nt = min(MIX_TT, T - t0);
    for (int e = tid; e < 5 * DM * MIX_TT; e += 320) {
        const int tt = e / (5 * DM), f = e % (5 * DM), m = f / DM, i = f % DM;  // coalesced reads
        sl[m][i][tt] = (tt < nt && i < D) ? a.lora[(size_t)(t0 + tt) * 5 * D + m * D + i] : 0.0f;
    }
    float w2v[DM];
    const float mu = maa_n[cc];
#pragma unroll
    for (int i = 0; i < DM; i++) {
        const float t = a.w2[((size_t)n * D + min(i, D - 1)) * C + cc];  // transposed [5][D][C]
        w2v[i] = i < D ? t : 0.0f;
    }
    uint8_t * rec = nullptr;
    int qoff = 0;
    if constexpr (TQ > 0) {
        // record of (token tile t0 / QG_TOK, block c / 32); byte of element c in half (c >> 4) & 1
        const size_t ri = (size_t)(t0 / QG_TOK) * (C >> 5) + (cc >> 5);
        rec = out_n.tq + ri * qg_a_bytes(TQ == 2);
        qoff = ((cc >> 4) & 1) * QG_TOK * 16 + (cc & 15);
    }
    __syncthreads();
    for (int tt = 0; tt < nt; tt += 4) {
        float xa[4], sx[4], acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const size_t ti = (size_t)(t0 + min(tt + j, nt - 1)) * C + cc;
            xa[j] = a.xa[ti];
            sx[j] = a.sx[ti];
        }
#pragma unroll
        for (int i = 0; i < DM; i++) {
            if (EXACT || i < D) {
                const float4 l = *(const float4 *)&sl[n][i][tt];
                acc[0] = fmaf(w2v[i], l.x, acc[0]);
                acc[1] = fmaf(w2v[i], l.y, acc[1]);
                acc[2] = fmaf(w2v[i], l.z, acc[2]);
                acc[3] = fmaf(w2v[i], l.w, acc[3]);
            }
        }
        if (!cval) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (tt + j >= nt) break;
            const float v = (acc[j] + mu) * sx[j] + xa[j];
            if constexpr (TQ > 0) {
                const Q32 q = quant32(v);
                const int tl = (t0 + tt + j) % QG_TOK;
                rec[qoff + tl * 16] = (uint8_t)(int8_t)q.q;
                if ((c & 31) == 0) {
                    ((float *)(rec + QG_A_D))[tl] = f16_round(q.d);
                    if constexpr (TQ == 2) ((float *)(rec + QG_A_S))[tl] = f16_round(q.d * (float)q.sum);
                }
            } else {
                emit32(out_n, t0 + tt + j, c, v);
            }
        }
    }
}

// The same mixes on the f32 MFMA (round 3): m[t][c] = the fmaf chain over i of W2[c][i] * lora[t][i]
// in order from 0 is exactly a chain of v_mfma_f32_16x16x4_f32 over i in quads (C first, k = 0..3
// in order: tools/mfma_f32_probe.hip), so the mixes stay bit-identical to k_v6_mix5 and the decode's
// k_v6_mix5_dec.  Workgroup = 5 waves, wave n = mix n over 32 channels x 64 tokens (2 x 4 tiles of
// 16 x 16; operands straight from L2); the epilogue quantizes each token's 32 channels -- one Q8
// block, held by lanes tok + 16 g of the D layout -- with xor-16/32 lane exchanges (order-free max
// and integer sum, quant32's values) and stores them into the token-tile records (TQ = 1: Q8_0,
// 2: Q8_1).
typedef float mixf4 __attribute__((ext_vector_type(4)));
template <int DM, int TQ>
__global__ __launch_bounds__(320) void k_v6_mix5m(Mix5Args a) {
    const int C = a.C, T = a.T;
    const int lane = threadIdx.x & 63, n = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ml = lane & 15, g = lane >> 4;
    const float * maa_n = a.maa[0];
    ActBuf out_n = a.out[0];
#pragma unroll
    for (int m = 1; m < 5; m++)
        if (n == m) {
            maa_n = a.maa[m];
            out_n = a.out[m];
        }
    const int c0 = blockIdx.x * 32, t0 = blockIdx.y * 64;
    // A operands: W2 (transposed [5][D][C]) of channels c0 + 16 ct + ml, i = 4 j + g
    float wa[2][DM / 4];
#pragma unroll
    for (int ct = 0; ct < 2; ct++)
#pragma unroll
        for (int j = 0; j < DM / 4; j++) wa[ct][j] = a.w2[((size_t)n * DM + 4 * j + g) * C + c0 + 16 * ct + ml];
    mixf4 acc[2][4];
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
        // B operands: lora[t][n][i] of token t0 + 16 nt + ml, i = 4 j + g
        const size_t tr = (size_t)min(t0 + 16 * nt + ml, T - 1) * 5 * DM + (size_t)n * DM + g;
        float lb[DM / 4];
#pragma unroll
        for (int j = 0; j < DM / 4; j++) lb[j] = a.lora[tr + 4 * j];
#pragma unroll
        for (int ct = 0; ct < 2; ct++) {
            mixf4 c = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < DM / 4; j++) c = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[ct][j], lb[j], c, 0, 0, 0);
            acc[ct][nt] = c;
        }
    }
    // epilogue: lane holds channels c0 + 16 ct + 4 g + i of token t0 + 16 nt + ml
    const int cb = c0 + 4 * g;
    mixf4 mu[2];
#pragma unroll
    for (int ct = 0; ct < 2; ct++) mu[ct] = *(const mixf4 *)(maa_n + cb + 16 * ct);
    uint8_t * rec = out_n.tq + ((size_t)(t0 / QG_TOK) * (C >> 5) + (c0 >> 5)) * qg_a_bytes(TQ == 2);
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
        const int t = t0 + 16 * nt + ml;
        const size_t ti = (size_t)min(t, T - 1) * C + cb;
        float v[2][4];
        float am = 0.0f;
#pragma unroll
        for (int ct = 0; ct < 2; ct++) {
            const mixf4 xa = *(const mixf4 *)(a.xa + ti + 16 * ct), sx = *(const mixf4 *)(a.sx + ti + 16 * ct);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                v[ct][i] = (acc[ct][nt][i] + mu[ct][i]) * sx[i] + xa[i];
                am = fmaxf(am, fabsf(v[ct][i]));
            }
        }
        am = fmaxf(am, __shfl_xor(am, 16));
        am = fmaxf(am, __shfl_xor(am, 32));
        const float id = (am != 0.0f) ? 127.f / am : 0.0f;
        const float d = am / 127.f;
        uint32_t packed[2];
        int sum = 0;
#pragma unroll
        for (int ct = 0; ct < 2; ct++) {
            packed[ct] = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int q = (int)rintf(v[ct][i] * id);
                sum += q;
                packed[ct] |= ((uint32_t)q & 0xffu) << (8 * i);
            }
        }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        if (t < T) {
            const int tl = t % QG_TOK;
#pragma unroll
            for (int ct = 0; ct < 2; ct++) *(uint32_t *)(rec + ct * QG_TOK * 16 + tl * 16 + 4 * g) = packed[ct];
            if (g == 0) {
                ((float *)(rec + QG_A_D))[tl] = f16_round(d);
                if constexpr (TQ == 2) ((float *)(rec + QG_A_S))[tl] = f16_round(d * (float)sum);
            }
        }
    }
}

bool launch_v6_mix5(hipStream_t st, int T, int C, int D, const float * lora, const float * w2,
                    const float * const * maa, const float * xa, const float * sx, const ActBuf * outs) {
    Mix5Args a;
    a.T = T;
    a.C = C;
    a.D = D;
    a.lora = lora;
    a.w2 = w2;
    for (int n = 0; n < 5; n++) {
        a.maa[n] = maa[n];
        a.out[n] = outs[n];
    }
    a.xa = xa;
    a.sx = sx;
    if (D > 64 || C % 32) {
        fprintf(stderr, "rwkv: v6 maa LoRA width %d / n_embed %d unsupported\n", D, C);
        return false;
    }
    const dim3 grid((C + 63) / 64, (T + MIX_TT - 1) / MIX_TT);
    int tq = 0;
    {
        bool all = true;
        for (int n = 0; n < 5; n++)
            all = all && outs[n].tiled && outs[n].fmt == outs[0].fmt && outs[n].K == C &&
                  (outs[n].fmt == A_Q8_0 || outs[n].fmt == A_Q8_1);
        if (all) tq = outs[0].fmt == A_Q8_1 ? 2 : 1;
    }
    // the f32-MFMA form: tiled Q8 outputs, LoRA width 32 or 64, whole 32-channel blocks
    if (tq > 0 && (D == 32 || D == 64) && C % 32 == 0) {
        const dim3 mgrid(C / 32, (T + 63) / 64);
        if (D == 32) {
            if (tq == 1) RK_LAUNCH((k_v6_mix5m<32, 1>), mgrid, dim3(320), 0, st, a);
            else RK_LAUNCH((k_v6_mix5m<32, 2>), mgrid, dim3(320), 0, st, a);
        } else {
            if (tq == 1) RK_LAUNCH((k_v6_mix5m<64, 1>), mgrid, dim3(320), 0, st, a);
            else RK_LAUNCH((k_v6_mix5m<64, 2>), mgrid, dim3(320), 0, st, a);
        }
        HIP_OK(hipGetLastError());
        return true;
    }
#define MIX5_L(DMv, TQv)                                                                  \
    do {                                                                                  \
        if (D == DMv) RK_LAUNCH((k_v6_mix5<DMv, TQv, true>), grid, dim3(320), 0, st, a); \
        else RK_LAUNCH((k_v6_mix5<DMv, TQv, false>), grid, dim3(320), 0, st, a);         \
    } while (0)
    if (D <= 32) {
        if (tq == 1) MIX5_L(32, 1);
        else if (tq == 2) MIX5_L(32, 2);
        else MIX5_L(32, 0);
    } else {
        if (tq == 1) MIX5_L(64, 1);
        else if (tq == 2) MIX5_L(64, 2);
        else MIX5_L(64, 0);
    }
#undef MIX5_L
    HIP_OK(hipGetLastError());
    return true;
}

// --------------------------------------------------------------------------- GroupNorm
template <int TQ>
__global__ __launch_bounds__(1024) void k_groupnorm(int T, int H, int S, float eps, const float * y, const float * w,
                                                    const float * b, int mode, const float * g, const float * v,
                                                    const float * bonus, ActBuf out) {
    const int t = blockIdx.x * TOKS_PER_WG + (threadIdx.x >> 8), C = H * S, tid = threadIdx.x & 255;
    if (t >= T) return;
    // channel block of 256 (4 heads of 64) per grid.y: one channel per thread
    {
        const int c0 = (int)blockIdx.y * 256, c = c0 + tid;
        // whole half-waves out of range (C % 32 == 0; a head of S = 64 makes C % 64 == 0, narrower heads
        // sum inside their own S <= 32 lanes): at C % 64 == 32 the last wave's upper half owns no channel
        if (c0 + (tid & ~31) >= C) return;
        const size_t i = (size_t)t * C + c;
        const float x = y[i];
        const double s = group_tree_sum_d((double)x, S);
        const float mean = (float)div_count(s, S);
        const float d = x - mean;
        const double s2 = group_tree_sum_d((double)(d * d), S);
        const float var = (float)div_count(s2, S);
        const float scale = 1.0f / sqrtf(var + eps);
        float o = d * scale;
        o = o * w[c];
        o = o + b[c];
        if (mode == 2) o = o + v[i] * bonus[(size_t)t * H + c / S];
        if (mode >= 1) o = o * g[i];
        if constexpr (TQ > 0) emit32_tile<TQ>(out.tq, C, t, c, o);
        else emit32(out, t, c, o);
    }
}

bool launch_groupnorm(hipStream_t st, int T, int H, int S, float eps, const float * y, const float * w,
                      const float * b, int mode, const float * g, const float * v, const float * bonus,
                      const ActBuf & out) {
    if (S > 64 || (S & (S - 1))) {
        fprintf(stderr, "rwkv: head size %d unsupported by groupnorm\n", S);
        return false;
    }
    const dim3 grid((T + TOKS_PER_WG - 1) / TOKS_PER_WG, (H * S + 255) / 256), block(256 * TOKS_PER_WG);
    const int tq = tile_q(&out, 1, H * S);
    if (tq == 1) RK_LAUNCH(k_groupnorm<1>, grid, block, 0, st, T, H, S, eps, y, w, b, mode, g, v, bonus, out);
    else if (tq == 2) RK_LAUNCH(k_groupnorm<2>, grid, block, 0, st, T, H, S, eps, y, w, b, mode, g, v, bonus, out);
    else RK_LAUNCH(k_groupnorm<0>, grid, block, 0, st, T, H, S, eps, y, w, b, mode, g, v, bonus, out);
    HIP_OK(hipGetLastError());
    return true;
}

__global__ void k_fill(float * p, size_t n, float value) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = value;
}

__global__ __launch_bounds__(256) void k_copy_rows(const float * src, const uint32_t * src_idx, float * dst,
                                                   const uint32_t * dst_idx, size_t len) {
    const size_t i = blockIdx.y;
    const float * s = src + (src_idx ? (size_t)src_idx[i] : i) * len;
    float * d = dst + (dst_idx ? (size_t)dst_idx[i] : i) * len;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < len; e += (size_t)gridDim.x * 256) d[e] = s[e];
}

bool launch_copy_rows(hipStream_t st, const float * src, const uint32_t * src_idx, float * dst, const uint32_t * dst_idx,
                      int n, size_t len) {
    if (n <= 0 || len == 0) return true;
    const unsigned gx = (unsigned)std::min<size_t>((len + 255) / 256, 1024);
    RK_LAUNCH(k_copy_rows, dim3(gx, (unsigned)n), dim3(256), 0, st, src, src_idx, dst, dst_idx, len);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_fill(hipStream_t st, float * p, size_t n, float value) {
    if (!n) return true;
    RK_LAUNCH(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, n, value);
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi

namespace rwkvmi {

template <int TQ>
__global__ __launch_bounds__(1024) void k_act_from_f32(const float * x, int T, int K, ActBuf out) {
    const int t = blockIdx.x * TOKS_PER_WG + (threadIdx.x >> 8), tid = threadIdx.x & 255;
    if (t >= T) return;
    // 256-channel blocks split over grid.y (v7-2.9B FFN value input, K = 10240: 31 -> 25 us)
    for (int k0 = (int)blockIdx.y * 256; k0 < K; k0 += (int)gridDim.y * 256) {
        const int k = k0 + tid;
        if (k0 + (tid & ~31) >= K) continue;  // half-wave uniform (K % 32 == 0)
        if constexpr (TQ > 0) emit32_tile<TQ>(out.tq, K, t, k, x[(size_t)t * K + k]);
        else emit32(out, t, k, x[(size_t)t * K + k]);
    }
}
bool launch_act_from_f32(hipStream_t st, const float * x, int T, int K, const ActBuf & out) {
    if (K % 32) return false;
    const dim3 grid((T + TOKS_PER_WG - 1) / TOKS_PER_WG, std::min((K + 255) / 256, 8)), block(256 * TOKS_PER_WG);
    const int tq = tile_q(&out, 1, K);
    if (tq == 1) RK_LAUNCH(k_act_from_f32<1>, grid, block, 0, st, x, T, K, out);
    else if (tq == 2) RK_LAUNCH(k_act_from_f32<2>, grid, block, 0, st, x, T, K, out);
    else RK_LAUNCH(k_act_from_f32<0>, grid, block, 0, st, x, T, K, out);
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace rwkvmi
