// wkv_serial.hip -- the serial WKV recurrences of the sequence path (WKV-4, WKV-6 for v5 / v6, v7's
// prep and WKV-7): the kernels whose bits decode, the oracle and every other form are pinned to.
// One kernel per recurrence, a template over the token span (wkv_span.hpp: one sequence, contexts,
// segments of a packed chunk); blockIdx.z is the span.
#include "wkv_span.hpp"

#include <type_traits>
#include "device_common.hpp"

#include <stdio.h>

namespace rwkvmi {

// --------------------------------------------------------------------------- v4 wkv
// tb (both WKV-4 kernels): the output row of the span's token 0
template <class Span>
__global__ __launch_bounds__(256) void k_wkv4(Span sp, int C, const float * r, const float * k, const float * v,
                                              const float * first, const float * decay, const float * sin,
                                              float * sout, ActBuf out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const WkvPlace pl = sp.at(blockIdx.z);
    wkv_advance((size_t)pl.row * C, r, k, v);
    sin += pl.sin, sout += pl.sout;
    const int T = pl.T, tb = (int)pl.row;
    float aa = sin[2 * C + c], bb = sin[3 * C + c], pp = sin[4 * C + c];
    const float fi = first[c], de = decay[c];
    for (int t = 0; t < T; t++) {
        const size_t i = (size_t)t * C + c;
        const float kt = k[i], vt = v[i];
        float ww = fi + kt;
        float qq = fmaxf(pp, ww);
        float e1 = rk_expf(pp - qq), e2 = rk_expf(ww - qq);
        const float an = e1 * aa + e2 * vt;
        const float bn = e1 * bb + e2;
        ww = pp + de;
        qq = fmaxf(ww, kt);
        e1 = rk_expf(ww - qq);
        e2 = rk_expf(kt - qq);
        aa = e1 * aa + e2 * vt;
        bb = e1 * bb + e2;
        pp = qq;
        emit32(out, tb + t, c, r[i] * (an / bn));
    }
    sout[2 * C + c] = aa;
    sout[3 * C + c] = bb;
    sout[4 * C + c] = pp;
}

// Sequence form (whole waves of channels, more than one token or a segment): the same per-channel
// recurrence, one wave per 64 channels.
// The k / v / r rows of the next WKV4_TT tokens are loaded while the current ones are computed
// (the recurrence's dependent chain no longer waits on a load round trip per token), and the
// outputs of a chunk are emitted after its recurrence steps, off the chain.  Per channel and
// token the operations are k_wkv4's, in its order, so decode and sequence stay bit-identical.
constexpr int WKV4_TT = 16;
template <class Span>
__global__ __launch_bounds__(64) void k_wkv4_seq(Span sp, int C, const float * r, const float * k, const float * v,
                                                 const float * first, const float * decay, const float * sin,
                                                 float * sout, ActBuf out) {
    const WkvPlace pl = sp.at(blockIdx.z);
    wkv_advance((size_t)pl.row * C, r, k, v);
    sin += pl.sin, sout += pl.sout;
    const int T = pl.T, tb = (int)pl.row;
    const int c = blockIdx.x * 64 + threadIdx.x;
    const int cl = min(c, C - 1);
    float aa = sin[2 * C + cl], bb = sin[3 * C + cl], pp = sin[4 * C + cl];
    const float fi = first[cl], de = decay[cl];
    float kn[WKV4_TT], vn[WKV4_TT], rn[WKV4_TT];
    auto load = [&](int t0) {
#pragma unroll
        for (int tt = 0; tt < WKV4_TT; tt++) {
            const size_t i = (size_t)min(t0 + tt, T - 1) * C + cl;
            kn[tt] = k[i];
            vn[tt] = v[i];
            rn[tt] = r[i];
        }
    };
    load(0);
#pragma unroll 1
    for (int t0 = 0; t0 < T; t0 += WKV4_TT) {
        float kc[WKV4_TT], vc[WKV4_TT], rc[WKV4_TT], y[WKV4_TT];
#pragma unroll
        for (int tt = 0; tt < WKV4_TT; tt++) kc[tt] = kn[tt], vc[tt] = vn[tt], rc[tt] = rn[tt];
        if (t0 + WKV4_TT < T) load(t0 + WKV4_TT);
        const int n = min(WKV4_TT, T - t0);
#pragma unroll
        for (int tt = 0; tt < WKV4_TT; tt++) {
            if (tt < n) {  // uniform
                const float kt = kc[tt], vt = vc[tt];
                float ww = fi + kt;
                float qq = fmaxf(pp, ww);
                float e1 = rk_expf(pp - qq), e2 = rk_expf(ww - qq);
                const float an = e1 * aa + e2 * vt;
                const float bn = e1 * bb + e2;
                ww = pp + de;
                qq = fmaxf(ww, kt);
                e1 = rk_expf(ww - qq);
                e2 = rk_expf(kt - qq);
                aa = e1 * aa + e2 * vt;
                bb = e1 * bb + e2;
                pp = qq;
                y[tt] = rc[tt] * (an / bn);
            }
        }
#pragma unroll
        for (int tt = 0; tt < WKV4_TT; tt++)
            if (tt < n) emit32(out, tb + t0 + tt, c, y[tt]);
    }
    if (c < C) {
        sout[2 * C + c] = aa;
        sout[3 * C + c] = bb;
        sout[4 * C + c] = pp;
    }
}

bool launch_wkv4(hipStream_t st, int T, int C, const float * r, const float * k, const float * v,
                 const float * first, const float * decay, const float * state_in, float * state_out,
                 const ActBuf & out, int bs, const SegTab * seg) {
    return with_span(T, bs, seg, [&](auto sp, int nz) {
        using Span = decltype(sp);
        // k_wkv4_seq for whole waves of channels, except one token of one sequence (decode) and the
        // contexts (a segment of one token takes it too: per channel and token the two kernels are
        // the same operations)
        if constexpr (!std::is_same_v<Span, SpanCtx>) {
            if (C % 64 == 0 && (seg || T > 1)) {
                RK_LAUNCH(k_wkv4_seq<Span>, dim3(C / 64, 1, nz), dim3(64), 0, st, sp, C, r, k, v, first, decay, state_in,
                          state_out, out);
                HIP_OK(hipGetLastError());
                return true;
            }
        }
        RK_LAUNCH(k_wkv4<Span>, dim3((C + 255) / 256, 1, nz), dim3(256), 0, st, sp, C, r, k, v, first, decay,
                  state_in, state_out, out);
        HIP_OK(hipGetLastError());
        return true;
    });
}

// --------------------------------------------------------------------------- wkv6 (v5/v6)
// One workgroup per head; lane group (j, g): j = value index, g splits the key index i.
// The state column S[i][j] for the lane's IPG keys lives in registers across all T tokens.
template <int IPG, class Span>
__global__ void k_wkv6(Span sp, int H, int S, int G, const float * k, const float * v, const float * r,
                       const float * u, const float * w, int w_per_token, const float * sin, float * sout,
                       float * y) {
    const int h = blockIdx.x;
    const int j = threadIdx.x / G, g = threadIdx.x % G;
    const int C = H * S;
    const WkvPlace pl = sp.at(blockIdx.z);
    wkv_advance((size_t)pl.row * C, k, v, r, y);
    if (w_per_token) wkv_advance((size_t)pl.row * C, w);
    sin += pl.sin, sout += pl.sout;
    const int T = pl.T;
    float st[IPG];
    const size_t hb = (size_t)h * S * S;
#pragma unroll
    for (int ii = 0; ii < IPG; ii++) st[ii] = sin[hb + (size_t)(g * IPG + ii) * S + j];
    float uu[IPG];
#pragma unroll
    for (int ii = 0; ii < IPG; ii++) uu[ii] = u[h * S + g * IPG + ii];
    for (int t = 0; t < T; t++) {
        const size_t th = (size_t)t * C + (size_t)h * S;
        const float * wt = w + (w_per_token ? (size_t)t * C : 0) + (size_t)h * S;
        const float vj = v[th + j];
        float acc = 0.0f;
#pragma unroll
        for (int ii = 0; ii < IPG; ii++) {
            const int i = g * IPG + ii;
            const float kv = vj * k[th + i];
            const float prev = st[ii];
            const float temp = kv * uu[ii] + prev;
            acc += temp * r[th + i];
            st[ii] = prev * wt[i] + kv;
        }
        acc = group_sum(acc, G);
        if (g == 0) y[th + j] = acc;
    }
#pragma unroll
    for (int ii = 0; ii < IPG; ii++) sout[hb + (size_t)(g * IPG + ii) * S + j] = st[ii];
}

// Head sizes other than 64 (WKV-6 and WKV-7): G = min(256 / S, S) lane groups split the keys, N = S / G
// keys per lane, a power of two up to 32.  f(G, integral_constant<int, N>) launches.
template <class F>
static bool with_key_groups(int S, F && f) {
    int G = 256 / S;
    if (G > S) G = S;
    if (G < 1) G = 1;
    switch (S / G) {
        case 1: return f(G, std::integral_constant<int, 1>());
        case 2: return f(G, std::integral_constant<int, 2>());
        case 4: return f(G, std::integral_constant<int, 4>());
        case 8: return f(G, std::integral_constant<int, 8>());
        case 16: return f(G, std::integral_constant<int, 16>());
        case 32: return f(G, std::integral_constant<int, 32>());
    }
    fprintf(stderr, "rwkv: unsupported head size %d\n", S);
    return false;
}

typedef float f2_t __attribute__((ext_vector_type(2)));

// Head size 64 (every released v5/v6 model), four keys per lane.  Workgroup = 4 waves over 16
// value columns of one head, grid (H, 4).  Lane (g = lane >> 4, jl = (lane >> 2) & 3, q = lane & 3)
// of wave wv owns column j = 16*blockIdx.y + 4*wv + jl for keys i = 16g + 4q + e (e < 4): the
// per-element arithmetic is k_att6_dec's (packed pairs, the same IEEE mul / add per element, no
// contraction).  The output sum has k_att6_dec's association exactly: each lane sums its 4 keys
// in order starting from 0 (p_q), the quad folds them as (p0 + p1) + (p2 + p3) (DPP quad
// permutes xor 1, xor 2; float addition commutes, so every lane of the quad holds the same bits),
// and the 4 key groups are folded with fold_g4 ((s0 + s2) + (s1 + s3)): 8 dependent VALU ops per
// token instead of a 16-add chain through the lanes.  Chunks of 64 tokens of k, r, w and v
// are staged in LDS with coalesced loads, the next chunk in flight while this one runs.

// Sum over the four lane groups g = lane >> 4: partner g ^ 2 (permlane32 swap), then g ^ 1
// (permlane16 swap) -- the (p0 + p2) + (p1 + p3) of group_sum(., 4) on adjacent lanes.
__device__ __forceinline__ float fold_g4(float v) {
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false);
    v = __int_as_float(a[0]) + __int_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false);
    return __int_as_float(b[0]) + __int_as_float(b[1]);
}

// v + (v of lane ^ 1) and v + (v of lane ^ 2) inside each quad
__device__ __forceinline__ float quad_add_x1(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
}
__device__ __forceinline__ float quad_add_x2(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
}

// acc continued over the lane's 4 terms in order
__device__ __forceinline__ float chain4(float acc, const f2_t (&x)[2]) {
    acc += x[0].x;
    acc += x[0].y;
    acc += x[1].x;
    acc += x[1].y;
    return acc;
}

// wkv6 chunk: 64 tokens, so the next chunk's loads have a whole chunk of compute to land in
constexpr int WKV6_TC = 64;
constexpr int WKV6_PAD = 8;  // >= 2 * the token group

// four waves per workgroup, fixed: the chunk staging below is written for it (four named float4 per
// operand and thread -- as arrays over a variable width they are kept in scratch)
constexpr int WKV6_NWV = 4;

template <bool WPT, class Span>
__global__ __launch_bounds__(64 * WKV6_NWV) void k_wkv6_s64(Span sp, int H, const float * k, const float * v,
                                                            const float * r, const float * u, const float * w,
                                                            const float * sin, float * sout, float * y) {
    constexpr int S = 64, NWV = WKV6_NWV;
    const WkvPlace pl = sp.at(blockIdx.z);
    wkv_advance((size_t)pl.row * H * S, k, v, r, y);
    if constexpr (WPT) wkv_advance((size_t)pl.row * H * S, w);
    sin += pl.sin, sout += pl.sout;
    const int T = pl.T;
    constexpr int CW = 4 * NWV, NT = 64 * NWV;
    static_assert(WKV6_TC * 16 == 4 * NT, "four float4 of k, r, w per thread and chunk");
    // WKV6_PAD rows past the chunk: a full chunk's look-ahead reads need no clamp (their tokens
    // are never used)
    constexpr int RW = WKV6_TC + WKV6_PAD;
    __shared__ __attribute__((aligned(16))) float sk[RW][S], sr[RW][S], sw[WPT ? RW : 1][S], sv[RW][CW],
        sy[WKV6_TC][CW];
    const int h = blockIdx.x, jb = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int q = lane & 3, jl = (lane >> 2) & 3, g = lane >> 4;
    const int jc = 4 * wv + jl, j = jb * CW + jc, i0 = g * 16 + 4 * q;
    const int C = H * S;
    const size_t hb = (size_t)h * S * S;
    f2_t st[2], uu[2], wc[2];
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int i = i0 + 2 * p;
        st[p] = f2_t{sin[hb + (size_t)i * S + j], sin[hb + (size_t)(i + 1) * S + j]};
        uu[p] = f2_t{u[h * S + i], u[h * S + i + 1]};
        wc[p] = WPT ? f2_t{0.f, 0.f} : f2_t{w[h * S + i], w[h * S + i + 1]};
    }
    // chunk staging: k/r/w rows of 64 floats = 16 float4 per token; thread moves float4
    // #(tid & 15) of tokens (tid >> 4) + (NT/16) qq, qq < 4; v: CW columns = NWV float4 per
    // token, threads < WKV6_TC*NWV move float4 #(tid % NWV) of token tid / NWV
    // the chunk's rows in named registers -- as arrays they are kept in scratch
    float4 k0, k1, k2, k3, r0, r1, r2, r3, w0, w1, w2, w3, pv;
#define WKV6_LD(QI, KV, RV, WV)                                                                           \
    do {                                                                                                  \
        const int t = min(t0 + (tid >> 4) + (NT / 16) * (QI), T - 1);                                     \
        const size_t base = (size_t)t * C + (size_t)h * S + 4 * (tid & 15);                               \
        KV = *(const float4 *)(k + base);                                                                 \
        RV = *(const float4 *)(r + base);                                                                 \
        if constexpr (WPT) WV = *(const float4 *)(w + base);                                              \
    } while (0)
#define WKV6_ST(QI, KV, RV, WV)                                                                           \
    do {                                                                                                  \
        const int tt = (tid >> 4) + (NT / 16) * (QI);                                                     \
        *(float4 *)&sk[tt][4 * (tid & 15)] = KV;                                                          \
        *(float4 *)&sr[tt][4 * (tid & 15)] = RV;                                                          \
        if constexpr (WPT) *(float4 *)&sw[tt][4 * (tid & 15)] = WV;                                       \
    } while (0)
    auto load_chunk = [&](int t0) __attribute__((always_inline)) {
        WKV6_LD(0, k0, r0, w0);
        WKV6_LD(1, k1, r1, w1);
        WKV6_LD(2, k2, r2, w2);
        WKV6_LD(3, k3, r3, w3);
        const int tv = min(tid, WKV6_TC * NWV - 1);
        const int t = min(t0 + tv / NWV, T - 1);
        pv = *(const float4 *)(v + (size_t)t * C + (size_t)h * S + jb * CW + 4 * (tv % NWV));
    };
    auto store_chunk = [&]() __attribute__((always_inline)) {
        WKV6_ST(0, k0, r0, w0);
        WKV6_ST(1, k1, r1, w1);
        WKV6_ST(2, k2, r2, w2);
        WKV6_ST(3, k3, r3, w3);
        if (tid < WKV6_TC * NWV) *(float4 *)&sv[tid / NWV][4 * (tid % NWV)] = pv;
    };
#undef WKV6_LD
#undef WKV6_ST
    struct Tok {
        f2_t k[2], r[2], w[2];
        float v;
    };
    auto read_tok = [&](Tok & o, int tt) __attribute__((always_inline)) {
        const float4 a = *(const float4 *)&sk[tt][i0];
        const float4 b = *(const float4 *)&sr[tt][i0];
        o.k[0] = f2_t{a.x, a.y}, o.k[1] = f2_t{a.z, a.w};
        o.r[0] = f2_t{b.x, b.y}, o.r[1] = f2_t{b.z, b.w};
        if constexpr (WPT) {
            const float4 c = *(const float4 *)&sw[tt][i0];
            o.w[0] = f2_t{c.x, c.y}, o.w[1] = f2_t{c.z, c.w};
        }
        o.v = sv[tt][jc];
    };
    load_chunk(0);
    for (int t0 = 0; t0 < T; t0 += WKV6_TC) {
        store_chunk();
        __syncthreads();
        if (t0 + WKV6_TC < T) load_chunk(t0 + WKV6_TC);  // in flight during this chunk
        const int n = min(WKV6_TC, T - t0);
        // Tokens in groups of TG: the state updates run token after token, then the TG output
        // chains (independent of each other) are interleaved step by step.
        constexpr int TG = 4;
        static_assert(2 * TG <= WKV6_PAD, "look-ahead rows");
        // FULL: a whole chunk (n == WKV6_TC), every token valid
        auto group = [&](const Tok (&o)[TG], int tt0, auto full) __attribute__((always_inline)) {
            constexpr bool FULL = decltype(full)::value;
            f2_t x[TG][2];
#pragma unroll
            for (int e = 0; e < TG; e++) {
                const bool val = FULL || tt0 + e < n;
                const f2_t vj = f2_t{o[e].v, o[e].v};
                f2_t kv[2];
#pragma unroll
                for (int p = 0; p < 2; p++) kv[p] = vj * o[e].k[p];
#pragma unroll
                for (int p = 0; p < 2; p++) x[e][p] = kv[p] * uu[p];
#pragma unroll
                for (int p = 0; p < 2; p++) x[e][p] = x[e][p] + st[p];
#pragma unroll
                for (int p = 0; p < 2; p++) x[e][p] = x[e][p] * o[e].r[p];
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    f2_t ns = st[p] * (WPT ? o[e].w[p] : wc[p]);
                    ns = ns + kv[p];
                    st[p] = val ? ns : st[p];
                }
            }
            // p_q (4 keys in order), (p0 + p1) + (p2 + p3) over the quad, TG sums side by side
            float acc[TG];
#pragma unroll
            for (int e = 0; e < TG; e++) acc[e] = chain4(0.0f, x[e]);
#pragma unroll
            for (int e = 0; e < TG; e++) acc[e] = quad_add_x1(acc[e]);
#pragma unroll
            for (int e = 0; e < TG; e++) acc[e] = quad_add_x2(acc[e]);
            // every lane of the column holds the same sum: all write it to the chunk's y tile
#pragma unroll
            for (int e = 0; e < TG; e++) {
                acc[e] = fold_g4(acc[e]);
                if (FULL || tt0 + e < n) sy[tt0 + e][jc] = acc[e];
            }
        };
        // two operand sets in turn: the next group's LDS reads overlap this group's arithmetic
        Tok A[TG], B[TG];
        if (n == WKV6_TC) {
            const std::integral_constant<bool, true> full;
#pragma unroll
            for (int e = 0; e < TG; e++) read_tok(A[e], e);
            for (int tt = 0; tt < WKV6_TC; tt += 2 * TG) {
#pragma unroll
                for (int e = 0; e < TG; e++) read_tok(B[e], tt + TG + e);
                group(A, tt, full);
#pragma unroll
                for (int e = 0; e < TG; e++) read_tok(A[e], tt + 2 * TG + e);
                group(B, tt + TG, full);
            }
        } else {
            const std::integral_constant<bool, false> part;
#pragma unroll
            for (int e = 0; e < TG; e++) read_tok(A[e], min(e, n - 1));
            for (int tt = 0; tt < n; tt += 2 * TG) {
#pragma unroll
                for (int e = 0; e < TG; e++) read_tok(B[e], min(tt + TG + e, n - 1));
                group(A, tt, part);
                if (tt + TG >= n) break;
#pragma unroll
                for (int e = 0; e < TG; e++) read_tok(A[e], min(tt + 2 * TG + e, n - 1));
                group(B, tt + TG, part);
            }
        }
        __syncthreads();
        // the chunk's y tile [n tokens][CW columns], one float4 per thread
        {
            const int tk = tid / NWV;
            if (tk < n)
                *(float4 *)(y + (size_t)(t0 + tk) * C + (size_t)h * S + jb * CW + 4 * (tid % NWV)) =
                    *(const float4 *)&sy[tk][4 * (tid % NWV)];
        }
    }
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int i = i0 + 2 * p;
        sout[hb + (size_t)i * S + j] = st[p].x;
        sout[hb + (size_t)(i + 1) * S + j] = st[p].y;
    }
}

bool launch_wkv6(hipStream_t st, int T, int H, int S, const float * k, const float * v, const float * r,
                 const float * u, const float * w, int w_per_token, const float * state_in, float * state_out,
                 float * y, const SegTab * seg) {
    return with_span(T, seg, [&](auto sp, int nz) {
        using Span = decltype(sp);
        if (S == 64) {
            const dim3 grid(H, 16 / WKV6_NWV, nz), block(64 * WKV6_NWV);
            if (w_per_token) RK_LAUNCH((k_wkv6_s64<true, Span>), grid, block, 0, st, sp, H, k, v, r, u, w, state_in, state_out, y);
            else RK_LAUNCH((k_wkv6_s64<false, Span>), grid, block, 0, st, sp, H, k, v, r, u, w, state_in, state_out, y);
            HIP_OK(hipGetLastError());
            return true;
        }
        return with_key_groups(S, [&](int G, auto ipg) {
            RK_LAUNCH((k_wkv6<decltype(ipg)::value, Span>), dim3(H, 1, nz), dim3(S * G), 0, st, sp, H, S, G, k, v, r, u, w,
                      w_per_token, state_in, state_out, y);
            HIP_OK(hipGetLastError());
            return true;
        });
    });
}

// --------------------------------------------------------------------------- v7
// Per token: thread per channel, heads are S consecutive channels (S <= 64, power of two).
__global__ __launch_bounds__(256) void k_v7_prep(int T, int H, int S, float * k, const float * a, const float * r,
                                                 const float * k_k, const float * k_a, const float * r_k, float * nb,
                                                 float * bb, float * bonus) {
    const int t = blockIdx.x, C = H * S;
    // one 256-channel block (whole heads) per grid.y: no serial walk over the channel blocks
    {
        const int c0 = (int)blockIdx.y * blockDim.x, c = c0 + threadIdx.x;
        if (c0 + (int)(threadIdx.x & ~63) >= C) return;  // whole wave out of range
        const size_t i = (size_t)t * C + c;
        const float kv = k[i];
        const float kkr = kv * k_k[c];
        const float sum = group_sum(kkr * kkr, S);
        const float scale = 1.0f / fmaxf(sqrtf(sum), 1e-12f);
        const float kk = kkr * scale;
        const float av = a[i];
        const float ka = kv * k_a[c];
        const float kadj = kv + (av * ka - ka);
        k[i] = kadj;
        nb[i] = -kk;
        bb[i] = kk * av;
        const float bsum = group_sum((kadj * r[i]) * r_k[c], S);
        if ((c % S) == 0) bonus[(size_t)t * H + c / S] = bsum;
    }
}

bool launch_v7_prep(hipStream_t st, int T, int H, int S, float * k, const float * a, const float * r,
                    const float * k_k, const float * k_a, const float * r_k, float * nb, float * bb, float * bonus) {
    if (S > 64 || (S & (S - 1))) {
        fprintf(stderr, "rwkv: v7 head size %d unsupported\n", S);
        return false;
    }
    RK_LAUNCH(k_v7_prep, dim3(T, (H * S + 255) / 256), dim3(256), 0, st, T, H, S, k, a, r, k_k, k_a, r_k, nb,
                       bb, bonus);
    HIP_OK(hipGetLastError());
    return true;
}

// state [h][i(value)][j(key)]; lane group (i, g): g splits j.
template <int JPG, class Span>
__global__ void k_wkv7(Span sp, int H, int S, int G, const float * r, const float * w, const float * k,
                       const float * v, const float * a, const float * b, const float * sin, float * sout,
                       float * y) {
    const int h = blockIdx.x;
    const int i = threadIdx.x / G, g = threadIdx.x % G;
    const int C = H * S;
    const WkvPlace pl = sp.at(blockIdx.z);
    wkv_advance((size_t)pl.row * C, r, w, k, v, a, b, y);
    sin += pl.sin, sout += pl.sout;
    const int T = pl.T;
    const size_t hb = (size_t)h * S * S + (size_t)i * S + g * JPG;
    float st[JPG];
#pragma unroll
    for (int jj = 0; jj < JPG; jj++) st[jj] = sin[hb + jj];
    for (int t = 0; t < T; t++) {
        const size_t th = (size_t)t * C + (size_t)h * S + g * JPG;
        float sa = 0.0f;
#pragma unroll
        for (int jj = 0; jj < JPG; jj++) sa += a[th + jj] * st[jj];
        sa = group_sum(sa, G);
        const float vi = v[(size_t)t * C + (size_t)h * S + i];
        float acc = 0.0f;
#pragma unroll
        for (int jj = 0; jj < JPG; jj++) {
            const float kv = vi * k[th + jj];
            const float ns = st[jj] * w[th + jj] + kv + sa * b[th + jj];
            st[jj] = ns;
            acc += ns * r[th + jj];
        }
        acc = group_sum(acc, G);
        if (g == 0) y[(size_t)t * C + (size_t)h * S + i] = acc;
    }
#pragma unroll
    for (int jj = 0; jj < JPG; jj++) sout[hb + jj] = st[jj];
}

// Head size 64: keys in 16 groups of 4 (k_att7_dec's split for S = 64, G = 16).  Workgroup = 4
// waves over 16 value rows of one head, grid (H, 4); lane (g = lane & 15, il = 4 wv + (lane >> 4))
// owns row i = 16 blockIdx.y + il, keys j = 4g .. 4g + 3.  Per token: sa = sum_j a_j s_ij (4 terms
// in order from 0, then the 16 groups folded by the butterfly xor 8, 4, 2, 1 -- DPP row rotations,
// every lane of the row ends with the same bits), the state update, and the output sum the same
// way.  r, w, k, a, b (and v) come in 16-token chunks staged in a double-buffered LDS tile (the next
// chunk in registers while the current one runs); y goes through an LDS tile, one store per chunk.
constexpr int WKV7_TC = 16;

// v + v(lane + 8 mod 16) + ... over a 16-lane DPP row: the butterfly of group_sum(., 16)
__device__ __forceinline__ float row_bfly16(float v) {
    v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, false));
    v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xF, 0xF, false));
    v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xF, 0xF, false));
    v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xF, 0xF, false));
    return v;
}

template <class Span>
__global__ __launch_bounds__(256) void k_wkv7_s64(Span sp, int H, const float * r, const float * w, const float * k,
                                                  const float * v, const float * a, const float * b,
                                                  const float * sin, float * sout, float * y) {
    constexpr int S = 64;
    const WkvPlace pl = sp.at(blockIdx.z);
    wkv_advance((size_t)pl.row * H * S, r, w, k, v, a, b, y);
    sin += pl.sin, sout += pl.sout;
    const int T = pl.T;
    __shared__ __attribute__((aligned(16))) float sr[2][WKV7_TC][S], sw[2][WKV7_TC][S], sk[2][WKV7_TC][S],
        sa_[2][WKV7_TC][S], sb[2][WKV7_TC][S], sv[2][WKV7_TC][16], sy[2][WKV7_TC][16];
    const int h = blockIdx.x, ib = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = lane & 15, il = 4 * wv + (lane >> 4), i = ib * 16 + il;
    const int C = H * S;
    const size_t hb = (size_t)h * S * S + (size_t)i * S + 4 * g;
    float st[4];
#pragma unroll
    for (int e = 0; e < 4; e++) st[e] = sin[hb + e];  // (state slices need not be 16-byte aligned)
    // staging: thread moves float4 #(tid & 15) of token (tid >> 4) of the five key-indexed rows;
    // threads < 64 one float4 of v (token tid >> 2, rows 4 (tid & 3) ..)
    float4 q0, q1, q2, q3, q4, qv;
    const int c4 = 4 * (tid & 15), tl = tid >> 4;
    auto load = [&](int t0) __attribute__((always_inline)) {
        const int t = min(t0 + tl, T - 1);
        const size_t base = (size_t)t * C + (size_t)h * S + c4;
        q0 = *(const float4 *)(r + base);
        q1 = *(const float4 *)(w + base);
        q2 = *(const float4 *)(k + base);
        q3 = *(const float4 *)(a + base);
        q4 = *(const float4 *)(b + base);
        if (tid < 64) {
            const int tv = min(t0 + (tid >> 2), T - 1);
            qv = *(const float4 *)(v + (size_t)tv * C + (size_t)h * S + ib * 16 + 4 * (tid & 3));
        }
    };
    auto store = [&](int bf) __attribute__((always_inline)) {
        *(float4 *)&sr[bf][tl][c4] = q0;
        *(float4 *)&sw[bf][tl][c4] = q1;
        *(float4 *)&sk[bf][tl][c4] = q2;
        *(float4 *)&sa_[bf][tl][c4] = q3;
        *(float4 *)&sb[bf][tl][c4] = q4;
        if (tid < 64) *(float4 *)&sv[bf][tid >> 2][4 * (tid & 3)] = qv;
    };
    load(0);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int t0 = 0; t0 < T; t0 += WKV7_TC) {
        const int n = min(WKV7_TC, T - t0);
        const bool nx = t0 + WKV7_TC < T;
        if (nx) load(t0 + WKV7_TC);  // in flight during this chunk
        // token tt's operands are in registers while token tt + 1's are read (the LDS latency stays
        // off the recurrence's critical path); whole chunks fully unrolled
        struct Op {
            float4 a, k, w, b, r;
            float v;
        };
        auto rd = [&](Op & o, int tt) __attribute__((always_inline)) {
            o.a = *(const float4 *)&sa_[buf][tt][4 * g];
            o.k = *(const float4 *)&sk[buf][tt][4 * g];
            o.w = *(const float4 *)&sw[buf][tt][4 * g];
            o.b = *(const float4 *)&sb[buf][tt][4 * g];
            o.r = *(const float4 *)&sr[buf][tt][4 * g];
            o.v = sv[buf][tt][il];
        };
        auto tok = [&](const Op & o, int tt) __attribute__((always_inline)) {
            float sa = 0.0f;
            sa += o.a.x * st[0];
            sa += o.a.y * st[1];
            sa += o.a.z * st[2];
            sa += o.a.w * st[3];
            sa = row_bfly16(sa);
            const float kk[4] = {o.k.x, o.k.y, o.k.z, o.k.w}, ww[4] = {o.w.x, o.w.y, o.w.z, o.w.w};
            const float bb[4] = {o.b.x, o.b.y, o.b.z, o.b.w}, rr[4] = {o.r.x, o.r.y, o.r.z, o.r.w};
            float acc = 0.0f;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float kv = o.v * kk[e];
                const float ns = st[e] * ww[e] + kv + sa * bb[e];
                st[e] = ns;
                acc += ns * rr[e];
            }
            acc = row_bfly16(acc);
            if (g == 0) sy[buf][tt][il] = acc;
        };
        Op cur, nxt;
        rd(cur, 0);
        if (n == WKV7_TC) {
            // two tokens ahead: token tt + 2's LDS reads are issued before token tt's chain, so the
            // recurrence never waits on the LDS
            Op ring[3];
            ring[0] = cur;
            rd(ring[1], 1);
#pragma unroll
            for (int tt = 0; tt < WKV7_TC; tt++) {
                if (tt + 2 < WKV7_TC) rd(ring[(tt + 2) % 3], tt + 2);
                tok(ring[tt % 3], tt);
            }
        } else {
#pragma unroll 1
            for (int tt = 0; tt < n; tt++) {
                rd(nxt, min(tt + 1, n - 1));
                tok(cur, tt);
                cur = nxt;
            }
        }
        if (nx) store(buf ^ 1);
        __syncthreads();
        // the chunk's y tile [n tokens][16 rows]: threads < 64 one float4
        if (tid < 64 && (tid >> 2) < n)
            *(float4 *)(y + (size_t)(t0 + (tid >> 2)) * C + (size_t)h * S + ib * 16 + 4 * (tid & 3)) =
                *(const float4 *)&sy[buf][tid >> 2][4 * (tid & 3)];
        buf ^= 1;
    }
#pragma unroll
    for (int e = 0; e < 4; e++) sout[hb + e] = st[e];
}

bool launch_wkv7(hipStream_t st, int T, int H, int S, const float * r, const float * w, const float * k,
                 const float * v, const float * a, const float * b, const float * state_in, float * state_out,
                 float * y, const SegTab * seg) {
    return with_span(T, seg, [&](auto sp, int nz) {
        using Span = decltype(sp);
        if (S == 64) {
            RK_LAUNCH(k_wkv7_s64<Span>, dim3(H, 4, nz), dim3(256), 0, st, sp, H, r, w, k, v, a, b, state_in, state_out, y);
            HIP_OK(hipGetLastError());
            return true;
        }
        return with_key_groups(S, [&](int G, auto jpg) {
            RK_LAUNCH((k_wkv7<decltype(jpg)::value, Span>), dim3(H, 1, nz), dim3(S * G), 0, st, sp, H, S, G, r, w, k, v, a, b,
                      state_in, state_out, y);
            HIP_OK(hipGetLastError());
            return true;
        });
    });
}

}  // namespace rwkvmi

