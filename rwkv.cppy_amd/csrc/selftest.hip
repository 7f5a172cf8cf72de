// selftest.hip -- kernel self-test entry points (include/rwkv_mi355x.h): run one kernel on
// host-provided operands so tests can check it against the oracle's primitive of the same
// name (oracle_quantize_act, oracle_matmul) without whole-model noise.
#include <string.h>

#include <tuple>
#include <vector>

#include "../../include/rwkv_mi355x.h"
#include "engine.hpp"
#include "kernels.hpp"
#include "mv_common.hpp"

using namespace rwkvmi;

namespace {

// One wave: lane l holds p[l][0..N-1].  sums[l] = what wave_sums<N> returns in lane l; ref[j] =
// wave_sum63 of slot j (from lane 63).
template <int N>
__global__ __launch_bounds__(64) void k_selftest_wave_sums(const float * p, float * sums, float * ref) {
    const int lane = threadIdx.x;
    float v[N];
#pragma unroll
    for (int j = 0; j < N; j++) v[j] = p[lane * N + j];
    sums[lane] = wave_sums<N>(v, lane);
#pragma unroll
    for (int j = 0; j < N; j++) {
        const float t = wave_sum63(v[j]);
        if (lane == 63) ref[j] = t;
    }
}

// The matvecs' row_sums<WF, 3> (a padded zero slot): p[l][0..2] = acc, p[l][3..5] = acc2 (read by
// the _1 form only); sums[l] = its result in lane l; ref[j] = the per-row expression it replaces.
template <int WF>
__global__ __launch_bounds__(64) void k_selftest_row_sums3(const float * p, float * sums, float * ref) {
    const int lane = threadIdx.x;
    float a[3], a2[3];
#pragma unroll
    for (int j = 0; j < 3; j++) a[j] = p[lane * 6 + j], a2[j] = p[lane * 6 + 3 + j];
    sums[lane] = row_sums<WF, 3>(a, a2, lane);
    constexpr bool one = WF == W_Q4_1 || WF == W_Q5_1;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float t = one ? wave_sum63(a[j]) + wave_sum63(a2[j]) : wave_sum63(a[j]) + 0.0f;
        if (lane == 63) ref[j] = t;
    }
}

struct DevBufs {
    std::vector<void *> p;
    void * alloc(size_t n) {
        void * q = nullptr;
        if (hipMalloc(&q, n + 64) != hipSuccess) return nullptr;
        (void)hipMemset(q, 0, n + 64);
        p.push_back(q);
        return q;
    }
    ~DevBufs() {
        for (void * q : p) (void)hipFree(q);
    }
};

bool make_act(DevBufs & b, int fmt, int T, int K, ActBuf & a) {
    memset(&a, 0, sizeof(a));
    a.fmt = fmt;
    a.K = K;
    const size_t n = (size_t)T * K, nb = n / 32 + 1;
    a.f = (float *)b.alloc(n * 4);
    a.h = (__half *)b.alloc(n * 2);
    a.q = (int8_t *)b.alloc(n);
    a.d = (float *)b.alloc(nb * 4);
    a.s = (float *)b.alloc(nb * 4);
    a.qsum = (int *)b.alloc(nb * 4);
    a.tq = (uint8_t *)b.alloc(((size_t)T + QG_TOK - 1) / QG_TOK * (K / 32) * qg_a_bytes(true));
    return a.f && a.h && a.q && a.d && a.s && a.qsum && a.tq;
}

// Token-tile records (common.hpp qg_*: what the GEMM's operand copy reads) of a [T][K] Q8 activation,
// back on the host as row-major q [T][K], d / s / qsum [T][K / 32] (any may be NULL; the records hold
// no block sums: qsum is the sum of the returned codes).
bool detile_act(const ActBuf & a, int T, int K, int8_t * q, float * d, float * s, int32_t * qsum) {
    const bool one = a.fmt == A_Q8_1;
    const size_t nbk = (size_t)K / 32, rb = qg_a_bytes(one);
    std::vector<uint8_t> h(((size_t)T + QG_TOK - 1) / QG_TOK * nbk * rb);
    if (hipMemcpy(h.data(), a.tq, h.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (int t = 0; t < T; t++)
        for (size_t b = 0; b < nbk; b++) {
            const uint8_t * rec = h.data() + ((size_t)(t / QG_TOK) * nbk + b) * rb;
            const int tl = t % QG_TOK;
            int sum = 0;
            for (int k = 0; k < 32; k++) {
                const int8_t v = (int8_t)rec[(k >> 4) * QG_TOK * 16 + tl * 16 + (k & 15)];
                sum += v;
                if (q) q[(size_t)t * K + b * 32 + k] = v;
            }
            if (d) d[t * nbk + b] = ((const float *)(rec + QG_A_D))[tl];
            if (s && one) s[t * nbk + b] = ((const float *)(rec + QG_A_S))[tl];
            if (qsum) qsum[t * nbk + b] = sum;
        }
    return true;
}

}  // namespace

extern "C" RWKV_API bool rwkv_mi355x_selftest_quantize_act(int wtype, const float * x, int T, int K, int8_t * q,
                                                           float * d, float * s) {
    if (K % 32 || T <= 0) return false;
    DevBufs b;
    ActBuf a;
    const int fmt = act_fmt_for(wtype);
    float * dx = (float *)b.alloc((size_t)T * K * 4);
    if (!dx || !make_act(b, fmt, T, K, a)) return false;
    if (hipMemcpy(dx, x, (size_t)T * K * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    if (!launch_act_from_f32(nullptr, dx, T, K, a)) return false;
    if (hipDeviceSynchronize() != hipSuccess) return false;
    const size_t nb = (size_t)T * K / 32;
    if (q && hipMemcpy(q, a.q, (size_t)T * K, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (d && hipMemcpy(d, a.d, nb * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (s && hipMemcpy(s, a.s, nb * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    return true;
}

static bool selftest_mm(int wtype, const void * W, int K, int M, const float * x, int T, float * y, bool mfma,
                        int split = 0) {
    if (K % 32 || T <= 0 || M <= 0) return false;
    HostTensor ht;
    ht.name = "selftest";
    ht.type = (uint32_t)wtype;
    ht.ndim = 2;
    ht.ne[0] = (uint32_t)K;
    ht.ne[1] = (uint32_t)M;
    const size_t nbytes = type_nbytes(ht.type, ht.nel());
    if (!nbytes) return false;
    ht.data.assign((const uint8_t *)W, (const uint8_t *)W + nbytes);
    DeviceModel dm;
    DMat dmat{};
    bool ok = upload_mat(dm, &ht, dmat, false, false);
    DevBufs b;
    ActBuf a;
    float * dx = (float *)b.alloc((size_t)T * K * 4);
    float * dy = (float *)b.alloc((size_t)T * M * 4);
    ok = ok && dx && dy && make_act(b, act_fmt_for(wtype), T, K, a);
    a.tiled = mfma ? 1 : 0;  // the GEMM reads token tiles, k_mm row-major blocks
    ok = ok && hipMemcpy(dx, x, (size_t)T * K * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && launch_act_from_f32(nullptr, dx, T, K, a);
    if (ok) {
        MMGroup g;
        memset(&g, 0, sizeof(g));
        g.n = 1;
        g.T = T;
        g.e[0].W = dmat;
        g.e[0].in = a;
        g.e[0].y = dy;
        g.e[0].ldy = M;
        g.e[0].epi = EPI_STORE;
        g.split = split;
        g.fmm = 1;  // the f32-MFMA form for float weights whenever it applies (T >= 16)
        g.part_floats = (size_t)8 * T * M;
        g.part = (float *)b.alloc(g.part_floats * 4);
        ok = g.part != nullptr;
        if (mfma) {
            g.m2_floats = (size_t)T * M;
            g.m2 = (float *)b.alloc(g.m2_floats * 4);
            ok = ok && g.m2 != nullptr;
        }
        ok = ok && (mfma ? launch_qgemm(nullptr, g, wtype) : launch_mm_group(nullptr, g, wtype));
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    ok = ok && hipMemcpy(y, dy, (size_t)T * M * 4, hipMemcpyDeviceToHost) == hipSuccess;
    free_model(dm);
    return ok;
}

extern "C" RWKV_API bool rwkv_mi355x_selftest_matmul(int wtype, const void * W, int K, int M, const float * x, int T,
                                                     float * y) {
    return selftest_mm(wtype, W, K, M, x, T, y, false, 1);  // unsplit (the float matmuls' reference form)
}

extern "C" RWKV_API bool rwkv_mi355x_selftest_gemm(int wtype, const void * W, int K, int M, const float * x, int T,
                                                   float * y) {
    if (!wtype_quantized(wtype) || T < 2) return false;
    return selftest_mm(wtype, W, K, M, x, T, y, true);
}

// The same with the split-K form chosen: 1 = unsplit, 4 / 8 = that many class subtrees + combine
// (quantized: the int8-MFMA GEMM; F16 / F32 over 16+ tokens, K >= 512: k_fmm).
extern "C" RWKV_API bool rwkv_mi355x_selftest_gemm_split(int wtype, const void * W, int K, int M, const float * x,
                                                         int T, float * y, int split) {
    if (split != 1 && split != 2 && split != 4 && split != 8) return false;
    if (wtype_quantized(wtype)) return T >= 2 && selftest_mm(wtype, W, K, M, x, T, y, true, split);
    return (wtype == W_F16 || wtype == W_F32) && T >= 16 && K >= 512 && selftest_mm(wtype, W, K, M, x, T, y, false, split);
}

// `fused` sits in the former padding in front of y: the layout older callers were built against holds
static_assert(sizeof(rwkv_mi355x_selftest_mm_entry) == 104 && offsetof(rwkv_mi355x_selftest_mm_entry, y) == 64 &&
                  offsetof(rwkv_mi355x_selftest_mm_entry, fused) == 60,
              "rwkv_mi355x_selftest_mm_entry layout");

// A whole MMGroup on host operands through one launcher (include/rwkv_mi355x.h has the contract):
// every entry its own weights, epilogue, epilogue operands and emission, one input shared by all.
extern "C" RWKV_API bool rwkv_mi355x_selftest_matmul_group(int form, int split, int T, int K, const float * x, int n,
                                                           struct rwkv_mi355x_selftest_mm_entry * ent, int * launched) {
    if (!launched) return false;
    *launched = 0;
    if (form < 0 || form > 3 || (split != 0 && split != 1 && split != 4 && split != 8)) return false;
    if (T <= 0 || K <= 0 || K % 32 || !x || n < 1 || n > MM_MAX_ENTRIES || !ent) return false;
    const int wtype = ent[0].wtype;
    if (form == 2 && (!wtype_quantized(wtype) || T < 2)) return false;
    size_t msum = 0;
    for (int i = 0; i < n; i++) {
        const rwkv_mi355x_selftest_mm_entry & s = ent[i];
        if (!s.W || s.M <= 0 || !s.y || s.epi < EPI_STORE || s.epi > EPI_VMIX7) return false;
        // the operands an epilogue dereferences must be there
        if ((s.epi == EPI_SIGMUL_ADD || s.epi == EPI_VMIX7) && !s.aux) return false;
        if ((s.epi == EPI_DECAY6 || s.epi == EPI_DECAY7 || s.epi == EPI_SIGMOID_BIAS || s.epi == EPI_VMIX7) && !s.bias)
            return false;
        // the GEMM emits token tiles or nothing (launch_qgemm's fuse_emit; else the pass is its caller's)
        if (s.emit && form == 2 && !s.out_tiled) return false;
        msum += (size_t)s.M;
    }
    DeviceModel dm;
    DevBufs b;
    ActBuf a;
    float * dx = (float *)b.alloc((size_t)T * K * 4);
    bool ok = dx && make_act(b, act_fmt_for(wtype), T, K, a);
    a.tiled = form == 2 ? 1 : 0;  // the GEMM reads token tiles, the other forms row-major blocks
    ok = ok && hipMemcpy(dx, x, (size_t)T * K * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && launch_act_from_f32(nullptr, dx, T, K, a);
    MMGroup g;
    memset(&g, 0, sizeof(g));
    g.n = n;
    g.T = T;
    g.split = split;
    g.fmm = 1;  // as selftest_mm: the f32-MFMA form for float weights from T = 16
    for (int i = 0; ok && i < n; i++) {
        const rwkv_mi355x_selftest_mm_entry & s = ent[i];
        const size_t TM = (size_t)T * s.M;
        HostTensor ht;
        ht.name = "selftest";
        ht.type = (uint32_t)s.wtype;
        ht.ndim = 2;
        ht.ne[0] = (uint32_t)K;
        ht.ne[1] = (uint32_t)s.M;
        const size_t nbytes = type_nbytes(ht.type, ht.nel());
        if (!nbytes) {
            ok = false;
            break;
        }
        ht.data.assign((const uint8_t *)s.W, (const uint8_t *)s.W + nbytes);
        MMEntry & e = g.e[i];
        ok = upload_mat(dm, &ht, e.W, false, false);
        // a host array on the device (NULL stays NULL)
        auto up = [&](const float * h, size_t count) -> float * {
            if (!h) return nullptr;
            float * d = (float *)b.alloc(count * 4);
            ok = ok && d && hipMemcpy(d, h, count * 4, hipMemcpyHostToDevice) == hipSuccess;
            return d;
        };
        e.in = a;
        // form 2: y starts as the caller's s.y (a fused entry must leave it alone)
        e.y = s.y0 ? up(s.y0, TM) : form == 2 ? up(s.y, TM) : (float *)b.alloc(TM * 4);
        e.ldy = s.M;
        e.aux = up(s.aux, TM);
        e.bias = up(s.bias, (size_t)s.M);
        e.epi = s.epi;
        e.emit = s.emit ? 1 : 0;
        ok = ok && e.y;
        if (s.emit) {
            ok = ok && make_act(b, s.out_q8_1 ? A_Q8_1 : A_Q8_0, T, s.M, e.out);
            e.out.tiled = s.out_tiled ? 1 : 0;
            // form 2 returns the records: poisoned, so a record nobody wrote shows
            if (form == 2 && ok)
                ok = hipMemset(e.out.tq, 0xA5, ((size_t)T + QG_TOK - 1) / QG_TOK * (s.M / 32) * qg_a_bytes(true)) ==
                     hipSuccess;
        }
    }
    if (ok) {
        g.part_floats = (size_t)8 * T * msum;
        g.part = (float *)b.alloc(g.part_floats * 4);
        ok = g.part != nullptr;
        if (form == 2) {
            g.m2_floats = (size_t)T * msum;
            g.m2 = (float *)b.alloc(g.m2_floats * 4);
            ok = ok && g.m2 != nullptr;
        }
    }
    bool ran = true;
    if (ok) {
        switch (form) {
            case 0: ok = launch_mm_group(nullptr, g, wtype); break;
            case 1: ok = launch_mvb_group(nullptr, g, wtype, &ran); break;
            case 2: ok = launch_qgemm(nullptr, g, wtype); break;
            default: ok = launch_fmm_group(nullptr, g, wtype, &ran); break;
        }
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    for (int i = 0; ok && ran && i < n; i++) {
        rwkv_mi355x_selftest_mm_entry & s = ent[i];
        const MMEntry & e = g.e[i];
        const size_t TM = (size_t)T * s.M, nb = TM / 32;
        ok = hipMemcpy(s.y, e.y, TM * 4, hipMemcpyDeviceToHost) == hipSuccess;
        s.fused = form == 2 ? e.fuse_emit : 0;
        if (ok && s.fused) ok = detile_act(e.out, T, s.M, s.q, s.d, s.out_q8_1 ? s.s : nullptr, s.qsum);
        if (!s.emit || s.out_tiled) continue;
        if (s.q) ok = ok && hipMemcpy(s.q, e.out.q, TM, hipMemcpyDeviceToHost) == hipSuccess;
        if (s.d) ok = ok && hipMemcpy(s.d, e.out.d, nb * 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (s.s && s.out_q8_1) ok = ok && hipMemcpy(s.s, e.out.s, nb * 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (s.qsum) ok = ok && hipMemcpy(s.qsum, e.out.qsum, nb * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    free_model(dm);
    *launched = ok && ran ? 1 : 0;
    return ok;
}

namespace {

// n bytes of 0xA5 on the device: an output nobody has written yet
void * alloc_poison(DevBufs & b, size_t n) {
    void * p = b.alloc(n);
    return p && hipMemset(p, 0xA5, n) == hipSuccess ? p : nullptr;
}

// one poisoned output row of K elements in format fmt
bool make_act_poison(DevBufs & b, int fmt, int K, ActBuf & a) {
    if (!make_act(b, fmt, 1, K, a)) return false;
    const size_t nb = (size_t)K / 32 + 1;
    return hipMemset(a.q, 0xA5, (size_t)K) == hipSuccess && hipMemset(a.d, 0xA5, nb * 4) == hipSuccess &&
           hipMemset(a.s, 0xA5, nb * 4) == hipSuccess && hipMemset(a.qsum, 0xA5, nb * 4) == hipSuccess;
}

bool act_down(const ActBuf & a, int K, int8_t * q, float * d, float * s, int32_t * qsum) {
    const size_t nb = (size_t)K / 32;
    return (!q || hipMemcpy(q, a.q, (size_t)K, hipMemcpyDeviceToHost) == hipSuccess) &&
           (!d || hipMemcpy(d, a.d, nb * 4, hipMemcpyDeviceToHost) == hipSuccess) &&
           (!s || hipMemcpy(s, a.s, nb * 4, hipMemcpyDeviceToHost) == hipSuccess) &&
           (!qsum || hipMemcpy(qsum, a.qsum, nb * 4, hipMemcpyDeviceToHost) == hipSuccess);
}

bool upload_w(DeviceModel & dm, int wtype, const void * W, int K, int M, DMat & out) {
    HostTensor ht;
    ht.name = "selftest";
    ht.type = (uint32_t)wtype;
    ht.ndim = 2;
    ht.ne[0] = (uint32_t)K;
    ht.ne[1] = (uint32_t)M;
    const size_t nbytes = type_nbytes(ht.type, ht.nel());
    if (!nbytes) return false;
    ht.data.assign((const uint8_t *)W, (const uint8_t *)W + nbytes);
    return upload_mat(dm, &ht, out, false, false);
}

float * up_floats(DevBufs & b, const float * h, size_t count, bool & ok) {
    if (!h) return nullptr;
    float * d = (float *)b.alloc(count * 4);
    ok = ok && d && hipMemcpy(d, h, count * 4, hipMemcpyHostToDevice) == hipSuccess;
    return d;
}

// x [K] quantized on the device into wtype's activation format (a decode matvec's SRC_ACT input)
bool act_row(DevBufs & b, int wtype, const float * x, int K, ActBuf & a) {
    bool ok = true;
    float * dx = up_floats(b, x, (size_t)K, ok);
    return ok && make_act(b, act_fmt_for(wtype), 1, K, a) && launch_act_from_f32(nullptr, dx, 1, K, a);
}

// the compute units launch_mv_group's thresholds count: the device's, as the engine sets them
int mv_device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 0;
    set_mv_device_cus(cus);
    return kQgCUs;
}

}  // namespace

// One MVGroup on host operands through launch_mv_group (include/rwkv_mi355x.h has the contract).  The
// shapes the launcher declines come back as *launched = 0: they are refused on the host, before a launch.
extern "C" RWKV_API bool rwkv_mi355x_selftest_mv_group(int n, const struct rwkv_mi355x_selftest_mv_entry * ent,
                                                       struct rwkv_mi355x_selftest_mv_shape * shape, int * launched) {
    if (!launched) return false;
    *launched = 0;
    if (n < 1 || n > MM_MAX_ENTRIES || !ent || !shape) return false;
    for (int i = 0; i < n; i++) {
        const rwkv_mi355x_selftest_mv_entry & s = ent[i];
        if (!s.W || s.M <= 0 || s.K < 8 || !s.x || !s.y || s.src < SRC_ACT || s.src > SRC_LNMIX) return false;
        if (s.epi < EPI_STORE || s.epi > EPI_VMIX7 || s.form < 0 || s.form > 2) return false;
        if ((s.epi == EPI_SIGMUL_ADD || s.epi == EPI_VMIX7) && !s.aux) return false;
        if ((s.epi == EPI_DECAY6 || s.epi == EPI_DECAY7 || s.epi == EPI_SIGMOID_BIAS || s.epi == EPI_VMIX7) && !s.bias)
            return false;
        if (s.src == SRC_LNMIX && (!s.lnw || !s.lnb || (s.form != 2 && (!s.carry || !s.mu)))) return false;
        if (s.mu2 && (s.src != SRC_LNMIX || s.form == 2 || !wtype_quantized(s.wtype))) return false;
    }
    const int cus = mv_device_cus();
    if (cus <= 0) return false;
    DeviceModel dm;
    DevBufs b;
    MVGroup g;
    memset(&g, 0, sizeof(g));
    g.n = n;
    bool ok = true;
    for (int i = 0; ok && i < n; i++) {
        const rwkv_mi355x_selftest_mv_entry & s = ent[i];
        MVEntry & e = g.e[i];
        const size_t K = (size_t)s.K, M = (size_t)s.M;
        ok = upload_w(dm, s.wtype, s.W, s.K, s.M, e.W);
        e.src = s.src;
        e.form = s.form;
        if (s.src == SRC_ACT) {
            // entries of one format, K and x share their activation row
            int j = 0;
            while (j < i && !(ent[j].src == SRC_ACT && ent[j].K == s.K && ent[j].x == s.x &&
                              act_fmt_for(ent[j].wtype) == act_fmt_for(s.wtype)))
                j++;
            if (j < i) e.act = g.e[j].act;
            else ok = ok && act_row(b, s.wtype, s.x, s.K, e.act);
        } else if (s.src == SRC_F32) {
            e.f = up_floats(b, s.x, K, ok);
        } else {
            e.x = up_floats(b, s.x, K, ok);
            e.lnw = up_floats(b, s.lnw, K, ok);
            e.lnb = up_floats(b, s.lnb, K, ok);
            e.carry = up_floats(b, s.carry, K, ok);
            e.mu = up_floats(b, s.mu, K, ok);
            e.mu2 = up_floats(b, s.mu2, K, ok);
            if (s.carry_out) ok = ok && (e.carry_out = (float *)alloc_poison(b, K * 4)) != nullptr;
            if (s.mu2) ok = ok && make_act_poison(b, act_fmt_for(s.wtype), s.K, e.act2_out);
        }
        e.y = s.y0 ? up_floats(b, s.y0, M, ok) : (float *)alloc_poison(b, M * 4);
        e.aux = up_floats(b, s.aux, M, ok);
        e.bias = up_floats(b, s.bias, M, ok);
        e.epi = s.epi;
        e.emit = s.emit ? 1 : 0;
        ok = ok && e.y;
        if (s.emit) ok = ok && make_act_poison(b, s.out_q8_1 ? A_Q8_1 : A_Q8_0, s.M, e.act_out);
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    const bool ran = ok && launch_mv_group(nullptr, g);
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    for (int i = 0; ok && ran && i < n; i++) {
        const rwkv_mi355x_selftest_mv_entry & s = ent[i];
        const MVEntry & e = g.e[i];
        ok = hipMemcpy(s.y, e.y, (size_t)s.M * 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (s.emit) ok = ok && act_down(e.act_out, s.M, s.q, s.d, s.s, s.qsum);
        if (e.carry_out) ok = ok && hipMemcpy(s.carry_out, e.carry_out, (size_t)s.K * 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (e.mu2) ok = ok && act_down(e.act2_out, s.K, s.q2, s.d2, s.s2, s.qsum2);
    }
    free_model(dm);
    if (ok && ran) {
        shape->rows = g.rows;
        shape->grid = g.grid;
        shape->stride = g.stride;
        shape->units_max = g.units_max;
        shape->cus = cus;
        *launched = 1;
    }
    return ok;
}

// launch_mv_sigmul (k_mvsig) on host operands: the value matvec Wv k with the receptance Wr xr as its
// EPI_SIGMUL_ADD gate, one launch.
extern "C" RWKV_API bool rwkv_mi355x_selftest_mv_sigmul(int wtype_v, const void * Wv, int Mv, int F, const float * k,
                                                        int wtype_r, const void * Wr, int Mr, int C, const float * xr,
                                                        const float * y0, float * y, int * launched) {
    if (!launched) return false;
    *launched = 0;
    if (!Wv || !Wr || !k || !xr || !y0 || !y || Mv <= 0 || Mr <= 0 || F <= 0 || C <= 0 || F % 32 || C % 32) return false;
    DeviceModel dm;
    DevBufs b;
    MVEntry ev, er;
    memset(&ev, 0, sizeof(ev));
    memset(&er, 0, sizeof(er));
    bool ok = upload_w(dm, wtype_v, Wv, F, Mv, ev.W) && upload_w(dm, wtype_r, Wr, C, Mr, er.W);
    ev.src = er.src = SRC_ACT;
    ok = ok && act_row(b, wtype_v, k, F, ev.act) && act_row(b, wtype_r, xr, C, er.act);
    ev.y = up_floats(b, y0, (size_t)Mv, ok);
    ev.epi = EPI_SIGMUL_ADD;
    er.epi = EPI_STORE;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    const bool ran = ok && mv_sigmul_supported(ev, er) && launch_mv_sigmul(nullptr, ev, er);
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (ok && ran) ok = hipMemcpy(y, ev.y, (size_t)Mv * 4, hipMemcpyDeviceToHost) == hipSuccess;
    free_model(dm);
    *launched = ok && ran ? 1 : 0;
    return ok;
}

// WKV-6 (v5 / v6) over T tokens of one context: chunked = 0 the serial k_wkv6_s64 (decode's
// association), 1 the chunk-parallel form (wkv_chunk.hip).  k, v, r, w: [T][H*64] (w: [H*64] when
// w_per_token = 0); u: [H*64]; state_in / state_out: [H][64][64]; y: [T][H*64]; all host.
extern "C" RWKV_API bool rwkv_mi355x_selftest_wkv6(int T, int H, int chunked, int w_per_token, const float * k,
                                                  const float * v, const float * r, const float * u, const float * w,
                                                  const float * state_in, float * state_out, float * y) {
    if (T < 1 || H < 1 || !k || !v || !r || !u || !w || !state_in || !state_out || !y) return false;
    if (chunked && !wkv6_chunked_supported(T, 64, 0)) return false;
    const size_t C = (size_t)H * 64, TC = (size_t)T * C, SN = C * 64, WN = w_per_token ? TC : C;
    DevBufs b;
    float *dk = (float *)b.alloc(TC * 4), *dv = (float *)b.alloc(TC * 4), *dr = (float *)b.alloc(TC * 4),
          *du = (float *)b.alloc(C * 4), *dw = (float *)b.alloc(WN * 4), *dsi = (float *)b.alloc(SN * 4),
          *dso = (float *)b.alloc(SN * 4), *dy = (float *)b.alloc(TC * 4), *ra = (float *)b.alloc(TC * 4),
          *kb = (float *)b.alloc(TC * 4), *sc = (float *)b.alloc(wkv6_chunked_scratch_floats(T, H) * 4);
    if (!dk || !dv || !dr || !du || !dw || !dsi || !dso || !dy || !ra || !kb || !sc) return false;
    const std::pair<float *, const float *> up[] = {{dk, k}, {dv, v}, {dr, r}, {dy, y}};
    for (const auto & p : up)
        if (hipMemcpy(p.first, p.second, TC * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    if (hipMemcpy(du, u, C * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dw, w, WN * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dsi, state_in, SN * 4, hipMemcpyHostToDevice) != hipSuccess)
        return false;
    const bool ok = chunked ? launch_wkv6_chunked(nullptr, T, H, dk, dv, dr, du, dw, w_per_token, dsi, dso, dy, ra, kb, sc)
                            : launch_wkv6(nullptr, T, H, 64, dk, dv, dr, du, dw, w_per_token, dsi, dso, dy);
    if (!ok || hipDeviceSynchronize() != hipSuccess) return false;
    return hipMemcpy(y, dy, TC * 4, hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(state_out, dso, SN * 4, hipMemcpyDeviceToHost) == hipSuccess;
}

// WKV-7 over T tokens of one context: chunked = 0 the serial k_wkv7_s64 (decode's association), 1 the
// chunk-parallel form (wkv7_chunk.hip).  r, w, k, v, a, b: [T][H*64]; state_in / state_out:
// [H][64 value rows][64 key columns]; y: [T][H*64]; all host.
extern "C" RWKV_API bool rwkv_mi355x_selftest_wkv7(int T, int H, int chunked, const float * r, const float * w,
                                                  const float * k, const float * v, const float * a, const float * b,
                                                  const float * state_in, float * state_out, float * y) {
    if (T < 1 || H < 1 || !r || !w || !k || !v || !a || !b || !state_in || !state_out || !y) return false;
    if (chunked && !wkv7_chunked_supported(T, 64, 0)) return false;
    const size_t C = (size_t)H * 64, TC = (size_t)T * C, SN = C * 64;
    DevBufs bf;
    float *dr = (float *)bf.alloc(TC * 4), *dw = (float *)bf.alloc(TC * 4), *dk = (float *)bf.alloc(TC * 4),
          *dv = (float *)bf.alloc(TC * 4), *da = (float *)bf.alloc(TC * 4), *db = (float *)bf.alloc(TC * 4),
          *dsi = (float *)bf.alloc(SN * 4), *dso = (float *)bf.alloc(SN * 4), *dy = (float *)bf.alloc(TC * 4),
          *sc = chunked ? (float *)bf.alloc(wkv7_chunked_scratch_floats(T, H) * 4) : nullptr;
    if (!dr || !dw || !dk || !dv || !da || !db || !dsi || !dso || !dy || (chunked && !sc)) return false;
    const std::pair<float *, const float *> up[] = {{dr, r}, {dw, w}, {dk, k}, {dv, v}, {da, a}, {db, b}, {dy, y}};
    for (const auto & p : up)
        if (hipMemcpy(p.first, p.second, TC * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    if (hipMemcpy(dsi, state_in, SN * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    const bool ok = chunked ? launch_wkv7_chunked(nullptr, T, H, dr, dw, dk, dv, da, db, dsi, dso, dy, sc)
                            : launch_wkv7(nullptr, T, H, 64, dr, dw, dk, dv, da, db, dsi, dso, dy);
    if (!ok || hipDeviceSynchronize() != hipSuccess) return false;
    return hipMemcpy(y, dy, TC * 4, hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(state_out, dso, SN * 4, hipMemcpyDeviceToHost) == hipSuccess;
}

// The token layouts of the serial WKV kernels (wkv_span.hpp) against each other, on operands drawn
// here from the seed (include/rwkv_mi355x.h has the contract).  Every form's outputs start as a
// poison word of its own, so a row or a state word that nobody wrote counts as a difference.
extern "C" RWKV_API bool rwkv_mi355x_selftest_wkv_layouts(int kind, int H, int S, const uint32_t * lens, int n_seg,
                                                         uint64_t seed, uint64_t * out) {
    if (kind < 4 || kind > 7 || H < 1 || S < 1 || !lens || n_seg < 1 || !out) return false;
    const size_t C = (size_t)H * S;
    // state floats per segment, and the slice of it the kernel writes (WKV-4: aa, bb, pp of the
    // layer's five rows)
    const size_t SL = kind == 4 ? 5 * C : C * S, S0 = kind == 4 ? 2 * C : 0, SW = SL - S0;
    std::vector<uint32_t> begin(n_seg), seg_of;
    std::vector<uint64_t> soff(n_seg);
    bool ones = true;
    for (int s = 0; s < n_seg; s++) {
        if (lens[s] < 1 || lens[s] > 4096) return false;
        begin[s] = (uint32_t)seg_of.size();
        soff[s] = (uint64_t)s * SL;
        seg_of.insert(seg_of.end(), lens[s], (uint32_t)s);
        ones = ones && lens[s] == 1;
    }
    const size_t T = seg_of.size(), TC = T * C, NS = (size_t)n_seg * SL;
    DevBufs bf;
    bool ok = true;
    uint64_t ctr = 0;
    // n floats lo + span * u, u the seed's next uniform draws, on the device
    auto draw = [&](size_t n, float lo, float span) -> float * {
        std::vector<float> h(n);
        for (float & x : h) x = lo + span * sample_uniform(seed, ctr++);
        float * d = (float *)bf.alloc(n * 4);
        ok = ok && d && hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice) == hipSuccess;
        return d;
    };
    auto up = [&](const void * h, size_t bytes) -> void * {
        void * d = bf.alloc(bytes);
        ok = ok && d && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
        return d;
    };
    // operands: k, v, r (and v7's a, b) in [-0.5, 0.5); WKV-6 / WKV-7 decays in [0.9, 1); WKV-4's
    // decay is the log-space rate the models store negative, in (-1, -0.9]
    const float * k = draw(TC, -0.5f, 1.0f), * v = draw(TC, -0.5f, 1.0f), * r = draw(TC, -0.5f, 1.0f);
    const float * a = kind == 7 ? draw(TC, -0.5f, 1.0f) : nullptr, * b = kind == 7 ? draw(TC, -0.5f, 1.0f) : nullptr;
    const float * w = kind == 4 ? draw(C, -0.9f, -0.1f) : draw(kind == 5 ? C : TC, 0.9f, 0.1f);
    const float * u = kind == 7 ? nullptr : draw(C, -0.5f, 1.0f);  // WKV-4: time_first
    // input states in [-0.5, 0.5); WKV-4: aa so, bb in [0.5, 1.5), pp = 0
    std::vector<float> hs(NS);
    for (float & x : hs) x = sample_uniform(seed, ctr++) - 0.5f;
    if (kind == 4)
        for (int s = 0; s < n_seg; s++)
            for (size_t c = 0; c < C; c++) hs[s * SL + 3 * C + c] += 1.0f, hs[s * SL + 4 * C + c] = 0.0f;
    const float * sin = (const float *)up(hs.data(), NS * 4);
    SegTab sg;
    sg.n = n_seg;
    sg.begin = (const uint32_t *)up(begin.data(), (size_t)n_seg * 4);
    sg.len = (const uint32_t *)up(lens, (size_t)n_seg * 4);
    sg.sin_off = sg.sout_off = (const uint64_t *)up(soff.data(), (size_t)n_seg * 8);
    sg.seg_of = (const uint32_t *)up(seg_of.data(), T * 4);
    // outputs of the forms: 0 one launch per segment, 1 the segmented launch, 2 the contexts
    float * y[3], * so[3];
    const int poison[3] = {0xA5, 0x5A, 0xC3};
    for (int f = 0; f < 3; f++) {
        y[f] = (float *)bf.alloc(TC * 4);
        so[f] = (float *)bf.alloc(NS * 4);
        ok = ok && y[f] && so[f] && hipMemset(y[f], poison[f], TC * 4) == hipSuccess &&
             hipMemset(so[f], poison[f], NS * 4) == hipSuccess;
    }
    if (!ok) return false;
    // one launch: n tokens from row `row`, states at float offset `st`, into form f's outputs
    auto run = [&](int f, int n, size_t row, size_t st, int bs, const SegTab * seg) {
        const size_t o = row * C;
        if (kind == 4) {
            ActBuf ob;
            memset(&ob, 0, sizeof(ob));
            ob.fmt = A_F32;
            ob.K = (int)C;
            ob.f = y[f] + o;
            return launch_wkv4(nullptr, n, (int)C, r + o, k + o, v + o, u, w, sin + st, so[f] + st, ob, bs, seg);
        }
        if (kind == 7) return launch_wkv7(nullptr, n, H, S, r + o, w + o, k + o, v + o, a + o, b + o, sin + st, so[f] + st, y[f] + o, seg);
        return launch_wkv6(nullptr, n, H, S, k + o, v + o, r + o, u, kind == 6 ? w + o : w, kind == 6, sin + st, so[f] + st, y[f] + o, seg);
    };
    for (int s = 0; s < n_seg; s++)
        if (!run(0, (int)lens[s], begin[s], (size_t)s * SL, 0, nullptr)) return false;
    if (!run(1, (int)T, 0, 0, 0, &sg)) return false;
    const bool ctx = kind == 4 && ones;
    if (ctx && !run(2, (int)T, 0, 0, (int)SL, nullptr)) return false;
    if (hipDeviceSynchronize() != hipSuccess) return false;
    std::vector<uint32_t> hy[3], hso[3];
    for (int f = 0; f < 3; f++) {
        hy[f].resize(TC), hso[f].resize(NS);
        if (hipMemcpy(hy[f].data(), y[f], TC * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hso[f].data(), so[f], NS * 4, hipMemcpyDeviceToHost) != hipSuccess)
            return false;
    }
    for (int f = 1; f < 3; f++) {
        uint64_t dy = 0, ds = 0;
        for (size_t i = 0; i < TC; i++) dy += hy[f][i] != hy[0][i];
        for (int s = 0; s < n_seg; s++)
            for (size_t i = S0; i < SL; i++) ds += hso[f][s * SL + i] != hso[0][s * SL + i];
        const bool ran = f == 1 || ctx;
        out[2 * (f - 1)] = ran ? dy : 0;
        out[2 * (f - 1) + 1] = ran ? ds : 0;
        out[3 + f] = ran ? TC + (uint64_t)n_seg * SW : 0;
    }
    return true;
}

// The host arrays of a self-test with log-probabilities (NULL: the plain self-test): device copies,
// uploaded before the launches and downloaded after them
struct SelftestLogprobs {
    uint32_t top_k;
    double * token_logprob;
    uint32_t * top_ids;
    double * top_logprobs;
    bool ok(int V) const {
        return top_k <= (uint32_t)LOGPROBS_MAX_TOP && top_k <= (uint32_t)V && token_logprob && top_ids && top_logprobs;
    }
    bool up(DevBufs & b, int rows, SampleArgs & a) const {
        const size_t R = (size_t)rows, T = R * top_k;
        a.lp_logz = (double *)b.alloc(R * 8);
        a.lp_token = (double *)b.alloc(R * 8);
        a.lp_top_ids = (uint32_t *)b.alloc(T * 4 + 4);
        a.lp_top = (double *)b.alloc(T * 8 + 8);
        a.lp_k = (int)top_k;
        return a.lp_logz && a.lp_token && a.lp_top_ids && a.lp_top &&
               hipMemcpy(a.lp_token, token_logprob, R * 8, hipMemcpyHostToDevice) == hipSuccess &&
               (!T || (hipMemcpy(a.lp_top_ids, top_ids, T * 4, hipMemcpyHostToDevice) == hipSuccess &&
                       hipMemcpy(a.lp_top, top_logprobs, T * 8, hipMemcpyHostToDevice) == hipSuccess));
    }
    bool down(int rows, const SampleArgs & a) const {
        const size_t R = (size_t)rows, T = R * top_k;
        return hipMemcpy(token_logprob, a.lp_token, R * 8, hipMemcpyDeviceToHost) == hipSuccess &&
               (!T || (hipMemcpy(top_ids, a.lp_top_ids, T * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                       hipMemcpy(top_logprobs, a.lp_top, T * 8, hipMemcpyDeviceToHost) == hipSuccess));
    }
};

// The sampler kernel (sample.hip) on host logits with the uniform draws given: what
// rwkv_mi355x_sample / _generate launch, one workgroup per row.
static bool selftest_sample(const float * logits, int rows, int V, const struct rwkv_mi355x_sampling * p, const float * u,
                            uint32_t * tokens, uint32_t * kept, float * cutoff, const SelftestLogprobs * lp) {
    if (!logits || !p || !u || !tokens || rows < 1 || V < 1 || V > SAMPLE_MAX_VOCAB || (lp && !lp->ok(V))) return false;
    if (!(p->temperature >= 0.0f) || !(p->top_p >= 0.0f && p->top_p <= 1.0f) || p->n_bias > (uint32_t)SAMPLE_MAX_BIAS)
        return false;
    if (p->n_bias && (!p->bias_ids || !p->bias_values)) return false;
    for (uint32_t i = 0; i < p->n_bias; i++)
        if (p->bias_ids[i] >= (uint32_t)V) return false;
    const size_t n = (size_t)rows * V;
    DevBufs b;
    SampleArgs a;
    memset(&a, 0, sizeof(a));
    float * dl = (float *)b.alloc(n * 4);
    float * du = (float *)b.alloc((size_t)rows * 4);
    uint32_t * bi = (uint32_t *)b.alloc(SAMPLE_MAX_BIAS * 4);
    float * bv = (float *)b.alloc(SAMPLE_MAX_BIAS * 4);
    a.tok = (uint32_t *)b.alloc((size_t)rows * 4);
    a.kept = (uint32_t *)b.alloc((size_t)rows * 4);
    a.cutoff = (float *)b.alloc((size_t)rows * 4);
    if (!dl || !du || !bi || !bv || !a.tok || !a.kept || !a.cutoff) return false;
    if (hipMemcpy(dl, logits, n * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(du, u, (size_t)rows * 4, hipMemcpyHostToDevice) != hipSuccess)
        return false;
    if (p->n_bias && (hipMemcpy(bi, p->bias_ids, p->n_bias * 4, hipMemcpyHostToDevice) != hipSuccess ||
                      hipMemcpy(bv, p->bias_values, p->n_bias * 4, hipMemcpyHostToDevice) != hipSuccess))
        return false;
    a.logits = dl;
    a.rows = rows;
    a.V = V;
    a.temperature = p->temperature;
    a.top_p = p->top_p;
    a.n_bias = (int)p->n_bias;
    a.bias_ids = bi;
    a.bias_vals = bv;
    a.u = du;
    if (lp && (!lp->up(b, rows, a) || !launch_logprobs(nullptr, a))) return false;
    if (!launch_sample(nullptr, a) || hipDeviceSynchronize() != hipSuccess) return false;
    if (hipMemcpy(tokens, a.tok, (size_t)rows * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (kept && hipMemcpy(kept, a.kept, (size_t)rows * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (cutoff && hipMemcpy(cutoff, a.cutoff, (size_t)rows * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    return !lp || lp->down(rows, a);
}

extern "C" RWKV_API bool rwkv_mi355x_selftest_sample(const float * logits, int rows, int V,
                                                    const struct rwkv_mi355x_sampling * p, const float * u,
                                                    uint32_t * tokens, uint32_t * kept, float * cutoff) {
    return selftest_sample(logits, rows, V, p, u, tokens, kept, cutoff, nullptr);
}

extern "C" RWKV_API bool rwkv_mi355x_selftest_sample_logprobs(const float * logits, int rows, int V,
                                                             const struct rwkv_mi355x_sampling * p, const float * u,
                                                             uint32_t * tokens, uint32_t * kept, float * cutoff,
                                                             uint32_t top_k, double * token_logprob, uint32_t * top_ids,
                                                             double * top_logprobs) {
    const SelftestLogprobs lp{top_k, token_logprob, top_ids, top_logprobs};
    return selftest_sample(logits, rows, V, p, u, tokens, kept, cutoff, &lp);
}

// The batched sampler kernel (sample.hip, k_sample_rows) on host operands: what
// rwkv_mi355x_generate_batch launches per step, with the uniform draws given.
static bool selftest_sample_rows(const float * logits, int rows, int V, const struct rwkv_mi355x_batch_sampling * p,
                                 const float * u, uint32_t step, uint32_t * counts, uint32_t * done, uint32_t * tokens,
                                 uint32_t * decode_tokens, uint32_t * kept, float * cutoff, uint32_t * lengths,
                                 uint32_t * active, const SelftestLogprobs * lp) {
    if (!logits || !p || !u || !done || !tokens || !decode_tokens || !kept || !cutoff || !lengths || !active) return false;
    if (lp && (V < 1 || !lp->ok(V))) return false;
    if (rows < 1 || V < 1 || V > SAMPLE_MAX_VOCAB || !p->temperature || !p->top_p) return false;
    if (p->n_bias > (uint32_t)SAMPLE_MAX_BIAS || (p->n_bias && (!p->bias_ids || !p->bias_values))) return false;
    if (p->n_stop > (uint32_t)SAMPLE_MAX_STOP || (p->n_stop && !p->stop_tokens)) return false;
    for (int r = 0; r < rows; r++)
        if (!(p->temperature[r] >= 0.0f) || !(p->top_p[r] >= 0.0f && p->top_p[r] <= 1.0f)) return false;
    for (uint32_t i = 0; i < p->n_bias; i++)
        if (p->bias_ids[i] >= (uint32_t)V) return false;
    for (uint32_t i = 0; i < p->n_stop; i++)
        if (p->stop_tokens[i] >= (uint32_t)V) return false;
    const size_t n = (size_t)rows * V, R = (size_t)rows * 4;
    DevBufs b;
    SampleArgs a;
    memset(&a, 0, sizeof(a));
    // a device copy of a host array of `bytes` bytes (NULL stays NULL)
    bool ok = true;
    auto up = [&](const void * h, size_t bytes) -> void * {
        if (!h) return nullptr;
        void * d = b.alloc(bytes);
        ok = ok && d && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
        return d;
    };
    a.logits = (const float *)up(logits, n * 4);
    a.u = (const float *)up(u, R);
    a.temperature_r = (const float *)up(p->temperature, R);
    a.top_p_r = (const float *)up(p->top_p, R);
    a.presence_r = (const float *)up(p->presence, R);
    a.frequency_r = (const float *)up(p->frequency, R);
    a.counts = (uint32_t *)up(counts, n * 4);
    a.done = (uint32_t *)up(done, R);
    a.tok = (uint32_t *)up(tokens, R);
    a.tok2 = (uint32_t *)up(decode_tokens, R);
    a.kept = (uint32_t *)up(kept, R);
    a.cutoff = (float *)up(cutoff, R);
    a.length = (uint32_t *)up(lengths, R);
    a.active = (uint32_t *)up(active, 4);
    a.fin_step = (uint32_t *)b.alloc(R);
    a.bias_ids = (const uint32_t *)up(p->n_bias ? p->bias_ids : nullptr, p->n_bias * 4);
    a.bias_vals = (const float *)up(p->n_bias ? p->bias_values : nullptr, p->n_bias * 4);
    if (!ok || !a.fin_step) return false;
    a.rows = rows;
    a.V = V;
    a.n_bias = (int)p->n_bias;
    a.n_stop = (int)p->n_stop;
    for (uint32_t i = 0; i < p->n_stop; i++) a.stop[i] = p->stop_tokens[i];
    a.step = step;
    if (lp && (!lp->up(b, rows, a) || !launch_logprobs(nullptr, a))) return false;
    if (!launch_sample(nullptr, a) || hipDeviceSynchronize() != hipSuccess) return false;
    const std::pair<void *, const void *> down[] = {{done, a.done},     {tokens, a.tok},     {decode_tokens, a.tok2},
                                                    {kept, a.kept},     {cutoff, a.cutoff}, {lengths, a.length}};
    for (const auto & d : down)
        if (hipMemcpy(d.first, d.second, R, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (counts && hipMemcpy(counts, a.counts, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (lp && !lp->down(rows, a)) return false;
    return hipMemcpy(active, a.active, 4, hipMemcpyDeviceToHost) == hipSuccess;
}

extern "C" RWKV_API bool rwkv_mi355x_selftest_sample_rows(const float * logits, int rows, int V,
                                                         const struct rwkv_mi355x_batch_sampling * p, const float * u,
                                                         uint32_t step, uint32_t * counts, uint32_t * done,
                                                         uint32_t * tokens, uint32_t * decode_tokens, uint32_t * kept,
                                                         float * cutoff, uint32_t * lengths, uint32_t * active) {
    return selftest_sample_rows(logits, rows, V, p, u, step, counts, done, tokens, decode_tokens, kept, cutoff, lengths,
                                active, nullptr);
}

extern "C" RWKV_API bool rwkv_mi355x_selftest_sample_rows_logprobs(
    const float * logits, int rows, int V, const struct rwkv_mi355x_batch_sampling * p, const float * u, uint32_t step,
    uint32_t * counts, uint32_t * done, uint32_t * tokens, uint32_t * decode_tokens, uint32_t * kept, float * cutoff,
    uint32_t * lengths, uint32_t * active, uint32_t top_k, double * token_logprob, uint32_t * top_ids,
    double * top_logprobs) {
    const SelftestLogprobs lp{top_k, token_logprob, top_ids, top_logprobs};
    return selftest_sample_rows(logits, rows, V, p, u, step, counts, done, tokens, decode_tokens, kept, cutoff, lengths,
                                active, &lp);
}

// The queue's turnover kernel (sample.hip, k_gen_turnover) on host operands: what
// rwkv_mi355x_generate_queue launches before step `step`.  lane_seq [lanes], done / lane / start [Q],
// *next and *active are uploaded, updated and downloaded; length and max_tokens [Q] are read;
// retire_to and admit_from [lanes] are written.
extern "C" RWKV_API bool rwkv_mi355x_selftest_gen_turnover(int lanes, int Q, uint32_t step, uint32_t * lane_seq,
                                                          uint32_t * done, const uint32_t * length,
                                                          const uint32_t * max_tokens, uint32_t * lane, uint32_t * start,
                                                          uint32_t * next, uint32_t * active, uint32_t * retire_to,
                                                          uint32_t * admit_from) {
    if (lanes < 1 || lanes > 256 || Q < 1 || Q > 65536 || !lane_seq || !done || !length || !max_tokens || !lane || !start ||
        !next || !active || !retire_to || !admit_from || *next > (uint32_t)Q)
        return false;
    for (int r = 0; r < lanes; r++)
        if (lane_seq[r] != GEN_NONE && lane_seq[r] >= (uint32_t)Q) return false;
    const size_t LB = (size_t)lanes * 4, QB = (size_t)Q * 4;
    DevBufs b;
    bool ok = true;
    auto up = [&](const void * h, size_t bytes) -> uint32_t * {
        void * d = b.alloc(bytes);
        ok = ok && d && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
        return (uint32_t *)d;
    };
    GenQueue q;
    q.lanes = lanes;
    q.Q = Q;
    q.lane_seq = up(lane_seq, LB);
    q.done = up(done, QB);
    q.length = up(length, QB);
    q.max_tokens = up(max_tokens, QB);
    q.lane = up(lane, QB);
    q.start = up(start, QB);
    q.retire_to = up(retire_to, LB);
    q.admit_from = up(admit_from, LB);
    q.next = up(next, 4);
    q.active = up(active, 4);
    if (!ok || !launch_gen_turnover(nullptr, q, step) || hipDeviceSynchronize() != hipSuccess) return false;
    const std::tuple<void *, const void *, size_t> down[] = {
        {lane_seq, q.lane_seq, LB}, {done, q.done, QB}, {lane, q.lane, QB},           {start, q.start, QB},
        {next, q.next, 4},          {active, q.active, 4}, {retire_to, q.retire_to, LB}, {admit_from, q.admit_from, LB}};
    for (const auto & d : down)
        if (hipMemcpy(std::get<0>(d), std::get<1>(d), std::get<2>(d), hipMemcpyDeviceToHost) != hipSuccess) return false;
    return true;
}

// The scoring kernel (xent.hip) on host operands: what rwkv_mi355x_score_sequence launches per head
// tile, one workgroup per row.  Targets beyond the row are refused here (the kernel clamps them).
extern "C" RWKV_API bool rwkv_mi355x_selftest_xent(const float * logits, int rows, int V, const uint32_t * targets,
                                                   double * losses, uint32_t * argmax) {
    if (!logits || rows < 1 || V < 1 || (losses && !targets)) return false;
    if (targets)
        for (int r = 0; r < rows; r++)
            if (targets[r] >= (uint32_t)V) return false;
    const size_t n = (size_t)rows * V;
    DevBufs b;
    float * dl = (float *)b.alloc(n * 4);
    uint32_t * dt = (uint32_t *)b.alloc((size_t)rows * 4);
    double * dloss = (double *)b.alloc((size_t)rows * 8);
    uint32_t * da = (uint32_t *)b.alloc((size_t)rows * 4);
    if (!dl || !dt || !dloss || !da) return false;
    if (hipMemcpy(dl, logits, n * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    if (targets && hipMemcpy(dt, targets, (size_t)rows * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    if (!launch_xent(nullptr, dl, rows, V, targets ? dt : nullptr, losses ? dloss : nullptr, da) ||
        hipDeviceSynchronize() != hipSuccess)
        return false;
    if (losses && hipMemcpy(losses, dloss, (size_t)rows * 8, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (argmax && hipMemcpy(argmax, da, (size_t)rows * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    return true;
}

// k_groupnorm (the sequence path's per-head norm after WKV) on host operands with an fp32 output:
// out[t][c] = ((y - mean_h) / sqrt(var_h + eps) * w[c] + b[c] (+ v * bonus[t][h], mode 2)) (* g, modes 1, 2).
// y, g, v, out: [T][H*S]; w, b: [H*S]; bonus: [T][H].  S a power of two <= 64, H*S a multiple of 32.
extern "C" RWKV_API bool rwkv_mi355x_selftest_groupnorm(int T, int H, int S, float eps, int mode, const float * y,
                                                       const float * w, const float * b, const float * g,
                                                       const float * v, const float * bonus, float * out) {
    if (T < 1 || H < 1 || S < 1 || mode < 0 || mode > 2 || !y || !w || !b || !out) return false;
    if ((mode >= 1 && !g) || (mode == 2 && (!v || !bonus)) || (H * S) % 32) return false;
    const size_t C = (size_t)H * S, TC = (size_t)T * C;
    DevBufs bf;
    ActBuf o;
    memset(&o, 0, sizeof(o));
    o.fmt = A_F32;
    o.K = (int)C;
    float *dy = (float *)bf.alloc(TC * 4), *dw = (float *)bf.alloc(C * 4), *db = (float *)bf.alloc(C * 4),
          *dg = (float *)bf.alloc(TC * 4), *dv = (float *)bf.alloc(TC * 4), *dbo = (float *)bf.alloc((size_t)T * H * 4);
    o.f = (float *)bf.alloc(TC * 4);
    if (!dy || !dw || !db || !dg || !dv || !dbo || !o.f) return false;
    if (hipMemcpy(dy, y, TC * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dw, w, C * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(db, b, C * 4, hipMemcpyHostToDevice) != hipSuccess)
        return false;
    if (mode >= 1 && hipMemcpy(dg, g, TC * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    if (mode == 2 && (hipMemcpy(dv, v, TC * 4, hipMemcpyHostToDevice) != hipSuccess ||
                      hipMemcpy(dbo, bonus, (size_t)T * H * 4, hipMemcpyHostToDevice) != hipSuccess))
        return false;
    if (!launch_groupnorm(nullptr, T, H, S, eps, dy, dw, db, mode, dg, dv, dbo, o) || hipDeviceSynchronize() != hipSuccess)
        return false;
    return hipMemcpy(out, o.f, TC * 4, hipMemcpyDeviceToHost) == hipSuccess;
}

// k_ln_emit (the LayerNorm in front of the head) on host operands with an fp32 output:
// out[r] = LN(x[r]) * w + b, eps 1e-5.  x, out: [rows][C]; w, b: [C]; C a multiple of 64.
extern "C" RWKV_API bool rwkv_mi355x_selftest_ln(int C, int rows, const float * x, const float * w, const float * b,
                                                float * out) {
    if (C < 64 || C % 64 || rows < 1 || !x || !w || !b || !out) return false;
    const size_t n = (size_t)rows * C;
    DevBufs bf;
    ActBuf o;
    memset(&o, 0, sizeof(o));
    o.fmt = A_F32;
    o.K = C;
    float *dx = (float *)bf.alloc(n * 4), *dw = (float *)bf.alloc((size_t)C * 4), *db = (float *)bf.alloc((size_t)C * 4);
    o.f = (float *)bf.alloc(n * 4);
    if (!dx || !dw || !db || !o.f) return false;
    if (hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dw, w, (size_t)C * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(db, b, (size_t)C * 4, hipMemcpyHostToDevice) != hipSuccess)
        return false;
    if (!launch_ln_emit(nullptr, C, dx, dw, db, o, rows) || hipDeviceSynchronize() != hipSuccess) return false;
    return hipMemcpy(out, o.f, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
}

// wave_sums<n> (device_common.hpp) against wave_sum63 on host operands, one wave.  n = 2, 4, ..., 64:
// p [64 lanes][n]; sums[l] = the wave_sums result of lane l (slot l & (n - 1)), ref[j] = wave_sum63 of
// slot j.  n = 3 / -3: the matvecs' padded three-row form row_sums<Q8_0 / Q4_1, 3> on p [64][6] (acc
// then acc2 per lane); ref[j] = wave_sum63(acc_j) + 0.0f / wave_sum63(acc_j) + wave_sum63(acc2_j).
extern "C" RWKV_API bool rwkv_mi355x_selftest_wave_sums(int n, const float * p, float * sums, float * ref) {
    if (!p || !sums || !ref) return false;
    const int width = (n == 3 || n == -3) ? 6 : n, slots = n < 0 ? -n : n;
    DevBufs b;
    float * dp = (float *)b.alloc((size_t)64 * width * 4);
    float * ds = (float *)b.alloc(64 * 4);
    float * dr = (float *)b.alloc(64 * 4);
    if (!dp || !ds || !dr) return false;
    if (hipMemcpy(dp, p, (size_t)64 * width * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
    switch (n) {
        case 2: hipLaunchKernelGGL(k_selftest_wave_sums<2>, dim3(1), dim3(64), 0, nullptr, dp, ds, dr); break;
        case 4: hipLaunchKernelGGL(k_selftest_wave_sums<4>, dim3(1), dim3(64), 0, nullptr, dp, ds, dr); break;
        case 8: hipLaunchKernelGGL(k_selftest_wave_sums<8>, dim3(1), dim3(64), 0, nullptr, dp, ds, dr); break;
        case 16: hipLaunchKernelGGL(k_selftest_wave_sums<16>, dim3(1), dim3(64), 0, nullptr, dp, ds, dr); break;
        case 32: hipLaunchKernelGGL(k_selftest_wave_sums<32>, dim3(1), dim3(64), 0, nullptr, dp, ds, dr); break;
        case 64: hipLaunchKernelGGL(k_selftest_wave_sums<64>, dim3(1), dim3(64), 0, nullptr, dp, ds, dr); break;
        case 3: hipLaunchKernelGGL(k_selftest_row_sums3<W_Q8_0>, dim3(1), dim3(64), 0, nullptr, dp, ds, dr); break;
        case -3: hipLaunchKernelGGL(k_selftest_row_sums3<W_Q4_1>, dim3(1), dim3(64), 0, nullptr, dp, ds, dr); break;
        default: return false;
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return false;
    return hipMemcpy(sums, ds, 64 * 4, hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(ref, dr, (size_t)slots * 4, hipMemcpyDeviceToHost) == hipSuccess;
}
