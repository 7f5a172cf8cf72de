// handoff.hpp -- the in-launch hand-off protocol of the fused decode launches, once (DESIGN.md
// "The hand-off protocol").
//
// A granule is 8 aligned bytes {tag (high word), value bits (low word)} written by ONE agent-scope
// store, so the data is its own flag: a reader that sees the tag it expects holds the value too.
//   tagged granules   carry Handoff::tag (layer and state parity, never 0 or 1): a value of another
//                     layer or step never matches, so nobody clears them in a launch (the host does
//                     when the parity flips without a fused decode, Engine: GranuleMem::clear_tagged).
//   cleared granules  carry GRAN_ONCE and have exactly one reader, which sweeps until it reads the
//                     tag and then clears the granule: one is only ever 0 or this launch's value.
// A consumer re-reads its granules -- the poll IS the gather: one round trip after the last value
// lands -- sleeping between passes, for at most spin_max + 1 passes; then it stores 1 to *err (a
// host-mapped word, system scope) and goes on with what it has: the host fails the call
// (Engine::handoff_check).  Everything here is __forceinline__: the callers are hot loops of kernels
// with tuned register budgets.
#pragma once
#include "kernels.hpp"

namespace rwkvmi {

typedef __attribute__((address_space(1))) unsigned long long gran_u64_t;
typedef __attribute__((address_space(1))) unsigned gran_u32_t;

constexpr unsigned GRAN_ONCE = 1;  // the tag of the cleared (single-reader) granules

__device__ __forceinline__ unsigned long long gran_pack(unsigned tag, unsigned bits) {
    return ((unsigned long long)tag << 32) | bits;
}
__device__ __forceinline__ unsigned gran_tag(unsigned long long x) { return (unsigned)(x >> 32); }
__device__ __forceinline__ unsigned gran_bits(unsigned long long x) { return (unsigned)x; }
__device__ __forceinline__ float gran_float(unsigned long long x) { return __uint_as_float((unsigned)x); }

__device__ __forceinline__ void gran_store(unsigned long long * g, unsigned tag, unsigned bits) {
    __hip_atomic_store((gran_u64_t *)g, gran_pack(tag, bits), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gran_store(unsigned long long * g, unsigned tag, float v) {
    gran_store(g, tag, __float_as_uint(v));
}
__device__ __forceinline__ unsigned long long gran_load(const unsigned long long * g) {
    return __hip_atomic_load((gran_u64_t *)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gran_clear(unsigned long long * g) {
    __hip_atomic_store((gran_u64_t *)g, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void handoff_fail(unsigned * err) {
    __hip_atomic_store((gran_u32_t *)err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The bounded wait of one wave.  pass() performs one pass's loads -- all of them, whatever the tags
// read: no load waits for a tag of the same pass -- and returns this lane's ok (a lane with nothing
// to wait for returns true); the payload read in the pass that succeeds is the gathered value.
// False after a timeout (*err set).
template <int SLEEP, class Pass>
__device__ __forceinline__ bool gran_wait(unsigned spin_max, unsigned * err, Pass && pass) {
    for (unsigned it = 0;; it++) {
        if (__all(pass())) return true;
        if (it >= spin_max) {
            handoff_fail(err);
            return false;
        }
        __builtin_amdgcn_s_sleep(SLEEP);
    }
}
// The same for a poll ahead of a gather on the same granules, each lane for itself: at most spin_max
// passes and no error store -- the gather after it reports the timeout.
template <int SLEEP, class Pass>
__device__ __forceinline__ void gran_wait_quiet(unsigned spin_max, Pass && pass) {
    for (unsigned it = 0; it < spin_max; it++) {
        if (pass()) break;
        __builtin_amdgcn_s_sleep(SLEEP);
    }
}

// One pass over N consecutive granules: their values -> v, true when every tag reads `tag`
template <int N>
__device__ __forceinline__ bool gran_read(const unsigned long long * g, unsigned tag, float (&v)[N]) {
    unsigned long long x[N];
#pragma unroll
    for (int j = 0; j < N; j++) x[j] = gran_load(g + j);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        v[j] = gran_float(x[j]);
        ok = ok && gran_tag(x[j]) == tag;
    }
    return ok;
}

// One wave sweeps N cleared granules per lane (g[k * stride], live[k] only) until every tag is set;
// the caller clears them.
template <int N>
__device__ __forceinline__ void gran_sweep(const unsigned long long * g, int stride, bool (&live)[N], float (&v)[N],
                                           unsigned * err, unsigned spin_max) {
    gran_wait<1>(spin_max, err, [&] {
        unsigned long long x[N];
#pragma unroll
        for (int k = 0; k < N; k++) x[k] = live[k] ? gran_load(g + k * stride) : gran_pack(GRAN_ONCE, 0);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < N; k++) {
            v[k] = gran_float(x[k]);
            ok = ok && gran_tag(x[k]) == GRAN_ONCE;
        }
        return ok;
    });
}

// Q8 blocks published by pub_q8 (mv_common.hpp; KG_STRIDE granules per 32-element block, nb blocks).
// Wait before their gather: ONE wave polls the d granule of every block, 64 blocks at a time (lane i:
// block b0 + i), with a sleep between passes until every tag reads `tag` -- a few hundred bytes per
// pass instead of the gather's whole vector, so a waiting workgroup adds little traffic beside the
// producers' weight streams (the gather after it checks every tag again).  (Several passes in flight
// at once -- a rolling poll -- measured far slower: v6-1B6 750 vs 693 us/token.)
__device__ __forceinline__ void q8_prepoll(const unsigned long long * kg, int nb, unsigned tag, unsigned * err,
                                           unsigned spin_max, int lane) {
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const unsigned long long * g = kg + (size_t)b0 * KG_STRIDE;
        const int n = min(64, nb - b0);
        gran_wait<4>(spin_max, err, [&] {
            const unsigned long long x = lane < n ? gran_load(g + 8 + (size_t)lane * KG_STRIDE) : gran_pack(tag, 0);
            return gran_tag(x) == tag;
        });
    }
}
// The gather: thread tid of nthr reads granules tid + nthr i (i < GI) into pay, re-reading until
// every tag it holds reads `tag`.  extra() loads one more granule of the same tag in the same pass
// (the caller keeps its payload) and returns it.
template <int GI, class Extra>
__device__ __forceinline__ void q8_gather(const unsigned long long * kg, int nb, unsigned tag, unsigned (&pay)[GI], int tid,
                                          int nthr, unsigned * err, unsigned spin_max, Extra && extra) {
    const int ng = KG_STRIDE * nb;
    gran_wait<2>(spin_max, err, [&] {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < GI; i++) {
            const int g = tid + nthr * i;
            unsigned long long x = gran_pack(tag, 0);
            if (g < ng) x = gran_load(kg + g);
            pay[i] = gran_bits(x);
            ok = ok && gran_tag(x) == tag;
        }
        const unsigned long long xe = extra();
        return ok && gran_tag(xe) == tag;
    });
}
// ... -> the LDS activation image: granule KG_STRIDE b + j is slot j of block b, slots 0..7 the q
// dwords, 8 d, 9 Q8_1's s.  The caller recomputes the qsums (q8_image_qsum) after a barrier.
template <int GI>
__device__ __forceinline__ void q8_scatter(const ActBuf & img, int nb, const unsigned (&pay)[GI], int tid, int nthr) {
    const int ng = KG_STRIDE * nb;
#pragma unroll
    for (int i = 0; i < GI; i++) {
        const int g = tid + nthr * i;
        if (g < ng) {
            const int b = g / KG_STRIDE, j = g - b * KG_STRIDE;
            if (j < 8) *(unsigned *)(img.q + (size_t)b * 32 + 4 * j) = pay[i];
            else if (j == 8) img.d[b] = __uint_as_float(pay[i]);
            else if (img.fmt == A_Q8_1) img.s[b] = __uint_as_float(pay[i]);
        }
    }
}
template <int GI>
__device__ __forceinline__ void q8_gather_image(const unsigned long long * kg, int nb, unsigned tag, const ActBuf & img,
                                                int tid, int nthr, unsigned * err, unsigned spin_max) {
    unsigned pay[GI];
    q8_gather<GI>(kg, nb, tag, pay, tid, nthr, err, spin_max, [&] { return gran_pack(tag, 0); });
    q8_scatter<GI>(img, nb, pay, tid, nthr);
}

}  // namespace rwkvmi
