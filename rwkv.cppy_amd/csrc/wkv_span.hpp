// wkv_span.hpp -- where a serial WKV workgroup's tokens and state live (wkv_serial.hip).
//
// A launch runs one recurrence per span; blockIdx.z is the span index in every kernel.  A span type
// is a plain struct passed by value as the kernel's first argument; at(i) places span i.  The
// recurrence bodies apply it once at the top (wkv_advance on their token-row and state pointers,
// then T) and are written for one sequence from there on, so their look-ahead clamps (T - 1) stay
// inside the span and a span's result is bit for bit the one-sequence kernel's on its tokens.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "kernels.hpp"

namespace rwkvmi {

struct WkvPlace {
    int T;          // tokens
    uint32_t row;   // first token row in the [rows][C] operands and outputs
    size_t sin;     // float offsets of the span's state from the launch's state pointers
    size_t sout;
};

// One sequence: T tokens from row 0, the state at the pointers.  Everything but T is a constant, so
// this instantiation is the plain kernel.
struct SpanSeq {
    int T;
    __device__ __forceinline__ WkvPlace at(uint32_t) const { return {T, 0u, 0, 0}; }
};

// Contexts (batched decode; WKV-4 only -- v5 / v6 / v7 take k_att6_dec / k_att7_dec there): row i is
// context i's one token, its state at i * bs.
struct SpanCtx {
    int bs;
    __device__ __forceinline__ WkvPlace at(uint32_t i) const { return {1, i, (size_t)i * bs, (size_t)i * bs}; }
};

// Segments of a packed chunk (batched prefill, SegTab in kernels.hpp).
struct SpanSeg {
    SegTab sg;
    __device__ __forceinline__ WkvPlace at(uint32_t s) const {
        return {(int)sg.len[s], sg.begin[s], (size_t)sg.sin_off[s], (size_t)sg.sout_off[s]};
    }
};

// p += o for every pointer
template <class... P>
__device__ __forceinline__ void wkv_advance(size_t o, P *&... p) {
    ((p += o), ...);
}

// The span of a launch and its count (grid.z), handed to f(span, nz).  bs and seg exclude each other.
template <class F>
bool with_span(int T, const SegTab * seg, F && f) {
    return seg ? f(SpanSeg{*seg}, seg->n) : f(SpanSeq{T}, 1);
}
template <class F>
bool with_span(int T, int bs, const SegTab * seg, F && f) {
    if (seg && bs) return false;
    return bs ? f(SpanCtx{bs}, T) : with_span(T, seg, f);
}

}  // namespace rwkvmi
