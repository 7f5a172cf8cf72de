// engine_sequence.hip -- the sequence program: the per-version layer functions over T rows, their
// matmul groups and the head, for a plain sequence, a batched decode step, a packed prefill chunk and
// the head tiles of the scorer and the prefill.  Which of them a forward is comes in one value, its
// SeqRun (engine.hpp).  Per-layer programs restate rwkv_graph.inc:
//   v4  :84-197 + FFN :484-511      v5  :199-292 + FFN :484-511
//   v6  :294-385 + FFN :513-531     v7  :387-482 + FFN :533-543
#include <assert.h>
#include <string.h>

#include <string>

#include "engine.hpp"

namespace rwkvmi {

// The one place a SeqRun is completed: the two implications between the modes, and tile_acts -- layer
// matmuls over all T rows take Q8 activations straight in GEMM tiles, contexts from batch_gemm_min_ rows on.
SeqRun Engine::make_run(SeqRun s) const {
    assert((!s.seg || !s.bs) && (!s.bs || s.rows));
    s.tile_acts = s.T >= 2 && !use_mm_ && (!s.rows || s.T >= batch_gemm_min_);
    return s;
}

SeqRun Engine::seq_run(int T, const float * sin, float * sout, uint32_t l0, uint32_t l1, const TokArg & tok,
                       float * head_out) const {
    return make_run(SeqRun{T, sin, sout, l0, l1, 0, nullptr, false, false, tok, head_out});
}

SeqRun Engine::rows_run(int B, size_t bs, const float * sin, float * sout, float * head_out) const {
    return make_run(SeqRun{B, sin, sout, 0, m_->n_layer, bs, nullptr, true, false, dtok(), head_out});
}

SeqRun Engine::packed_run(int T, const SegTab * seg, float * states) const {
    return make_run(SeqRun{T, states, states, 0, m_->n_layer, 0, seg, false, false, dtok(), nullptr});
}

// Collects matmul entries and launches them grouped by weight type.
struct MMBatch {
    std::vector<MMEntry> e;
    void add(const DMat & W, const ActBuf & in, float * y, int ldy, int epi, const float * aux = nullptr,
             const float * bias = nullptr, const ActBuf * out = nullptr) {
        MMEntry m;
        memset(&m, 0, sizeof(m));
        m.W = W;
        m.in = in;
        m.y = y;
        m.ldy = ldy;
        m.aux = aux;
        m.bias = bias;
        m.epi = epi;
        if (out) {
            m.out = *out;
            m.emit = 1;
        }
        e.push_back(m);
    }
    bool run(Engine & eng, const SeqRun & s) { return run(eng, s.T, s.rows, s.tile_acts); }
    bool run(Engine & eng, int T, bool rows, bool tile_acts) {
        std::vector<bool> done(e.size(), false);
        for (size_t i = 0; i < e.size(); i++) {
            if (done[i]) continue;
            MMGroup g;
            memset(&g, 0, sizeof(g));
            g.T = T;
            const int type = e[i].W.type;
            for (size_t j = i; j < e.size() && g.n < MM_MAX_ENTRIES; j++) {
                if (!done[j] && e[j].W.type == type) {
                    g.e[g.n++] = e[j];
                    done[j] = true;
                }
            }
            if (!eng.mm_launch(g, type, eng.mm_route(T, type, rows, tile_acts))) return false;
        }
        e.clear();
        return true;
    }
};

// Where a matmul group of T rows goes.  Rows as contexts (batched decode, the head tiles): the decode
// matvec over the contexts, unless the layer's activations are in token tiles -- then the quantized matmuls
// take the sequence GEMM (the same bits).  Else quantized weights over two or more rows go to the GEMM.
Engine::MMRoute Engine::mm_route(int T, int wtype, bool rows, bool tile_acts) const {
    if (rows && !(tile_acts && wtype_quantized(wtype))) return MM_ROWS;
    return T < 2 || !wtype_quantized(wtype) || use_mm_ ? MM_KMM : MM_QGEMM;
}

// Sequence matmuls on quantized weights go to the int8-MFMA GEMM; entries that only emit get
// a scratch y, and emission is a separate quantization pass (same bits as k_mm's epilogue).
bool Engine::mm_dispatch(MMGroup & g, int wtype, MMRoute route) {
    if (!wtype_quantized(wtype) && g.T >= 32) {
        // k_fmm may split the class tree of a small grid (the v7 LoRA first stage): partials, only
        // when launch_fmm_group's rule can split this group (below 2 workgroups per CU)
        size_t msum = 0;
        int blocks = 0;
        bool splittable = true;
        for (int i = 0; i < g.n; i++) {
            msum += g.e[i].W.M;
            blocks += (g.e[i].W.M + 63) / 64 * ((g.T + 63) / 64);
            splittable = splittable && g.e[i].W.K >= 512 && g.e[i].W.M % 32 == 0;
        }
        if (splittable && blocks < 2 * kQgCUs) {
            const size_t split = (size_t)blocks * 4 >= (size_t)2 * kQgCUs ? 4 : 8;
            const size_t pneed = split * g.T * msum;
            if (!grow(part_, pneed, pneed, GRAPHS_BATCH)) return false;
            g.part = part_;
            g.part_floats = part_.size();
        }
    }
    if (route == MM_ROWS) {
        // k_mvb; float weights (the F16 head, LoRA) over 16+ contexts: the f32-MFMA form; k_mm for
        // the shapes neither covers -- the same bits
        bool launched = false;
        if (!launch_fmm_group(stream_, g, wtype, &launched)) return false;
        if (launched) return true;
        if (!launch_mvb_group(stream_, g, wtype, &launched)) return false;
        if (launched) return true;
    }
    if (route != MM_QGEMM) return launch_mm_group(stream_, g, wtype);
    size_t need = 0;
    for (int i = 0; i < g.n; i++)
        if (!g.e[i].y) need += (size_t)g.T * g.e[i].W.M;
    if (!grow(gy_, need, need, GRAPHS_BATCH)) return false;
    // split-K partials (launch_qgemm splits groups with few tiles: small T or small M)
    {
        const int rows = qg_rows(wtype), tilesT = (g.T + QG_TOK - 1) / QG_TOK;
        size_t msum = 0, tiles = 0;
        for (int i = 0; i < g.n; i++) {
            msum += g.e[i].W.M;
            tiles += (size_t)(g.e[i].W.M + rows - 1) / rows * tilesT;
        }
        if (tiles < 1024) {
            const size_t pneed = (size_t)8 * g.T * msum;
            if (!grow(part_, pneed, pneed, GRAPHS_BATCH)) return false;
            g.part = part_;
            g.part_floats = part_.size();
        }
        if (qg_one(wtype)) {
            const size_t mneed = (size_t)g.T * msum;
            if (!grow(m2_, mneed, mneed, GRAPHS_BATCH)) return false;
            g.m2 = m2_;
            g.m2_floats = m2_.size();
        }
    }
    size_t off = 0;
    for (int i = 0; i < g.n; i++) {
        MMEntry & e = g.e[i];
        if (!e.y) {
            e.y = gy_ + off;
            e.ldy = e.W.M;
            off += (size_t)g.T * e.W.M;
        }
    }
    if (!launch_qgemm(stream_, g, wtype)) return false;
    for (int i = 0; i < g.n; i++) {
        const MMEntry & e = g.e[i];
        if (e.emit && !e.fuse_emit && e.ldy == e.W.M && !launch_act_from_f32(stream_, e.y, g.T, e.W.M, e.out))
            return false;
        if (e.emit && e.ldy != e.W.M) {
            fprintf(stderr, "rwkv: emitting GEMM entry needs ldy == M\n");
            return false;
        }
    }
    return true;
}

bool Engine::mm_launch(MMGroup & g, int wtype, MMRoute route) {
    if (!timing_) return mm_dispatch(g, wtype, route);
    bool emit = false;
    double bytes = 0, flops = 0;
    for (int i = 0; i < g.n; i++) {
        const MMEntry & e = g.e[i];
        emit |= e.emit != 0;
        bytes += (double)type_nbytes((uint32_t)e.W.type, (uint64_t)e.W.M * e.W.K) + act_bytes(e.in, g.T);
        if (e.y) bytes += (double)g.T * e.W.M * 4 * ((e.epi == EPI_ADD || e.epi == EPI_SIGMUL_ADD || e.epi == EPI_VMIX7) ? 2 : 1);
        if (e.emit) bytes += act_bytes(e.out, g.T);
        flops += 2.0 * e.W.M * e.W.K * g.T;
    }
    // kernel class = the template instantiation rocprofv3 reports: k_mm<WF, RPW, NT>; every launch of
    // the rows-as-contexts route goes by k_mvb's name
    const std::string name = route == MM_QGEMM ? "k_qgemm<" + std::to_string(wtype) + ">"
                           : route == MM_ROWS ? "k_mvb<" + std::to_string(wtype) + ">"
                                              : "k_mm<" + std::to_string(wtype) + ", " + (emit ? "8" : "2") + ", " + (g.T == 1 ? "1" : "4") + ">";
    const int si = add_stat(name);
    hipEvent_t a, b;  // a pair from the pool, as a timed RK_LAUNCH takes one
    if (!begin(&a, &b)) return false;
    HIP_OK(hipEventRecord(a, stream_));
    const bool ok = mm_dispatch(g, wtype, route);
    HIP_OK(hipEventRecord(b, stream_));
    pending_.push_back(Pending{si, a, b, bytes, flops});
    return ok;
}

// The LayerNorm + token shift + mix launch of a sequence / batched layer, up to its outputs:
// carry_in / carry_out = the layer's *_xx state row (context t's at + t * s.bs in a batched step)
LnMixArgs Engine::ln_mix_args(const SeqRun & s, const float * carry_in, float * carry_out, const float * lnw,
                              const float * lnb) const {
    LnMixArgs a;
    memset(&a, 0, sizeof(a));
    a.T = s.T;
    a.C = (int)m_->n_embed;
    a.x = x_;
    a.carry_in = carry_in;
    a.carry_out = carry_out;
    a.bs = s.bs;
    a.lnw = lnw;
    a.lnb = lnb;
    return a;
}

bool Engine::ffn(const SeqRun & s, int l, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed;
    LnMixArgs a = ln_mix_args(s, si, so, L.ln2_w, L.ln2_b);  // ffn_xx at layer offset 0
    // v4/v5: rwkv_graph.inc:484-511 (form 0); v6: :513-531 (form 1); v7: :533-543 (form 1, the key only)
    const bool hasr = m_->major != 7;
    a.form = m_->major >= 6 ? 1 : 0;
    a.n_out = hasr ? 2 : 1;
    a.mu[0] = m_->major == 7 ? L.ffn_x_k : m_->major == 6 ? L.ffn_maa_k : L.ffn_mix_k;
    a.out[0] = A(s, 0, L.ffn_k);
    if (hasr) {
        a.mu[1] = m_->major == 6 ? L.ffn_maa_r : L.ffn_mix_r;
        a.out[1] = A(s, 1, L.ffn_r);
    }
    if (!launch_ln_mix(stream_, a, s.seg)) return false;
    ActBuf kin = A(s, hasr ? 2 : 1, L.ffn_v);
    MMBatch b;
    if (hasr) b.add(L.ffn_r, a.out[1], fr_, C, EPI_STORE);
    b.add(L.ffn_k, a.out[0], nullptr, 0, EPI_RELU_SQ, nullptr, nullptr, &kin);
    if (!b.run(*this, s)) return false;
    b.add(L.ffn_v, kin, x_, C, hasr ? EPI_SIGMUL_ADD : EPI_ADD, hasr ? fr_ : nullptr);
    return b.run(*this, s);
}

static bool launch_att_dec(hipStream_t st, const Att6Dec & a) { return launch_att6_dec(st, a); }
static bool launch_att_dec(hipStream_t st, const Att7Dec & a) { return launch_att7_dec(st, a); }

// Batched decode (s.bs > 0): the attention core of every context is the decode kernel itself (one
// workgroup per head and context, k_att6_dec / k_att7_dec); its output goes to Wo's input `o`
// (emitted by the kernel when heads are whole quantization blocks, else fp32 y_ converted).
// The rest of such a layer: a = att6_args / att7_args, then Wo (input slot wo_slot) and the FFN.
template <class Att>
bool Engine::batch_att_tail(const SeqRun & s, Att a, int wo_slot, int l, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed;
    ActBuf o = A(s, wo_slot, L.att_o);
    a.nb = s.T;
    a.bs = s.bs;
    if (a.S >= 32) a.yq = o;
    if (!launch_att_dec(stream_, a)) return false;
    if (a.S < 32 && !launch_act_from_f32(stream_, y_, s.T, C, o)) return false;
    MMBatch b;
    b.add(L.att_o, o, x_, C, EPI_ADD);
    if (!b.run(*this, s)) return false;
    return ffn(s, l, si, so);
}

bool Engine::layer_v4(const SeqRun & s, int l, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed;
    LnMixArgs a = ln_mix_args(s, si + C, so + C, L.ln1_w, L.ln1_b);
    a.form = 0;
    a.n_out = 3;
    a.mu[0] = L.att_mix_k;
    a.mu[1] = L.att_mix_v;
    a.mu[2] = L.att_mix_r;
    a.out[0] = A(s, 0, L.att_k);
    a.out[1] = A(s, 1, L.att_v);
    a.out[2] = A(s, 2, L.att_r);
    if (!launch_ln_mix(stream_, a, s.seg)) return false;
    MMBatch b;
    b.add(L.att_r, A(s, 2, L.att_r), r_, C, EPI_SIGMOID);
    b.add(L.att_k, A(s, 0, L.att_k), k_, C, EPI_STORE);
    b.add(L.att_v, A(s, 1, L.att_v), v_, C, EPI_STORE);
    if (!b.run(*this, s)) return false;
    ActBuf o = A(s, 3, L.att_o);
    if (!launch_wkv4(stream_, s.T, C, r_, k_, v_, L.att_first, L.att_decay, si, so, o, (int)s.bs, s.seg)) return false;
    b.add(L.att_o, o, x_, C, EPI_ADD);
    if (!b.run(*this, s)) return false;
    return ffn(s, l, si, so);
}

// v5/v6 sequence wkv: the serial recurrence (k_wkv6_s64, bit-exact with decode; a prefill's packed
// chunk always: its segmented form), or behind the wkv_chunk_ switch the chunk-parallel form (RA / KB
// in the v7-only nb_ / bb_ buffers, free during a v5/v6 layer; the chunk matrices and states in
// wkvc_, grown on demand)
bool Engine::wkv6(const SeqRun & s, int H, int S, const float * u, const float * w, int wpt, const float * sin, float * sout) {
    if (wkv_chunk_ && !s.seg && wkv6_chunked_supported(s.T, S, (int)s.bs)) {
        const size_t need = wkv6_chunked_scratch_floats(s.T, H);
        if (!grow(wkvc_, need, need, GRAPHS_NONE)) return false;
        return launch_wkv6_chunked(stream_, s.T, H, k_, v_, r_, u, w, wpt, sin, sout, y_, nb_, bb_, wkvc_);
    }
    return launch_wkv6(stream_, s.T, H, S, k_, v_, r_, u, w, wpt, sin, sout, y_, s.seg);
}

bool Engine::layer_v5(const SeqRun & s, int l, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed, H = (int)m_->H, S = (int)m_->S;
    const bool v52 = m_->minor >= 2;
    LnMixArgs a = ln_mix_args(s, si + C, so + C, L.ln1_w, L.ln1_b);
    a.form = 0;
    a.n_out = v52 ? 4 : 3;
    a.mu[0] = L.att_mix_k;
    a.mu[1] = L.att_mix_v;
    a.mu[2] = L.att_mix_r;
    a.out[0] = A(s, 0, L.att_k);
    a.out[1] = A(s, 1, L.att_v);
    a.out[2] = A(s, 2, L.att_r);
    if (v52) {
        a.mu[3] = L.att_mix_g;
        a.out[3] = A(s, 3, L.att_g);
    }
    if (!launch_ln_mix(stream_, a, s.seg)) return false;
    MMBatch b;
    b.add(L.att_r, A(s, 2, L.att_r), r_, C, EPI_STORE);
    b.add(L.att_k, A(s, 0, L.att_k), k_, C, EPI_STORE);
    b.add(L.att_v, A(s, 1, L.att_v), v_, C, EPI_STORE);
    if (v52) b.add(L.att_g, A(s, 3, L.att_g), g_, C, EPI_SILU);
    if (!b.run(*this, s)) return false;
    if (s.bs) return batch_att_tail(s, att6_args(L, si, so, s.bs), 4, l, si, so);
    if (!wkv6(s, H, S, L.att_u, L.att_w, 0, si + 2 * C, so + 2 * C)) return false;
    ActBuf o = A(s, 4, L.att_o);
    if (!launch_groupnorm(stream_, s.T, H, S, 1e-5f, y_, L.att_lnx_w, L.att_lnx_b, v52 ? 1 : 0, g_, nullptr, nullptr, o))
        return false;
    b.add(L.att_o, o, x_, C, EPI_ADD);
    if (!b.run(*this, s)) return false;
    return ffn(s, l, si, so);
}

bool Engine::layer_v6(const SeqRun & s, int l, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int T = s.T, C = (int)m_->n_embed, H = (int)m_->H, S = (int)m_->S, D = m_->maa_D;
    LnMixArgs a = ln_mix_args(s, si + C, so + C, L.ln1_w, L.ln1_b);
    a.form = 1;
    a.n_out = 1;
    a.mu[0] = L.maa_x;
    a.out[0] = A(s, 0, L.maa_w1);
    a.out_xa = xa_;
    a.out_sx = sx_;
    if (!launch_ln_mix(stream_, a, s.seg)) return false;
    MMBatch b;
    b.add(L.maa_w1, A(s, 0, L.maa_w1), lora_, 5 * D, EPI_TANH);
    if (!b.run(*this, s)) return false;
    // order w, k, v, r, g (rwkv_graph.inc:336-346)
    ActBuf outs[5] = {A(s, 1, L.decay_w1), A(s, 2, L.att_k), A(s, 3, L.att_v), A(s, 4, L.att_r), A(s, 5, L.att_g)};
    // batched decode: the decode kernel's per-(mix, channel) arithmetic over the contexts; from
    // batch_gemm_min_ contexts on (token-tile outputs) the sequence kernel's f32-MFMA form over the
    // contexts as tokens -- W2 read once per 64 contexts instead of once per context, same bits
    if ((s.bs && !s.tile_acts) ? !launch_v6_mix5_dec(stream_, C, D, xa_, nullptr, lora_, L.maa_w2t, L.maa, outs, T, sx_)
                               : !launch_v6_mix5(stream_, T, C, D, lora_, L.maa_w2t, L.maa, xa_, sx_, outs))
        return false;
    ActBuf dl = A(s, 6, L.decay_w2);
    // decay tail by threads (k_att6_dec's rows) when Wd2 is quantized; dl fp32 then reuses lora_
    // (consumed by mix5 above)
    const int DD = L.decay_w2.K;  // decay LoRA width (64 for the released checkpoints)
    const bool dseq = v6_decay_seq_supported(L.decay_w2.type, DD) && L.decay_w1.M == DD;
    b.add(L.att_r, outs[3], r_, C, EPI_STORE);
    b.add(L.att_k, outs[1], k_, C, EPI_STORE);
    b.add(L.att_v, outs[2], v_, C, EPI_STORE);
    b.add(L.att_g, outs[4], g_, C, EPI_SILU);
    if (s.bs) {
        // decode's split: decay W1 (tanh) with r,k,v,g; the LoRA tail, wkv and GroupNorm per head
        b.add(L.decay_w1, outs[0], lora_, L.decay_w1.M, EPI_TANH);
        if (!b.run(*this, s)) return false;
        return batch_att_tail(s, att6_args(L, si, so, s.bs), 7, l, si, so);
    }
    if (dseq) b.add(L.decay_w1, outs[0], lora_, DD, EPI_TANH);
    else b.add(L.decay_w1, outs[0], nullptr, 0, EPI_TANH, nullptr, nullptr, &dl);
    if (!b.run(*this, s)) return false;
    if (dseq) {
        if (!launch_v6_decay_seq(stream_, T, C, L.decay_w2, lora_, L.decay6, w_)) return false;
    } else {
        b.add(L.decay_w2, dl, w_, C, EPI_DECAY6, nullptr, L.decay6);
        if (!b.run(*this, s)) return false;
    }
    if (!wkv6(s, H, S, L.att_u, w_, 1, si + 2 * C, so + 2 * C)) return false;
    ActBuf o = A(s, 7, L.att_o);
    if (!launch_groupnorm(stream_, T, H, S, 64e-5f, y_, L.att_lnx_w, L.att_lnx_b, 1, g_, nullptr, nullptr, o)) return false;
    b.add(L.att_o, o, x_, C, EPI_ADD);
    if (!b.run(*this, s)) return false;
    return ffn(s, l, si, so);
}

bool Engine::layer_v7(const SeqRun & s, int l, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int T = s.T, C = (int)m_->n_embed, H = (int)m_->H, S = (int)m_->S;
    LnMixArgs a = ln_mix_args(s, si + C, so + C, L.ln1_w, L.ln1_b);
    a.form = 1;
    // order r, w, k, v, a, g (rwkv_graph.inc:404-413)
    const DMat * cons[6] = {&L.att_r, &L.w1, &L.att_k, &L.att_v, &L.a1, &L.g1};
    a.n_out = 6;
    for (int n = 0; n < 6; n++) {
        a.mu[n] = L.x_rwkvag + (size_t)n * C;
        a.out[n] = A(s, n, *cons[n]);
    }
    const bool vlora = l != 0;
    ActBuf xv1;
    if (vlora) {
        xv1 = A(s, 9, L.v1);
        if (xv1.fmt == a.out[3].fmt) {
            xv1 = a.out[3];
            xv1.K = L.v1.K;
        } else {
            // second emission of xv in the LoRA's input format; mix kernels take <= 6 outputs,
            // so re-run the mix for this one vector
            LnMixArgs a2 = a;
            a2.n_out = 1;
            a2.mu[0] = a.mu[3];
            a2.out[0] = xv1;
            a2.carry_out = nullptr;
            if (!launch_ln_mix(stream_, a2, s.seg)) return false;
        }
    }
    if (!launch_ln_mix(stream_, a, s.seg)) return false;
    MMBatch b;
    ActBuf lw = A(s, 6, L.w2), la = A(s, 7, L.a2), lg = A(s, 8, L.g2);
    b.add(L.att_r, a.out[0], r_, C, EPI_STORE);
    b.add(L.att_k, a.out[2], k_, C, EPI_STORE);
    b.add(L.att_v, a.out[3], v_, C, EPI_STORE);
    b.add(L.w1, a.out[1], nullptr, 0, EPI_TANH, nullptr, nullptr, &lw);
    b.add(L.a1, a.out[4], nullptr, 0, EPI_STORE, nullptr, nullptr, &la);
    b.add(L.g1, a.out[5], nullptr, 0, EPI_SIGMOID, nullptr, nullptr, &lg);
    ActBuf lvv;
    if (vlora) {
        lvv = A(s, 10, L.v2);
        b.add(L.v1, xv1, nullptr, 0, EPI_STORE, nullptr, nullptr, &lvv);
    }
    if (!b.run(*this, s)) return false;
    if (l == 0) HIP_OK(hipMemcpyAsync(vfirst_, v_, (size_t)T * C * 4, hipMemcpyDeviceToDevice, stream_));
    b.add(L.w2, lw, w_, C, EPI_DECAY7, nullptr, L.w0);
    b.add(L.a2, la, a_, C, EPI_SIGMOID_BIAS, nullptr, L.a0);
    b.add(L.g2, lg, g_, C, EPI_STORE);
    if (vlora) b.add(L.v2, lvv, v_, C, EPI_VMIX7, vfirst_, L.v0);
    if (!b.run(*this, s)) return false;
    if (s.bs) return batch_att_tail(s, att7_args(L, si, so), 0, l, si, so);
    if (!launch_v7_prep(stream_, T, H, S, k_, a_, r_, L.k_k, L.k_a, L.r_k, nb_, bb_, bonus_)) return false;
    // the serial recurrence (bit-exact with decode), or behind the wkv_chunk_ switch the chunk-parallel
    // form (wkv7_chunk.hip; scratch in wkvc_)
    if (wkv_chunk_ && !s.seg && wkv7_chunked_supported(T, S, (int)s.bs)) {
        const size_t need = wkv7_chunked_scratch_floats(T, H);
        if (!grow(wkvc_, need, need, GRAPHS_NONE)) return false;
        if (!launch_wkv7_chunked(stream_, T, H, r_, w_, k_, v_, nb_, bb_, si + 2 * C, so + 2 * C, y_, wkvc_)) return false;
    } else if (!launch_wkv7(stream_, T, H, S, r_, w_, k_, v_, nb_, bb_, si + 2 * C, so + 2 * C, y_, s.seg)) {
        return false;
    }
    ActBuf o = A(s, 0, L.att_o);
    if (!launch_groupnorm(stream_, T, H, S, 64e-5f, y_, L.att_lnx_w, L.att_lnx_b, 2, g_, v_, bonus_, o)) return false;
    b.add(L.att_o, o, x_, C, EPI_ADD);
    if (!b.run(*this, s)) return false;
    return ffn(s, l, si, so);
}

// Layers [s.l0, s.l1) over s.T rows; l0 == 0 embeds the tokens into x_, otherwise x_ (and, v7, vfirst_)
// already hold the stream entering l0.  With s.head_out and l1 == n_layer the head runs: on the last token
// of a sequence, on every context of a batched step (scoring runs it over every token afterwards, score_chunk).
bool Engine::forward_range(const SeqRun & s) {
    last_decode_ = false;
    if (s.l0 == 0 && !launch_embed_ln(stream_, s.tok, s.T, m_->emb, m_->ln0_w, m_->ln0_b, x_)) return false;
    const size_t per_layer = layer_state_len();
    for (uint32_t l = s.l0; l < s.l1; l++) {
        const float * si = s.sin + l * per_layer;
        float * so = s.sout + l * per_layer;
        bool ok = false;
        switch (m_->major) {
            case 4: ok = layer_v4(s, (int)l, si, so); break;
            case 5: ok = layer_v5(s, (int)l, si, so); break;
            case 6: ok = layer_v6(s, (int)l, si, so); break;
            case 7: ok = layer_v7(s, (int)l, si, so); break;
        }
        if (!ok) return false;
    }
    if (!s.head_out || s.l1 != m_->n_layer) return true;
    if (s.rows) return head_rows(s, x_);
    return head_rows(seq_run(1, nullptr, nullptr, s.l1, s.l1, s.tok, s.head_out), x_ + (size_t)(s.T - 1) * m_->n_embed);
}

// rwkv_graph.inc:704-708 / :850-854: final LayerNorm + head over the h.T residual rows at x into
// h.head_out [h.T][n_vocab].  Never in token tiles, whatever h.tile_acts says of the layers: the head
// has no tile records (upload_mat), so its rows go as contexts (h.rows) or through k_mm.
bool Engine::head_rows(const SeqRun & h, const float * x) {
    ActBuf hin = A(0, m_->head);
    if (!launch_ln_emit(stream_, (int)m_->n_embed, x, m_->lnout_w, m_->lnout_b, hin, h.T)) return false;
    MMBatch b;
    b.add(m_->head, hin, h.head_out, (int)m_->n_vocab, EPI_STORE);
    return b.run(*this, h.T, h.rows, false);
}

}  // namespace rwkvmi
