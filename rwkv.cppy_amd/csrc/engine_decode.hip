// engine_decode.hip -- the single-token forward: the fused decode program (kernels_decode.hip).
//
// Per layer:
//   v6: W1+LN (1) -> mix5 (1) -> r,k,v,g,Wd1 (1) -> decay tail+wkv+GN (1) -> Wo (1) -> FFN k,r+LN (1) -> FFN v (1)
//   v5: r,k,v,g+LN (1) -> wkv+GN (1) -> Wo (1) -> FFN (2)      v4: r,k,v+LN (1) -> wkv4 (1) -> Wo (1) -> FFN (2)
//   v7: r,k,v,LoRA-in+LN (1) -> LoRA-out (1) -> prep+wkv7+GN (1) -> Wo (1) -> FFN (2)
// Every fused launch (Engine::FUSE_*) has an unfused form of the same bits.  While a step is timed
// (timing_), the algorithmic bytes / flops of a launch that is not a matvec group are set just
// before it (kt_bytes_, kt_flops_; Engine::end hands them to the next launch).
#include <string.h>

#include <algorithm>

#include "engine.hpp"

namespace rwkvmi {

// One forward_decode call: the state buffers, the layer range and what one layer's launches leave
// for the next (or took over from the embedding).
struct DecodeRun {
    const float * sin;
    float * sout;
    uint32_t l0, l1;
    TokArg tok;            // the step's token id, for the launch that embeds it
    MaaDec emaa;          // v6, emb_in: layer 0's maa launch with the embedding LayerNorm inside
    bool emb_in = false;   // layer 0's first launch computes the embedding LayerNorm itself
    bool emb4_in = false;  // ... and it is v4's fused attention launch (with Wo: the Wo rows store x)
    bool maa_done = false; // this layer's maa ran in the previous layer's channel-mix launch (k_sig_maa)
};

// Builder for decode matvec groups.
struct MV {
    MVGroup g;
    MV() { memset(&g, 0, sizeof(g)); }
    MVEntry & next() { return g.e[g.n++]; }
    MVEntry & add(const DMat & W, float * y, int epi, const float * aux = nullptr, const float * bias = nullptr) {
        MVEntry & e = next();
        e.W = W;
        e.y = y;
        e.epi = epi;
        e.aux = aux;
        e.bias = bias;
        return e;
    }
};

static void src_lnmix(MVEntry & e, const float * x, const float * carry, const float * lnw, const float * lnb,
                      const float * mu, int form, float * carry_out = nullptr) {
    e.src = SRC_LNMIX;
    e.x = x;
    e.carry = carry;
    e.lnw = lnw;
    e.lnb = lnb;
    e.mu = mu;
    e.form = form;
    e.carry_out = carry_out;
}

// One LayerNorm + token shift shared by the entries of a layer's prologue launch: each entry mixes
// with its own mu; the entry given carry_out writes the new *_xx state.
struct LnMixSrc {
    const float * x, * carry, * lnw, * lnb;
    int form;
    void operator()(MVEntry & e, const float * mu, float * carry_out = nullptr) const {
        src_lnmix(e, x, carry, lnw, lnb, mu, form, carry_out);
    }
};

static void src_f32(MVEntry & e, const float * f) {
    e.src = SRC_F32;
    e.f = f;
}

static void src_act(MVEntry & e, const ActBuf & a) {
    e.src = SRC_ACT;
    e.act = a;
}

static double wbytes(const DMat & W) { return (double)type_nbytes((uint32_t)W.type, (uint64_t)W.M * W.K); }

// Wo matvec after a per-head attention kernel: its input is emitted by that kernel in Wo's format
// (q) when heads are whole 32-blocks, else read as fp32 by Wo's own prologue
template <class Att>
static MV wo_after(Att & a, const DMat & Wo, const ActBuf & q, float * x) {
    MV wo;
    MVEntry & e = wo.add(Wo, x, EPI_ADD);
    if (a.S >= 32) {
        a.yq = q;
        src_act(e, q);
    } else {
        src_f32(e, a.y);
    }
    return wo;
}

bool Engine::mv(MVGroup & g, hipStream_t st) {
    if (timing_) {
        // the group's single launch is timed by its own dispatch events (RK_LAUNCH, g_klt)
        double bytes = 0, flops = 0;
        for (int i = 0; i < g.n; i++) {
            const MVEntry & e = g.e[i];
            bytes += (double)type_nbytes((uint32_t)e.W.type, (uint64_t)e.W.M * e.W.K);
            bytes += e.src == SRC_ACT ? act_bytes(e.act, 1) : (double)e.W.K * 4 * (e.src == SRC_LNMIX ? 5 : 1);
            bytes += (double)e.W.M * 4 * ((e.epi == EPI_ADD || e.epi == EPI_SIGMUL_ADD || e.epi == EPI_VMIX7) ? 2 : 1);
            flops += 2.0 * e.W.M * e.W.K;
        }
        kt_bytes_ = bytes;
        kt_flops_ = flops;
    }
    return launch_mv_group(st ? st : stream_, g);
}

// v5/v6 attention core arguments of layer L (k_att6_dec; also Att6Fused::att), state slices si / so:
// fp32 y into y_ until the caller asks for an emission (yq).  Used by the decode program (bs == 0)
// and, with nb / bs added, by the batched step (batch_att_tail; bs = its state stride).
Att6Dec Engine::att6_args(const DLayer & L, const float * si, float * so, size_t bs) const {
    const int C = (int)m_->n_embed;
    Att6Dec a;
    memset(&a, 0, sizeof(a));
    a.H = (int)m_->H;
    a.S = (int)m_->S;
    a.r = r_;
    a.k = k_;
    a.v = v_;
    a.u = L.att_u;
    a.sin = si + 2 * C;
    a.sout = so + 2 * C;
    a.lnx_w = L.att_lnx_w;
    a.lnx_b = L.att_lnx_b;
    a.y = y_;
    a.yq.fmt = -1;
    if (m_->major == 5) {
        a.g = m_->minor >= 2 ? g_ : nullptr;
        a.w = L.att_w;
        a.eps = 1e-5f;
    } else {
        a.g = g_;
        a.wd2 = L.decay_w2;
        a.decay = L.decay6;
        a.eps = 64e-5f;
        // tanh(Wd1 . xw): one token's in dsmall_[0]; the batched step's, a row per context, in lora_
        a.dl = bs ? lora_ : dsmall_[0];
        a.ldd = bs ? L.decay_w1.M : 0;
    }
    return a;
}

// The same for v7 (k_att7_dec; also Att7Lora::att).
Att7Dec Engine::att7_args(const DLayer & L, const float * si, float * so) const {
    const int C = (int)m_->n_embed;
    Att7Dec a;
    memset(&a, 0, sizeof(a));
    a.H = (int)m_->H;
    a.S = (int)m_->S;
    a.r = r_;
    a.w = w_;
    a.k = k_;
    a.v = v_;
    a.a = a_;
    a.g = g_;
    a.k_k = L.k_k;
    a.k_a = L.k_a;
    a.r_k = L.r_k;
    a.sin = si + 2 * C;
    a.sout = so + 2 * C;
    a.lnx_w = L.att_lnx_w;
    a.lnx_b = L.att_lnx_b;
    a.y = y_;
    a.yq.fmt = -1;
    return a;
}

bool Engine::decode_att_v4(DecodeRun & d, uint32_t l) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed;
    const float * si = d.sin + l * layer_state_len();
    float * so = d.sout + l * layer_state_len();
    ActBuf o = A(0, L.att_o);
    MV c;  // Wo, when it is its own launch
    if ((fuse_ & FUSE_ATT4) && v4_att_fused_supported(C, L.att_r, L.att_k, L.att_v, o)) {
        // LN + r, k, v rows + WKV-4 in one launch, 8 channels per workgroup (mv_att4f.hip)
        if (timing_) {
            kt_bytes_ = 3 * wbytes(L.att_r) + 9.0 * C * 4 + 6.0 * C * 4 + C * 4.0 + act_bytes(o, 1);
            kt_flops_ = 6.0 * C * C;
        }
        V4WoFused wf;
        memset(&wf, 0, sizeof(wf));
        const bool wo_in = (fuse_ & FUSE_WO4) && L.att_o.type == L.att_r.type && C % 8 == 0;
        if (wo_in && d.emb4_in && l == 0) {
            wf.tok = d.tok;
            wf.emb = m_->emb;
            wf.ln0w = m_->ln0_w;
            wf.ln0b = m_->ln0_b;
            if (timing_) kt_bytes_ += (double)C * (m_->emb.type == W_F16 ? 2 : 4) + 2.0 * C * 4;
        }
        if (wo_in) {
            wf.wo = L.att_o;
            wf.xres = x_;
            wf.ygran = gran_.y;
            wf.h = handoff(l);
            if (timing_) {
                kt_bytes_ += wbytes(L.att_o) + 2.0 * C * 8 + 2.0 * C * 4;
                kt_flops_ += 2.0 * C * C;
            }
        }
        if (!launch_v4_att_fused(stream_, C, L.att_r, L.att_k, L.att_v, x_, si + C, so + C, L.ln1_w, L.ln1_b,
                                 L.att_mix_r, L.att_mix_k, L.att_mix_v, L.att_first, L.att_decay, si, so, o, y_,
                                 wo_in ? &wf : nullptr))
            return false;
        if (wo_in) return true;
        // y fp32: Wo quantizes it in its own prologue (the same Q8 bits as the emission)
        src_f32(c.add(L.att_o, x_, EPI_ADD), y_);
    } else {
        const LnMixSrc mix{x_, si + C, L.ln1_w, L.ln1_b, 0};
        MV b;
        mix(b.add(L.att_r, r_, EPI_SIGMOID), L.att_mix_r, so + C);
        mix(b.add(L.att_k, k_, EPI_STORE), L.att_mix_k);
        mix(b.add(L.att_v, v_, EPI_STORE), L.att_mix_v);
        if (!mv(b.g)) return false;
        if (!launch_wkv4(stream_, 1, C, r_, k_, v_, L.att_first, L.att_decay, si, so, o)) return false;
        src_act(c.add(L.att_o, x_, EPI_ADD), o);
    }
    return mv(c.g);
}

bool Engine::decode_att_v5(DecodeRun & d, uint32_t l) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed;
    const float * si = d.sin + l * layer_state_len();
    float * so = d.sout + l * layer_state_len();
    const LnMixSrc mix{x_, si + C, L.ln1_w, L.ln1_b, 0};
    MV b;
    mix(b.add(L.att_r, r_, EPI_STORE), L.att_mix_r, so + C);
    mix(b.add(L.att_k, k_, EPI_STORE), L.att_mix_k);
    mix(b.add(L.att_v, v_, EPI_STORE), L.att_mix_v);
    if (m_->minor >= 2) mix(b.add(L.att_g, g_, EPI_SILU), L.att_mix_g);
    if (!mv(b.g)) return false;
    Att6Dec a = att6_args(L, si, so, 0);
    MV c_wo = wo_after(a, L.att_o, A(6, L.att_o), x_);
    return launch_att6_dec(stream_, a) && mv(c_wo.g);
}

bool Engine::decode_att_v6(DecodeRun & d, uint32_t l) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed, H = (int)m_->H, S = (int)m_->S, D = m_->maa_D;
    const float * si = d.sin + l * layer_state_len();
    float * so = d.sout + l * layer_state_len();
    ActBuf outs[5] = {A(1, L.decay_w1), A(2, L.att_k), A(3, L.att_v), A(4, L.att_r), A(5, L.att_g)};
    if (d.maa_done) {
        d.maa_done = false;
    } else if (d.emb_in && l == 0) {
        if (timing_) {
            // + the embedding row, LN0 vectors and x written
            kt_bytes_ = wbytes(L.maa_w1) + 5.0 * D * C * 4 + 11.0 * C * 4 + C * 4.0 + 5 * act_bytes(outs[0], 1) +
                        (double)C * (m_->emb.type == W_F16 ? 2 : 4) + 3.0 * C * 4;
            kt_flops_ = 2.0 * L.maa_w1.M * L.maa_w1.K + 2.0 * 5 * D * C;
        }
        if (!launch_v6_maa_dec_emb(stream_, d.emaa)) return false;
    } else if (v6_maa_dec_supported(C, D, L.maa_w1.type) && !split_maa_) {
        // W1 rows + mix in one launch (mv_maa.hip)
        if (timing_) {
            // W1, W2 (fp32), x / carry / LN / maa vectors in, carry and 5 Q8 mixes out
            kt_bytes_ = wbytes(L.maa_w1) + 5.0 * D * C * 4 + 11.0 * C * 4 + C * 4.0 + 5 * act_bytes(outs[0], 1);
            kt_flops_ = 2.0 * L.maa_w1.M * L.maa_w1.K + 2.0 * 5 * D * C;
        }
        if (!launch_v6_maa_dec(stream_, C, D, L.maa_w1, x_, si + C, so + C, L.ln1_w, L.ln1_b, L.maa_x,
                               L.maa_w2t, L.maa, outs))
            return false;
    } else {
        MV b;
        src_lnmix(b.add(L.maa_w1, lora_, EPI_TANH), x_, si + C, L.ln1_w, L.ln1_b, L.maa_x, 1, so + C);
        if (!mv(b.g)) return false;
        if (!launch_v6_mix5_dec(stream_, C, D, so + C, si + C, lora_, L.maa_w2t, L.maa, outs))
            return false;
    }
    const int mats[5] = {3, 1, 2, 4, 0};  // r, k, v, g, w
    float * ys[5] = {r_, k_, v_, g_, dsmall_[0]};
    const DMat * Ws[5] = {&L.att_r, &L.att_k, &L.att_v, &L.att_g, &L.decay_w1};
    const int epis[5] = {EPI_STORE, EPI_STORE, EPI_STORE, EPI_SILU, EPI_TANH};
    Att6Dec a = att6_args(L, si, so, 0);
    MV c_wo = wo_after(a, L.att_o, A(6, L.att_o), x_);
    // r, k, v, g, Wd1 rows and the per-head attention in one launch (mv_att6f.hip), else
    // the k_mva group + k_att6_dec pair (the same bits)
    Att6Fused f;
    memset(&f, 0, sizeof(f));
    f.H = H;
    f.C = C;
    f.D = L.decay_w1.M;
    for (int i = 0; i < 4; i++) {
        f.W[i] = *Ws[i];
        f.x[i] = outs[mats[i]];
    }
    f.wd1 = L.decay_w1;
    f.xw = outs[mats[4]];
    f.att = a;
    f.gran = gran_.cleared;
    f.h = handoff(l);
    f.skip_wg = dbg_skip_gran_;
    // Wo inside the same launch (the head outputs handed to the non-reducer workgroups as
    // granules tagged by layer and state parity); else Wo is its own k_mva launch below
    bool wo_in = false;
    if ((fuse_ & FUSE_WO6) && (fuse_ & FUSE_ATT6)) {
        f.wo = L.att_o;
        f.xres = x_;
        f.ygran = gran_.y;
        f.wo_rows = wo_rows_;
        f.wo_prepoll = wo_prepoll_;
        wo_in = v6_att_fused_supported(f);
        if (!wo_in) {
            memset(&f.wo, 0, sizeof(f.wo));
            f.xres = nullptr;
            f.ygran = nullptr;
        }
    }
    if ((fuse_ & FUSE_ATT6) && v6_att_fused_supported(f)) {
        if (timing_) {
            // r, k, v, g, Wd1, Wd2 weights, their 5 Q8 inputs, the head state in and out,
            // u / decay / ln_x vectors, r / k / v / g / dl written (sc1) and read back, Wo's input out
            kt_bytes_ = 4 * wbytes(L.att_r) + wbytes(L.decay_w1) + wbytes(L.decay_w2) + 5 * act_bytes(outs[0], 1) +
                        2.0 * H * S * S * 4 + 4.0 * C * 4 + 2.0 * (4.0 * C + f.D) * 4 + act_bytes(a.yq, 1);
            kt_flops_ = 2.0 * (4.0 * C + f.D) * C + 2.0 * C * f.D;
            if (wo_in) {
                // Wo weights, the y granules (Q8 blocks) written and gathered, x read and written
                kt_bytes_ += wbytes(L.att_o) + 2.0 * KG_STRIDE * (C / 32) * 8 + 2.0 * C * 4 - act_bytes(a.yq, 1);
                kt_flops_ += 2.0 * C * C;
            }
        }
        // the co-resident layout when this context has the device to itself (choose_co)
        if (co_ && v6_att_co_supported(f) ? !launch_v6_att_co(stream_, f) : !launch_v6_att_fused(stream_, f))
            return false;
    } else {
        MV c;
        for (int i = 0; i < 5; i++) src_act(c.add(*Ws[i], ys[i], epis[i]), outs[mats[i]]);
        if (!mv(c.g)) return false;
        if (!launch_att6_dec(stream_, a)) return false;
    }
    return wo_in || mv(c_wo.g);
}

bool Engine::decode_att_v7(DecodeRun & d, uint32_t l) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed, H = (int)m_->H, S = (int)m_->S;
    const float * si = d.sin + l * layer_state_len();
    float * so = d.sout + l * layer_state_len();
    // order r, w, k, v, a, g of x_rwkvag (rwkv_graph.inc:404-413)
    const LnMixSrc mix{x_, si + C, L.ln1_w, L.ln1_b, 1};
    const float * mu = L.x_rwkvag;
    MV b;
    mix(b.add(L.att_r, r_, EPI_STORE), mu, so + C);
    mix(b.add(L.att_k, k_, EPI_STORE), mu + 2 * (size_t)C);
    mix(b.add(L.att_v, v_, EPI_STORE), mu + 3 * (size_t)C);
    // the LoRA first stages (F16 in the released files) as their own launch when their type
    // differs from r,k,v: one weight type per launch keeps the fixed-type kernels (fewer
    // registers, no per-entry type switch, no padded units)
    MV lb;
    MV & bl = L.w1.type == L.att_r.type ? b : lb;
    mix(bl.add(L.w1, dsmall_[0], EPI_TANH), mu + 1 * (size_t)C);
    mix(bl.add(L.a1, dsmall_[1], EPI_STORE), mu + 4 * (size_t)C);
    mix(bl.add(L.g1, dsmall_[2], EPI_SIGMOID), mu + 5 * (size_t)C);
    if (l != 0) mix(bl.add(L.v1, dsmall_[3], EPI_STORE), mu + 3 * (size_t)C);
    if (!mv(b.g)) return false;
    if (lb.g.n && !mv(lb.g)) return false;
    if (l == 0) HIP_OK(hipMemcpyAsync(vfirst_, v_, (size_t)C * 4, hipMemcpyDeviceToDevice, stream_));
    Att7Dec a = att7_args(L, si, so);
    MV c_wo = wo_after(a, L.att_o, A(6, L.att_o), x_);
    // LoRA second stages + attention in one launch (mv_att7f.hip), else the LoRA-out matvec
    // group + k_att7_dec (the same bits)
    Att7Lora f;
    memset(&f, 0, sizeof(f));
    f.att = a;
    f.W2[0] = L.w2;
    f.W2[1] = L.a2;
    f.W2[2] = L.g2;
    f.W2[3] = L.v2;
    for (int i = 0; i < 4; i++) f.lin[i] = dsmall_[i];
    f.bias[0] = L.w0;
    f.bias[1] = L.a0;
    f.bias[2] = nullptr;
    f.bias[3] = L.v0;
    f.vfirst = vfirst_;
    f.has_v = l != 0;
    if ((fuse_ & FUSE_ATT7) && att7_lora_supported(f)) {
        if (timing_) {
            double lb = wbytes(L.w2) + wbytes(L.a2) + wbytes(L.g2) + (l ? wbytes(L.v2) : 0.0);
            kt_bytes_ = lb + 2.0 * H * S * S * 4 + 12.0 * C * 4 + act_bytes(a.yq, 1);
            kt_flops_ = 2.0 * (L.w2.K + L.a2.K + L.g2.K + (l ? L.v2.K : 0)) * C;
        }
        if (!launch_att7_lora(stream_, f)) return false;
        v7_fused_lora_ = true;  // w, a, g and the mixed v never leave the launch (debug_copy)
    } else {
        MV c;
        src_f32(c.add(L.w2, w_, EPI_DECAY7, nullptr, L.w0), dsmall_[0]);
        src_f32(c.add(L.a2, a_, EPI_SIGMOID_BIAS, nullptr, L.a0), dsmall_[1]);
        src_f32(c.add(L.g2, g_, EPI_STORE), dsmall_[2]);
        if (l != 0) src_f32(c.add(L.v2, v_, EPI_VMIX7, vfirst_, L.v0), dsmall_[3]);
        if (!mv(c.g)) return false;
        if (!launch_att7_dec(stream_, a)) return false;
    }
    return mv(c_wo.g);
}

// Channel mixing.  v4/v5 (form 0), v6 (form 1): key and receptance; v7 (form 1): the key only
// (rwkv_graph.inc:484-543).
bool Engine::decode_ffn(DecodeRun & d, uint32_t l) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed;
    const float * si = d.sin + l * layer_state_len();
    float * so = d.sout + l * layer_state_len();
    const bool hasr = m_->major != 7;
    const int form = m_->major >= 6 ? 1 : 0;
    const float * muk = m_->major == 7 ? L.ffn_x_k : m_->major == 6 ? L.ffn_maa_k : L.ffn_mix_k;
    const float * mur = m_->major == 6 ? L.ffn_maa_r : L.ffn_mix_r;
    const LnMixSrc mix{x_, si, L.ln2_w, L.ln2_b, form};
    const ActBuf kin = A(0, L.ffn_v);
    // the key rows: relu^2 emitted as the value's input; writes the new ffn_xx
    auto key = [&](MVEntry & e) {
        e.W = L.ffn_k;
        e.epi = EPI_RELU_SQ;
        mix(e, muk, so);
        e.emit = 1;
        e.act_out = kin;
    };
    // the whole channel mix in one launch (mv_ffnf.hpp), else the key group + the value rows
    const bool ffco = co_ && (fuse_ & FUSE_FFNCO);
    if ((fuse_ & FUSE_FFN) || ffco) {
        FfnFused ff;
        memset(&ff, 0, sizeof(ff));
        ff.co = ffco;
        key(ff.e[0]);
        if (hasr) {
            MVEntry & fr = ff.e[1];
            fr.W = L.ffn_r;
            fr.epi = EPI_STORE;
            mix(fr, mur);
            ff.rg = gran_.r;
        }
        ff.wv = L.ffn_v;
        ff.x = x_;
        ff.kg = gran_.k;
        ff.h = handoff(l);
        const double wr = hasr ? wbytes(L.ffn_r) : 0.0;
        ff.wdelay = ffn_wdelay_ >= 0 ? ffn_wdelay_ : (int)std::min(2000.0, (wbytes(L.ffn_k) + wr) / 4e4);
        ff.prepoll = ffn_prepoll_;
        if (ff.co && !ffn_fused_supported(ff, form, hasr)) ff.co = 0;  // the ordered form, if on
        if ((ff.co || (fuse_ & FUSE_FFN)) && ffn_fused_supported(ff, form, hasr)) {
            if (timing_) {
                // with a receptance: + its rows' granules written and gathered and fr's C floats
                kt_bytes_ = wbytes(L.ffn_k) + wr + wbytes(L.ffn_v) + 5.0 * C * 4 + 2.0 * C * 4 +
                            (double)L.ffn_k.M / 32 * KG_STRIDE * 8 * 2 + (hasr ? 2.0 * C * 8 + C * 4.0 : 0.0);
                kt_flops_ = 2.0 * ((double)L.ffn_k.M * L.ffn_k.K + (hasr ? (double)L.ffn_r.M * L.ffn_r.K : 0.0) +
                                   (double)L.ffn_v.M * L.ffn_v.K);
            }
            return launch_ffn_fused(stream_, ff, form, hasr);
        }
    }
    MV b;
    MVEntry & ek = b.next();
    key(ek);
    // the receptance rows go with the value rows (k_mvsig) when the key launch can emit
    // their input: one launch of 224 workgroups for the key instead of 288 for key +
    // receptance (more workgroups than CUs), and fr_ never leaves the wave
    MVEntry sv, sr;
    bool sig = false;
    if (hasr) {
        memset(&sv, 0, sizeof(sv));
        memset(&sr, 0, sizeof(sr));
        sv.W = L.ffn_v;
        src_act(sv, kin);
        sv.y = x_;
        sv.epi = EPI_SIGMUL_ADD;
        sr.W = L.ffn_r;
        src_act(sr, A(7, L.ffn_r));
        sr.epi = EPI_STORE;
        sig = (fuse_ & FUSE_SIG) && L.ffn_r.type == L.ffn_k.type && mv_sigmul_supported(sv, sr);
        if (sig) {
            ek.mu2 = mur;
            ek.act2_out = sr.act;
        } else {
            mix(b.add(L.ffn_r, fr_, EPI_STORE), mur);
        }
    }
    if (!mv(b.g)) return false;
    if (!sig) {
        MV c;
        src_act(c.add(L.ffn_v, x_, hasr ? EPI_SIGMUL_ADD : EPI_ADD, hasr ? fr_ : nullptr), kin);
        return mv(c.g);
    }
    // co-resident: the next layer's maa in this launch (mv_sigmaa.hip), its x from granules
    if (co_ && (fuse_ & FUSE_SIGMAA) && m_->major == 6 && l + 1 < d.l1 && !split_maa_) {
        const DLayer & N = m_->layers[l + 1];
        const float * si1 = d.sin + (l + 1) * layer_state_len();
        float * so1 = d.sout + (l + 1) * layer_state_len();
        const ActBuf outs1[5] = {A(1, N.decay_w1), A(2, N.att_k), A(3, N.att_v), A(4, N.att_r), A(5, N.att_g)};
        SigMaa sm;
        memset(&sm, 0, sizeof(sm));
        mv_fill_hot(sv, sm.hv);
        mv_fill_hot(sr, sm.hr);
        sm.wtype = L.ffn_v.type;
        v6_maa_dec_args(sm.maa, C, m_->maa_D, N.maa_w1, x_, si1 + C, so1 + C, N.ln1_w, N.ln1_b, N.maa_x,
                        N.maa_w2t, N.maa, outs1);
        sm.nm = 5 * (C / 64);
        sm.xg = gran_.x;
        sm.h = handoff(l);
        if (sig_maa_supported(sm)) {
            if (timing_) {
                // + the maa's W1, W2 (fp32), LayerNorm vectors, carry and mixes; x granules out / in
                kt_bytes_ = wbytes(L.ffn_v) + wbytes(L.ffn_r) + act_bytes(kin, 1) + act_bytes(sr.act, 1) +
                            2.0 * C * 4 + wbytes(N.maa_w1) + 5.0 * m_->maa_D * C * 4 + 11.0 * C * 4 +
                            5 * act_bytes(outs1[0], 1) + 2.0 * C * 8;
                kt_flops_ = 2.0 * ((double)L.ffn_v.M * L.ffn_v.K + (double)L.ffn_r.M * L.ffn_r.K) +
                            2.0 * N.maa_w1.M * N.maa_w1.K + 2.0 * 5 * m_->maa_D * C;
            }
            d.maa_done = true;
            return launch_sig_maa(stream_, sm);
        }
    }
    if (timing_) {
        kt_bytes_ = wbytes(L.ffn_v) + wbytes(L.ffn_r) + act_bytes(kin, 1) + act_bytes(sr.act, 1) + 2.0 * C * 4;
        kt_flops_ = 2.0 * ((double)L.ffn_v.M * L.ffn_v.K + (double)L.ffn_r.M * L.ffn_r.K);
    }
    return launch_mv_sigmul(stream_, sv, sr);
}

// Layers [l0, l1) (embedding when l0 == 0, head when l1 == n_layer and logits).
bool Engine::forward_decode(const float * sin, float * sout, bool logits, const TokArg & tok, uint32_t l0, uint32_t l1) {
    const int C = (int)m_->n_embed;
    DecodeRun d;
    d.sin = sin;
    d.sout = sout;
    d.l0 = l0;
    d.l1 = std::min(l1, m_->n_layer);
    d.tok = tok;
    const bool emb_layer = l0 == 0 && d.l1 > 0 && (fuse_ & FUSE_EMBMAA);
    // v6: layer 0's maa launch computes the embedding LayerNorm itself (k_v6_maa_dec4 EMB: the same
    // bits as k_embed_ln; one launch and one boundary less per token)
    if (emb_layer && m_->major == 6 && !split_maa_) {
        const DLayer & F = m_->layers[0];
        const ActBuf o0[5] = {A(1, F.decay_w1), A(2, F.att_k), A(3, F.att_v), A(4, F.att_r), A(5, F.att_g)};
        v6_maa_dec_args(d.emaa, C, m_->maa_D, F.maa_w1, x_, sin + C, sout + C, F.ln1_w, F.ln1_b, F.maa_x, F.maa_w2t,
                        F.maa, o0);
        d.emaa.tok = tok;
        d.emaa.emb = m_->emb;
        d.emaa.ln0w = m_->ln0_w;
        d.emaa.ln0b = m_->ln0_b;
        d.emaa.xout = x_;
        d.emb_in = v6_maa_emb_supported(d.emaa);
    }
    // v4: the same inside layer 0's fused attention launch (with Wo fused: the Wo rows store x)
    if (emb_layer && m_->major == 4 && (fuse_ & FUSE_ATT4) && (fuse_ & FUSE_WO4)) {
        const DLayer & F = m_->layers[0];
        d.emb4_in = v4_att_fused_supported(C, F.att_r, F.att_k, F.att_v, A(0, F.att_o)) && F.att_o.type == F.att_r.type &&
                    C % 8 == 0 && (m_->emb.type == W_F16 || m_->emb.type == W_F32) && (int)m_->emb.K == C;
        d.emb_in = d.emb4_in;
    }
    if (l0 == 0 && !d.emb_in && !launch_embed_ln(stream_, tok, 1, m_->emb, m_->ln0_w, m_->ln0_b, x_)) return false;
    v7_fused_lora_ = false;
    for (uint32_t l = d.l0; l < d.l1; l++) {
        bool ok;
        switch (m_->major) {
            case 4: ok = decode_att_v4(d, l); break;
            case 5: ok = decode_att_v5(d, l); break;
            case 6: ok = decode_att_v6(d, l); break;
            default: ok = decode_att_v7(d, l); break;
        }
        if (!ok || !decode_ffn(d, l)) return false;
    }
    if (logits && d.l1 == m_->n_layer) {
        MV h;
        src_lnmix(h.add(m_->head, logits_, EPI_STORE), x_, nullptr, m_->lnout_w, m_->lnout_b, nullptr, 2);
        if (!mv(h.g)) return false;
    }
    return true;
}

}  // namespace rwkvmi
