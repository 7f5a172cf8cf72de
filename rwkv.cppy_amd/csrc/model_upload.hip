// model_upload.hip -- the model file's tensors repacked into the device layouts of common.hpp
// (DeviceModel, engine.hpp).  The weights are allocated once, recorded in DeviceModel::allocs and
// freed by free_model.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "engine.hpp"

namespace rwkvmi {

template <typename T>
static T * dalloc(DeviceModel & dm, size_t n) {
    void * p = nullptr;
    if (hipMalloc(&p, n * sizeof(T) + 16) != hipSuccess) return nullptr;
    dm.allocs.push_back(p);
    return (T *)p;
}

static float * upload_vec(DeviceModel & dm, const HostTensor * t) {
    if (!t) return nullptr;
    const uint64_t n = t->nel();
    std::vector<float> v(n);
    if (t->type == W_F32) {
        memcpy(v.data(), t->data.data(), n * 4);
    } else if (t->type == W_F16) {
        for (uint64_t i = 0; i < n; i++) {
            uint16_t h;
            memcpy(&h, t->data.data() + 2 * i, 2);
            v[i] = f16_to_f32(h);
        }
    } else {
        fprintf(stderr, "rwkv: parameter %s must be FP32/FP16\n", t->name.c_str());
        return nullptr;
    }
    float * d = dalloc<float>(dm, n);
    if (!d || hipMemcpy(d, v.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    dm.small_param_bytes += (double)n * 4;
    return d;
}

static float * upload_host_floats(DeviceModel & dm, const std::vector<float> & v) {
    float * d = dalloc<float>(dm, v.size());
    if (!d || hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    dm.small_param_bytes += (double)v.size() * 4;
    return d;
}

// Repack one ggml-order matrix ne=[K, M] into the device layout of common.hpp.
bool upload_mat(DeviceModel & dm, const HostTensor * t, DMat & out, bool count_bytes, bool is_head) {
    if (!t) return true;
    if (t->ndim != 2) {
        fprintf(stderr, "rwkv: %s: matrix expected\n", t->name.c_str());
        return false;
    }
    out.type = (int)t->type;
    out.gt = nullptr;
    out.mt = nullptr;
    out.K = (int)t->ne[0];
    out.M = (int)t->ne[1];
    const size_t M = out.M, K = out.K;
    if (t->type == W_F32 || t->type == W_F16) {
        const size_t bytes = t->data.size();
        uint8_t * d = dalloc<uint8_t>(dm, bytes);
        if (!d || hipMemcpy(d, t->data.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return false;
        out.qs = d;
    } else {
        if (K % 32) {
            fprintf(stderr, "rwkv: %s: K=%zu not a multiple of 32\n", t->name.c_str(), K);
            return false;
        }
        const size_t nb = K / 32, nblk = M * nb, bb = type_block_bytes(t->type);
        const size_t qbytes = (t->type == W_Q8_0) ? 32 : 16;
        std::vector<uint8_t> qs(nblk * qbytes);
        std::vector<uint32_t> qh;
        std::vector<uint16_t> sc16;
        std::vector<uint32_t> sc32;
        const bool q5 = t->type == W_Q5_0 || t->type == W_Q5_1;
        const bool one = t->type == W_Q4_1 || t->type == W_Q5_1;
        if (q5) qh.resize(nblk);
        if (one) sc32.resize(nblk); else sc16.resize(nblk);
        const uint8_t * src = t->data.data();
        for (size_t i = 0; i < nblk; i++) {
            const uint8_t * b = src + i * bb;
            uint16_t d, mm;
            memcpy(&d, b, 2);
            switch (t->type) {
                case W_Q4_0: sc16[i] = d; memcpy(&qs[i * 16], b + 2, 16); break;
                case W_Q4_1: memcpy(&mm, b + 2, 2); sc32[i] = (uint32_t)d | ((uint32_t)mm << 16); memcpy(&qs[i * 16], b + 4, 16); break;
                case W_Q5_0: sc16[i] = d; memcpy(&qh[i], b + 2, 4); memcpy(&qs[i * 16], b + 6, 16); break;
                case W_Q5_1: memcpy(&mm, b + 2, 2); sc32[i] = (uint32_t)d | ((uint32_t)mm << 16); memcpy(&qh[i], b + 4, 4); memcpy(&qs[i * 16], b + 8, 16); break;
                case W_Q8_0: sc16[i] = d; memcpy(&qs[i * 32], b + 2, 32); break;
                default: return false;
            }
        }
        uint8_t * dq = dalloc<uint8_t>(dm, qs.size());
        if (!dq || hipMemcpy(dq, qs.data(), qs.size(), hipMemcpyHostToDevice) != hipSuccess) return false;
        out.qs = dq;
        if (q5) {
            uint32_t * dh = dalloc<uint32_t>(dm, qh.size());
            if (!dh || hipMemcpy(dh, qh.data(), qh.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
            out.qh = dh;
        }
        if (one) {
            uint32_t * ds = dalloc<uint32_t>(dm, sc32.size());
            if (!ds || hipMemcpy(ds, sc32.data(), sc32.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
            out.sc = ds;
        } else {
            uint16_t * ds = dalloc<uint16_t>(dm, sc16.size());
            if (!ds || hipMemcpy(ds, sc16.data(), sc16.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return false;
            out.sc = ds;
        }
        // the same blocks again as sequence-GEMM tile records (common.hpp qg_*); the head never
        // takes that GEMM: it runs on one token, or over rows through the batched decode's forms
        // (eval_batch, score_chunk)
        if (!is_head) {
            const int wt = (int)t->type, R = qg_rows(wt);
            const size_t tiles = (M + R - 1) / R, rb = qg_w_bytes(wt);
            std::vector<uint8_t> gt(tiles * nb * rb, 0);
            for (size_t rt = 0; rt < tiles; rt++)
                for (size_t b = 0; b < nb; b++) {
                    uint8_t * rec = &gt[(rt * nb + b) * rb];
                    for (int r = 0; r < R && rt * R + r < M; r++) {
                        const size_t i = (rt * R + r) * nb + b;
                        int8_t * w8 = (int8_t *)rec;
                        for (int j = 0; j < 32; j++) {
                            int v;
                            if (wt == W_Q8_0) {
                                v = (int8_t)qs[i * 32 + j];
                            } else {
                                const uint8_t byte = qs[i * 16 + (j & 15)];
                                v = j < 16 ? (byte & 0xF) : (byte >> 4);
                                if (q5) v |= (int)((qh[i] >> j) & 1u) << 4;
                                if (wt == W_Q4_0) v -= 8;
                                if (wt == W_Q5_0) v -= 16;
                            }
                            w8[qg_w_off(r, j)] = (int8_t)v;
                        }
                        const float d = f16_to_f32(one ? (uint16_t)(sc32[i] & 0xFFFFu) : sc16[i]);
                        memcpy(rec + qg_w_d(wt) + r * 4, &d, 4);
                    }
                }
            uint8_t * dg = dalloc<uint8_t>(dm, gt.size());
            if (!dg || hipMemcpy(dg, gt.data(), gt.size(), hipMemcpyHostToDevice) != hipSuccess) return false;
            out.gt = dg;
            if (one) {  // the mins, block-major, for the m*s chain kernel
                const size_t MS = qm_stride((int)M);  // rows padded to k_qg_msum's 8-row loads
                std::vector<float> mt(nb * MS, 0.0f);
                for (size_t r = 0; r < M; r++)
                    for (size_t b = 0; b < nb; b++) mt[b * MS + r] = f16_to_f32((uint16_t)(sc32[r * nb + b] >> 16));
                float * dmt = dalloc<float>(dm, mt.size());
                if (!dmt || hipMemcpy(dmt, mt.data(), mt.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return false;
                out.mt = dmt;
            }
        }
    }
    if (count_bytes) {
        const double bytes = (double)type_nbytes(t->type, t->nel());
        const double flops = 2.0 * (double)M * (double)K;
        if (is_head) {
            dm.head_weight_bytes += bytes;
            dm.head_flops += flops;
        } else {
            dm.layer_weight_bytes += bytes;
            dm.layer_flops += flops;
        }
    }
    if (out.K > dm.kmax) dm.kmax = out.K;
    return true;
}

bool upload_model(const ModelFile & mf, DeviceModel & dm, uint32_t layer_begin, uint32_t layer_end) {
    dm.n_vocab = mf.header.n_vocab;
    dm.n_embed = mf.header.n_embed;
    dm.n_layer = mf.header.n_layer;
    dm.layer_lo = std::min(layer_begin, dm.n_layer);
    dm.layer_hi = std::min(layer_end, dm.n_layer);
    if (dm.layer_lo >= dm.layer_hi) {
        fprintf(stderr, "rwkv: empty layer range [%u, %u)\n", layer_begin, layer_end);
        return false;
    }
    const bool first = dm.layer_lo == 0, last = dm.layer_hi == dm.n_layer;
    dm.major = mf.arch_major;
    dm.minor = mf.arch_minor;
    dm.H = mf.head_count;
    dm.S = mf.head_size;
    const size_t C = dm.n_embed;
    dm.state_len = dm.major >= 5 ? C * (2 + (size_t)dm.S) * dm.n_layer : C * 5 * dm.n_layer;
    if (C % 64) {
        fprintf(stderr, "rwkv: n_embed %zu must be a multiple of 64\n", C);
        return false;
    }
    auto T = [&](const std::string & n) { return mf.find(n); };
    // a pipeline stage holds only its layers (+ embedding on the first, head on the last)
    if (first && (!upload_mat(dm, T("emb.weight"), dm.emb, false, false) ||
                  !(dm.ln0_w = upload_vec(dm, T("blocks.0.ln0.weight"))) ||
                  !(dm.ln0_b = upload_vec(dm, T("blocks.0.ln0.bias")))))
        return false;
    if (last && (!upload_mat(dm, T("head.weight"), dm.head, true, true) ||
                 !(dm.lnout_w = upload_vec(dm, T("ln_out.weight"))) || !(dm.lnout_b = upload_vec(dm, T("ln_out.bias")))))
        return false;
    dm.layers.resize(dm.n_layer);
    for (uint32_t i = dm.layer_lo; i < dm.layer_hi; i++) {
        DLayer & L = dm.layers[i];
        const std::string p = "blocks." + std::to_string(i) + ".";
        auto V = [&](const char * n) { return upload_vec(dm, T(p + n)); };
        auto Mt = [&](const char * n, DMat & d) { return upload_mat(dm, T(p + n), d, true, false); };
        bool ok = (L.ln1_w = V("ln1.weight")) && (L.ln1_b = V("ln1.bias")) && (L.ln2_w = V("ln2.weight")) &&
                  (L.ln2_b = V("ln2.bias"));
        ok = ok && Mt("att.key.weight", L.att_k) && Mt("att.value.weight", L.att_v) &&
             Mt("att.receptance.weight", L.att_r) && Mt("att.output.weight", L.att_o) &&
             Mt("ffn.key.weight", L.ffn_k) && Mt("ffn.value.weight", L.ffn_v);
        if (!ok) return false;
        dm.F = L.ffn_k.M;
        if (dm.major != 7 && !Mt("ffn.receptance.weight", L.ffn_r)) return false;
        if (dm.major == 4 || dm.major == 5) {
            ok = (L.att_mix_k = V("att.time_mix_k")) && (L.att_mix_v = V("att.time_mix_v")) &&
                 (L.att_mix_r = V("att.time_mix_r")) && (L.ffn_mix_k = V("ffn.time_mix_k")) &&
                 (L.ffn_mix_r = V("ffn.time_mix_r"));
            if (!ok) return false;
        }
        if (dm.major == 4) {
            if (!(L.att_first = V("att.time_first")) || !(L.att_decay = V("att.time_decay"))) return false;
        }
        if (dm.major >= 5) {
            if (!(L.att_lnx_w = V("att.ln_x.weight")) || !(L.att_lnx_b = V("att.ln_x.bias"))) return false;
        }
        if (dm.major == 5) {
            // wkv6 operands u and w expanded to [C] (5.1 repeats per head, rwkv_graph.inc:256-273)
            const HostTensor * dec = T(p + "att.time_decay");
            const HostTensor * fu = dm.minor >= 2 ? T(p + "att.time_faaaa") : T(p + "att.time_first");
            std::vector<float> u(C), w(C);
            const float * dd = (const float *)dec->data.data();
            const float * ff = (const float *)fu->data.data();
            if (dec->type != W_F32 || fu->type != W_F32) return false;
            for (int64_t h = 0; h < dm.H; h++)
                for (int64_t j = 0; j < dm.S; j++) {
                    u[h * dm.S + j] = dm.minor >= 2 ? ff[h * dm.S + j] : ff[h];
                    w[h * dm.S + j] = dm.minor >= 2 ? dd[h * dm.S + j] : dd[h];
                }
            if (!(L.att_u = upload_host_floats(dm, u)) || !(L.att_w = upload_host_floats(dm, w))) return false;
            if (dm.minor >= 2) {
                if (!(L.att_mix_g = V("att.time_mix_g")) || !Mt("att.gate.weight", L.att_g)) return false;
            }
        }
        if (dm.major == 6) {
            ok = (L.maa_x = V("att.time_maa_x")) && (L.maa[0] = V("att.time_maa_w")) && (L.maa[1] = V("att.time_maa_k")) &&
                 (L.maa[2] = V("att.time_maa_v")) && (L.maa[3] = V("att.time_maa_r")) && (L.maa[4] = V("att.time_maa_g")) &&
                 (L.maa_w2 = V("att.time_maa_w2")) && (L.att_u = V("att.time_faaaa")) && (L.decay6 = V("att.time_decay")) &&
                 (L.ffn_maa_k = V("ffn.time_maa_k")) && (L.ffn_maa_r = V("ffn.time_maa_r"));
            ok = ok && Mt("att.time_maa_w1", L.maa_w1) && Mt("att.time_decay_w1", L.decay_w1) &&
                 Mt("att.time_decay_w2", L.decay_w2) && Mt("att.gate.weight", L.att_g);
            if (!ok) return false;
            dm.maa_D = (int)T(p + "att.time_maa_w2")->ne[0];
            {
                const HostTensor * w2 = T(p + "att.time_maa_w2");
                if (w2->type != W_F32) return false;
                const size_t D = w2->ne[0], Cc = w2->ne[1];
                const float * src = (const float *)w2->data.data();
                std::vector<float> t(5 * D * Cc);
                for (size_t n = 0; n < 5; n++)
                    for (size_t c = 0; c < Cc; c++)
                        for (size_t i = 0; i < D; i++) t[(n * D + i) * Cc + c] = src[(n * Cc + c) * D + i];
                if (!(L.maa_w2t = upload_host_floats(dm, t))) return false;
                dm.small_param_bytes -= (double)t.size() * 4;  // same bytes as maa_w2, counted once
            }
            if (L.maa_w1.M != 5 * dm.maa_D) {
                fprintf(stderr, "rwkv: unexpected time_maa_w1 shape\n");
                return false;
            }
        }
        if (dm.major == 7) {
            ok = (L.x_rwkvag = V("att.x_rwkvag")) && (L.w0 = V("att.w0")) && (L.a0 = V("att.a0")) &&
                 (L.k_k = V("att.k_k")) && (L.k_a = V("att.k_a")) && (L.r_k = V("att.r_k")) && (L.ffn_x_k = V("ffn.x_k"));
            ok = ok && Mt("att.w1", L.w1) && Mt("att.w2", L.w2) && Mt("att.a1", L.a1) && Mt("att.a2", L.a2) &&
                 Mt("att.g1", L.g1) && Mt("att.g2", L.g2);
            if (ok && i != 0) ok = (L.v0 = V("att.v0")) && Mt("att.v1", L.v1) && Mt("att.v2", L.v2);
            if (!ok) return false;
        }
    }
    if (dm.H && dm.S > 64) {
        fprintf(stderr, "rwkv: head size %lld > 64 unsupported\n", (long long)dm.S);
        return false;
    }
    return hipDeviceSynchronize() == hipSuccess;
}

void free_model(DeviceModel & dm) {
    for (void * p : dm.allocs) (void)hipFree(p);
    dm.allocs.clear();
}

}  // namespace rwkvmi
