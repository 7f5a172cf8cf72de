// engine.hip -- the engine core: lifetime, workspace, the per-version sequence / batched forward
// programs, the state I/O and the evaluation entry points on host or device state.  The
// single-token decode program: engine_decode.hip; batched decode and generation: engine_batch.hip;
// sampling, generation and scoring: engine_generate.hip; the weights: model_upload.hip.
//
// A token step is a fixed sequence of launches on the context's stream.  The T == 1 step
// is captured once into a hipGraph per (state parity, logits) and replayed, so decode pays
// no host launch cost.  Per-layer programs restate rwkv_graph.inc:
//   v4  :84-197 + FFN :484-511      v5  :199-292 + FFN :484-511
//   v6  :294-385 + FFN :513-531     v7  :387-482 + FFN :533-543
#include "engine.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <string>

#include "kernels.hpp"
#include "stamp.hpp"

namespace rwkvmi {

thread_local KLaunchTimer * g_klt = nullptr;
thread_local TokLaunch * g_tokl = nullptr;

#ifdef RWKV_STAMP
// Diagnostic builds (stamp.hpp): every kernel translation unit registers a setter for its copy
// of the device-side control block; the rings are dumped to $RWKV_STAMP_OUT when an engine dies.
static std::vector<void (*)(const StampCtl &)> & stamp_setters() {
    static std::vector<void (*)(const StampCtl &)> v;
    return v;
}
int stamp_register(void (*f)(const StampCtl &)) {
    stamp_setters().push_back(f);
    return 0;
}
static StampCtl g_host_stamp = {nullptr, nullptr};
static void stamp_init() {
    if (g_host_stamp.buf) return;
    const size_t bytes = (size_t)kStampCUs * kStampRing * 64;
    // the process's rings, never freed (static destructors run after the HIP runtime's)
    static auto & buf = *new DevBuf<unsigned long long>;
    static auto & ctr = *new DevBuf<unsigned>;
    if (!buf.alloc(bytes / 8) || !ctr.alloc(kStampCUs)) return;
    g_host_stamp = {buf, ctr};
    (void)hipMemset(g_host_stamp.buf, 0, bytes);
    (void)hipMemset(g_host_stamp.ctr, 0, kStampCUs * 4);
    for (auto f : stamp_setters()) f(g_host_stamp);
    (void)hipDeviceSynchronize();
}
static void stamp_dump() {
    const char * out = getenv("RWKV_STAMP_OUT");
    if (!out || !g_host_stamp.buf) return;
    const size_t bytes = (size_t)kStampCUs * kStampRing * 64;
    std::vector<unsigned long long> h(bytes / 8);
    if (hipMemcpy(h.data(), g_host_stamp.buf, bytes, hipMemcpyDeviceToHost) != hipSuccess) return;
    FILE * f = fopen(out, "wb");
    if (!f) return;
    // only the non-empty records: {t0, t1, t2, tag, x0..x3}
    for (size_t i = 0; i < h.size(); i += 8)
        if (h[i]) fwrite(&h[i], 8, 8, f);
    fclose(f);
}
#else
static void stamp_init() {}
static void stamp_dump() {}
#endif

// ------------------------------------------------------------------------- engine

__global__ void k_init_state(float * st, size_t n, int C, int v4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = 0.0f;
    if (v4) {
        const size_t in_layer = i % (5 * (size_t)C);
        if (in_layer >= 4 * (size_t)C) v = -1e30f;  // rwkv_eval.inc:224-241
    }
    st[i] = v;
}

Engine::~Engine() {
    if (stream_) (void)hipStreamSynchronize(stream_);
    release_device();
    stamp_dump();
    drop_graphs();
    drop_io_graphs();
    for (hipStream_t s : io_stream_)
        if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : io_ev_) (void)hipEventDestroy(e);
    if (io_entry_ev_) (void)hipEventDestroy(io_entry_ev_);
    drop_batch_graphs();
    // (device memory: the DevBuf members free themselves)
    if (htokens_) (void)hipHostFree(htokens_);
    if (herr_h_) (void)hipHostFree(herr_h_);
    collect_timing();
    for (hipEvent_t e : event_pool_) (void)hipEventDestroy(e);
    if (tok_event_) (void)hipEventDestroy(tok_event_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

bool GranuleMem::alloc(size_t C, size_t F) {
    const size_t kg = (size_t)KG_STRIDE * (F / 32);
    // cleared: 4 C + H D (D <= 128, H = C / 64)
    if (!cleared.alloc(6 * C) || !tagged.alloc(C + kg + C + C)) return false;
    HIP_OK(hipMemset(cleared, 0, cleared.size() * 8));
    HIP_OK(hipMemset(tagged, 0, tagged.size() * 8));
    y = tagged;
    k = y + C;
    r = k + kg;
    x = r + C;
    return true;
}

bool Engine::init() {
    HIP_OK(hipSetDevice(m_->device));
    stamp_init();
    {
        int cus = 0;
        HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m_->device));
        set_mv_device_cus(cus);
    }
    HIP_OK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&tok_event_, hipEventDisableTiming));
    HIP_OK(hipEventRecord(tok_event_, stream_));
    if (!dstate_[0].alloc(m_->state_len) || !dstate_[1].alloc(m_->state_len) || !logits_.alloc(m_->n_vocab)) {
        fprintf(stderr, "rwkv: device state and logits allocation failed\n");
        return false;
    }
    // in-launch hand-offs (handoff.hpp): the timeout flag is a host-mapped word, so checking it
    // costs the host one load after a sync
    HIP_OK(hipHostMalloc((void **)&herr_h_, 64, hipHostMallocMapped | hipHostMallocCoherent));
    *(volatile unsigned *)herr_h_ = 0;
    HIP_OK(hipHostGetDevicePointer((void **)&herr_d_, herr_h_, 0));
    if (!gran_.alloc(m_->n_embed, (size_t)std::max(m_->F, 32))) return false;
    // Per-context switches read when the context is created (each arm tested):
    const char * io = getenv("RWKV_MI355X_STATE_PIPELINE");  // 0: host state copied whole
    io_pipeline_ = !(io && io[0] == '0');
    const char * ic = getenv("RWKV_MI355X_IO_CHUNK");  // layers per chunk graph (host-state decode)
    io_chunk_ = ic ? std::max(1, atoi(ic)) : 4;
    const char * sm = getenv("RWKV_MI355X_SPLIT_MAA");  // 1: v6 decode W1 and mix as two launches
    split_maa_ = sm && sm[0] == '1';
    const char * df = getenv("RWKV_MI355X_DECODE_FUSION");  // mask of Engine::FUSE_* (default all)
    fuse_ = df ? (unsigned)strtoul(df, nullptr, 0) & FUSE_ALL : FUSE_DEFAULT | (m_->major == 4 ? FUSE_FFNCO : 0u);
    const char * wc = getenv("RWKV_MI355X_WKV_CHUNK");  // 1: chunk-parallel wkv6 (not bit-exact)
    wkv_chunk_ = wc && wc[0] == '1';
    // the fused decode prologues hold LayerNorm inputs in registers up to n_embed 4096
    if (m_->n_embed > 4096 || m_->n_embed % 64) generic_decode_ = true;
    return ensure_workspace(1) && init_state(dstate_[0]);
}

void Engine::drop_graphs() {
    for (auto & pc : graphs_)
        for (auto & pl : pc)
            for (TokGraph & g : pl) g.destroy();
}

void Engine::TokGraph::destroy() {
    if (ge) (void)hipGraphExecDestroy(ge);
    if (g) (void)hipGraphDestroy(g);
    ge = nullptr;
    g = nullptr;
    node = nullptr;
    args.clear();
}

// The next replay embeds t: nothing to do while the node already holds it (generation: every
// step reads the word the sampler wrote), else the node's argument block is replaced -- host work
// only; replays already enqueued keep the arguments they were launched with.
bool Engine::TokGraph::set_tok(const TokArg & t) {
    if (!node) {
        fprintf(stderr, "rwkv: a decode graph without its token node\n");
        return false;
    }
    TokArg cur;
    memcpy(&cur, args.data() + off, sizeof(cur));
    if (cur.ptr == t.ptr && cur.imm == t.imm && cur.id == t.id) return true;
    memcpy(args.data() + off, &t, sizeof(t));
    void * argv[1] = {args.data()};
    p.kernelParams = argv;
    const hipError_t e = hipGraphExecKernelNodeSetParams(ge, node, &p);
    p.kernelParams = nullptr;
    HIP_OK(e);
    return true;
}

// Contexts of this process with decode work queued per device (a context counts once from its
// first decode launch until it synchronises its stream).  The co-resident v6 attention layout
// (mv_att6c.hip) is safe only while its launches cannot share the compute units with another
// context's waiting launches: a context picks it when the count is 1 (itself).  Two contexts that
// claim at once both see 2; a context that picks it keeps the count until its launches finished.
static std::atomic<int> g_dev_claims[64];

void Engine::claim_device() {
    if (claimed_) return;
    claimed_ = true;
    g_dev_claims[m_->device & 63].fetch_add(1);
}

void Engine::release_device() {
    if (!claimed_) return;
    claimed_ = false;
    g_dev_claims[m_->device & 63].fetch_sub(1);
}

bool Engine::choose_co() {
    claim_device();
    bool co = co_knob_ == 1 || (co_knob_ < 0 && co_ok_ && g_dev_claims[m_->device & 63].load() == 1);
    // the co-resident forms: the v6 attention launch (with its Wo) and the channel mix's
    const bool att6 = (fuse_ & FUSE_ATT6) && (fuse_ & FUSE_WO6), sigmaa = (fuse_ & FUSE_SIGMAA) && (fuse_ & FUSE_SIG);
    co = co && ((m_->major == 6 && (att6 || sigmaa)) || (fuse_ & FUSE_FFNCO));
    // (both layouts hand y to Wo as the same Q8-block granules under the same tags: a switch needs
    // no clearing)
    co_ = co;
    co_pending_ += co;
    return co;
}

bool Engine::settle(unsigned graphs) {
    HIP_OK(hipStreamSynchronize(stream_));
    if (graphs & GRAPHS_DECODE) drop_graphs();
    if (graphs & GRAPHS_IO) drop_io_graphs();
    if (graphs & GRAPHS_BATCH) drop_batch_graphs();
    return true;
}

bool Workspace::alloc(size_t cap, size_t C, size_t kmax, size_t H) {
    bool ok = true;
    for (auto * b : {&x_, &xa_, &sx_, &r_, &k_, &v_, &g_, &w_, &y_, &a_, &nb_, &bb_, &vfirst_, &fr_})
        ok = ok && b->alloc(cap * C);
    ok = ok && lora_.alloc(cap * kmax) && bonus_.alloc(cap * H);
    for (auto & b : dsmall_) ok = ok && b.alloc(kmax);
    ok = ok && dtokens_.alloc(cap);
    for (auto & s : slots_) {
        const size_t n = cap * kmax, nbk = n / 32 + 1;
        // sequence-GEMM token tiles: whole QG_TOK-token tiles, records of up to qg_a_bytes(true)
        const size_t ttiles = (cap + QG_TOK - 1) / QG_TOK;
        ok = ok && s.q.alloc(n) && s.d.alloc(nbk) && s.s.alloc(nbk) && s.qsum.alloc(nbk) && s.h.alloc(n) && s.f.alloc(n) &&
             s.tq.alloc(ttiles * (kmax / 32 + 1) * qg_a_bytes(true));
    }
    return ok;
}

bool Engine::ensure_workspace(int T) {
    if ((size_t)T <= dtokens_.size()) return true;
    if (!settle(GRAPHS_ALL)) return false;
    // until every allocation below has succeeded the workspace counts as absent (empty buffers),
    // so a failed grow can never leave a capacity that points at freed or missing buffers
    static_cast<Workspace &>(*this) = Workspace{};
    HIP_OK(hipEventSynchronize(tok_event_));
    if (htokens_) {
        (void)hipHostFree(htokens_);
        htokens_ = nullptr;
    }
    const size_t cap = doubled(1, (size_t)T), C = m_->n_embed;
    Workspace ws;
    uint32_t * htok = nullptr;
    if (!ws.alloc(cap, C, std::max<size_t>((size_t)m_->kmax, C), (size_t)std::max<int64_t>(1, m_->H)) ||
        hipHostMalloc((void **)&htok, cap * 4, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();  // clear the sticky out-of-memory status: later launches check it
        fprintf(stderr, "rwkv: device workspace allocation for %zu tokens failed\n", cap);
        return false;  // the workspace stays absent: the next call retries the allocation
    }
    static_cast<Workspace &>(*this) = std::move(ws);
    htokens_ = htok;
    return true;
}

// the pinned token buffer may still feed the previous (async) call's copy
bool Engine::stage_tokens(const uint32_t * tokens, size_t n) {
    HIP_OK(hipEventSynchronize(tok_event_));
    memcpy(htokens_, tokens, n * 4);
    HIP_OK(hipMemcpyAsync(dtokens_, htokens_, n * 4, hipMemcpyHostToDevice, stream_));
    HIP_OK(hipEventRecord(tok_event_, stream_));
    return true;
}

bool Engine::copy_logits(float * host_out) {
    HIP_OK(hipMemcpyAsync(host_out, logits_, (size_t)m_->n_vocab * 4, hipMemcpyDeviceToHost, stream_));
    return true;
}

bool Engine::init_state(float * st, size_t n) {
    if (!n) n = m_->state_len;
    RK_LAUNCH(k_init_state, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream_, st, n,
                       (int)m_->n_embed, m_->major == 4 ? 1 : 0);
    HIP_OK(hipGetLastError());
    return true;
}

ActBuf Engine::Aview(int slot, int K, int fmt) const {
    const ActSlot & s = slots_[slot];
    ActBuf a;
    a.fmt = fmt;
    a.K = K;
    a.f = s.f;
    a.h = s.h;
    a.q = s.q;
    a.d = s.d;
    a.s = s.s;
    a.qsum = s.qsum;
    a.tq = s.tq;
    a.tiled = tile_acts_ && (fmt == A_Q8_0 || fmt == A_Q8_1);
    return a;
}

ActBuf Engine::A(int slot, const DMat & W) const { return Aview(slot, W.K, act_fmt_for(W.type)); }

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
    bool run(Engine & eng, int T) {
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
            if (!eng.mm_launch(g, type)) return false;
        }
        e.clear();
        return true;
    }
};

void Engine::set_timing(bool on) {
    (void)hipStreamSynchronize(stream_);
    collect_timing();
    timing_ = on;
    if (on) stats_.clear();
}

// Sequence matmuls on quantized weights go to the int8-MFMA GEMM; entries that only emit get
// a scratch y, and emission is a separate quantization pass (same bits as k_mm's epilogue).
bool Engine::mm_dispatch(MMGroup & g, int wtype) {
    // batched decode (bs_ > 0): the decode matvec over the contexts (k_mvb; k_mm for shapes it
    // does not cover -- the same bits); from batch_gemm_min_ contexts on, the quantized matmuls
    // take the int8-MFMA sequence GEMM on token tiles instead (tile_acts_; also the same bits)
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
    if (bs_ && !(tile_acts_ && wtype_quantized(wtype))) {
        bool launched = false;
        // float weights (the F16 head, LoRA) over 16+ contexts: the f32-MFMA form, same bits
        if (!launch_fmm_group(stream_, g, wtype, &launched)) return false;
        if (launched) return true;
        if (!launch_mvb_group(stream_, g, wtype, &launched)) return false;
        if (launched) return true;
        return launch_mm_group(stream_, g, wtype);
    }
    if (g.T < 2 || !wtype_quantized(wtype) || use_mm_) return launch_mm_group(stream_, g, wtype);
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

bool Engine::mm_launch(MMGroup & g, int wtype) {
    if (!timing_) return mm_dispatch(g, wtype);
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
    // kernel class = the template instantiation rocprofv3 reports: k_mm<WF, RPW, NT>
    const bool mfma = g.T >= 2 && wtype_quantized(wtype) && !use_mm_ && (!bs_ || tile_acts_);
    const std::string name = mfma ? "k_qgemm<" + std::to_string(wtype) + ">"
                           : bs_ ? "k_mvb<" + std::to_string(wtype) + ">"
                                  : "k_mm<" + std::to_string(wtype) + ", " + (emit ? "8" : "2") + ", " + (g.T == 1 ? "1" : "4") + ">";
    const int si = add_stat(name);
    hipEvent_t a, b;
    if (event_pool_.size() >= 2) {
        a = event_pool_.back();
        event_pool_.pop_back();
        b = event_pool_.back();
        event_pool_.pop_back();
    } else {
        HIP_OK(hipEventCreate(&a));
        HIP_OK(hipEventCreate(&b));
    }
    HIP_OK(hipEventRecord(a, stream_));
    const bool ok = mm_dispatch(g, wtype);
    HIP_OK(hipEventRecord(b, stream_));
    pending_.push_back(Pending{si, a, b, bytes, flops});
    return ok;
}

int Engine::add_stat(const std::string & name) {
    for (size_t i = 0; i < stats_.size(); i++)
        if (stats_[i].name == name) return (int)i;
    stats_.push_back(KernelStat{name});
    return (int)stats_.size() - 1;
}

void Engine::collect_timing() {
    for (auto & p : pending_) {
        float ms = 0;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            KernelStat & s = stats_[p.stat];
            s.total_ms += ms;
            s.total_bytes += p.bytes;
            s.total_flops += p.flops;
            s.launches++;
        }
        event_pool_.push_back(p.a);
        event_pool_.push_back(p.b);
    }
    pending_.clear();
}

const std::vector<KernelStat> & Engine::stats() {
    (void)hipStreamSynchronize(stream_);
    collect_timing();
    return stats_;
}

// The LayerNorm + token shift + mix launch of a sequence / batched layer, up to its outputs:
// carry_in / carry_out = the layer's *_xx state row (context t's at + t * bs_ in a batched step)
LnMixArgs Engine::ln_mix_args(int T, const float * carry_in, float * carry_out, const float * lnw, const float * lnb) const {
    LnMixArgs a;
    memset(&a, 0, sizeof(a));
    a.T = T;
    a.C = (int)m_->n_embed;
    a.x = x_;
    a.carry_in = carry_in;
    a.carry_out = carry_out;
    a.bs = bs_;
    a.lnw = lnw;
    a.lnb = lnb;
    return a;
}

bool Engine::ffn(int l, int T, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed;
    LnMixArgs a = ln_mix_args(T, si, so, L.ln2_w, L.ln2_b);  // ffn_xx at layer offset 0
    MMBatch b;
    if (m_->major == 7) {
        // rwkv_graph.inc:533-543
        a.form = 1;
        a.n_out = 1;
        a.mu[0] = L.ffn_x_k;
        a.out[0] = A(0, L.ffn_k);
        if (!launch_ln_mix(stream_, a, seg_)) return false;
        ActBuf kin = A(1, L.ffn_v);
        b.add(L.ffn_k, A(0, L.ffn_k), nullptr, 0, EPI_RELU_SQ, nullptr, nullptr, &kin);
        if (!b.run(*this, T)) return false;
        b.add(L.ffn_v, kin, x_, C, EPI_ADD);
        return b.run(*this, T);
    }
    // v4/v5: rwkv_graph.inc:484-511 (form 0); v6: :513-531 (form 1)
    a.form = m_->major == 6 ? 1 : 0;
    a.n_out = 2;
    a.mu[0] = m_->major == 6 ? L.ffn_maa_k : L.ffn_mix_k;
    a.mu[1] = m_->major == 6 ? L.ffn_maa_r : L.ffn_mix_r;
    a.out[0] = A(0, L.ffn_k);
    a.out[1] = A(1, L.ffn_r);
    if (!launch_ln_mix(stream_, a, seg_)) return false;
    ActBuf kin = A(2, L.ffn_v);
    b.add(L.ffn_r, A(1, L.ffn_r), fr_, C, EPI_STORE);
    b.add(L.ffn_k, A(0, L.ffn_k), nullptr, 0, EPI_RELU_SQ, nullptr, nullptr, &kin);
    if (!b.run(*this, T)) return false;
    b.add(L.ffn_v, kin, x_, C, EPI_SIGMUL_ADD, fr_);
    return b.run(*this, T);
}

static bool launch_att_dec(hipStream_t st, const Att6Dec & a) { return launch_att6_dec(st, a); }
static bool launch_att_dec(hipStream_t st, const Att7Dec & a) { return launch_att7_dec(st, a); }

// Batched decode (bs_ > 0): the attention core of every context is the decode kernel itself (one
// workgroup per head and context, k_att6_dec / k_att7_dec); its output goes to Wo's input `o`
// (emitted by the kernel when heads are whole quantization blocks, else fp32 y_ converted).
// The rest of such a layer: a = att6_args / att7_args, then Wo (input slot wo_slot) and the FFN.
template <class Att>
bool Engine::batch_att_tail(Att a, int wo_slot, int l, int T, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed;
    ActBuf o = A(wo_slot, L.att_o);
    a.nb = T;
    a.bs = bs_;
    if (a.S >= 32) a.yq = o;
    if (!launch_att_dec(stream_, a)) return false;
    if (a.S < 32 && !launch_act_from_f32(stream_, y_, T, C, o)) return false;
    MMBatch b;
    b.add(L.att_o, o, x_, C, EPI_ADD);
    if (!b.run(*this, T)) return false;
    return ffn(l, T, si, so);
}

bool Engine::layer_v4(int l, int T, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed;
    LnMixArgs a = ln_mix_args(T, si + C, so + C, L.ln1_w, L.ln1_b);
    a.form = 0;
    a.n_out = 3;
    a.mu[0] = L.att_mix_k;
    a.mu[1] = L.att_mix_v;
    a.mu[2] = L.att_mix_r;
    a.out[0] = A(0, L.att_k);
    a.out[1] = A(1, L.att_v);
    a.out[2] = A(2, L.att_r);
    if (!launch_ln_mix(stream_, a, seg_)) return false;
    MMBatch b;
    b.add(L.att_r, A(2, L.att_r), r_, C, EPI_SIGMOID);
    b.add(L.att_k, A(0, L.att_k), k_, C, EPI_STORE);
    b.add(L.att_v, A(1, L.att_v), v_, C, EPI_STORE);
    if (!b.run(*this, T)) return false;
    ActBuf o = A(3, L.att_o);
    if (!launch_wkv4(stream_, T, C, r_, k_, v_, L.att_first, L.att_decay, si, so, o, (int)bs_, seg_)) return false;
    b.add(L.att_o, o, x_, C, EPI_ADD);
    if (!b.run(*this, T)) return false;
    return ffn(l, T, si, so);
}

// v5/v6 sequence wkv: the serial recurrence (k_wkv6_s64, bit-exact with decode; a prefill's packed
// chunk always: its segmented form), or behind the wkv_chunk_ switch the chunk-parallel form (RA / KB in the v7-only nb_ / bb_ buffers, free during a
// v5/v6 layer; the chunk matrices and states in wkvc_, grown on demand)
bool Engine::wkv6(int T, int H, int S, const float * u, const float * w, int wpt, const float * sin, float * sout) {
    if (wkv_chunk_ && !seg_ && wkv6_chunked_supported(T, S, (int)bs_)) {
        const size_t need = wkv6_chunked_scratch_floats(T, H);
        if (!grow(wkvc_, need, need, GRAPHS_NONE)) return false;
        return launch_wkv6_chunked(stream_, T, H, k_, v_, r_, u, w, wpt, sin, sout, y_, nb_, bb_, wkvc_);
    }
    return launch_wkv6(stream_, T, H, S, k_, v_, r_, u, w, wpt, sin, sout, y_, seg_);
}

bool Engine::layer_v5(int l, int T, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed, H = (int)m_->H, S = (int)m_->S;
    const bool v52 = m_->minor >= 2;
    LnMixArgs a = ln_mix_args(T, si + C, so + C, L.ln1_w, L.ln1_b);
    a.form = 0;
    a.n_out = v52 ? 4 : 3;
    a.mu[0] = L.att_mix_k;
    a.mu[1] = L.att_mix_v;
    a.mu[2] = L.att_mix_r;
    a.out[0] = A(0, L.att_k);
    a.out[1] = A(1, L.att_v);
    a.out[2] = A(2, L.att_r);
    if (v52) {
        a.mu[3] = L.att_mix_g;
        a.out[3] = A(3, L.att_g);
    }
    if (!launch_ln_mix(stream_, a, seg_)) return false;
    MMBatch b;
    b.add(L.att_r, A(2, L.att_r), r_, C, EPI_STORE);
    b.add(L.att_k, A(0, L.att_k), k_, C, EPI_STORE);
    b.add(L.att_v, A(1, L.att_v), v_, C, EPI_STORE);
    if (v52) b.add(L.att_g, A(3, L.att_g), g_, C, EPI_SILU);
    if (!b.run(*this, T)) return false;
    if (bs_) return batch_att_tail(att6_args(L, si, so), 4, l, T, si, so);
    if (!wkv6(T, H, S, L.att_u, L.att_w, 0, si + 2 * C, so + 2 * C)) return false;
    ActBuf o = A(4, L.att_o);
    if (!launch_groupnorm(stream_, T, H, S, 1e-5f, y_, L.att_lnx_w, L.att_lnx_b, v52 ? 1 : 0, g_, nullptr, nullptr, o))
        return false;
    b.add(L.att_o, o, x_, C, EPI_ADD);
    if (!b.run(*this, T)) return false;
    return ffn(l, T, si, so);
}

bool Engine::layer_v6(int l, int T, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed, H = (int)m_->H, S = (int)m_->S, D = m_->maa_D;
    LnMixArgs a = ln_mix_args(T, si + C, so + C, L.ln1_w, L.ln1_b);
    a.form = 1;
    a.n_out = 1;
    a.mu[0] = L.maa_x;
    a.out[0] = A(0, L.maa_w1);
    a.out_xa = xa_;
    a.out_sx = sx_;
    if (!launch_ln_mix(stream_, a, seg_)) return false;
    MMBatch b;
    b.add(L.maa_w1, A(0, L.maa_w1), lora_, 5 * D, EPI_TANH);
    if (!b.run(*this, T)) return false;
    // order w, k, v, r, g (rwkv_graph.inc:336-346)
    ActBuf outs[5] = {A(1, L.decay_w1), A(2, L.att_k), A(3, L.att_v), A(4, L.att_r), A(5, L.att_g)};
    // batched decode: the decode kernel's per-(mix, channel) arithmetic over the contexts; from
    // batch_gemm_min_ contexts on (token-tile outputs) the sequence kernel's f32-MFMA form over the
    // contexts as tokens -- W2 read once per 64 contexts instead of once per context, same bits
    if ((bs_ && !tile_acts_) ? !launch_v6_mix5_dec(stream_, C, D, xa_, nullptr, lora_, L.maa_w2t, L.maa, outs, T, sx_)
                             : !launch_v6_mix5(stream_, T, C, D, lora_, L.maa_w2t, L.maa, xa_, sx_, outs))
        return false;
    ActBuf dl = A(6, L.decay_w2);
    // decay tail by threads (k_att6_dec's rows) when Wd2 is quantized; dl fp32 then reuses lora_
    // (consumed by mix5 above)
    const int DD = L.decay_w2.K;  // decay LoRA width (64 for the released checkpoints)
    const bool dseq = v6_decay_seq_supported(L.decay_w2.type, DD) && L.decay_w1.M == DD;
    if (bs_) {
        // decode's split: decay W1 (tanh) with r,k,v,g; the LoRA tail, wkv and GroupNorm per head
        b.add(L.att_r, outs[3], r_, C, EPI_STORE);
        b.add(L.att_k, outs[1], k_, C, EPI_STORE);
        b.add(L.att_v, outs[2], v_, C, EPI_STORE);
        b.add(L.att_g, outs[4], g_, C, EPI_SILU);
        b.add(L.decay_w1, outs[0], lora_, L.decay_w1.M, EPI_TANH);
        if (!b.run(*this, T)) return false;
        return batch_att_tail(att6_args(L, si, so), 7, l, T, si, so);
    }
    b.add(L.att_r, outs[3], r_, C, EPI_STORE);
    b.add(L.att_k, outs[1], k_, C, EPI_STORE);
    b.add(L.att_v, outs[2], v_, C, EPI_STORE);
    b.add(L.att_g, outs[4], g_, C, EPI_SILU);
    if (dseq) b.add(L.decay_w1, outs[0], lora_, DD, EPI_TANH);
    else b.add(L.decay_w1, outs[0], nullptr, 0, EPI_TANH, nullptr, nullptr, &dl);
    if (!b.run(*this, T)) return false;
    if (dseq) {
        if (!launch_v6_decay_seq(stream_, T, C, L.decay_w2, lora_, L.decay6, w_)) return false;
    } else {
        b.add(L.decay_w2, dl, w_, C, EPI_DECAY6, nullptr, L.decay6);
        if (!b.run(*this, T)) return false;
    }
    if (!wkv6(T, H, S, L.att_u, w_, 1, si + 2 * C, so + 2 * C)) return false;
    ActBuf o = A(7, L.att_o);
    if (!launch_groupnorm(stream_, T, H, S, 64e-5f, y_, L.att_lnx_w, L.att_lnx_b, 1, g_, nullptr, nullptr, o)) return false;
    b.add(L.att_o, o, x_, C, EPI_ADD);
    if (!b.run(*this, T)) return false;
    return ffn(l, T, si, so);
}

bool Engine::layer_v7(int l, int T, const float * si, float * so) {
    const DLayer & L = m_->layers[l];
    const int C = (int)m_->n_embed, H = (int)m_->H, S = (int)m_->S;
    LnMixArgs a = ln_mix_args(T, si + C, so + C, L.ln1_w, L.ln1_b);
    a.form = 1;
    // order r, w, k, v, a, g (rwkv_graph.inc:404-413)
    const DMat * cons[6] = {&L.att_r, &L.w1, &L.att_k, &L.att_v, &L.a1, &L.g1};
    a.n_out = 6;
    for (int n = 0; n < 6; n++) {
        a.mu[n] = L.x_rwkvag + (size_t)n * C;
        a.out[n] = A(n, *cons[n]);
    }
    const bool vlora = l != 0;
    ActBuf xv1;
    if (vlora) {
        xv1 = A(9, L.v1);
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
            if (!launch_ln_mix(stream_, a2, seg_)) return false;
        }
    }
    if (!launch_ln_mix(stream_, a, seg_)) return false;
    MMBatch b;
    ActBuf lw = A(6, L.w2), la = A(7, L.a2), lg = A(8, L.g2);
    b.add(L.att_r, a.out[0], r_, C, EPI_STORE);
    b.add(L.att_k, a.out[2], k_, C, EPI_STORE);
    b.add(L.att_v, a.out[3], v_, C, EPI_STORE);
    b.add(L.w1, a.out[1], nullptr, 0, EPI_TANH, nullptr, nullptr, &lw);
    b.add(L.a1, a.out[4], nullptr, 0, EPI_STORE, nullptr, nullptr, &la);
    b.add(L.g1, a.out[5], nullptr, 0, EPI_SIGMOID, nullptr, nullptr, &lg);
    ActBuf lvv;
    if (vlora) {
        lvv = A(10, L.v2);
        b.add(L.v1, xv1, nullptr, 0, EPI_STORE, nullptr, nullptr, &lvv);
    }
    if (!b.run(*this, T)) return false;
    if (l == 0) {
        HIP_OK(hipMemcpyAsync(vfirst_, v_, (size_t)T * C * 4, hipMemcpyDeviceToDevice, stream_));
    }
    b.add(L.w2, lw, w_, C, EPI_DECAY7, nullptr, L.w0);
    b.add(L.a2, la, a_, C, EPI_SIGMOID_BIAS, nullptr, L.a0);
    b.add(L.g2, lg, g_, C, EPI_STORE);
    if (vlora) b.add(L.v2, lvv, v_, C, EPI_VMIX7, vfirst_, L.v0);
    if (!b.run(*this, T)) return false;
    if (bs_) return batch_att_tail(att7_args(L, si, so), 0, l, T, si, so);
    if (!launch_v7_prep(stream_, T, H, S, k_, a_, r_, L.k_k, L.k_a, L.r_k, nb_, bb_, bonus_)) return false;
    // the serial recurrence (bit-exact with decode), or behind the wkv_chunk_ switch the chunk-parallel
    // form (wkv7_chunk.hip; scratch in wkvc_)
    if (wkv_chunk_ && !seg_ && wkv7_chunked_supported(T, S, (int)bs_)) {
        const size_t need = wkv7_chunked_scratch_floats(T, H);
        if (!grow(wkvc_, need, need, GRAPHS_NONE)) return false;
        if (!launch_wkv7_chunked(stream_, T, H, r_, w_, k_, v_, nb_, bb_, si + 2 * C, so + 2 * C, y_, wkvc_)) return false;
    } else if (!launch_wkv7(stream_, T, H, S, r_, w_, k_, v_, nb_, bb_, si + 2 * C, so + 2 * C, y_, seg_)) {
        return false;
    }
    ActBuf o = A(0, L.att_o);
    if (!launch_groupnorm(stream_, T, H, S, 64e-5f, y_, L.att_lnx_w, L.att_lnx_b, 2, g_, v_, bonus_, o)) return false;
    b.add(L.att_o, o, x_, C, EPI_ADD);
    if (!b.run(*this, T)) return false;
    return ffn(l, T, si, so);
}

bool Engine::forward(int T, const float * sin, float * sout, bool logits) {
    if (T == 1 && !generic_decode_) return forward_decode(sin, sout, logits);
    return forward_range(T, sin, sout, 0, m_->n_layer, logits);
}

// Layers [l0, l1) over T tokens; l0 == 0 embeds the tokens into x_, otherwise x_ (and, v7,
// vfirst_) already hold the stream entering l0.  Head on the last token when l1 == n_layer.
bool Engine::forward_range(int T, const float * sin, float * sout, uint32_t l0, uint32_t l1, bool logits) {
    const size_t C = m_->n_embed;
    last_decode_ = false;
    // one token of its own sequence: the step's id (tok_arg); batches and packed prompts read dtokens_
    const TokArg tk = T == 1 && !bs_ && !seg_ ? tok_arg() : TokArg{dtokens_.get(), 0u, 0u};
    if (l0 == 0 && !launch_embed_ln(stream_, tk, T, m_->emb, m_->ln0_w, m_->ln0_b, x_)) return false;
    const size_t per_layer = layer_state_len();
    // layer matmuls run over all T tokens: Q8 activations go straight into GEMM tiles
    tile_acts_ = T >= 2 && !use_mm_ && (!bs_ || T >= batch_gemm_min_);
    for (uint32_t l = l0; l < l1; l++) {
        const float * si = sin + l * per_layer;
        float * so = sout + l * per_layer;
        bool ok = false;
        switch (m_->major) {
            case 4: ok = layer_v4((int)l, T, si, so); break;
            case 5: ok = layer_v5((int)l, T, si, so); break;
            case 6: ok = layer_v6((int)l, T, si, so); break;
            case 7: ok = layer_v7((int)l, T, si, so); break;
            default: break;
        }
        if (!ok) {
            tile_acts_ = false;
            return false;
        }
    }
    // the head runs on the last token only (batched decode: on every context; scoring runs it over
    // every token afterwards, score_chunk)
    tile_acts_ = false;
    if (logits && l1 == m_->n_layer) {
        const int rows = bs_ ? T : 1;
        return head_rows(x_ + (size_t)(T - rows) * C, rows, head_out_ ? head_out_ : logits_);
    }
    return true;
}

// rwkv_graph.inc:704-708 / :850-854
bool Engine::head_rows(const float * x, int rows, float * out) {
    ActBuf hin = A(0, m_->head);
    if (!launch_ln_emit(stream_, (int)m_->n_embed, x, m_->lnout_w, m_->lnout_b, hin, rows)) return false;
    MMBatch b;
    b.add(m_->head, hin, out, (int)m_->n_vocab, EPI_STORE);
    return b.run(*this, rows);
}

// KLaunchTimer (common.hpp): while a decode step is timed, every RK_LAUNCH takes an event pair
// bound to its dispatch; the algorithmic bytes / flops set by the caller just before (kt_bytes_)
// go to the first launch after them.
bool Engine::begin(hipEvent_t * a, hipEvent_t * b) {
    if (event_pool_.size() < 2) {
        hipEvent_t x, y;
        if (hipEventCreate(&x) != hipSuccess) return false;
        if (hipEventCreate(&y) != hipSuccess) {
            (void)hipEventDestroy(x);
            return false;
        }
        event_pool_.push_back(x);
        event_pool_.push_back(y);
    }
    *a = event_pool_.back();
    event_pool_.pop_back();
    *b = event_pool_.back();
    event_pool_.pop_back();
    kt_a_ = *a;
    kt_b_ = *b;
    return true;
}

void Engine::end(const char * kernel) {
    // "(k_mva<WFIX, Rv, Uv>)" -> "k_mva"
    std::string n(kernel);
    while (!n.empty() && (n[0] == '(' || n[0] == ' ')) n.erase(0, 1);
    const size_t cut = n.find_first_of("<) ");
    if (cut != std::string::npos) n.resize(cut);
    pending_.push_back(Pending{add_stat(n), kt_a_, kt_b_, kt_bytes_, kt_flops_});
    kt_bytes_ = kt_flops_ = 0;
}

// Runs T tokens from dstate_[cur_] (ping-pong), chunked by the workspace capacity.
bool Engine::run_tokens(const uint32_t * tokens, size_t T, bool want_logits) {
    // a failed call restores the ping-pong parity it started with, so the next state upload
    // (every rwkv_eval with state_in, rwkv_mi355x_state_upload) lands where the next step reads;
    // the device state's contents after a failure are unspecified (re-upload it)
    const int cur0 = cur_;
    logits_valid_ = false;
    if (!run_tokens_impl(tokens, T, want_logits)) {
        step_imm_ = false;
        (void)hipStreamSynchronize(stream_);
        (void)gran_.clear_tagged(stream_);  // a replay runs at the same parity (GranuleMem::clear_tagged)
        (void)hipStreamSynchronize(stream_);
        release_device();
        cur_ = cur0;
        return false;
    }
    logits_valid_ = want_logits;
    return true;
}

bool Engine::run_tokens_impl(const uint32_t * tokens, size_t T, bool want_logits) {
    size_t done = 0;
    while (done < T) {
        const size_t n = std::min(T - done, kChunkMax);
        const bool last = done + n == T;
        if (!ensure_workspace((int)n)) return false;
        // one token: its id goes by value in the argument block of the step's first launch (TokArg;
        // a graph replay: set_tok), and nothing is enqueued to deliver it -- hipStreamWriteValue32,
        // which stood here, runs as a kernel of the runtime (__amd_rocclr_streamOpsWrite) on this
        // stream: 4.3 us and one more kernel boundary per token
        step_imm_ = tokens && n == 1;
        step_id_ = step_imm_ ? tokens[done] : 0;
        if (!tokens) {
            // generate: the sampler enqueued just before this step writes dtokens_[0]
        } else if (n > 1 && !stage_tokens(tokens + done, n)) {
            return false;
        }
        // scoring: a one-token chunk's step writes logits_ (score_chunk reads it), longer chunks get
        // their head from score_chunk
        const bool lg = score_ ? n == 1 : last && want_logits;
        last_decode_ = n == 1 && !generic_decode_;
        const bool co = last_decode_ ? choose_co() : (co_ = false);
        if (timing_) {
            // eager launches; a decode step's kernels each carry a dispatch-bound event pair
            // (RK_LAUNCH through g_klt), the sequence path's matmul groups an event pair around
            // the group (mm_launch)
            if (n == 1) g_klt = this;
            const bool ok = forward((int)n, dstate_[cur_], dstate_[cur_ ^ 1], lg);
            g_klt = nullptr;
            if (!ok) return false;
        } else if (n == 1 && use_graphs_) {
            TokGraph & tg = graphs_[co][cur_][lg ? 1 : 0];
            if (!tg.ge && !capture_tok(tg, [&] { return forward(1, dstate_[cur_], dstate_[cur_ ^ 1], lg); })) return false;
            if (!tg.set_tok(tok_arg())) return false;
            HIP_OK(hipGraphLaunch(tg.ge, stream_));
        } else {
            if (!forward((int)n, dstate_[cur_], dstate_[cur_ ^ 1], lg)) return false;
        }
        step_imm_ = false;
        if (score_ && !score_chunk(done, n, last)) return false;
        // a step without the fused decode flips the parity (GranuleMem::clear_tagged)
        if (n > 1 || generic_decode_) HIP_OK(gran_.clear_tagged(stream_));
        // tokens buffer is reused by the next chunk: wait before overwriting the pinned copy
        if (!last) HIP_OK(hipStreamSynchronize(stream_));
        cur_ ^= 1;
        done += n;
    }
    return true;
}

bool Engine::state_upload(const float * state) {
    logits_valid_ = false;
    if (state) {
        HIP_OK(hipMemcpyAsync(dstate_[cur_], state, m_->state_len * 4, hipMemcpyHostToDevice, stream_));
        io_h2d_ += m_->state_len * 4.0;
        return true;
    }
    return init_state(dstate_[cur_]);
}

bool Engine::state_download(float * state) {
    HIP_OK(hipMemcpyAsync(state, dstate_[cur_], m_->state_len * 4, hipMemcpyDeviceToHost, stream_));
    HIP_OK(hipStreamSynchronize(stream_));
    io_d2h_ += m_->state_len * 4.0;
    return handoff_check();
}

// The host layout is per layer contiguous (rwkv_graph.inc:545-606), so layers [l0, l1) are one
// range of the device-resident state: only that range crosses PCIe.
bool Engine::state_upload_layers(const float * slice, uint32_t l0, uint32_t l1) {
    const size_t per = layer_state_len(), off = (size_t)l0 * per, n = (size_t)(l1 - l0) * per;
    logits_valid_ = false;
    if (slice) {
        HIP_OK(hipMemcpyAsync(dstate_[cur_] + off, slice, n * 4, hipMemcpyHostToDevice, stream_));
        io_h2d_ += n * 4.0;
        return true;
    }
    return init_state(dstate_[cur_] + off, n);
}

bool Engine::state_download_layers(float * slice, uint32_t l0, uint32_t l1) {
    const size_t per = layer_state_len(), off = (size_t)l0 * per, n = (size_t)(l1 - l0) * per;
    HIP_OK(hipMemcpyAsync(slice, dstate_[cur_] + off, n * 4, hipMemcpyDeviceToHost, stream_));
    HIP_OK(hipStreamSynchronize(stream_));
    io_d2h_ += n * 4.0;
    return handoff_check();
}

bool Engine::sync() {
    HIP_OK(hipStreamSynchronize(stream_));
    return handoff_check();
}

// Every waiting loop of an in-launch hand-off gives up after spin_max_ passes and sets the
// host-mapped flag (handoff.hpp: gran_wait, handoff_fail).  Every call that synchronises the
// stream reads it: a set flag fails that call (the reference's error convention: false +
// RWKV_ERROR_CTX, rwkv_error_handling.inc:1-54).  A producer that arrives after the timeout leaves
// its granule tagged, which the next launch would read as its own value, so every granule is
// cleared before the flag is re-armed.
bool Engine::handoff_check() {
    // called after the stream has drained: nothing of this context is queued any more
    release_device();
    const bool co_seen = co_pending_ > 0;
    co_pending_ = 0;
    if (*(volatile unsigned *)herr_h_ == 0) return true;
    logits_valid_ = false;
    (void)hipStreamSynchronize(stream_);
    gran_.clear_all(stream_);
    (void)hipStreamSynchronize(stream_);
    *(volatile unsigned *)herr_h_ = 0;
    if (co_seen && co_knob_ < 0) {
        // the co-resident layout lost its co-residency (another process's launches on the device):
        // this context uses the ordered layout from now on; a synchronous one-token call re-runs
        co_ok_ = false;
        co_retry_ = true;
        fprintf(stderr, "rwkv: in-launch hand-off timed out in the co-resident attention layout; using the ordered layout\n");
    } else {
        fprintf(stderr, "rwkv: in-launch hand-off timed out: the evaluation's results are invalid\n");
    }
    return false;
}

bool Engine::debug_set(const char * name, long long value) {
    if (!name) return false;
    const std::string n(name);
    // "delay_us": a kernel that holds the context's stream for value us, enqueued now (no sync) --
    // the timing pass puts one ahead of each eager decode step, so the host queues the step's
    // launches before the GPU reaches them and they run back to back, as in a graph replay (and as
    // under a profiler, whose slower launches would otherwise leave the GPU idle between kernels)
    if (n == "delay_us") return value > 0 && value <= 100000 && launch_delay(stream_, (int)value);
    if (n == "skip_granule") dbg_skip_gran_ = (int)value;
    else if (n == "spin_max") spin_max_ = value > 0 ? (unsigned)std::min<long long>(value, 0xffffffffLL) : (1u << 20);
    else if (n == "wkv_chunk") wkv_chunk_ = value != 0;
    else if (n == "generic_decode") generic_decode_ = value != 0 || m_->n_embed > 4096;
    else if (n == "graphs") use_graphs_ = value != 0;
    // the packing cap of prefill_batch in tokens (tests reach row splits at small shapes); <= 0: the default
    else if (n == "prefill_chunk" && value <= (long long)kChunkMax) prefill_chunk_ = value <= 0 ? kChunkMax : (size_t)value;
    else if (n == "co_mode" && value >= -1 && value <= 1) co_knob_ = (int)value;
    else if (n == "decode_fusion")  // -1: the default for this model
        fuse_ = value < 0 ? FUSE_DEFAULT | (m_->major == 4 ? FUSE_FFNCO : 0u) : (unsigned)value & FUSE_ALL;
    else if (n == "wo_rows" && (value == 4 || value == 8)) wo_rows_ = (int)value;
    else if (n == "wo_prepoll") wo_prepoll_ = value != 0;
    else if (n == "ffn_wdelay" && value >= -1 && value <= 10000) ffn_wdelay_ = (int)value;
    else if (n == "ffn_prepoll") ffn_prepoll_ = value != 0;
    else return false;
    // the decode graphs captured the old values; the new decode program may lack a hand-off
    // (GranuleMem::clear_tagged)
    (void)hipStreamSynchronize(stream_);
    drop_graphs();
    drop_io_graphs();
    (void)gran_.clear_tagged(stream_);
    (void)hipStreamSynchronize(stream_);
    return true;
}

// ---------------------------------------------------------------- ABI decode with host state
// rwkv_eval's contract hands the whole recurrent state over as host buffers on every call
// (rwkv_eval.inc:2-22): 13 MB each way for v6-1B6, ~0.5 ms of PCIe against a 0.82 ms decode.
// The decode runs as io_chunk_-layer graphs instead of one, so the copies of one chunk's state
// slice overlap the other chunks' kernels: the host uploads chunk c+1 (copy stream 0) while the
// GPU runs chunk c, and downloads chunk c-1 (copy stream 1) while the GPU runs chunk c.  This
// works for ordinary pageable buffers too: a pageable hipMemcpyAsync holds the HOST until its
// bytes are staged, but the chunk graphs are already queued, so the GPU keeps computing.  The
// bytes moved and every result are exactly those of the one-graph path.
// Both caller state buffers page-locked (registered with / allocated by the HIP runtime)?  NULL
// buffers count as page-locked (no copy).
static bool host_pinned(const void * p) {
    if (!p) return true;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

bool Engine::pinned_io(const float * state_in, const float * state_out) {
    return host_pinned(state_in) && host_pinned(state_out);
}

bool Engine::eval_host_chunked(uint32_t token, const float * state_in, float * state_out, float * logits_out) {
    const uint32_t NL = m_->n_layer, K = (uint32_t)io_chunk_, NC = (NL + K - 1) / K;
    const size_t per_layer = layer_state_len();
    logits_valid_ = false;
    if (!ensure_workspace(1)) return false;
    if (!io_stream_[0]) {
        // copy streams (high-priority queues and CU-masked download queues measured no better)
        HIP_OK(hipStreamCreateWithFlags(&io_stream_[0], hipStreamNonBlocking));
        HIP_OK(hipStreamCreateWithFlags(&io_stream_[1], hipStreamNonBlocking));
        HIP_OK(hipEventCreateWithFlags(&io_entry_ev_, hipEventDisableTiming));
    }
    // the copy streams start behind everything already queued on stream_ (an earlier
    // rwkv_mi355x_eval_device(sync = false) may still be writing dstate_[cur_], the upload target)
    HIP_OK(hipEventRecord(io_entry_ev_, stream_));
    for (auto & st : io_stream_) HIP_OK(hipStreamWaitEvent(st, io_entry_ev_, 0));
    if (io_ev_.size() < 2 * (size_t)NC) {
        for (hipEvent_t e : io_ev_) (void)hipEventDestroy(e);
        io_ev_.assign(2 * NC, nullptr);
        for (auto & e : io_ev_) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const bool lg = logits_out != nullptr;
    const bool co = choose_co();
    std::vector<TokGraph> & gs = io_graphs_[co][cur_][lg ? 1 : 0];
    if (gs.size() != NC) {
        for (TokGraph & g : gs) g.destroy();
        gs.assign(NC, TokGraph{});
    }
    float * din = dstate_[cur_], * dout = dstate_[cur_ ^ 1];
    // the id by value, as in run_tokens_impl: chunk 0's first launch consumes it, no other chunk's
    // graph holds one
    step_imm_ = true;
    step_id_ = token;
    for (uint32_t c = 0; c < NC; c++) {
        if (gs[c].ge) continue;
        const bool ok = capture_tok(gs[c], [&] { return forward_decode(din, dout, lg, c * K, (c + 1) * K); });
        if (!ok) {
            step_imm_ = false;
            return false;
        }
    }
    const TokArg tk = tok_arg();
    step_imm_ = false;
    if (!gs[0].set_tok(tk)) return false;
    auto slice = [&](uint32_t c, size_t & off, size_t & bytes) {
        const uint32_t l0 = c * K, l1 = std::min(NL, l0 + K);
        off = l0 * per_layer;
        bytes = (l1 - l0) * per_layer * 4;
    };
    hipEvent_t * in_ev = io_ev_.data(), * done_ev = io_ev_.data() + NC;
    size_t off, bytes;
    last_decode_ = true;
    if (!state_in && !init_state(din)) return false;
    auto upload = [&](uint32_t c) -> bool {
        slice(c, off, bytes);
        HIP_OK(hipMemcpyAsync(din + off, state_in + off, bytes, hipMemcpyHostToDevice, io_stream_[0]));
        HIP_OK(hipEventRecord(in_ev[c], io_stream_[0]));
        io_h2d_ += (double)bytes;
        return true;
    };
    auto download = [&](uint32_t c) -> bool {
        slice(c, off, bytes);
        HIP_OK(hipStreamWaitEvent(io_stream_[1], done_ev[c], 0));
        HIP_OK(hipMemcpyAsync(state_out + off, dout + off, bytes, hipMemcpyDeviceToHost, io_stream_[1]));
        io_d2h_ += (double)bytes;
        return true;
    };
    auto launch = [&](uint32_t c) -> bool {
        if (state_in) HIP_OK(hipStreamWaitEvent(stream_, in_ev[c], 0));
        HIP_OK(hipGraphLaunch(gs[c].ge, stream_));
        HIP_OK(hipEventRecord(done_ev[c], stream_));
        return true;
    };
    // Page-locked caller buffers: every copy call returns at once, so all uploads are queued first
    // (they only read din, which no chunk graph writes), then the graphs, then the downloads.  A
    // rocprofv3 memory-copy trace of the interleaved order showed each upload starting only when
    // the previous chunk's kernels ended: the download call issued between them held the host
    // until its chunk had finished.  Pageable buffers: a copy call returns once the runtime has
    // staged the bytes, so the interleaved order keeps the GPU fed; downloads lag two chunks.
    if (pinned_io(state_in, state_out)) {
        for (uint32_t c = 0; state_in && c < NC; c++)
            if (!upload(c)) return false;
        for (uint32_t c = 0; c < NC; c++)
            if (!launch(c)) return false;
        for (uint32_t c = 0; state_out && c < NC; c++)
            if (!download(c)) return false;
    } else {
        if (state_in && !upload(0)) return false;
        for (uint32_t c = 0; c < NC; c++) {
            if (!launch(c)) return false;
            if (state_in && c + 1 < NC && !upload(c + 1)) return false;
            if (state_out && c >= 2 && !download(c - 2)) return false;
        }
        for (uint32_t c = NC >= 2 ? NC - 2 : 0; state_out && c < NC; c++)
            if (!download(c)) return false;
    }
    if (logits_out && !copy_logits(logits_out)) return false;
    HIP_OK(hipStreamSynchronize(io_stream_[1]));
    HIP_OK(hipStreamSynchronize(io_stream_[0]));
    HIP_OK(hipStreamSynchronize(stream_));
    if (!handoff_check()) return false;
    cur_ ^= 1;
    logits_valid_ = lg;
    return true;
}

void Engine::drop_io_graphs() {
    for (auto & pc : io_graphs_)
        for (auto & p : pc)
            for (auto & v : p) {
                for (TokGraph & g : v) g.destroy();
                v.clear();
            }
}

bool Engine::eval(const uint32_t * tokens, size_t T, const float * state_in, float * state_out, float * logits_out) {
    co_retry_ = false;
    const int pend0 = co_pending_;
    if (eval_once(tokens, T, state_in, state_out, logits_out)) return true;
    // a co-resident layout timeout in this call's own launches (none of an earlier asynchronous
    // call was pending): the inputs are untouched (host state_in, or the device state this call
    // started from), so the call runs again, in the ordered layout
    if (!co_retry_ || pend0 > 0) return false;
    co_retry_ = false;
    return eval_once(tokens, T, state_in, state_out, logits_out);
}

bool Engine::eval_once(const uint32_t * tokens, size_t T, const float * state_in, float * state_out, float * logits_out) {
    HIP_OK(hipSetDevice(m_->device));
    // one token with host state: chunked decode, copies overlapped (needs graphs; timing and the
    // generic decode path keep the whole-state copies)
    if (T == 1 && io_pipeline_ && use_graphs_ && !timing_ && !generic_decode_ && (state_in || state_out)) {
        const int cur0 = cur_;
        if (eval_host_chunked(tokens[0], state_in, state_out, logits_out)) return true;
        (void)hipStreamSynchronize(stream_);
        cur_ = cur0;
        return false;
    }
    if (!state_upload(state_in)) return false;
    const int cur0 = cur_;
    if (!run_tokens(tokens, T, logits_out != nullptr)) return false;
    if (logits_out && !copy_logits(logits_out)) return false;
    if (state_out) {
        HIP_OK(hipMemcpyAsync(state_out, dstate_[cur_], m_->state_len * 4, hipMemcpyDeviceToHost, stream_));
        io_d2h_ += m_->state_len * 4.0;
    }
    HIP_OK(hipStreamSynchronize(stream_));
    if (!handoff_check()) {
        cur_ = cur0;
        return false;
    }
    return true;
}

// One layer-pipeline stage step on the device-resident state: x_io / vfirst_io
// are device buffers [T][C] on this engine's device carrying the residual stream (and v7's
// layer-0 values) between stages.  Synchronous: on return x_io holds this stage's output.
bool Engine::eval_layers(const uint32_t * tokens, size_t T, uint32_t l0, uint32_t l1, float * x_io, float * vfirst_io,
                         bool want_logits, float * logits_out, bool sync) {
    HIP_OK(hipSetDevice(m_->device));
    co_ = false;  // pipeline stages: the ordered layouts only
    if (!ensure_workspace((int)T)) return false;
    const size_t bytes = T * (size_t)m_->n_embed * 4;
    if (l0 == 0) {
        if (!stage_tokens(tokens, T)) return false;
    } else {
        HIP_OK(hipMemcpyAsync(x_, x_io, bytes, hipMemcpyDeviceToDevice, stream_));
        if (m_->major == 7) HIP_OK(hipMemcpyAsync(vfirst_, vfirst_io, bytes, hipMemcpyDeviceToDevice, stream_));
    }
    const bool lg = (want_logits || logits_out) && l1 == m_->n_layer;
    logits_valid_ = false;
    if (!forward_range((int)T, dstate_[cur_], dstate_[cur_ ^ 1], l0, l1, lg)) return false;
    // only this range's slices were written: copy them back instead of flipping the ping-pong
    // pair, so later calls on other ranges still read a complete current state
    const size_t per_layer = layer_state_len();
    HIP_OK(hipMemcpyAsync(dstate_[cur_] + l0 * per_layer, dstate_[cur_ ^ 1] + l0 * per_layer,
                          (size_t)(l1 - l0) * per_layer * 4, hipMemcpyDeviceToDevice, stream_));
    if (x_io) HIP_OK(hipMemcpyAsync(x_io, x_, bytes, hipMemcpyDeviceToDevice, stream_));
    if (vfirst_io && m_->major == 7) HIP_OK(hipMemcpyAsync(vfirst_io, vfirst_, bytes, hipMemcpyDeviceToDevice, stream_));
    if (lg && logits_out && !copy_logits(logits_out)) return false;
    logits_valid_ = lg;
    if (sync) {
        HIP_OK(hipStreamSynchronize(stream_));
        return handoff_check();
    }
    return true;  // async: the caller orders on stream() (pipeline.py) and synchronises (sync())
}

// Names: x xa sx r k v g w y a nb bb vfirst fr lora bonus logits, slot<i>.<q|d|s|qsum|h|f>.
// Returns -1 for an unknown name, a buffer that is not allocated, or more bytes than it holds.
long long Engine::debug_copy(const char * name, void * out, size_t bytes) {
    if (!name || !out) return -1;
    const std::string n(name);
    const void * src = nullptr;
    size_t cap_bytes = 0;
    auto pick = [&](const auto & b) { src = b.get(), cap_bytes = b.size() * sizeof(*b.get()); };
    const std::pair<const char *, const DevBuf<float> *> fb[] = {{"x", &x_}, {"xa", &xa_}, {"sx", &sx_}, {"r", &r_},
        {"k", &k_}, {"v", &v_}, {"g", &g_}, {"w", &w_}, {"y", &y_}, {"a", &a_}, {"nb", &nb_}, {"bb", &bb_},
        {"vfirst", &vfirst_}, {"fr", &fr_}, {"lora", &lora_}, {"bonus", &bonus_}, {"logits", &logits_}};
    for (const auto & p : fb)
        if (n == p.first) pick(*p.second);
    // the fused v7 decode (k_att7_lora) keeps w, a, g and the mixed v in LDS: those buffers hold
    // another evaluation's values, so they are refused rather than returned stale
    if (last_decode_ && v7_fused_lora_ && (n == "w" || n == "a" || n == "g" || n == "v")) return -1;
    if (n == "granules") pick(gran_.cleared);  // the fused v6 attention's
    if (!src && n.rfind("slot", 0) == 0) {
        const size_t dot = n.find('.');
        const int i = atoi(n.c_str() + 4);
        if (dot == std::string::npos || i < 0 || i >= kSlots) return -1;
        const std::string f = n.substr(dot + 1);
        const ActSlot & s = slots_[i];
        if (f == "q") pick(s.q);
        else if (f == "d") pick(s.d);
        else if (f == "s") pick(s.s);
        else if (f == "qsum") pick(s.qsum);
        else if (f == "h") pick(s.h);
        else if (f == "f") pick(s.f);
    }
    if (!src || bytes > cap_bytes) return -1;
    if (hipStreamSynchronize(stream_) != hipSuccess || hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return (long long)bytes;
}

bool Engine::eval_device(const uint32_t * tokens, size_t T, bool want_logits, float * logits_out, bool sync_after) {
    HIP_OK(hipSetDevice(m_->device));
    const int cur0 = cur_, pend0 = co_pending_;
    co_retry_ = false;
    for (int attempt = 0;; attempt++) {
        if (!run_tokens(tokens, T, want_logits || logits_out != nullptr)) return false;
        if (logits_out && !copy_logits(logits_out)) return false;
        if (!(sync_after || logits_out)) return true;
        HIP_OK(hipStreamSynchronize(stream_));
        if (handoff_check()) return true;
        // a co-resident layout timeout in this one-token call (an earlier asynchronous call's
        // timeout cannot be re-run: its state has moved on): run the token again from the state it
        // started from, in the ordered layout
        if (!co_retry_ || pend0 > 0 || attempt > 0 || T != 1 || cur_ != (cur0 ^ 1)) return false;
        co_retry_ = false;
        cur_ = cur0;
    }
}

}  // namespace rwkvmi
