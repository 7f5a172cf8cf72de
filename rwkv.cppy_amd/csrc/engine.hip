// engine.hip -- the engine core: lifetime, workspace, the timing tables, the state I/O, the
// evaluation entry points on host or device state and the debug hooks.  The two forward programs:
// engine_decode.hip (one token) and engine_sequence.hip (T rows: sequences, batched steps, packed
// chunks); batched decode and generation: engine_batch.hip; sampling, generation and scoring:
// engine_generate.hip; batched prefill: engine_prefill.hip; the weights: model_upload.hip.
//
// A token step is a fixed sequence of launches on the context's stream.  The T == 1 step
// is captured once into a hipGraph per (state parity, logits) and replayed, so decode pays
// no host launch cost.
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

ActBuf Engine::A(int slot, const DMat & W, bool tiled) const {
    const ActSlot & s = slots_[slot];
    ActBuf a;
    a.fmt = act_fmt_for(W.type);
    a.K = W.K;
    a.f = s.f;
    a.h = s.h;
    a.q = s.q;
    a.d = s.d;
    a.s = s.s;
    a.qsum = s.qsum;
    a.tq = s.tq;
    a.tiled = tiled && (a.fmt == A_Q8_0 || a.fmt == A_Q8_1);
    return a;
}

void Engine::set_timing(bool on) {
    (void)hipStreamSynchronize(stream_);
    collect_timing();
    timing_ = on;
    if (on) stats_.clear();
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

bool Engine::forward(int T, const float * sin, float * sout, bool logits, const TokArg & tok) {
    if (T == 1 && !generic_decode_) return forward_decode(sin, sout, logits, tok);
    return forward_range(seq_run(T, sin, sout, 0, m_->n_layer, tok, logits ? logits_.get() : nullptr));
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
bool Engine::run_tokens(const uint32_t * tokens, size_t T, bool want_logits, const ScoreRun * score) {
    // a failed call restores the ping-pong parity it started with, so the next state upload
    // (every rwkv_eval with state_in, rwkv_mi355x_state_upload) lands where the next step reads;
    // the device state's contents after a failure are unspecified (re-upload it)
    const int cur0 = cur_;
    logits_valid_ = false;
    if (!run_tokens_impl(tokens, T, want_logits, score)) {
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

bool Engine::run_tokens_impl(const uint32_t * tokens, size_t T, bool want_logits, const ScoreRun * score) {
    size_t done = 0;
    while (done < T) {
        const size_t n = std::min(T - done, kChunkMax);
        const bool last = done + n == T;
        if (!ensure_workspace((int)n)) return false;
        // one token: its id goes by value in the argument block of the step's first launch (TokArg;
        // a graph replay: set_tok), and nothing is enqueued to deliver it -- hipStreamWriteValue32,
        // which stood here, runs as a kernel of the runtime (__amd_rocclr_streamOpsWrite) on this
        // stream: 4.3 us and one more kernel boundary per token
        const bool imm = tokens && n == 1;
        const TokArg tok{dtokens_.get(), imm ? tokens[done] : 0u, imm ? 1u : 0u};
        // (tokens == NULL, generate: the sampler enqueued just before this step writes dtokens_[0])
        if (tokens && n > 1 && !stage_tokens(tokens + done, n)) return false;
        // scoring: a one-token chunk's step writes logits_ (score_chunk reads it), longer chunks get
        // their head from score_chunk
        const bool lg = score ? n == 1 : last && want_logits;
        last_decode_ = n == 1 && !generic_decode_;
        const bool co = last_decode_ ? choose_co() : (co_ = false);
        if (n == 1 && use_graphs_ && !timing_) {
            TokGraph & tg = graphs_[co][cur_][lg ? 1 : 0];
            if (!tg.ge && !capture_tok(tg, [&] { return forward(1, dstate_[cur_], dstate_[cur_ ^ 1], lg, tok); })) return false;
            if (!tg.set_tok(tok)) return false;
            HIP_OK(hipGraphLaunch(tg.ge, stream_));
        } else {
            // eager launches; timed, a decode step's kernels each carry a dispatch-bound event pair
            // (RK_LAUNCH through g_klt), the sequence path's matmul groups an event pair around
            // the group (mm_launch)
            const LaunchTimerScope timed(this, timing_ && n == 1);
            if (!forward((int)n, dstate_[cur_], dstate_[cur_ ^ 1], lg, tok)) return false;
        }
        if (score && !score_chunk(*score, done, n, last)) return false;
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
    const TokArg tok{dtokens_.get(), token, 1u};
    for (uint32_t c = 0; c < NC; c++)
        if (!gs[c].ge && !capture_tok(gs[c], [&] { return forward_decode(din, dout, lg, tok, c * K, (c + 1) * K); }))
            return false;
    if (!gs[0].set_tok(tok)) return false;
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
    if (!forward_range(seq_run((int)T, dstate_[cur_], dstate_[cur_ ^ 1], l0, l1, dtok(), lg ? logits_.get() : nullptr)))
        return false;
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
