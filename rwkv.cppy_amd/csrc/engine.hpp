// engine.hpp -- device-resident RWKV model and the per-version forward programs.
#pragma once

#include <stdio.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "devbuf.hpp"
#include "kernels.hpp"
#include "model_file.hpp"

namespace rwkvmi {

struct DLayer {
    float *ln1_w = nullptr, *ln1_b = nullptr, *ln2_w = nullptr, *ln2_b = nullptr;
    // v4 / v5
    float *att_mix_k = nullptr, *att_mix_v = nullptr, *att_mix_r = nullptr, *att_mix_g = nullptr;
    float *att_first = nullptr, *att_decay = nullptr;  // v4 (per channel)
    float *att_u = nullptr, *att_w = nullptr;          // v5/v6 wkv6 u (faaaa/first) and v5 w, expanded to [C]
    float *att_lnx_w = nullptr, *att_lnx_b = nullptr;
    // v6
    float *maa_x = nullptr, *maa[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, *maa_w2 = nullptr;
    float *maa_w2t = nullptr;  // time_maa_w2 transposed to [5][D][C] (coalesced per-channel dots)
    float *decay6 = nullptr;
    // v7
    float *x_rwkvag = nullptr, *w0 = nullptr, *a0 = nullptr, *v0 = nullptr, *k_k = nullptr, *k_a = nullptr, *r_k = nullptr;
    // ffn
    float *ffn_mix_k = nullptr, *ffn_mix_r = nullptr, *ffn_maa_k = nullptr, *ffn_maa_r = nullptr, *ffn_x_k = nullptr;
    DMat att_r{}, att_k{}, att_v{}, att_o{}, att_g{}, maa_w1{}, decay_w1{}, decay_w2{};
    DMat w1{}, w2{}, a1{}, a2{}, g1{}, g2{}, v1{}, v2{};
    DMat ffn_k{}, ffn_v{}, ffn_r{};
};

struct DeviceModel {
    int refcount = 0;
    int device = 0;
    uint32_t layer_lo = 0, layer_hi = 0;  // layers whose weights are resident: [layer_lo, layer_hi)
    bool partial() const { return layer_lo != 0 || layer_hi != n_layer; }
    uint32_t n_vocab = 0, n_embed = 0, n_layer = 0;
    int major = 4, minor = 0;
    int64_t H = 0, S = 0;
    int F = 0;          // FFN width
    int maa_D = 0;      // v6 maa LoRA width (per mix)
    int kmax = 0;       // largest matmul K
    size_t state_len = 0;
    DMat emb{}, head{};
    float *ln0_w = nullptr, *ln0_b = nullptr, *lnout_w = nullptr, *lnout_b = nullptr;
    std::vector<DLayer> layers;
    std::vector<void *> allocs;
    double layer_weight_bytes = 0;   // algorithmic bytes of all layer matrices (original block sizes)
    double head_weight_bytes = 0;
    double layer_flops = 0, head_flops = 0;  // 2*M*K per token
    double small_param_bytes = 0;    // fp32 vectors read per token
};

bool upload_model(const ModelFile & mf, DeviceModel & dm, uint32_t layer_begin = 0, uint32_t layer_end = UINT32_MAX);
// repacks one ggml-order matrix into the device layout (allocations recorded in dm.allocs)
bool upload_mat(DeviceModel & dm, const HostTensor * t, DMat & out, bool count_bytes, bool is_head);
void free_model(DeviceModel & dm);

struct ActSlot {
    DevBuf<int8_t> q;
    DevBuf<float> d, s;
    DevBuf<int> qsum;
    DevBuf<__half> h;
    DevBuf<float> f;
    DevBuf<uint8_t> tq;  // sequence-GEMM token-tile records
};

// The buffers sized by the token capacity.  Engine::ensure_workspace builds a fresh one and moves
// it into the engine (its private base, so the members keep their names) once it is complete.
struct Workspace {
    static constexpr int kSlots = 12;
    DevBuf<float> x_, xa_, sx_, r_, k_, v_, g_, w_, y_, a_, nb_, bb_, vfirst_, fr_;  // [cap][C]
    DevBuf<float> lora_, bonus_;  // [cap][kmax], [cap][H]
    DevBuf<float> dsmall_[4];     // decode LoRA intermediates [kmax]
    DevBuf<uint32_t> dtokens_;    // [cap]
    ActSlot slots_[kSlots];
    bool alloc(size_t cap, size_t C, size_t kmax, size_t H);
};

// The words a generation call drives on the device, as views of one allocation (GenSlots::gwords_).
// bind() is the layout: the arrays follow one another in the order of the members, K words each,
// `active` and `next` one word each.  Nothing else computes an address in gwords_.
struct GenWords {
    // every call (SampleArgs, GenRows): per sequence; active = the sequences not yet ended
    uint32_t *done = nullptr, *length = nullptr, *fin_step = nullptr, *active = nullptr;
    // the queue's (GenQueue): max_tokens per sequence; the table lane_seq per lane; lane, start per
    // sequence; retire_to, admit_from per lane; next = the first waiting sequence
    uint32_t *max_tokens = nullptr, *lane_seq = nullptr, *lane = nullptr, *start = nullptr, *retire_to = nullptr,
             *admit_from = nullptr, *next = nullptr;
    // points the members into base (NULL: nowhere) and returns the words the layout takes
    size_t bind(uint32_t * base, size_t K) {
        size_t at = 0;
        auto take = [&](uint32_t *& p, size_t n) {
            p = base ? base + at : nullptr;
            at += n;
        };
        take(done, K), take(length, K), take(fin_step, K), take(active, 1);
        take(max_tokens, K), take(lane_seq, K), take(lane, K), take(start, K), take(retire_to, K), take(admit_from, K);
        take(next, 1);
        return at;
    }
};

// The generation slots' buffers (Engine::batch_reserve), replaced as a whole in the same way: the
// live states [2][slots][state_len] (slots are stored in and loaded from gstate_[0]; the batched step
// alternates the two) and one fresh state behind them, all one allocation, so that a prefill's segment
// table names any of them by its float offset from gstates_ (state_off); the live logits [slots][n_vocab], the finished rows' snapshots of both, the
// penalty counts [slots][n_vocab], the per-row parameters and the words
struct GenSlots {
    DevBuf<float> gstates_, glogits_, gsnap_state_, gsnap_logits_;
    float * gstate_[2] = {nullptr, nullptr};  // views of gstates_
    float * gfresh_ = nullptr;                // the fresh state (Engine::batch_reserve fills it)
    DevBuf<uint32_t> gcounts_;
    DevBuf<float> gparams_;      // temperature, top_p, presence, frequency: [4][kBatchMax]
    DevBuf<uint64_t> gstreams_;  // seed, offset: [2][kBatchMax]
    DevBuf<uint32_t> gwords_;
    GenWords gw_;  // views of gwords_
    bool alloc(size_t n_slots, size_t state_len, size_t n_vocab, size_t batch_max);
};

// The granule memory of the in-launch hand-offs (handoff.hpp; DESIGN.md "The hand-off protocol").
struct GranuleMem {
    // cleared granules (tag 1, zeroed here and re-armed by their one reader): the fused v6
    // attention's r, k, v, g [4 C] and decay-LoRA values [H D]
    DevBuf<unsigned long long> cleared;
    // tagged granules (Engine::handoff_tag, never cleared by their readers), one allocation: y [C]
    // head / channel outputs -> fused Wo rows; k [KG_STRIDE F / 32] FFN key blocks and r [C]
    // receptance rows -> fused FFN value rows; x [C] v6 x rows -> the next layer's maa (k_sig_maa)
    DevBuf<unsigned long long> tagged;
    unsigned long long *y = nullptr, *k = nullptr, *r = nullptr, *x = nullptr;
    bool alloc(size_t C, size_t F);
    // A tag names a layer and a state parity, so a step that flips the parity without running the
    // fused decode (a sequence chunk, the generic decode, a decode program without the hand-off
    // after a debug knob changed) leaves the granules of the decode before it in place: the next
    // decode runs at that decode's parity again and could take a stale value for its own (one-layer
    // engines: the same layer tag).  So does a failed call that is replayed at the parity it started
    // with.  Every such step clears the tagged granules in stream order.
    hipError_t clear_tagged(hipStream_t st) const { return hipMemsetAsync(tagged, 0, tagged.size() * 8, st); }
    // after a timeout: a producer that arrived late left its granule set, cleared or tagged
    void clear_all(hipStream_t st) const {
        (void)hipMemsetAsync(cleared, 0, cleared.size() * 8, st);
        (void)clear_tagged(st);
    }
};

// Per-kernel-class timing collected with hipEvents on the context stream (bench roofline).
struct KernelStat {
    std::string name;
    long long launches = 0;
    double total_ms = 0;
    double total_bytes = 0;   // algorithmic bytes (weights at original block size + activations)
    double total_flops = 0;
};

// algorithmic bytes of T rows of an activation buffer (roofline formulas)
inline double act_bytes(const ActBuf & a, double T) {
    const double K = a.K;
    switch (a.fmt) {
        case A_F32: return T * K * 4;
        case A_F16: return T * K * 2;
        case A_Q8_1: return T * K + T * K / 32 * 12;
        default: return T * K + T * K / 32 * 8;
    }
}

struct DecodeRun;  // engine_decode.hip
struct MMBatch;    // engine_sequence.hip

// One forward of the sequence program (engine_sequence.hip) over T rows: all that its layer functions
// know of their caller -- a forward's mode is an argument, never an engine member written around the call.
// Made only by Engine::seq_run (a sequence), rows_run (B contexts) and packed_run (a packed prefill chunk).
struct SeqRun {
    int T;
    const float * sin;
    float * sout;
    uint32_t l0, l1;
    size_t bs;            // state floats between two contexts; 0: one sequence, or rows without state (a head tile)
    const SegTab * seg;   // the packed chunk's segment table, or NULL
    bool rows;            // the matmuls take the T rows as independent contexts (k_fmm / k_mvb / k_mm)
    bool tile_acts;       // the layers' Q8 activations go into sequence-GEMM token tiles
    TokArg tok;           // one token of its own sequence: the step's id; else read from dtokens_
    float * head_out;     // where the head writes its rows; NULL: no head
};

// The scope of the launch timer (common.hpp): while one made with `on` lives, every RK_LAUNCH of
// this thread takes its event pair from t.  Nothing else assigns g_klt.
struct LaunchTimerScope {
    LaunchTimerScope(KLaunchTimer * t, bool on) { if (on) g_klt = t; }
    ~LaunchTimerScope() { g_klt = nullptr; }
};

// rwkv_mi355x_sampling with the bias arrays still on the host (include/rwkv_mi355x.h)
struct SamplingParams {
    float temperature = 1.0f, top_p = 0.8f;
    uint32_t n_bias = 0;
    const uint32_t * bias_ids = nullptr;
    const float * bias_values = nullptr;
    uint64_t seed = 0, offset = 0;
};

// rwkv_mi355x_batch_sampling, checked by the caller (include/rwkv_mi355x.h): host arrays of B rows
struct BatchSamplingParams {
    const float *temperature = nullptr, *top_p = nullptr;
    const float *presence = nullptr, *frequency = nullptr;  // may be NULL: 0
    const uint64_t *seed = nullptr, *offset = nullptr;
    uint32_t n_bias = 0;
    const uint32_t * bias_ids = nullptr;
    const float * bias_values = nullptr;
    uint32_t n_stop = 0;
    const uint32_t * stop_tokens = nullptr;
    bool keep_counts = false;
    uint32_t check_every = 0;
};

// rwkv_mi355x_logprobs, checked by the caller (include/rwkv_mi355x.h): the host arrays that receive
// the log-probabilities of a call's draws, [rows][n] columns with the rows n apart, as tokens_out
struct LogprobsOut {
    uint32_t top_k = 0;
    double * token_logprob = nullptr;
    uint32_t * top_ids = nullptr;      // top_k per column
    double * top_logprobs = nullptr;   // top_k per column
};

class Engine : public KLaunchTimer, private Workspace, private GenSlots {
  public:
    explicit Engine(DeviceModel * m) : m_(m) {}
    ~Engine();
    bool begin(hipEvent_t * a, hipEvent_t * b) override;
    void end(const char * kernel) override;

    bool init();
    // ABI-level evaluation (host buffers).  tokens host, T >= 1.
    bool eval_once(const uint32_t * tokens, size_t T, const float * state_in, float * state_out, float * logits_out);
    bool eval(const uint32_t * tokens, size_t T, const float * state_in, float * state_out, float * logits_out);
    // device-resident evaluation on the context's own state
    bool eval_device(const uint32_t * tokens, size_t T, bool want_logits, float * logits_out, bool sync);
    bool eval_layers(const uint32_t * tokens, size_t T, uint32_t l0, uint32_t l1, float * x_io, float * vfirst_io,
                     bool want_logits, float * logits_out, bool sync = true);
    // Token sampling on the device logits (sample.hip).  sample: one draw with counter p.offset, the
    // state is untouched.  generate: n times { draw i with counter p.offset + i, one decode step on
    // the drawn token with logits on }, all enqueued without a host synchronisation; one copy of the
    // n tokens (and, logits_out != NULL, of the final logits) and one synchronisation at the end.  A
    // hand-off timeout anywhere in the chain fails the call (no re-run: the state has moved on).
    // Both need logits_valid().
    // lp != NULL (all four generation calls): k_logprobs runs in front of every sampler launch and the
    // sampler's LP form writes the drawn token's log-probability; the device arrays start as 0xFF bytes
    // and are copied out with the tokens.  lp == NULL: the call as it was.
    bool sample(const SamplingParams & p, uint32_t * token_out, const LogprobsOut * lp = nullptr);
    bool generate(const SamplingParams & p, size_t n, uint32_t * tokens_out, float * logits_out,
                  const LogprobsOut * lp = nullptr);
    // The device arrays of a call with log-probabilities: rows * n columns of 8 + 12 top_k bytes and one
    // logZ word per row, grown here and never inside a loop.  Enqueues nothing; the callers of the four
    // calls run it first, so that a failed allocation fails the call before anything else happens.
    bool lp_reserve(size_t rows, size_t n, uint32_t top_k);
    // Scoring (rwkv_mi355x_score_sequence): eval_device(tokens, T, want_logits = true, sync = true)
    // with the head on every token.  Each chunk's final residual rows go through the head in tiles
    // of kScoreRows rows (LayerNorm, the batched decode's head matmul, k_xent); losses and argmaxes
    // stay in device buffers until one copy at the end, logits_out (host [T][n_vocab], may be NULL)
    // receives each tile.  targets / losses_out: both NULL or both set; argmax_out may be NULL.
    bool score(const uint32_t * tokens, size_t T, const uint32_t * targets, double * losses_out, uint32_t * argmax_out,
               float * logits_out);
    static constexpr int kScoreRows = 128;  // a multiple of 64 (k_fmm's token tile); <= kBatchMax (k_mvb)
    // the device logits follow the device state: set by an evaluation that ran the head, cleared by
    // one that did not and by every state upload
    bool logits_valid() const { return logits_valid_; }
    // batched decode: B contexts, one token each; states [B][state_len] (host or device, see dev)
    bool eval_batch(const uint32_t * tokens, size_t B, const float * state_in, float * state_out, float * logits_out,
                    bool dev);
    static constexpr int kBatchMax = 256;
    // Batched generation (rwkv_mi355x_generate_batch).  A context owns n_slots <= kBatchMax slots,
    // each a state and its logits, apart from the context's own state and from eval_batch's staging.
    // reserve: (re)allocates the slots, all of them invalid afterwards; 0 frees.  store / load: the
    // context's device state and logits to / from a slot, device to device on the context's stream.
    // generate_batch over slots [0, B): n times { k_sample_rows on the slots' logits, k_gen_snapshot
    // of the rows that stopped, one batched decode step of the drawn tokens }, nothing crossing PCIe
    // but `active` every check_every steps; a finished row's slot ends with the state before its stop
    // token and the logits that produced it.  A failed call leaves slots [0, B) invalid.
    bool batch_reserve(size_t n_slots);
    size_t batch_slots() const { return gslots_; }
    bool batch_slot_valid(size_t slot) const { return slot < gslots_ && gvalid_[slot]; }
    bool batch_store(size_t slot);
    bool batch_load(size_t slot);
    bool generate_batch(size_t B, const BatchSamplingParams & p, size_t n, uint32_t * tokens_out, uint32_t * lengths_out,
                        uint32_t * steps_out, const LogprobsOut * lp = nullptr);
    // A queue of Q sequences (slots [0, Q)) over L = min(lanes, Q) decode rows
    // (rwkv_mi355x_generate_queue): per step k_gen_turnover frees the lanes of ended
    // sequences and admits the waiting ones, k_gen_move copies a capped sequence's result out of its
    // lane and an admitted slot in, then the sampler, the snapshot and one batched step over the L
    // lanes as in generate_batch.  Every per-row array of p is [Q]; max_tokens[s] in [1, n].
    bool generate_queue(size_t Q, size_t lanes, const BatchSamplingParams & p, const uint32_t * max_tokens, size_t n,
                        uint32_t * tokens_out, uint32_t * lengths_out, uint32_t * lane_out, uint32_t * start_out,
                        uint32_t * steps_out, const LogprobsOut * lp = nullptr);
    // Batched prefill (rwkv_mi355x_prefill_batch; engine_prefill.hip): n_rows prompts, concatenated in
    // tokens, are packed into chunks of at most prefill_chunk_ tokens (prefill_plan.hpp) and each chunk
    // runs as one sequence pass whose token shift and WKV kernels follow a segment table (SegTab);
    // the head runs once, over the residual rows that end the prompts.  Row i lands in slots[i] as
    // batch_store leaves a slot.  The caller has checked the arguments (distinct slots below
    // batch_slots(), lengths >= 1, tokens in range, cont rows valid).  A failure after the first launch
    // leaves the call's slots invalid.  Never captured into a graph.
    bool prefill_batch(size_t n_rows, const uint32_t * slots, const uint32_t * tokens, const size_t * lengths,
                       const uint8_t * cont);
    static constexpr size_t kChunkMax = 1024;  // tokens per sequence pass (run_tokens_impl, prefill_batch)
    float * device_logits() const { return logits_; }
    bool state_upload(const float * state);
    bool state_download(float * state);
    // the state of layers [l0, l1) only (a pipeline stage's or replica's slice); slice = those
    // layers in the host layout, NULL on upload = fresh state for them
    size_t layer_state_len() const { return m_->major >= 5 ? (size_t)m_->n_embed * (2 + (size_t)m_->S) : 5 * (size_t)m_->n_embed; }
    bool state_upload_layers(const float * slice, uint32_t l0, uint32_t l1);
    bool state_download_layers(float * slice, uint32_t l0, uint32_t l1);
    // state bytes moved host->device / device->host by this context (state APIs and rwkv_eval)
    double io_bytes_h2d() const { return io_h2d_; }
    double io_bytes_d2h() const { return io_d2h_; }
    bool sync();
    hipStream_t stream() const { return stream_; }
    void set_timing(bool on);
    const std::vector<KernelStat> & stats();
    float * device_state() const { return dstate_[cur_]; }
    // debugging aid (rwkv_mi355x_debug_buffer): copies a workspace buffer of the last evaluation
    long long debug_copy(const char * name, void * out, size_t bytes);
    // test hooks (rwkv_mi355x_debug_set): "skip_granule" = producer workgroup of k_v6_att_fused that
    // publishes nothing (-1 off), "spin_max" = the hand-off sweep bound, "prefill_chunk" = the packing
    // cap of prefill_batch in tokens (1 .. kChunkMax; <= 0 the default); returns false for unknown names
    bool debug_set(const char * name, long long value);
    // false when an in-launch hand-off of the work completed so far timed out: reports it, clears the
    // granules and the flag (the caller fails the evaluation with RWKV_ERROR_CTX)
    bool handoff_check();

  private:
    // Device memory.  Every device allocation of an engine is a DevBuf member (devbuf.hpp), freed
    // with the engine; the weights belong to the DeviceModel.  A buffer is replaced in one place,
    // grow(): nothing happens while b holds `need` elements; otherwise the stream is drained, the
    // graph caches named in `graphs` are dropped and b is reallocated with `cap` >= need elements
    // (empty after a failure).  The rule for `graphs`: every cache whose graphs may hold the old
    // address -- the decode graphs (graphs_, io_graphs_) capture the workspace, state, logits and
    // granules; the batched graphs (bgraphs_) the workspace, the GEMM scratch (gy_, part_, m2_),
    // eval_batch's staging and the generation slots; nothing captures a buffer that only eager
    // launches and copies touch (tokens drawn, scores, bias, wkvc_).  Never called while a capture
    // is open: whatever a captured step may grow has been grown by an eager step before it.
    enum : unsigned { GRAPHS_NONE = 0, GRAPHS_DECODE = 1, GRAPHS_IO = 2, GRAPHS_BATCH = 4, GRAPHS_ALL = 7 };
    bool settle(unsigned graphs);  // drains stream_ and drops those caches
    template <class T>
    bool grow(DevBuf<T> & b, size_t need, size_t cap, unsigned graphs);
    static size_t doubled(size_t floor, size_t n) {  // floor * 2^k >= n
        while (floor < n) floor *= 2;
        return floor;
    }
    bool ensure_workspace(int T);
    // the pinned staging copy of n tokens into dtokens_, in stream order
    bool stage_tokens(const uint32_t * tokens, size_t n);
    bool copy_logits(float * host_out);  // logits_ to the host on stream_
    // the sampler's logit bias, (allocated and) uploaded in stream order
    bool upload_bias(uint32_t n_bias, const uint32_t * ids, const float * values);
    bool init_state(float * st, size_t n = 0);
    // tok: the step's token id, handed on to the program that runs (DecodeRun / SeqRun)
    bool forward(int T, const float * sin, float * sout, bool logits, const TokArg & tok);
    // the sequence program (engine_sequence.hip) and the three makers of its argument
    bool forward_range(const SeqRun & s);
    SeqRun seq_run(int T, const float * sin, float * sout, uint32_t l0, uint32_t l1, const TokArg & tok,
                   float * head_out) const;
    // bs == 0: rows without state, for head_rows only (score_chunk, prefill_batch)
    SeqRun rows_run(int B, size_t bs, const float * sin, float * sout, float * head_out) const;
    SeqRun packed_run(int T, const SegTab * seg, float * states) const;  // every segment's state at its offset in states
    SeqRun make_run(SeqRun s) const;
    TokArg dtok() const { return TokArg{dtokens_.get(), 0u, 0u}; }  // row t's id is dtokens_[t]
    // the decode program (engine_decode.hip): per layer one decode_att_v* and decode_ffn
    bool forward_decode(const float * sin, float * sout, bool logits, const TokArg & tok, uint32_t l0 = 0,
                        uint32_t l1 = UINT32_MAX);
    bool decode_att_v4(DecodeRun & d, uint32_t l);
    bool decode_att_v5(DecodeRun & d, uint32_t l);
    bool decode_att_v6(DecodeRun & d, uint32_t l);
    bool decode_att_v7(DecodeRun & d, uint32_t l);
    bool decode_ffn(DecodeRun & d, uint32_t l);
    bool mv(MVGroup & g, hipStream_t st = nullptr);
    // argument blocks shared by the decode program (bs == 0) and the batched step (SeqRun::bs) of layer_v5/6/7
    Att6Dec att6_args(const DLayer & L, const float * si, float * so, size_t bs) const;
    Att7Dec att7_args(const DLayer & L, const float * si, float * so) const;
    LnMixArgs ln_mix_args(const SeqRun & s, const float * carry_in, float * carry_out, const float * lnw,
                          const float * lnb) const;
    template <class Att>
    bool batch_att_tail(const SeqRun & s, Att a, int wo_slot, int l, const float * si, float * so);
    // the tag of layer l's in-launch hand-offs at the current state parity, and what its launches poll with
    unsigned handoff_tag(uint32_t l) const { return (unsigned)(l + 1) | ((unsigned)(cur_ + 1) << 16); }
    Handoff handoff(uint32_t l) const { return Handoff{handoff_tag(l), herr_d_, spin_max_}; }
    // captures what build() enqueues on stream_ into an executable graph; keep: the graph itself
    // is handed over instead of destroyed
    template <class F>
    bool capture(hipGraphExec_t & ge, F && build, hipGraph_t * keep = nullptr);
    // A decode graph.  When its first launch takes the step's token id (TokArg: layers from 0), the
    // graph, that kernel node and a host copy of the node's argument block stay with it, and a
    // replay with another id updates that one node first (set_tok) -- no stream operation delivers
    // the id between two replays.
    struct TokGraph {
        hipGraphExec_t ge = nullptr;
        hipGraph_t g = nullptr;
        hipGraphNode_t node = nullptr;
        hipKernelNodeParams p = {};
        std::vector<char> args;  // the node's argument block (its kernel's one parameter)
        size_t off = 0;          // of the TokArg in it
        bool set_tok(const TokArg & t);
        void destroy();
    };
    template <class F>
    bool capture_tok(TokGraph & tg, F && build);
    // score(): what run_tokens_impl does after the layers of each chunk of a scoring call
    struct ScoreRun {
        const uint32_t * targets;
        float * logits_out;
    };
    // tokens == NULL (T == 1): the token is already in dtokens_[0] (generate: the sampler wrote it);
    // score: NULL when not scoring
    bool run_tokens(const uint32_t * tokens, size_t T, bool want_logits, const ScoreRun * score = nullptr);
    bool run_tokens_impl(const uint32_t * tokens, size_t T, bool want_logits, const ScoreRun * score);
    bool sampler_buffers(const SamplingParams & p, size_t n, SampleArgs & a);
    // final LayerNorm + head over the h.T residual rows at x into h.head_out [h.T][n_vocab]
    bool head_rows(const SeqRun & h, const float * x);
    bool score_buffers(size_t T);
    bool score_chunk(const ScoreRun & score, size_t done, size_t n, bool last);
    DevBuf<float> score_tile_;         // [kScoreRows][n_vocab] head tile (lazily allocated)
    DevBuf<uint32_t> score_targets_;   // one element per token of the longest call so far
    DevBuf<double> score_loss_;
    DevBuf<uint32_t> score_argmax_;
    bool layer_v4(const SeqRun & s, int l, const float * si, float * so);
    bool wkv6(const SeqRun & s, int H, int S, const float * u, const float * w, int wpt, const float * sin, float * sout);
    bool layer_v5(const SeqRun & s, int l, const float * si, float * so);
    bool layer_v6(const SeqRun & s, int l, const float * si, float * so);
    bool layer_v7(const SeqRun & s, int l, const float * si, float * so);
    bool ffn(const SeqRun & s, int l, const float * si, float * so);
    // workspace slot `slot` as the input of W; tiled: Q8 activations in sequence-GEMM token tiles
    ActBuf A(int slot, const DMat & W, bool tiled = false) const;
    ActBuf A(const SeqRun & s, int slot, const DMat & W) const { return A(slot, W, s.tile_acts); }

    DeviceModel * m_;
    hipStream_t stream_ = nullptr;
    double io_h2d_ = 0, io_d2h_ = 0;
    DevBuf<float> logits_;
    uint32_t * htokens_ = nullptr;  // pinned, as many tokens as the Workspace's dtokens_
    bool logits_valid_ = false;
    DevBuf<uint32_t> gen_tokens_;   // generate: the drawn tokens
    DevBuf<uint32_t> bias_ids_;     // the sampler's logit bias [SAMPLE_MAX_BIAS]
    DevBuf<float> bias_vals_;
    // log-probabilities of a call's draws (lp_reserve): one double per column, top_k ids and doubles
    // per column, logZ per row of a sampler launch [kBatchMax]
    DevBuf<double> lp_token_, lp_top_, lp_logz_;
    DevBuf<uint32_t> lp_ids_;
    // the fill of a call's columns (every byte 0xFF) and the arrays into the sampler's arguments;
    // the copies out at the end of the call
    bool lp_begin(const LogprobsOut * lp, size_t rows, size_t n, SampleArgs & a);
    bool lp_copy_out(const LogprobsOut * lp, size_t rows, size_t n);
    DevBuf<float> dstate_[2];
    int cur_ = 0;
    unsigned * herr_h_ = nullptr;  // hand-off timeout flag, host-mapped (herr_d_ = its device address)
    unsigned * herr_d_ = nullptr;
    GranuleMem gran_;
    int dbg_skip_gran_ = -1;
    unsigned spin_max_ = 1u << 20;
    // chunk-parallel wkv6 for sequences (wkv_chunk.hip; re-associated, not bit-exact): 0 = serial
    // k_wkv6_s64 (default); RWKV_MI355X_WKV_CHUNK=1 or rwkv_mi355x_debug_set(ctx, "wkv_chunk", 1)
    bool wkv_chunk_ = false;
    DevBuf<float> wkvc_;  // its chunk matrices / chunk states, grown on demand
    TokGraph graphs_[2][2][2];  // [co-resident layout][cur][logits]
    bool use_graphs_ = true;
    bool split_maa_ = false;       // RWKV_MI355X_SPLIT_MAA=1: v6 decode W1 + mix as two launches
    // Decode fusions (RWKV_MI355X_DECODE_FUSION, a mask read at init; rwkv_mi355x_debug_set
    // "decode_fusion"): every fused launch has an unfused form of the same bits.
    enum : unsigned {
        FUSE_ATT6 = 1,   // k_v6_att_fused (r, k, v, g, decay-LoRA rows + per-head attention)
        FUSE_WO6 = 2,    // + Wo in that launch
        FUSE_ATT4 = 4,   // k_v4_att_fused (LN + r, k, v rows + WKV-4)
        FUSE_WO4 = 8,    // + Wo in that launch
        FUSE_ATT7 = 16,  // k_att7_lora (v7 LoRA second stages + attention)
        FUSE_SIG = 32,   // k_mvsig (FFN value + receptance rows)
        FUSE_FFN = 64,   // k_ffn_fused (the whole channel mix: key, receptance and value rows)
        FUSE_FFNCO = 128,  // its co-resident form, while the co-resident layouts are in use (co_mode)
        FUSE_SIGMAA = 256, // v6: the FFN value rows + the next layer's maa in one launch (co-resident only)
        FUSE_EMBMAA = 512, // the embedding LayerNorm inside layer 0's first launch (v6 maa, v4 attention)
        FUSE_ALL = 1023,
        // the one-launch channel mix measured slower than the key + value pair (same box, separate
        // processes: v6-1B6 716 vs 692 us/token, v4-169M 234 vs 228): off by default
        // (FUSE_FFNCO is added at creation for RWKV-4 only: v4-169M 222.5-223.0 vs 230.5-230.9 us/token,
        // v6-1B6 697.8-699.7 vs 655.9-659.2 -- profiles/r6_ab_ffco_v4.txt, r6_ab_ffco_v6.txt)
        FUSE_DEFAULT = FUSE_ALL & ~FUSE_FFN & ~FUSE_FFNCO,
    };
    unsigned fuse_ = FUSE_DEFAULT;
    // v6 attention launch layout (mv_att6c.hip vs mv_att6f.hip, the same bits).  The co-resident
    // layout needs all its workgroups resident at once: it is used only while this context is the
    // process's only one with work queued on the device (claim_device / the per-device count) and
    // until a hand-off timeout (another process's launches holding the compute units) turns it off
    // for the context.  co_knob_ ("co_mode"): -1 that rule, 0 never, 1 always (tests, A/B).
    int co_knob_ = -1;
    bool co_ok_ = true;       // cleared for good by a hand-off timeout in the co-resident layout
    bool co_ = false;         // the layout the launches being enqueued / captured use
    bool claimed_ = false;    // this context holds one count on its device (released at a sync)
    bool co_retry_ = false;   // the last failed check saw co-resident layout launches
    int co_pending_ = 0;      // co-resident layout decodes enqueued since the last check
    void claim_device();
    void release_device();
    bool choose_co();         // claim the device, pick the layout for the next decode launches
    int wo_rows_ = 8;      // k_v6_att_fused: Wo rows per wave of a Wo workgroup (debug knob "wo_rows": 4 / 8)
    int ffn_wdelay_ = -1;  // k_ffn_fused: consumer weight-issue delay in 100 MHz ticks ("ffn_wdelay"; -1:
                           // the producers' weight bytes at 4 TB/s, so the two streams do not overlap)
    int ffn_prepoll_ = 1;  // k_ffn_fused: poll the key blocks' d granules before the gather ("ffn_prepoll")
    int wo_prepoll_ = 1;   // k_v6_att_fused: one wave polls a granule per head before the gather ("wo_prepoll"; 0: 707.5 -> 708.9 us/token)
    bool generic_decode_ = false;  // RWKV_MI355X_GENERIC_DECODE=1: decode through the T>1 kernels
    hipEvent_t tok_event_ = nullptr;
    bool v7_fused_lora_ = false;  // the decode program runs k_att7_lora (w/a/g/v buffers not written)
    bool last_decode_ = false;    // the last step ran the decode program (debug_copy)
    bool timing_ = false;
    struct Pending {
        int stat;
        hipEvent_t a, b;
        double bytes, flops;
    };

    int add_stat(const std::string & name);
    double kt_bytes_ = 0, kt_flops_ = 0;  // algorithmic work of the next timed launch
    hipEvent_t kt_a_ = nullptr, kt_b_ = nullptr;
    // a matmul group of the sequence program: where it goes (mm_route, the one place that decides),
    // the launches (mm_dispatch) and, timed, its stat named after the route (mm_launch)
    friend struct MMBatch;
    enum MMRoute { MM_QGEMM, MM_ROWS, MM_KMM };  // the sequence GEMM; rows as contexts; k_mm
    MMRoute mm_route(int T, int wtype, bool rows, bool tile_acts) const;
    bool mm_dispatch(MMGroup & g, int wtype, MMRoute route);
    bool mm_launch(MMGroup & g, int wtype, MMRoute route);
    // the GEMM scratch, grown to the exact size a group needs (captured batched graphs point at it)
    DevBuf<float> gy_;    // scratch y of emit-only GEMM entries
    DevBuf<float> part_;  // split-K partials (launch_qgemm, k_fmm)
    DevBuf<float> m2_;    // _1 formats: m*s chain totals (launch_qgemm, k_qg_msum)
    bool use_mm_ = false;
    size_t prefill_chunk_ = kChunkMax;  // debug knob "prefill_chunk": the packing cap in tokens
    DevBuf<uint32_t> ptokens_;          // a prefill's tokens
    DevBuf<uint64_t> ptab_;             // its segment tables and row lists
    DevBuf<float> pend_x_;              // [kBatchMax][C] the residual rows that end its prompts
    int batch_gemm_min_ = 16;  // batched decode: contexts from which the quantized matmuls take the sequence GEMM
    // batched decode (eval_batch): the engine-owned staging buffers / graphs
    DevBuf<float> bstate_[2], blogits_;  // staging of host states / logits: a power of two >= B rows
    struct BatchGraph {
        size_t B;
        const float * sin;
        float * sout;
        float * lout;
        hipGraphExec_t ge;
    };
    std::vector<BatchGraph> bgraphs_;
    void drop_batch_graphs();
    // generation slots (batch_reserve; their buffers: GenSlots)
    size_t gslots_ = 0;
    std::vector<char> gvalid_;
    DevBuf<uint32_t> gtokens_;  // the drawn tokens [B][n] of a call
    std::vector<float> gparams_h_;   // the host copies the uploads read
    std::vector<uint64_t> gstreams_h_;
    std::vector<uint32_t> gqueue_h_;  // max_tokens up, start down (generate_queue)
    void free_slots();
    // generate_batch and generate_queue are one driver (engine_batch.hip): sequences [0, Q) over the
    // rows of a batched step; with a QueueCall the rows are lanes the sequences pass through
    struct QueueCall {
        size_t lanes;
        const uint32_t * max_tokens;
        uint32_t *lane_out, *start_out;
    };
    bool generate_slots(size_t Q, const BatchSamplingParams & p, size_t n, uint32_t * tokens_out, uint32_t * lengths_out,
                        uint32_t * steps_out, const LogprobsOut * lp, const QueueCall * qc);
    // the per-sequence arrays of Q sequences to the device and the token buffer [Q][n] set to
    // 0xFFFFFFFF; the sampler's arguments for `rows` rows
    bool gen_upload(size_t Q, const BatchSamplingParams & p, size_t n);
    SampleArgs gen_sample_args(size_t rows, const BatchSamplingParams & p, size_t n);
    // the one way out of a call on slots[0 .. n) (NULL: slots 0 .. n - 1) that fails after its first
    // enqueue: the stream drained, the hand-off checked, the slots invalid.  Returns false.
    bool slots_fail(size_t n, const uint32_t * slots = nullptr);
    // rwkv_eval with host state buffers: the decode as io_chunk_-layer graphs with the state
    // copies of other chunks overlapped (eval_host_chunked)
    bool io_pipeline_ = true;
    int io_chunk_ = 4;
    hipStream_t io_stream_[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> io_ev_;
    hipEvent_t io_entry_ev_ = nullptr;  // work already queued on stream_ at entry (copy streams wait)
    // [co-resident layout][cur][logits] per chunk; chunk 0's takes the token id
    std::vector<TokGraph> io_graphs_[2][2][2];
    bool eval_host_chunked(uint32_t token, const float * state_in, float * state_out, float * logits_out);
    bool pinned_io(const float * state_in, const float * state_out);
    void drop_io_graphs();
    void drop_graphs();
    std::vector<Pending> pending_;
    std::vector<hipEvent_t> event_pool_;
    std::vector<KernelStat> stats_;
    void collect_timing();
};

template <class T>
bool Engine::grow(DevBuf<T> & b, size_t need, size_t cap, unsigned graphs) {
    if (need <= b.size()) return true;
    if (!settle(graphs)) return false;
    if (b.alloc(cap)) return true;
    fprintf(stderr, "rwkv: device allocation of %zu bytes failed\n", cap * sizeof(T));
    return false;
}

// Captures what build() enqueues on stream_ and instantiates it as ge.  A failed build still ends
// the capture (the stream has to leave capture mode) before its graph is dropped.
template <class F>
bool Engine::capture(hipGraphExec_t & ge, F && build, hipGraph_t * keep) {
    hipGraph_t g = nullptr;
    HIP_OK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
    const bool ok = build();
    HIP_OK(hipStreamEndCapture(stream_, &g));
    if (!ok) {
        (void)hipGraphDestroy(g);
        return false;
    }
    const hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    if (e != hipSuccess || !keep) (void)hipGraphDestroy(g);
    HIP_OK(e);
    if (keep) *keep = g;
    return true;
}

// As capture(); when a launch of build() took the step's TokArg (it left its argument block in
// g_tokl), that launch is the chain's first kernel node: the node, its launch parameters and the
// argument block are kept for set_tok.  The node's own copy of the block must equal the launch's --
// anything else means the first node is not that launch, and the capture fails.
template <class F>
bool Engine::capture_tok(TokGraph & tg, F && build) {
    tg.destroy();
    TokLaunch rec;
    g_tokl = &rec;
    const bool ok = capture(tg.ge, build, &tg.g);
    g_tokl = nullptr;
    if (!ok) return false;
    if (!rec.size) {  // layers from l0 > 0: no id in this graph
        (void)hipGraphDestroy(tg.g);
        tg.g = nullptr;
        return true;
    }
    size_t n = 1;
    hipKernelNodeParams p;
    hipGraphNodeType type;
    if (hipGraphGetRootNodes(tg.g, &tg.node, &n) != hipSuccess || n != 1 ||
        hipGraphNodeGetType(tg.node, &type) != hipSuccess || type != hipGraphNodeTypeKernel ||
        hipGraphKernelNodeGetParams(tg.node, &p) != hipSuccess || !p.kernelParams || !p.kernelParams[0] ||
        memcmp(p.kernelParams[0], rec.args, rec.size) != 0) {
        (void)hipGetLastError();
        fprintf(stderr, "rwkv: the decode graph's first node is not the launch that takes the token id\n");
        tg.destroy();
        return false;
    }
    tg.p = p;
    tg.p.kernelParams = nullptr;  // set_tok points it at args
    tg.p.extra = nullptr;
    tg.args.assign(rec.args, rec.args + rec.size);
    tg.off = rec.off;
    return true;
}

}  // namespace rwkvmi
