// taco_lib.hip -- host side of libtaco_hip.so: weight pack, stage orchestration, hipGraph plans and
// the C ABI of include/taco_abi.h.  Replaces the TF1 graph built by Tacotron.initialize()
// (models/tacotron.py:21-271 of the reference) and its sess.run execution (synthesizer.py:166-167).
// No CPU compute path exists here: every stage is a gfx950 kernel from taco_kernels.h.
#include "taco_kernels.h"
#include "taco_decoder_xcd.h"
#include "taco_bigru_xcd.h"
#include "taco_chain.h"
#include "taco_front.h"
#include "taco_head.h"
#include "taco_train_kernels.h"
#include "taco_backward_kernels.h"
#include "taco_wgrad_planes.h"
#include "taco_decoder_bwd_xcd.h"
#include "../../include/taco_abi.h"
#include "../../include/taco_debug.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <functional>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// "An output must not overlap an input or another output": an entry point lists its buffers as spans, the outputs first.  Byte counts are
// 128-bit so that element counts near 2^63 are not mistaken for small ones.
typedef unsigned __int128 u128;
struct Span { const void* p; u128 bytes; const char* name; };

// [p, p + bytes) and [q, q + qbytes) share a byte
static bool ta_overlap(const void* p, u128 bytes, const void* q, u128 qbytes) {
  const u128 a = (uintptr_t)p, b = (uintptr_t)q;
  return bytes && qbytes && a < b + qbytes && b < a + bytes;
}

// each of the first n_out spans against every span behind it; null pointers and spans of no bytes overlap nothing
static int no_overlap(std::initializer_list<Span> spans, int n_out) {
  for (const Span* o = spans.begin(); o < spans.begin() + n_out; ++o)
    for (const Span* q = o + 1; q < spans.end(); ++q)
      if (o->p && q->p && ta_overlap(o->p, o->bytes, q->p, q->bytes)) return fail(TACO_ERR_ARG, "%s and %s overlap", o->name, q->name);
  return 0;
}
// ------------------------------------------------------------------------------------------------
// one whole-chip kernel at a time per device and process
// ------------------------------------------------------------------------------------------------
// The persistent kernels (k_decoder_xcd, k_bigru_oct / duo and their backward twins) need all 256 workgroups resident at once.  Two of them
// dispatched to one device together -- two models or plans of ONE process on different streams or threads -- can each end up waiting for compute
// units the other one holds until their bounded spins expire.  A ChipTurn in the scope of every such launch (and of every replay of a plan that
// contains one) puts them in a total order: under a per-device mutex, a launch on ANOTHER stream than the previous whole-chip launch first records
// an event on that previous stream (behind everything enqueued there so far) and makes its own stream wait for it.  Launches that follow each other
// on one stream -- the serving loop, bench.py -- cost a mutex and a pointer compare, no event (an event record behind every replay was measured:
// +0.01 ms per C2 forward).  Everything else of a forward still overlaps across streams.  Inside a stream capture nothing is waited for or
// recorded; the capture is only marked (g_captured_whole_chip), and taco_plan_launch takes the turn for the whole graph.  Other PROCESSES on the
// device are outside its reach: one process per GPU stays the deployment rule.
#include <mutex>
struct ChipTurnState { std::mutex mu; hipEvent_t ev = nullptr; hipStream_t last = nullptr; bool armed = false; };
static ChipTurnState g_turn[32];
static int g_chip_turns = 1;                                   // taco_debug_set_chip_turns: 0 switches the ordering off (A/B)
static thread_local bool g_captured_whole_chip = false;        // a whole-chip launch was captured on this thread since the flag was last cleared
struct ChipTurn {
  ChipTurnState* t = nullptr; hipStream_t st;
  ChipTurn(int device, hipStream_t stream) : st(stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) { g_captured_whole_chip = true; return; }
    (void)hipGetLastError();
    if (!g_chip_turns || device < 0 || device >= 32) return;
    t = &g_turn[device];
    t->mu.lock();
    if (t->armed && t->last != st) {
      bool ordered = false;
      if (t->ev || hipEventCreateWithFlags(&t->ev, hipEventDisableTiming) == hipSuccess)
        ordered = hipEventRecord(t->ev, t->last) == hipSuccess && hipStreamWaitEvent(st, t->ev, 0) == hipSuccess;
      if (!ordered) { (void)hipGetLastError(); (void)hipDeviceSynchronize(); }      // the previous stream is gone (destroyed by its owner): its work may still run
    }
  }
  ~ChipTurn() {
    if (!t) return;
    t->armed = true; t->last = st;
    t->mu.unlock();
  }
  ChipTurn(const ChipTurn&) = delete; ChipTurn& operator=(const ChipTurn&) = delete;
};

// Stream-ordered zero fill as a kernel launch.  hipMemsetAsync nodes of a captured graph were seen to fill with a stale 16-byte
// pattern after another plan of the process had been destroyed (round 2: the census words and the exchange tags of a decoder plan,
// the BatchNorm sums of a captured train step); a kernel node has no such state.
// Up to ZERO_MAX regions in ONE launch, blockIdx.y picks the region (a forward clears every word its persistent kernels poll up front, the
// backward pass a dozen small accumulators in a row: the fill launches and their graph edges less); every region 4-byte aligned and sized
#define ZERO_MAX 12
struct ZeroList { uint32_t* p[ZERO_MAX]; unsigned long long nw[ZERO_MAX]; };
__global__ __launch_bounds__(256) void k_zero_fill(const ZeroList z) {
  uint32_t* p = z.p[blockIdx.y];
  const size_t nw = z.nw[blockIdx.y];
  const size_t n16 = (reinterpret_cast<uintptr_t>(p) & 15) ? 0 : nw / 4;
  const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  uint4* q = reinterpret_cast<uint4*>(p);
  for (size_t i = i0; i < n16; i += stride) q[i] = make_uint4(0u, 0u, 0u, 0u);
  for (size_t i = n16 * 4 + i0; i < nw; i += stride) p[i] = 0u;
}
static hipError_t zero_async(void* p, size_t bytes, hipStream_t st) {      // the one-region case
  if (!bytes) return hipSuccess;
  if ((reinterpret_cast<uintptr_t>(p) & 3) || (bytes & 3)) return hipMemsetAsync(p, 0, bytes, st);
  const size_t nw = bytes / 4;
  ZeroList z; memset(&z, 0, sizeof z);
  z.p[0] = static_cast<uint32_t*>(p); z.nw[0] = nw;
  const size_t n16 = (reinterpret_cast<uintptr_t>(p) & 15) ? 0 : nw / 4;
  const size_t items = n16 ? n16 + (nw - n16 * 4) : nw;
  const unsigned blocks = (unsigned)std::min<size_t>((items + 255) / 256, 2048);
  hipLaunchKernelGGL(k_zero_fill, dim3(blocks), dim3(256), 0, st, z);
  return hipGetLastError();
}
// The regions a caller up the stack clears with ONE launch (forward_pass: every word the persistent kernels of a forward poll; the first CH_RIDERS
// entries of z).  It lives on that caller's stack; `enqueued` is set by whoever has JUST put that launch into the stream -- never before.
struct UpFrontClear {
  ZeroList z; bool enqueued = false;
  bool covers(const void* q, size_t bytes) const {
    for (int i = 0; enqueued && i < CH_RIDERS; ++i)
      if (z.p[i] == q && z.nw[i] * 4 >= bytes) return true;
    return false;
  }
};
// Words a persistent kernel polls: zero when it is launched.  The stage that launches it clears them through clear(): skipped only when exactly this
// region -- same start, at least as many bytes -- is in the caller's launch, so a stage whose region changes (or a new stage) clears itself instead of
// trusting a list kept elsewhere.  cleared is null wherever a stage runs on its own: a stage entry, the training step, a debug hook.
struct Polled {
  void* p = nullptr; size_t bytes = 0; const UpFrontClear* cleared = nullptr;
  hipError_t clear(hipStream_t st) const { return cleared && cleared->covers(p, bytes) ? hipSuccess : zero_async(p, bytes, st); }
};

// collects zero fills that follow one another on a stream and issues them as one launch (run() -- also from the destructor's caller)
struct ZeroBatch {
  ZeroList z; int n = 0; size_t big = 0; hipStream_t st;
  explicit ZeroBatch(hipStream_t s) : st(s) { memset(&z, 0, sizeof z); }
  hipError_t add(void* p, size_t bytes) {
    if (!bytes) return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(p) & 3) || (bytes & 3)) return zero_async(p, bytes, st);
    if (n == ZERO_MAX) { hipError_t e = run(); if (e != hipSuccess) return e; }
    z.p[n] = static_cast<uint32_t*>(p); z.nw[n] = bytes / 4; big = std::max(big, bytes / 16); ++n;
    return hipSuccess;
  }
  hipError_t run() {
    if (!n) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<size_t>(std::max<size_t>((big + 255) / 256, 1), 1024);
    hipLaunchKernelGGL(k_zero_fill, dim3(blocks, n), dim3(256), 0, st, z);
    n = 0; big = 0; memset(&z, 0, sizeof z);
    return hipGetLastError();
  }
};

#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(TACO_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define TRY(expr)            \
  do {                       \
    int rc_ = (expr);        \
    if (rc_ != 0) return rc_; \
  } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int rup(int a, int b) { return cdiv(a, b) * b; }
static inline size_t rup_sz(size_t a, size_t b) { return (a + b - 1) / b * b; }

// ------------------------------------------------------------------------------------------------
// model
// ------------------------------------------------------------------------------------------------
struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool set = false;
};

struct ConvL {  // a k_gemm layer (conv1d+BN, dense, highway, hoisted GRU input projection)
  int kw = 1, cin = 0, cin_pad = 0, N = 0;
  size_t wp = 0, wp2 = 0, bias = 0, bias2 = 0, bns = 0, bnb = 0;  // arena offsets (+1; 0 = absent)
  size_t bh = 0, bl = 0, bh2 = 0, bl2 = 0;                          // split-bf16 packs (k_gemm_bf3), 0 = not built
  size_t bl3 = 0, bl3_2 = 0;                                       // third planes (training shadow model: the six-product instantiation)
  bool x6 = false;                                                 // inference: run this layer on the six-product (fp32-grade) instantiation (its third plane is built)
  int K16 = 0, cin_pad16 = 0;
  size_t wtail = 0; int ntail = 0;                                 // the last N % 32 (<= 4) columns as fp32 rows [ntail][cin]: the vector-ALU tail of k_head_sweep (taco_head.h)
  int var_index = -1;                                              // index into the device GemmVar array
};
struct SkW {  // a k_skinny weight
  int K = 0, Kq = 0, N = 0;
  size_t wp = 0, bias = 0;
};
struct GruDec { SkW gx, ch; int I = 0, H = 0; };   // gx: [I+H, 3H] = [gates (r|u) | x-rows of candidate]; ch: h-rows of candidate
struct Cbhg {
  int in_dim = 0, K = 0, C = 0, maxpool = 1, depth = 0, rnn = 0, pw = 3;
  int nproj = 0, proj_dim[4] = {0, 0, 0, 0};   // known from hparams alone (workspace sizing before finalize)
  std::vector<ConvL> bank;  // ordered widest first (longest workgroups are dispatched first)
  int bank_var0 = -1;
  std::vector<ConvL> proj;
  bool has_dense = false;
  ConvL dense;
  std::vector<ConvL> hw;
  ConvL xproj;              // N = 2 directions x (2H gates | H candidate), biases folded in
  SkW gh[2], ch[2];
  size_t raw_gh[2] = {0, 0}, raw_ch[2] = {0, 0};   // h-rows of the GRU kernels in TF layout (row-parallel scan)
  size_t res_g2[2] = {0, 0};                       // h-rows of gates/kernel as (r, u) pairs per unit: [H][H][2] (k_bigru_res)
  size_t gd_pack = 0;                                  // k_bigru_duo: the UPW = 1 layout of bigru_fwd_pack (taco_pack.h) -- the same bytes as go_pack[0], both kept
  size_t go_pack[3] = {0, 0, 0};                       // k_bigru_oct<UPW>, UPW = 1, 2, 4
  size_t gb_pack = 0, gob_pack = 0;                    // training: k_bigru_duo_bwd (one unit per wave) / k_bigru_oct_bwd (four)
  // fused front (taco_front.h): per bank width (same order as `bank`) the produce pack [k32 step][16-channel tile][lane][8] (hi, lo)
  // and its step count; front_kind 0 = not built, 1 = <TN 2, XS 80, CINP 80, KWMAX 8> (post-net), 2 = <TN 1, XS 144, CINP 128, KWMAX 16> (encoder)
  std::vector<size_t> fr_wh, fr_wl; std::vector<int> fr_ns; int front_kind = 0;
  size_t res_g2p[2] = {0, 0}, res_c1p[2] = {0, 0}; // the same and the candidate h-rows with the columns in k_bigru_resw's thread order
                                                   // (column jb*4 + u = unit jb + 64*u): a thread's four units are 32 / 16 contiguous bytes
};

struct taco_model {
  taco_hparams hp;
  int device = 0;
  bool finalized = false;
  std::vector<std::pair<std::string, std::vector<int64_t>>> spec;  // required tensors
  std::map<std::string, HostTensor> raw;
  // packed
  std::vector<float> harena;
  float* darena = nullptr;
  size_t arena_n = 0;
  std::vector<GemmVar> hvars;
  std::map<std::string, ConvL> convs;
  std::map<std::string, SkW> skinny;
  std::map<std::string, GruDec> grus;
  std::vector<ConvL> enc_prenet;
  Cbhg enc, post;
  ConvL memory_layer, linear;
  std::vector<SkW> dec_prenet;
  GruDec att_gru;
  std::vector<GruDec> dec_gru;
  SkW query, concat_proj, frame_proj, lin_spk;   // lin_spk: speaker rows of the linear head ('simple')
  SkW prenet1_next;   // decoder prenet layer 1 of step t+1 as a function of step t's [GRU-stack output | context] (frame projection folded in)
  int fuse_prenet1 = 1;
  GruDec gru1_fold;   // decoder GRU 1 with the concat projection folded into its x rows: input [h_att | ctx (| spk)], extra columns = o0
  int fuse_concat = 0;
  int att_split = -1;   // -1: heuristic; 0/1: one workgroup per row; >1: k_att_scores + k_att_context with that many slices per row
  size_t att_v = 0, att_b = 0, att_sb = 0, emb = 0, spk_emb = 0, raw_wq = 0;
  std::vector<SkW> spk_dense;      // deepvoice: before_highway, enc_init, att_init, dec_init_i
  std::vector<size_t> spk_table;   // speaker_embedding_size == 1 variant
  int force_cfg = -1;          // debug: force the exact-fp32 k_gemm and its config (a GemmCfg; CFG_AUTO: the model's level, gemm_plan's heuristic)
  unsigned* d_err = nullptr;   // set by a persistent kernel whose bounded spin expired
  int persist = 1;             // which BiGRU scan runs: a ScanMode (scan_plan; taco_debug_set_persistent)
  int ff_rot = 1;              // k_pointwise_chain: workgroups of an XCD start their K loops at different steps (0: taco_model_set_batch_invariant)
  int bf3 = 1;                 // feed-forward GEMMs (both CBHGs, linear head) on the bf16 matrix cores with 3-term split operands
  int bf3x6 = 0;               // training shadow model: feed-forward GEMMs on the six-product (fp32-grade) split-bf16 instantiation
  int bf3_tn = 0;              // debug: force the k_gemm_bf3 tile (a GemmTile; TILE_AUTO: gemm_plan's heuristic)
  int chain = 1;               // point-wise tail of a CBHG as one launch (taco_chain.h); 0: one launch per layer
  int front_entry = 1;         // proj_1's epilogue + proj_2 inside the point-wise chain's entry (taco_chain.h) when the fused front ran
  int front_prio = 1; int front_delay = 0;      // shader clocks by which the second K half of a k_cbhg_front workgroup starts late (taco_front.h)
  int head_sweep = 1;          // wide dense layers over many rows (the linear head) as a row sweep (taco_head.h); 0: k_gemm_bf3 tiles
  int front = 1;               // conv bank -> max-pool -> proj_1 of a CBHG as one launch (taco_front.h); 0: bank and proj_1 as two k_gemm_bf3 launches
  // persistent XCD-local decoder (taco_decoder_xcd.h): per-thread weight pack and the bias vectors its epilogues read
  size_t dx_fold_n = 0;        // training shadow model: elements of the GRU-1 fold buffer (k_dx_fold), addressed by the index map as NP + 1 + i
  size_t dx_spkw = 0;          // 'simple': speaker rows of the attention GRU and of the folded GRU 1, [S][DXRB_N][256] (k_dx_rowbias)
  // training shadow model: split-bf16 packs as index maps (pack_bf3): element e of the concatenated list copies parameter bf3_idx[e] - 1
  std::vector<unsigned> bf3_idx; std::vector<Bf3Seg> bf3_segs;
  int last_bptt = 0;           // the last decoder backward ran as the persistent launch (taco_debug_decoder_info out16[9])
  size_t dbx_pack = 0;         // training shadow model: the persistent BPTT kernel's rows (dbx_build_pack)
  size_t dx_pack = 0, dx_p1o_raw = 0, dx_qpack[4] = {0, 0, 0, 0}, dx_b_p1_0 = 0, dx_b_p1c = 0, dx_b_p2 = 0, dx_b_p3 = 0, dx_b_ag = 0, dx_b_ac = 0, dx_b_g1f = 0,
         dx_b_g1c = 0, dx_b_g2g = 0, dx_b_g2c = 0, dx_b_f = 0;
  int cu_count = 0;            // compute units of the device (the whole-chip persistent kernels need one workgroup per CU on 256 CUs)
  int dx_mode = 1;             // 0: launch-per-stage decoder; 1: persistent decoder when the configuration fits; 2: same, write-through exchanges
  int dx_rows = 0;             // debug: force the rows per group (1,2,4,8); 0 = smallest that covers the batch
  long long* d_trace = nullptr;   // debug: phase stamps of group 0 / member 0 (taco_debug_decoder_trace): [decoder half | scan half];
                                  // allocated on first use and kept until the model is destroyed (captured plans may hold the pointer)
  int trace_on = 0;
  int skip_scans = 0;          // timing hook (taco_debug_set_skip_scans): the recurrent scans of both CBHGs are not launched
  struct TrainPacks* tp = nullptr;   // set on the shadow model of a taco_train: finalize also builds the backward packs
};
static inline const float* AP(const taco_model* m, size_t off1) { return off1 ? m->darena + (off1 - 1) : nullptr; }

// ---- required tensor list (tests/test_host.py checks it against the CPU checker) ----
static void spec_add(taco_model* m, const std::string& n, std::vector<int64_t> s) { m->spec.push_back({n, s}); }
static void spec_dense(taco_model* m, const std::string& n, int i, int o, bool bias = true) {
  spec_add(m, n + "/kernel", {i, o});
  if (bias) spec_add(m, n + "/bias", {o});
}
static void spec_conv(taco_model* m, const std::string& n, int k, int i, int o) {
  spec_add(m, n + "/kernel", {k, i, o});
  spec_add(m, n + "/bias", {o});
  for (const char* p : {"gamma", "beta", "moving_mean", "moving_variance"}) spec_add(m, n + "/" + p, {o});
}
static void spec_gru(taco_model* m, const std::string& n, int i, int h) {
  spec_add(m, n + "/gates/kernel", {i + h, 2 * h});
  spec_add(m, n + "/gates/bias", {2 * h});
  spec_add(m, n + "/candidate/kernel", {i + h, h});
  spec_add(m, n + "/candidate/bias", {h});
}
static void spec_cbhg(taco_model* m, const std::string& sc, int in_dim, int K, int C, int depth, int rnn,
                      const int* projs, int nproj, int pw) {
  for (int k = 1; k <= K; ++k) spec_conv(m, sc + "/conv_bank/conv1d_" + std::to_string(k), k, in_dim, C);
  int d = K * C;
  for (int i = 0; i < nproj; ++i) {
    spec_conv(m, sc + "/proj_" + std::to_string(i + 1), pw, d, projs[i]);
    d = projs[i];
  }
  if (d != rnn) spec_dense(m, sc + "/dense", d, rnn);
  for (int i = 0; i < depth; ++i) {
    spec_dense(m, sc + "/highway_" + std::to_string(i + 1) + "/H", rnn, rnn);
    spec_dense(m, sc + "/highway_" + std::to_string(i + 1) + "/T", rnn, rnn);
  }
  spec_gru(m, sc + "/bigru/fw", rnn, rnn);
  spec_gru(m, sc + "/bigru/bw", rnn, rnn);
}
// deepvoice: the vectors computed from the speaker embedding, in the order of SpkWs::vec (before_highway, the three initial states)
static std::vector<std::string> spk_vector_names(const taco_hparams& hp) {
  std::vector<std::string> names = {"before_highway", "encoder_rnn_init", "attention_rnn_init"};
  for (int i = 0; i < hp.dec_layer_num; ++i) names.push_back("decoder_rnn_init_" + std::to_string(i + 1));
  return names;
}

static int build_spec(taco_model* m) {
  const taco_hparams& hp = m->hp;
  m->spec.clear();
  spec_add(m, "embedding", {hp.num_symbols, hp.embedding_size});
  const bool multi = hp.num_speakers > 1;
  const int spk = hp.speaker_embedding_size;
  if (multi) {
    if (spk != 1) spec_add(m, "speaker_embedding", {hp.num_speakers, spk});
    if (hp.model_type == 2) {
      const int dims[3] = {hp.enc_prenet[hp.enc_prenet_n - 1], hp.enc_rnn_size * 2, hp.attention_state_size};
      const std::vector<std::string> names = spk_vector_names(hp);
      for (size_t i = 0; i < names.size(); ++i) {
        const int dd = i < 3 ? dims[i] : hp.dec_rnn_size;
        if (spk == 1) spec_add(m, "spk/" + names[i] + "/table", {hp.num_speakers, dd});
        else spec_dense(m, "spk/" + names[i], spk, dd);
      }
    }
  }
  int d = hp.embedding_size;
  for (int i = 0; i < hp.enc_prenet_n; ++i) {
    spec_dense(m, "prenet/dense_" + std::to_string(i + 1), d, hp.enc_prenet[i]);
    d = hp.enc_prenet[i];
  }
  spec_cbhg(m, "encoder_cbhg", d, hp.enc_bank_size, hp.enc_bank_channels, hp.enc_highway_depth, hp.enc_rnn_size,
            hp.enc_proj, hp.enc_proj_n, hp.enc_proj_width);
  const int enc_out = 2 * hp.enc_rnn_size, A = hp.attention_size;
  spec_dense(m, "attention/memory_layer", enc_out, A, false);
  spec_dense(m, "attention/query_layer", hp.attention_state_size, A, false);
  spec_add(m, "attention/attention_v", {A});
  if (hp.attention_type == 2) spec_add(m, "attention/attention_score_bias", {});
  if (hp.attention_type == 1) {
    spec_add(m, "attention/attention_g", {});
    spec_add(m, "attention/attention_b", {A});
  }
  d = hp.num_mels + enc_out;
  for (int i = 0; i < hp.dec_prenet_n; ++i) {
    spec_dense(m, "decoder/prenet/dense_" + std::to_string(i + 1), d, hp.dec_prenet[i]);
    d = hp.dec_prenet[i];
  }
  const int sspk = (multi && hp.model_type == 1) ? spk : 0;   // 'simple': speaker embedding concatenated (tacotron.py:82-86)
  spec_gru(m, "decoder/attention_gru", d + sspk, hp.attention_state_size);                       // rnn_wrappers.py:372-376
  spec_dense(m, "decoder/concat_projection", hp.attention_state_size + enc_out + sspk, hp.dec_rnn_size);   // :405-413
  for (int i = 0; i < hp.dec_layer_num; ++i) spec_gru(m, "decoder/gru_" + std::to_string(i + 1), hp.dec_rnn_size, hp.dec_rnn_size);
  spec_dense(m, "decoder/frame_projection", hp.dec_rnn_size, hp.num_mels * hp.reduction_factor);
  spec_cbhg(m, "post_cbhg", hp.num_mels, hp.post_bank_size, hp.post_bank_channels, hp.post_highway_depth,
            hp.post_rnn_size, hp.post_proj, hp.post_proj_n, hp.post_proj_width);
  spec_dense(m, "linear", 2 * hp.post_rnn_size + sspk, hp.num_freq);   // tacotron.py:226-235 (embedding in front)
  return 0;
}

#include "taco_pack.h"      // the model build: every pack builder, the composite weights, model_pack_host

// ------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------
enum GemmForce { GEMM_FORCE_NONE, GEMM_FORCE_EXACT, GEMM_FORCE_BF3 };
struct GemmCall {
  const float* x = nullptr; const int* gather = nullptr; int ldx = 0;
  int M = 0, T = 0, mpw = 1, act = ACT_NONE;
  const float* res = nullptr; int ldres = 0;
  const float* rowvec = nullptr; int ldrv = 0;
  const int* rev_len = nullptr; int rev_col0 = -1;
  float* out = nullptr; int ldo = 0;
  bool tiles_only = false;         // never k_head_sweep (a CBHG's dense layer: the sweep is the linear head's kernel, cbhg_ff)
  float* aux0 = nullptr; float* aux1 = nullptr;   // highway H / T saved for the backward pass (training tape)
  int force = GEMM_FORCE_NONE;     // this call's level whatever the model's switches say (gemm_level): exact fp32, or split-bf16 at three products
};

// ---- which kernels run the feed-forward launches ----
// The arithmetic of a layer that run_gemm serves: exact fp32 (k_gemm), or operands split into bf16 planes with three products (k_gemm_bf3; the fused
// kernels exist at this level only) or six (k_gemm_bf3<..., X6>, fp32-grade: a training shadow model's default, taco_debug_set_bf3 bit 6).
// force (GemmCall::force): one call's override of the model's switches
enum GemmLevel { GEMM_EXACT, GEMM_BF3, GEMM_BF3X6 };
static GemmLevel gemm_level(const taco_model* m, const ConvL& L, int force = GEMM_FORCE_NONE) {
  const bool bf3 = force == GEMM_FORCE_BF3;
  if (force == GEMM_FORCE_EXACT || !((m->bf3 || m->bf3x6 || bf3) && m->force_cfg < 0 && L.bh)) return GEMM_EXACT;
  return (m->bf3x6 && !bf3) || (m->bf3 && L.x6) ? GEMM_BF3X6 : GEMM_BF3;
}
// First reason against a fused kernel (k_cbhg_front, k_pointwise_chain, the chain's fused entry, k_head_sweep); NONE: it runs
enum FfWhyNot { FF_WHY_NONE, FF_WHY_EXACT, FF_WHY_X6, FF_WHY_CFG, FF_WHY_TILE, FF_WHY_SWITCH, FF_WHY_WIDTHS, FF_WHY_NEEDS_BOTH };
// The term all of them share, once: L (a layer the kernel would serve) at the three-product level -- split-bf16 on, not the six-product
// level, no forced k_gemm config -- and no forced k_gemm_bf3 tile
static FfWhyNot ff_fused_why(const taco_model* m, const ConvL& L, int force = GEMM_FORCE_NONE) {
  const GemmLevel lv = gemm_level(m, L, force);
  return lv == GEMM_BF3X6 ? FF_WHY_X6 : lv == GEMM_EXACT ? (m->force_cfg >= 0 ? FF_WHY_CFG : FF_WHY_EXACT) : m->bf3_tn ? FF_WHY_TILE : FF_WHY_NONE;
}
// k_head_sweep (taco_head.h) for a dense layer L over the rows of call c: a wide layer over many rows with a plain epilogue (the linear head).
// Pure: the one term left to the launch is the 16-byte alignment of c.x -- a workspace carved by Carver (256-byte steps) has it.
static FfWhyNot head_sweep_why(const taco_model* m, const ConvL& L, int nvar, bool dual, const GemmCall& c) {
  if (const FfWhyNot why = ff_fused_why(m, L, c.force)) return why;
  if (!m->head_sweep) return FF_WHY_SWITCH;
  return nvar == 1 && !dual && L.kw == 1 && c.mpw <= 1 && !c.gather && !c.res && !c.rev_len && c.rev_col0 < 0 && !c.tiles_only && !c.aux0 && !c.aux1 &&
         c.act == ACT_NONE && !L.bns && c.ldx % 4 == 0 && (L.cin == 256 || L.cin == 512) && L.N >= 512 && L.N % 32 == L.ntail && (L.ntail == 0 || L.wtail) &&
         c.M >= 256 && (long)c.M * c.ldo < (1L << 30) ? FF_WHY_NONE : FF_WHY_WIDTHS;
}

// ---- which instantiation of k_gemm_bf3 / k_gemm a launch gets ----
// k_gemm_bf3 tiles (rows x columns of the output per workgroup); the numbers are taco_debug_set_bf3's tile_n
enum GemmTile {
  TILE_AUTO = 0,
  TILE_64x64 = 4,          // 2 x 2 waves
  TILE_64x64_K4 = 5,       // the same by four wave groups that split K
  TILE_64x256 = 7,         // one row of 8 waves side by side over the columns, two row tiles each
  TILE_64x128 = 9,         // one row of 4 waves
  TILE_64x256_K2 = 10,     // 64x256 by two wave groups that split K (16 waves per CU)
};
// k_gemm configs; the numbers are taco_debug_force_gemm_config's cfg
enum GemmCfg {
  CFG_AUTO = -1,
  CFG_64x64 = 1,           // 2 x 2 waves
  CFG_32x64_K4 = 2,        // 1 x 2 waves by four wave groups that split K
};
static inline bool gemm_tile_known(int t) { return t == TILE_AUTO || t == TILE_64x64 || t == TILE_64x64_K4 || t == TILE_64x256 || t == TILE_64x128 || t == TILE_64x256_K2; }
static inline bool gemm_cfg_known(int c) { return c == CFG_AUTO || c == CFG_64x64 || c == CFG_32x64_K4; }
// Every instantiation that exists, once: the plan takes a member's shape from here, run_gemm its kernel, gemm_set_attributes its LDS attribute.
//   X(tile, WM, WN, TM, DUAL, GPI, KS, X6): WM x WN waves per wave group, TM row tiles of 32 per wave, KS wave groups.
// What is NOT here is a rule of gemm_plan: the split-K-by-two tile exists at three products without DUAL only, GPI = 2 on the plain 64x256 tile only,
// and six products with DUAL have no four-wave-group tile (it would spill with two accumulator sets and three planes).
#define GEMM_BF3_LIST(X) \
  X(TILE_64x64, 2, 2, 1, false, 1, 1, false)     X(TILE_64x64, 2, 2, 1, true, 1, 1, false) \
  X(TILE_64x64_K4, 2, 2, 1, false, 1, 4, false)  X(TILE_64x64_K4, 2, 2, 1, true, 1, 4, false) \
  X(TILE_64x256, 1, 8, 2, false, 1, 1, false)    X(TILE_64x256, 1, 8, 2, true, 1, 1, false)    X(TILE_64x256, 1, 8, 2, false, 2, 1, false) \
  X(TILE_64x128, 1, 4, 2, false, 1, 1, false)    X(TILE_64x128, 1, 4, 2, true, 1, 1, false) \
  X(TILE_64x256_K2, 1, 8, 2, false, 1, 2, false) \
  X(TILE_64x64, 2, 2, 1, false, 1, 1, true)      X(TILE_64x64, 2, 2, 1, true, 1, 1, true) \
  X(TILE_64x64_K4, 2, 2, 1, false, 1, 4, true) \
  X(TILE_64x256, 1, 8, 2, false, 1, 1, true)     X(TILE_64x256, 1, 8, 2, true, 1, 1, true) \
  X(TILE_64x128, 1, 4, 2, false, 1, 1, true)     X(TILE_64x128, 1, 4, 2, true, 1, 1, true)
//   X(cfg, WM, WN, KS, DUAL): one 32 x 32 tile per wave
#define GEMM_EXACT_LIST(X) \
  X(CFG_64x64, 2, 2, 1, false)     X(CFG_64x64, 2, 2, 1, true) \
  X(CFG_32x64_K4, 1, 2, 4, false)  X(CFG_32x64_K4, 1, 2, 4, true)
#define GEMM_BF3_KERNEL(TILE, WM, WN, TM, DUAL, GPI, KS, X6) k_gemm_bf3<WM, WN, TM, 1, DUAL, GPI, KS, X6>
#define GEMM_EXACT_KERNEL(CFG, WM, WN, KS, DUAL) k_gemm<WM, WN, 1, 1, KS, DUAL>
// a member's name inside one level (tile: a GemmTile, or a GemmCfg for the exact level)
static constexpr int gemm_key(int tile, bool dual, int gpi, bool x6) { return tile | (dual ? 16 : 0) | (gpi == 2 ? 32 : 0) | (x6 ? 64 : 0); }

struct GemmPlan {
  GemmLevel level = GEMM_EXACT;
  bool head_sweep = false;     // k_head_sweep<K> instead of a tile kernel (three-product level only)
  bool x6 = false;             // the six-product instantiation (level GEMM_BF3X6 and every layer of the launch has its third planes)
  int tile = 0;                // GemmTile (split-bf16 levels) or GemmCfg (exact level)
  int gpi = 1;                 // k_gemm_bf3: k16 steps per weight prefetch group
  dim3 grid = dim3(0, 0, 0); unsigned block = 0; size_t lds = 0;      // block 0: the list has no such member
};
// Everything a run_gemm launch decides, from integers and the model's switches alone (x_aligned: c.x on a 16-byte boundary, see head_sweep_why)
static GemmPlan gemm_plan(const taco_model* m, const ConvL* layers, int nvar, bool dual, const GemmCall& c, bool x_aligned) {
  GemmPlan p;
  const ConvL& L0 = layers[0];
  int kw_max = 1, Nmax = 0;
  for (int i = 0; i < nvar; ++i) { kw_max = std::max(kw_max, layers[i].kw); Nmax = std::max(Nmax, layers[i].N); }
  const bool vec_ok = c.ldx % 4 == 0 && L0.cin % 4 == 0 && x_aligned;
  p.level = gemm_level(m, L0, c.force);
  int BM = 0, BN = 0, KS = 1, waves = 0, tiles = 0;      // of the member: rows, columns, wave groups, waves per group, 32 x 32 tiles per wave
  if (p.level != GEMM_EXACT) {      // split-bf16 (every feed-forward layer of inference)
    // a wide dense layer over many rows (the linear head): every workgroup keeps its 64 rows for ALL columns (taco_head.h)
    if (vec_ok && head_sweep_why(m, L0, nvar, dual, c) == FF_WHY_NONE) {
      p.head_sweep = true;
      p.grid = dim3(cdiv(c.M, HD_BM)); p.block = 512; p.lds = (size_t)2 * HD_BM * (L0.cin + 8) * sizeof(unsigned short);
      return p;
    }
    p.tile = m->bf3_tn;
    if (p.tile == TILE_AUTO) {
      // measured (tools/time_gemm_layers.py).  Small-M layers (encoder, short utterances): 64x64 tiles; if even those leave most CUs idle, four
      // wave groups per workgroup split K.  Otherwise one row of waves side by side over the columns (64x256 by 1x8 waves, 64x128 by 1x4): every
      // wave streams its OWN weight columns and all of them share the staged activation tile, so no weight fragment is fetched twice by a
      // workgroup (2x2 arrangements of larger tiles fetch each one twice through a 16 KB L1 that cannot hold them: measured 20-30 % slower on
      // every large layer; a 128 x 256 tile by 1 x 8 waves measured slower on the linear head, 116 vs 85 us: one workgroup of 8 waves per CU and
      // three rounds of workgroups.  Both were retired.)
      const int Ktot = L0.kw * L0.cin;
      const long g128 = (long)cdiv(c.M, 128) * cdiv(Nmax, 64) * nvar, g64 = (long)cdiv(c.M, 64) * cdiv(Nmax, 64) * nvar;
      const long wide = (long)cdiv(c.M, 64) * cdiv(Nmax, 256) * nvar;      // workgroups of the 64x256 tile
      if (g128 < 384 && !((Ktot >= 1024 || Nmax > 512) && wide >= 192)) p.tile = g64 >= 384 ? TILE_64x64 : TILE_64x64_K4;
      else if (Nmax <= 128) p.tile = TILE_64x128;
      else p.tile = (!dual && wide <= 320) ? TILE_64x256_K2 : TILE_64x256;      // few workgroups: two wave groups split K (16 waves/CU)
    }
    // six products (fp32-grade): the training forward (taco_train_set_exact_gemm mode 4); needs the third planes of every layer of the launch
    p.x6 = p.level == GEMM_BF3X6;
    for (int i = 0; i < nvar; ++i) p.x6 = p.x6 && layers[i].bl3 && (!dual || layers[i].bl3_2);
    // what the list does not have, chosen or forced: the same tile without split-K
    if (p.tile == TILE_64x256_K2 && (dual || p.x6)) p.tile = TILE_64x256;
    if (p.tile == TILE_64x64_K4 && dual && p.x6) p.tile = TILE_64x64;
    switch (gemm_key(p.tile, dual, 1, p.x6)) {
#define X(TILE, WM, WN, TM, DUAL, GPI, KS_, X6) case gemm_key(TILE, DUAL, GPI, X6): BM = WM * TM * 32; BN = WN * 32; KS = KS_; waves = WM * WN; tiles = TM; break;
      GEMM_BF3_LIST(X)
#undef X
      default: return p;
    }
    p.lds = (size_t)KS * (p.x6 ? 3 : 2) * (BM + 15) * BF3_LDSW * sizeof(unsigned short);
    if (KS > 1) p.lds = std::max(p.lds, (size_t)(KS - 1) * waves * tiles * 16 * 64 * (dual ? 2 : 1) * sizeof(float));      // split-K reduction
  } else {
    p.tile = m->force_cfg;
    if (p.tile == CFG_AUTO) {
      // measured (tools/time_gemm_layers.py): the 64x64 tile (32 VGPRs, 8 waves/SIMD) beats 128x64 and 128x128 (retired) on
      // every large layer -- the kernel is bound by latency hiding, not operand reuse; small-M layers need split-K
      p.tile = (long)cdiv(c.M, 64) * cdiv(Nmax, 64) * nvar >= 512 ? CFG_64x64 : CFG_32x64_K4;
    }
    switch (gemm_key(p.tile, dual, 1, false)) {
#define X(CFG, WM, WN, KS_, DUAL) case gemm_key(CFG, DUAL, 1, false): BM = WM * 32; BN = WN * 32; KS = KS_; waves = WM * WN; tiles = 1; break;
      GEMM_EXACT_LIST(X)
#undef X
      default: return p;
    }
    p.lds = (size_t)(BM + kw_max - 1) * TACO_LDSW * sizeof(float);
    if (KS > 1) p.lds = std::max(p.lds, (size_t)(KS - 1) * waves * 1024 * (dual ? 2 : 1) * sizeof(float));
  }
  p.grid = dim3(cdiv(c.M, BM), cdiv(Nmax, BN), nvar);
  p.block = 64 * waves * KS;
  // weight prefetch depth of k_gemm_bf3: two k16 steps ahead when the grid leaves at most ~2 workgroups per CU (occupancy is grid-limited there);
  // instantiated for the plain 64x256 tile only, and it needs four k16 steps in every chunk (even group count)
  if (p.level != GEMM_EXACT && p.tile == TILE_64x256 && !dual && !p.x6 && (long)p.grid.x * p.grid.y * p.grid.z <= 320) {
    p.gpi = 2;
    for (int i = 0; i < nvar; ++i) if (layers[i].cin_pad16 % 64) p.gpi = 1;
  }
  return p;
}
// > 64 KB of dynamic LDS has to be asked for, per kernel and device: the split-K members (taco_model_finalize, taco_gl_create)
static int gemm_set_attributes() {
#define X(TILE, WM, WN, TM, DUAL, GPI, KS, X6) \
  if (KS > 1) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&GEMM_BF3_KERNEL(TILE, WM, WN, TM, DUAL, GPI, KS, X6)), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  GEMM_BF3_LIST(X)
#undef X
  return 0;
}
static int run_gemm(const taco_model* m, hipStream_t st, const ConvL* layers, int nvar, bool dual, const GemmCall& c) {
  GemmArgs a;
  memset(&a, 0, sizeof a);
  const ConvL& L0 = layers[0];
  const bool x_aligned = (reinterpret_cast<uintptr_t>(c.x) & 15) == 0;
  a.x = c.x; a.gather = c.gather; a.res = c.res; a.rowvec = c.rowvec; a.out = c.out;
  a.ldx = c.ldx; a.M = c.M; a.T = c.T > 0 ? c.T : c.M; a.Cin = L0.cin; a.cin_pad = L0.cin_pad; a.mpw = c.mpw;
  a.act = c.act; a.ldres = c.ldres; a.ldrv = c.ldrv; a.ldo = c.ldo; a.rev_len = c.rev_len; a.rev_col0 = c.rev_col0;
  a.aux0 = c.aux0; a.aux1 = c.aux1;
  a.vec_ok = (c.ldx % 4 == 0) && (L0.cin % 4 == 0) && x_aligned;
  for (int i = 0; i < nvar && i < 16; ++i) {
    if (layers[i].var_index < 0) return fail(TACO_ERR_STATE, "layer has no GemmVar");
    a.v[i] = m->hvars[layers[i].var_index];
  }
  if (nvar > 16) return fail(TACO_ERR_UNSUPPORTED, "conv bank wider than 16 is not supported");
  const GemmPlan p = gemm_plan(m, layers, nvar, dual, c, x_aligned);
  if (p.head_sweep) {
    HeadArgs h;
    memset(&h, 0, sizeof h);
    h.x = c.x; h.ldx = c.ldx; h.bh = a.v[0].bh; h.bl = a.v[0].bl; h.NT = a.v[0].NT; h.K16 = L0.cin / 16; h.bias = a.v[0].bias;
    h.wtail = L0.wtail ? AP(m, L0.wtail) : nullptr; h.ntail = L0.ntail; h.rowvec = c.rowvec; h.ldrv = c.ldrv; h.T = a.T;
    h.out = c.out; h.ldo = c.ldo; h.M = c.M; h.K = L0.cin; h.N = L0.N;
    if (L0.cin == 512) hipLaunchKernelGGL(k_head_sweep<512>, p.grid, dim3(p.block), p.lds, st, h);
    else hipLaunchKernelGGL(k_head_sweep<256>, p.grid, dim3(p.block), p.lds, st, h);
    HIPCHK(hipGetLastError());
    return 0;
  }
  void (*kernel)(const GemmArgs) = nullptr;
  if (p.level != GEMM_EXACT) {
    switch (gemm_key(p.tile, dual, p.gpi, p.x6)) {
#define X(TILE, WM, WN, TM, DUAL, GPI, KS, X6) case gemm_key(TILE, DUAL, GPI, X6): kernel = GEMM_BF3_KERNEL(TILE, WM, WN, TM, DUAL, GPI, KS, X6); break;
      GEMM_BF3_LIST(X)
#undef X
    }
  } else {
    switch (gemm_key(p.tile, dual, 1, false)) {
#define X(CFG, WM, WN, KS, DUAL) case gemm_key(CFG, DUAL, 1, false): kernel = GEMM_EXACT_KERNEL(CFG, WM, WN, KS, DUAL); break;
      GEMM_EXACT_LIST(X)
#undef X
    }
  }
  if (!kernel) return fail(TACO_ERR_STATE, "gemm_plan names a k_gemm / k_gemm_bf3 instantiation that does not exist");
  hipLaunchKernelGGL(kernel, p.grid, dim3(p.block), p.lds, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- skinny jobs ----
static SkJob sk_base(const taco_model* m, const SkW& w, const float* x0, int ldx0, int K0, const float* x1, int ldx1) {
  SkJob j;
  memset(&j, 0, sizeof j);
  j.x0 = x0; j.ldx0 = ldx0; j.K0 = K0; j.x1 = x1; j.ldx1 = ldx1;
  j.K = w.K; j.Kq = w.Kq; j.N = w.N; j.wp = AP(m, w.wp); j.bias = AP(m, w.bias);
  return j;
}
static SkJob sk_linear(const taco_model* m, const SkW& w, const float* x0, int ldx0, int K0, const float* x1, int ldx1,
                       int act, float* out, int ldo) {
  SkJob j = sk_base(m, w, x0, ldx0, K0, x1, ldx1);
  j.act = act; j.o0 = out; j.ldo0 = ldo;
  return j;
}
// fp32 MFMA sustains only 256 FLOP/clk per CU, so the MFMA chain of a stage is kept short by giving every
// 16-row tile of the batch its own workgroup (grid.y) instead of looping row tiles inside one.
template <int EPI>
static void launch_skinny_rt(hipStream_t st, int rowgroups, int tiles, bool vec, const SkArgs& a) {
  const bool multi = a.njobs > 1;
  const dim3 grid(tiles, rowgroups), blk(64 * SK_NW);
  if (vec && !multi) hipLaunchKernelGGL((k_skinny<1, EPI, true, false>), grid, blk, 0, st, a);
  else if (vec) hipLaunchKernelGGL((k_skinny<1, EPI, true, true>), grid, blk, 0, st, a);
  else if (!multi) hipLaunchKernelGGL((k_skinny<1, EPI, false, false>), grid, blk, 0, st, a);
  else hipLaunchKernelGGL((k_skinny<1, EPI, false, true>), grid, blk, 0, st, a);
}
// all jobs of one launch share the epilogue type
static int run_skinny(hipStream_t st, int R, SkJob* jobs, int njobs, int epi = EPI_LINEAR) {
  if (R > 64) return fail(TACO_ERR_UNSUPPORTED, "batch %d > 64 rows per device is not supported: shard the batch", R);
  SkArgs a;
  memset(&a, 0, sizeof a);
  a.R = R; a.njobs = njobs;
  int tiles = 0;
  bool vec = true;
  // float4 activation loads are legal when every row segment is 16-byte aligned and a multiple of 4 long
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  for (int i = 0; i < njobs; ++i) {
    const SkJob& j = jobs[i];
    vec = vec && (j.K0 % 4 == 0) && (j.K % 4 == 0) && (j.ldx0 % 4 == 0) && al16(j.x0) && (!j.x1 || ((j.ldx1 % 4 == 0) && al16(j.x1)));
    jobs[i].tile0 = tiles; tiles += cdiv(jobs[i].N, 16); a.j[i] = jobs[i];
  }
  const int RG = cdiv(R, 16);
  if (epi == EPI_LINEAR) launch_skinny_rt<EPI_LINEAR>(st, RG, tiles, vec, a);
  else if (epi == EPI_GRU_GATES) launch_skinny_rt<EPI_GRU_GATES>(st, RG, tiles, vec, a);
  else launch_skinny_rt<EPI_GRU_CAND>(st, RG, tiles, vec, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// One GRUCell step for a decoder GRU (A.6), two launches: gates (+ x-part of candidate) then candidate.
//   x [R, I] (ldx), h [R, H] updated in place; out_res (optional) = h' + x (ResidualWrapper, tacotron.py:172)
//   ldh: row stride of h (0 = H).  ldxc > 0: the gates launch writes [x-part of candidate | extra columns] rows of that stride into xc
//   (folded cells: the extra columns are the cell input itself, which the residual then reads from there instead of from x).
static int run_gru_cell(const taco_model* m, hipStream_t st, const GruDec& g, int R, const float* x, int ldx,
                        float* h, float* rh, float* u, float* xc, float* out_res, int ldh = 0, int ldxc = 0) {
  if (!ldh) ldh = g.H;
  const int lxc = ldxc ? ldxc : g.H;
  SkJob ja = sk_base(m, g.gx, x, ldx, g.I, h, ldh);
  ja.H = g.H; ja.e0 = h; ja.lde0 = ldh; ja.o0 = rh; ja.ldo0 = g.H; ja.o1 = u; ja.ldo1 = g.H; ja.o2 = xc; ja.ldo2 = lxc;
  TRY(run_skinny(st, R, &ja, 1, EPI_GRU_GATES));
  SkJob jb = sk_base(m, g.ch, rh, g.H, g.H, nullptr, 0);
  jb.H = g.H; jb.e0 = h; jb.lde0 = ldh; jb.e1 = xc; jb.lde1 = lxc; jb.e2 = u; jb.lde2 = g.H;
  jb.o0 = h; jb.ldo0 = ldh;
  if (out_res) {
    if (ldxc) { jb.e3 = xc + g.H; jb.lde3 = lxc; } else { jb.e3 = x; jb.lde3 = ldx; }
    jb.o1 = out_res; jb.ldo1 = g.H;
  }
  TRY(run_skinny(st, R, &jb, 1, EPI_GRU_CAND));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// workspace carving
// ------------------------------------------------------------------------------------------------
struct Carver {
  char* base; size_t off = 0, cap;
  Carver(void* p, size_t c) : base((char*)p), cap(c) {}
  float* f(size_t n) { return (float*)raw(n * sizeof(float)); }
  int* i(size_t n) { return (int*)raw(n * sizeof(int)); }
  void* raw(size_t bytes) {
    void* p = base ? base + off : nullptr;
    off += rup_sz(bytes, 256);
    return p;
  }
  bool ok() const { return !base || off <= cap; }
};

// The exchange of a whole-chip persistent kernel: its granules and, carved back to back behind them, 256 bytes of census words -- all of it polled
struct Xchg : Polled {
  void carve(Carver& cv, size_t granules) { bytes = rup_sz(granules * sizeof(unsigned long long), 256) + 256; p = cv.raw(bytes); }
  unsigned long long* buf() const { return static_cast<unsigned long long*>(p); }
  unsigned* ctl() const { return p ? reinterpret_cast<unsigned*>(static_cast<char*>(p) + bytes - 256) : nullptr; }
};

struct CbhgWs { float *bank, *p[4], *hi0, *hi1, *xproj, *h, *rh, *u; Xchg gx; };
static void carve_cbhg(Carver& cv, const Cbhg& c, int B, int T, CbhgWs& w) {
  const size_t M = (size_t)B * T;
  w.bank = cv.f(M * c.K * c.C);
  for (int i = 0; i < c.nproj; ++i) w.p[i] = cv.f(M * c.proj_dim[i]);
  w.hi0 = cv.f(M * c.rnn); w.hi1 = cv.f(M * c.rnn);
  w.xproj = cv.f(M * 6 * c.rnn);
  w.h = cv.f((size_t)2 * B * c.rnn); w.rh = cv.f((size_t)2 * B * c.rnn); w.u = cv.f((size_t)2 * B * c.rnn);
  // exchange granules of the whole-chip forward scans: k_bigru_duo at its 8 rows per group needs the most (a training tape carves its own)
  static_assert(gd_xbuf_granules(8) == (size_t)16 * 2 * 8 * 256 && gd_xbuf_granules(8) >= go_xbuf_granules(), "gx holds the granules of k_bigru_duo<8> and of k_bigru_oct");
  w.gx.carve(cv, gd_xbuf_granules(8));
}

// Row-parallel persistent BiGRU: R rows per workgroup.  Returns false when it does not fit.
static bool bigru_rows_cfg(int B, int H, int* R_out, size_t* lds_out) {
  if (H % 4) return false;
  for (int R : {2, 1}) {                                   // R = 4 spills at the 128-VGPR budget of a 1024-thread workgroup
    if (R > 1 && B < R) continue;
    if ((size_t)R * 2 * H > 2 * RP_NT) continue;          // <= 2 gate outputs per thread
    const size_t fl = (size_t)3 * R * H + (size_t)RP_NT * R * 4 + 64;
    if (fl * sizeof(float) <= 160 * 1024) { *R_out = R; *lds_out = fl * sizeof(float); return true; }
  }
  return false;
}

static size_t bigru_res_lds(int H, int KL, int R) {
  const int NQ = 512 / H;
  return ((size_t)3 * R * H + (size_t)NQ * R * 3 * H) * sizeof(float) + (size_t)KL * NQ * H * 3 * sizeof(float);
}

// The whole-chip persistent kernels (BiGRU scans, decoder loop and its backward loop): one workgroup per CU, all resident at once -- only on a whole MI355X (a partition
// of it -- CPX / DPX modes -- or a smaller part would leave workgroups waiting for CUs held by workgroups that wait for them); at most 8 rows on each of the 8 groups
static constexpr int CHIP_CUS = DX_NGROUP * DX_GROUP, CHIP_ROWS = 8 * DX_NGROUP;
// ---- which BiGRU scan runs ----
// taco_debug_set_persistent(m, mode): SCAN_AUTO is the default; the others force one engine where it fits (A/B tests, tools/).
enum ScanMode { SCAN_PER_STEP = 0, SCAN_AUTO = 1, SCAN_ROWS = 2, SCAN_RES = 3, SCAN_RESW = 7, SCAN_OCT = 10, SCAN_DUO = 11 };
enum ScanKernel { SCAN_K_STEPS, SCAN_K_ROWS, SCAN_K_RES, SCAN_K_QUAD, SCAN_K_RESW, SCAN_K_DUO, SCAN_K_OCT };
enum ScanBwd { SCAN_BWD_ROWS, SCAN_BWD_DUO, SCAN_BWD_OCT };       // ROWS: the per-row kernels (k_bigru_resb / k_bigru_rows_bwd, picked by width)
enum ScanWhyNot { SCAN_WHY_NONE, SCAN_WHY_ENGINE_OFF, SCAN_WHY_CUS, SCAN_WHY_ROWS, SCAN_WHY_MODE, SCAN_WHY_WIDTH, SCAN_WHY_FRAMES };
struct ScanPlan {
  ScanKernel kernel;        // what bigru_scan launches (the training forward runs the TAPE instantiation of it where there is one)
  int upw;                  // k_bigru_oct: units per wave -- one row per cluster of 32 / upw CUs
  int rg;                   // k_bigru_duo / k_bigru_duo_bwd: rows per group of 32 CUs
  ScanBwd bwd;              // the backward scan of a training step
  ScanWhyNot why_not_whole_chip;      // first reason against k_bigru_duo (NONE: it fits; k_bigru_oct needs no more, only fewer rows)
};
// The one place that decides.  Pure: launches nothing, touches no device state.
// tape: the training forward -- below the whole-chip kernels only k_bigru_res / k_bigru_quad / k_bigru_rows have TAPE instantiations,
// and a forced mode does not choose among them (SCAN_K_STEPS then means: no kernel fits).
static ScanPlan scan_plan(const taco_model* m, const Cbhg& c, int B, int T, bool tape = false) {
  const int mode = m->persist, H = c.rnn;
  ScanPlan p = {SCAN_K_STEPS, 0, 1, SCAN_BWD_ROWS, SCAN_WHY_NONE};
  while (p.rg * DX_NGROUP < B) p.rg *= 2;
  // the whole-chip kernels (taco_bigru_xcd.h): H = 256, an unpartitioned MI355X, the decoder engine not switched off
  const bool chip = m->dx_mode && H == GX_H && T >= 2 && m->cu_count >= CHIP_CUS;
  if (!m->dx_mode) p.why_not_whole_chip = SCAN_WHY_ENGINE_OFF;
  else if (m->cu_count < CHIP_CUS) p.why_not_whole_chip = SCAN_WHY_CUS;
  else if (B > CHIP_ROWS) p.why_not_whole_chip = SCAN_WHY_ROWS;
  else if (mode != SCAN_AUTO && mode != SCAN_OCT && mode != SCAN_DUO) p.why_not_whole_chip = SCAN_WHY_MODE;
  else if (H != GX_H || !c.gd_pack) p.why_not_whole_chip = SCAN_WHY_WIDTH;
  else if (T < 2) p.why_not_whole_chip = SCAN_WHY_FRAMES;
  // k_bigru_oct: up to 32 rows.  SCAN_AUTO: from 9 rows on -- up to eight rows k_bigru_duo<1> IS the one-row geometry on 32 CUs;
  // SCAN_OCT: wherever it fits; SCAN_DUO: never (round 4's engine)
  if (chip && (mode == SCAN_AUTO || mode == SCAN_OCT) && c.go_pack[0] && B <= 32) p.upw = B > 16 ? 4 : B > 8 ? 2 : mode == SCAN_OCT ? 1 : 0;
  if (p.upw) p.kernel = SCAN_K_OCT;
  else if (p.why_not_whole_chip == SCAN_WHY_NONE) p.kernel = SCAN_K_DUO;
  // weights resident on the CU, one (direction, row) per workgroup.  H = 256: four units per thread, k_bigru_resw 3.74 us/step (one unit
  // per thread, k_bigru_res: 5.7; re-streaming everything, k_bigru_rows: 7.1); H = 128: k_bigru_quad (SCAN_RES: its libm reference)
  else if (!tape && (mode == SCAN_AUTO || mode == SCAN_RESW) && H == 256) p.kernel = SCAN_K_RESW;
  else if ((tape || mode == SCAN_AUTO || mode == SCAN_RES) && (H == 256 || H == 128)) p.kernel = H == 128 && mode == SCAN_AUTO ? SCAN_K_QUAD : SCAN_K_RES;
  else {      // any other width, or a forced mode that does not fit: the whole scan in one launch, weights streamed from L2 every step
    int R = 0; size_t lds = 0;
    p.kernel = (tape || mode != SCAN_PER_STEP) && bigru_rows_cfg(B, H, &R, &lds) ? SCAN_K_ROWS : SCAN_K_STEPS;
  }
  // the backward scans run on the geometry of the forward one where the training packs exist
  if (p.why_not_whole_chip == SCAN_WHY_NONE && c.gb_pack) p.bwd = p.upw && c.gob_pack ? SCAN_BWD_OCT : SCAN_BWD_DUO;
  return p;
}
static const char* scan_kernel_name(ScanKernel k) {
  static const char* const names[] = {"two launches per step", "k_bigru_rows", "k_bigru_res", "k_bigru_quad", "k_bigru_resw", "k_bigru_duo", "k_bigru_oct"};
  return names[k];
}

// A/B build -DGO_KNOB_RT: the twelve knobs of k_bigru_oct and (entries 12..15) the four second requests of k_bigru_oct_bwd from
// TACO_GO_KNOB (taco_bigru_xcd.h); eager launches only
static int go_knob_upload() {
#ifdef GO_KNOB_RT
  int d[16]; for (int i = 0; i < 16; ++i) d[i] = i < 12 ? go_knob_default(i) : gob_knob_default(i - 12);
  if (const char* e = getenv("TACO_GO_KNOB")) { int i = 0; const char* p = e; while (*p && i < 16) { d[i++] = atoi(p); while (*p && *p != ',') ++p; if (*p == ',') ++p; } }
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_go_knob), d, sizeof d));
#endif
  return 0;
}
template <bool TAPE, bool TRACE>
static void duo_launch_rg(int RG, dim3 grid, dim3 blk, size_t lds, hipStream_t st, const GdArgs& a) {
  switch (RG) {
    case 1: hipLaunchKernelGGL((k_bigru_duo<1, TAPE, TRACE>), grid, blk, lds, st, a); break;
    case 2: hipLaunchKernelGGL((k_bigru_duo<2, TAPE, TRACE>), grid, blk, lds, st, a); break;
    case 4: hipLaunchKernelGGL((k_bigru_duo<4, TAPE, TRACE>), grid, blk, lds, st, a); break;
    default: hipLaunchKernelGGL((k_bigru_duo<8, TAPE, TRACE>), grid, blk, lds, st, a); break;
  }
}
template <bool TAPE, bool TRACE>
static void oct_launch_upw(int UPW, dim3 grid, dim3 blk, size_t lds, hipStream_t st, const GdArgs& a) {
  switch (UPW) {
    case 1: hipLaunchKernelGGL((k_bigru_oct<1, TAPE, TRACE>), grid, blk, lds, st, a); break;
    case 2: hipLaunchKernelGGL((k_bigru_oct<2, TAPE, TRACE>), grid, blk, lds, st, a); break;
    default: hipLaunchKernelGGL((k_bigru_oct<4, TAPE, TRACE>), grid, blk, lds, st, a); break;
  }
}
// both directions of RG rows on one group of 32 CUs, software-pipelined against each other; gsave != null: the TAPE instantiation
static int duo_launch(const taco_model* m, hipStream_t st, const Cbhg& c, int RG, int B, int T, const float* xproj, const int* lengths, const float* init_state,
                      float* out, float* gsave, const Xchg& gx) {
  ChipTurn turn(m->device, st);
  GdArgs a; memset(&a, 0, sizeof a);
  a.wpack = AP(m, c.gd_pack); a.xproj = xproj; a.h0 = init_state; a.lengths = lengths; a.out = out; a.gsave = gsave;
  a.xbuf = gx.buf(); a.ctl = gx.ctl(); a.err = m->d_err; a.trace = (m->trace_on && m->d_trace && !gsave) ? m->d_trace + DX_TRACE_STEPS * DX_TRACE_SLOTS : nullptr;
  a.B = B; a.T = T; a.force_wt = m->dx_mode == 2 ? 1 : 0;
  HIPCHK(gx.clear(st));
  const size_t lds = std::max(gd_lds_floats(RG) * sizeof(float), (size_t)96 * 1024);      // one workgroup per CU
  const dim3 grid(DX_NGROUP * GD_MEMBERS), blk(512);
  if (a.trace) duo_launch_rg<false, true>(RG, grid, blk, lds, st, a);          // the stamped instantiations (tools/trace_bigru.py): inference only
  else if (gsave) duo_launch_rg<true, false>(RG, grid, blk, lds, st, a);
  else duo_launch_rg<false, false>(RG, grid, blk, lds, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}
// the backward scan on the geometry of k_bigru_duo: both directions of RG rows per group of 32 CUs, software-pipelined against each other.
// Unlike the forward launchers, this one and oct_bwd_launch do not clear gx: their caller has (cbhg_backward says why)
static int duo_bwd_launch(const taco_model* m, hipStream_t st, const Cbhg& c, int RG, int B, int T, const float* dout, const float* out, const float* gsave,
                          const float* h0, const int* lengths, float* dg, float* rh, float* dh0, const Xchg& gx) {
  ChipTurn turn(m->device, st);
  GbArgs a; memset(&a, 0, sizeof a);
  a.wpack = AP(m, c.gb_pack); a.dout = dout; a.out = out; a.gsave = gsave; a.h0 = h0; a.lengths = lengths; a.dg = dg; a.rh = rh; a.dh0 = dh0;
  a.xbuf = gx.buf(); a.ctl = gx.ctl(); a.err = m->d_err; a.B = B; a.T = T; a.force_wt = m->dx_mode == 2 ? 1 : 0;
  const size_t lds = std::max(gb_lds_floats(RG) * sizeof(float), (size_t)96 * 1024);      // one workgroup per CU
  const dim3 grid(DX_NGROUP * GD_MEMBERS), blk(512);
  switch (RG) {
    case 1: hipLaunchKernelGGL((k_bigru_duo_bwd<1>), grid, blk, lds, st, a); break;
    case 2: hipLaunchKernelGGL((k_bigru_duo_bwd<2>), grid, blk, lds, st, a); break;
    case 4: hipLaunchKernelGGL((k_bigru_duo_bwd<4>), grid, blk, lds, st, a); break;
    default: hipLaunchKernelGGL((k_bigru_duo_bwd<8>), grid, blk, lds, st, a); break;
  }
  HIPCHK(hipGetLastError());
  return 0;
}
// the backward scan on the geometry of k_bigru_oct (k_bigru_oct_bwd; four units per wave: up to 32 rows), where the forward scan runs on it
static int oct_bwd_launch(const taco_model* m, hipStream_t st, const Cbhg& c, int B, int T, const float* dout, const float* out, const float* gsave,
                          const float* h0, const int* lengths, float* dg, float* rh, float* dh0, const Xchg& gx) {
  ChipTurn turn(m->device, st);
  TRY(go_knob_upload());
  GbArgs a; memset(&a, 0, sizeof a);
  a.wpack = AP(m, c.gob_pack); a.dout = dout; a.out = out; a.gsave = gsave; a.h0 = h0; a.lengths = lengths; a.dg = dg; a.rh = rh; a.dh0 = dh0;
  a.xbuf = gx.buf(); a.ctl = gx.ctl(); a.err = m->d_err; a.B = B; a.T = T; a.force_wt = m->dx_mode == 2 ? 1 : 0;
  const size_t lds = std::max(gob_lds_floats() * sizeof(float), (size_t)96 * 1024);      // one workgroup per CU
  hipLaunchKernelGGL(k_bigru_oct_bwd, dim3(CHIP_CUS), dim3(512), lds, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}
// k_bigru_oct: one row per cluster of 32 / UPW CUs (UPW = 4: up to 32 rows, 2: 16, 1: 8); gsave != null: the TAPE instantiation
static int oct_launch(const taco_model* m, hipStream_t st, const Cbhg& c, int UPW, int B, int T, const float* xproj, const int* lengths, const float* init_state,
                      float* out, float* gsave, const Xchg& gx) {
  ChipTurn turn(m->device, st);
  TRY(go_knob_upload());
  GdArgs a; memset(&a, 0, sizeof a);
  a.wpack = AP(m, c.go_pack[UPW == 4 ? 2 : UPW == 2 ? 1 : 0]); a.xproj = xproj; a.h0 = init_state; a.lengths = lengths; a.out = out; a.gsave = gsave;
  a.xbuf = gx.buf(); a.ctl = gx.ctl(); a.err = m->d_err; a.trace = (m->trace_on && m->d_trace && !gsave) ? m->d_trace + DX_TRACE_STEPS * DX_TRACE_SLOTS : nullptr;
  a.B = B; a.T = T; a.force_wt = m->dx_mode == 2 ? 1 : 0;
  HIPCHK(gx.clear(st));
  const size_t lds = std::max(go_lds_floats(UPW) * sizeof(float), (size_t)96 * 1024);      // one workgroup per CU
  const dim3 grid(CHIP_CUS), blk(512);
  if (a.trace) oct_launch_upw<false, true>(UPW, grid, blk, lds, st, a);        // the stamped instantiations (tools/trace_bigru.py): inference only
  else if (gsave) oct_launch_upw<true, false>(UPW, grid, blk, lds, st, a);
  else oct_launch_upw<false, false>(UPW, grid, blk, lds, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// BiGRU (modules.py:82-96 -> TF bidirectional_dynamic_rnn, A.7): hoisted x.[Wg_x|Wc_x]+b for both
// directions as one GEMM, then the scan that scan_plan picks; without a single-launch kernel, T sequential steps of two launches
// (gates; candidate+update), both directions side by side in each launch.  x [B*T, rnn], out [B*T, 2*rnn].
static int bigru_scan(const taco_model* m, hipStream_t st, const Cbhg& c, int B, int T,
                      const int* lengths, const float* init_state, float* out, const CbhgWs& w) {
  const int H = c.rnn;
  if (m->skip_scans) return 0;
  const ScanPlan sp = scan_plan(m, c, B, T);
  if (sp.kernel == SCAN_K_OCT) return oct_launch(m, st, c, sp.upw, B, T, w.xproj, lengths, init_state, out, nullptr, w.gx);
  if (sp.kernel == SCAN_K_DUO) return duo_launch(m, st, c, sp.rg, B, T, w.xproj, lengths, init_state, out, nullptr, w.gx);
  if (sp.kernel == SCAN_K_RESW || sp.kernel == SCAN_K_RES || sp.kernel == SCAN_K_QUAD) {
    BigruSArgs a; memset(&a, 0, sizeof a);
    a.xproj = w.xproj; a.g2_0 = (const float2*)AP(m, c.res_g2[0]); a.g2_1 = (const float2*)AP(m, c.res_g2[1]);
    a.c1_0 = AP(m, c.raw_ch[0]); a.c1_1 = AP(m, c.raw_ch[1]); a.h0 = init_state; a.lengths = lengths; a.out = out; a.B = B; a.T = T;
    const dim3 grid(2 * B);
    if (sp.kernel == SCAN_K_RESW) {      // wave-local exchanges, a thread's four units adjacent in the (column-permuted) packs
      a.g2_0 = (const float2*)AP(m, c.res_g2p[0]); a.g2_1 = (const float2*)AP(m, c.res_g2p[1]); a.c1_0 = AP(m, c.res_c1p[0]); a.c1_1 = AP(m, c.res_c1p[1]);
      const size_t lds = ((size_t)3 * H + (size_t)8 * 3 * H) * sizeof(float) + (size_t)4 * 8 * H * 12;      // state, r*h, u; 8 waves of partial sums; KL = 4 rows per K-slice
      hipLaunchKernelGGL((k_bigru_resw<16, 4, 2>), grid, dim3(512), lds, st, a);
    }
    else if (sp.kernel == SCAN_K_QUAD) hipLaunchKernelGGL(k_bigru_quad<false>, grid, dim3(512), 0, st, a);       // quad-local K split: two barriers per step
    else if (H == 256) hipLaunchKernelGGL((k_bigru_res<256, 64, 24, 1, false>), grid, dim3(512), bigru_res_lds(256, 24, 1), st, a);
    else hipLaunchKernelGGL((k_bigru_res<128, 32, 0, 1, false>), grid, dim3(512), bigru_res_lds(128, 0, 1), st, a);
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (sp.kernel == SCAN_K_ROWS) {
    int R = 0; size_t lds = 0;
    bigru_rows_cfg(B, H, &R, &lds);
    BigruRArgs a; memset(&a, 0, sizeof a);
    a.xproj = w.xproj; a.wg0 = AP(m, c.raw_gh[0]); a.wg1 = AP(m, c.raw_gh[1]); a.wc0 = AP(m, c.raw_ch[0]); a.wc1 = AP(m, c.raw_ch[1]);
    a.h0 = init_state; a.lengths = lengths; a.out = out; a.B = B; a.T = T; a.H = H;
    const dim3 grid(2 * cdiv(B, R));
    if (R == 2) hipLaunchKernelGGL((k_bigru_rows<2, false>), grid, dim3(RP_NT), lds, st, a);
    else hipLaunchKernelGGL((k_bigru_rows<1, false>), grid, dim3(RP_NT), lds, st, a);
    HIPCHK(hipGetLastError());
    return 0;
  }
  for (int dir = 0; dir < 2; ++dir)
    hipLaunchKernelGGL(k_copy2d, dim3(cdiv(B * H, 256)), dim3(256), 0, st, init_state ? init_state + dir * H : nullptr,
                       2 * H, w.h + (size_t)dir * B * H, H, B, H);
  HIPCHK(hipGetLastError());
  for (int s = 0; s < T; ++s) {
    SkJob ja[2], jb[2];
    for (int dir = 0; dir < 2; ++dir) {
      float* h = w.h + (size_t)dir * B * H; float* rh = w.rh + (size_t)dir * B * H; float* u = w.u + (size_t)dir * B * H;
      ja[dir] = sk_base(m, c.gh[dir], h, H, H, nullptr, 0);
      ja[dir].H = H; ja[dir].e0 = h; ja[dir].lde0 = H;
      ja[dir].e1 = w.xproj + dir * 3 * H; ja[dir].lde1 = 6 * H;
      ja[dir].o0 = rh; ja[dir].ldo0 = H; ja[dir].o1 = u; ja[dir].ldo1 = H;
      ja[dir].step = s; ja[dir].T = T; ja[dir].dir = dir;
      jb[dir] = sk_base(m, c.ch[dir], rh, H, H, nullptr, 0);
      jb[dir].H = H; jb[dir].e0 = h; jb[dir].lde0 = H;
      jb[dir].e1 = w.xproj + dir * 3 * H + 2 * H; jb[dir].lde1 = 6 * H; jb[dir].e2 = u; jb[dir].lde2 = H;
      jb[dir].o0 = h; jb[dir].ldo0 = H; jb[dir].o2 = out; jb[dir].ldo2 = 2 * H; jb[dir].seq_coff = dir * H;
      jb[dir].lengths = lengths; jb[dir].step = s; jb[dir].T = T; jb[dir].dir = dir;
    }
    TRY(run_skinny(st, B, ja, 2, EPI_GRU_GATES));
    TRY(run_skinny(st, B, jb, 2, EPI_GRU_CAND));
  }
  return 0;
}

// ---- the point-wise tail of a CBHG as one launch (taco_chain.h) ----
// the widths k_pointwise_chain serves (a term of ff_plan)
static bool chain_fits(const Cbhg& c, int in_dim) {
  const int W = c.rnn;
  if (W != 128 && W != 256) return false;
  if ((int)c.hw.size() != c.depth || c.depth + (c.has_dense ? 2 : 1) > CH_MAXL) return false;
  if (c.has_dense) { if (!c.dense.bh || c.dense.cin != in_dim || c.dense.cin_pad16 > W || c.dense.N != W) return false; }
  else if (in_dim != W) return false;
  for (const ConvL& h : c.hw) if (!h.bh || !h.bh2 || h.cin != W || h.N != W) return false;
  return c.xproj.bh && c.xproj.cin == W && c.xproj.N == 6 * W;
}
// LDS of a chain launch: two plane sets (a layer reads one and writes the other); the entry's planes of proj_1's output (+ 1 frame each side)
// lie behind the first set, over the second, which is first written when they are dead.  W = 256: 67584 + max(67584, 69696) = 137280 bytes
static size_t chain_lds(int W, bool entry) {
  const size_t set = (size_t)2 * CH_BM * (W + 8) * sizeof(unsigned short), ent = (size_t)2 * (CH_BM + 2) * (W + 8) * sizeof(unsigned short);
  return set + std::max(set, entry ? ent : (size_t)0);
}
static int run_chain(const taco_model* m, hipStream_t st, const Cbhg& c, const float* x, int in_dim, int M, int T, const int* lengths,
                     const CbhgWs& w, const ChainEntry* entry = nullptr) {
  ChainArgs a; memset(&a, 0, sizeof a);
  if (entry) a.e = *entry;
  a.x = x; a.ldx = in_dim; a.Cin = in_dim; a.out = w.xproj; a.ldo = 6 * c.rnn; a.rev_len = lengths; a.rev_col0 = 3 * c.rnn;
  a.M = M; a.T = T; a.krot = m->ff_rot;
  auto add = [&](const ConvL& L, int type) {
    const GemmVar& v = m->hvars[L.var_index];
    ChainLayer& l = a.L[a.nlayers++];
    l.bh = v.bh; l.bl = v.bl; l.bh2 = v.bh2; l.bl2 = v.bl2; l.bias = v.bias; l.bias2 = v.bias2;
    l.type = type; l.K16 = v.K16; l.NT = v.NT; l.N = v.N; l.act = ACT_NONE;
  };
  if (c.has_dense) add(c.dense, CH_DENSE);
  for (int i = 0; i < c.depth; ++i) add(c.hw[i], CH_HIGHWAY);
  add(c.xproj, CH_XPROJ);
  const dim3 grid(cdiv(M, CH_BM)), blk(512);
  const size_t lds = chain_lds(c.rnn, entry != nullptr);      // (entry: N1 == rnn, ff_plan)
  if (c.rnn == 256) hipLaunchKernelGGL((k_pointwise_chain<256>), grid, blk, lds, st, a);
  else hipLaunchKernelGGL((k_pointwise_chain<128>), grid, blk, lds, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- conv bank -> max-pool -> proj_1 as one launch (taco_front.h) ----
static int run_front(const taco_model* m, hipStream_t st, const Cbhg& c, const float* x, int B, int T, const CbhgWs& w, bool combine, int* P_out) {
  FrArgs a; memset(&a, 0, sizeof a);
  const int TN = c.front_kind == 1 ? 2 : 1, cinp = c.front_kind == 1 ? 80 : 128, kwmax = c.front_kind == 1 ? 8 : 16;
  const ConvL& P1 = c.proj[0];
  const GemmVar& pv = m->hvars[P1.var_index];
  a.x = x; a.ldx = c.in_dim; a.B = B; a.T = T; a.Cin = c.in_dim; a.tiles_per_b = cdiv(T, FR_BM);
  a.ph = pv.bh; a.pl = pv.bl; a.pNT = pv.NT; a.pK16tap = P1.cin_pad16 / 16;
  a.part = w.bank; a.N1 = P1.N;
  a.delay = m->front_delay;
  a.prio = m->front_prio;
  const int cpw = c.C / FR_CH, nchunks = c.K * cpw, padlmax = (kwmax - 1) / 2;
  for (int i = 0; i < c.K; ++i) {
    const ConvL& L = c.bank[i];
    FrWidth& fw = a.w[i];
    fw.wh = (const unsigned short*)AP(m, c.fr_wh[i]); fw.wl = (const unsigned short*)AP(m, c.fr_wl[i]);
    fw.bias = AP(m, L.bias); fw.scale = AP(m, L.bns); fw.shift = AP(m, L.bnb);
    fw.kw = L.kw; fw.xoff = padlmax - (L.kw - 1) / 2; fw.ns = c.fr_ns[i]; fw.nct = c.C / 16;
  }
  // parts: as many as fill the chip (the makespan is rounds of workgroups x the work of one part), at most what the partial-sum
  // slabs (kept in the bank buffer) and the chunk count allow; chunks go to the least loaded part, heaviest first
  const int ntiles = B * a.tiles_per_b, ncu = m->cu_count > 0 ? m->cu_count : 256;
  const int pmax = std::max(1, std::min(std::min(nchunks, FR_MAXP), (c.K * c.C) / P1.N));
  int P = 1; double best = 1e30;
  for (int p = 1; p <= pmax; ++p) {
    const double cost = (double)cdiv(ntiles * p, ncu) * ((double)cdiv(nchunks, p) / nchunks + 0.03);
    if (cost < best - 1e-9) { best = cost; P = p; }
  }
  a.P = P;
  { std::vector<std::pair<long, int>> order;        // (cost, chunk id = width index * cpw + sub-chunk)
    for (int i = 0; i < c.K; ++i)
      for (int j = 0; j < cpw; ++j) order.push_back({432L * c.fr_ns[i] + 4608L * TN, i * cpw + j});
    std::stable_sort(order.begin(), order.end(), [](const std::pair<long, int>& u, const std::pair<long, int>& v) { return u.first > v.first; });
    std::vector<long> load(P, 0); std::vector<std::vector<int>> mine(P);
    for (auto& o : order) {
      int tgt = 0;
      for (int p = 1; p < P; ++p) if (load[p] < load[tgt]) tgt = p;
      load[tgt] += o.first; mine[tgt].push_back(o.second);
    }
    int n = 0;
    for (int p = 0; p < P; ++p) {
      a.pstart[p] = n;
      std::sort(mine[p].begin(), mine[p].end());
      for (int id : mine[p]) {
        const int i = id / cpw, j = id % cpw;
        a.ch[n].wi = i; a.ch[n].ct0 = j * (FR_CH / 16); a.ch[n].cg0 = (c.bank[i].kw - 1) * c.C + j * FR_CH; ++n;
      }
    }
    a.pstart[P] = n; }
  const int xs = c.front_kind == 1 ? 80 : 144, xrows = c.front_kind == 1 ? 16 * FR_NRT + kwmax : FR_PR + kwmax;
  (void)cinp;
  if ((size_t)2 * xrows * xs * 2 + (size_t)2 * FR_PR * FR_ALD * 2 > FR_SMEM_CNT || (size_t)8 * 2 * TN * 16 * 64 * sizeof(float) > FR_SMEM_CNT)
    return fail(TACO_ERR_STATE, "k_cbhg_front: LDS layout does not fit");
  const size_t lds = 160 * 1024;           // planes + reduction scratch below FR_SMEM_CNT, the two group-barrier counters at it
  const dim3 grid(ntiles * P), blk(512);
  if (c.front_kind == 1) hipLaunchKernelGGL((k_cbhg_front<2, 80, 80, 8>), grid, blk, lds, st, a);      // (> 64 KB of LDS: attribute set at finalize)
  else hipLaunchKernelGGL((k_cbhg_front<1, 144, 128, 16>), grid, blk, lds, st, a);
  HIPCHK(hipGetLastError());
  if (P_out) *P_out = P;
  if (!combine) return 0;                  // the chain kernel's fused entry sums the parts itself (taco_chain.h)
  const size_t MN = (size_t)B * T * P1.N;
  hipLaunchKernelGGL(k_front_combine, dim3((unsigned)cdiv((int)(MN / 4), 256)), dim3(256), 0, st, (const float*)w.bank, P, MN, P1.N,
                     AP(m, P1.bias), AP(m, P1.bns), AP(m, P1.bnb), c.proj.size() > 1 ? 1 : 0, w.p[0]);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- which kernels run the feed-forward part of a CBHG ----
struct FfPlan {
  GemmLevel level;          // of the layers that stay launches of their own (k_gemm / k_gemm_bf3, one per layer; the conv bank is one)
  int front_kind;           // k_cbhg_front: conv bank -> max-pool -> proj_1 as one launch, this instantiation (Cbhg::front_kind); 0: two GEMM launches
  bool entry;               // the sum of the front's parts, proj_1's epilogue and proj_2 (+ residual) inside the chain's entry: front + chain = 2 launches
  int chain_w;              // k_pointwise_chain<chain_w>: dense, highways and the hoisted GRU projection as one launch; 0: one launch per layer
  int launches;
  FfWhyNot why_front, why_entry, why_chain;      // first reason against each (NONE: used)
};
// The one place that decides.  Pure: launches nothing.
static FfPlan ff_plan(const taco_model* m, const Cbhg& c) {
  const ConvL& P1 = c.proj[0]; const ConvL& P2 = c.proj.back();
  FfPlan p; memset(&p, 0, sizeof p);
  p.level = gemm_level(m, P1);
  p.why_front = ff_fused_why(m, P1);
  if (!p.why_front) p.why_front = !m->front ? FF_WHY_SWITCH : c.front_kind != 0 && P1.cin == c.K * c.C && P1.cin_pad16 == c.K * c.C ? FF_WHY_NONE : FF_WHY_WIDTHS;
  p.why_chain = ff_fused_why(m, c.xproj);
  if (!p.why_chain) p.why_chain = !m->chain ? FF_WHY_SWITCH : chain_fits(c, P2.N) ? FF_WHY_NONE : FF_WHY_WIDTHS;
  p.why_entry = p.why_front || p.why_chain ? FF_WHY_NEEDS_BOTH : !m->front_entry ? FF_WHY_SWITCH :
                c.proj.size() == 2 && P2.bh && P2.kw == 3 && P2.cin == P1.N && P2.cin_pad16 == P1.N && P1.N == c.rnn && P2.N <= c.rnn && c.in_dim == P2.N
                    ? FF_WHY_NONE : FF_WHY_WIDTHS;     // (k16 steps of proj_2: 3 rnn / 16 = a multiple of the entry's block pairs)
  p.front_kind = p.why_front ? 0 : c.front_kind; p.entry = !p.why_entry; p.chain_w = p.why_chain ? 0 : c.rnn;
  // front (+ k_front_combine) or bank + proj_1; the other projections; the tail
  p.launches = (p.entry ? 1 : 2) + ((int)c.proj.size() - (p.entry ? 2 : 1)) + (p.chain_w ? 1 : (c.has_dense ? 1 : 0) + c.depth + 1);
  return p;
}
// Feed-forward part of a CBHG (modules.py:27-77), by ff_plan: x [B*T, in_dim] -> the hoisted BiGRU input projection in w.xproj
static int cbhg_ff(const taco_model* m, hipStream_t st, const Cbhg& c, const float* x, int B, int T,
                   const int* lengths, const float* before_highway, const CbhgWs& w) {
  const int M = B * T;
  const FfPlan fp = ff_plan(m, c);
  // bank -> max-pool -> proj_1 as ONE launch, the bank tensor never leaves the CU (taco_front.h); with the entry, proj_1's epilogue and
  // proj_2 (+ residual) move into the point-wise chain: front + chain = the whole feed-forward part in two launches
  int parts = 1;
  if (fp.front_kind) TRY(run_front(m, st, c, x, B, T, w, !fp.entry, &parts));
  else {  // conv bank: all K widths in one launch, written channel-concatenated (modules.py:35-44)
    GemmCall g; g.x = x; g.ldx = c.in_dim; g.M = M; g.T = T; g.act = ACT_RELU; g.out = w.bank; g.ldo = c.K * c.C;
    // (c.bank is ordered widest first, so the longest workgroups are dispatched first; narrowest first measured 0.47 vs 0.445 ms
    // for the encoder stage)
    TRY(run_gemm(m, st, c.bank.data(), c.K, false, g));
  }
  // maxpool (fused into the staging of proj_1) + projections (modules.py:47-59); the front has run proj_1, and the chain's entry runs proj_2
  const size_t absorbed = fp.front_kind ? (fp.entry ? 2 : 1) : 0;
  const float* cur = w.bank; int curd = c.K * c.C;
  for (size_t i = 0; i < c.proj.size(); ++i) {
    if (i >= absorbed) {
      GemmCall p;
      p.x = cur; p.ldx = curd; p.M = M; p.T = T; p.mpw = (i == 0) ? c.maxpool : 1;
      p.act = (i + 1 == c.proj.size()) ? ACT_NONE : ACT_RELU;
      p.out = w.p[i]; p.ldo = c.proj[i].N;
      if (i + 1 == c.proj.size()) {  // residual (modules.py:62-69)
        p.res = x; p.ldres = c.in_dim;
        p.rowvec = before_highway; p.ldrv = c.in_dim;
      }
      TRY(run_gemm(m, st, &c.proj[i], 1, false, p));
    }
    cur = w.p[i]; curd = c.proj[i].N;
  }
  // point-wise chain: optional dense (modules.py:72-73), highway x depth (:76-77), hoisted BiGRU input projection
  if (fp.chain_w) {
    // the whole tail as ONE launch, activations resident on the CU from layer to layer (taco_chain.h)
    ChainEntry E; memset(&E, 0, sizeof E);
    if (fp.entry) {
      const ConvL& P1 = c.proj[0]; const ConvL& P2 = c.proj[1];
      const GemmVar& v2 = m->hvars[P2.var_index];
      E.part = w.bank; E.P = parts; E.MN = (size_t)M * P1.N; E.N1 = P1.N;
      E.b1 = AP(m, P1.bias); E.s1 = AP(m, P1.bns); E.h1 = AP(m, P1.bnb); E.relu1 = 1;
      E.bh = v2.bh; E.bl = v2.bl; E.NT2 = v2.NT; E.K16tap = P2.cin_pad16 / 16; E.N2 = P2.N;
      E.b2 = AP(m, P2.bias); E.s2 = AP(m, P2.bns); E.h2 = AP(m, P2.bnb);
      E.res = x; E.ldres = c.in_dim; E.rowvec = before_highway; E.ldrv = c.in_dim;
    }
    return run_chain(m, st, c, cur, curd, M, T, lengths, w, fp.entry ? &E : nullptr);
  }
  if (c.has_dense) {
    // (tiles_only: at 256 or 512 inputs and 512 outputs and more this layer has the linear head's shape, and it stays on the tile kernel
    // that ff_plan's launch count and engine_plan's sentence name)
    GemmCall d; d.x = cur; d.ldx = curd; d.M = M; d.T = T; d.out = w.hi0; d.ldo = c.rnn; d.tiles_only = true;
    TRY(run_gemm(m, st, &c.dense, 1, false, d));
    cur = w.hi0;
  }
  float* bufs[2] = {w.hi0, w.hi1};
  int sel = (cur == w.hi0) ? 1 : 0;
  for (int i = 0; i < c.depth; ++i) {
    GemmCall h; h.x = cur; h.ldx = c.rnn; h.M = M; h.T = T; h.out = bufs[sel]; h.ldo = c.rnn;
    TRY(run_gemm(m, st, &c.hw[i], 1, true, h));
    cur = bufs[sel]; sel ^= 1;
  }
  // backward-direction columns are stored time-reversed per row (reverse_sequence), so scan step s reads row s
  GemmCall xp; xp.x = cur; xp.ldx = c.rnn; xp.M = M; xp.T = T; xp.out = w.xproj; xp.ldo = 6 * c.rnn;
  xp.rev_len = lengths; xp.rev_col0 = 3 * c.rnn;
  return run_gemm(m, st, &c.xproj, 1, false, xp);
}

// modules.py:27-96.  x [B*T, in_dim], out [B*T, 2*rnn].
static int cbhg_forward(const taco_model* m, hipStream_t st, const Cbhg& c, const float* x, int B, int T,
                        const int* lengths, const float* before_highway, const float* init_state, float* out,
                        const CbhgWs& w) {
  TRY(cbhg_ff(m, st, c, x, B, T, lengths, before_highway, w));
  return bigru_scan(m, st, c, B, T, lengths, init_state, out, w);
}

// ---- speaker conditioning (tacotron.py:41-94) ----
struct SpkWs { float *emb, *vec[8]; };
static void carve_spk(Carver& cv, const taco_model* m, int B, SpkWs& w) {
  const taco_hparams& hp = m->hp;
  w.emb = cv.f((size_t)B * std::max(hp.speaker_embedding_size, 1));
  const int dims[3] = {hp.enc_prenet[hp.enc_prenet_n - 1], hp.enc_rnn_size * 2, hp.attention_state_size};
  for (int i = 0; i < 3 + hp.dec_layer_num; ++i) w.vec[i] = cv.f((size_t)B * (i < 3 ? dims[i] : hp.dec_rnn_size));
}
static size_t spk_weights_offset(int b0, int num_speakers) { return (size_t)b0 * (size_t)num_speakers; }      // where row b0 of [B, num_speakers] starts
// Which speaker each batch row speaks with: one trained speaker by id [B], or a mixture of all of them by weights [B, num_speakers]
// (taco_abi.h, "speaker mixtures") -- never both.  Device pointers, read by kernels only.
struct SpkSel {
  const int* id = nullptr;
  const float* w = nullptr;
  bool given() const { return id || w; }
  SpkSel rows_from(int b0, int num_speakers) const { SpkSel s; s.id = id ? id + b0 : nullptr; s.w = w ? w + spk_weights_offset(b0, num_speakers) : nullptr; return s; }
};
static SpkSel spk_ids(const int* id) { SpkSel s; s.id = id; return s; }
static SpkSel spk_mix(const float* w) { SpkSel s; s.w = w; return s; }
// a _mix entry point's selector: weights are required exactly where the model has speakers to mix
static int spk_mix_check(const taco_model* m, const float* w) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  if (m->hp.num_speakers > 1 && !w) return fail(TACO_ERR_ARG, "speaker_weights required for a multi-speaker model");
  if (m->hp.num_speakers <= 1 && w) return fail(TACO_ERR_ARG, "speaker_weights given to a single-speaker model");
  return 0;
}
// out[b, :] = the speaker row of batch row b out of table [num_speakers, D]: looked up by id, or mixed by weights
static int spk_rows(const taco_model* m, hipStream_t st, const SpkSel& sel, const float* table, int B, int D, float* out) {
  if (sel.w) hipLaunchKernelGGL(k_mix_rows, dim3(cdiv(B * D, 256)), dim3(256), 0, st, table, sel.w, B, m->hp.num_speakers, D, out);
  else hipLaunchKernelGGL(k_gather_rows, dim3(cdiv(B * D, 256)), dim3(256), 0, st, table, sel.id, B, D, out);
  HIPCHK(hipGetLastError());
  return 0;
}
// computes vec[0..2+L) = before_highway, encoder_rnn_init, attention_rnn_init, decoder_rnn_init_i
static int spk_forward(const taco_model* m, hipStream_t st, const SpkSel& sel, int B, const SpkWs& w) {
  const taco_hparams& hp = m->hp;
  const int nv = 3 + hp.dec_layer_num;
  const int dims[3] = {hp.enc_prenet[hp.enc_prenet_n - 1], hp.enc_rnn_size * 2, hp.attention_state_size};
  if (hp.speaker_embedding_size == 1) {
    for (int i = 0; i < nv; ++i) {
      const int D = i < 3 ? dims[i] : hp.dec_rnn_size;
      TRY(spk_rows(m, st, sel, AP(m, m->spk_table[i]), B, D, w.vec[i]));
    }
    return 0;
  }
  const int S = hp.speaker_embedding_size;
  TRY(spk_rows(m, st, sel, AP(m, m->spk_emb), B, S, w.emb));
  for (int i0 = 0; i0 < nv; i0 += SK_MAXJOBS) {
    SkJob js[SK_MAXJOBS];
    const int nj = std::min(SK_MAXJOBS, nv - i0);
    for (int i = 0; i < nj; ++i) {
      const int D = (i0 + i) < 3 ? dims[i0 + i] : hp.dec_rnn_size;
      js[i] = sk_linear(m, m->spk_dense[i0 + i], w.emb, S, S, nullptr, 0, ACT_SOFTSIGN, w.vec[i0 + i], D);
    }
    TRY(run_skinny(st, B, js, nj));
  }
  return 0;
}

// ---- encoder (tacotron.py:34-112) ----
struct EncWs { float* pre[4]; CbhgWs cb; SpkWs spk; };
static void carve_enc(Carver& cv, const taco_model* m, int B, int T, EncWs& w) {
  for (int i = 0; i < m->hp.enc_prenet_n; ++i) w.pre[i] = cv.f((size_t)B * T * m->hp.enc_prenet[i]);
  carve_cbhg(cv, m->enc, B, T, w.cb);
  carve_spk(cv, m, B, w.spk);
}
// The encoder prenet (modules.py:18-25: two dense + ReLU layers over the looked-up embeddings) as ONE launch of the point-wise chain kernel
// (taco_chain.h): gathered rows -> planes, a 256-wide ReLU layer, and the second layer as the chain's last link (stored straight to the
// prenet output).  Two k_gemm_bf3 launches of 11 us each at C2 otherwise -- a 64-row tile of 4096 rows leaves them latency-bound.
// NONE: that launch; else one GEMM launch per layer.  One answer per forward: the caller asks once and hands it to encoder_forward.
static FfWhyNot prenet_chain_why(const taco_model* m) {
  const taco_hparams& hp = m->hp;
  if (const FfWhyNot why = ff_fused_why(m, m->enc_prenet[0])) return why;
  if (!m->chain) return FF_WHY_SWITCH;
  if (hp.enc_prenet_n != 2) return FF_WHY_WIDTHS;
  const ConvL& a = m->enc_prenet[0]; const ConvL& b = m->enc_prenet[1];
  return b.bh && a.kw == 1 && b.kw == 1 && a.N == 256 && a.cin == hp.embedding_size && a.cin_pad16 <= 256 && (hp.embedding_size & 3) == 0 &&
         b.cin == 256 && b.N == hp.enc_prenet[1] && a.var_index >= 0 && b.var_index >= 0 ? FF_WHY_NONE : FF_WHY_WIDTHS;
}
// riders (nullable): its regions are cleared by the launch's spare workgroups -- the words the persistent kernels of the same forward poll (forward_pass)
static int run_prenet_chain(const taco_model* m, hipStream_t st, const int* ids, int M, float* out, UpFrontClear* riders) {
  const taco_hparams& hp = m->hp;
  ChainArgs a; memset(&a, 0, sizeof a);
  a.x = AP(m, m->emb); a.ldx = hp.embedding_size; a.Cin = hp.embedding_size; a.gather = ids;
  a.out = out; a.ldo = hp.enc_prenet[1]; a.rev_len = nullptr; a.rev_col0 = -1; a.M = M; a.T = M; a.krot = m->ff_rot;
  const int types[2] = {CH_DENSE, CH_XPROJ};
  for (int i = 0; i < 2; ++i) {
    const GemmVar& v = m->hvars[m->enc_prenet[i].var_index];
    ChainLayer& l = a.L[a.nlayers++];
    l.bh = v.bh; l.bl = v.bl; l.bh2 = v.bh2; l.bl2 = v.bl2; l.bias = v.bias; l.bias2 = v.bias2;
    l.type = types[i]; l.K16 = v.K16; l.NT = v.NT; l.N = v.N; l.act = ACT_RELU;
  }
  int nwg = cdiv(M, CH_BM);
  if (riders) {
    a.ntiles = nwg;
    for (int i = 0; i < CH_RIDERS; ++i) { a.zp[i] = riders->z.p[i]; a.znw[i] = riders->z.nw[i]; }
    nwg += std::min(192, std::max(16, 256 - nwg));
  }
  hipLaunchKernelGGL((k_pointwise_chain<256>), dim3(nwg), dim3(512), chain_lds(256, false), st, a);
  HIPCHK(hipGetLastError());
  if (riders) riders->enqueued = true;      // the riders are in the stream now: the persistent kernels behind this launch need no fill of their own
  return 0;
}
// prenet_chain: prenet_chain_why(m) == NONE, asked once by the caller; riders: see run_prenet_chain -- they travel in that launch only (the caller
// clears the regions itself otherwise)
static int encoder_forward(const taco_model* m, hipStream_t st, const int* ids, const int* lengths, const SpkSel& sel,
                           int B, int T, float* enc_out, const EncWs& w, bool spk_done, bool prenet_chain, UpFrontClear* riders = nullptr) {
  const taco_hparams& hp = m->hp;
  const int M = B * T;
  if (is_deepvoice(m) && !spk_done) TRY(spk_forward(m, st, sel, B, w.spk));
  const float* cur = AP(m, m->emb); int curd = hp.embedding_size;
  if (prenet_chain) {
    TRY(run_prenet_chain(m, st, ids, M, w.pre[1], riders));
    cur = w.pre[1];
  } else for (int i = 0; i < hp.enc_prenet_n; ++i) {  // embedding_lookup fused as a row gather (tacotron.py:38-39)
    GemmCall g; g.x = cur; g.ldx = curd; g.gather = (i == 0) ? ids : nullptr; g.M = M; g.act = ACT_RELU;
    g.out = w.pre[i]; g.ldo = hp.enc_prenet[i];
    TRY(run_gemm(m, st, &m->enc_prenet[i], 1, false, g));
    cur = w.pre[i]; curd = hp.enc_prenet[i];
  }
  return cbhg_forward(m, st, m->enc, cur, B, T, lengths, is_deepvoice(m) ? w.spk.vec[0] : nullptr,
                      is_deepvoice(m) ? w.spk.vec[1] : nullptr, enc_out, w.cb);
}

// ---- decoder (tacotron.py:120-214) ----
struct DecWs {
  float *keys, *zero, *ctx, *pz[4], *h_att, *rh, *u, *xc, *q, *align, *o[5], *hd[4], *Y, *escr;
  Polled nz;                                                      // the rows' stop flags [n, B] (int): polled by the persistent decoder, read by k_stop_step
  int* nzp() const { return static_cast<int*>(nz.p); }
  Xchg dx;                                                        // persistent decoder: exchange granules, census words
  float* rowbias;                                                 // persistent decoder, 'simple': [B, DXRB_N, 256]
  SpkWs spk;
};
static void carve_dec(Carver& cv, const taco_model* m, int B, int T_in, int n, DecWs& w) {
  const taco_hparams& hp = m->hp;
  const int D = 2 * hp.enc_rnn_size, As = hp.attention_state_size, Hd = hp.dec_rnn_size;
  const int Hmax = std::max(As, Hd);
  w.keys = cv.f((size_t)B * T_in * hp.attention_size);
  w.zero = cv.f((size_t)B * hp.num_mels);
  const int S = simple_S(m);     // 'simple': the speaker embedding rides in the last S columns of ctx and of the prenet output
  // [h_att | ctx (| spk)] share one row (stride As + D + S): the concat projection's input is then ONE contiguous segment
  w.h_att = cv.f((size_t)B * (As + D + S)); w.ctx = w.h_att ? w.h_att + As : nullptr;
  for (int i = 0; i < hp.dec_prenet_n; ++i) w.pz[i] = cv.f((size_t)B * (hp.dec_prenet[i] + S));
  w.rh = cv.f((size_t)B * Hmax); w.u = cv.f((size_t)B * Hmax); w.xc = cv.f((size_t)B * 2 * Hmax);
  w.q = cv.f((size_t)B * hp.attention_size);
  w.align = cv.f((size_t)B * T_in);
  w.escr = cv.f((size_t)B * T_in);
  for (int i = 0; i <= hp.dec_layer_num; ++i) w.o[i] = cv.f((size_t)B * Hd);
  for (int i = 0; i < hp.dec_layer_num; ++i) w.hd[i] = cv.f((size_t)B * Hd);
  w.Y = nullptr;
  w.nz.bytes = (size_t)n * B * sizeof(int); w.nz.p = cv.raw(w.nz.bytes);
  carve_spk(cv, m, B, w.spk);
  {  // persistent decoder (taco_decoder_xcd.h): sized for the largest rows-per-group, so a debug override cannot outgrow it
    w.dx.carve(cv, (size_t)DX_NGROUP * dx_xlayout(8, T_in).total);
    w.rowbias = cv.f(is_simple(m) ? (size_t)B * DXRB_N * DX_W : 1);
  }
}
// ---- which engine runs the decoder loop ----
static constexpr size_t DX_LDS_BUDGET = 160 * 1024;      // dynamic LDS a member of k_decoder_xcd / k_decoder_bwd_xcd may request
enum DecUse { DEC_INFER, DEC_TEACHER, DEC_TRAIN_FWD, DEC_TRAIN_BWD };      // TEACHER: taco_decoder_forward with teacher frames; TRAIN_*: taco_train.h
enum DecWhyNot { DEC_WHY_NONE, DEC_WHY_ENGINE_OFF, DEC_WHY_CUS, DEC_WHY_ROWS, DEC_WHY_WIDTHS, DEC_WHY_TEACHER_ROWS, DEC_WHY_NO_INSTANTIATION, DEC_WHY_LDS, DEC_WHY_TAPE_LAYOUT };
static_assert((int)DEC_WHY_ENGINE_OFF == SCAN_WHY_ENGINE_OFF && (int)DEC_WHY_CUS == SCAN_WHY_CUS && (int)DEC_WHY_ROWS == SCAN_WHY_ROWS, "taco_model_engine_plan words the shared reasons once");
struct DecPlan {
  bool persistent;          // the whole loop as ONE launch: k_decoder_xcd (DEC_TRAIN_BWD: k_decoder_bwd_xcd); else one launch per stage
  int rg, aw, pd;           // the instantiation: rows per group of 32 CUs, attention_size, prenet layers
  bool tape;                // the TAPE instantiation: the training forward, or teacher frames on an inference model (manual alignments: a launch argument)
  size_t lds_bytes;         // what the launch requests
  DecWhyNot why;            // first reason against the persistent kernel (NONE: it runs)
};
// The one place that decides.  Pure: launches nothing, touches no device state.  n: decoder steps (the training tape's extent; unused otherwise)
static DecPlan decoder_plan(const taco_model* m, int B, int T_in, int n, DecUse use) {
  const taco_hparams& hp = m->hp;
  const bool bwd = use == DEC_TRAIN_BWD, train = bwd || use == DEC_TRAIN_FWD;
  DecPlan p = {false, 0, hp.attention_size, dx_prenet_depth(m), use != DEC_INFER, 0, DEC_WHY_NONE};
  // rows per group: the smallest of 1 / 2 / 4 / 8 that covers the batch with 8 groups.  The other presets (attention_size 128 / 512, three prenet layers) are instantiated
  // for 4 and 8 only: smaller batches run as padded groups of 4 (a step costs the same there: its time is the chain of exchanges, not the rows)
  const int lo = dx_reference_widths(m) ? 1 : 4;
  for (p.rg = lo; p.rg < 8 && p.rg * DX_NGROUP < B; p.rg *= 2) {}
  if (m->dx_rows >= lo && m->dx_rows * DX_NGROUP >= B) p.rg = m->dx_rows;      // taco_debug_set_decoder_persist: an override that does not fit this call is ignored
  p.lds_bytes = (bwd ? db_lds_floats(p.rg, T_in) : dx_lds_floats(p.rg, T_in, p.tape, p.aw)) * sizeof(float);
  if (!m->dx_mode) p.why = DEC_WHY_ENGINE_OFF;
  else if (m->cu_count < CHIP_CUS) p.why = DEC_WHY_CUS;
  else if (B > CHIP_ROWS) p.why = DEC_WHY_ROWS;
  else if (!(bwd ? m->dbx_pack : m->dx_pack)) p.why = DEC_WHY_WIDTHS;      // the packs exist where dx_widths_ok(m) (taco_model_finalize; dbx_pack: training shadow model)
  // teacher frames need the raw prenet rows where inference keeps the frame-projection composite: the shadow model's pack has them, an inference model beside its pack (dx_build_pack)
  else if (use == DEC_TEACHER && !m->tp && !(m->dx_p1o_raw && hp.num_mels <= DX_P2)) p.why = DEC_WHY_TEACHER_ROWS;
  else if (p.aw == 512 && p.rg > 4) p.why = DEC_WHY_NO_INSTANTIATION;      // 128 score channels per member: query registers, the q / v slots
  else if (p.lds_bytes > DX_LDS_BUDGET) p.why = DEC_WHY_LDS;
  // the tape (carve_dec_tape): the step's own frame in a 128-wide slot (forward only), 32-bit element offsets over the DXT_N slots of [B, n, 256]
  else if (train && ((!bwd && hp.num_mels > DX_P2) || (size_t)DXT_N * B * n * DX_W >= (1u << 31))) p.why = DEC_WHY_TAPE_LAYOUT;
  p.persistent = p.why == DEC_WHY_NONE;
  return p;
}
template <int RG, bool TAPE, int AW = DX_W, int PD = 2>
static int dx_launch_rg(hipStream_t st, const DxArgs& a_in, size_t lds) {
  DxArgs a = a_in;
  if constexpr (!TAPE && AW == DX_W && PD == 2) {      // the stamped instantiation (tools/time_decoder.py): the plain decoder at the reference widths only
    if (a.trace && !a.manual) { hipLaunchKernelGGL((k_decoder_xcd<RG, false, false, AW, PD, true>), dim3(CHIP_CUS), dim3(DX_NT), lds, st, a); HIPCHK(hipGetLastError()); return 0; }
  }
  a.trace = nullptr;
  // manual alignments: their own instantiation (the score phases are compiled out); with teacher frames as well (round 6: teacher-forced decoding under
  // manual alignments on an inference model -- taco_decoder_forward with both -- used to fall to the launch-per-stage loop)
  if (a.manual) { hipLaunchKernelGGL((k_decoder_xcd<RG, TAPE, true, AW, PD>), dim3(CHIP_CUS), dim3(DX_NT), lds, st, a); HIPCHK(hipGetLastError()); return 0; }
  hipLaunchKernelGGL((k_decoder_xcd<RG, TAPE, false, AW, PD>), dim3(CHIP_CUS), dim3(DX_NT), lds, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}
// Every (rows per group, TAPE, attention_size, prenet layers) k_decoder_xcd is instantiated for, each with and without manual alignments: the reference
// widths plain (these also stamped, tools/time_decoder.py) and TAPE (teacher frames; the training forward), and the presets of hparams.py:71-117 that the reference
// ships switched off -- "Single Speaker", "Single Speaker with generalization", the first "Deep Voice 2" block, and the two remaining combinations
#define DX_REFERENCE(X) X(1, false, DX_W, 2) X(2, false, DX_W, 2) X(4, false, DX_W, 2) X(8, false, DX_W, 2)
#define DX_REFERENCE_TAPE(X) X(1, true, DX_W, 2) X(2, true, DX_W, 2) X(4, true, DX_W, 2) X(8, true, DX_W, 2)
#define DX_PRESETS(X) X(4, false, 128, 2) X(8, false, 128, 2) X(4, false, 256, 3) X(8, false, 256, 3) X(4, false, 512, 3) X(4, false, 128, 3) X(8, false, 128, 3) X(4, false, 512, 2)
static constexpr int dx_inst(int rg, bool tape, int aw, int pd) { return rg | (tape ? 16 : 0) | pd << 8 | aw << 12; }
// dp: decoder_plan's, persistent; `tape`: null, or where dp.tape the TAPE instantiation's extra arguments already filled in (teacher, tape pointers)
// 'simple': the speaker rows are ready_rows [B, S] if given (training), else sel's -- ids looked up by k_dx_rowbias itself, weights mixed into mix_rows [B, S] first
static int dx_launch(const taco_model* m, hipStream_t st, const DecPlan& dp, const float* enc_out, const SpkSel& sel, const float* ready_rows, float* mix_rows, int B, int T_in, int n,
                     const float* manual, float* mel, float* align_out, float* dbg, int dbgw, const float* keys, int* nz,
                     const Xchg& dx, float* rowbias, const float* h_att0, const float* h10, const float* h20,
                     const DxArgs* tape = nullptr) {
  ChipTurn turn(m->device, st);
#ifdef DX_DLY_RT
  {   // A/B build: the eleven first-poll sleeps (units of 64 clocks) from TACO_DX_DLY = "a,b,c,..." (sites 0..10 of taco_decoder_xcd.h); eager launches only
    int d[32];
    for (int i = 0; i < 32; ++i) d[i] = (i & 15) < 11 ? dx_site_delay(i & 15, dp.rg) : 0;
    if (const char* e = getenv("TACO_DX_DLY")) { int i = 0; const char* p = e; while (*p && i < 11) { d[i] = d[16 + i] = atoi(p); ++i; while (*p && *p != ',') ++p; if (*p == ',') ++p; } }
    if (const char* e = getenv("TACO_DX_DLY_B")) { int i = 0; const char* p = e; while (*p && i < 11) { d[16 + i] = atoi(p); ++i; while (*p && *p != ',') ++p; if (*p == ',') ++p; } }      // waves 4-7
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_dx_dly), d, sizeof d));
  }
#endif
  DxArgs a; memset(&a, 0, sizeof a);
  if (tape) a = *tape;
  a.manual = manual;
  if (is_simple(m)) {   // the speaker embedding's share of the attention GRU and GRU 1 pre-activations, once per launch
    if (!ready_rows && sel.w) { TRY(spk_rows(m, st, sel, AP(m, m->spk_emb), B, m->hp.speaker_embedding_size, mix_rows)); ready_rows = mix_rows; }
    hipLaunchKernelGGL(k_dx_rowbias, dim3(B), dim3(DX_W), 0, st, ready_rows ? ready_rows : AP(m, m->spk_emb), ready_rows ? (const int*)nullptr : sel.id,
                       AP(m, m->dx_spkw), m->hp.speaker_embedding_size, rowbias);
    HIPCHK(hipGetLastError());
    a.rowbias = rowbias;
  }
  a.wpack = AP(m, m->dx_pack);
  a.qpack = AP(m, m->dx_qpack[dp.rg == 1 ? 0 : dp.rg == 2 ? 1 : dp.rg == 4 ? 2 : 3]);
  a.b_p1_0 = AP(m, m->dx_b_p1_0); a.b_p1c = AP(m, m->dx_b_p1c); a.b_p2 = AP(m, m->dx_b_p2); a.b_p3 = AP(m, m->dx_b_p3); a.b_ag = AP(m, m->dx_b_ag); a.b_ac = AP(m, m->dx_b_ac);
  a.b_g1f = AP(m, m->dx_b_g1f); a.b_g1c = AP(m, m->dx_b_g1c); a.b_g2g = AP(m, m->dx_b_g2g); a.b_g2c = AP(m, m->dx_b_g2c);
  a.b_f = AP(m, m->dx_b_f);
  a.att_v = AP(m, m->att_v); a.att_b = AP(m, m->att_b); a.score_bias = AP(m, m->att_sb);
  a.keys = keys; a.values = enc_out; a.h_att0 = h_att0; a.h10 = h10; a.h20 = h20;
  a.mel = mel; a.hist = align_out; a.nz = nz; a.dbg = dbg; a.dbgw = dbgw;
  a.xbuf = dx.buf(); a.ctl = dx.ctl(); a.err = m->d_err; a.trace = m->trace_on ? m->d_trace : nullptr;
  if (a.trace) { const char* e = getenv("TACO_TRACE_MEMBER"); a.trc_member = e ? atoi(e) : 0; e = getenv("TACO_TRACE_TID"); a.trc_tid = e ? atoi(e) : 0; }
  a.B = B; a.T_in = T_in; a.n = n; a.rM = m->hp.num_mels * m->hp.reduction_factor; a.att_type = m->hp.attention_type;
  a.mels = m->hp.num_mels;
  a.grp0 = 0; a.ngroups = cdiv(B, dp.rg); a.force_wt = m->dx_mode == 2 ? 1 : 0;
  // every polled word starts from zero on every launch (tags are step numbers, the census counts arrivals)
  HIPCHK(dx.clear(st));
  switch (dx_inst(dp.rg, dp.tape, dp.aw, dp.pd)) {
#define X(RG, TAPE, AW, PD) case dx_inst(RG, TAPE, AW, PD): return dx_launch_rg<RG, TAPE, AW, PD>(st, a, dp.lds_bytes);
    DX_REFERENCE(X) DX_REFERENCE_TAPE(X) DX_PRESETS(X)
#undef X
    default: return fail(TACO_ERR_STATE, "no persistent decoder instantiation for attention_size %d, %d prenet layers, %d rows per group%s", dp.aw, dp.pd, dp.rg, dp.tape ? ", tape" : "");
  }
}
// persistent BPTT (taco_decoder_bwd_xcd.h); dp: decoder_plan(..., DEC_TRAIN_BWD), persistent
static size_t dbx_xbuf_granules(int T_in) {
  size_t g = 0;
  for (int RG = 1; RG <= 8; RG *= 2) g = std::max(g, (size_t)db_xlayout(RG, T_in).total);
  return g;
}
static int dbx_launch(const taco_model* m, hipStream_t st, const DecPlan& dp, DbArgs a, int B, int T_in, int n, const Xchg& dx) {
  ChipTurn turn(m->device, st);
#ifdef DX_DLY_RT
  {   // A/B build: the twelve first-poll sleeps of the backward loop from TACO_DB_DLY (sites 0..11 of taco_decoder_bwd_xcd.h)
    int d[16];
    for (int i = 0; i < 16; ++i) d[i] = i < 12 ? db_site_delay(i) : 0;
    if (const char* e = getenv("TACO_DB_DLY")) { int i = 0; const char* p = e; while (*p && i < 12) { d[i++] = atoi(p); while (*p && *p != ',') ++p; if (*p == ',') ++p; } }
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_db_dly), d, sizeof d));
  }
#endif
  a.wpack = AP(m, m->dbx_pack);
  a.att_v = AP(m, m->att_v); a.att_b = AP(m, m->att_b); a.score_bias = AP(m, m->att_sb);
  a.xbuf = dx.buf(); a.ctl = dx.ctl(); a.err = m->d_err; a.trace = (m->trace_on && m->d_trace) ? m->d_trace + 2 * DX_TRACE_STEPS * DX_TRACE_SLOTS : nullptr;
  a.B = B; a.T_in = T_in; a.n = n; a.att_type = m->hp.attention_type;
  a.force_wt = m->dx_mode == 2 ? 1 : 0;
  HIPCHK(dx.clear(st));
  const dim3 grid(CHIP_CUS), blk(DX_NT);
  if (a.trace && dp.rg == 4) {      // the stamped instantiation (tools/trace_bptt.py): the C4 shard's geometry only
    hipLaunchKernelGGL((k_decoder_bwd_xcd<4, true>), grid, blk, dp.lds_bytes, st, a);
    HIPCHK(hipGetLastError());
    return 0;
  }
  a.trace = nullptr;
  switch (dp.rg) {
    case 1: hipLaunchKernelGGL((k_decoder_bwd_xcd<1>), grid, blk, dp.lds_bytes, st, a); break;
    case 2: hipLaunchKernelGGL((k_decoder_bwd_xcd<2>), grid, blk, dp.lds_bytes, st, a); break;
    case 4: hipLaunchKernelGGL((k_decoder_bwd_xcd<4>), grid, blk, dp.lds_bytes, st, a); break;
    default: hipLaunchKernelGGL((k_decoder_bwd_xcd<8>), grid, blk, dp.lds_bytes, st, a); break;
  }
  HIPCHK(hipGetLastError());
  return 0;
}
static int decoder_forward(const taco_model* m, hipStream_t st, const float* enc_out, const SpkSel& sel, int B,
                           int T_in, int n, const float* manual, const float* teacher, float* mel, float* align_out,
                           int* stop_step, float* dbg, const DecWs& w, bool spk_ready, const SpkWs* spk_in) {
  const taco_hparams& hp = m->hp;
  const int D = 2 * hp.enc_rnn_size, As = hp.attention_state_size, Hd = hp.dec_rnn_size, A = hp.attention_size;
  const int Mm = hp.num_mels, rM = hp.num_mels * hp.reduction_factor, L = hp.dec_layer_num;
  if (T_in > ATT_MAXT) return fail(TACO_ERR_UNSUPPORTED, "T_in %d > %d", T_in, ATT_MAXT);
  if ((A % 4) || (D % 4)) return fail(TACO_ERR_UNSUPPORTED, "attention_size and 2*enc_rnn_size must be multiples of 4");
  const SpkWs* spk = spk_in ? spk_in : &w.spk;
  if (is_deepvoice(m) && !spk_ready) TRY(spk_forward(m, st, sel, B, *spk));
  if (is_simple(m) && !sel.given()) return fail(TACO_ERR_ARG, "speaker_id required for a multi-speaker model");
  // attention memory: keys = values . W_mem, no bias, no length mask (A.8)
  { GemmCall g; g.x = enc_out; g.ldx = D; g.M = B * T_in; g.out = w.keys; g.ldo = A;
    TRY(run_gemm(m, st, &m->memory_layer, 1, false, g)); }
  // initial state (rnn_wrappers.py:186-216; tacotron.py:183-197)
  auto fill = [&](const float* src, int lds, float* dst, int C) {
    hipLaunchKernelGGL(k_copy2d, dim3(cdiv(B * C, 256)), dim3(256), 0, st, src, lds, dst, C, B, C);
  };
  const bool dv = is_deepvoice(m);
  const int S = simple_S(m), ldc = As + D + S, np = hp.dec_prenet_n;   // ldc: row stride of [h_att | ctx | spk]
  const int Ilast = hp.dec_prenet[np - 1], ldz = Ilast + S;
  const int ldY = n * rM;   // mel buffer viewed as Y [B, n, r*num_mels] (tacotron.py:213-214 is a pure reshape)
  const int dbgw = As + D + L * Hd;
  HIPCHK(w.nz.clear(st));
  if (const DecPlan dp = decoder_plan(m, B, T_in, n, teacher ? DEC_TEACHER : DEC_INFER); dp.persistent) {
    // the whole loop as ONE persistent launch (taco_decoder_xcd.h), which builds its initial state itself (zeros or the deepvoice
    // vectors); the launch-per-stage loop below is the general path
    DxArgs ta; memset(&ta, 0, sizeof ta);
    if (teacher) { ta.teacher = teacher; ta.p1o_raw = m->tp ? nullptr : AP(m, m->dx_p1o_raw); }     // teacher-forced: the TAPE instantiation without a tape
    TRY(dx_launch(m, st, dp, enc_out, sel, nullptr, spk->emb, B, T_in, n, manual, mel, align_out, dbg, dbgw, w.keys, w.nzp(), w.dx, w.rowbias,
                  dv ? spk->vec[2] : nullptr, dv ? spk->vec[3] : nullptr, dv ? spk->vec[4] : nullptr, teacher ? &ta : nullptr));
    if (stop_step) {
      hipLaunchKernelGGL(k_stop_step, dim3(1), dim3(1024), 0, st, w.nzp(), B, n, stop_step);
      HIPCHK(hipGetLastError());
    }
    return 0;
  }
  fill(nullptr, 0, w.zero, Mm);
  hipLaunchKernelGGL(k_copy2d, dim3(cdiv(B * D, 256)), dim3(256), 0, st, (const float*)nullptr, 0, w.ctx, ldc, B, D);
  if (S) {  // speaker_embed = embedding_lookup(table, speaker_id) (tacotron.py:44-49), parked behind ctx and behind the prenet output
    TRY(spk_rows(m, st, sel, AP(m, m->spk_emb), B, S, spk->emb));
    hipLaunchKernelGGL(k_copy2d, dim3(cdiv(B * S, 256)), dim3(256), 0, st, spk->emb, S, w.ctx + D, ldc, B, S);
    hipLaunchKernelGGL(k_copy2d, dim3(cdiv(B * S, 256)), dim3(256), 0, st, spk->emb, S, w.pz[np - 1] + Ilast, ldz, B, S);
  }
  hipLaunchKernelGGL(k_copy2d, dim3(cdiv(B * As, 256)), dim3(256), 0, st, dv ? (const float*)spk->vec[2] : (const float*)nullptr, As, w.h_att, ldc, B, As);
  for (int i = 0; i < L; ++i) fill(dv ? spk->vec[3 + i] : nullptr, Hd, w.hd[i], Hd);
  hipLaunchKernelGGL(k_init_align, dim3(cdiv(B * T_in, 256)), dim3(256), 0, st, w.align, B, T_in, hp.attention_type == 2 ? 1 : 0);
  HIPCHK(hipGetLastError());
  for (int t = 0; t < n; ++t) {
    // frame fed to the prenet: zeros at t=0 (helpers.py:70-72), else last of the r frames (helpers.py:31)
    const float* frame; int ldf;
    if (t == 0) { frame = w.zero; ldf = Mm; }
    else if (teacher) { frame = teacher + (size_t)(t - 1) * Mm; ldf = n * Mm; }
    else { frame = mel + (size_t)(t - 1) * rM + (rM - Mm); ldf = ldY; }
    // DecoderPrenetWrapper (rnn_wrappers.py:249,367-378): prenet(concat(frame, previous context))
    const float* cur = nullptr; int curd = 0;
    // layer 1 of steps t >= 1 was already produced by step t-1's frame-projection launch (prenet1_next), unless frames are teacher-forced
    const bool fuse_p1 = m->fuse_prenet1 && !teacher && np > 1;
    for (int i = 0; i < hp.dec_prenet_n; ++i) {
      const int ldo = (i == np - 1) ? ldz : hp.dec_prenet[i];
      if (!(i == 0 && fuse_p1 && t > 0)) {
        SkJob j = (i == 0) ? sk_linear(m, m->dec_prenet[0], frame, ldf, Mm, w.ctx, ldc, ACT_RELU, w.pz[0], ldo)
                           : sk_linear(m, m->dec_prenet[i], cur, curd, curd, nullptr, 0, ACT_RELU, w.pz[i], ldo);
        TRY(run_skinny(st, B, &j, 1));
      }
      cur = w.pz[i]; curd = hp.dec_prenet[i];
    }
    // attention GRUCell (tacotron.py:127-130); 'simple': input = concat(prenet_out, speaker_embed) (rnn_wrappers.py:372-376)
    TRY(run_gru_cell(m, st, m->att_gru, B, cur, ldz, w.h_att, w.rh, w.u, w.xc, nullptr, ldc));
    // query + score + normaliser + context (rnn_wrappers.py:304-341)
    // the query mat-vec runs inside the attention kernel (one launch less) when its partials fit the kernel's LDS
    const bool fuse_q = (A % 4 == 0) && A <= ATT_MAXT && A / 4 <= 64 * ATT_NW;
    if (!fuse_q) { SkJob j = sk_linear(m, m->query, w.h_att, ldc, As, nullptr, 0, ACT_NONE, w.q, A);
      TRY(run_skinny(st, B, &j, 1)); }
    { AttnArgs a; memset(&a, 0, sizeof a);
      a.q = fuse_q ? nullptr : w.q; a.hq = w.h_att; a.ldhq = ldc; a.wq = AP(m, m->raw_wq); a.As = As; a.keys = w.keys; a.values = enc_out; a.v = AP(m, m->att_v); a.battn = AP(m, m->att_b);
      a.score_bias = AP(m, m->att_sb); a.manual = manual; a.align = w.align; a.hist = align_out; a.ctx = w.ctx; a.ldctx = ldc;
      a.T_in = T_in; a.A = A; a.D = D; a.type = hp.attention_type; a.step = t; a.n_steps = n;
      // few rows x many encoder positions (C5): two launches that spread every row over att_split workgroups
      const int att_split = (m->att_split >= 0) ? m->att_split : ((B <= 16 && T_in >= 256 && A % 4 == 0 && A <= 1024 && A / 4 <= 64 * ATS_NW) ? 4 : 0);
      if (att_split > 1 && fuse_q) {
        if (!manual) hipLaunchKernelGGL(k_att_scores, dim3(B, att_split), dim3(64 * ATS_NW), 0, st, a, w.escr, att_split);
        hipLaunchKernelGGL(k_att_context, dim3(B, att_split), dim3(64 * ATS_NW), 0, st, a, (const float*)w.escr, att_split);
      } else {
        hipLaunchKernelGGL(k_attention, dim3(B), dim3(64 * ATT_NW), 0, st, a);
      }
      HIPCHK(hipGetLastError()); }
    // ConcatOutputAndAttentionWrapper + OutputProjectionWrapper (rnn_wrappers.py:405-415; tacotron.py:166-170)
    // 'simple': + speaker_embed (rnn_wrappers.py:408-413).  The projection is linear, so by default it is folded into the x rows
    // of the first decoder GRU (gru1_fold): its gates launch reads [h_att | ctx | spk] directly and also emits o0 for the residual.
    const bool fold = m->fuse_concat && L > 0;
    if (!fold) { SkJob j = sk_linear(m, m->concat_proj, w.h_att, ldc, As, w.ctx, ldc, ACT_NONE, w.o[0], Hd);
      TRY(run_skinny(st, B, &j, 1)); }
    // residual GRU stack (tacotron.py:171-172)
    for (int i = 0; i < L; ++i) {
      if (i == 0 && fold) TRY(run_gru_cell(m, st, m->gru1_fold, B, w.h_att, ldc, w.hd[0], w.rh, w.u, w.xc, w.o[1], 0, 2 * Hd));
      else TRY(run_gru_cell(m, st, m->dec_gru[i], B, w.o[i], Hd, w.hd[i], w.rh, w.u, w.xc, w.o[i + 1]));
    }
    // frame projection to r frames (tacotron.py:178-179), written straight into the mel buffer
    { SkJob j[2];
      j[0] = sk_linear(m, m->frame_proj, w.o[L], Hd, Hd, nullptr, 0, ACT_NONE, mel + (size_t)t * rM, ldY);
      j[0].o2 = reinterpret_cast<float*>(w.nzp() + (size_t)t * B);
      int nj = 1;
      if (fuse_p1 && t + 1 < n) { j[1] = sk_linear(m, m->prenet1_next, w.o[L], Hd, Hd, w.ctx, ldc, ACT_RELU, w.pz[0], hp.dec_prenet[0]); nj = 2; }
      TRY(run_skinny(st, B, j, nj)); }
    if (dbg) {
      float* d = dbg + (size_t)t * B * dbgw;
      hipLaunchKernelGGL(k_copy2d, dim3(cdiv(B * As, 256)), dim3(256), 0, st, w.h_att, ldc, d, dbgw, B, As);
      hipLaunchKernelGGL(k_copy2d, dim3(cdiv(B * D, 256)), dim3(256), 0, st, w.ctx, ldc, d + As, dbgw, B, D);
      for (int i = 0; i < L; ++i)
        hipLaunchKernelGGL(k_copy2d, dim3(cdiv(B * Hd, 256)), dim3(256), 0, st, w.hd[i], Hd, d + As + D + i * Hd, dbgw, B, Hd);
      HIPCHK(hipGetLastError());
    }
  }
  if (stop_step) {
    hipLaunchKernelGGL(k_stop_step, dim3(1), dim3(1024), 0, st, w.nzp(), B, n, stop_step);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// ---- post-net + linear head (tacotron.py:219-235) ----
struct PostWs { CbhgWs cb; float* post_out; float* spk_emb; float* rowvec; };
static void carve_post(Carver& cv, const taco_model* m, int B, int T, PostWs& w) {
  carve_cbhg(cv, m->post, B, T, w.cb);
  w.post_out = cv.f((size_t)B * T * 2 * m->hp.post_rnn_size);
  w.spk_emb = cv.f((size_t)B * std::max(simple_S(m), 1));
  w.rowvec = cv.f((size_t)B * m->hp.num_freq);
}
static int postnet_forward(const taco_model* m, hipStream_t st, const float* mel, const SpkSel& sel, int B, int T,
                           float* linear, float* post_out_user, const PostWs& w) {
  TRY(cbhg_ff(m, st, m->post, mel, B, T, nullptr, nullptr, w.cb));
  float* po = post_out_user ? post_out_user : w.post_out;
  TRY(bigru_scan(m, st, m->post, B, T, nullptr, nullptr, po, w.cb));
  GemmCall g; g.x = po; g.ldx = 2 * m->hp.post_rnn_size; g.M = B * T; g.out = linear; g.ldo = m->hp.num_freq;
  if (is_simple(m)) {
    // linear(concat(tiled speaker_embed, post)) (tacotron.py:226-235) = post . W[S:] + (speaker_embed . W[:S]) per batch row
    if (!sel.given()) return fail(TACO_ERR_ARG, "speaker_id required for a multi-speaker model");
    const int S = simple_S(m), F = m->hp.num_freq;
    TRY(spk_rows(m, st, sel, AP(m, m->spk_emb), B, S, w.spk_emb));
    SkJob j = sk_linear(m, m->lin_spk, w.spk_emb, S, S, nullptr, 0, ACT_NONE, w.rowvec, F);
    TRY(run_skinny(st, B, &j, 1));
    g.T = T; g.rowvec = w.rowvec; g.ldrv = F;
  }
  return run_gemm(m, st, &m->linear, 1, false, g);
}

struct FullWs { EncWs enc; DecWs dec; PostWs post; float* enc_out; };
static void carve_full(Carver& cv, const taco_model* m, int B, int T_in, int n, FullWs& w) {
  carve_enc(cv, m, B, T_in, w.enc);
  w.enc_out = cv.f((size_t)B * T_in * 2 * m->hp.enc_rnn_size);
  carve_dec(cv, m, B, T_in, n, w.dec);
  carve_post(cv, m, B, n * m->hp.reduction_factor, w.post);
}

static int check_model_shape(const taco_model* m, int B, int T) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  if (!m->finalized) return fail(TACO_ERR_STATE, "model not finalized");
  if (B <= 0 || T <= 0) return fail(TACO_ERR_ARG, "bad batch/time %d/%d", B, T);
  return 0;
}
static int check_common(const taco_model* m, int B, int T) {      // an entry that serves one pass only
  TRY(check_model_shape(m, B, T));
  if (B > 64) return fail(TACO_ERR_UNSUPPORTED, "batch %d > 64 rows per device is not supported: shard the batch", B);
  return 0;
}

// Any batch size (synthesizer.py:120-131 and eval.py:86-119 put no cap on it): more than `cap` rows -- 64, what the persistent kernels place on one
// chip: 8 groups x 8 rows -- run as ceil(B / cap) passes of equal size over the SAME workspace, back to back on the caller's stream (batch rows are
// independent at inference: BatchNorm uses the moving statistics, modules.py:131).  The forward and every stage entry validate their arguments
// once, carve one pass's workspace at pp.rows, and hand each pass to a single-pass function through for_each_pass.
struct PassPlan { int passes, rows; };
static PassPlan pass_plan(int B, int cap = 64) { PassPlan p; p.passes = (B + cap - 1) / cap; p.rows = p.passes ? (B + p.passes - 1) / p.passes : 0; return p; }
template <class Body>
static int for_each_pass(const PassPlan& pp, int B, Body body) {      // body(b0, rows, pass index): rows b0 .. b0 + rows - 1 of the batch
  for (int p = 0, b0 = 0; b0 < B; ++p, b0 += pp.rows) TRY(body(b0, std::min(pp.rows, B - b0), p));
  return 0;
}
// The stop step of the batch (helpers.py:29 with dynamic_decode's all-rows-finished loop condition) is the maximum over the passes' stop steps -- a
// row's `finished` is sticky, so the loop would have ended when the LAST pass's rows were all done; a negative pass word (a persistent kernel gave
// up) wins.  The passes' words are carved behind the pass workspace (null: one pass, which writes the caller's word itself).
static int32_t* carve_pass_stops(Carver& cv, const PassPlan& pp) { return pp.passes > 1 ? (int32_t*)cv.i((size_t)pp.passes) : nullptr; }
__global__ void k_stop_combine(const int* pstop, int np, int* stop) {
  if (threadIdx.x == 0) {
    int worst = 0, err = 0;
    for (int i = 0; i < np; ++i) { const int v = pstop[i]; if (v < 0 && !err) err = v; worst = max(worst, v); }
    *stop = err ? err : worst;
  }
}
static int combine_pass_stops(hipStream_t st, const int32_t* pstop, const PassPlan& pp, int32_t* stop) {
  if (!stop || !pstop) return 0;
  hipLaunchKernelGGL(k_stop_combine, dim3(1), dim3(64), 0, st, (const int*)pstop, pp.passes, stop);
  HIPCHK(hipGetLastError());
  return 0;
}
// Rows one pass of the decoder loop may hold: 64 (8 groups x 8 rows) -- but an inference model with attention_size 512 (hparams.py:71-82, the first
// "Deep Voice 2" block) has no persistent instantiation at 8 rows per group, so its passes hold at most 32 rows: two passes on the persistent decoder
// instead of one on the launch-per-stage loop, which is four times slower per step.  state_dump (taco_decoder_forward's, laid out [step][row]): one pass.
static int decoder_pass_rows(const taco_model* m, bool state_dump = false) {
  // (with the call's T_in and n passed down: `&& decoder_plan(m, CHIP_ROWS / 2, T_in, n, DEC_INFER).persistent` -- today the rule looks at no shape)
  return !state_dump && decoder_plan(m, CHIP_ROWS, 0, 0, DEC_INFER).why == DEC_WHY_NO_INSTANTIATION ? CHIP_ROWS / 2 : CHIP_ROWS;
}

// One pass of the forward: B <= decoder_pass_rows(m) rows, arguments validated and w carved (for at least B rows) by forward_enqueue; w is this
// pass's own copy, so what it learns about cleared regions ends with the pass
static int forward_pass(taco_model* m, hipStream_t st, const int32_t* ids, const int32_t* lengths, const SpkSel& spk,
                        int B, int T_in, int n, const float* manual, float* mel, float* linear, float* align,
                        int32_t* stop, FullWs w) {
  const int r = m->hp.reduction_factor, T_mel = n * r;
  const bool ride = prenet_chain_why(m) == FF_WHY_NONE;      // the encoder prenet as the chain launch: asked once per forward
  // every word a persistent kernel polls and the stop flags, cleared by ONE launch in front of the forward -- riding in the encoder prenet's
  // launch where that is the chain kernel: the first launch of the forward, with CUs to spare; the stop rule and the error latch are ONE
  // launch behind it (11 graph nodes at C2 with the clears riding; 13 in round 4, 20 in round 3).  The regions count as cleared
  // (Polled::clear then skips its own fill) only from the point where the launch that clears them HAS been enqueued: here for the fill
  // kernel, inside run_prenet_chain for the riders.
  Polled* const polled[CH_RIDERS] = {&w.dec.dx, &w.dec.nz, &w.post.cb.gx, &w.enc.cb.gx};      // (an encoder of width 256 scans on k_bigru_duo too)
  UpFrontClear up; memset(&up.z, 0, sizeof up.z);
  for (int i = 0; i < CH_RIDERS; ++i) { up.z.p[i] = static_cast<uint32_t*>(polled[i]->p); up.z.nw[i] = polled[i]->bytes / 4; polled[i]->cleared = &up; }
  if (!ride) {
    hipLaunchKernelGGL(k_zero_fill, dim3(256, CH_RIDERS), dim3(256), 0, st, up.z);
    HIPCHK(hipGetLastError());
    up.enqueued = true;
  }
  TRY(encoder_forward(m, st, ids, lengths, spk, B, T_in, w.enc_out, w.enc, false, ride, ride ? &up : nullptr));
  TRY(decoder_forward(m, st, w.enc_out, spk, B, T_in, n, manual, nullptr, mel, align, nullptr, nullptr, w.dec, true, &w.enc.spk));
  TRY(postnet_forward(m, st, mel, spk, B, T_mel, linear, nullptr, w.post));
  if (stop) {
    hipLaunchKernelGGL(k_stop_step, dim3(1), dim3(1024), 0, st, (const int*)w.dec.nzp(), B, n, stop, (const unsigned*)m->d_err);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

static PassPlan forward_passes(const taco_model* m, int B) { return pass_plan(B, decoder_pass_rows(m)); }
static int32_t* carve_forward(Carver& cv, const taco_model* m, const PassPlan& pp, int T_in, int n, FullWs& w) {      // -> the passes' stop words
  carve_full(cv, m, pp.rows, T_in, n, w);
  return carve_pass_stops(cv, pp);
}
static int forward_enqueue(taco_model* m, hipStream_t st, const int32_t* ids, const int32_t* lengths, const SpkSel& spk,
                           int B, int T_in, int n, const float* manual, float* mel, float* linear, float* align,
                           int32_t* stop, void* ws, size_t ws_bytes) {
  TRY(check_model_shape(m, B, T_in));
  if (n <= 0) return fail(TACO_ERR_ARG, "n_steps must be positive");
  if (!ids || !lengths || !mel || !linear || !align || !ws) return fail(TACO_ERR_ARG, "null buffer");
  if (m->hp.num_speakers > 1 && !spk.given()) return fail(TACO_ERR_ARG, "speaker_id required for a multi-speaker model");
  const PassPlan pp = forward_passes(m, B);
  Carver cv(ws, ws_bytes);
  FullWs w;
  int32_t* pstop = carve_forward(cv, m, pp, T_in, n, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes, have %zu", cv.off, ws_bytes);
  const size_t rM = (size_t)m->hp.reduction_factor * m->hp.num_mels, T_mel = (size_t)n * m->hp.reduction_factor;
  TRY(for_each_pass(pp, B, [&](int b0, int rows, int p) {
    return forward_pass(m, st, ids + (size_t)b0 * T_in, lengths + b0, spk.rows_from(b0, m->hp.num_speakers), rows, T_in, n,
                        manual ? manual + (size_t)b0 * n * T_in : nullptr, mel + (size_t)b0 * n * rM, linear + (size_t)b0 * T_mel * m->hp.num_freq,
                        align + (size_t)b0 * T_in * n, !stop ? nullptr : pstop ? pstop + p : stop, w);
  }));
  return combine_pass_stops(st, pstop, pp, stop);
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
#include "taco_segnorm.h"
// The priority band of add_loss (tacotron.py:283-288): bins [lo, hi) of linear_loss[:, :, lo:hi].  A slice clamps its upper end to the axis: below
// 10000 Hz the 5 kHz bin lies past num_freq (8000 Hz, 1025 bins: 1281), and the band's mean is over the bins that exist.  The loss and the step's
// L1 gradient (head_backward, taco_train.h) both count the band with this.
static void loss_band(int sample_rate, int num_freq, int* lo, int* hi) {
  *hi = std::min((int)(5000 / (sample_rate * 0.5) * num_freq), num_freq);
  *lo = std::min((int)(165 / (sample_rate * 0.5) * num_freq), *hi);
}
#include "taco_train.h"
#include "taco_audio.h"
#include "taco_resample.h"
#include "taco_feed.h"
#include "taco_align.h"
#include "taco_dtw.h"
#include "taco_f0.h"
#include "taco_warp.h"
#include "taco_envelope.h"

extern "C" {

int taco_abi_version(void) { return TACO_ABI_VERSION; }
const char* taco_last_error(void) { return g_err.c_str(); }

int taco_model_create(const taco_hparams* hp, int device, taco_model** out) {
  if (!hp || !out) return fail(TACO_ERR_ARG, "null argument");
  if (hp->model_type < 0 || hp->model_type > 2) return fail(TACO_ERR_UNSUPPORTED, " [!] Unkown multi-speaker model type: %d", hp->model_type);
  if (hp->attention_type < 0 || hp->attention_type > 2) return fail(TACO_ERR_UNSUPPORTED, " [!] Unkown attention type: %d", hp->attention_type);
  if (hp->num_speakers > 1 && hp->model_type == 1 && hp->speaker_embedding_size == 1)
    return fail(TACO_ERR_UNSUPPORTED, "model_type 'simple' with speaker_embedding_size 1 leaves speaker_embed undefined in the reference (tacotron.py:44-49,82-86)");
  if (hp->num_speakers > 1 && hp->model_type == 1 && hp->speaker_embedding_size % 4)
    return fail(TACO_ERR_UNSUPPORTED, "model_type 'simple' needs speaker_embedding_size to be a multiple of 4");
  if (hp->num_speakers > 1 && hp->model_type == 0)
    return fail(TACO_ERR_UNSUPPORTED, " [!] Unkown multi-speaker model type: single (num_speakers > 1 needs simple or deepvoice)");
  if (hp->enc_prenet_n < 1 || hp->enc_prenet_n > 4 || hp->dec_prenet_n < 1 || hp->dec_prenet_n > 4 || hp->enc_proj_n < 1 ||
      hp->enc_proj_n > 4 || hp->post_proj_n < 1 || hp->post_proj_n > 4 || hp->dec_layer_num < 1 || hp->dec_layer_num > 4)
    return fail(TACO_ERR_ARG, "layer-count hparams out of range");
  if (hp->enc_proj[hp->enc_proj_n - 1] != hp->enc_prenet[hp->enc_prenet_n - 1])
    return fail(TACO_ERR_SHAPE, "encoder CBHG residual needs enc_proj_sizes[-1] == enc_prenet_sizes[-1]");
  if (hp->post_proj[hp->post_proj_n - 1] != hp->num_mels)
    return fail(TACO_ERR_SHAPE, "post CBHG residual needs post_proj_sizes[-1] == num_mels");
  if (hp->attention_state_size % 4 || hp->dec_rnn_size % 4 || hp->enc_rnn_size % 4 || hp->post_rnn_size % 4 || hp->num_mels % 4)
    return fail(TACO_ERR_UNSUPPORTED, "rnn sizes and num_mels must be multiples of 4");
  taco_model* m = new taco_model();
  m->hp = *hp;
  m->device = device;
  build_spec(m);
  cbhg_dims(m->enc, hp->enc_prenet[hp->enc_prenet_n - 1], hp->enc_bank_size, hp->enc_bank_channels, hp->enc_maxpool,
            hp->enc_highway_depth, hp->enc_rnn_size, hp->enc_proj, hp->enc_proj_n, hp->enc_proj_width);
  cbhg_dims(m->post, hp->num_mels, hp->post_bank_size, hp->post_bank_channels, hp->post_maxpool, hp->post_highway_depth,
            hp->post_rnn_size, hp->post_proj, hp->post_proj_n, hp->post_proj_width);
  *out = m;
  return 0;
}

int taco_model_num_weights(const taco_model* m) { return m ? (int)m->spec.size() : 0; }

int taco_model_weight_name(const taco_model* m, int i, char* buf, int buflen, int64_t* shape4, int* ndim) {
  if (!m || i < 0 || i >= (int)m->spec.size() || !buf) return fail(TACO_ERR_ARG, "bad index");
  snprintf(buf, buflen, "%s", m->spec[i].first.c_str());
  if (ndim) *ndim = (int)m->spec[i].second.size();
  if (shape4) for (size_t d = 0; d < m->spec[i].second.size() && d < 4; ++d) shape4[d] = m->spec[i].second[d];
  return 0;
}

int taco_model_set_weight(taco_model* m, const char* name, const float* host, const int64_t* shape, int ndim) {
  if (!m || !name || !host || ndim < 0 || (ndim > 0 && !shape)) return fail(TACO_ERR_ARG, "null argument");
  if (m->finalized) return fail(TACO_ERR_STATE, "model already finalized");
  for (auto& s : m->spec) {
    if (s.first != name) continue;
    if ((int)s.second.size() != ndim) return fail(TACO_ERR_SHAPE, "%s: rank %d, expected %zu", name, ndim, s.second.size());
    size_t n = 1;
    for (int d = 0; d < ndim; ++d) {
      if (shape[d] != s.second[d]) return fail(TACO_ERR_SHAPE, "%s: dim %d is %lld, expected %lld", name, d, (long long)shape[d], (long long)s.second[d]);
      n *= (size_t)shape[d];
    }
    HostTensor& t = m->raw[name];
    t.shape.assign(shape, shape + ndim);
    t.data.assign(host, host + n);
    t.set = true;
    return 0;
  }
  return fail(TACO_ERR_ARG, "unknown weight name '%s'", name);
}

// step 3 of taco_model_finalize: the arena on the device, the GemmVar table's offsets resolved to pointers into it, the sticky error word
static int model_upload(taco_model* m) {
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipDeviceGetAttribute(&m->cu_count, hipDeviceAttributeMultiprocessorCount, m->device));
  HIPCHK(hipMalloc((void**)&m->darena, m->harena.size() * sizeof(float)));
  HIPCHK(hipMemcpy(m->darena, m->harena.data(), m->harena.size() * sizeof(float), hipMemcpyHostToDevice));
  m->arena_n = m->harena.size();
  m->harena.clear(); m->harena.shrink_to_fit();
  for (auto& v : m->hvars) {
    v.wp = AP(m, (size_t)v.wp); v.wp2 = AP(m, (size_t)v.wp2); v.bias = AP(m, (size_t)v.bias); v.bias2 = AP(m, (size_t)v.bias2);
    v.bn_scale = AP(m, (size_t)v.bn_scale); v.bn_shift = AP(m, (size_t)v.bn_shift);
    v.bh = (const unsigned short*)AP(m, (size_t)v.bh); v.bl = (const unsigned short*)AP(m, (size_t)v.bl);
    v.bh2 = (const unsigned short*)AP(m, (size_t)v.bh2); v.bl2 = (const unsigned short*)AP(m, (size_t)v.bl2);
    v.bl3 = (const unsigned short*)AP(m, (size_t)v.bl3); v.bl3_2 = (const unsigned short*)AP(m, (size_t)v.bl3_2);
  }
  HIPCHK(hipMalloc((void**)&m->d_err, 256));
  HIPCHK(hipMemset(m->d_err, 0, 256));
  return 0;
}
// step 4: > 64 KB of dynamic LDS has to be asked for, per kernel and device; the persistent kernels carve up to the full 160 KiB
static int set_kernel_attributes() {
#define LDS_ATTR(bytes, ...) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&__VA_ARGS__), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
#define LDS_160K(...) LDS_ATTR(160 * 1024, __VA_ARGS__)
  LDS_160K(k_cbhg_front<2, 80, 80, 8>) LDS_160K(k_cbhg_front<1, 144, 128, 16>)
  LDS_160K(k_bigru_res<256, 64, 24, 1, false>) LDS_160K(k_bigru_res<128, 32, 0, 1, false>)
  LDS_160K(k_bigru_res<256, 64, 24, 1, true>) LDS_160K(k_bigru_res<128, 32, 0, 1, true>)
  LDS_160K(k_bigru_resw<16, 4, 2>)
  LDS_160K(k_bigru_rows<1, false>) LDS_160K(k_bigru_rows<2, false>) LDS_160K(k_bigru_rows<1, true>) LDS_160K(k_bigru_rows<2, true>)
  LDS_160K(k_pointwise_chain<256>) LDS_160K(k_head_sweep<512>) LDS_160K(k_head_sweep<256>) LDS_160K(k_pointwise_chain<128>)
  TRY(gemm_set_attributes());
#define DX_ATTR(...) LDS_ATTR(DX_LDS_BUDGET, k_decoder_xcd<__VA_ARGS__>)
#define PLAIN(RG, TAPE, AW, PD) DX_ATTR(RG, TAPE, false, AW, PD)
#define MANUAL(RG, TAPE, AW, PD) DX_ATTR(RG, TAPE, true, AW, PD)
#define BOTH(RG, TAPE, AW, PD) PLAIN(RG, TAPE, AW, PD) MANUAL(RG, TAPE, AW, PD)
#define STAMPED(RG, TAPE, AW, PD) DX_ATTR(RG, TAPE, false, AW, PD, true)
  DX_REFERENCE(PLAIN) DX_REFERENCE(MANUAL) DX_REFERENCE_TAPE(BOTH) DX_REFERENCE(STAMPED) DX_PRESETS(BOTH)      // (the order of the kernels in the code object)
#undef DX_ATTR
#undef PLAIN
#undef MANUAL
#undef BOTH
#undef STAMPED
#undef LDS_160K
#undef LDS_ATTR
  return 0;
}

int taco_model_finalize(taco_model* m) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  if (m->finalized) return 0;
  for (auto& s : m->spec)
    if (!m->raw.count(s.first) || !m->raw[s.first].set) return fail(TACO_ERR_STATE, "weight '%s' was never set", s.first.c_str());
  TRY(model_pack_host(m));
  TRY(model_upload(m));
  TRY(set_kernel_attributes());
  m->raw.clear();
  m->finalized = true;
  return 0;
}

void taco_model_destroy(taco_model* m) {
  if (!m) return;
  if (m->darena) (void)hipFree(m->darena);
  if (m->d_err) (void)hipFree(m->d_err);
  if (m->d_trace) (void)hipFree(m->d_trace);
  delete m;
}

int taco_model_device_errors(taco_model* m, int* out) {
  if (!m || !m->finalized || !out) return fail(TACO_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(m->device));
  unsigned v = 0;
  HIPCHK(hipMemcpy(&v, m->d_err, sizeof v, hipMemcpyDeviceToHost));
  if (v) HIPCHK(hipMemset(m->d_err, 0, 256));
  *out = (int)v;
  return 0;
}

// test hook: raise the sticky device error word by hand (what a persistent kernel does when its bounded spin expires)
int taco_debug_raise_device_error(taco_model* m, int value) {
  if (!m || !m->finalized) return fail(TACO_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(m->device));
  const unsigned v = (unsigned)value;
  HIPCHK(hipMemcpy(m->d_err, &v, sizeof v, hipMemcpyHostToDevice));
  return 0;
}

int taco_debug_set_bf3(taco_model* m, int on, int tile_n) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  if (!gemm_tile_known(tile_n)) return fail(TACO_ERR_ARG, "tile_n is not one of 0, 4, 5, 7, 9, 10");
  m->bf3 = (on & 1) != 0; m->bf3_tn = tile_n;
  m->chain = (on & 4) ? 0 : 1;     // on = 5: split-bf16 GEMMs with one launch per point-wise layer (A/B of taco_chain.h)
  m->front = (on & 8) ? 0 : 1;     // on = 9: conv bank and proj_1 as two k_gemm_bf3 launches (A/B of taco_front.h)
  m->front_entry = (on & 16) ? 0 : 1;   // on = 17: fused front, but k_front_combine and proj_2 as launches of their own (A/B of the chain's fused entry)
  m->head_sweep = (on & 32) ? 0 : 1;    // on = 33: the linear head on k_gemm_bf3's 64 x 256 tiles (A/B of taco_head.h)
  // on = 65: EVERY feed-forward layer on the six-product instantiation of k_gemm_bf3 (operands split three ways: fp32-grade products on the bf16
  // pipe), one launch per layer -- the fused front / chain / head kernels are three-product kernels and stay out of this mode
  if (!m->tp) m->bf3x6 = (on & 64) ? 1 : 0;
  return 0;
}

int taco_attention_trim(void* hip_stream, const float* d_alignments, const int32_t* d_seq_len, int B, int T_in, int n_steps,
                        int reduction_factor, int32_t* d_spec_end) {
  if (!d_alignments || !d_seq_len || !d_spec_end || B <= 0 || T_in <= 0 || n_steps <= 0) return fail(TACO_ERR_ARG, "bad argument");
  if ((size_t)n_steps * sizeof(int) > 64 * 1024) return fail(TACO_ERR_UNSUPPORTED, "more than 16384 decoder steps");
  hipLaunchKernelGGL(k_attention_trim, dim3(B), dim3(64), (size_t)n_steps * sizeof(int), (hipStream_t)hip_stream, d_alignments, d_seq_len, T_in,
                     n_steps, reduction_factor, d_spec_end);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_manual_alignments(void* hip_stream, const float* d_alignments, int B, int T_in, int n_steps, int mode, float* d_manual) {
  if (!d_alignments || !d_manual) return fail(TACO_ERR_ARG, "null pointer");
  if (B < 1 || T_in < 1 || n_steps < 1) return fail(TACO_ERR_ARG, "B, T_in and n_steps must be >= 1, got %d, %d, %d", B, T_in, n_steps);
  const u128 bytes = (u128)B * (unsigned)T_in * (unsigned)n_steps * sizeof(float);
  TRY(no_overlap({{d_manual, bytes, "d_manual"}, {d_alignments, bytes, "d_alignments"}}, 1));      // the transpose cannot run in place
  if (mode == 2) return fail(TACO_ERR_UNSUPPORTED, "manual_attention_mode 2 is broken in the reference (np.pow, synthesizer.py:181-188)");
  if (mode != 1 && mode != 3) return fail(TACO_ERR_ARG, "manual_attention_mode %d: accepted are 1 (argmax one hot) and 3 (prunning)", mode);
  const int tiles = (T_in + MA_TE - 1) / MA_TE;
  if ((long long)B * tiles > 0x7fffffffLL) return fail(TACO_ERR_UNSUPPORTED, "more than 2^31 - 1 workgroups (B * ceil(T_in / %d))", MA_TE);
  hipLaunchKernelGGL(k_manual_alignments, dim3((unsigned)(B * tiles)), dim3(MA_TE / MA_ROWS * 64), 0, (hipStream_t)hip_stream, d_alignments, T_in, n_steps, tiles, mode,
                     d_manual);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_stop_steps(void* hip_stream, const float* d_mel, int B, int n_steps, int width, int rows_per_group, int32_t* d_stop) {
  if (!d_mel || !d_stop || B <= 0 || n_steps <= 0 || width <= 0 || rows_per_group <= 0 || B % rows_per_group)
    return fail(TACO_ERR_ARG, "bad argument");
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHK(zero_async(d_stop, (size_t)(B / rows_per_group) * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_stop_groups, dim3(B), dim3(256), 0, st, d_mel, n_steps, width, rows_per_group, d_stop);
  HIPCHK(hipGetLastError());
  return 0;
}

// on: every tile of k_pointwise_chain walks a layer's K from step 0, so a row's fp32 accumulation order does not depend on the tile -- i.e. on
// the batch position or the shard -- it lands in: outputs are bit-invariant under batch permutation at any size.  off (default): the
// workgroups of an XCD start at different steps (they do not all ask the L2 for the same weight slices at once): results
// stay reproducible run to run, and equal under permutation to fp32 rounding, bitwise only while the launch has fewer than 8 tiles.
int taco_model_set_batch_invariant(taco_model* m, int on) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  m->ff_rot = on ? 0 : 1;
  return 0;
}
int taco_debug_set_att_split(taco_model* m, int slices) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  m->att_split = slices;
  return 0;
}
int taco_debug_set_fuse_prenet(taco_model* m, int on) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  m->fuse_prenet1 = on ? 1 : 0;
  return 0;
}
#ifdef TACO_TRACE
int taco_debug_read_trace(long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(taco_trace), 64 * sizeof(long long)) == hipSuccess ? 0 : -1; }
int taco_debug_read_trace_front(long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(taco_trace_front), 64 * sizeof(long long)) == hipSuccess ? 0 : -1; }
int taco_debug_read_trace_head(long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(taco_trace_head), 16 * sizeof(long long)) == hipSuccess ? 0 : -1; }
int taco_debug_read_trace_chain(long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(taco_trace_chain), 64 * sizeof(long long)) == hipSuccess ? 0 : -1; }
#endif
int taco_debug_set_fuse_concat(taco_model* m, int on) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  if (on && !m->gru1_fold.H) return fail(TACO_ERR_STATE, "the folded GRU pack was not built for this model");
  m->fuse_concat = on ? 1 : 0;
  return 0;
}
int taco_debug_set_overlap(taco_model* m, int on) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  return on ? fail(TACO_ERR_ARG, "the chunked post-net overlap is retired") : 0;
}

int taco_debug_set_persistent(taco_model* m, int on) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  switch (on) {
    case SCAN_PER_STEP: case SCAN_AUTO: case SCAN_ROWS: case SCAN_RES: case SCAN_RESW: case SCAN_OCT: case SCAN_DUO: break;
    default: return fail(TACO_ERR_ARG, "scan mode %d: accepted are 0 (two launches per step), 1 (default: the fastest kernel that fits), 2 (k_bigru_rows), "
                                       "3 (k_bigru_res), 7 (k_bigru_resw), 10 (k_bigru_oct wherever it fits), 11 (k_bigru_duo, never k_bigru_oct)", on);
  }
  m->persist = on;
  return 0;
}

int taco_debug_set_decoder_persist(taco_model* m, int mode, int rows_per_group) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  if (mode < 0 || mode > 2) return fail(TACO_ERR_ARG, "mode must be 0 (launch per stage), 1 (persistent) or 2 (persistent, write-through exchanges)");
  if (rows_per_group != 0 && rows_per_group != 1 && rows_per_group != 2 && rows_per_group != 4 && rows_per_group != 8)
    return fail(TACO_ERR_ARG, "rows_per_group %d: accepted are 0 (the smallest that covers the batch), 1, 2, 4 and 8", rows_per_group);
  m->dx_mode = mode; m->dx_rows = rows_per_group;
  return 0;
}
int taco_debug_decoder_info(taco_model* m, int* out16) {
  if (!m || !m->finalized || !out16) return fail(TACO_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(m->device));
  unsigned v[16];
  HIPCHK(hipMemcpy(v, m->d_err + 8, sizeof v, hipMemcpyDeviceToHost));
  for (int i = 0; i < 16; ++i) out16[i] = (int)v[i];
  { unsigned b = 0; HIPCHK(hipMemcpy(&b, m->d_err + 40, sizeof b, hipMemcpyDeviceToHost)); out16[9] = m->last_bptt ? (int)b : 0; }
  out16[14] = m->cu_count;
  out16[15] = m->dx_pack ? 1 : 0;
  return 0;
}
// Which engine a call of this shape would run on, and why not the persistent one when it would not (nothing is launched).  flags: taco_abi.h
int taco_model_engine_plan(taco_model* m, int B, int T_in, int T_mel, int flags, char* out, int out_len) {
  if (!m || !m->finalized || !out || out_len < 64) return fail(TACO_ERR_ARG, "bad argument");
  std::string s;
  const int cap = decoder_pass_rows(m, (flags & 4) != 0), n = std::max(1, T_mel / std::max(1, m->hp.reduction_factor));
  if (B > cap && !m->tp) {      // taco_forward_infer / taco_plan_create serve any batch as passes of at most 64 rows (32: attention_size 512); the plan below is a pass's
    const PassPlan pp = pass_plan(B, cap);
    s = std::to_string(B) + " rows = " + std::to_string(pp.passes) + " passes of " + std::to_string(pp.rows) + " (the last one " + std::to_string(B - (pp.passes - 1) * pp.rows) + "); per pass: ";
    B = pp.rows;
  }
  auto why_common = [&](int why, int rows) -> std::string {      // SCAN_WHY_* / DEC_WHY_*: the reasons all whole-chip kernels share
    if (why == DEC_WHY_ENGINE_OFF) return "switched off (taco_debug_set_decoder_persist 0)";
    if (why == DEC_WHY_CUS) return "the device exposes " + std::to_string(m->cu_count) + " compute units (a partition of an MI355X, or another part): the whole-chip kernels need 256";
    return why == DEC_WHY_ROWS ? std::to_string(rows) + " rows > 64 per launch" : "";
  };
  auto dec_why = [&](const DecPlan& dp) -> std::string {
    switch (dp.why) {
      case DEC_WHY_WIDTHS: return "widths outside the presets (256-wide decoder cells and memory, attention_size 128 / 256 / 512, prenet 256-128[-64], 2 decoder layers, r * num_mels <= 512)";
      case DEC_WHY_TEACHER_ROWS: return "teacher frames on an inference model outside the reference widths (attention_size 256, prenet 256-128, num_mels <= 128)";
      case DEC_WHY_NO_INSTANTIATION: return "attention_size 512 with more than 32 rows (no instantiation at 8 rows per group)";
      case DEC_WHY_LDS: return "T_in = " + std::to_string(T_in) + " does not fit a member's LDS at " + std::to_string(dp.rg) + " rows per group";
      case DEC_WHY_TAPE_LAYOUT: return "a tape of " + std::to_string(B) + " rows x " + std::to_string(n) + " steps at num_mels " + std::to_string(m->hp.num_mels) + " is outside the kernel's layout (num_mels <= 128, 20 x rows x steps x 256 < 2^31)";
      default: return why_common(dp.why, B);
    }
  };
  {  // decoder loop
    const DecPlan dp = decoder_plan(m, B, T_in, n, m->tp ? DEC_TRAIN_FWD : (flags & 2) ? DEC_TEACHER : DEC_INFER);
    if (dp.persistent)
      s += "decoder loop: persistent k_decoder_xcd<" + std::to_string(dp.rg) + (dx_reference_widths(m) ? std::string("") : ", attention " + std::to_string(dp.aw) + ", " +
           std::to_string(dp.pd) + " prenet layers") + "> (" + std::string((flags & 1) ? "manual alignments" : "computed alignments") + ", " +
           std::string(m->dx_mode == 2 ? "write-through exchanges forced" : "XCD-local exchanges when the census finds 32 workgroups per XCD") + ")";
    else s += "decoder loop: one launch per stage -- " + dec_why(dp);
  }
  // the two scans, from the plan bigru_scan itself follows
  auto scan_why = [&](const Cbhg& c, const ScanPlan& sp, const char* width_name, int rows) -> std::string {
    switch (sp.why_not_whole_chip) {
      case SCAN_WHY_MODE: return "taco_debug_set_persistent(" + std::to_string(m->persist) + "): " + scan_kernel_name(sp.kernel);
      case SCAN_WHY_WIDTH: return std::string(width_name) + " " + std::to_string(c.rnn) + " != 256";
      case SCAN_WHY_FRAMES: return "fewer than 2 frames";
      default: return why_common(sp.why_not_whole_chip, rows);
    }
  };
  {  // post-net scan
    const Cbhg& c = m->post;
    const ScanPlan sp = scan_plan(m, c, B, T_mel, m->tp != nullptr);
    if (sp.kernel == SCAN_K_OCT) s += "; post-net scan: persistent k_bigru_oct<" + std::to_string(sp.upw) + "> (one row per cluster of " + std::to_string(DX_GROUP / sp.upw) + " CUs)";
    else if (sp.kernel == SCAN_K_DUO) s += "; post-net scan: persistent k_bigru_duo<" + std::to_string(sp.rg) + ">";
    else if (sp.kernel == SCAN_K_QUAD) s += "; post-net scan: k_bigru_quad (post_rnn_size 128: a row and direction per workgroup, its weights resident, no exchange between workgroups)";
    else s += "; post-net scan: resident per-row kernels -- " + scan_why(c, sp, "post_rnn_size", B);
  }
  {  // encoder scan
    const Cbhg& c = m->enc;
    const ScanPlan sp = scan_plan(m, c, B, T_in, m->tp != nullptr);
    if (sp.kernel == SCAN_K_OCT) s += "; encoder scan: persistent k_bigru_oct<" + std::to_string(sp.upw) + ">";
    else if (sp.kernel == SCAN_K_DUO) s += "; encoder scan: persistent k_bigru_duo<" + std::to_string(sp.rg) + ">";
    else if (sp.kernel == SCAN_K_QUAD) s += "; encoder scan: k_bigru_quad (a row and direction per workgroup, K split inside a quad of lanes)";
    else if (sp.kernel == SCAN_K_RES || sp.kernel == SCAN_K_RESW) s += std::string("; encoder scan: ") + scan_kernel_name(sp.kernel) + " (rows resident per workgroup)";
    else s += std::string("; encoder scan: ") + scan_kernel_name(sp.kernel);
    s += "; feed-forward: ";
  }
  // the feed-forward launches, from the plans cbhg_ff, forward_pass and run_gemm themselves follow (ff_plan, prenet_chain_why, head_sweep_why);
  // a training forward (taco_train.h) runs every layer as a launch of its own, between its BatchNorm passes
  auto gemm_name = [](GemmLevel lv) { return lv == GEMM_BF3 ? "k_gemm_bf3" : lv == GEMM_BF3X6 ? "k_gemm_bf3<..., X6>" : "k_gemm"; };
  auto launches = [](int k) { return std::to_string(k) + (k == 1 ? " launch" : " launches"); };
  auto ff_why = [&](const char* kernel, FfWhyNot why, int bit, const char* widths = "widths outside the presets") -> std::string {
    static const char* const words[] = {"", "exact fp32 is switched on", "the six-product level has no fused kernels", "taco_debug_force_gemm_config", "a k_gemm_bf3 tile is forced"};
    return std::string(" -- no ") + kernel + ": " + (why == FF_WHY_SWITCH ? "taco_debug_set_bf3 bit " + std::to_string(bit) : why == FF_WHY_WIDTHS ? std::string(widths) : std::string(words[why]));
  };
  auto cbhg_words = [&](const char* name, const Cbhg& c) -> std::string {
    const FfPlan fp = ff_plan(m, c);
    const int per_layer = 1 + (int)c.proj.size() + (c.has_dense ? 1 : 0) + c.depth + 1;
    std::string r = std::string("; ") + name + " CBHG: ";
    if (m->tp) return r + launches(per_layer) + " of " + gemm_name(fp.level) + ", one per layer";
    r += launches(fp.launches) + ": ";
    r += fp.front_kind == 1 ? "k_cbhg_front<2, 80, 80, 8>" : fp.front_kind ? "k_cbhg_front<1, 144, 128, 16>" : std::string("conv bank and proj_1 on ") + gemm_name(fp.level);
    if (fp.front_kind && !fp.entry) r += " + k_front_combine";
    if (const int np = (int)c.proj.size() - (fp.entry ? 2 : 1)) r += ", " + std::to_string(np) + (np == 1 ? " projection on " : " projections on ") + gemm_name(fp.level);
    if (fp.chain_w) r += ", k_pointwise_chain<" + std::to_string(fp.chain_w) + ">" + (fp.entry ? " (the last projection in its entry)" : "");
    else r += ", " + std::to_string(fp.launches - 1 - (int)c.proj.size()) + " point-wise layers on " + gemm_name(fp.level);
    if (fp.why_front) r += ff_why("k_cbhg_front", fp.why_front, 3);
    if (fp.why_chain) r += ff_why("k_pointwise_chain", fp.why_chain, 2);
    if (fp.why_entry && fp.why_entry != FF_WHY_NEEDS_BOTH) r += ff_why("fused chain entry", fp.why_entry, 4);
    return r;
  };
  { const GemmLevel lv = gemm_level(m, m->linear);
    s += lv == GEMM_BF3 ? "split-bf16 MFMA, three products (k_gemm_bf3 and the fused kernels)" : lv == GEMM_BF3X6 ? "split-bf16 MFMA, six products (k_gemm_bf3<..., X6>: fp32-grade)" : "exact-fp32 MFMA (k_gemm)";
    s += cbhg_words("encoder", m->enc) + cbhg_words("post-net", m->post);
    const FfWhyNot pw = prenet_chain_why(m);
    if (!m->tp && !pw) s += "; encoder prenet: one k_pointwise_chain launch (1 launch: embedding rows gathered, both layers; the forward's zero fills ride in it)";
    else s += "; encoder prenet: one GEMM launch per layer (" + launches(m->hp.enc_prenet_n) + " of " + gemm_name(gemm_level(m, m->enc_prenet[0])) +
              (m->tp ? ")" : std::string(" + 1 launch of k_zero_fill in front: the forward's zero fills") + ff_why("k_pointwise_chain", pw, 2) + ")");
    GemmCall g; g.ldx = 2 * m->hp.post_rnn_size; g.M = B * T_mel; g.ldo = m->hp.num_freq;      // the call of postnet_forward (and of the training forward)
    const FfWhyNot hw = head_sweep_why(m, m->linear, 1, false, g);
    s += std::string("; linear head: 1 launch of ") + (hw ? gemm_name(lv) + ff_why("k_head_sweep", hw, 5, "it serves 256 rows and more, 256 or 512 inputs, 512 columns and more") :
                                                                m->linear.cin == 512 ? "k_head_sweep<512>" : "k_head_sweep<256>"); }
  if (m->tp) {        // the training step's backward scans (taco_train.h: cbhg_backward)
    const Cbhg& c = m->post;
    const ScanBwd bwd = scan_plan(m, c, B, T_mel).bwd;
    s += std::string("; backward scans: post-net ") + (bwd == SCAN_BWD_OCT ? "k_bigru_oct_bwd (one row per cluster of 8 CUs)" : bwd == SCAN_BWD_DUO ? "k_bigru_duo_bwd" : "k_bigru_rows_bwd") +
         ", encoder " + (m->enc.rnn == 128 ? "k_bigru_resb (recurrent kernels in registers)" : "k_bigru_rows_bwd");
    const DecPlan bp = decoder_plan(m, B, T_in, n, DEC_TRAIN_BWD);      // (taco_train_set_bptt_engine(t, 0) switches it off per trainer)
    s += "; decoder backward loop: " + (bp.persistent ? "persistent k_decoder_bwd_xcd<" + std::to_string(bp.rg) + ">" : "one launch per stage -- " + dec_why(bp));
  }
  snprintf(out, (size_t)out_len, "%s", s.c_str());
  return 0;
}
int taco_debug_decoder_trace(taco_model* m, int enable, long long* out) {
  if (!m || !m->finalized) return fail(TACO_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(m->device));
  const size_t half = (size_t)DX_TRACE_STEPS * DX_TRACE_SLOTS * sizeof(long long);
  if ((enable & 1) && !m->d_trace) { HIPCHK(hipMalloc((void**)&m->d_trace, 3 * half)); HIPCHK(hipMemset(m->d_trace, 0, 3 * half)); }
  // enable bit 1 selects the scan's third of the buffer for the read-back, bit 2 the persistent BPTT's
  if (out && m->d_trace) HIPCHK(hipMemcpy(out, (const char*)m->d_trace + ((enable & 4) ? 2 * half : (enable & 2) ? half : 0), half, hipMemcpyDeviceToHost));
  m->trace_on = enable & 1;      // the buffer itself stays until taco_model_destroy: a captured plan may still carry its address
  return 0;
}

int taco_debug_set_front(taco_model* m, int delay_clocks, int prio) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  m->front_delay = delay_clocks; m->front_prio = prio;     // k_cbhg_front: start delay and s_setprio level of the second K half (tools/time_front.py)
  return 0;
}
int taco_debug_set_chip_turns(int on) { g_chip_turns = on ? 1 : 0; return 0; }
int taco_debug_set_skip_scans(taco_model* m, int on) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  m->skip_scans = on ? 1 : 0;
  return 0;
}

int taco_debug_force_gemm_config(taco_model* m, int cfg) {
  if (!m) return fail(TACO_ERR_ARG, "null model");
  if (!gemm_cfg_known(cfg)) return fail(TACO_ERR_ARG, "cfg is not one of -1, 1, 2");
  m->force_cfg = cfg;
  return 0;
}

size_t taco_workspace_bytes(const taco_model* m, int B, int T_in, int n_steps) {
  if (!m || B <= 0) return 0;
  Carver cv(nullptr, 0);
  FullWs w;
  carve_forward(cv, m, forward_passes(m, B), T_in, n_steps, w);      // (more than one pass: the workspace of ONE pass + the passes' stop words)
  return cv.off;
}

size_t taco_stage_workspace_bytes(const taco_model* m, int B, int T) {
  if (!m) return 0;
  // large enough for any single stage at (B, T): encoder at T_in=T, decoder with T_in=T and n_steps=T, post-net at T_mel=T -- each from the pass
  // plan its entry follows; the decoder from the plain plan and from the state dump's (one pass of up to 64 rows), whichever is larger
  Carver a(nullptr, 0), b(nullptr, 0), bd(nullptr, 0), c(nullptr, 0);
  const PassPlan pp = pass_plan(B), dec = pass_plan(B, decoder_pass_rows(m)), dump = pass_plan(B, decoder_pass_rows(m, true));
  EncWs e; carve_enc(a, m, pp.rows, T, e);
  DecWs d; carve_dec(b, m, dec.rows, T, T, d); carve_dec(bd, m, dump.rows, T, T, d);
  PostWs p; carve_post(c, m, pp.rows, T, p);
  Carver all(nullptr, 0);
  all.off = std::max(std::max(a.off, c.off), std::max(b.off, bd.off));
  carve_pass_stops(all, dec);      // (no plan has more passes than the plain decoder's)
  return all.off;
}

int taco_forward_infer(taco_model* m, void* hip_stream, const int32_t* d_inputs, const int32_t* d_input_lengths,
                       const int32_t* d_speaker_id, int B, int T_in, int n_steps, const float* d_manual_alignments,
                       float* d_mel, float* d_linear, float* d_alignments, int32_t* d_stop_step, void* d_workspace,
                       size_t workspace_bytes) {
  if (m) HIPCHK(hipSetDevice(m->device));
  return forward_enqueue(m, (hipStream_t)hip_stream, d_inputs, d_input_lengths, spk_ids(d_speaker_id), B, T_in, n_steps,
                         d_manual_alignments, d_mel, d_linear, d_alignments, d_stop_step, d_workspace, workspace_bytes);
}
int taco_forward_infer_mix(taco_model* m, void* hip_stream, const int32_t* d_inputs, const int32_t* d_input_lengths,
                           const float* d_speaker_weights, int B, int T_in, int n_steps, const float* d_manual_alignments,
                           float* d_mel, float* d_linear, float* d_alignments, int32_t* d_stop_step, void* d_workspace,
                           size_t workspace_bytes) {
  TRY(spk_mix_check(m, d_speaker_weights));
  HIPCHK(hipSetDevice(m->device));
  return forward_enqueue(m, (hipStream_t)hip_stream, d_inputs, d_input_lengths, spk_mix(d_speaker_weights), B, T_in, n_steps,
                         d_manual_alignments, d_mel, d_linear, d_alignments, d_stop_step, d_workspace, workspace_bytes);
}

struct taco_plan {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  size_t nodes = 0;
  int device = 0;
  bool whole_chip = false;      // the graph contains a whole-chip persistent kernel: a replay takes the device's turn (ChipTurn)
};

static int plan_create(taco_model* m, const int32_t* d_inputs, const int32_t* d_input_lengths, const SpkSel& sel,
                       int B, int T_in, int n_steps, const float* d_manual_alignments, float* d_mel, float* d_linear,
                       float* d_alignments, int32_t* d_stop_step, void* d_workspace, size_t workspace_bytes, taco_plan** out) {
  if (!m || !out) return fail(TACO_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t cs;
  HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) { (void)hipStreamDestroy(cs); return fail(TACO_ERR_HIP, "hipStreamBeginCapture: %s", hipGetErrorString(e)); }
  g_captured_whole_chip = false;
  int rc = forward_enqueue(m, cs, d_inputs, d_input_lengths, sel, B, T_in, n_steps, d_manual_alignments, d_mel,
                           d_linear, d_alignments, d_stop_step, d_workspace, workspace_bytes);
  const bool whole_chip = g_captured_whole_chip;
  hipGraph_t g = nullptr;
  e = hipStreamEndCapture(cs, &g);
  (void)hipStreamDestroy(cs);
  if (rc != 0) { if (g) (void)hipGraphDestroy(g); return rc; }
  if (e != hipSuccess) return fail(TACO_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
  taco_plan* p = new taco_plan();
  p->graph = g; p->device = m->device; p->whole_chip = whole_chip;
  e = hipGraphInstantiate(&p->exec, g, nullptr, nullptr, 0);
  if (e != hipSuccess) { (void)hipGraphDestroy(g); delete p; return fail(TACO_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
  (void)hipGraphGetNodes(g, nullptr, &p->nodes);
  *out = p;
  return 0;
}
int taco_plan_create(taco_model* m, const int32_t* d_inputs, const int32_t* d_input_lengths, const int32_t* d_speaker_id,
                     int B, int T_in, int n_steps, const float* d_manual_alignments, float* d_mel, float* d_linear,
                     float* d_alignments, int32_t* d_stop_step, void* d_workspace, size_t workspace_bytes, taco_plan** out) {
  return plan_create(m, d_inputs, d_input_lengths, spk_ids(d_speaker_id), B, T_in, n_steps, d_manual_alignments, d_mel, d_linear, d_alignments,
                     d_stop_step, d_workspace, workspace_bytes, out);
}
// the weights buffer is baked in like every other pointer and read on every replay: the caller changes voices by writing it
int taco_plan_create_mix(taco_model* m, const int32_t* d_inputs, const int32_t* d_input_lengths, const float* d_speaker_weights,
                         int B, int T_in, int n_steps, const float* d_manual_alignments, float* d_mel, float* d_linear,
                         float* d_alignments, int32_t* d_stop_step, void* d_workspace, size_t workspace_bytes, taco_plan** out) {
  TRY(spk_mix_check(m, d_speaker_weights));
  return plan_create(m, d_inputs, d_input_lengths, spk_mix(d_speaker_weights), B, T_in, n_steps, d_manual_alignments, d_mel, d_linear, d_alignments,
                     d_stop_step, d_workspace, workspace_bytes, out);
}

int taco_plan_launch(taco_plan* p, void* hip_stream) {
  if (!p || !p->exec) return fail(TACO_ERR_ARG, "null plan");
  if (p->whole_chip) {
    ChipTurn turn(p->device, (hipStream_t)hip_stream);
    HIPCHK(hipGraphLaunch(p->exec, (hipStream_t)hip_stream));
    return 0;
  }
  HIPCHK(hipGraphLaunch(p->exec, (hipStream_t)hip_stream));
  return 0;
}
int taco_plan_num_nodes(const taco_plan* p) { return p ? (int)p->nodes : 0; }
int taco_plan_whole_chip(const taco_plan* p) { return (p && p->whole_chip) ? 1 : 0; }
void taco_plan_destroy(taco_plan* p) {
  if (!p) return;
  if (p->exec) (void)hipGraphExecDestroy(p->exec);
  if (p->graph) (void)hipGraphDestroy(p->graph);
  delete p;
}

static int encoder_entry(taco_model* m, void* hip_stream, const int32_t* d_inputs, const int32_t* d_input_lengths,
                         const SpkSel& sel, int B, int T_in, float* d_encoder_out, void* d_workspace,
                         size_t workspace_bytes) {
  TRY(check_model_shape(m, B, T_in));
  if (!d_inputs || !d_input_lengths || !d_encoder_out || !d_workspace) return fail(TACO_ERR_ARG, "null buffer");
  if (m->hp.num_speakers > 1 && !sel.given()) return fail(TACO_ERR_ARG, "speaker_id required for a multi-speaker model");
  HIPCHK(hipSetDevice(m->device));
  const PassPlan pp = pass_plan(B);
  Carver cv(d_workspace, workspace_bytes);
  EncWs w; carve_enc(cv, m, pp.rows, T_in, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes", cv.off);
  const bool chain = prenet_chain_why(m) == FF_WHY_NONE;
  return for_each_pass(pp, B, [&](int b0, int rows, int) {
    return encoder_forward(m, (hipStream_t)hip_stream, d_inputs + (size_t)b0 * T_in, d_input_lengths + b0, sel.rows_from(b0, m->hp.num_speakers), rows, T_in,
                           d_encoder_out + (size_t)b0 * T_in * 2 * m->hp.enc_rnn_size, w, false, chain);
  });
}
int taco_encoder_forward(taco_model* m, void* hip_stream, const int32_t* d_inputs, const int32_t* d_input_lengths,
                         const int32_t* d_speaker_id, int B, int T_in, float* d_encoder_out, void* d_workspace,
                         size_t workspace_bytes) {
  return encoder_entry(m, hip_stream, d_inputs, d_input_lengths, spk_ids(d_speaker_id), B, T_in, d_encoder_out, d_workspace, workspace_bytes);
}
int taco_encoder_forward_mix(taco_model* m, void* hip_stream, const int32_t* d_inputs, const int32_t* d_input_lengths,
                             const float* d_speaker_weights, int B, int T_in, float* d_encoder_out, void* d_workspace,
                             size_t workspace_bytes) {
  TRY(spk_mix_check(m, d_speaker_weights));
  return encoder_entry(m, hip_stream, d_inputs, d_input_lengths, spk_mix(d_speaker_weights), B, T_in, d_encoder_out, d_workspace, workspace_bytes);
}

static int decoder_entry(taco_model* m, void* hip_stream, const float* d_encoder_out, const SpkSel& sel, int B,
                         int T_in, int n_steps, const float* d_manual_alignments, const float* d_teacher_frames,
                         float* d_mel, float* d_alignments, int32_t* d_stop_step, float* d_dbg_states, void* d_workspace,
                         size_t workspace_bytes) {
  TRY(check_model_shape(m, B, T_in));
  if (n_steps <= 0 || !d_encoder_out || !d_mel || !d_alignments || !d_workspace) return fail(TACO_ERR_ARG, "bad argument");
  if (m->hp.num_speakers > 1 && !sel.given()) return fail(TACO_ERR_ARG, "speaker_id required for a multi-speaker model");
  const PassPlan pp = pass_plan(B, decoder_pass_rows(m, d_dbg_states != nullptr));      // passes of at most 64 (32) rows
  if (pp.passes > 1 && d_dbg_states) return fail(TACO_ERR_UNSUPPORTED, "the per-step state dump is laid out [step][row]: at most 64 rows per call");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)hip_stream;
  Carver cv(d_workspace, workspace_bytes);
  DecWs w; carve_dec(cv, m, pp.rows, T_in, n_steps, w);
  int32_t* pstop = carve_pass_stops(cv, pp);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes", cv.off);
  const size_t rM = (size_t)m->hp.reduction_factor * m->hp.num_mels, D = (size_t)2 * m->hp.enc_rnn_size;
  TRY(for_each_pass(pp, B, [&](int b0, int rows, int p) {
    return decoder_forward(m, st, d_encoder_out + (size_t)b0 * T_in * D, sel.rows_from(b0, m->hp.num_speakers), rows, T_in, n_steps,
                           d_manual_alignments ? d_manual_alignments + (size_t)b0 * n_steps * T_in : nullptr,
                           d_teacher_frames ? d_teacher_frames + (size_t)b0 * n_steps * m->hp.num_mels : nullptr, d_mel + (size_t)b0 * n_steps * rM,
                           d_alignments + (size_t)b0 * T_in * n_steps, !d_stop_step ? nullptr : pstop ? pstop + p : d_stop_step, d_dbg_states, w, false, nullptr);
  }));
  return combine_pass_stops(st, pstop, pp, d_stop_step);
}
int taco_decoder_forward(taco_model* m, void* hip_stream, const float* d_encoder_out, const int32_t* d_speaker_id, int B,
                         int T_in, int n_steps, const float* d_manual_alignments, const float* d_teacher_frames,
                         float* d_mel, float* d_alignments, int32_t* d_stop_step, float* d_dbg_states, void* d_workspace,
                         size_t workspace_bytes) {
  return decoder_entry(m, hip_stream, d_encoder_out, spk_ids(d_speaker_id), B, T_in, n_steps, d_manual_alignments, d_teacher_frames, d_mel,
                       d_alignments, d_stop_step, d_dbg_states, d_workspace, workspace_bytes);
}
int taco_decoder_forward_mix(taco_model* m, void* hip_stream, const float* d_encoder_out, const float* d_speaker_weights, int B,
                             int T_in, int n_steps, const float* d_manual_alignments, const float* d_teacher_frames,
                             float* d_mel, float* d_alignments, int32_t* d_stop_step, float* d_dbg_states, void* d_workspace,
                             size_t workspace_bytes) {
  TRY(spk_mix_check(m, d_speaker_weights));
  return decoder_entry(m, hip_stream, d_encoder_out, spk_mix(d_speaker_weights), B, T_in, n_steps, d_manual_alignments, d_teacher_frames, d_mel,
                       d_alignments, d_stop_step, d_dbg_states, d_workspace, workspace_bytes);
}

static int postnet_entry(taco_model* m, void* hip_stream, const float* d_mel, const SpkSel& sel, int B, int T_mel,
                         float* d_linear, float* d_post_out, void* d_workspace, size_t workspace_bytes) {
  TRY(check_model_shape(m, B, T_mel));
  if (!d_mel || !d_linear || !d_workspace) return fail(TACO_ERR_ARG, "null buffer");
  HIPCHK(hipSetDevice(m->device));
  const PassPlan pp = pass_plan(B);
  Carver cv(d_workspace, workspace_bytes);
  PostWs w; carve_post(cv, m, pp.rows, T_mel, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes", cv.off);
  return for_each_pass(pp, B, [&](int b0, int rows, int) {
    return postnet_forward(m, (hipStream_t)hip_stream, d_mel + (size_t)b0 * T_mel * m->hp.num_mels, sel.rows_from(b0, m->hp.num_speakers), rows, T_mel,
                           d_linear + (size_t)b0 * T_mel * m->hp.num_freq, d_post_out ? d_post_out + (size_t)b0 * T_mel * 2 * m->hp.post_rnn_size : nullptr, w);
  });
}
int taco_postnet_forward(taco_model* m, void* hip_stream, const float* d_mel, const int32_t* d_speaker_id, int B, int T_mel,
                         float* d_linear, float* d_post_out, void* d_workspace, size_t workspace_bytes) {
  return postnet_entry(m, hip_stream, d_mel, spk_ids(d_speaker_id), B, T_mel, d_linear, d_post_out, d_workspace, workspace_bytes);
}
int taco_postnet_forward_mix(taco_model* m, void* hip_stream, const float* d_mel, const float* d_speaker_weights, int B, int T_mel,
                             float* d_linear, float* d_post_out, void* d_workspace, size_t workspace_bytes) {
  TRY(spk_mix_check(m, d_speaker_weights));
  return postnet_entry(m, hip_stream, d_mel, spk_mix(d_speaker_weights), B, T_mel, d_linear, d_post_out, d_workspace, workspace_bytes);
}

static const ConvL* find_conv(taco_model* m, const char* layer) {
  auto it = m->convs.find(layer ? layer : "");
  return it == m->convs.end() ? nullptr : &it->second;
}

int taco_conv1d_bn_f32(taco_model* m, void* hip_stream, const char* layer, const float* d_x, int B, int T, int act,
                       int maxpool_width, float* d_out) {
  if (!m || !m->finalized) return fail(TACO_ERR_STATE, "model not finalized");
  const ConvL* L = find_conv(m, layer);
  if (!L) return fail(TACO_ERR_ARG, "unknown conv layer '%s'", layer ? layer : "(null)");
  if (!d_x || !d_out || B <= 0 || T <= 0) return fail(TACO_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(m->device));
  GemmCall g; g.x = d_x; g.ldx = L->cin; g.M = B * T; g.T = T; g.act = act; g.mpw = maxpool_width < 1 ? 1 : maxpool_width;
  g.out = d_out; g.ldo = L->N;
  return run_gemm(m, (hipStream_t)hip_stream, L, 1, false, g);
}

int taco_dense_f32(taco_model* m, void* hip_stream, const char* layer, const float* d_x, int rows, int act, float* d_out) {
  if (!m || !m->finalized) return fail(TACO_ERR_STATE, "model not finalized");
  if (!d_x || !d_out || rows <= 0) return fail(TACO_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(m->device));
  auto sk = m->skinny.find(layer ? layer : "");
  if (sk != m->skinny.end()) {
    SkJob j = sk_linear(m, sk->second, d_x, sk->second.K, sk->second.K, nullptr, 0, act, d_out, sk->second.N);
    return run_skinny((hipStream_t)hip_stream, rows, &j, 1);
  }
  const ConvL* L = find_conv(m, layer);
  if (!L || L->kw != 1) return fail(TACO_ERR_ARG, "unknown dense layer '%s'", layer ? layer : "(null)");
  GemmCall g; g.x = d_x; g.ldx = L->cin; g.M = rows; g.act = act; g.out = d_out; g.ldo = L->N;
  return run_gemm(m, (hipStream_t)hip_stream, L, 1, false, g);
}

int taco_highway_f32(taco_model* m, void* hip_stream, const char* layer, const float* d_x, int rows, float* d_out) {
  if (!m || !m->finalized) return fail(TACO_ERR_STATE, "model not finalized");
  const ConvL* L = find_conv(m, layer);
  if (!L || !L->wp2) return fail(TACO_ERR_ARG, "unknown highway layer '%s'", layer ? layer : "(null)");
  if (!d_x || !d_out || rows <= 0 || d_x == d_out) return fail(TACO_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(m->device));
  GemmCall g; g.x = d_x; g.ldx = L->cin; g.M = rows; g.out = d_out; g.ldo = L->N;
  return run_gemm(m, (hipStream_t)hip_stream, L, 1, true, g);
}

int taco_bigru_f32(taco_model* m, void* hip_stream, const char* scope, const float* d_x, const int32_t* d_lengths,
                   const float* d_init_state, int B, int T, float* d_out, void* d_workspace, size_t workspace_bytes) {
  TRY(check_common(m, B, T));
  const std::string sc = scope ? scope : "";
  const Cbhg* c = sc == "encoder_cbhg" ? &m->enc : (sc == "post_cbhg" ? &m->post : nullptr);
  if (!c) return fail(TACO_ERR_ARG, "unknown BiGRU scope '%s'", sc.c_str());
  if (!d_x || !d_out || !d_workspace) return fail(TACO_ERR_ARG, "null buffer");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)hip_stream;
  Carver cv(d_workspace, workspace_bytes);
  CbhgWs w; carve_cbhg(cv, *c, B, T, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes", cv.off);
  { const int H = c->rnn;   // hoisted input projection (backward columns stored time-reversed), then the scan
    GemmCall xp; xp.x = d_x; xp.ldx = H; xp.M = B * T; xp.T = T; xp.out = w.xproj; xp.ldo = 6 * H;
    xp.rev_len = d_lengths; xp.rev_col0 = 3 * H;
    TRY(run_gemm(m, st, &c->xproj, 1, false, xp)); }
  return bigru_scan(m, st, *c, B, T, d_lengths, d_init_state, d_out, w);
}

int taco_attention_step_f32(taco_model* m, void* hip_stream, const float* d_cell_output, const float* d_keys,
                            const float* d_values, const float* d_prev_alignments, int B, int T_in, float* d_alignments,
                            float* d_context, void* d_workspace, size_t workspace_bytes) {
  TRY(check_common(m, B, T_in));
  if (!d_cell_output || !d_keys || !d_values || !d_prev_alignments || !d_alignments || !d_context || !d_workspace)
    return fail(TACO_ERR_ARG, "null buffer");
  if (T_in > ATT_MAXT) return fail(TACO_ERR_UNSUPPORTED, "T_in %d > %d", T_in, ATT_MAXT);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)hip_stream;
  const taco_hparams& hp = m->hp;
  const int A = hp.attention_size, D = 2 * hp.enc_rnn_size, As = hp.attention_state_size;
  Carver cv(d_workspace, workspace_bytes);
  float* q = cv.f((size_t)B * A);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small");
  SkJob j = sk_linear(m, m->query, d_cell_output, As, As, nullptr, 0, ACT_NONE, q, A);
  TRY(run_skinny(st, B, &j, 1));
  if (d_alignments != d_prev_alignments)
    HIPCHK(hipMemcpyAsync(d_alignments, d_prev_alignments, (size_t)B * T_in * sizeof(float), hipMemcpyDeviceToDevice, st));
  AttnArgs a; memset(&a, 0, sizeof a);
  a.q = q; a.keys = d_keys; a.values = d_values; a.v = AP(m, m->att_v); a.battn = AP(m, m->att_b); a.score_bias = AP(m, m->att_sb);
  a.align = d_alignments; a.ctx = d_context; a.ldctx = D; a.T_in = T_in; a.A = A; a.D = D; a.type = hp.attention_type; a.n_steps = 1;
  hipLaunchKernelGGL(k_attention, dim3(B), dim3(64 * ATT_NW), 0, st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

/* One GRUCell step of a decoder GRU by name ("decoder/attention_gru", "decoder/gru_1", ...):
 * d_h [R,H] is updated in place; d_out_res (nullable) = h' + x (ResidualWrapper).  Workspace: 3*R*H floats. */
int taco_gru_cell_f32(taco_model* m, void* hip_stream, const char* name, const float* d_x, float* d_h, int R,
                      float* d_out_res, void* d_workspace, size_t workspace_bytes) {
  if (!m || !m->finalized) return fail(TACO_ERR_STATE, "model not finalized");
  auto it = m->grus.find(name ? name : "");
  if (it == m->grus.end()) return fail(TACO_ERR_ARG, "unknown GRU '%s'", name ? name : "(null)");
  if (!d_x || !d_h || !d_workspace || R <= 0) return fail(TACO_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(m->device));
  const GruDec& g = it->second;
  Carver cv(d_workspace, workspace_bytes);
  float* rh = cv.f((size_t)R * g.H); float* u = cv.f((size_t)R * g.H); float* xc = cv.f((size_t)R * g.H);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small");
  if (d_out_res && g.I != g.H) return fail(TACO_ERR_SHAPE, "residual needs input size == state size");
  return run_gru_cell(m, (hipStream_t)hip_stream, g, R, d_x, g.I, d_h, rh, u, xc, d_out_res);
}

/* add_loss (tacotron.py:274-302) on device tensors.  d_losses[4] = loss, mel_loss, linear_loss, loss_without_coeff.
 * Workspace: 2 * 1024 * 4 doubles. */
int taco_loss_f32(void* hip_stream, const float* d_mel_out, const float* d_mel_tgt, const float* d_lin_out,
                  const float* d_lin_tgt, const float* d_loss_coeff, int B, int T, int num_mels, int num_freq,
                  int prioritize_loss, int sample_rate, float* d_losses, void* d_workspace, size_t workspace_bytes) {
  if (!d_mel_out || !d_mel_tgt || !d_lin_out || !d_lin_tgt || !d_losses || !d_workspace || B <= 0 || T <= 0)
    return fail(TACO_ERR_ARG, "bad argument");
  if (workspace_bytes < (size_t)2 * TR_MAXBLK * 4 * sizeof(double)) return fail(TACO_ERR_STATE, "workspace too small");
  hipStream_t st = (hipStream_t)hip_stream;
  double* pm = (double*)d_workspace; double* pl = pm + (size_t)TR_MAXBLK * 4;
  const int rows = B * T;
  int lo = 0, hi = 0;
  if (prioritize_loss) loss_band(sample_rate, num_freq, &lo, &hi);
  const int nbm = std::min(TR_MAXBLK, cdiv(rows * num_mels, TR_NT * 8)), nbl = std::min(TR_MAXBLK, cdiv(rows * num_freq, TR_NT * 8));
  hipLaunchKernelGGL(k_l1_partial, dim3(nbm), dim3(TR_NT), 0, st, d_mel_out, d_mel_tgt, d_loss_coeff, rows, T, num_mels, 0, 0, pm);
  hipLaunchKernelGGL(k_l1_partial, dim3(nbl), dim3(TR_NT), 0, st, d_lin_out, d_lin_tgt, d_loss_coeff, rows, T, num_freq, lo, hi, pl);
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(TR_NT), 0, st, pm, nbm, pl, nbl, (double)rows * num_mels, (double)rows * num_freq,
                     (double)rows * std::max(hi - lo, 1), prioritize_loss, d_losses);
  HIPCHK(hipGetLastError());
  return 0;
}

/* learning rate of tacotron.py:313-325 for `global_step` (0-based count of completed updates). */
float taco_learning_rate(long long global_step, float initial_learning_rate, int decay_learning_rate_mode, int is_randomly_initialized) {
  const double step = (double)(global_step + 1);
  if (decay_learning_rate_mode == 0) {
    const double w = is_randomly_initialized ? 4000.0 : 40000.0;
    return (float)(initial_learning_rate * std::sqrt(w) * std::min(step * std::pow(w, -1.5), std::pow(step, -0.5)));
  }
  return (float)(initial_learning_rate * std::pow(0.95, step / 3000.0));
}

/* add_optimizer's update (tacotron.py:327-336) on flat buffers of n floats: clip_by_global_norm(clip_norm), then
 * tf.train.AdamOptimizer(lr, beta1, beta2) in TF form.  `global_step` = completed updates so far (Adam's t = +1).
 * d_gnorm_out (nullable) receives the global gradient norm.  Workspace: 1024 doubles. */
int taco_adam_step_f32(void* hip_stream, float* d_params, const float* d_grads, float* d_m, float* d_v, size_t n,
                       long long global_step, float learning_rate, float beta1, float beta2, float epsilon, float clip_norm,
                       float* d_gnorm_out, void* d_workspace, size_t workspace_bytes) {
  if (!d_params || !d_grads || !d_m || !d_v || !d_workspace || n == 0) return fail(TACO_ERR_ARG, "bad argument");
  if (workspace_bytes < (size_t)TR_MAXBLK * sizeof(double)) return fail(TACO_ERR_STATE, "workspace too small");
  if ((reinterpret_cast<uintptr_t>(d_grads) & 15) != 0) return fail(TACO_ERR_ARG, "gradient buffer must be 16-byte aligned");
  hipStream_t st = (hipStream_t)hip_stream;
  double* part = (double*)d_workspace;
  const int nblk = (int)std::min<size_t>(TR_MAXBLK, (n + TR_NT * 16 - 1) / (TR_NT * 16));
  const double t = (double)(global_step + 1);
  const float lr_t = (float)((double)learning_rate * std::sqrt(1.0 - std::pow((double)beta2, t)) / (1.0 - std::pow((double)beta1, t)));
  hipLaunchKernelGGL(k_sumsq_partial, dim3(nblk), dim3(TR_NT), 0, st, d_grads, n, part);
  hipLaunchKernelGGL(k_adam, dim3(std::max(nblk, 1) * 2), dim3(TR_NT), 0, st, d_params, d_grads, d_m, d_v, n, part, nblk, lr_t, beta1,
                     beta2, epsilon, clip_norm, d_gnorm_out);
  HIPCHK(hipGetLastError());
  return 0;
}

#include "taco_train_api.h"
#include "taco_audio_api.h"
#include "taco_resample_api.h"
#include "taco_align_api.h"
#include "taco_dtw_api.h"
#include "taco_f0_api.h"
#include "taco_warp_api.h"
#include "taco_envelope_api.h"

}  // extern "C"
