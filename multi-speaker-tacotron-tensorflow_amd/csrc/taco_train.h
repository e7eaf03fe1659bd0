// taco_train.h -- host side of the training path (included at the end of taco_lib.hip):
//   * taco_train: a "shadow" taco_model whose weight packs are regenerated on the device from ONE flat fp32
//     parameter buffer (index maps built by running the normal packers over index-valued tensors), plus the
//     transposed packs the backward pass needs;
//   * training-mode forward (tacotron.py:26 is_training graph: batch-statistics BatchNorm with moving-average
//     updates, TacoTrainingHelper teacher forcing helpers.py:35-67) that records a tape in the caller's workspace;
//   * the backward pass (tf.gradients of tacotron.py:274-336's loss), gradients accumulated into one flat buffer
//     laid out like the parameters (the single RCCL all-reduce bucket of the data-parallel step).
// modules.py:24 calls tf.layers.dropout without training=True, so the prenet dropout is the identity in the
// reference even when training; nothing is dropped here either.
// Supported for training: single-speaker and multi-speaker ('simple', 'deepvoice') models, attention bah / bah_norm / bah_mon.
#pragma once

struct CbhgT {
  std::vector<ConvL> bank_f, bank_d;   // training-forward (no folded BN) and data-gradient layers, order of Cbhg.bank
  std::vector<ConvL> proj_f, proj_d;
  ConvL dense_d;
  std::vector<ConvL> hw_d;             // [2D -> D]: rows = [W_H^T ; W_T^T]
  ConvL xproj_d;                       // [6H -> I]
  size_t ghT[2] = {0, 0}, chT[2] = {0, 0};   // transposed h-rows of the GRU kernels (raw, arena offsets)
};
struct GruT { SkW gT, cT; int I = 0, H = 0; };   // gates/kernel^T (K = 2H, N = I+H), candidate/kernel^T (K = H, N = I+H)
struct TrainPacks {
  std::vector<ConvL> encpre_d;
  CbhgT enc, post;
  ConvL mem_d, lin_d, frame_d;         // frame_d: [r*num_mels -> Hd], the frame projection's data gradient for all steps at once (persistent BPTT)
  std::vector<SkW> decpre_T;
  SkW decpre0_ctxT;                     // transposed decoder prenet layer 1, context rows only: [P0 -> D] (the teacher frame gets no gradient)
  GruT att, dec[4];
  SkW concat_T, frame_T;
  size_t wqT = 0;
  std::vector<SkW> spk_T;              // deepvoice speaker layers transposed: [dim_i -> S]
  SkW lin_spk_T;                       // 'simple': speaker rows of the linear head transposed [F -> S]
};

struct taco_train {
  taco_model* sm = nullptr;            // shadow model (arena = gather of the flat parameters)
  TrainPacks tp;
  std::map<std::string, size_t> poff;  // flat offset of every spec tensor
  size_t NP = 0, arena_n = 0;
  float* d_map = nullptr;              // index map of the arena
  size_t n_bf3 = 0; int n_bf3_segs = 0; bool want_bf3_planes = false; bool bf3_current = false;   // planes regenerated from the current parameters by the last refresh?
  int wgrad_bf3 = 1, dgrad_bf3 = 0, dgrad_exact = 0;   // engine switches of THIS trainer (taco_train_set_exact_wgrad / _gemm): run_wgrad / run_dgrad read them through the step's TrainCtx
  unsigned* d_bf3_idx = nullptr; Bf3Seg* d_bf3_segs = nullptr;   // index list and segment table of the split-bf16 packs (k_bf3_gather)
  float* d_fold = nullptr;             // [Z + 1, 3H] concat projection folded into decoder GRU 1 (k_dx_fold), the index map's second source
  // synchronised BatchNorm over the data-parallel group: the host sums a device vector in place over all ranks
  // (ordered on the step's stream); null = statistics of this rank's rows only
  void (*sync_fn)(void* user, float* d_vec, int n) = nullptr;
  void* sync_user = nullptr;
  int sync_world = 1;
  int resident_bwd_scan = 1;           // the encoder's backward scan with the recurrent kernels in registers (k_bigru_resb); 0 (with taco_train_set_bptt_engine(t, 0)): k_bigru_rows_bwd
  int bptt_persistent = 1;             // taco_train_set_bptt_engine: the decoder's BPTT as one persistent launch (k_decoder_bwd_xcd) where it fits
  int planes_problems = 0;     // weight gradients of the last backward pass that were computed from pre-split planes (a conv bank counts once)
  int wgrad_planes = 1;                // taco_train_set_wgrad_planes: 1 = large weight gradients from pre-split bf16 planes (taco_wgrad_planes.h), 2 = every eligible one (tests), 0 = off
  int deterministic = 1;               // taco_train_set_deterministic: ordered two-stage sums (default since round 4) or fp32 atomics; the former needs DET_SCRATCH_FLOATS of workspace
  taco_segnorm_plan* gn_plan = nullptr;   // taco_train_grad_norms: one segment per spec tensor (poff order), built on the first call
};
#define WP_SCRATCH_COLS 2048           // plane scratch: room for (widest conv bank + WP_SCRATCH_COLS) columns of the longest row set, three bf16 planes each
#define DET_SCRATCH_FLOATS ((size_t)48 << 20)      // 192 MB: e.g. 30 M-slices of the largest weight gradient (post-net proj_1, 3 x 2048 x 256)

// ---------------------------------------------------------------------------------------------------------------
// backward packs (the last part of model_pack_host on a shadow model, taco_pack.h: host only, before the arena upload)
// ---------------------------------------------------------------------------------------------------------------
static ConvL make_conv_T(taco_model* m, const float* W, int kw, int cin, int N) {
  // data gradient of y[t] = sum_j W[j] x[t + j - padl] is the SAME-padded correlation of dy with
  // WT[j'][n][c] = W[kw-1-j'][c][n] and left padding kw-1-padl
  std::vector<float> WT((size_t)kw * N * cin);
  for (int j = 0; j < kw; ++j)
    for (int c = 0; c < cin; ++c)
      for (int n = 0; n < N; ++n) WT[((size_t)(kw - 1 - j) * N + n) * cin + c] = W[((size_t)j * cin + c) * N + n];
  ConvL L; L.kw = kw; L.cin = N; L.N = cin;
  L.wp = pack_w32(m, WT.data(), kw, N, cin, &L.cin_pad);
  pack_bf3(m, WT.data(), kw, N, cin, &L.bh, &L.bl, &L.K16, &L.cin_pad16);
  add_var(m, L, 0);
  m->hvars[L.var_index].padl = kw - 1 - (kw - 1) / 2;
  return L;
}
static ConvL make_conv_T_named(taco_model* m, const std::string& name) {
  const HostTensor& k = T_(m, name + "/kernel");
  if (k.shape.size() == 3) return make_conv_T(m, k.data.data(), (int)k.shape[0], (int)k.shape[1], (int)k.shape[2]);
  return make_conv_T(m, k.data.data(), 1, (int)k.shape[0], (int)k.shape[1]);
}
static std::vector<float> transpose2d(const float* W, int rows, int cols, int r0 = 0, int nr = -1) {
  if (nr < 0) nr = rows - r0;
  std::vector<float> Tt((size_t)cols * nr);
  for (int r = 0; r < nr; ++r)
    for (int c = 0; c < cols; ++c) Tt[(size_t)c * nr + r] = W[(size_t)(r0 + r) * cols + c];
  return Tt;
}
static SkW pack_w16_T(taco_model* m, const float* W, int rows, int cols) {   // pack of W^T: K = cols, N = rows
  std::vector<float> Tt = transpose2d(W, rows, cols);
  return pack_w16(m, Tt.data(), rows, 0, cols, 0, rows, nullptr);
}
static ConvL conv_noBN(taco_model* m, const ConvL& L, int coff) {
  ConvL F = L; F.bns = F.bnb = 0; F.var_index = -1;      // (the split-bf16 planes are the same weights: kept)
  add_var(m, F, coff);
  return F;
}
static void build_cbhg_T(taco_model* m, const Cbhg& c, const std::string& sc, CbhgT& t) {
  for (size_t i = 0; i < c.bank.size(); ++i) {
    const int k = c.bank[i].kw;
    t.bank_f.push_back(conv_noBN(m, c.bank[i], (k - 1) * c.C));
    t.bank_d.push_back(make_conv_T_named(m, sc + "/conv_bank/conv1d_" + std::to_string(k)));
  }
  for (size_t i = 0; i < c.proj.size(); ++i) {
    t.proj_f.push_back(conv_noBN(m, c.proj[i], 0));
    t.proj_d.push_back(make_conv_T_named(m, sc + "/proj_" + std::to_string(i + 1)));
  }
  if (c.has_dense) t.dense_d = make_conv_T_named(m, sc + "/dense");
  const int D = c.rnn;
  for (int i = 0; i < c.depth; ++i) {
    const std::string n = sc + "/highway_" + std::to_string(i + 1);
    const auto& WH = T_(m, n + "/H/kernel").data; const auto& WT = T_(m, n + "/T/kernel").data;
    std::vector<float> cat((size_t)2 * D * D);          // [2D, D] = [W_H^T ; W_T^T]
    for (int r = 0; r < D; ++r)
      for (int q = 0; q < D; ++q) { cat[(size_t)q * D + r] = WH[(size_t)r * D + q]; cat[(size_t)(D + q) * D + r] = WT[(size_t)r * D + q]; }
    ConvL L; L.kw = 1; L.cin = 2 * D; L.N = D;
    L.wp = pack_w32(m, cat.data(), 1, 2 * D, D, &L.cin_pad);
    pack_bf3(m, cat.data(), 1, 2 * D, D, &L.bh, &L.bl, &L.K16, &L.cin_pad16);
    add_var(m, L, 0);
    t.hw_d.push_back(L);
  }
  const int H = c.rnn, I = c.rnn;
  std::vector<float> WxT((size_t)6 * H * I);              // [6H, I]: transposed hoisted input projection
  for (int dir = 0; dir < 2; ++dir) {
    const GruW w = bigru_w(m, sc, dir);
    const auto &gk = w.gk, &ck = w.ck;
    for (int i = 0; i < I; ++i) {
      for (int j = 0; j < 2 * H; ++j) WxT[(size_t)(dir * 3 * H + j) * I + i] = gk[(size_t)i * 2 * H + j];
      for (int j = 0; j < H; ++j) WxT[(size_t)(dir * 3 * H + 2 * H + j) * I + i] = ck[(size_t)i * H + j];
    }
    std::vector<float> gT = transpose2d(gk.data(), I + H, 2 * H, I, H);   // [2H, H]
    std::vector<float> cT = transpose2d(ck.data(), I + H, H, I, H);       // [H, H]
    t.ghT[dir] = arena_put(m, gT.data(), gT.size());
    t.chT[dir] = arena_put(m, cT.data(), cT.size());
  }
  ConvL X; X.kw = 1; X.cin = 6 * H; X.N = I;
  X.wp = pack_w32(m, WxT.data(), 1, 6 * H, I, &X.cin_pad);
  pack_bf3(m, WxT.data(), 1, 6 * H, I, &X.bh, &X.bl, &X.K16, &X.cin_pad16);
  add_var(m, X, 0);
  t.xproj_d = X;
}
static GruT make_gru_T(taco_model* m, const std::string& name, int I, int H) {
  GruT g; g.I = I; g.H = H;
  g.gT = pack_w16_T(m, T_(m, name + "/gates/kernel").data.data(), I + H, 2 * H);
  g.cT = pack_w16_T(m, T_(m, name + "/candidate/kernel").data.data(), I + H, H);
  return g;
}
static int build_train_packs(taco_model* m) {
  TrainPacks& tp = *m->tp;
  const taco_hparams& hp = m->hp;
  for (int i = 0; i < hp.enc_prenet_n; ++i) tp.encpre_d.push_back(make_conv_T_named(m, "prenet/dense_" + std::to_string(i + 1)));
  build_cbhg_T(m, m->enc, "encoder_cbhg", tp.enc);
  build_cbhg_T(m, m->post, "post_cbhg", tp.post);
  tp.mem_d = make_conv_T_named(m, "attention/memory_layer");
  tp.lin_d = make_conv_T_named(m, "linear");
  const int D = 2 * hp.enc_rnn_size, As = hp.attention_state_size, Hd = hp.dec_rnn_size, A = hp.attention_size;
  int d = hp.num_mels + D;
  for (int i = 0; i < hp.dec_prenet_n; ++i) {
    tp.decpre_T.push_back(pack_w16_T(m, T_(m, "decoder/prenet/dense_" + std::to_string(i + 1) + "/kernel").data.data(), d, hp.dec_prenet[i]));
    d = hp.dec_prenet[i];
  }
  { const HostTensor& k = T_(m, "decoder/prenet/dense_1/kernel");      // [Mm + D, P0]: rows Mm.. transposed -> [P0, D]
    const int Mm = hp.num_mels, P0 = hp.dec_prenet[0];
    std::vector<float> Tt = transpose2d(k.data.data(), Mm + D, P0, Mm, D);
    tp.decpre0_ctxT = pack_w16(m, Tt.data(), D, 0, P0, 0, D, nullptr); }
  tp.att = make_gru_T(m, "decoder/attention_gru", d + simple_S(m), As);
  for (int i = 0; i < hp.dec_layer_num; ++i) tp.dec[i] = make_gru_T(m, "decoder/gru_" + std::to_string(i + 1), Hd, Hd);
  tp.concat_T = pack_w16_T(m, T_(m, "decoder/concat_projection/kernel").data.data(), As + D + simple_S(m), Hd);
  if (is_simple(m)) tp.lin_spk_T = pack_w16_T(m, T_(m, "linear/kernel_spk").data.data(), hp.speaker_embedding_size, hp.num_freq);
  tp.frame_d = make_conv_T_named(m, "decoder/frame_projection");
  tp.frame_T = pack_w16_T(m, T_(m, "decoder/frame_projection/kernel").data.data(), Hd, hp.num_mels * hp.reduction_factor);
  { std::vector<float> wqT = transpose2d(T_(m, "attention/query_layer/kernel").data.data(), As, A);
    tp.wqT = arena_put(m, wqT.data(), wqT.size()); }
  if (is_deepvoice(m) && hp.speaker_embedding_size != 1) {
    for (auto& n : spk_vector_names(hp)) {
      const HostTensor& k = T_(m, "spk/" + n + "/kernel");
      tp.spk_T.push_back(pack_w16_T(m, k.data.data(), (int)k.shape[0], (int)k.shape[1]));
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------------------------------------------
#define EWGRID(n) dim3((unsigned)(((size_t)(n) + 255) / 256)), dim3(256)
static inline bool al16h(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }      // may a matrix be read four columns at a time (the _v4 kernels)
// Batching region for small weight gradients (k_wgrad_bf3_group): while a WgRegion is open, run_wgrad calls that take the one-wave
// tile are collected and launched together -- at wg_flush / the region's end, or when the table is full.  The caller flushes before
// anything overwrites an operand of a collected problem or reads one of their outputs.
// Deterministic mode: the collected problems write per-slice partials into consecutive regions of the deterministic scratch (det_used: the
// cursor; a problem that does not fit flushes the region first) and two more group launches add the slices up in a fixed order.  (Problems
// launched on their own in between use the scratch from its start: everything is stream ordered, the group's kernels run at the flush.)
struct WgBatch { WgGroup g; ColGroup c; WgRedGroup r; ColRedGroup cr; size_t det_used = 0; bool active = false; };
// The mutable state of the step in flight: one object on the stack of train_forward_backward, reached through TrainCtx::s.
// det: deterministic reductions (taco_train_set_deterministic) -- the sums over rows that normally leave their workgroups through fp32
// atomics (weight gradients, bias / BatchNorm sums, embedding gradients, d attention_v) are written as per-slice partials into this
// scratch and added up in a fixed order by a second launch: the step becomes run-to-run reproducible, as the reference's
// single-device step is.  Null: atomics.
struct StepState {
  float* det = nullptr; size_t det_cap = 0;
  uint4* wps = nullptr; size_t wps_cap = 0;      // bf16 planes of the weight gradients' operands (taco_wgrad_planes.h); null: that path is off
  int planes_problems = 0;                       // weight gradients of this step that were computed from pre-split planes so far
  unsigned paths = 0;                            // CBHG_PATH_* bits: which branch each dispatch of a CBHG took, OR-ed in where it is taken (taco_train_debug_cbhg)
  unsigned dec_paths = 0;                        // DEC_PATH_* bits: which engine ran the decoder loop and its BPTT, OR-ed in where each is launched (taco_train_debug_decoder)
  unsigned end_paths = 0;                        // FRONT_PATH_* bits: which embedding-gradient kernel and which speaker backward ran, OR-ed in where each is launched (taco_train_debug_front)
  WgBatch wgb;
};
// The word of taco_train_debug_cbhg (include/taco_debug.h documents the layout): one bit per form of every two-way dispatch of
// cbhg_forward_train / cbhg_backward, and the scan kernels that were launched.  Set at the launch, never recomputed from the predicates.
enum : unsigned {
  CBHG_PATH_BANK_FWD_FUSED = 1u << 0, CBHG_PATH_BANK_FWD_PLAIN = 1u << 1,      // k_bn_pool_bank_v4 | k_bn_apply per width + k_maxpool_fwd
  CBHG_PATH_POOL_BWD_FUSED = 1u << 2, CBHG_PATH_POOL_BWD_PLAIN = 1u << 3,      // k_maxpool_bwd_bn_v4 | k_maxpool_bwd
  CBHG_PATH_PROJ_BN_V4 = 1u << 4, CBHG_PATH_PROJ_BN_PLAIN = 1u << 5,           // k_bn_apply_v4 | k_bn_apply on a projection
  CBHG_PATH_BN_BWD_V4 = 1u << 6, CBHG_PATH_BN_BWD_PLAIN = 1u << 7,             // k_bn_bwd_v4 | k_bn_bwd (projections, and bank widths without the one-launch dz)
  CBHG_PATH_BANK_DZ_ONE = 1u << 8, CBHG_PATH_BANK_DZ_EACH = 1u << 9,           // k_bn_bwd_bank_v4 | dz per width
  CBHG_PATH_BANK_WG_PLANES = 1u << 10, CBHG_PATH_BANK_WG_EACH = 1u << 11,      // run_wgrad_bank_planes | run_wgrad per width
  CBHG_PATH_HW_BWD_V4 = 1u << 12, CBHG_PATH_HW_BWD_PLAIN = 1u << 13,           // k_highway_bwd_v4 | k_highway_bwd
  CBHG_PATH_SCAN_FWD_SHIFT = 16, CBHG_PATH_SCAN_BWD_SHIFT = 20                 // four bits each: ScanKernel of the forward launch; CBHG_SCAN_BWD_* of the backward one
};
enum { CBHG_SCAN_BWD_ROWS = 1, CBHG_SCAN_BWD_RESB = 2, CBHG_SCAN_BWD_DUO = 3, CBHG_SCAN_BWD_OCT = 4 };
// The word of taco_train_debug_decoder (include/taco_debug.h): set where decoder_forward_train / decoder_backward launch, never recomputed from the plan.
// The two protocol bits are the hook's: it reads them back from the census words of the launches (taco_debug_decoder_info's) once they have run.
enum : unsigned {
  DEC_PATH_FWD_PERSISTENT = 1u << 0, DEC_PATH_FWD_STAGES = 1u << 1,            // k_decoder_xcd<RG, true> | one launch per stage
  DEC_PATH_BWD_PERSISTENT = 1u << 2, DEC_PATH_BWD_STAGES = 1u << 3,            // k_decoder_bwd_xcd<RG> | one launch per stage
  DEC_PATH_FWD_RG_SHIFT = 4, DEC_PATH_BWD_RG_SHIFT = 8,                        // four bits each: rows per group (1, 2, 4, 8) of the persistent launch
  DEC_PATH_XCD_LOCAL = 1u << 12, DEC_PATH_WRITE_THROUGH = 1u << 13             // a persistent launch of the call exchanged through XCD-local stores | write-through
};

// The word of taco_train_debug_front (include/taco_debug.h): set where run_embed_bwd / front_backward launch.
enum : unsigned {
  FRONT_PATH_EMBED_DET = 1u << 0, FRONT_PATH_EMBED_ATOMIC = 1u << 1,           // k_embed_bwd_det | k_embed_bwd
  FRONT_PATH_SPK_TABLES = 1u << 2, FRONT_PATH_SPK_DENSE = 1u << 3              // deepvoice speaker backward: tables (S = 1) | softsign + dense layers
};

struct TrainCtx {
  const taco_train* t; hipStream_t st; float* P; float* G;    // flat parameters (moving statistics are updated in place) and gradients
  bool update_moving;   // BatchNorm moving averages follow this pass (UPDATE_OPS run only as a dependency of `optimize`, tacotron.py:334)
  StepState* s;
  float* p(const std::string& n) const { return P + t->poff.at(n); }
  float* g(const std::string& n) const { return G + t->poff.at(n); }
};
static void wg_reset(WgBatch& b) { b.g.n = 0; b.g.start[0] = 0; b.c.n = 0; b.c.start[0] = 0; b.r.n = 0; b.r.start[0] = 0; b.cr.n = 0; b.cr.start[0] = 0; b.det_used = 0; }
static int wg_flush(const TrainCtx& x) {      // (column sums of the region ride along: same hazards, same flush points)
  WgBatch& b = x.s->wgb;
  if (b.c.n > 0) hipLaunchKernelGGL(k_colsum_group, dim3(b.c.start[b.c.n]), dim3(256), 0, x.st, b.c);
  if (b.g.n > 0) hipLaunchKernelGGL(k_wgrad_bf3_group, dim3(b.g.start[b.g.n]), dim3(64), 0, x.st, b.g);
  if (b.cr.n > 0) hipLaunchKernelGGL(k_colsum_reduce_group, dim3(b.cr.start[b.cr.n]), dim3(256), 0, x.st, b.cr);
  if (b.r.n > 0) hipLaunchKernelGGL(k_wgrad_reduce_group, dim3(b.r.start[b.r.n]), dim3(256), 0, x.st, b.r);
  if (b.c.n > 0 || b.g.n > 0) HIPCHK(hipGetLastError());
  wg_reset(b);
  return 0;
}
struct WgRegion {      // RAII: a region ends (and flushes) on every return path; end() for the caller that must see the flush's status
  const TrainCtx& x;
  explicit WgRegion(const TrainCtx& x_) : x(x_) { wg_reset(x.s->wgb); x.s->wgb.active = true; }
  int end() { const int rc = wg_flush(x); x.s->wgb.active = false; return rc; }
  ~WgRegion() { if (x.s->wgb.active) (void)end(); }
};
// A problem joins the region's group launch in deterministic mode: `need` floats of the scratch at the cursor for its partials, summed by the
// group's reduce launch.  Two problems of one reduce launch must not add into the same output: their read-modify-writes would race, where
// the atomics of the other mode simply accumulate (e.g. the five speaker projections of model type deepvoice sum into one embedding
// gradient) -- so a problem whose output (o1, o2; nullable) is already written by the region, or that does not fit, flushes the region first.
static int wg_reserve(const TrainCtx& x, const float* o1, const float* o2, size_t need, float** part) {
  WgBatch& b = x.s->wgb;
  bool clash = false;
  for (const float* o : {o1, o2}) {
    for (int i = 0; o && i < b.cr.n; ++i) clash = clash || b.cr.p[i].out1 == o || b.cr.p[i].out2 == o;
    for (int i = 0; o && i < b.r.n; ++i) clash = clash || b.r.p[i].dw == o;
  }
  if (clash || b.det_used + need > x.s->det_cap) TRY(wg_flush(x));
  *part = x.s->det + b.det_used; b.det_used += need;
  return 0;
}
static int run_colsum(const TrainCtx& x, const float* a, int lda, const float* b, int ldb, const float* mu, const float* rstd,
                      float* out1, float* out2, int M, int C, int mode, bool assign = false) {
  // assign (deterministic mode only -- the caller zero-fills otherwise): the ordered sums replace out1 / out2 instead of being added to them
  ColArgs g; g.a = a; g.b = b; g.mu = mu; g.rstd = rstd; g.out1 = out1; g.out2 = out2; g.lda = lda; g.ldb = ldb; g.M = M; g.C = C;
  g.mode = mode; g.rpb = 256; g.part = nullptr;
  if (x.s->det) {
    while ((size_t)cdiv(M, g.rpb) * 2 * C > x.s->det_cap) g.rpb *= 2;
    g.part = x.s->det;
  }
  const int nchunks = cdiv(M, g.rpb);
  if (x.s->wgb.active) {      // inside a batching region: joins the group launch (the caller flushes before the sums are read)
    if (g.part) {
      TRY(wg_reserve(x, out1, out2, (size_t)nchunks * 2 * C, &g.part));
      ColRedGroup& R = x.s->wgb.cr;
      R.p[R.n].part = g.part; R.p[R.n].out1 = out1; R.p[R.n].out2 = out2; R.p[R.n].nchunks = nchunks; R.p[R.n].C = C; R.p[R.n].mode = mode | (assign ? 8 : 0);
      R.start[R.n + 1] = R.start[R.n] + cdiv(C, 256); ++R.n;
    }
    ColGroup& G = x.s->wgb.c;
    G.p[G.n] = g;
    G.start[G.n + 1] = G.start[G.n] + cdiv(C, 64) * nchunks;
    if (++G.n == COL_MAXP) return wg_flush(x);
    return 0;
  }
  hipLaunchKernelGGL(k_colsum, dim3(cdiv(C, 64), nchunks), dim3(256), 0, x.st, g);
  if (g.part) hipLaunchKernelGGL(k_colsum_reduce, EWGRID(C), 0, x.st, (const float*)g.part, nchunks, C, mode | (assign ? 8 : 0), out1, out2);
  HIPCHK(hipGetLastError());
  return 0;
}
// ---- which kernel a weight gradient gets: wgrad_plan / wgrad_bank_plan decide, run_wgrad / run_wgrad_bank_planes launch what they say ----
// 1 (default): weight gradients on the bf16 matrix cores with operands split three ways and six products per tile (k_wgrad_bf3:
// fp32-grade); 0: exact-fp32 MFMA (k_wgrad).  taco_train_set_exact_wgrad.
// From pre-split planes (taco_wgrad_planes.h): the operands of a LARGE weight gradient are converted once into bf16 planes (k_wp_split:
// fragment-major, the tap shifts and their batch-row masks applied to copies of the narrower operand) and multiplied by a kernel that
// converts nothing (k_wp_gemm).  Measured per problem against k_wgrad_bf3 (tools/ubench_wgrad_planes.hip, profiles/r06_ubench_wgrad_planes.txt):
// the conversion pass is bound by its 10 bytes per element, so it pays where an element meets many products -- post-net proj_1 (542 -> 382 us),
// the linear head (365 -> 208), a whole conv bank as ONE product launch over one conversion of its dz (post-net: ~1240 -> ~330) -- and loses on
// 256 x 256-sized problems (highway, GRU kernels, the decoder's hoisted gradients), which stay on k_wgrad_bf3.
#define WP_MIN_MACS 3.0e9                               // planes mode 1: problems below this many multiply-adds stay on k_wgrad_bf3
constexpr int WP_WK = 2, WP_WN = 2, WP_SM = 1, WP_NB = 3;      // k_wp_gemm: 128 x 128 workgroup tile (2 x 2 waves, 72 KB of LDS, two workgroups per CU), 16-row stages, ring of three
constexpr size_t WP_LDS = (size_t)WP_NB * 3 * 2 * (WP_WK + WP_WN) * WP_SM * 1024;      // (taco_train_create raises the kernel's dynamic-LDS limit to this)
enum { WG_NONE = 0, WG_PLANES, WG_BF3_4W, WG_BF3_1W, WG_BF3_GROUP, WG_EXACT };      // NONE: cannot run (WgPlan::why) / a bank that is not eligible
struct WgEnv {         // everything besides the problem that a plan may depend on
  int bf3, planes;     // the trainer's switches (wgrad_bf3, wgrad_planes)
  bool det; size_t det_cap, wps_cap;      // deterministic scratch present, its floats; plane scratch in uint4 (0: none)
  bool region;         // a batching region is open
};
struct WgPlan {
  int engine = WG_NONE, rpb = 0, nsplit = 0;       // rows per M-slice, slices
  int a_per_tap = 0, Mp = 0; size_t na = 0, nb = 0;      // planes: the x planes carry the tap copies (else dy's), padded rows, uint4 of the two plane sets
  const char* why = nullptr;
};
static WgEnv wg_env(const TrainCtx& x) { return WgEnv{x.t->wgrad_bf3, x.s->wps ? x.t->wgrad_planes : 0, x.s->det != nullptr, x.s->det_cap, x.s->wps_cap, x.s->wgb.active}; }
// slices of a planes product: ~768 workgroups; in deterministic mode the slices' partial tiles (`per` floats each) must fit the scratch
static void wp_slices(const WgEnv& e, long tiles, size_t per, WgPlan& p) {
  int rpb = p.Mp;
  while (rpb > 256 && tiles * cdiv(p.Mp, rpb) < 768) rpb >>= 1;
  rpb = cdiv(rpb, 16 * WP_SM) * 16 * WP_SM;
  if (e.det) while ((size_t)cdiv(p.Mp, rpb) * per > e.det_cap && rpb < p.Mp) rpb *= 2;
  p.rpb = rpb; p.nsplit = cdiv(p.Mp, rpb);
}
// one weight gradient dW [kw][K][N] = sum over M rows (T per batch row; 0: no time axis) of x (shifted by tap - padl) . dy
static WgPlan wgrad_plan(const WgEnv& e, int M, int T, int K, int N, int kw, int padl, bool gather, bool ygather) {
  WgPlan p;
  const size_t per = (size_t)kw * K * N;
  if (e.det && per > e.det_cap) { p.why = "deterministic-reduction scratch too small"; return p; }
  const bool bf3 = e.bf3 != 0, shifted = kw > 1 || padl != 0;
  if (bf3 && !ygather && e.planes && !(e.planes == 1 && (double)M * K * N * kw < WP_MIN_MACS) && !(shifted && (gather || T <= 0))) {
    const int Mp = cdiv(M, 64) * 64;
    const bool a_per_tap = K <= N;            // the narrower operand carries the tap copies
    const size_t na = wp_plane_uint4(K, Mp, a_per_tap ? kw : 1), nb = wp_plane_uint4(N, Mp, a_per_tap ? 1 : kw);
    if (na + nb <= e.wps_cap) {
      p.engine = WG_PLANES; p.a_per_tap = a_per_tap ? 1 : 0; p.Mp = Mp; p.na = na; p.nb = nb;
      wp_slices(e, (long)cdiv(K, 64 * WP_WK) * cdiv(N, 64 * WP_WN) * kw, per, p);
      return p;
    }
  }
  // split-bf16 kernel: 128 x 128 tiles (4 waves) when those alone give a few hundred workgroups, else 64 x 64 tiles (1 wave): every
  // M-slice a workgroup takes ends in one atomic per output element, so slices are kept LONG (>= 256 rows where the grid allows)
  const long t128 = (long)cdiv(K, 128) * cdiv(N, 128) * kw, t64 = (long)cdiv(K, 64) * cdiv(N, 64) * kw;
  const bool big = bf3 && t128 >= 64;
  const long tiles = big ? t128 : t64;
  const long want = bf3 ? (big ? 768 : 1024) : 2048;      // workgroups (one-wave workgroups: four times as many fit a CU).  (Ordered sums: halving or doubling the
                                                           // slices of the small problems changes nothing, 15.87 / 15.88 ms; a quarter of them: 16.14 -- the partials' traffic is not what the mode costs)
  p.rpb = 1024;
  while (p.rpb > (bf3 ? 128 : 64) && tiles * cdiv(M, p.rpb) < want) p.rpb >>= 1;
  if (e.det) while ((size_t)cdiv(M, p.rpb) * per > e.det_cap) p.rpb *= 2;      // fewer, longer slices if the scratch is short
  p.nsplit = cdiv(M, p.rpb);
  p.engine = !bf3 ? WG_EXACT : big ? WG_BF3_4W : e.region ? WG_BF3_GROUP : WG_BF3_1W;      // a small problem inside a batching region joins the group launch
  return p;
}
// ALL widths 1 .. nw of a conv bank as one planes problem (run_wgrad_bank_planes); engine WG_NONE: not eligible, the widths go one by one
static WgPlan wgrad_bank_plan(const WgEnv& e, int M, int T, int K, int Cw, int nw, bool gather) {
  WgPlan p;
  if (!e.bf3 || !e.planes || gather || nw < 2 || nw > WP_MAXW || (Cw & 31) || T <= 0) return p;
  const int ntap = nw * (nw + 1) / 2;
  if (e.planes == 1 && (double)M * K * Cw * ntap < WP_MIN_MACS) return p;
  const int Mp = cdiv(M, 64) * 64;
  const size_t na = wp_plane_uint4(K, Mp, nw), nb = wp_plane_uint4(nw * Cw, Mp, 1), per = (size_t)ntap * K * Cw;
  if (na + nb > e.wps_cap || (e.det && per > e.det_cap)) return p;
  p.engine = WG_PLANES; p.a_per_tap = 1; p.Mp = Mp; p.na = na; p.nb = nb;
  wp_slices(e, (long)cdiv(K, 64 * WP_WK) * cdiv(Cw, 64 * WP_WN) * ntap, per, p);
  return p;
}
static void wp_split_launch(hipStream_t st, const float* src, const int* gather, int ld, int M, int T, int C, int Mp, int ncopy, int sigma0, int dsigma, uint4* out) {
  WpSplitArgs a; a.src = src; a.gather = gather; a.out = out; a.ld = ld; a.M = M; a.T = T; a.C = C; a.Mp = Mp; a.ncopy = ncopy; a.sigma0 = sigma0; a.dsigma = dsigma;
  hipLaunchKernelGGL(k_wp_split, dim3(cdiv(cdiv(C, 32), 4), Mp / 64, ncopy), dim3(256), 0, st, a);
}
static void wp_gemm_launch(hipStream_t st, const WpGemmArgs& g, int z) {
  hipLaunchKernelGGL((k_wp_gemm<WP_WK, WP_WN, WP_SM, WP_NB>), dim3(cdiv(g.K, 64 * WP_WK), cdiv(g.N, 64 * WP_WN), z), dim3(64 * WP_WK * WP_WN), WP_LDS, st, g);
}
// one weight gradient from planes (the arguments of run_wgrad, its plan)
static int run_wgrad_planes(const TrainCtx& x, const WgPlan& p, const float* xs, const int* gather, int ldx, const float* dy, int ldy, float* dw, int lddw,
                            int M, int T, int K, int N, int kw, int padl) {
  const bool shifted = kw > 1 || padl != 0, a_per_tap = p.a_per_tap != 0;
  uint4* pa = x.s->wps; uint4* pb = x.s->wps + p.na;
  // dW[tap] = sum_m X[m + s] dY[m], s = tap - padl: either X carries the shift s, or dY carries -s (m' = m + s)
  wp_split_launch(x.st, xs, gather, ldx, M, T, K, p.Mp, a_per_tap ? kw : 1, (shifted && a_per_tap) ? -padl : 0, a_per_tap ? 1 : 0, pa);
  wp_split_launch(x.st, dy, nullptr, ldy, M, T, N, p.Mp, a_per_tap ? 1 : kw, (shifted && !a_per_tap) ? padl : 0, a_per_tap ? 0 : -1, pb);
  WpGemmArgs g; memset(&g, 0, sizeof g);
  g.a = pa; g.b = pb; g.K = K; g.N = N; g.Mp = p.Mp; g.kw = kw; g.a_per_tap = p.a_per_tap; g.dw = dw; g.lddw = lddw; g.nw = 0;
  g.rpb = p.rpb; g.part = x.s->det;
  wp_gemm_launch(x.st, g, kw * p.nsplit);
  if (g.part) hipLaunchKernelGGL(k_wgrad_reduce, EWGRID((size_t)kw * K * N), 0, x.st, (const float*)g.part, p.nsplit, kw, K, N, dw, lddw);
  HIPCHK(hipGetLastError());
  ++x.s->planes_problems;
  return 0;
}
// ALL widths 1 .. nw of a conv bank (dz of every width complete in dY [M, nw * Cw]; p: their wgrad_bank_plan): one conversion of dz, nw shifted copies
// of the bank's input, one product launch, one ordered sum per width (a group launch).  dwk[k - 1] = the kernel gradient of width k [k][K][Cw].
static int run_wgrad_bank_planes(const TrainCtx& x, const WgPlan& p, const float* xs, int ldx, const float* dY, int ldy, float* const* dwk, int M, int T, int K, int Cw, int nw) {
  const int ntap = nw * (nw + 1) / 2;
  uint4* pa = x.s->wps; uint4* pb = x.s->wps + p.na;
  wp_split_launch(x.st, xs, nullptr, ldx, M, T, K, p.Mp, nw, -((nw - 1) / 2), 1, pa);       // copy j: shift j - (nw - 1) / 2; width k, tap: shift tap - (k - 1) / 2
  wp_split_launch(x.st, dY, nullptr, ldy, M, T, nw * Cw, p.Mp, 1, 0, 0, pb);
  WpGemmArgs g; memset(&g, 0, sizeof g);
  g.a = pa; g.b = pb; g.K = K; g.N = Cw; g.Mp = p.Mp; g.kw = 1; g.a_per_tap = 1; g.lddw = Cw; g.nw = nw;
  g.rpb = p.rpb; g.part = x.s->det;
  size_t off = 0;
  for (int k = 1; k <= nw; ++k) { g.dwk[k - 1] = dwk[k - 1]; g.part_off[k - 1] = (unsigned)off; off += (size_t)p.nsplit * k * K * Cw; }
  wp_gemm_launch(x.st, g, ntap * p.nsplit);
  if (g.part) {
    WgRedGroup R; R.n = 0; R.start[0] = 0;
    for (int k = 1; k <= nw; ++k) {
      R.p[R.n].part = g.part + g.part_off[k - 1]; R.p[R.n].dw = dwk[k - 1]; R.p[R.n].nsplit = p.nsplit; R.p[R.n].kw = k; R.p[R.n].K = K; R.p[R.n].N = Cw; R.p[R.n].lddw = Cw;
      R.start[R.n + 1] = R.start[R.n] + cdiv(k * K * Cw, 256); ++R.n;
    }
    hipLaunchKernelGGL(k_wgrad_reduce_group, dim3(R.start[R.n]), dim3(256), 0, x.st, R);
  }
  HIPCHK(hipGetLastError());
  ++x.s->planes_problems;
  return 0;
}
static int run_wgrad(const TrainCtx& x, const float* xs, const int* gather, int ldx, const float* dy, int ldy, float* dw, int lddw,
                     int M, int T, int K, int N, int kw = 1, int padl = 0, const int* ygather = nullptr) {
  const WgPlan p = wgrad_plan(wg_env(x), M, T, K, N, kw, padl, gather != nullptr, ygather != nullptr);
  if (p.engine == WG_NONE) return fail(TACO_ERR_STATE, "%s for a %d x %d x %d weight gradient", p.why, kw, K, N);
  if (p.engine == WG_PLANES) return run_wgrad_planes(x, p, xs, gather, ldx, dy, ldy, dw, lddw, M, T, K, N, kw, padl);
  WgArgs g; g.ygather = ygather; g.x = xs; g.gather = gather; g.dy = dy; g.dw = dw; g.ldx = ldx; g.ldy = ldy; g.lddw = lddw; g.M = M; g.T = T; g.K = K; g.N = N;
  g.kw = kw; g.padl = padl; g.rpb = p.rpb;
  g.part = x.s->det;      // per-slice partial tiles + an ordered sum instead of atomics
  if (p.engine == WG_BF3_GROUP) {
    if (g.part) {
      TRY(wg_reserve(x, dw, nullptr, (size_t)p.nsplit * kw * K * N, &g.part));
      WgRedGroup& R = x.s->wgb.r;
      R.p[R.n].part = g.part; R.p[R.n].dw = dw; R.p[R.n].nsplit = p.nsplit; R.p[R.n].kw = kw; R.p[R.n].K = K; R.p[R.n].N = N; R.p[R.n].lddw = lddw;
      R.start[R.n + 1] = R.start[R.n] + cdiv(kw * K * N, 256); ++R.n;
    }
    WgGroup& G = x.s->wgb.g;
    G.p[G.n] = g;
    G.start[G.n + 1] = G.start[G.n] + cdiv(K, 64) * cdiv(N, 64) * kw * p.nsplit;
    if (++G.n == WG_MAXP) return wg_flush(x);
    return 0;
  }
  if (p.engine == WG_BF3_4W) hipLaunchKernelGGL((k_wgrad_bf3<4>), dim3(cdiv(K, 128), cdiv(N, 128), kw * p.nsplit), dim3(256), 0, x.st, g);
  else if (p.engine == WG_BF3_1W) hipLaunchKernelGGL((k_wgrad_bf3<1>), dim3(cdiv(K, 64), cdiv(N, 64), kw * p.nsplit), dim3(64), 0, x.st, g);
  else hipLaunchKernelGGL(k_wgrad, dim3(cdiv(K, 64), cdiv(N, 64), kw * p.nsplit), dim3(256), 0, x.st, g);
  if (g.part) hipLaunchKernelGGL(k_wgrad_reduce, EWGRID((size_t)kw * K * N), 0, x.st, (const float*)g.part, p.nsplit, kw, K, N, dw, lddw);
  HIPCHK(hipGetLastError());
  return 0;
}
static void run_embed_bwd(const TrainCtx& x, const float* dx, const int* ids, float* dE, int M, int E, int V) {
  x.s->end_paths |= x.s->det ? FRONT_PATH_EMBED_DET : FRONT_PATH_EMBED_ATOMIC;
  if (x.s->det) hipLaunchKernelGGL(k_embed_bwd_det, EWGRID((size_t)V * ((E + 63) / 64) * 64), 0, x.st, dx, ids, dE, M, E, V);      // one wave per (table row, 64 columns)
  else hipLaunchKernelGGL(k_embed_bwd, EWGRID((size_t)M * E), 0, x.st, dx, ids, dE, M, E);
}
// y = x . W^T style data gradient through k_gemm: out = conv_T(dy) (+ res).  taco_train_set_exact_gemm(t, 3): forward GEMMs exact fp32, data
// gradients split-bf16; (t, 2): data gradients on the exact-fp32 MFMA, forward GEMMs split-bf16 (A/B hook)
static int run_dgrad(const TrainCtx& x, const ConvL& Ld, const float* dy, int lddy, int M, int T, float* out, int ldo,
                     const float* res = nullptr, int ldres = 0) {
  GemmCall g; g.x = dy; g.ldx = lddy; g.M = M; g.T = T; g.out = out; g.ldo = ldo; g.res = res; g.ldres = ldres;
  g.force = x.t->dgrad_exact ? GEMM_FORCE_EXACT : x.t->dgrad_bf3 ? GEMM_FORCE_BF3 : GEMM_FORCE_NONE;
  return run_gemm(x.t->sm, x.st, &Ld, 1, false, g);
}

// ---------------------------------------------------------------------------------------------------------------
// tape layout
// ---------------------------------------------------------------------------------------------------------------
// BatchNorm + max-pool of a conv bank as one pass (k_bn_pool_bank_v4): the widths fit the pointer table and the columns go four at a time.
// The tape layout, the forward and the backward read this alone; the 16-byte alignment the pass needs is the workspace's (train_forward_backward refuses another)
static inline bool bank_pool_fused(const Cbhg& c) { return c.K <= BNB_MAXK && (c.C & 3) == 0; }
struct CbhgTape {
  float *bank_a, *bank_y, *pool, *bank_mu, *bank_rs;
  float *pa[4], *py[4], *pmu[4], *prs[4];
  float *res, *hx[10], *hH[8], *hT[8];
  float *xproj, *out, *gsave;
  float *dg, *rh, *d0, *d1, *dcat, *dbig0, *dbig1, *stat;
  Xchg gx;      // the whole-chip scans, forward and backward: exchange granules, census words
};
static void carve_cbhg_tape(Carver& cv, const Cbhg& c, int B, int T, CbhgTape& w) {
  const size_t M = (size_t)B * T, KC = (size_t)c.K * c.C;
  w.bank_a = cv.f(M * KC); w.bank_y = cv.f(bank_pool_fused(c) ? 1 : M * KC); w.pool = cv.f(M * KC); w.bank_mu = cv.f(KC); w.bank_rs = cv.f(KC);
  size_t wide = std::max<size_t>(c.in_dim, c.rnn);
  for (int i = 0; i < c.nproj; ++i) {
    w.pa[i] = cv.f(M * c.proj_dim[i]); w.py[i] = cv.f(M * c.proj_dim[i]); w.pmu[i] = cv.f(c.proj_dim[i]); w.prs[i] = cv.f(c.proj_dim[i]);
    wide = std::max<size_t>(wide, c.proj_dim[i]);
  }
  w.res = cv.f(M * c.in_dim);
  for (int i = 0; i <= c.depth; ++i) w.hx[i] = cv.f(M * c.rnn);
  for (int i = 0; i < c.depth; ++i) { w.hH[i] = cv.f(M * c.rnn); w.hT[i] = cv.f(M * c.rnn); }
  w.xproj = cv.f(M * 6 * c.rnn); w.out = cv.f(M * 2 * c.rnn); w.gsave = cv.f(M * 6 * c.rnn);
  w.dg = cv.f(M * 6 * c.rnn); w.rh = cv.f(M * 2 * c.rnn);
  w.d0 = cv.f(M * wide); w.d1 = cv.f(M * wide); w.dcat = cv.f(M * 2 * c.rnn);
  w.dbig0 = cv.f(M * KC); w.dbig1 = cv.f(M * KC); w.stat = cv.f(5 * std::max<size_t>(KC, wide));   // sums, centred sums + the 3-vector SyncBN exchange pack
  w.gx.carve(cv, std::max(gd_xbuf_granules(8), gb_xbuf_granules(8)));
}
struct DecTape {     // every per-step tensor is [B, n, W]: step t of row b at (b*n + t)*W
  float *keys, *zero, *ctx, *pz[4], *hA, *rA, *uA, *cA, *rhA, *xcA, *alpha, *alpha0;
  float *o[5], *h[4], *r[4], *u[4], *c[4], *rh[4], *xc[4];
  int* nz;
  float* tape256 = nullptr; size_t tstride = 0;          // the 256-wide per-step arrays in DXT_* order, back to back (persistent decoder, TAPE)
  Xchg dx; float* rowbias = nullptr;   // its exchange granules and census words (the backward loop's too), 'simple' row biases
  // backward
  float *dkeys, *dvalues, *dv_acc, *dsb_acc, *dalpha, *dctx, *dctx_t, *dhA, *dh[4], *dht, *dhp, *tmp1, *tmp2, *do_[5];
  float *g_dgp[4], *g_dcp[4], *g_dgpA, *g_dcpA, *g_do0, *g_do2, *g_dq, *g_dz[4], *dpz, *dIn;
  float *g_q, *g_e, *g_de, *g_dctx;   // attention tape: processed query, raw scores, their gradients' inputs
};
static void carve_dec_tape(Carver& cv, const taco_model* m, int B, int T_in, int n, DecTape& w) {
  const taco_hparams& hp = m->hp;
  const int D = 2 * hp.enc_rnn_size, As = hp.attention_state_size, Hd = hp.dec_rnn_size, A = hp.attention_size, L = hp.dec_layer_num;
  const size_t R = (size_t)B * n;
  w.keys = cv.f((size_t)B * T_in * A); w.zero = cv.f((size_t)B * std::max(std::max(hp.num_mels, As), std::max(Hd, D)));
  const int S = simple_S(m);      // 'simple': the speaker embedding rides behind the context and behind the last prenet output of every step
  w.ctx = cv.f(R * (D + S));
  // The persistent decoder (k_decoder_xcd<RG, true>) addresses its 256-wide per-step arrays as ONE block, slot s at tape256 + s * R * 256
  // (DXT_* order: P1, HA, RA, UA, CA, RHA, Q, O0, R1, U1, C1, RH1, H1, O1, R2, U2, C2, RH2, H2, O2): carve them back to back in that order.
  const bool dxl = dx_widths_ok(m);     // reference widths: every one of them is [R, 256]
  if (dxl) {
    float** slot[DXT_N] = {&w.pz[0], &w.hA, &w.rA, &w.uA, &w.cA, &w.rhA, &w.g_q, &w.o[0], &w.r[0], &w.u[0], &w.c[0], &w.rh[0], &w.h[0], &w.o[1],
                           &w.r[1], &w.u[1], &w.c[1], &w.rh[1], &w.h[1], &w.o[2]};
    for (int i = 0; i < DXT_N; ++i) *slot[i] = cv.f(R * DX_W);
    w.tape256 = w.pz[0]; w.tstride = R * DX_W;
    w.pz[1] = cv.f(R * (hp.dec_prenet[1] + S));
    w.xcA = cv.f(R * As);
    for (int i = 0; i < L; ++i) w.xc[i] = cv.f(R * Hd);
  } else {
    for (int i = 0; i < hp.dec_prenet_n; ++i) w.pz[i] = cv.f(R * (hp.dec_prenet[i] + (i == hp.dec_prenet_n - 1 ? S : 0)));
    w.hA = cv.f(R * As); w.rA = cv.f(R * As); w.uA = cv.f(R * As); w.cA = cv.f(R * As); w.rhA = cv.f(R * As); w.xcA = cv.f(R * As);
    for (int i = 0; i <= L; ++i) w.o[i] = cv.f(R * Hd);
    for (int i = 0; i < L; ++i) { w.h[i] = cv.f(R * Hd); w.r[i] = cv.f(R * Hd); w.u[i] = cv.f(R * Hd); w.c[i] = cv.f(R * Hd); w.rh[i] = cv.f(R * Hd); w.xc[i] = cv.f(R * Hd); }
  }
  w.alpha = cv.f((size_t)B * (n + 1) * T_in); w.alpha0 = cv.f((size_t)B * T_in);   // slot 0 = initial alignments, slot t+1 = step t
  { w.dx.carve(cv, (size_t)DX_NGROUP * std::max((size_t)dx_xlayout(8, T_in).total, dbx_xbuf_granules(T_in)));
    w.rowbias = cv.f(is_simple(m) ? (size_t)B * DXRB_N * DX_W : 1); }
  w.nz = cv.i((size_t)n * B);
  w.dkeys = cv.f((size_t)B * T_in * A); w.dvalues = cv.f((size_t)B * T_in * D); w.dv_acc = cv.f((size_t)B * A); w.dsb_acc = cv.f(B);
  w.dalpha = cv.f((size_t)B * T_in); w.dctx = cv.f((size_t)B * D); w.dctx_t = cv.f((size_t)B * D); w.dhA = cv.f((size_t)B * As);
  for (int i = 0; i < L; ++i) w.dh[i] = cv.f((size_t)B * Hd);
  const int Wmax = std::max(std::max(As, Hd), D);
  w.dht = cv.f((size_t)B * Wmax); w.dhp = cv.f((size_t)B * Wmax);
  const int W2 = std::max(std::max(2 * Hd, As + D), std::max(hp.dec_prenet[hp.dec_prenet_n - 1] + As, hp.num_mels + D)) + Wmax + S;
  w.tmp1 = cv.f((size_t)B * W2); w.tmp2 = cv.f((size_t)B * W2);
  for (int i = 0; i <= L; ++i) w.do_[i] = cv.f((size_t)B * Hd);
  for (int i = 0; i < L; ++i) { w.g_dgp[i] = cv.f(R * 2 * Hd); w.g_dcp[i] = cv.f(R * Hd); }
  w.g_dgpA = cv.f(R * 2 * As); w.g_dcpA = cv.f(R * As); w.g_do0 = cv.f(R * Hd); w.g_dq = cv.f(R * A); w.g_do2 = cv.f(R * Hd);
  for (int i = 0; i < hp.dec_prenet_n; ++i) w.g_dz[i] = cv.f(R * hp.dec_prenet[i]);
  w.dpz = cv.f((size_t)B * W2); w.dIn = cv.f((size_t)B * W2);
  if (!dxl) w.g_q = cv.f(R * A);
  w.g_e = cv.f(R * T_in); w.g_de = cv.f(R * T_in); w.g_dctx = cv.f(R * D);
}
struct TrainWs {
  float* pre[4]; float* dpre[4];
  CbhgTape enc, post;
  DecTape dec;
  float *teach, *mel, *linear, *dmel, *dlin, *denc, *dpost, *dmel_post, *demb, *losspart;
  SpkWs spk; float* dvec[8]; float* dspk_emb; float* dzs; int* rowidx;   // deepvoice: speaker vectors, their gradients, scratch
  float *linrv, *dlin_sum;                                               // simple: speaker term of the linear head [B, F], time-summed dlin
  float* detscr;                                                         // deterministic reductions: per-slice partial sums
  uint4* wpscr; size_t wps_uint4;                                        // bf16 planes of the weight gradients' operands (taco_wgrad_planes.h)
};
// plane scratch of a step whose longest row set has `rows` rows, in uint4 (1: the planes path is off)
static size_t wps_scratch_uint4(const taco_train* t, size_t rows) {
  const taco_hparams& hp = t->sm->hp;
  const size_t rp = (size_t)cdiv((int)rows, 64) * 64;
  const size_t cols = (size_t)std::max(hp.enc_bank_size * hp.enc_bank_channels, hp.post_bank_size * hp.post_bank_channels) + WP_SCRATCH_COLS;
  return t->wgrad_planes ? rp / 16 * (cols / 32) * 3 * 64 : 1;
}
static void carve_train(Carver& cv, const taco_train* t, int B, int T_in, int n, TrainWs& w) {
  const taco_model* m = t->sm;
  const taco_hparams& hp = m->hp;
  const size_t Me = (size_t)B * T_in, Mp = (size_t)B * n * hp.reduction_factor;
  for (int i = 0; i < hp.enc_prenet_n; ++i) { w.pre[i] = cv.f(Me * hp.enc_prenet[i]); w.dpre[i] = cv.f(Me * std::max(hp.enc_prenet[i], hp.embedding_size)); }
  carve_cbhg_tape(cv, m->enc, B, T_in, w.enc);
  carve_cbhg_tape(cv, m->post, B, n * hp.reduction_factor, w.post);
  carve_dec_tape(cv, m, B, T_in, n, w.dec);
  w.teach = cv.f((size_t)B * n * hp.num_mels);
  w.mel = cv.f(Mp * hp.num_mels); w.linear = cv.f(Mp * hp.num_freq);
  w.dmel = cv.f(Mp * hp.num_mels); w.dlin = cv.f(Mp * hp.num_freq);
  w.denc = cv.f(Me * 2 * hp.enc_rnn_size);
  w.dpost = cv.f(Mp * 2 * hp.post_rnn_size); w.dmel_post = cv.f(Mp * hp.num_mels); w.demb = cv.f(Me * hp.embedding_size);
  w.losspart = (float*)cv.raw((size_t)TR_MAXBLK * 8 * sizeof(double));
  carve_spk(cv, m, B, w.spk);
  { const int dims[3] = {hp.enc_prenet[hp.enc_prenet_n - 1], hp.enc_rnn_size * 2, hp.attention_state_size};
    int dmax = 1;
    for (int i = 0; i < 3 + hp.dec_layer_num; ++i) { const int dd = i < 3 ? dims[i] : hp.dec_rnn_size; w.dvec[i] = cv.f((size_t)B * dd); dmax = std::max(dmax, dd); }
    w.dspk_emb = cv.f((size_t)B * std::max(hp.speaker_embedding_size, 1)); w.dzs = cv.f((size_t)B * dmax); w.rowidx = cv.i(B); }
  const size_t nrv = is_simple(m) ? (size_t)B * hp.num_freq : 1;
  w.linrv = cv.f(nrv); w.dlin_sum = cv.f(nrv);
  w.detscr = cv.f(t->deterministic ? DET_SCRATCH_FLOATS : 1);
  w.wps_uint4 = wps_scratch_uint4(t, std::max(Me, Mp));
  w.wpscr = (uint4*)cv.raw(w.wps_uint4 * sizeof(uint4));
}

// ---------------------------------------------------------------------------------------------------------------
// CBHG: training forward with tape, and backward
// ---------------------------------------------------------------------------------------------------------------
// batch statistics of a [M, C] activation -> mu, rstd (and the moving averages of layer `name` in the parameter buffer)
static int bn_stats(const TrainCtx& x, const float* a, int lda, int M, int C, float* mu, float* rstd, float* scratch,
                    const std::string* names, const int* cols, int nnames) {
  hipStream_t st = x.st;
  // data-parallel SyncBN: mean and centred variance are those of the global batch -- what the reference's single-device step over
  // the whole batch computes (modules.py:131) -- merged from the ranks' own (mean, centred sum) pairs
  const bool sync = x.t->sync_fn && x.t->sync_world > 1;
  const float invM = 1.0f / ((float)M * (sync ? x.t->sync_world : 1));
  const bool det = x.s->det != nullptr;      // the ordered sums replace the scratch; the atomics of the other mode need it cleared
  if (!det) HIPCHK(zero_async(scratch, (size_t)2 * C * sizeof(float), st));
  TRY(run_colsum(x, a, lda, nullptr, 0, nullptr, nullptr, scratch, nullptr, M, C, 0, det));
  hipLaunchKernelGGL(k_bn_mean, EWGRID(C), 0, st, scratch, mu, C, 1.0f / (float)M);
  TRY(run_colsum(x, a, lda, nullptr, 0, mu, nullptr, nullptr, scratch + C, M, C, 1, det));
  if (sync) {
    // ONE exchange per layer (the layer's columns, or all widths of a conv bank at once): rank means, centred sums, squared means
    // (means are exchanged as offsets from the layer's moving mean, which every rank holds identically: k_bn_sync_pack)
    float* pack = scratch + 2 * C;
    for (int i = 0, c0 = 0; i < nnames; c0 += cols[i], ++i)
      hipLaunchKernelGGL(k_bn_sync_pack, EWGRID(cols[i]), 0, st, mu, scratch + C, (const float*)x.p(names[i] + "/moving_mean"), pack, C, c0, cols[i]);
    x.t->sync_fn(x.t->sync_user, pack, 3 * C);
    for (int i = 0, c0 = 0; i < nnames; c0 += cols[i], ++i)
      hipLaunchKernelGGL(k_bn_sync_combine, EWGRID(cols[i]), 0, st, pack, (const float*)x.p(names[i] + "/moving_mean"), mu, scratch + C, C, c0, cols[i],
                         (float)M, (float)x.t->sync_world);
  }
  bool even = nnames > 1 && nnames <= BNB_MAXK;
  for (int i = 1; i < nnames; ++i) even = even && cols[i] == cols[0];
  if (even) {                          // the layers of a conv bank: one launch for all of them
    BnBank nb; memset(&nb, 0, sizeof nb); nb.Cw = cols[0];
    for (int i = 0; i < nnames; ++i) {
      nb.mov_mean[i] = x.update_moving ? x.p(names[i] + "/moving_mean") : (float*)nullptr;
      nb.mov_var[i] = x.update_moving ? x.p(names[i] + "/moving_variance") : (float*)nullptr;
    }
    hipLaunchKernelGGL(k_bn_finalize_bank, EWGRID(C), 0, st, mu, scratch + C, rstd, nb, C, invM, 1e-3f, 0.99f);
    HIPCHK(hipGetLastError());
    return 0;
  }
  int c0 = 0;
  for (int i = 0; i < nnames; ++i) {   // one BatchNorm layer per column block (conv bank) or the whole matrix
    // forward-only passes (loss fetches, the test model, a capture warm-up) leave the moving statistics alone, as the reference does
    hipLaunchKernelGGL(k_bn_finalize, EWGRID(cols[i]), 0, st, mu + c0, scratch + C + c0, rstd + c0,
                       x.update_moving ? x.p(names[i] + "/moving_mean") : (float*)nullptr,
                       x.update_moving ? x.p(names[i] + "/moving_variance") : (float*)nullptr, cols[i], invM, 1e-3f, 0.99f);
    c0 += cols[i];
  }
  HIPCHK(hipGetLastError());
  return 0;
}
static int cbhg_forward_train(const TrainCtx& x, const Cbhg& c, const CbhgT& ct, const std::string& sc, const float* in, int B, int T,
                              const int* lengths, const CbhgTape& w, const float* before_highway = nullptr, const float* init_state = nullptr) {
  const taco_model* m = x.t->sm; hipStream_t st = x.st;
  const int M = B * T, KC = c.K * c.C;
  { GemmCall g; g.x = in; g.ldx = c.in_dim; g.M = M; g.T = T; g.act = ACT_RELU; g.out = w.bank_a; g.ldo = KC;
    TRY(run_gemm(m, st, ct.bank_f.data(), c.K, false, g)); }
  { std::vector<std::string> names; std::vector<int> cols;
    // column block k-1 of the concatenation belongs to conv1d_k (modules.py:35-44)
    for (int k = 1; k <= c.K; ++k) { names.push_back(sc + "/conv_bank/conv1d_" + std::to_string(k)); cols.push_back(c.C); }
    TRY(bn_stats(x, w.bank_a, KC, M, KC, w.bank_mu, w.bank_rs, w.stat, names.data(), cols.data(), c.K));
    if (bank_pool_fused(c)) {      // BatchNorm of all widths + the max-pool in ONE pass: the BatchNorm output is never stored (k_bn_pool_bank_v4)
      BnBank nb; memset(&nb, 0, sizeof nb); nb.Cw = c.C;
      for (int k = 1; k <= c.K; ++k) { nb.gamma[k - 1] = x.p(names[k - 1] + "/gamma"); nb.beta[k - 1] = x.p(names[k - 1] + "/beta"); }
      hipLaunchKernelGGL(k_bn_pool_bank_v4, EWGRID((size_t)M * KC / 4), 0, st, (const float*)w.bank_a, KC, (const float*)w.bank_mu, (const float*)w.bank_rs, nb, w.pool, KC, M, T, KC, c.maxpool);
      x.s->paths |= CBHG_PATH_BANK_FWD_FUSED;
    } else {
    x.s->paths |= CBHG_PATH_BANK_FWD_PLAIN;
    for (int k = 1; k <= c.K; ++k) {
      const int c0 = (k - 1) * c.C;
      hipLaunchKernelGGL(k_bn_apply, EWGRID((size_t)M * c.C), 0, st, w.bank_a + c0, KC, w.bank_mu + c0, w.bank_rs + c0,
                         x.p(names[k - 1] + "/gamma"), x.p(names[k - 1] + "/beta"), w.bank_y + c0, KC, M, c.C);
    }
    hipLaunchKernelGGL(k_maxpool_fwd, EWGRID((size_t)M * KC), 0, st, w.bank_y, w.pool, M, T, KC, c.maxpool);
    } }
  HIPCHK(hipGetLastError());
  const float* cur = w.pool; int curd = KC;
  for (int i = 0; i < c.nproj; ++i) {
    const std::string n = sc + "/proj_" + std::to_string(i + 1);
    const int N = c.proj_dim[i];
    GemmCall p; p.x = cur; p.ldx = curd; p.M = M; p.T = T; p.act = (i + 1 == c.nproj) ? ACT_NONE : ACT_RELU; p.out = w.pa[i]; p.ldo = N;
    TRY(run_gemm(m, st, &ct.proj_f[i], 1, false, p));
    TRY(bn_stats(x, w.pa[i], N, M, N, w.pmu[i], w.prs[i], w.stat, &n, &N, 1));
    if ((N & 3) == 0 && al16h(w.pa[i]) && al16h(w.py[i])) {
      x.s->paths |= CBHG_PATH_PROJ_BN_V4;
      hipLaunchKernelGGL(k_bn_apply_v4, EWGRID((size_t)M * N / 4), 0, st, (const float*)w.pa[i], N, (const float*)w.pmu[i], (const float*)w.prs[i], (const float*)x.p(n + "/gamma"), (const float*)x.p(n + "/beta"), w.py[i], N, M, N);
    } else {
      x.s->paths |= CBHG_PATH_PROJ_BN_PLAIN;
      hipLaunchKernelGGL(k_bn_apply, EWGRID((size_t)M * N), 0, st, w.pa[i], N, w.pmu[i], w.prs[i], x.p(n + "/gamma"), x.p(n + "/beta"), w.py[i], N, M, N);
    }
    cur = w.py[i]; curd = N;
  }
  // residual (modules.py:62-69)
  hipLaunchKernelGGL(k_copy2d, EWGRID((size_t)M * c.in_dim), 0, st, cur, c.in_dim, w.res, c.in_dim, M, c.in_dim);
  hipLaunchKernelGGL(k_add2d, EWGRID((size_t)M * c.in_dim), 0, st, w.res, c.in_dim, in, c.in_dim, M, c.in_dim);
  if (before_highway) hipLaunchKernelGGL(k_add_rowvec, EWGRID((size_t)M * c.in_dim), 0, st, w.res, before_highway, M, T, c.in_dim);   // modules.py:66-69
  HIPCHK(hipGetLastError());
  if (c.has_dense) { GemmCall d; d.x = w.res; d.ldx = c.in_dim; d.M = M; d.out = w.hx[0]; d.ldo = c.rnn; TRY(run_gemm(m, st, &c.dense, 1, false, d)); }
  else hipLaunchKernelGGL(k_copy2d, EWGRID((size_t)M * c.rnn), 0, st, w.res, c.rnn, w.hx[0], c.rnn, M, c.rnn);
  for (int i = 0; i < c.depth; ++i) {
    GemmCall h; h.x = w.hx[i]; h.ldx = c.rnn; h.M = M; h.out = w.hx[i + 1]; h.ldo = c.rnn; h.aux0 = w.hH[i]; h.aux1 = w.hT[i];
    TRY(run_gemm(m, st, &c.hw[i], 1, true, h));
  }
  const int H = c.rnn;
  { GemmCall xp; xp.x = w.hx[c.depth]; xp.ldx = H; xp.M = M; xp.T = T; xp.out = w.xproj; xp.ldo = 6 * H; xp.rev_len = lengths; xp.rev_col0 = 3 * H;
    TRY(run_gemm(m, st, &c.xproj, 1, false, xp)); }
  if (lengths) HIPCHK(zero_async(w.gsave, (size_t)M * 6 * H * sizeof(float), st));      // (without lengths -- the post-net -- every step of every row is active and written)
  const ScanPlan sp = scan_plan(m, c, B, T, true);
  if (sp.kernel == SCAN_K_OCT || sp.kernel == SCAN_K_DUO) x.s->paths |= (unsigned)sp.kernel << CBHG_PATH_SCAN_FWD_SHIFT;
  if (sp.kernel == SCAN_K_OCT)     // the whole-chip scans of inference with the gate tape (k_bigru_oct<UPW, true> / k_bigru_duo<RG, true>)
    return oct_launch(m, st, c, sp.upw, B, T, w.xproj, lengths, init_state, w.out, w.gsave, w.gx);
  if (sp.kernel == SCAN_K_DUO)
    return duo_launch(m, st, c, sp.rg, B, T, w.xproj, lengths, init_state, w.out, w.gsave, w.gx);
  if (sp.kernel == SCAN_K_RES || sp.kernel == SCAN_K_QUAD) {     // recurrent weights resident on the CU (k_bigru_res; H = 128: k_bigru_quad, as inference runs it), gates saved for the backward scan
    BigruSArgs a; memset(&a, 0, sizeof a);
    a.xproj = w.xproj; a.g2_0 = (const float2*)AP(m, c.res_g2[0]); a.g2_1 = (const float2*)AP(m, c.res_g2[1]);
    a.c1_0 = AP(m, c.raw_ch[0]); a.c1_1 = AP(m, c.raw_ch[1]); a.lengths = lengths; a.out = w.out; a.gsave = w.gsave; a.B = B; a.T = T;
    a.h0 = init_state;
    const bool quad = H != 256 && sp.kernel == SCAN_K_QUAD && x.t->resident_bwd_scan;      // (the A/B engine keeps k_bigru_res)
    x.s->paths |= (unsigned)(quad ? SCAN_K_QUAD : SCAN_K_RES) << CBHG_PATH_SCAN_FWD_SHIFT;
    if (H == 256) hipLaunchKernelGGL((k_bigru_res<256, 64, 24, 1, true>), dim3(2 * B), dim3(512), bigru_res_lds(256, 24, 1), st, a);
    else if (quad) hipLaunchKernelGGL(k_bigru_quad<true>, dim3(2 * B), dim3(512), 0, st, a);
    else hipLaunchKernelGGL((k_bigru_res<128, 32, 0, 1, true>), dim3(2 * B), dim3(512), bigru_res_lds(128, 0, 1), st, a);
  } else {
    int R = 0; size_t lds = 0;
    if (sp.kernel != SCAN_K_ROWS || !bigru_rows_cfg(B, H, &R, &lds)) return fail(TACO_ERR_UNSUPPORTED, "rnn size %d does not fit the row-parallel BiGRU kernel", H);
    BigruRArgs a; memset(&a, 0, sizeof a);
    a.xproj = w.xproj; a.wg0 = AP(m, c.raw_gh[0]); a.wg1 = AP(m, c.raw_gh[1]); a.wc0 = AP(m, c.raw_ch[0]); a.wc1 = AP(m, c.raw_ch[1]);
    a.lengths = lengths; a.out = w.out; a.gsave = w.gsave; a.B = B; a.T = T; a.H = H; a.h0 = init_state;
    x.s->paths |= (unsigned)SCAN_K_ROWS << CBHG_PATH_SCAN_FWD_SHIFT;
    if (R == 2) hipLaunchKernelGGL((k_bigru_rows<2, true>), dim3(2 * cdiv(B, R)), dim3(RP_NT), lds, st, a);
    else hipLaunchKernelGGL((k_bigru_rows<1, true>), dim3(2 * cdiv(B, R)), dim3(RP_NT), lds, st, a);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// one conv1d+act+BN(train) layer backward: dy (grad of BN output) -> weight/bias/gamma/beta grads and dz (pre-activation grad).
// Two halves so that layers whose dy exist at the same time (the widths of a conv bank) share ONE SyncBN exchange:
// _sums: per-channel sum dy, sum dy*xhat into the beta / gamma gradients (+ a copy at sync_scratch[c0], sync_scratch[Ctot + c0]);
// _apply: dz and the bias gradient from those sums (the global ones when synchronised).
static int conv_bn_backward_sums(const TrainCtx& x, const std::string& name, const float* a, int lda, const float* dy, int lddy, const float* mu,
                                 const float* rstd, int M, int C, float* sync_scratch, int c0, int Ctot) {
  hipStream_t st = x.st;
  TRY(run_colsum(x, a, lda, dy, lddy, mu, rstd, x.g(name + "/beta"), x.g(name + "/gamma"), M, C, 2));
  if (x.t->sync_fn && x.t->sync_world > 1) {
    TRY(wg_flush(x));                  // (the sums are copied right here)
    // the gradient buffers keep this rank's own sums (the flat all-reduce after backward averages them like every other gradient)
    HIPCHK(hipMemcpyAsync(sync_scratch + c0, x.g(name + "/beta"), (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(sync_scratch + Ctot + c0, x.g(name + "/gamma"), (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  return 0;
}
static void conv_bn_backward_exchange(const TrainCtx& x, float* sync_scratch, int Ctot) {
  if (x.t->sync_fn && x.t->sync_world > 1) x.t->sync_fn(x.t->sync_user, sync_scratch, 2 * Ctot);
}
static int conv_bn_backward_apply(const TrainCtx& x, const std::string& name, const float* a, int lda, const float* dy, int lddy, const float* mu,
                                  const float* rstd, bool relu, float* dz, int lddz, int M, int C, const float* sync_scratch, int c0, int Ctot,
                                  bool dz_done = false) {      // dz_done: the caller formed dz for all layers of a bank in one launch (bank_bn_bwd)
  hipStream_t st = x.st;
  const bool sync = x.t->sync_fn && x.t->sync_world > 1;
  const float* sdy = sync ? sync_scratch + c0 : x.g(name + "/beta");
  const float* sdyxh = sync ? sync_scratch + Ctot + c0 : x.g(name + "/gamma");
  const float invM = 1.0f / ((float)M * (sync ? x.t->sync_world : 1));
  if (dz_done) {}
  else if ((C & 3) == 0 && (lda & 3) == 0 && (lddy & 3) == 0 && (lddz & 3) == 0 && al16h(a) && al16h(dy) && al16h(dz)) {
    x.s->paths |= CBHG_PATH_BN_BWD_V4;
    hipLaunchKernelGGL(k_bn_bwd_v4, EWGRID((size_t)M * C / 4), 0, st, a, lda, dy, lddy, mu, rstd, (const float*)x.p(name + "/gamma"), sdy,
                       sdyxh, relu ? 1 : 0, dz, lddz, M, C, invM);
  } else {
  x.s->paths |= CBHG_PATH_BN_BWD_PLAIN;
  hipLaunchKernelGGL(k_bn_bwd, EWGRID((size_t)M * C), 0, st, a, lda, dy, lddy, mu, rstd, x.p(name + "/gamma"), sdy,
                     sdyxh, relu ? 1 : 0, dz, lddz, M, C, invM);
  }
  TRY(run_colsum(x, dz, lddz, nullptr, 0, nullptr, nullptr, x.g(name + "/bias"), nullptr, M, C, 0));
  HIPCHK(hipGetLastError());
  return 0;
}
static int conv_bn_backward(const TrainCtx& x, const std::string& name, const float* a, int lda, const float* dy, int lddy, const float* mu,
                            const float* rstd, bool relu, float* dz, int lddz, int M, int C, float* sync_scratch) {
  TRY(conv_bn_backward_sums(x, name, a, lda, dy, lddy, mu, rstd, M, C, sync_scratch, 0, C));
  TRY(wg_flush(x));                    // (inside a batching region the sums above are still queued)
  conv_bn_backward_exchange(x, sync_scratch, C);
  return conv_bn_backward_apply(x, name, a, lda, dy, lddy, mu, rstd, relu, dz, lddz, M, C, sync_scratch, 0, C);
}
// dout [M, 2*rnn] -> din [M, in_dim]
static int cbhg_backward(const TrainCtx& x, const Cbhg& c, const CbhgT& ct, const std::string& sc, const float* in, const int* in_gather,
                         int B, int T, const int* lengths, const float* dout, float* din, const CbhgTape& w,
                         const float* h0 = nullptr, float* dh0 = nullptr, float* d_before = nullptr, int* rowidx = nullptr) {
  const taco_model* m = x.t->sm; hipStream_t st = x.st;
  const int M = B * T, KC = c.K * c.C, H = c.rnn, I = c.rnn;
  // ---- BiGRU ----
  // (the backward scans write the steps inside a row's length only; k_bigru_duo_bwd without lengths -- the post-net -- writes every element)
  const ScanPlan sp = scan_plan(m, c, B, T, true);
  const bool duo_bwd = sp.bwd != SCAN_BWD_ROWS;       // a whole-chip backward scan (k_bigru_duo_bwd / k_bigru_oct_bwd)
  // The whole-chip backward scans poll w.gx like the forward ones, but do not clear it themselves: here its clear shares ONE fill launch with
  // the two accumulators below (a launch and its graph edge less per CBHG and step), so duo_bwd_launch / oct_bwd_launch expect it done
  ZeroBatch zb(st);
  if (!(duo_bwd && !lengths)) {
    HIPCHK(zb.add(w.dg, (size_t)M * 6 * H * sizeof(float)));
    HIPCHK(zb.add(w.rh, (size_t)M * 2 * H * sizeof(float)));
  }
  if (duo_bwd) HIPCHK(zb.add(w.gx.p, w.gx.bytes));
  HIPCHK(zb.run());
  if (sp.bwd == SCAN_BWD_OCT) {
    // one row per cluster of 8 CUs, as the forward scan of these shapes (k_bigru_oct_bwd)
    x.s->paths |= (unsigned)CBHG_SCAN_BWD_OCT << CBHG_PATH_SCAN_BWD_SHIFT;
    TRY(oct_bwd_launch(m, st, c, B, T, dout, w.out, w.gsave, h0, lengths, w.dg, w.rh, dh0, w.gx));
  } else if (duo_bwd) {
    // both directions of RG rows per group of 32 CUs, the directions software-pipelined against each other (k_bigru_duo_bwd)
    x.s->paths |= (unsigned)CBHG_SCAN_BWD_DUO << CBHG_PATH_SCAN_BWD_SHIFT;
    TRY(duo_bwd_launch(m, st, c, sp.rg, B, T, dout, w.out, w.gsave, h0, lengths, w.dg, w.rh, dh0, w.gx));
  } else if (H == 128 && x.t->resident_bwd_scan) {
    // recurrent kernels resident in registers, one workgroup per (direction, row) (k_bigru_resb): the encoder at the reference width
    BigruQArgs a; memset(&a, 0, sizeof a);
    a.dout = dout; a.out = w.out; a.gsave = w.gsave; a.gh0 = AP(m, c.raw_gh[0]); a.gh1 = AP(m, c.raw_gh[1]); a.ch0 = AP(m, c.raw_ch[0]); a.ch1 = AP(m, c.raw_ch[1]);
    a.lengths = lengths; a.dg = w.dg; a.rh = w.rh; a.h0 = h0; a.dh0 = dh0; a.B = B; a.T = T;
    x.s->paths |= (unsigned)CBHG_SCAN_BWD_RESB << CBHG_PATH_SCAN_BWD_SHIFT;
    hipLaunchKernelGGL(k_bigru_resb<128>, dim3(2 * B), dim3(512), 0, st, a);
    HIPCHK(hipGetLastError());
  } else {
    int R = (B >= 2 && 2 * H <= RP_NT) ? 2 : 1;
    if ((size_t)R * H > RP_NT || (H % 4)) return fail(TACO_ERR_UNSUPPORTED, "rnn size %d does not fit the BiGRU backward kernel", H);
    const size_t lds = ((size_t)4 * R * H + (size_t)RP_NT * R * 4 + 64) * sizeof(float);
    BigruBArgs a; memset(&a, 0, sizeof a);
    a.dout = dout; a.out = w.out; a.gsave = w.gsave; a.wgT0 = AP(m, ct.ghT[0]); a.wgT1 = AP(m, ct.ghT[1]); a.wcT0 = AP(m, ct.chT[0]); a.wcT1 = AP(m, ct.chT[1]);
    a.lengths = lengths; a.dg = w.dg; a.rh = w.rh; a.B = B; a.T = T; a.H = H; a.h0 = h0; a.dh0 = dh0;
    x.s->paths |= (unsigned)CBHG_SCAN_BWD_ROWS << CBHG_PATH_SCAN_BWD_SHIFT;
    if (R == 2) hipLaunchKernelGGL(k_bigru_rows_bwd<2>, dim3(2 * cdiv(B, R)), dim3(RP_NT), lds, st, a);
    else hipLaunchKernelGGL(k_bigru_rows_bwd<1>, dim3(2 * cdiv(B, R)), dim3(RP_NT), lds, st, a);
    HIPCHK(hipGetLastError());
  }
  const float* hlast = w.hx[c.depth];
  WgRegion wgr(x);           // small weight gradients of this CBHG join group launches; flushed wherever an operand is about to be reused
  for (int dir = 0; dir < 2; ++dir) {
    const std::string n = sc + "/bigru/" + (dir ? "bw" : "fw");
    const float* dgg = w.dg + dir * 3 * H;          // gates columns (r|u), candidate at +2H
    float* Gg = x.g(n + "/gates/kernel"); float* Gc = x.g(n + "/candidate/kernel");
    TRY(run_wgrad(x, hlast, nullptr, I, dgg, 6 * H, Gg, 2 * H, M, T, I, 2 * H));                                   // x rows of gates
    TRY(run_wgrad(x, hlast, nullptr, I, dgg + 2 * H, 6 * H, Gc, H, M, T, I, H));                                    // x rows of candidate
    // h rows: state before the step = output one step earlier in the direction's own time (zero at the sequence start / past the length)
    TRY(run_wgrad(x, w.out + dir * H, nullptr, 2 * H, dgg, 6 * H, Gg + (size_t)I * 2 * H, 2 * H, M, T, H, 2 * H, 1, dir ? -1 : 1));
    TRY(run_wgrad(x, w.rh + dir * H, nullptr, 2 * H, dgg + 2 * H, 6 * H, Gc + (size_t)I * H, H, M, T, H, H));
    if (h0) {   // first step of the direction: the state before it is the initial state, not a row of the output tape
      if (dir == 0) TRY(run_wgrad(x, h0, nullptr, 2 * H, dgg, T * 6 * H, Gg + (size_t)I * 2 * H, 2 * H, B, 0, H, 2 * H));
      else {
        hipLaunchKernelGGL(k_last_row_index, EWGRID(B), 0, st, lengths, rowidx, B, T);
        TRY(run_wgrad(x, h0 + H, nullptr, 2 * H, dgg, 6 * H, Gg + (size_t)I * 2 * H, 2 * H, B, 0, H, 2 * H, 1, 0, rowidx));
      }
    }
    TRY(run_colsum(x, dgg, 6 * H, nullptr, 0, nullptr, nullptr, x.g(n + "/gates/bias"), nullptr, M, 2 * H, 0));
    TRY(run_colsum(x, dgg + 2 * H, 6 * H, nullptr, 0, nullptr, nullptr, x.g(n + "/candidate/bias"), nullptr, M, H, 0));
  }
  TRY(wg_flush(x));
  float* dcur = w.d0; float* dalt = w.d1;
  TRY(run_dgrad(x, ct.xproj_d, w.dg, 6 * H, M, T, dcur, I));
  // ---- highways ----
  for (int i = c.depth - 1; i >= 0; --i) {
    const std::string n = sc + "/highway_" + std::to_string(i + 1);
    if ((H & 3) == 0 && al16h(dcur) && al16h(w.hx[i]) && al16h(w.hH[i]) && al16h(w.hT[i]) && al16h(w.dcat) && al16h(dalt)) {
      x.s->paths |= CBHG_PATH_HW_BWD_V4;
      hipLaunchKernelGGL(k_highway_bwd_v4, EWGRID((size_t)M * H / 4), 0, st, (const float*)dcur, (const float*)w.hx[i], (const float*)w.hH[i], (const float*)w.hT[i], w.dcat, dalt, M, H);
    } else {
      x.s->paths |= CBHG_PATH_HW_BWD_PLAIN;
      hipLaunchKernelGGL(k_highway_bwd, EWGRID((size_t)M * H), 0, st, dcur, w.hx[i], w.hH[i], w.hT[i], w.dcat, dalt, M, H);
    }
    HIPCHK(hipGetLastError());
    TRY(run_wgrad(x, w.hx[i], nullptr, H, w.dcat, 2 * H, x.g(n + "/H/kernel"), H, M, 0, H, H));
    TRY(run_wgrad(x, w.hx[i], nullptr, H, w.dcat + H, 2 * H, x.g(n + "/T/kernel"), H, M, 0, H, H));
    TRY(run_colsum(x, w.dcat, 2 * H, nullptr, 0, nullptr, nullptr, x.g(n + "/H/bias"), nullptr, M, H, 0));
    TRY(run_colsum(x, w.dcat + H, 2 * H, nullptr, 0, nullptr, nullptr, x.g(n + "/T/bias"), nullptr, M, H, 0));
    TRY(run_dgrad(x, ct.hw_d[i], w.dcat, 2 * H, M, 0, dalt, H, dalt, H));   // += direct path
    TRY(wg_flush(x));                                                            // (dcat is the next layer's scratch)
    std::swap(dcur, dalt);
  }
  // ---- dense (post-net) ----
  if (c.has_dense) {
    TRY(run_wgrad(x, w.res, nullptr, c.in_dim, dcur, H, x.g(sc + "/dense/kernel"), H, M, 0, c.in_dim, H));
    TRY(run_colsum(x, dcur, H, nullptr, 0, nullptr, nullptr, x.g(sc + "/dense/bias"), nullptr, M, H, 0));
    TRY(run_dgrad(x, ct.dense_d, dcur, H, M, 0, dalt, c.in_dim));
    TRY(wg_flush(x));
    std::swap(dcur, dalt);
  }
  // dcur = gradient of (proj_last + x (+ before_highway)): keep a copy for the residual path
  if (d_before) { hipLaunchKernelGGL(k_time_sum, EWGRID((size_t)B * c.in_dim), 0, st, dcur, d_before, B, T, c.in_dim); HIPCHK(hipGetLastError()); }
  float* dres = din;
  hipLaunchKernelGGL(k_copy2d, EWGRID((size_t)M * c.in_dim), 0, st, dcur, c.in_dim, dres, c.in_dim, M, c.in_dim);
  HIPCHK(hipGetLastError());
  // ---- projections (last first) ----
  for (int i = c.nproj - 1; i >= 0; --i) {
    const std::string n = sc + "/proj_" + std::to_string(i + 1);
    const int N = c.proj_dim[i];
    const float* xin = (i == 0) ? w.pool : w.py[i - 1]; const int xd = (i == 0) ? KC : c.proj_dim[i - 1];
    TRY(conv_bn_backward(x, n, w.pa[i], N, dcur, N, w.pmu[i], w.prs[i], i + 1 != c.nproj, dalt, N, M, N, w.stat));
    TRY(run_wgrad(x, xin, nullptr, xd, dalt, N, x.g(n + "/kernel"), N, M, T, xd, N, c.pw, (c.pw - 1) / 2));
    float* dnext = (i == 0) ? w.dbig0 : dcur;
    TRY(run_dgrad(x, ct.proj_d[i], dalt, N, M, T, dnext, xd));
    TRY(wg_flush(x));                                                            // (dalt is rewritten by the next projection)
    if (i > 0) { /* dnext == dcur already holds the gradient of py[i-1] */ }
  }
  // ---- maxpool + conv bank ----
  if (bank_pool_fused(c)) {      // (the forward's test: the pool's input is recomputed from the bank's activations)
    BnBank nb; memset(&nb, 0, sizeof nb); nb.Cw = c.C;
    for (int k = 1; k <= c.K; ++k) { const std::string n = sc + "/conv_bank/conv1d_" + std::to_string(k); nb.gamma[k - 1] = x.p(n + "/gamma"); nb.beta[k - 1] = x.p(n + "/beta"); }
    hipLaunchKernelGGL(k_maxpool_bwd_bn_v4, EWGRID((size_t)M * KC / 4), 0, st, (const float*)w.bank_a, KC, (const float*)w.bank_mu, (const float*)w.bank_rs, nb, (const float*)w.dbig0, w.dbig1, M, T, KC, c.maxpool);
    x.s->paths |= CBHG_PATH_POOL_BWD_FUSED;
  } else {
    hipLaunchKernelGGL(k_maxpool_bwd, EWGRID((size_t)M * KC), 0, st, w.bank_y, w.dbig0, w.dbig1, M, T, KC, c.maxpool);
    x.s->paths |= CBHG_PATH_POOL_BWD_PLAIN;
  }
  HIPCHK(hipGetLastError());
  for (size_t bi = 0; bi < c.bank.size(); ++bi) {     // the bank's BatchNorm sums of all widths, then one exchange for all of them
    const int k = c.bank[bi].kw, c0 = (k - 1) * c.C;
    const std::string n = sc + "/conv_bank/conv1d_" + std::to_string(k);
    TRY(conv_bn_backward_sums(x, n, w.bank_a + c0, KC, w.dbig1 + c0, KC, w.bank_mu + c0, w.bank_rs + c0, M, c.C, w.stat, c0, KC));
  }
  TRY(wg_flush(x));                    // the sums of all widths: one group launch
  conv_bn_backward_exchange(x, w.stat, KC);
  // dz of ALL widths in one launch (their BatchNorm sums are complete: the flush above); the layers' own vectors through a pointer table
  bool bank_dz = false;
  if ((int)c.bank.size() == c.K && c.K <= BNB_MAXK && (c.C & 3) == 0 && al16h(w.bank_a) && al16h(w.dbig0) && al16h(w.dbig1)) {
    const bool sync = x.t->sync_fn && x.t->sync_world > 1;
    BnBank nb; memset(&nb, 0, sizeof nb); nb.Cw = c.C;
    bool all = true;
    for (size_t bi = 0; bi < c.bank.size(); ++bi) {
      const int k = c.bank[bi].kw, c0 = (k - 1) * c.C;
      if (k < 1 || k > c.K || nb.gamma[k - 1]) { all = false; break; }
      const std::string n = sc + "/conv_bank/conv1d_" + std::to_string(k);
      nb.gamma[k - 1] = x.p(n + "/gamma");
      nb.sdy[k - 1] = sync ? w.stat + c0 : x.g(n + "/beta");
      nb.sdyxh[k - 1] = sync ? w.stat + KC + c0 : x.g(n + "/gamma");
    }
    if (all) {
      const float invM = 1.0f / ((float)M * (sync ? x.t->sync_world : 1));
      hipLaunchKernelGGL(k_bn_bwd_bank_v4, EWGRID((size_t)M * KC / 4), 0, st, (const float*)w.bank_a, KC, (const float*)w.dbig1, KC, (const float*)w.bank_mu, (const float*)w.bank_rs, nb, 1,
                         w.dbig0, KC, M, KC, invM);
      HIPCHK(hipGetLastError());
      bank_dz = true;
    }
  }
  x.s->paths |= bank_dz ? CBHG_PATH_BANK_DZ_ONE : CBHG_PATH_BANK_DZ_EACH;
  // every width's kernel gradient from ONE conversion of dz and one product launch (taco_wgrad_planes.h), where dz of all widths is complete
  const WgPlan bank_plan = bank_dz ? wgrad_bank_plan(wg_env(x), M, T, c.in_dim, c.C, c.K, in_gather != nullptr) : WgPlan();
  x.s->paths |= bank_plan.engine == WG_PLANES ? CBHG_PATH_BANK_WG_PLANES : CBHG_PATH_BANK_WG_EACH;
  if (bank_plan.engine == WG_PLANES) {
    float* dwk[WP_MAXW];
    for (size_t bi = 0; bi < c.bank.size(); ++bi) dwk[c.bank[bi].kw - 1] = x.g(sc + "/conv_bank/conv1d_" + std::to_string(c.bank[bi].kw) + "/kernel");
    TRY(run_wgrad_bank_planes(x, bank_plan, in, c.in_dim, w.dbig0, KC, dwk, M, T, c.in_dim, c.C, c.K));
  }
  for (size_t bi = 0; bi < c.bank.size(); ++bi) {
    const int k = c.bank[bi].kw, c0 = (k - 1) * c.C;
    const std::string n = sc + "/conv_bank/conv1d_" + std::to_string(k);
    TRY(conv_bn_backward_apply(x, n, w.bank_a + c0, KC, w.dbig1 + c0, KC, w.bank_mu + c0, w.bank_rs + c0, true, w.dbig0 + c0, KC, M, c.C, w.stat, c0, KC, bank_dz));
    if (bank_plan.engine != WG_PLANES) TRY(run_wgrad(x, in, in_gather, c.in_dim, w.dbig0 + c0, KC, x.g(n + "/kernel"), c.C, M, T, c.in_dim, c.C, k, (k - 1) / 2));
    TRY(run_dgrad(x, ct.bank_d[bi], w.dbig0 + c0, KC, M, T, din, c.in_dim, din, c.in_dim));   // accumulates onto the residual path
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// decoder: teacher-forced training forward with tape (TacoTrainingHelper, helpers.py:35-67), and BPTT
// ---------------------------------------------------------------------------------------------------------------
static int gru_cell_train(const taco_model* m, hipStream_t st, const GruDec& g, int B, const float* xin, int ldx, const float* hprev, int ldh,
                          float* hnew, float* rh, float* u, float* xc, float* r, float* c, int ld, float* out_res) {
  SkJob ja = sk_base(m, g.gx, xin, ldx, g.I, hprev, ldh);
  ja.H = g.H; ja.e0 = hprev; ja.lde0 = ldh; ja.o0 = rh; ja.ldo0 = ld; ja.o1 = u; ja.ldo1 = ld; ja.o2 = xc; ja.ldo2 = ld; ja.o3 = r; ja.ldo3 = ld;
  TRY(run_skinny(st, B, &ja, 1, EPI_GRU_GATES));
  SkJob jb = sk_base(m, g.ch, rh, ld, g.H, nullptr, 0);
  jb.H = g.H; jb.e0 = hprev; jb.lde0 = ldh; jb.e1 = xc; jb.lde1 = ld; jb.e2 = u; jb.lde2 = ld; jb.o0 = hnew; jb.ldo0 = ld; jb.o3 = c; jb.ldo3 = ld;
  if (out_res) { jb.e3 = xin; jb.lde3 = ldx; jb.o1 = out_res; jb.ldo1 = ld; }
  TRY(run_skinny(st, B, &jb, 1, EPI_GRU_CAND));
  return 0;
}
// What the training kernels of the decoder serve, asked before anything is launched (the step, and taco_train_debug_decoder ahead of its first HIP call)
static int decoder_fwd_check(const taco_model* m, int T_in) {
  const taco_hparams& hp = m->hp;
  const int D = 2 * hp.enc_rnn_size, As = hp.attention_state_size, A = hp.attention_size;
  if (T_in > ATT_MAXT) return fail(TACO_ERR_UNSUPPORTED, "T_in %d > %d", T_in, ATT_MAXT);
  if (!((A % 4 == 0) && A <= ATT_MAXT && A / 4 <= 64 * ATT_NW) || (D % 4) || A > 1024 || D > 1024 || As > 1024)
    return fail(TACO_ERR_UNSUPPORTED, "attention sizes not supported by the training kernels");
  return 0;
}
static size_t attention_bwd_lds(const taco_model* m, int T_in) {
  const int D = 2 * m->hp.enc_rnn_size, A = m->hp.attention_size;
  return (size_t)(2 * ((A + 3) & ~3) + ((D + 3) & ~3) + 5 * ((T_in + 3) & ~3) + ATB_NW * 256) * sizeof(float);
}
static int decoder_bwd_check(const taco_model* m, int T_in) {
  const taco_hparams& hp = m->hp;
  if (attention_bwd_lds(m, T_in) > 160 * 1024 || (hp.attention_state_size % 4) || ((2 * hp.enc_rnn_size) % 4) || (hp.attention_size % 4))
    return fail(TACO_ERR_UNSUPPORTED, "attention sizes not supported by the backward kernel");
  return 0;
}
static int decoder_forward_train(const TrainCtx& x, const float* enc_out, int B, int T_in, int n, const float* teach, float* mel,
                                 float* align_hist, const DecTape& w, bool feed_back, const float* att_init = nullptr,
                                 const float* const* dec_init = nullptr, const float* spk_emb = nullptr) {
  const taco_model* m = x.t->sm; hipStream_t st = x.st;
  const taco_hparams& hp = m->hp;
  const int D = 2 * hp.enc_rnn_size, As = hp.attention_state_size, Hd = hp.dec_rnn_size, A = hp.attention_size;
  const int Mm = hp.num_mels, rM = Mm * hp.reduction_factor, L = hp.dec_layer_num, np = hp.dec_prenet_n;
  TRY(decoder_fwd_check(m, T_in));
  { GemmCall g; g.x = enc_out; g.ldx = D; g.M = B * T_in; g.out = w.keys; g.ldo = A; TRY(run_gemm(m, st, &m->memory_layer, 1, false, g)); }
  const int Wz = std::max(std::max(Mm, As), std::max(Hd, D));
  hipLaunchKernelGGL(k_copy2d, EWGRID((size_t)B * Wz), 0, st, (const float*)nullptr, 0, w.zero, Wz, B, Wz);
  hipLaunchKernelGGL(k_init_align, EWGRID((size_t)B * T_in), 0, st, w.alpha0, B, T_in, hp.attention_type == 2 ? 1 : 0);
  const int ldal = (n + 1) * T_in;
  hipLaunchKernelGGL(k_copy2d, EWGRID((size_t)B * T_in), 0, st, w.alpha0, T_in, w.alpha, ldal, B, T_in);
  HIPCHK(hipGetLastError());
  HIPCHK(zero_async(w.nz, (size_t)n * B * sizeof(int), st));
  const int Pl = hp.dec_prenet[np - 1];
  const int S = simple_S(m), Dc = D + S, Pz = Pl + S;      // 'simple': speaker embedding parked behind ctx and behind the last prenet output
  if (S) {
    if (!spk_emb) return fail(TACO_ERR_ARG, "speaker embedding missing");
    hipLaunchKernelGGL(k_tile_rows, EWGRID((size_t)B * n * S), 0, st, spk_emb, w.ctx, Dc, D, B, n, S);
    hipLaunchKernelGGL(k_tile_rows, EWGRID((size_t)B * n * S), 0, st, spk_emb, w.pz[np - 1], Pz, Pl, B, n, S);
    HIPCHK(hipGetLastError());
  }
  if (const DecPlan dp = decoder_plan(m, B, T_in, n, DEC_TRAIN_FWD); dp.persistent) {      // (the widths of carve_dec_tape's tape256 layout among its terms)
    // the whole teacher-forced loop as ONE persistent launch that also writes the tape (k_decoder_xcd<RG, true>, taco_decoder_xcd.h);
    // rnn_decoder_test_mode (feed_back): the same launch, the step's own last frame exchanged in place of the teacher's
    DxArgs ta; memset(&ta, 0, sizeof ta);
    ta.teacher = feed_back ? nullptr : teach; ta.own_fb = feed_back ? 1 : 0; ta.tape = w.tape256; ta.tstride = w.tstride; ta.tp_p2 = w.pz[np - 1]; ta.ld_p2 = Pz; ta.tp_ctx = w.ctx; ta.ld_ctx = Dc;
    ta.tp_e = w.g_e; ta.tp_alpha = w.alpha;
    x.s->dec_paths |= DEC_PATH_FWD_PERSISTENT | (unsigned)dp.rg << DEC_PATH_FWD_RG_SHIFT;
    return dx_launch(m, st, dp, enc_out, SpkSel(), spk_emb, nullptr, B, T_in, n, nullptr, mel, align_hist, nullptr, 0, w.keys, w.nz, w.dx, w.rowbias,
                     att_init, dec_init ? dec_init[0] : nullptr, dec_init ? dec_init[1] : nullptr, &ta);
  }
  x.s->dec_paths |= DEC_PATH_FWD_STAGES;
  for (int t = 0; t < n; ++t) {
    // helpers.py:44,66,70-72: previous teacher frame; rnn_decoder_test_mode (:63-64): last of the r frames the decoder just emitted
    const float* frame = (t == 0) ? w.zero : (feed_back ? mel + (size_t)(t - 1) * rM + (rM - Mm) : teach + (size_t)(t - 1) * Mm);
    const int ldf = (t == 0) ? Mm : (feed_back ? n * rM : n * Mm);
    const float* cprev = (t == 0) ? w.zero : w.ctx + (size_t)(t - 1) * Dc; const int ldcp = (t == 0) ? D : n * Dc;
    for (int i = 0; i < np; ++i) {
      const int P = hp.dec_prenet[i], Pw = (i == np - 1) ? Pz : P;      // row width of this layer's tape
      SkJob j = (i == 0) ? sk_linear(m, m->dec_prenet[0], frame, ldf, Mm, cprev, ldcp, ACT_RELU, w.pz[0] + (size_t)t * Pw, n * Pw)
                         : sk_linear(m, m->dec_prenet[i], w.pz[i - 1] + (size_t)t * hp.dec_prenet[i - 1], n * hp.dec_prenet[i - 1],
                                     hp.dec_prenet[i - 1], nullptr, 0, ACT_RELU, w.pz[i] + (size_t)t * Pw, n * Pw);
      TRY(run_skinny(st, B, &j, 1));
    }
    const float* hAp = (t == 0) ? (att_init ? att_init : w.zero) : w.hA + (size_t)(t - 1) * As; const int ldhA = (t == 0) ? As : n * As;   // tacotron.py:183-197
    const size_t oa = (size_t)t * As;
    TRY(gru_cell_train(m, st, m->att_gru, B, w.pz[np - 1] + (size_t)t * Pz, n * Pz, hAp, ldhA, w.hA + oa, w.rhA + oa, w.uA + oa, w.xcA + oa,
                       w.rA + oa, w.cA + oa, n * As, nullptr));
    { AttnArgs a; memset(&a, 0, sizeof a);
      a.hq = w.hA + oa; a.ldhq = n * As; a.wq = AP(m, m->raw_wq); a.As = As; a.keys = w.keys; a.values = enc_out; a.v = AP(m, m->att_v); a.battn = AP(m, m->att_b);
      a.score_bias = AP(m, m->att_sb); a.align = w.alpha + (size_t)(t + 1) * T_in; a.align_prev = w.alpha + (size_t)t * T_in; a.ldalign = ldal;
      a.hist = align_hist; a.ctx = w.ctx + (size_t)t * Dc; a.ldctx = n * Dc;
      a.q_out = w.g_q + (size_t)t * A; a.ldq_out = n * A; a.e_out = w.g_e + (size_t)t * T_in; a.lde_out = n * T_in;
      a.T_in = T_in; a.A = A; a.D = D; a.type = hp.attention_type; a.step = t; a.n_steps = n;
      hipLaunchKernelGGL(k_attention, dim3(B), dim3(64 * ATT_NW), 0, st, a);
      HIPCHK(hipGetLastError()); }
    { SkJob j = sk_linear(m, m->concat_proj, w.hA + oa, n * As, As, w.ctx + (size_t)t * Dc, n * Dc, ACT_NONE, w.o[0] + (size_t)t * Hd, n * Hd);
      TRY(run_skinny(st, B, &j, 1)); }
    const size_t oh = (size_t)t * Hd;
    for (int i = 0; i < L; ++i) {
      const float* hp_ = (t == 0) ? ((dec_init && dec_init[i]) ? dec_init[i] : w.zero) : w.h[i] + (size_t)(t - 1) * Hd; const int ldhp = (t == 0) ? Hd : n * Hd;
      TRY(gru_cell_train(m, st, m->dec_gru[i], B, w.o[i] + oh, n * Hd, hp_, ldhp, w.h[i] + oh, w.rh[i] + oh, w.u[i] + oh, w.xc[i] + oh,
                         w.r[i] + oh, w.c[i] + oh, n * Hd, w.o[i + 1] + oh));
    }
    { SkJob j = sk_linear(m, m->frame_proj, w.o[L] + oh, n * Hd, Hd, nullptr, 0, ACT_NONE, mel + (size_t)t * rM, n * rM);
      j.o2 = reinterpret_cast<float*>(w.nz + (size_t)t * B);
      TRY(run_skinny(st, B, &j, 1)); }
  }
  return 0;
}

static SkJob sk_T(const taco_model* m, const SkW& wT, const float* dy, int lddy, float* out, int ldo) {
  return sk_linear(m, wT, dy, lddy, wT.K, nullptr, 0, ACT_NONE, out, ldo);
}
// one GRUCell backward: dout [B,H] (+carry) -> dx [B,I] (+dres), new carry; tape slices at step t.
// skip_a: the 'a' part (dht, dcp, dgp_u) was already produced by the k_gru_bwd_ca of the cell above.
// next: when given, the 'c' part also runs the 'a' part of the cell below (k_gru_bwd_ca).  relu_of: mask dx by relu_of > 0.
struct GruBwdNext { const float* carry; const float* u; const float* c; const float* hprev; float* dcp; float* dgp; int ldh; };
static int gru_cell_backward(const TrainCtx& x, const GruT& gt, int B, const float* dout, int lddo, float* carry, bool add_carry,
                             const float* u, const float* c, const float* r, const float* hprev, int ld, float* g_dcp, float* g_dgp,
                             const float* dres, int lddres, float* dx, int lddx, const DecTape& w, bool skip_a = false,
                             const GruBwdNext* next = nullptr, const float* relu_of = nullptr, int ldrelu = 0, int ldh = -1) {
  if (ldh < 0) ldh = ld;
  const taco_model* m = x.t->sm; hipStream_t st = x.st;
  const int H = gt.H, I = gt.I, W = I + H;
  if (!skip_a)
    hipLaunchKernelGGL(k_gru_bwd_a, EWGRID((size_t)B * H), 0, st, dout, lddo, add_carry ? carry : (const float*)nullptr, u, ld, c, ld, hprev, ldh,
                       w.dht, g_dcp, ld, g_dgp, 2 * ld, B, H);
  { SkJob j = sk_T(m, gt.cT, g_dcp, ld, w.tmp1, W); TRY(run_skinny(st, B, &j, 1)); }
  hipLaunchKernelGGL(k_gru_bwd_b, EWGRID((size_t)B * H), 0, st, w.tmp1, W, I, hprev, ldh, r, ld, u, ld, w.dht, g_dgp, 2 * ld, w.dhp, B, H);
  { SkJob j = sk_T(m, gt.gT, g_dgp, 2 * ld, w.tmp2, W); TRY(run_skinny(st, B, &j, 1)); }
  if (next)   // note: dht of the lower cell overwrites w.dht -- this cell's dht was consumed by its 'b' part above
    hipLaunchKernelGGL(k_gru_bwd_ca, EWGRID((size_t)B * W), 0, st, w.tmp1, w.tmp2, W, I, dres, lddres, w.dhp, dx, lddx, carry, B, H,
                       next->carry, next->u, ld, next->c, ld, next->hprev, next->ldh, w.dht, next->dcp, ld, next->dgp, 2 * ld);
  else
    hipLaunchKernelGGL(k_gru_bwd_c, EWGRID((size_t)B * W), 0, st, w.tmp1, w.tmp2, W, I, dres, lddres, w.dhp, dx, lddx, carry, B, H, relu_of, ldrelu);
  HIPCHK(hipGetLastError());
  return 0;
}
static int gru_weight_grads(const TrainCtx& x, const std::string& name, int I, int H, const float* xin, int ldx, const float* hseq,
                            const float* rh, const float* g_dgp, const float* g_dcp, int R, int n) {
  float* Gg = x.g(name + "/gates/kernel"); float* Gc = x.g(name + "/candidate/kernel");
  TRY(run_wgrad(x, xin, nullptr, ldx, g_dgp, 2 * H, Gg, 2 * H, R, 0, I, 2 * H));
  TRY(run_wgrad(x, hseq, nullptr, H, g_dgp, 2 * H, Gg + (size_t)I * 2 * H, 2 * H, R, n, H, 2 * H, 1, 1));   // previous state = one step earlier
  TRY(run_wgrad(x, xin, nullptr, ldx, g_dcp, H, Gc, H, R, 0, I, H));
  TRY(run_wgrad(x, rh, nullptr, H, g_dcp, H, Gc + (size_t)I * H, H, R, 0, H, H));
  TRY(run_colsum(x, g_dgp, 2 * H, nullptr, 0, nullptr, nullptr, x.g(name + "/gates/bias"), nullptr, R, 2 * H, 0));
  TRY(run_colsum(x, g_dcp, H, nullptr, 0, nullptr, nullptr, x.g(name + "/candidate/bias"), nullptr, R, H, 0));
  return 0;
}
static int decoder_backward(const TrainCtx& x, const float* enc_out, int B, int T_in, int n, const float* teach, const float* dmel,
                            float* denc, const DecTape& w, const float* att_init = nullptr, const float* const* dec_init = nullptr,
                            float* d_att_init = nullptr, float* const* d_dec_init = nullptr, float* dspk = nullptr) {
  const taco_model* m = x.t->sm; hipStream_t st = x.st;
  const TrainPacks& tp = x.t->tp;
  const taco_hparams& hp = m->hp;
  const int D = 2 * hp.enc_rnn_size, As = hp.attention_state_size, Hd = hp.dec_rnn_size, A = hp.attention_size;
  const int Mm = hp.num_mels, rM = Mm * hp.reduction_factor, L = hp.dec_layer_num, np = hp.dec_prenet_n, Pl = hp.dec_prenet[np - 1];
  const int ldal = (n + 1) * T_in, R = B * n;
  const int S = simple_S(m), Dc = D + S, Pz = Pl + S;
  if (S && !dspk) return fail(TACO_ERR_ARG, "speaker-embedding gradient buffer missing");
  { ZeroBatch zb(st);               // the loop's accumulators: one fill launch
    HIPCHK(zb.add(w.dkeys, (size_t)B * T_in * A * sizeof(float)));
    HIPCHK(zb.add(w.dvalues, (size_t)B * T_in * D * sizeof(float)));
    HIPCHK(zb.add(w.dv_acc, (size_t)B * A * sizeof(float)));
    HIPCHK(zb.add(w.dsb_acc, (size_t)B * sizeof(float)));
    HIPCHK(zb.add(w.dalpha, (size_t)B * T_in * sizeof(float)));
    HIPCHK(zb.add(w.dctx, (size_t)B * D * sizeof(float)));
    HIPCHK(zb.add(w.dhA, (size_t)B * As * sizeof(float)));
    for (int i = 0; i < L; ++i) HIPCHK(zb.add(w.dh[i], (size_t)B * Hd * sizeof(float)));
    HIPCHK(zb.run()); }
  const size_t attn_lds = attention_bwd_lds(m, T_in);
  TRY(decoder_bwd_check(m, T_in));
  // the whole loop as ONE persistent launch (k_decoder_bwd_xcd, taco_decoder_bwd_xcd.h) when the forward left its tape in that
  // kernel's layout; the launch-per-stage loop below is the general path (other widths, 'simple', more than 64 rows)
  const DecPlan bp = decoder_plan(m, B, T_in, n, DEC_TRAIN_BWD);
  const bool persistent = x.t->bptt_persistent && bp.persistent;
  x.t->sm->last_bptt = persistent ? 1 : 0;
  if (persistent) {
    DbArgs a; memset(&a, 0, sizeof a);
    a.tape = w.tape256; a.tstride = w.tstride; a.tp_p2 = w.pz[1]; a.ld_p2 = Pz; a.tp_e = w.g_e; a.tp_alpha = w.alpha;
    a.keys = w.keys; a.values = enc_out;
    // d o2 of every step does not depend on the recurrence: ONE GEMM [B n, r M] x [r M, 256] ahead of the loop
    TRY(run_dgrad(x, tp.frame_d, dmel, rM, R, 0, w.g_do2, Hd));
    a.g_do2 = w.g_do2;
    a.h_att0 = att_init; a.h10 = dec_init ? dec_init[0] : nullptr; a.h20 = dec_init ? dec_init[1] : nullptr;
    a.g_dcp2 = w.g_dcp[1]; a.g_dgp2 = w.g_dgp[1]; a.g_dcp1 = w.g_dcp[0]; a.g_dgp1 = w.g_dgp[0]; a.g_do0 = w.g_do0;
    a.g_dcpA = w.g_dcpA; a.g_dgpA = w.g_dgpA; a.g_dz1 = w.g_dz[0]; a.g_dz2 = w.g_dz[1]; a.g_dq = w.g_dq; a.g_de = w.g_de; a.g_dctx = w.g_dctx;
    a.d_att_init = d_att_init; a.d_h10 = d_dec_init ? d_dec_init[0] : nullptr; a.d_h20 = d_dec_init ? d_dec_init[1] : nullptr;
    a.dsb_acc = w.dsb_acc;
    x.s->dec_paths |= DEC_PATH_BWD_PERSISTENT | (unsigned)bp.rg << DEC_PATH_BWD_RG_SHIFT;
    TRY(dbx_launch(m, st, bp, a, B, T_in, n, w.dx));
    if (S) {
      // 'simple': d speaker embedding = sum over steps of [d o0 . Wcc^T]_spk + [d c_pre(att) . Wc^T + d gates(att) . Wg^T]_spk.  Linear in the
      // pre-activation gradients: sum those over time first, then ONE transposed product each (the per-stage chain adds step by step).
      hipLaunchKernelGGL(k_time_sum, EWGRID((size_t)B * Hd), 0, st, (const float*)w.g_do0, w.dht, B, n, Hd);
      { SkJob j = sk_T(m, tp.concat_T, w.dht, Hd, w.dIn, As + Dc); TRY(run_skinny(st, B, &j, 1)); }
      hipLaunchKernelGGL(k_add2d, EWGRID((size_t)B * S), 0, st, dspk, S, w.dIn + As + D, As + Dc, B, S);
      hipLaunchKernelGGL(k_time_sum, EWGRID((size_t)B * As), 0, st, (const float*)w.g_dcpA, w.dht, B, n, As);
      { SkJob j = sk_T(m, tp.att.cT, w.dht, As, w.tmp1, Pz + As); TRY(run_skinny(st, B, &j, 1)); }
      hipLaunchKernelGGL(k_add2d, EWGRID((size_t)B * S), 0, st, dspk, S, w.tmp1 + Pl, Pz + As, B, S);
      hipLaunchKernelGGL(k_time_sum, EWGRID((size_t)B * 2 * As), 0, st, (const float*)w.g_dgpA, w.dpz, B, n, 2 * As);
      { SkJob j = sk_T(m, tp.att.gT, w.dpz, 2 * As, w.tmp2, Pz + As); TRY(run_skinny(st, B, &j, 1)); }
      hipLaunchKernelGGL(k_add2d, EWGRID((size_t)B * S), 0, st, dspk, S, w.tmp2 + Pl, Pz + As, B, S);
      HIPCHK(hipGetLastError());
    }
  }
  if (!persistent) x.s->dec_paths |= DEC_PATH_BWD_STAGES;
  for (int t = n - 1; t >= 0 && !persistent; --t) {
    const size_t oh = (size_t)t * Hd, oa = (size_t)t * As;
    { SkJob j = sk_T(m, tp.frame_T, dmel + (size_t)t * rM, n * rM, w.do_[L], Hd); TRY(run_skinny(st, B, &j, 1)); }
    for (int i = L - 1; i >= 0; --i) {
      auto hp_of = [&](int l) -> const float* { return (t == 0) ? ((dec_init && dec_init[l]) ? dec_init[l] : nullptr) : w.h[l] + (size_t)(t - 1) * Hd; };
      const float* hprev = hp_of(i);
      const int ldh = (t == 0) ? Hd : n * Hd;
      float* dx = (i == 0) ? w.g_do0 + oh : w.do_[i]; const int lddx = (i == 0) ? n * Hd : Hd;
      GruBwdNext nx; const GruBwdNext* pnx = nullptr;
      if (i > 0) {   // the cell below consumes this dx at once: its 'a' part rides in this cell's 'c' launch
        nx.carry = w.dh[i - 1]; nx.u = w.u[i - 1] + oh; nx.c = w.c[i - 1] + oh; nx.hprev = hp_of(i - 1); nx.ldh = ldh;
        nx.dcp = w.g_dcp[i - 1] + oh; nx.dgp = w.g_dgp[i - 1] + 2 * oh; pnx = &nx;
      }
      TRY(gru_cell_backward(x, tp.dec[i], B, w.do_[i + 1], Hd, w.dh[i], true, w.u[i] + oh, w.c[i] + oh, w.r[i] + oh, hprev, n * Hd,
                            w.g_dcp[i] + oh, w.g_dgp[i] + 2 * oh, w.do_[i + 1], Hd, dx, lddx, w, i < L - 1, pnx, nullptr, 0, ldh));
    }
    // concat projection: [h_att | ctx] <- d o0; the attention backward adds the two halves to dhA / dctx itself
    { SkJob j = sk_T(m, tp.concat_T, w.g_do0 + oh, n * Hd, w.dIn, As + Dc); TRY(run_skinny(st, B, &j, 1)); }
    if (S) hipLaunchKernelGGL(k_add2d, EWGRID((size_t)B * S), 0, st, dspk, S, w.dIn + As + D, As + Dc, B, S);
    { AttnBArgs a; memset(&a, 0, sizeof a);
      a.q = w.g_q + (size_t)t * A; a.ldq = n * A; a.e = w.g_e + (size_t)t * T_in; a.lde = n * T_in; a.wqT = AP(m, tp.wqT);
      a.keys = w.keys; a.values = enc_out; a.v = AP(m, m->att_v); a.score_bias = AP(m, m->att_sb); a.battn = AP(m, m->att_b);
      a.alpha = w.alpha + (size_t)(t + 1) * T_in; a.alpha_prev = w.alpha + (size_t)t * T_in; a.ldal = ldal;
      a.dctx = w.dctx; a.lddctx = D; a.dctx_out = w.g_dctx + (size_t)t * D; a.lddco = n * D; a.dalpha = w.dalpha;
      a.de_out = w.g_de + (size_t)t * T_in; a.ldde = n * T_in; a.dsb_acc = w.dsb_acc;
      a.dq = w.g_dq + (size_t)t * A; a.lddq = n * A; a.dhq = w.dhA; a.lddhq = As; a.T_in = T_in; a.A = A; a.D = D; a.As = As; a.type = hp.attention_type;
      a.cat = w.dIn; a.ldcat = As + Dc;
      hipLaunchKernelGGL(k_attention_bwd, dim3(B), dim3(64 * ATB_NW), attn_lds, st, a);
      HIPCHK(hipGetLastError()); }
    { const float* hprev = (t == 0) ? att_init : w.hA + (size_t)(t - 1) * As;
      // dx of the attention GRU = gradient of the (ReLU) prenet output: masked here, written straight to the tape
      if (!S) {
        TRY(gru_cell_backward(x, tp.att, B, w.dhA, As, w.dhA, false, w.uA + oa, w.cA + oa, w.rA + oa, hprev, n * As, w.g_dcpA + oa,
                              w.g_dgpA + 2 * oa, nullptr, 0, w.g_dz[np - 1] + (size_t)t * Pl, n * Pl, w, false, nullptr,
                              w.pz[np - 1] + (size_t)t * Pl, n * Pl, (t == 0) ? As : n * As));
      } else {   // 'simple': the cell input is [prenet output | speaker embedding]: split its gradient
        TRY(gru_cell_backward(x, tp.att, B, w.dhA, As, w.dhA, false, w.uA + oa, w.cA + oa, w.rA + oa, hprev, n * As, w.g_dcpA + oa,
                              w.g_dgpA + 2 * oa, nullptr, 0, w.dpz, Pz, w, false, nullptr, nullptr, 0, (t == 0) ? As : n * As));
        hipLaunchKernelGGL(k_relu_bwd, EWGRID((size_t)B * Pl), 0, st, w.dpz, Pz, w.pz[np - 1] + (size_t)t * Pz, n * Pz, w.g_dz[np - 1] + (size_t)t * Pl, n * Pl, B, Pl);
        hipLaunchKernelGGL(k_add2d, EWGRID((size_t)B * S), 0, st, dspk, S, w.dpz + Pl, Pz, B, S);
      } }
    for (int i = np - 1; i >= 1; --i) {   // prenet layers np..2: d z_{i-1} = (d z_i . W_i^T) masked by the ReLU of layer i-1 (skinny epilogue)
      const int P = hp.dec_prenet[i], Pm = hp.dec_prenet[i - 1];
      SkJob j = sk_T(m, tp.decpre_T[i], w.g_dz[i] + (size_t)t * P, n * P, w.g_dz[i - 1] + (size_t)t * Pm, n * Pm);
      j.e0 = w.pz[i - 1] + (size_t)t * Pm; j.lde0 = n * Pm;
      TRY(run_skinny(st, B, &j, 1));
    }
    // layer 1: only the context columns of its input carry a gradient (the frame is the teacher's): d ctx(t-1) = d z_0 . W1[Mm:,:]^T
    { SkJob j = sk_T(m, tp.decpre0_ctxT, w.g_dz[0] + (size_t)t * hp.dec_prenet[0], n * hp.dec_prenet[0], w.dctx, D); TRY(run_skinny(st, B, &j, 1)); }
    HIPCHK(hipGetLastError());
  }
  // gradients of the initial states (deepvoice: they come from the speaker layers) = the carries left after step 0
  if (d_att_init && !persistent) hipLaunchKernelGGL(k_copy2d, EWGRID((size_t)B * As), 0, st, w.dhA, As, d_att_init, As, B, As);
  for (int i = 0; i < L && !persistent; ++i)
    if (d_dec_init && d_dec_init[i]) hipLaunchKernelGGL(k_copy2d, EWGRID((size_t)B * Hd), 0, st, w.dh[i], Hd, d_dec_init[i], Hd, B, Hd);
  HIPCHK(hipGetLastError());
  // first-step terms of the recurrent kernels' gates rows: the state before step 0 is the initial state, not a tape row
  if (att_init) TRY(run_wgrad(x, att_init, nullptr, As, w.g_dgpA, n * 2 * As, x.g("decoder/attention_gru/gates/kernel") + (size_t)Pz * 2 * As, 2 * As, B, 0, As, 2 * As));
  for (int i = 0; i < L; ++i)
    if (dec_init && dec_init[i])
      TRY(run_wgrad(x, dec_init[i], nullptr, Hd, w.g_dgp[i], n * 2 * Hd, x.g("decoder/gru_" + std::to_string(i + 1) + "/gates/kernel") + (size_t)Hd * 2 * Hd, 2 * Hd, B, 0, Hd, 2 * Hd));
  // ---- weight gradients, hoisted over all steps: rows (b, t) of the [B, n, .] tapes ----
  WgRegion wgr(x);           // ~50 small products over final tapes: a few group launches (ended before d values is read below)
  TRY(run_wgrad(x, w.o[L], nullptr, Hd, dmel, rM, x.g("decoder/frame_projection/kernel"), rM, R, 0, Hd, rM));
  TRY(run_colsum(x, dmel, rM, nullptr, 0, nullptr, nullptr, x.g("decoder/frame_projection/bias"), nullptr, R, rM, 0));
  for (int i = 0; i < L; ++i)
    TRY(gru_weight_grads(x, "decoder/gru_" + std::to_string(i + 1), Hd, Hd, w.o[i], Hd, w.h[i], w.rh[i], w.g_dgp[i], w.g_dcp[i], R, n));
  { float* Gk = x.g("decoder/concat_projection/kernel");
    TRY(run_wgrad(x, w.hA, nullptr, As, w.g_do0, Hd, Gk, Hd, R, 0, As, Hd));
    TRY(run_wgrad(x, w.ctx, nullptr, Dc, w.g_do0, Hd, Gk + (size_t)As * Hd, Hd, R, 0, Dc, Hd));     // context (+ speaker) rows
    TRY(run_colsum(x, w.g_do0, Hd, nullptr, 0, nullptr, nullptr, x.g("decoder/concat_projection/bias"), nullptr, R, Hd, 0)); }
  TRY(run_wgrad(x, w.hA, nullptr, As, w.g_dq, A, x.g("attention/query_layer/kernel"), A, R, 0, As, A));
  TRY(gru_weight_grads(x, "decoder/attention_gru", Pz, As, w.pz[np - 1], Pz, w.hA, w.rhA, w.g_dgpA, w.g_dcpA, R, n));
  for (int i = np - 1; i >= 0; --i) {
    const int P = hp.dec_prenet[i];
    const std::string nm = "decoder/prenet/dense_" + std::to_string(i + 1);
    float* Gk = x.g(nm + "/kernel");
    if (i > 0) TRY(run_wgrad(x, w.pz[i - 1], nullptr, hp.dec_prenet[i - 1], w.g_dz[i], P, Gk, P, R, 0, hp.dec_prenet[i - 1], P));
    else {   // input = concat(previous teacher frame, previous context): both one step earlier, zero at t = 0
      TRY(run_wgrad(x, teach, nullptr, Mm, w.g_dz[0], P, Gk, P, R, n, Mm, P, 1, 1));
      TRY(run_wgrad(x, w.ctx, nullptr, Dc, w.g_dz[0], P, Gk + (size_t)Mm * P, P, R, n, D, P, 1, 1));
    }
    TRY(run_colsum(x, w.g_dz[i], P, nullptr, 0, nullptr, nullptr, x.g(nm + "/bias"), nullptr, R, P, 0));
  }
  { const bool vn = hp.attention_type == 1;   // bah_norm: the kernels see v_hat = g*v/|v|; its gradient is mapped back to v and g below
    float* dvdst = vn ? w.dv_acc : x.g("attention/attention_v");
    if (vn) HIPCHK(zero_async(w.dv_acc, (size_t)A * sizeof(float), st));
    AttnKArgs k; k.keys = w.keys; k.q = w.g_q; k.de = w.g_de; k.v = AP(m, m->att_v); k.battn = AP(m, m->att_b); k.dkeys = w.dkeys; k.dv = dvdst;
    k.T_in = T_in; k.A = A; k.n = n;
    const int nj = cdiv(T_in, ATK_J);
    k.part = (x.s->det && (size_t)B * nj * A <= x.s->det_cap) ? x.s->det : nullptr;
    hipLaunchKernelGGL(k_attention_keys_bwd, dim3(cdiv(A, 256), nj, B), dim3(256), 0, st, k);
    if (k.part) hipLaunchKernelGGL(k_rows_reduce, EWGRID(A), 0, st, (const float*)k.part, B * nj, A, dvdst);
    if (vn) {
      hipLaunchKernelGGL(k_vnorm_bwd, dim3(1), dim3(256), 0, st, x.p("attention/attention_v"), x.p("attention/attention_g"), w.dv_acc,
                         x.g("attention/attention_v"), x.g("attention/attention_g"), A);
      TRY(run_colsum(x, w.g_dq, A, nullptr, 0, nullptr, nullptr, x.g("attention/attention_b"), nullptr, R, A, 0));   // b enters like the query
    }
    HIPCHK(hipGetLastError()); }
  for (int b = 0; b < B; ++b)    // d values[b] = alpha[b]^T . dctx[b]  ([T_in x n] . [n x D])
    TRY(run_wgrad(x, w.alpha + ((size_t)b * (n + 1) + 1) * T_in, nullptr, T_in, w.g_dctx + (size_t)b * n * D, D,
                  w.dvalues + (size_t)b * T_in * D, D, n, 0, T_in, D));
  if (hp.attention_type == 2) { hipLaunchKernelGGL(k_sum_all, dim3(1), dim3(256), 0, st, w.dsb_acc, B, x.g("attention/attention_score_bias")); HIPCHK(hipGetLastError()); }
  TRY(run_wgrad(x, enc_out, nullptr, D, w.dkeys, A, x.g("attention/memory_layer/kernel"), A, B * T_in, 0, D, A));
  TRY(wgr.end());            // d values (the per-row products above) is an operand of the data gradient below
  TRY(run_dgrad(x, tp.mem_d, w.dkeys, A, B * T_in, 0, denc, D, w.dvalues, D));
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The two ends of the step and the seams between its blocks, as the step calls them and as the test hooks taco_train_debug_front /
// taco_train_debug_head (include/taco_debug.h) call them alone.
// ---------------------------------------------------------------------------------------------------------------
// Input end, forward: embedding gather + encoder prenet -> pre[i] [B*T_in, enc_prenet[i]]; the speaker rows of 'simple' -> spk.emb; the speaker
// vectors of deepvoice (before_highway, encoder / attention / decoder initial states; tacotron.py:52-79) -> spk.vec[]
static int front_forward_train(const TrainCtx& x, const int* ids, const int* speaker_id, int B, int T_in, float* const* pre, const SpkWs& spk) {
  taco_model* m = x.t->sm; hipStream_t st = x.st;
  const taco_hparams& hp = m->hp;
  const int Me = B * T_in;
  const float* cur = x.p("embedding"); int curd = hp.embedding_size;
  for (int i = 0; i < hp.enc_prenet_n; ++i) {
    GemmCall g; g.x = cur; g.ldx = curd; g.gather = (i == 0) ? ids : nullptr; g.M = Me; g.act = ACT_RELU; g.out = pre[i]; g.ldo = hp.enc_prenet[i];
    TRY(run_gemm(m, st, &m->enc_prenet[i], 1, false, g));
    cur = pre[i]; curd = hp.enc_prenet[i];
  }
  const bool dv = is_deepvoice(m), simple = is_simple(m);
  const int S = hp.speaker_embedding_size;
  if ((dv || simple) && !speaker_id) return fail(TACO_ERR_ARG, "speaker_id required for a multi-speaker model");
  if (simple) {      // the embedding row of every utterance (tacotron.py:47-50); concatenated in the decoder and the linear head
    hipLaunchKernelGGL(k_gather_rows, EWGRID((size_t)B * S), 0, st, AP(m, m->spk_emb), speaker_id, B, S, spk.emb);
    HIPCHK(hipGetLastError());
  }
  if (dv) TRY(spk_forward(m, st, spk_ids(speaker_id), B, spk));       // before_highway, encoder / attention / decoder initial states (tacotron.py:52-79)
  return 0;
}
// teacher inputs: every r-th target frame (helpers.py:44): teach[b, t] = mel_targets[b, t*r + r-1]
static int teacher_frames(const TrainCtx& x, const float* mel_tgt, int B, int n, float* teach) {
  const taco_hparams& hp = x.t->sm->hp;
  const int r = hp.reduction_factor, Mm = hp.num_mels;
  hipLaunchKernelGGL(k_copy2d, EWGRID((size_t)B * n * Mm), 0, x.st, mel_tgt + (size_t)(r - 1) * Mm, r * Mm, teach, Mm, B * n, Mm);
  HIPCHK(hipGetLastError());
  return 0;
}
// Output end, forward: the linear head over the post CBHG's output [B*T_out, 2*post_rnn_size] -> lin [B*T_out, num_freq] (spk_emb [B, S]: the speaker
// rows of 'simple', else null; linrv [B, num_freq] their scratch), then add_loss (tacotron.py:274-302) -> d_losses[4] (nullable: no loss)
static int head_forward_train(const TrainCtx& x, const float* post_out, const float* mel, const float* spk_emb, const float* mel_tgt, const float* lin_tgt,
                              const float* loss_coeff, int B, int T_out, int prioritize_loss, int sample_rate, float* lin, float* linrv, float* d_losses,
                              float* losspart) {
  taco_model* m = x.t->sm; hipStream_t st = x.st;
  const taco_hparams& hp = m->hp;
  const int Mm = hp.num_mels, F = hp.num_freq, S = hp.speaker_embedding_size, Mp = B * T_out;
  { GemmCall g; g.x = post_out; g.ldx = 2 * hp.post_rnn_size; g.M = Mp; g.out = lin; g.ldo = F;
    if (spk_emb) {    // linear(concat(tiled speaker_embed, post)) (tacotron.py:226-235): the speaker rows give one vector per utterance
      SkJob j = sk_linear(m, m->lin_spk, spk_emb, S, S, nullptr, 0, ACT_NONE, linrv, F);
      TRY(run_skinny(st, B, &j, 1));
      g.T = T_out; g.rowvec = linrv; g.ldrv = F;
    }
    TRY(run_gemm(m, st, &m->linear, 1, false, g)); }
  // ---- loss (tacotron.py:274-302) ----
  if (d_losses) TRY(taco_loss_f32((void*)st, mel, mel_tgt, lin, lin_tgt, loss_coeff, B, T_out, Mm, F, prioritize_loss, sample_rate, d_losses,
                                  losspart, (size_t)TR_MAXBLK * 8 * sizeof(double)));
  return 0;
}
// Output end, backward: d loss / d mel -> dmel and d loss / d linear -> dlin (the two L1 gradients, loss_coeff and the priority band included), the
// gradients of linear/kernel and linear/bias, dpost = dlin . W^T; 'simple' (spk_emb given): the speaker rows of linear/kernel and the head's share of
// d(speaker rows) -> dspk_emb [B, S] (overwritten), over the time-summed dlin (dlin_sum [B, num_freq])
static int head_backward(const TrainCtx& x, const float* post_out, const float* mel, const float* lin, const float* spk_emb, const float* mel_tgt,
                         const float* lin_tgt, const float* loss_coeff, int B, int T_out, int prioritize_loss, int sample_rate, float* dmel, float* dlin,
                         float* dlin_sum, float* dspk_emb, float* dpost) {
  const taco_train* t = x.t; taco_model* m = t->sm; hipStream_t st = x.st;
  const taco_hparams& hp = m->hp;
  const int Mm = hp.num_mels, F = hp.num_freq, S = hp.speaker_embedding_size, Mp = B * T_out;
  const bool simple = spk_emb != nullptr;
  int c_lo = 0, c_hi = 0; float s_lin = 1.0f / ((float)Mp * F), s_band = 0.f;
  if (prioritize_loss) {
    loss_band(sample_rate, F, &c_lo, &c_hi);      // clamped to the bins that exist, as the reference's slice is
    s_lin = 0.5f / ((float)Mp * F); s_band = 0.5f / ((float)Mp * std::max(c_hi - c_lo, 1));
  }
  hipLaunchKernelGGL(k_l1_grad, EWGRID((size_t)Mp * Mm), 0, st, mel, mel_tgt, loss_coeff, Mp, T_out, Mm, 1.0f / ((float)Mp * Mm), 0, 0, 0.f, dmel);
  hipLaunchKernelGGL(k_l1_grad, EWGRID((size_t)Mp * F), 0, st, lin, lin_tgt, loss_coeff, Mp, T_out, F, s_lin, c_lo, c_hi, s_band, dlin);
  HIPCHK(hipGetLastError());
  const int Hp2 = 2 * hp.post_rnn_size;
  TRY(run_wgrad(x, post_out, nullptr, Hp2, dlin, F, x.g("linear/kernel") + (simple ? (size_t)S * F : 0), F, Mp, 0, Hp2, F));
  if (simple) {      // speaker rows of the head: the embedding is constant over time, so they see the time-summed gradient
    HIPCHK(zero_async(dspk_emb, (size_t)B * S * sizeof(float), st));
    hipLaunchKernelGGL(k_time_sum, EWGRID((size_t)B * F), 0, st, dlin, dlin_sum, B, T_out, F);
    HIPCHK(hipGetLastError());
    TRY(run_wgrad(x, spk_emb, nullptr, S, dlin_sum, F, x.g("linear/kernel"), F, B, 0, S, F));
    SkJob j = sk_T(m, t->tp.lin_spk_T, dlin_sum, F, dspk_emb, S);
    TRY(run_skinny(st, B, &j, 1));
  }
  TRY(run_colsum(x, dlin, F, nullptr, 0, nullptr, nullptr, x.g("linear/bias"), nullptr, Mp, F, 0));
  return run_dgrad(x, t->tp.lin_d, dlin, F, Mp, 0, dpost, Hp2);
}
// ... and behind the post CBHG's backward: dmel += dmel_post, the gradient the post-net hands back to the decoder's frames
static int head_backward_join(const TrainCtx& x, float* dmel, const float* dmel_post, int B, int T_out) {
  const int Mm = x.t->sm->hp.num_mels, Mp = B * T_out;
  hipLaunchKernelGGL(k_add2d, EWGRID((size_t)Mp * Mm), 0, x.st, dmel, Mm, dmel_post, Mm, Mp, Mm);
  HIPCHK(hipGetLastError());
  return 0;
}
// 'simple': what the decoder and the head hand back for the speaker rows, dspk_emb [B, S] -> the gradient of speaker_embedding
static int speaker_rows_backward(const TrainCtx& x, const float* dspk_emb, const int* speaker_id, int B) {
  const taco_hparams& hp = x.t->sm->hp;
  run_embed_bwd(x, dspk_emb, speaker_id, x.g("speaker_embedding"), B, hp.speaker_embedding_size, hp.num_speakers);
  HIPCHK(hipGetLastError());
  return 0;
}
// Input end, backward.  deepvoice: the speaker conditioning (tacotron.py:52-79) from dvec[i], the gradients of the speaker vectors that the encoder
// CBHG and the decoder left (S = 1: straight into the tables; else through softsign and the dense layers into speaker_embedding; dspk_emb [B, S],
// dzs [B, widest vector] and tmp [B, S] are scratch).  Then the encoder prenet from dpre[last] (in place) down to demb, and the embedding's gradient.
static int front_backward(const TrainCtx& x, const int* ids, const int* speaker_id, int B, int T_in, float* const* pre, float* const* dpre_of, float* demb,
                          const SpkWs& spk, const float* const* dvec, float* dspk_emb, float* dzs, float* tmp) {
  const taco_train* t = x.t; taco_model* m = t->sm; hipStream_t st = x.st;
  const taco_hparams& hp = m->hp;
  const int Me = B * T_in, S = hp.speaker_embedding_size;
  if (is_deepvoice(m)) {   // speaker conditioning backward (tacotron.py:52-79)
    const std::vector<std::string> names = spk_vector_names(hp);
    const int dims[3] = {hp.enc_prenet[hp.enc_prenet_n - 1], hp.enc_rnn_size * 2, hp.attention_state_size};
    if (S == 1) {
      x.s->end_paths |= FRONT_PATH_SPK_TABLES;
      for (size_t i = 0; i < names.size(); ++i) {
        const int dd = i < 3 ? dims[i] : hp.dec_rnn_size;
        run_embed_bwd(x, dvec[i], speaker_id, x.g("spk/" + names[i] + "/table"), B, dd, hp.num_speakers);
      }
    } else {
      x.s->end_paths |= FRONT_PATH_SPK_DENSE;
      HIPCHK(zero_async(dspk_emb, (size_t)B * S * sizeof(float), st));
      for (size_t i = 0; i < names.size(); ++i) {
        const int dd = i < 3 ? dims[i] : hp.dec_rnn_size;
        hipLaunchKernelGGL(k_softsign_bwd, EWGRID((size_t)B * dd), 0, st, dvec[i], spk.vec[i], dzs, B * dd);
        TRY(run_wgrad(x, spk.emb, nullptr, S, dzs, dd, x.g("spk/" + names[i] + "/kernel"), dd, B, 0, S, dd));
        TRY(run_colsum(x, dzs, dd, nullptr, 0, nullptr, nullptr, x.g("spk/" + names[i] + "/bias"), nullptr, B, dd, 0));
        SkJob j = sk_T(m, t->tp.spk_T[i], dzs, dd, tmp, S);
        TRY(run_skinny(st, B, &j, 1));
        hipLaunchKernelGGL(k_add2d, EWGRID((size_t)B * S), 0, st, dspk_emb, S, tmp, S, B, S);
      }
      run_embed_bwd(x, dspk_emb, speaker_id, x.g("speaker_embedding"), B, S, hp.num_speakers);
    }
    HIPCHK(hipGetLastError());
  }
  float* dpre = dpre_of[hp.enc_prenet_n - 1];
  for (int i = hp.enc_prenet_n - 1; i >= 0; --i) {
    const int N = hp.enc_prenet[i];
    const std::string nm = "prenet/dense_" + std::to_string(i + 1);
    hipLaunchKernelGGL(k_relu_bwd, EWGRID((size_t)Me * N), 0, st, dpre, N, pre[i], N, dpre, N, Me, N);
    HIPCHK(hipGetLastError());
    if (i > 0) TRY(run_wgrad(x, pre[i - 1], nullptr, hp.enc_prenet[i - 1], dpre, N, x.g(nm + "/kernel"), N, Me, 0, hp.enc_prenet[i - 1], N));
    else TRY(run_wgrad(x, x.p("embedding"), ids, hp.embedding_size, dpre, N, x.g(nm + "/kernel"), N, Me, 0, hp.embedding_size, N));
    TRY(run_colsum(x, dpre, N, nullptr, 0, nullptr, nullptr, x.g(nm + "/bias"), nullptr, Me, N, 0));
    float* dnext = (i > 0) ? dpre_of[i - 1] : demb;
    const int nd = (i > 0) ? hp.enc_prenet[i - 1] : hp.embedding_size;
    TRY(run_dgrad(x, t->tp.encpre_d[i], dpre, N, Me, 0, dnext, nd));
    dpre = dnext;
  }
  run_embed_bwd(x, dpre, ids, x.g("embedding"), (int)Me, hp.embedding_size, hp.num_symbols);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// whole step: forward (tape) + loss + backward
// ---------------------------------------------------------------------------------------------------------------
static int train_forward_backward(taco_train* t, hipStream_t st, float* P, float* G, const int* ids, const int* lengths, const int* speaker_id, const float* mel_tgt,
                                  const float* lin_tgt, const float* loss_coeff, int B, int T_in, int T_out, int prioritize_loss,
                                  int sample_rate, float* d_losses, float* mel_out, float* lin_out, float* align_out, void* ws, size_t ws_bytes,
                                  bool do_backward, bool feed_back, bool freeze_moving = false) {
  taco_model* m = t->sm;
  const taco_hparams& hp = m->hp;
  const int r = hp.reduction_factor;
  if (T_out % r) return fail(TACO_ERR_SHAPE, "T_out %d is not a multiple of the reduction factor %d", T_out, r);
  const int n = T_out / r;
  if (n > hp.max_iters) return fail(TACO_ERR_SHAPE, "T_out/r = %d exceeds max_iters %d", n, hp.max_iters);
  TRY(check_common(m, B, T_in));
  if (!al16h(ws)) return fail(TACO_ERR_ARG, "workspace %p is not 16-byte aligned (the tape is carved in 256-byte steps from it; its four-column kernels need the alignment)", ws);
  if ((m->bf3 || m->bf3x6 || t->dgrad_bf3) && !t->bf3_current) return fail(TACO_ERR_STATE, "taco_train_set_exact_gemm(0) needs a taco_train_refresh before the next step (the split-bf16 weight planes are stale)");
  Carver cv(ws, ws_bytes);
  TrainWs w; carve_train(cv, t, B, T_in, n, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes, have %zu", cv.off, ws_bytes);
  StepState s;
  if (t->deterministic) { s.det = w.detscr; s.det_cap = DET_SCRATCH_FLOATS; }
  if (t->wgrad_planes) { s.wps = w.wpscr; s.wps_cap = w.wps_uint4; }
  TrainCtx x{t, st, P, G, do_backward && !freeze_moving, &s};
  const auto step = [&]() -> int {      // (a lambda so that the count below is published on every path out of the step, one that fails half-way included)
  // ---- forward ----
  TRY(front_forward_train(x, ids, speaker_id, B, T_in, w.pre, w.spk));
  const float* cur = w.pre[hp.enc_prenet_n - 1];
  const bool dv = is_deepvoice(m), simple = is_simple(m);
  const int L = hp.dec_layer_num;
  const float* dec_init[4] = {nullptr, nullptr, nullptr, nullptr}; float* d_dec_init[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < L && dv; ++i) { dec_init[i] = w.spk.vec[3 + i]; d_dec_init[i] = w.dvec[3 + i]; }
  TRY(cbhg_forward_train(x, m->enc, t->tp.enc, "encoder_cbhg", cur, B, T_in, lengths, w.enc, dv ? w.spk.vec[0] : nullptr, dv ? w.spk.vec[1] : nullptr));
  const float* enc_out = w.enc.out;
  TRY(teacher_frames(x, mel_tgt, B, n, w.teach));
  float* mel = mel_out ? mel_out : w.mel; float* lin = lin_out ? lin_out : w.linear;
  if (feed_back && do_backward) return fail(TACO_ERR_UNSUPPORTED, "rnn_decoder_test_mode is forward-only (the reference uses it for the test model's loss, train.py:158-166)");
  TRY(decoder_forward_train(x, enc_out, B, T_in, n, w.teach, mel, align_out, w.dec, feed_back, dv ? w.spk.vec[2] : nullptr, dv ? dec_init : nullptr,
                            simple ? w.spk.emb : nullptr));
  TRY(cbhg_forward_train(x, m->post, t->tp.post, "post_cbhg", mel, B, T_out, nullptr, w.post));
  TRY(head_forward_train(x, w.post.out, mel, simple ? w.spk.emb : nullptr, mel_tgt, lin_tgt, loss_coeff, B, T_out, prioritize_loss, sample_rate, lin, w.linrv,
                         d_losses, w.losspart));
  if (!do_backward) return 0;
  // ---- backward ----
  HIPCHK(zero_async(G, t->NP * sizeof(float), st));
  TRY(head_backward(x, w.post.out, mel, lin, simple ? w.spk.emb : nullptr, mel_tgt, lin_tgt, loss_coeff, B, T_out, prioritize_loss, sample_rate, w.dmel, w.dlin,
                    w.dlin_sum, w.dspk_emb, w.dpost));
  TRY(cbhg_backward(x, m->post, t->tp.post, "post_cbhg", mel, nullptr, B, T_out, nullptr, w.dpost, w.dmel_post, w.post));
  TRY(head_backward_join(x, w.dmel, w.dmel_post, B, T_out));
  TRY(decoder_backward(x, enc_out, B, T_in, n, w.teach, w.dmel, w.denc, w.dec, dv ? w.spk.vec[2] : nullptr, dv ? dec_init : nullptr,
                       dv ? w.dvec[2] : nullptr, dv ? d_dec_init : nullptr, simple ? w.dspk_emb : nullptr));
  if (simple) TRY(speaker_rows_backward(x, w.dspk_emb, speaker_id, B));
  TRY(cbhg_backward(x, m->enc, t->tp.enc, "encoder_cbhg", cur, nullptr, B, T_in, lengths, w.denc, w.dpre[hp.enc_prenet_n - 1], w.enc,
                    dv ? w.spk.vec[1] : nullptr, dv ? w.dvec[1] : nullptr, dv ? w.dvec[0] : nullptr, w.rowidx));
  return front_backward(x, ids, speaker_id, B, T_in, w.pre, w.dpre, w.demb, w.spk, w.dvec, w.dspk_emb, w.dzs, w.dec.tmp1);
  };
  const int rc = step();
  t->planes_problems = s.planes_problems;
  return rc;
}
