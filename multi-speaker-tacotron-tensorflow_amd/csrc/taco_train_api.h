// taco_train_api.h -- C ABI of the training path (declared in include/taco_abi.h); included inside extern "C".

// index-valued "weights" of a trainer's shadow model (the packs become index maps) and its TrainPacks
static int train_shadow_weights(taco_train* t) {
  taco_model* sm = t->sm;
  size_t off = 0;
  for (auto& s : sm->spec) {          // flat layout = spec order, TF tensor layout, no padding
    size_t cnt = 1;
    for (int64_t d : s.second) cnt *= (size_t)d;
    t->poff[s.first] = off;
    HostTensor ht; ht.shape = s.second; ht.data.resize(cnt); ht.set = true;
    for (size_t k = 0; k < cnt; ++k) ht.data[k] = (float)(off + k + 1);     // index-valued "weights": the packs become index maps
    sm->raw[s.first] = ht;
    off += cnt;
  }
  t->NP = off;
  if (off >= (1u << 24)) return fail(TACO_ERR_UNSUPPORTED, "more than 2^24 parameters");
  sm->tp = &t->tp;
  sm->bf3 = 1;                        // finalize builds the split-bf16 packs (as index lists) next to the fp32 ones ...
  return 0;
}

int taco_train_create(const taco_hparams* hp, int device, taco_train** out) {
  if (!hp || !out) return fail(TACO_ERR_ARG, "null argument");
  taco_train* t = new taco_train();
  int rc = taco_model_create(hp, device, &t->sm);
  if (rc != 0) { delete t; return rc; }
  taco_model* sm = t->sm;
  rc = train_shadow_weights(t);
  if (rc != 0) { taco_model_destroy(sm); delete t; return rc; }
  rc = taco_model_finalize(sm);
  if (rc != 0) { taco_model_destroy(sm); delete t; return rc; }
  sm->bf3 = 0; sm->bf3x6 = 1;         // ... and the step starts with its forward GEMMs on the six-product split (fp32-grade; mode 4) and its data
  t->dgrad_bf3 = 1; t->want_bf3_planes = true;   // gradients on the split-bf16 kernel (mode 4 of taco_train_set_exact_gemm, the default)
  if (!sm->bf3_idx.empty()) {
    if (hipMalloc((void**)&t->d_bf3_idx, sm->bf3_idx.size() * sizeof(unsigned)) != hipSuccess ||
        hipMalloc((void**)&t->d_bf3_segs, sm->bf3_segs.size() * sizeof(Bf3Seg)) != hipSuccess ||
        hipMemcpy(t->d_bf3_idx, sm->bf3_idx.data(), sm->bf3_idx.size() * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(t->d_bf3_segs, sm->bf3_segs.data(), sm->bf3_segs.size() * sizeof(Bf3Seg), hipMemcpyHostToDevice) != hipSuccess) {
      taco_model_destroy(sm); delete t; return fail(TACO_ERR_HIP, "split-bf16 index list allocation failed");
    }
    t->n_bf3 = sm->bf3_idx.size(); t->n_bf3_segs = (int)sm->bf3_segs.size();
    std::vector<unsigned>().swap(sm->bf3_idx);          // the host copy (tens of MB) is not needed again
  }
  t->arena_n = sm->arena_n;
  if (hipMalloc((void**)&t->d_map, t->arena_n * sizeof(float)) != hipSuccess ||
      hipMemcpy(t->d_map, sm->darena, t->arena_n * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess) {
    taco_model_destroy(sm); delete t; return fail(TACO_ERR_HIP, "index map allocation failed");
  }
  if (sm->dx_fold_n && hipMalloc((void**)&t->d_fold, sm->dx_fold_n * sizeof(float)) != hipSuccess) {
    taco_model_destroy(sm); delete t; return fail(TACO_ERR_HIP, "fold buffer allocation failed");
  }
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bigru_rows_bwd<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bigru_rows_bwd<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attention_bwd), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_wp_gemm<WP_WK, WP_WN, WP_SM, WP_NB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)WP_LDS);
  *out = t;
  return 0;
}

void taco_train_destroy(taco_train* t) {
  if (!t) return;
  if (t->d_map) (void)hipFree(t->d_map);
  if (t->d_fold) (void)hipFree(t->d_fold);
  if (t->d_bf3_idx) (void)hipFree(t->d_bf3_idx);
  if (t->d_bf3_segs) (void)hipFree(t->d_bf3_segs);
  taco_segnorm_plan_destroy(t->gn_plan);
  if (t->sm) taco_model_destroy(t->sm);
  delete t;
}

taco_model* taco_train_model(taco_train* t) { return t ? t->sm : nullptr; }

int taco_train_set_sync_bn(taco_train* t, taco_sync_sum_fn fn, void* user, int world_size) {
  if (!t) return fail(TACO_ERR_ARG, "null argument");
  if (fn && world_size < 1) return fail(TACO_ERR_ARG, "world_size %d", world_size);
  t->sync_fn = fn; t->sync_user = user; t->sync_world = fn ? world_size : 1;
  return 0;
}
int taco_train_set_exact_wgrad(taco_train* t, int on) {
  if (!t) return fail(TACO_ERR_ARG, "null argument");
  t->wgrad_bf3 = on ? 0 : 1;          // per trainer: run_wgrad reads it through the step's TrainCtx
  return 0;
}
int taco_train_set_wgrad_planes(taco_train* t, int mode) {
  if (!t) return fail(TACO_ERR_ARG, "null argument");
  if (mode < 0 || mode > 2) return fail(TACO_ERR_ARG, "mode %d (0 off, 1 large problems, 2 every eligible problem)", mode);
  t->wgrad_planes = mode;             // (0 -> non-zero changes the workspace size: ask taco_train_workspace_bytes again)
  return 0;
}
int taco_train_planes_problems(const taco_train* t) { return t ? t->planes_problems : 0; }
int taco_train_set_exact_gemm(taco_train* t, int on) {
  if (!t) return fail(TACO_ERR_ARG, "null argument");
  if (on != 1 && !t->d_bf3_idx) return fail(TACO_ERR_STATE, "this model has no split-bf16 packs");
  t->sm->bf3 = (on == 1 || on == 3 || on == 4) ? 0 : 1;       // the planes are regenerated by the next taco_train_refresh: call it before the next step
  t->sm->bf3x6 = on == 4 ? 1 : 0;                  // mode 4: forward GEMMs with operands split three ways, six products (fp32-grade) on the bf16 pipe
  t->dgrad_exact = on == 2 ? 1 : 0;
  t->dgrad_bf3 = (on == 3 || on == 4) ? 1 : 0;
  t->want_bf3_planes = on != 1;
  return 0;
}
int taco_train_set_bptt_engine(taco_train* t, int persistent) {
  if (!t) return fail(TACO_ERR_ARG, "null argument");
  t->bptt_persistent = persistent ? 1 : 0;
  t->resident_bwd_scan = persistent ? 1 : 0;      // (the A/B engine keeps round 1's scan kernel as well)
  return 0;
}
int taco_train_set_deterministic(taco_train* t, int on) {
  if (!t) return fail(TACO_ERR_ARG, "null argument");
  t->deterministic = on ? 1 : 0;      // changes taco_train_workspace_bytes
  return 0;
}
// Test hook: the post-net BiGRU scan alone, forward with the gate tape and backward, on caller data -- ragged lengths and initial
// states included, which the post-net itself never has.  persistent = 1: k_bigru_oct<UPW, true> (9 to 32 rows) or k_bigru_duo<RG, true>, + k_bigru_duo_bwd (needs H = 256 on a
// whole MI355X); 0: k_bigru_res<..., true> + k_bigru_rows_bwd.  All buffers device, caller-owned:
//   xproj [B*T, 6H] (the hoisted input projection, backward direction time-reversed per row), lengths [B] or null, h0 [B, 2H] or null,
//   dout [B*T, 2H]  ->  out [B*T, 2H], gsave [B*T, 6H], dg [B*T, 6H], rh [B*T, 2H], dh0 [B, 2H] (nullable); scratch: >= 1 MB.
int taco_train_debug_bigru(taco_train* t, void* hip_stream, const float* xproj, const int32_t* lengths, const float* h0, const float* dout,
                           int B, int T, int persistent, float* out, float* gsave, float* dg, float* rh, float* dh0, void* scratch, size_t scratch_bytes) {
  if (!t || !xproj || !dout || !out || !gsave || !dg || !rh || !scratch) return fail(TACO_ERR_ARG, "null argument");
  const taco_model* m = t->sm; const Cbhg& c = m->post; const int H = c.rnn;
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHK(hipSetDevice(m->device));
  Carver cv(scratch, scratch_bytes);
  Xchg gx; gx.carve(cv, std::max(gd_xbuf_granules(8), gb_xbuf_granules(8)));
  if (!cv.ok()) return fail(TACO_ERR_STATE, "scratch too small: need %zu bytes", cv.off);
  const size_t M = (size_t)B * T;
  HIPCHK(zero_async(gsave, M * 6 * H * sizeof(float), st));
  HIPCHK(zero_async(dg, M * 6 * H * sizeof(float), st));
  HIPCHK(zero_async(rh, M * 2 * H * sizeof(float), st));
  if (persistent) {
    const ScanPlan sp = scan_plan(m, c, B, T, true);
    if (sp.bwd == SCAN_BWD_ROWS) return fail(TACO_ERR_UNSUPPORTED, "the whole-chip scans need H = 256, at most 64 rows and an unpartitioned MI355X");
    if (sp.kernel == SCAN_K_OCT) TRY(oct_launch(m, st, c, sp.upw, B, T, xproj, lengths, h0, out, gsave, gx));      // as the training forward picks
    else TRY(duo_launch(m, st, c, sp.rg, B, T, xproj, lengths, h0, out, gsave, gx));
    HIPCHK(gx.clear(st));      // (the backward launchers expect their caller to have cleared: cbhg_backward)
    if (sp.bwd == SCAN_BWD_OCT) return oct_bwd_launch(m, st, c, B, T, dout, out, gsave, h0, lengths, dg, rh, dh0, gx);      // as the training step picks
    return duo_bwd_launch(m, st, c, sp.rg, B, T, dout, out, gsave, h0, lengths, dg, rh, dh0, gx);
  }
  if (H != 256) return fail(TACO_ERR_UNSUPPORTED, "post-net rnn size %d", H);
  { BigruSArgs a; memset(&a, 0, sizeof a);
    a.xproj = xproj; a.g2_0 = (const float2*)AP(m, c.res_g2[0]); a.g2_1 = (const float2*)AP(m, c.res_g2[1]);
    a.c1_0 = AP(m, c.raw_ch[0]); a.c1_1 = AP(m, c.raw_ch[1]); a.lengths = lengths; a.out = out; a.gsave = gsave; a.B = B; a.T = T; a.h0 = h0;
    hipLaunchKernelGGL((k_bigru_res<256, 64, 24, 1, true>), dim3(2 * B), dim3(512), bigru_res_lds(256, 24, 1), st, a); }
  { const CbhgT& ct = t->tp.post;
    const int R = (B >= 2) ? 2 : 1;
    const size_t lds = ((size_t)4 * R * H + (size_t)RP_NT * R * 4 + 64) * sizeof(float);
    BigruBArgs a; memset(&a, 0, sizeof a);
    a.dout = dout; a.out = out; a.gsave = gsave; a.wgT0 = AP(m, ct.ghT[0]); a.wgT1 = AP(m, ct.ghT[1]); a.wcT0 = AP(m, ct.chT[0]); a.wcT1 = AP(m, ct.chT[1]);
    a.lengths = lengths; a.dg = dg; a.rh = rh; a.B = B; a.T = T; a.H = H; a.h0 = h0; a.dh0 = dh0;
    if (R == 2) hipLaunchKernelGGL(k_bigru_rows_bwd<2>, dim3(2 * cdiv(B, R)), dim3(RP_NT), lds, st, a);
    else hipLaunchKernelGGL(k_bigru_rows_bwd<1>, dim3(2 * cdiv(B, R)), dim3(RP_NT), lds, st, a); }
  HIPCHK(hipGetLastError());
  return 0;
}
// Test hook: ONE CBHG of the trainer -- cbhg_forward_train, then cbhg_backward -- on caller data, as the step calls them: the same TrainCtx and
// StepState (deterministic scratch, plane scratch sized as the step's), the tape of carve_cbhg_tape, the trainer's current switches; cbhg_backward opens
// its own WgRegion, as in the step.  Moving statistics are frozen.  The scope's parameter gradients are ADDED into d_grads at their
// taco_train_param_offset (the step zero-fills the buffer first: so does the caller, inside the scope); nothing else of d_grads is written.
struct CbhgDebugWs { CbhgTape tape; float* detscr; uint4* wpscr; size_t wps_uint4; int* rowidx; };
static void carve_cbhg_debug(Carver& cv, const taco_train* t, const Cbhg& c, int B, int T, CbhgDebugWs& w) {
  carve_cbhg_tape(cv, c, B, T, w.tape);
  w.detscr = cv.f(t->deterministic ? DET_SCRATCH_FLOATS : 1);
  w.wps_uint4 = wps_scratch_uint4(t, (size_t)B * T);
  w.wpscr = (uint4*)cv.raw(w.wps_uint4 * sizeof(uint4));
  w.rowidx = cv.i(B);
}
size_t taco_train_debug_cbhg_workspace_bytes(const taco_train* t, int which, int B, int T) {
  if (!t || (which != 0 && which != 1) || B <= 0 || T <= 0) return 0;
  Carver cv(nullptr, 0);
  CbhgDebugWs w; carve_cbhg_debug(cv, t, which ? t->sm->post : t->sm->enc, B, T, w);
  return cv.off;
}
int taco_train_debug_cbhg(taco_train* t, void* hip_stream, int which, float* d_params, float* d_grads, const float* d_in, const int32_t* d_lengths,
                          const float* d_h0, const float* d_before, const float* d_dout, int B, int T, float* d_out, float* d_din, float* d_dh0,
                          float* d_dbefore, void* d_ws, size_t ws_bytes, uint32_t* paths) {
  if (!t || !d_params || !d_grads || !d_in || !d_dout || !d_out || !d_din || !d_ws) return fail(TACO_ERR_ARG, "null argument");
  if (which != 0 && which != 1) return fail(TACO_ERR_ARG, "which %d (0 encoder CBHG, 1 post CBHG)", which);
  if ((d_dh0 && !d_h0) || (d_dbefore && !d_before)) return fail(TACO_ERR_ARG, "a gradient output without its input");
  taco_model* m = t->sm;
  HIPCHK(hipSetDevice(m->device));
  TRY(check_common(m, B, T));
  if (!al16h(d_ws)) return fail(TACO_ERR_ARG, "workspace %p is not 16-byte aligned", d_ws);
  if ((m->bf3 || m->bf3x6 || t->dgrad_bf3) && !t->bf3_current) return fail(TACO_ERR_STATE, "taco_train_set_exact_gemm(0) needs a taco_train_refresh before the next step (the split-bf16 weight planes are stale)");
  const Cbhg& c = which ? m->post : m->enc;
  const CbhgT& ct = which ? t->tp.post : t->tp.enc;
  const char* sc = which ? "post_cbhg" : "encoder_cbhg";
  Carver cv(d_ws, ws_bytes);
  CbhgDebugWs w; carve_cbhg_debug(cv, t, c, B, T, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes, have %zu", cv.off, ws_bytes);
  hipStream_t st = (hipStream_t)hip_stream;
  StepState s;
  if (t->deterministic) { s.det = w.detscr; s.det_cap = DET_SCRATCH_FLOATS; }
  if (t->wgrad_planes) { s.wps = w.wpscr; s.wps_cap = w.wps_uint4; }
  TrainCtx x{t, st, d_params, d_grads, false, &s};
  const auto run = [&]() -> int {
    TRY(cbhg_forward_train(x, c, ct, sc, d_in, B, T, d_lengths, w.tape, d_before, d_h0));
    TRY(cbhg_backward(x, c, ct, sc, d_in, nullptr, B, T, d_lengths, d_dout, d_din, w.tape, d_h0, d_dh0, d_dbefore, w.rowidx));
    HIPCHK(hipMemcpyAsync(d_out, w.tape.out, (size_t)B * T * 2 * c.rnn * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
  };
  const int rc = run();
  t->planes_problems = s.planes_problems;
  // (k_highway_bwd, the plain form of the highway backward, cannot be reached through a trainer: taco_model_create requires rnn sizes that are
  // multiples of 4 and the tape is carved in 256-byte steps, so CBHG_PATH_HW_BWD_PLAIN stays clear in every word this hook returns)
  if (paths) *paths = s.paths;
  return rc;
}
// Test hook: the decoder of the trainer alone -- decoder_forward_train (teacher forced, feed_back = false), then decoder_backward -- on caller data, as the
// step calls them: the same TrainCtx and StepState (deterministic scratch, plane scratch sized as the step's), the tape of carve_dec_tape, the trainer's
// current switches.  The scope's parameter gradients (decoder/*, attention/*) are ADDED into d_grads at their taco_train_param_offset; nothing else of
// d_grads is written.  Every refusal below comes before the first HIP call.
struct DecDebugWs { DecTape tape; float* detscr; uint4* wpscr; size_t wps_uint4; };
static void carve_dec_debug(Carver& cv, const taco_train* t, int B, int T_in, int n, DecDebugWs& w) {
  carve_dec_tape(cv, t->sm, B, T_in, n, w.tape);
  w.detscr = cv.f(t->deterministic ? DET_SCRATCH_FLOATS : 1);
  w.wps_uint4 = wps_scratch_uint4(t, std::max((size_t)B * T_in, (size_t)B * n * t->sm->hp.reduction_factor));
  w.wpscr = (uint4*)cv.raw(w.wps_uint4 * sizeof(uint4));
}
size_t taco_train_debug_decoder_workspace_bytes(const taco_train* t, int B, int T_in, int n) {
  if (!t || B <= 0 || T_in <= 0 || n <= 0) return 0;
  Carver cv(nullptr, 0);
  DecDebugWs w; carve_dec_debug(cv, t, B, T_in, n, w);
  return cv.off;
}
int taco_train_debug_decoder(taco_train* t, void* hip_stream, float* d_params, float* d_grads, const float* d_enc_out, const float* d_teacher,
                             const float* d_dmel, const float* d_att_init, const float* const* d_dec_init, const float* d_spk_emb, int B, int T_in, int n,
                             float* d_mel, float* d_alignments, float* d_denc, float* d_datt_init, float* const* d_ddec_init, float* d_dspk_emb,
                             void* d_ws, size_t ws_bytes, uint32_t* paths) {
  if (!t || !d_params || !d_grads || !d_enc_out || !d_teacher || !d_dmel || !d_mel || !d_alignments || !d_denc || !d_ws) return fail(TACO_ERR_ARG, "null argument");
  taco_model* m = t->sm;
  const taco_hparams& hp = m->hp;
  const int L = hp.dec_layer_num, S = simple_S(m);
  if (L > 4) return fail(TACO_ERR_UNSUPPORTED, "%d decoder layers", L);
  const float* dec_init[4] = {nullptr, nullptr, nullptr, nullptr}; float* ddec_init[4] = {nullptr, nullptr, nullptr, nullptr};
  bool any_init = false;
  for (int i = 0; i < L; ++i) {
    dec_init[i] = d_dec_init ? d_dec_init[i] : nullptr; ddec_init[i] = d_ddec_init ? d_ddec_init[i] : nullptr;
    any_init = any_init || dec_init[i];
    if (ddec_init[i] && !dec_init[i]) return fail(TACO_ERR_ARG, "a gradient output without its input (initial state of decoder layer %d)", i + 1);
  }
  if ((d_datt_init && !d_att_init) || (d_dspk_emb && !d_spk_emb)) return fail(TACO_ERR_ARG, "a gradient output without its input");
  if ((d_att_init || any_init) && !is_deepvoice(m)) return fail(TACO_ERR_ARG, "initial states are model type deepvoice's");
  if (S && !(d_spk_emb && d_dspk_emb)) return fail(TACO_ERR_ARG, "model type simple: the speaker rows and their gradient buffer are required");
  if (!S && d_spk_emb) return fail(TACO_ERR_ARG, "speaker rows enter the decoder of model type simple only");
  TRY(check_common(m, B, T_in));
  if (n <= 0) return fail(TACO_ERR_ARG, "bad number of decoder steps %d", n);
  if (n > hp.max_iters) return fail(TACO_ERR_SHAPE, "%d decoder steps exceed max_iters %d", n, hp.max_iters);
  if (!al16h(d_ws)) return fail(TACO_ERR_ARG, "workspace %p is not 16-byte aligned", d_ws);
  if ((m->bf3 || m->bf3x6 || t->dgrad_bf3) && !t->bf3_current) return fail(TACO_ERR_STATE, "taco_train_set_exact_gemm(0) needs a taco_train_refresh before the next step (the split-bf16 weight planes are stale)");
  TRY(decoder_fwd_check(m, T_in));
  TRY(decoder_bwd_check(m, T_in));
  Carver cv(d_ws, ws_bytes);
  DecDebugWs w; carve_dec_debug(cv, t, B, T_in, n, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes, have %zu", cv.off, ws_bytes);
  if (!m->d_err) return fail(TACO_ERR_STATE, "a host-only trainer (taco_debug_train_create_host) cannot run");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)hip_stream;
  StepState s;
  if (t->deterministic) { s.det = w.detscr; s.det_cap = DET_SCRATCH_FLOATS; }
  if (t->wgrad_planes) { s.wps = w.wpscr; s.wps_cap = w.wps_uint4; }
  TrainCtx x{t, st, d_params, d_grads, false, &s};
  const bool inits = d_att_init || any_init;
  const auto run = [&]() -> int {
    TRY(decoder_forward_train(x, d_enc_out, B, T_in, n, d_teacher, d_mel, d_alignments, w.tape, false, d_att_init, inits ? dec_init : nullptr, d_spk_emb));
    if (S) HIPCHK(zero_async(d_dspk_emb, (size_t)B * S * sizeof(float), st));      // the step zero-fills it ahead of the head's share
    TRY(decoder_backward(x, d_enc_out, B, T_in, n, d_teacher, d_dmel, d_denc, w.tape, d_att_init, inits ? dec_init : nullptr, d_datt_init,
                         inits ? ddec_init : nullptr, d_dspk_emb));
    return 0;
  };
  int rc = run();
  t->planes_problems = s.planes_problems;
  if (paths) {
    if (rc == 0 && (s.dec_paths & (DEC_PATH_FWD_PERSISTENT | DEC_PATH_BWD_PERSISTENT))) {      // the census words of the launches, once they have run
      unsigned fw = 0, bw = 0;
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipMemcpy(&fw, m->d_err + 8, sizeof fw, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(&bw, m->d_err + 40, sizeof bw, hipMemcpyDeviceToHost));
      for (const unsigned v : {(s.dec_paths & DEC_PATH_FWD_PERSISTENT) ? fw : 0u, (s.dec_paths & DEC_PATH_BWD_PERSISTENT) ? bw : 0u})
        s.dec_paths |= v == 1 ? DEC_PATH_XCD_LOCAL : v == 2 ? DEC_PATH_WRITE_THROUGH : 0u;
    }
    *paths = s.dec_paths;
  }
  return rc;
}
// Test hooks: the two ENDS of the step alone -- front_forward_train + [speaker_rows_backward +] front_backward, and teacher_frames + head_forward_train +
// head_backward + head_backward_join -- on caller data, as the step calls them: the same TrainCtx and StepState (deterministic scratch, plane scratch sized
// as the step's for these rows), the step's buffers carved as carve_train carves them, the trainer's current switches.  The scope's parameter gradients are
// ADDED into d_grads at their taco_train_param_offset; nothing else of d_grads is written.  Every refusal below comes before the first HIP call.
struct FrontDebugWs { float* pre[4]; float* dpre[4]; float* demb; SpkWs spk; float *dspk_emb, *dzs, *tmp, *detscr; uint4* wpscr; size_t wps_uint4; };
static void carve_front_debug(Carver& cv, const taco_train* t, int B, int T_in, FrontDebugWs& w) {
  const taco_model* m = t->sm;
  const taco_hparams& hp = m->hp;
  const size_t Me = (size_t)B * T_in;
  for (int i = 0; i < hp.enc_prenet_n; ++i) { w.pre[i] = cv.f(Me * hp.enc_prenet[i]); w.dpre[i] = cv.f(Me * std::max(hp.enc_prenet[i], hp.embedding_size)); }
  w.demb = cv.f(Me * hp.embedding_size);
  carve_spk(cv, m, B, w.spk);
  int dmax = std::max(std::max(hp.enc_prenet[hp.enc_prenet_n - 1], hp.enc_rnn_size * 2), std::max(hp.attention_state_size, hp.dec_rnn_size));
  const size_t S = (size_t)std::max(hp.speaker_embedding_size, 1);
  w.dspk_emb = cv.f(B * S); w.dzs = cv.f((size_t)B * dmax); w.tmp = cv.f(B * S);
  w.detscr = cv.f(t->deterministic ? DET_SCRATCH_FLOATS : 1);
  w.wps_uint4 = wps_scratch_uint4(t, Me);
  w.wpscr = (uint4*)cv.raw(w.wps_uint4 * sizeof(uint4));
}
size_t taco_train_debug_front_workspace_bytes(const taco_train* t, int B, int T_in) {
  if (!t || B <= 0 || T_in <= 0) return 0;
  Carver cv(nullptr, 0);
  FrontDebugWs w; carve_front_debug(cv, t, B, T_in, w);
  return cv.off;
}
int taco_train_debug_front(taco_train* t, void* hip_stream, float* d_params, float* d_grads, const int32_t* d_ids, const int32_t* d_speaker_id,
                           const float* d_dpre, const float* const* d_dvec, const float* d_dspk_emb, int B, int T_in, float* d_pre, float* const* d_vec,
                           float* d_spk_emb, void* d_ws, size_t ws_bytes, uint32_t* paths) {
  if (!t || !d_params || !d_grads || !d_ids || !d_dpre || !d_pre || !d_ws) return fail(TACO_ERR_ARG, "null argument");
  taco_model* m = t->sm;
  const taco_hparams& hp = m->hp;
  const bool dv = is_deepvoice(m), simple = is_simple(m);
  const int nv = 3 + hp.dec_layer_num, S = hp.speaker_embedding_size, np = hp.enc_prenet_n;
  if (nv > 8 || np < 1 || np > 4) return fail(TACO_ERR_UNSUPPORTED, "%d decoder layers, %d encoder prenet layers", hp.dec_layer_num, np);
  if (!dv && !simple && (d_speaker_id || d_dvec || d_dspk_emb || d_vec || d_spk_emb)) return fail(TACO_ERR_ARG, "speaker inputs and outputs given to a single-speaker model");
  if ((dv || simple) && !d_speaker_id) return fail(TACO_ERR_ARG, "speaker_id required for a multi-speaker model");
  if ((d_dvec && !d_vec) || (d_dspk_emb && !d_spk_emb)) return fail(TACO_ERR_ARG, "a gradient without its forward output (speaker vectors / speaker rows)");
  if (dv) {
    if (d_dspk_emb) return fail(TACO_ERR_ARG, "the gradient of the speaker rows is an input of model type simple only");
    if (!d_vec || !d_dvec) return fail(TACO_ERR_ARG, "model type deepvoice: the speaker vectors and their gradients are required");
    for (int i = 0; i < nv; ++i) if (!d_vec[i] || !d_dvec[i]) return fail(TACO_ERR_ARG, "model type deepvoice: speaker vector %d or its gradient is null", i);
    if (S == 1 && d_spk_emb) return fail(TACO_ERR_ARG, "speaker_embedding_size 1 has no speaker rows (the vectors come from tables)");
  }
  if (simple) {
    if (d_vec || d_dvec) return fail(TACO_ERR_ARG, "speaker vectors are model type deepvoice's");
    if (!d_spk_emb || !d_dspk_emb) return fail(TACO_ERR_ARG, "model type simple: the speaker rows and their gradient are required");
  }
  TRY(check_common(m, B, T_in));
  if (!al16h(d_ws)) return fail(TACO_ERR_ARG, "workspace %p is not 16-byte aligned", d_ws);
  if ((m->bf3 || m->bf3x6 || t->dgrad_bf3) && !t->bf3_current) return fail(TACO_ERR_STATE, "taco_train_set_exact_gemm(0) needs a taco_train_refresh before the next step (the split-bf16 weight planes are stale)");
  Carver cv(d_ws, ws_bytes);
  FrontDebugWs w; carve_front_debug(cv, t, B, T_in, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes, have %zu", cv.off, ws_bytes);
  if (!m->d_err) return fail(TACO_ERR_STATE, "a host-only trainer (taco_debug_train_create_host) cannot run");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)hip_stream;
  StepState s;
  if (t->deterministic) { s.det = w.detscr; s.det_cap = DET_SCRATCH_FLOATS; }
  if (t->wgrad_planes) { s.wps = w.wpscr; s.wps_cap = w.wps_uint4; }
  TrainCtx x{t, st, d_params, d_grads, false, &s};
  const size_t Me = (size_t)B * T_in;
  const int dims[3] = {hp.enc_prenet[np - 1], hp.enc_rnn_size * 2, hp.attention_state_size};
  const auto run = [&]() -> int {
    TRY(front_forward_train(x, d_ids, d_speaker_id, B, T_in, w.pre, w.spk));
    HIPCHK(hipMemcpyAsync(d_pre, w.pre[np - 1], Me * hp.enc_prenet[np - 1] * sizeof(float), hipMemcpyDeviceToDevice, st));
    for (int i = 0; i < nv && dv; ++i)
      HIPCHK(hipMemcpyAsync(d_vec[i], w.spk.vec[i], (size_t)B * (i < 3 ? dims[i] : hp.dec_rnn_size) * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (d_spk_emb) HIPCHK(hipMemcpyAsync(d_spk_emb, w.spk.emb, (size_t)B * S * sizeof(float), hipMemcpyDeviceToDevice, st));
    // the step's dpre is what the encoder CBHG's backward leaves in the last prenet layer's gradient buffer; the prenet backward works in place
    HIPCHK(hipMemcpyAsync(w.dpre[np - 1], d_dpre, Me * hp.enc_prenet[np - 1] * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (simple) TRY(speaker_rows_backward(x, d_dspk_emb, d_speaker_id, B));
    return front_backward(x, d_ids, d_speaker_id, B, T_in, w.pre, w.dpre, w.demb, w.spk, d_dvec, w.dspk_emb, w.dzs, w.tmp);
  };
  const int rc = run();
  t->planes_problems = s.planes_problems;
  if (paths) *paths = s.end_paths;
  return rc;
}
struct HeadDebugWs { float *dlin, *linrv, *dlin_sum, *losspart, *detscr; uint4* wpscr; size_t wps_uint4; };
static void carve_head_debug(Carver& cv, const taco_train* t, int B, int T_out, HeadDebugWs& w) {
  const taco_model* m = t->sm;
  const taco_hparams& hp = m->hp;
  const size_t Mp = (size_t)B * T_out;
  w.dlin = cv.f(Mp * hp.num_freq);
  w.losspart = (float*)cv.raw((size_t)TR_MAXBLK * 8 * sizeof(double));
  const size_t nrv = is_simple(m) ? (size_t)B * hp.num_freq : 1;
  w.linrv = cv.f(nrv); w.dlin_sum = cv.f(nrv);
  w.detscr = cv.f(t->deterministic ? DET_SCRATCH_FLOATS : 1);
  w.wps_uint4 = wps_scratch_uint4(t, Mp);
  w.wpscr = (uint4*)cv.raw(w.wps_uint4 * sizeof(uint4));
}
size_t taco_train_debug_head_workspace_bytes(const taco_train* t, int B, int T_out) {
  if (!t || B <= 0 || T_out <= 0) return 0;
  Carver cv(nullptr, 0);
  HeadDebugWs w; carve_head_debug(cv, t, B, T_out, w);
  return cv.off;
}
int taco_train_debug_head(taco_train* t, void* hip_stream, float* d_params, float* d_grads, const float* d_post_out, const float* d_mel, const float* d_mel_tgt,
                          const float* d_lin_tgt, const float* d_loss_coeff, const float* d_dmel_post, const float* d_spk_emb, int B, int T_out,
                          int prioritize_loss, int sample_rate, float* d_teacher, float* d_lin, float* d_losses, float* d_dmel, float* d_dpost,
                          float* d_dspk_emb, void* d_ws, size_t ws_bytes) {
  if (!t || !d_params || !d_grads || !d_post_out || !d_mel || !d_mel_tgt || !d_lin_tgt || !d_teacher || !d_lin || !d_losses || !d_dmel || !d_dpost || !d_ws)
    return fail(TACO_ERR_ARG, "null argument");
  taco_model* m = t->sm;
  const taco_hparams& hp = m->hp;
  const int S = simple_S(m), r = hp.reduction_factor;
  if (d_dspk_emb && !d_spk_emb) return fail(TACO_ERR_ARG, "a gradient output without its input");
  if (S && !(d_spk_emb && d_dspk_emb)) return fail(TACO_ERR_ARG, "model type simple: the speaker rows and their gradient buffer are required");
  if (!S && d_spk_emb) return fail(TACO_ERR_ARG, "speaker rows enter the linear head of model type simple only");
  if (B <= 0 || T_out <= 0 || sample_rate <= 0) return fail(TACO_ERR_ARG, "bad shape B=%d T_out=%d or sample rate %d", B, T_out, sample_rate);
  if (B > 64) return fail(TACO_ERR_UNSUPPORTED, "batch %d > 64 rows per device is not supported: shard the batch", B);
  if (T_out % r) return fail(TACO_ERR_SHAPE, "T_out %d is not a multiple of the reduction factor %d", T_out, r);
  const int n = T_out / r;
  if (n > hp.max_iters) return fail(TACO_ERR_SHAPE, "T_out/r = %d exceeds max_iters %d", n, hp.max_iters);
  if (!al16h(d_ws)) return fail(TACO_ERR_ARG, "workspace %p is not 16-byte aligned", d_ws);
  if ((m->bf3 || m->bf3x6 || t->dgrad_bf3) && !t->bf3_current) return fail(TACO_ERR_STATE, "taco_train_set_exact_gemm(0) needs a taco_train_refresh before the next step (the split-bf16 weight planes are stale)");
  Carver cv(d_ws, ws_bytes);
  HeadDebugWs w; carve_head_debug(cv, t, B, T_out, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes, have %zu", cv.off, ws_bytes);
  if (!m->d_err) return fail(TACO_ERR_STATE, "a host-only trainer (taco_debug_train_create_host) cannot run");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)hip_stream;
  StepState s;
  if (t->deterministic) { s.det = w.detscr; s.det_cap = DET_SCRATCH_FLOATS; }
  if (t->wgrad_planes) { s.wps = w.wpscr; s.wps_cap = w.wps_uint4; }
  TrainCtx x{t, st, d_params, d_grads, false, &s};
  const auto run = [&]() -> int {
    TRY(teacher_frames(x, d_mel_tgt, B, n, d_teacher));
    TRY(head_forward_train(x, d_post_out, d_mel, d_spk_emb, d_mel_tgt, d_lin_tgt, d_loss_coeff, B, T_out, prioritize_loss, sample_rate, d_lin, w.linrv, d_losses,
                           w.losspart));
    TRY(head_backward(x, d_post_out, d_mel, d_lin, d_spk_emb, d_mel_tgt, d_lin_tgt, d_loss_coeff, B, T_out, prioritize_loss, sample_rate, d_dmel, w.dlin, w.dlin_sum,
                      d_dspk_emb, d_dpost));
    if (d_dmel_post) TRY(head_backward_join(x, d_dmel, d_dmel_post, B, T_out));
    return 0;
  };
  const int rc = run();
  t->planes_problems = s.planes_problems;
  return rc;
}
// Test hook: a trainer that stays on the host -- the shadow model is packed (model_pack_host) and never uploaded, no device is touched.  It serves the
// argument and state checks of the taco_train_debug_* hooks, which come before their first HIP call; nothing may be launched on it.
int taco_debug_train_create_host(const taco_hparams* hp, taco_train** out) {
  if (!hp || !out) return fail(TACO_ERR_ARG, "null argument");
  taco_train* t = new taco_train();
  int rc = taco_model_create(hp, 0, &t->sm);
  if (rc != 0) { delete t; return rc; }
  rc = train_shadow_weights(t);
  if (rc == 0) rc = model_pack_host(t->sm);
  if (rc != 0) { taco_train_destroy(t); return rc; }
  taco_model* sm = t->sm;
  sm->raw.clear(); sm->finalized = true;
  sm->bf3 = 0; sm->bf3x6 = 1; t->dgrad_bf3 = 1; t->want_bf3_planes = true;      // the switches of taco_train_create; the planes were never generated
  *out = t;
  return 0;
}
// Test hook: what wgrad_plan (nw = 0) / wgrad_bank_plan (nw > 0: a conv bank of widths 1 .. nw, N = channels per width) decide -- no handle, no device.
int taco_debug_wgrad_plan(int wgrad_bf3, int wgrad_planes, int deterministic, long long det_floats, long long planes_uint4, int region_open,
                          int M, int T, int K, int N, int kw, int padl, int gather, int ygather, int nw, int* out8) {
  if (!out8 || det_floats < 0 || planes_uint4 < 0 || M < 1 || K < 1 || N < 1 || kw < 1 || nw < 0) return fail(TACO_ERR_ARG, "bad argument");
  const WgEnv e{wgrad_bf3, planes_uint4 ? wgrad_planes : 0, deterministic != 0, (size_t)det_floats, (size_t)planes_uint4, region_open != 0};
  const WgPlan p = nw ? wgrad_bank_plan(e, M, T, K, N, nw, gather != 0) : wgrad_plan(e, M, T, K, N, kw, padl, gather != 0, ygather != 0);
  const int o[8] = {p.engine, p.rpb, p.nsplit, p.a_per_tap, p.Mp, (int)p.na, (int)p.nb, p.why ? 1 : 0};
  memcpy(out8, o, sizeof o);
  return 0;
}
// Test hook: the host half of taco_model_finalize alone (model_pack_host) -- no handle, no device.
static uint64_t fnv1a64(const void* p, size_t n, uint64_t h = 14695981039346656037ull) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
static uint64_t pack_mask(const taco_model* m) {
  uint64_t k = 0;
  auto bit = [&](int b, bool on) { if (on) k |= 1ull << b; };
  bit(0, m->dx_pack); bit(1, m->dx_p1o_raw); bit(2, m->dx_spkw);
  for (int q = 0; q < 4; ++q) bit(3 + q, m->dx_qpack[q]);
  bit(7, m->dbx_pack);
  const Cbhg* cb[2] = {&m->enc, &m->post};
  for (int i = 0; i < 2; ++i) {
    const Cbhg& c = *cb[i];
    bit(8 + i, c.gd_pack && c.go_pack[0] && c.go_pack[1] && c.go_pack[2]);
    bit(10 + i, c.gb_pack && c.gob_pack);
    bit(12 + i, c.front_kind != 0);
    bit(20, c.res_g2p[0] && c.res_g2p[1] && c.res_c1p[0] && c.res_c1p[1]);
  }
  for (auto& kv : m->convs) bit(14, kv.second.wtail);
  bit(15, !m->spk_table.empty()); bit(16, !m->spk_dense.empty());
  bit(17, m->att_b); bit(18, m->att_sb); bit(19, m->gru1_fold.gx.wp);
  return k;
}
int taco_debug_pack_host(const taco_hparams* hp, int shadow, const float* flat_weights, size_t n_floats, uint64_t out[5]) {
  if (!hp || !out || (shadow != 0) != (flat_weights == nullptr)) return fail(TACO_ERR_ARG, "bad argument (a shadow model takes no weights)");
  taco_train* t = new taco_train();
  int rc = taco_model_create(hp, 0, &t->sm);
  if (rc != 0) { delete t; return rc; }
  taco_model* m = t->sm;
  if (shadow) rc = train_shadow_weights(t);
  else {
    size_t total = 0;
    for (auto& s : m->spec) { size_t cnt = 1; for (int64_t d : s.second) cnt *= (size_t)d; total += cnt; }
    if (n_floats != total) rc = fail(TACO_ERR_SHAPE, "%zu floats, the spec holds %zu", n_floats, total);
    for (size_t i = 0, off = 0; rc == 0 && i < m->spec.size(); ++i) {
      HostTensor& ht = m->raw[m->spec[i].first];
      ht.shape = m->spec[i].second;
      size_t cnt = 1; for (int64_t d : ht.shape) cnt *= (size_t)d;
      ht.data.assign(flat_weights + off, flat_weights + off + cnt); ht.set = true;
      off += cnt;
    }
  }
  if (rc == 0) rc = model_pack_host(m);
  if (rc == 0) {
    out[0] = m->harena.size();
    out[1] = fnv1a64(m->harena.data(), m->harena.size() * sizeof(float));
    out[2] = fnv1a64(m->hvars.data(), m->hvars.size() * sizeof(GemmVar));
    out[3] = (m->bf3_idx.empty() && m->bf3_segs.empty()) ? 0
             : fnv1a64(m->bf3_segs.data(), m->bf3_segs.size() * sizeof(Bf3Seg), fnv1a64(m->bf3_idx.data(), m->bf3_idx.size() * sizeof(unsigned)));
    out[4] = pack_mask(m);
  }
  taco_train_destroy(t);
  return rc;
}
size_t taco_train_num_params(const taco_train* t) { return t ? t->NP : 0; }

int taco_train_param_offset(const taco_train* t, const char* name, size_t* offset) {
  if (!t || !name || !offset) return fail(TACO_ERR_ARG, "null argument");
  auto it = t->poff.find(name);
  if (it == t->poff.end()) return fail(TACO_ERR_ARG, "unknown parameter '%s'", name);
  *offset = it->second;
  return 0;
}

int taco_train_refresh(taco_train* t, void* hip_stream, const float* d_params) {
  if (!t || !d_params) return fail(TACO_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(t->sm->device));
  const taco_model* sm = t->sm;
  if (sm->dx_fold_n) {   // the persistent decoder's one computed operand: concat projection folded into GRU 1, from the current parameters
    const int H = sm->hp.dec_rnn_size, Z = sm->hp.attention_state_size + 2 * sm->hp.enc_rnn_size + simple_S(sm);
    hipLaunchKernelGGL(k_dx_fold, dim3((Z + 1 + DXF_ROWS - 1) / DXF_ROWS), dim3(256), 0, (hipStream_t)hip_stream, d_params + t->poff.at("decoder/concat_projection/kernel"),
                       d_params + t->poff.at("decoder/concat_projection/bias"), d_params + t->poff.at("decoder/gru_1/gates/kernel"),
                       d_params + t->poff.at("decoder/gru_1/gates/bias"), d_params + t->poff.at("decoder/gru_1/candidate/kernel"), t->d_fold, Z, H);
  }
  hipLaunchKernelGGL(k_pack_gather, dim3(2048), dim3(256), 0, (hipStream_t)hip_stream, t->d_map, d_params, t->sm->darena, t->arena_n, (unsigned)t->NP,
                     (const float*)t->d_fold, (unsigned)sm->dx_fold_n);
  t->bf3_current = t->d_bf3_idx && (t->sm->bf3 || t->want_bf3_planes);
  if (t->bf3_current)                   // the same weights as split-bf16 planes, when that engine is selected (the map holds zeros there: this runs after the fp32 gather)
    hipLaunchKernelGGL(k_bf3_gather, dim3(2048), dim3(256), 0, (hipStream_t)hip_stream, (const unsigned*)t->d_bf3_idx, (const Bf3Seg*)t->d_bf3_segs,
                       t->n_bf3_segs, d_params, t->sm->darena, t->n_bf3, (unsigned)t->NP);
  if (t->sm->hp.attention_type == 1)    // bah_norm: the pack holds v_hat = g * v / |v| (computed, not copied)
    hipLaunchKernelGGL(k_vnorm_fold, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, d_params + t->poff.at("attention/attention_v"),
                       d_params + t->poff.at("attention/attention_g"), t->sm->darena + (t->sm->att_v - 1), t->sm->hp.attention_size);
  HIPCHK(hipGetLastError());
  return 0;
}

size_t taco_train_workspace_bytes(const taco_train* t, int B, int T_in, int T_out) {
  if (!t || B <= 0 || T_in <= 0 || T_out <= 0) return 0;
  const int r = t->sm->hp.reduction_factor;
  Carver cv(nullptr, 0);
  TrainWs w; carve_train(cv, t, B, T_in, (T_out + r - 1) / r, w);
  return cv.off;
}

int taco_train_forward_backward(taco_train* t, void* hip_stream, float* d_params, float* d_grads, const int32_t* d_inputs,
                                const int32_t* d_input_lengths, const int32_t* d_speaker_id, const float* d_mel_targets, const float* d_linear_targets,
                                const float* d_loss_coeff, int B, int T_in, int T_out, int prioritize_loss, int sample_rate, float* d_losses,
                                float* d_mel_out, float* d_linear_out, float* d_alignments, int rnn_decoder_test_mode, void* d_workspace,
                                size_t workspace_bytes) {
  if (!t || !d_params || !d_inputs || !d_input_lengths || !d_mel_targets || !d_linear_targets || !d_workspace)
    return fail(TACO_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(t->sm->device));
  TRY(train_forward_backward(t, (hipStream_t)hip_stream, d_params, d_grads, d_inputs, d_input_lengths, d_speaker_id, d_mel_targets, d_linear_targets,
                             d_loss_coeff, B, T_in, T_out, prioritize_loss, sample_rate, d_losses, d_mel_out, d_linear_out, d_alignments,
                             d_workspace, workspace_bytes, d_grads != nullptr, (rnn_decoder_test_mode & 1) != 0, (rnn_decoder_test_mode & 2) != 0));
  // A persistent kernel that gave up (bounded spin expired: the chip was shared, or a workgroup never became resident) leaves tape and
  // gradients invalid.  The step says so in its own outputs: losses and the first gradient element become NaN -- which survives the
  // data-parallel all-reduce, so EVERY rank's clip-and-Adam (k_adam) sees a non-finite global norm and skips the update.
  hipLaunchKernelGGL(k_train_latch, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, (const unsigned*)t->sm->d_err, d_losses, d_grads);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- segmented norms: per-variable gradient norms, their maximum and the global norm (add_stats, train.py:50-77) ----
int taco_segnorm_piece_floats(void) { return SEGN_P; }

// Test hook: the host-only piece table builder (taco_segnorm.h) -- no handle, no device.
int taco_debug_segnorm_pieces(const uint64_t* h_offsets, int n_seg, const uint8_t* h_skip, uint64_t* out_begin, int32_t* out_len,
                              int32_t* out_seg, int cap, int* n_pieces) {
  if (!h_offsets || !out_begin || !out_len || !out_seg || !n_pieces || cap < 0) return fail(TACO_ERR_ARG, "null argument or negative cap");
  std::vector<SegPiece> pieces; std::vector<int> pfirst;
  if (const char* why = segnorm_pieces(h_offsets, n_seg, h_skip, pieces, pfirst)) return fail(TACO_ERR_ARG, "%s", why);
  *n_pieces = (int)pieces.size();
  if (pieces.size() > (size_t)cap) return fail(TACO_ERR_ARG, "%zu pieces, room for %d", pieces.size(), cap);
  for (size_t i = 0; i < pieces.size(); ++i) { out_begin[i] = pieces[i].begin; out_len[i] = pieces[i].len; out_seg[i] = pieces[i].seg; }
  return 0;
}

// the host half of a plan: the table is built and checked, nothing is allocated
static int segnorm_plan_host(const uint64_t* h_offsets, int n_seg, const uint8_t* h_skip, int device, taco_segnorm_plan** out,
                             std::vector<SegPiece>& pieces, std::vector<int>& pfirst, std::vector<unsigned char>& skip) {
  if (!h_offsets || !out) return fail(TACO_ERR_ARG, "null argument");
  if (const char* why = segnorm_pieces(h_offsets, n_seg, h_skip, pieces, pfirst)) return fail(TACO_ERR_ARG, "%s", why);
  skip.assign((size_t)n_seg, 0);
  for (int s = 0; h_skip && s < n_seg; ++s) skip[s] = h_skip[s] ? 1 : 0;
  taco_segnorm_plan* p = new taco_segnorm_plan();
  p->device = device; p->n_seg = n_seg; p->n_pieces = (int)pieces.size(); p->end = h_offsets[n_seg];
  *out = p;
  return 0;
}
// Test hook: a plan that stays on the host -- no device is touched.  It serves the argument checks of taco_segment_norms, which come before
// its first device call, on a machine without a GPU; a call that passes them is refused with TACO_ERR_STATE.  Freed by taco_segnorm_plan_destroy.
int taco_debug_segnorm_plan_create_host(const uint64_t* h_offsets, int n_seg, const uint8_t* h_skip, taco_segnorm_plan** out) {
  std::vector<SegPiece> pieces; std::vector<int> pfirst; std::vector<unsigned char> skip;
  return segnorm_plan_host(h_offsets, n_seg, h_skip, 0, out, pieces, pfirst, skip);
}

int taco_segnorm_plan_create(const uint64_t* h_offsets, int n_seg, const uint8_t* h_skip, int device, taco_segnorm_plan** out) {
  std::vector<SegPiece> pieces; std::vector<int> pfirst; std::vector<unsigned char> skip;
  taco_segnorm_plan* p = nullptr;
  if (!out) return fail(TACO_ERR_ARG, "null argument");
  TRY(segnorm_plan_host(h_offsets, n_seg, h_skip, device, &p, pieces, pfirst, skip));
  const size_t np = std::max<size_t>(pieces.size(), 1);      // (a table without pieces -- every segment empty or skipped -- launches no k_segsq_piece)
  if (hipSetDevice(device) != hipSuccess ||
      hipMalloc((void**)&p->d_pieces, np * sizeof(SegPiece)) != hipSuccess ||
      hipMalloc((void**)&p->d_partial, np * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&p->d_pfirst, pfirst.size() * sizeof(int)) != hipSuccess ||
      hipMalloc((void**)&p->d_skip, skip.size()) != hipSuccess ||
      hipMalloc((void**)&p->d_segsum, (size_t)n_seg * sizeof(double)) != hipSuccess ||
      (!pieces.empty() && hipMemcpy(p->d_pieces, pieces.data(), pieces.size() * sizeof(SegPiece), hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(p->d_pfirst, pfirst.data(), pfirst.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(p->d_skip, skip.data(), skip.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    taco_segnorm_plan_destroy(p);
    return fail(TACO_ERR_HIP, "segment table allocation failed");
  }
  *out = p;
  return 0;
}

void taco_segnorm_plan_destroy(taco_segnorm_plan* p) {
  if (!p) return;
  if (p->d_pieces) (void)hipFree(p->d_pieces);
  if (p->d_partial) (void)hipFree(p->d_partial);
  if (p->d_pfirst) (void)hipFree(p->d_pfirst);
  if (p->d_skip) (void)hipFree(p->d_skip);
  if (p->d_segsum) (void)hipFree(p->d_segsum);
  delete p;
}

// the argument checks of a call that do not need the plan: all before any HIP call
static int segnorm_check_buffers(const float* d_flat, size_t n, int n_seg, const float* d_norms, const float* d_stats, const int32_t* d_argmax) {
  if (!d_flat || !d_norms || !d_stats) return fail(TACO_ERR_ARG, "null pointer");
  if (reinterpret_cast<uintptr_t>(d_flat) & 3) return fail(TACO_ERR_ARG, "the input buffer %p is not 4-byte aligned", (const void*)d_flat);
  const Span in = {d_flat, (u128)n * sizeof(float), "the input buffer"};      // each output against the input, not against the other outputs
  TRY(no_overlap({{d_norms, (u128)(size_t)n_seg * sizeof(float), "d_norms"}, in}, 1));
  TRY(no_overlap({{d_stats, 2 * sizeof(float), "d_stats"}, in}, 1));
  return no_overlap({{d_argmax, sizeof(int32_t), "d_argmax"}, in}, 1);
}

int taco_segment_norms(const taco_segnorm_plan* p, void* hip_stream, const float* d_flat, size_t n, float* d_norms, float* d_stats, int32_t* d_argmax) {
  if (!p) return fail(TACO_ERR_ARG, "null pointer");
  TRY(segnorm_check_buffers(d_flat, n, p->n_seg, d_norms, d_stats, d_argmax));
  if (p->end > n) return fail(TACO_ERR_ARG, "the segment table ends at element %llu, the buffer holds %zu", (unsigned long long)p->end, n);
  if (!p->d_pfirst) return fail(TACO_ERR_STATE, "a host-only plan (taco_debug_segnorm_plan_create_host) cannot run");
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHK(hipSetDevice(p->device));
  if (p->n_pieces) hipLaunchKernelGGL(k_segsq_piece, dim3((unsigned)p->n_pieces), dim3(TR_NT), 0, st, d_flat, (const SegPiece*)p->d_pieces, p->d_partial);
  hipLaunchKernelGGL(k_segsq_segment, dim3((unsigned)cdiv(p->n_seg, TR_NT / 64)), dim3(TR_NT), 0, st, (const double*)p->d_partial, (const int*)p->d_pfirst,
                     p->n_seg, p->d_segsum, d_norms);
  hipLaunchKernelGGL(k_segnorm_stats, dim3(1), dim3(TR_NT), 0, st, (const double*)p->d_segsum, (const float*)d_norms, (const unsigned char*)p->d_skip,
                     p->n_seg, d_stats, d_argmax);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_train_grad_norms(taco_train* t, void* hip_stream, const float* d_grads, float* d_norms, float* d_stats, int32_t* d_argmax) {
  if (!t || !d_grads || !d_norms || !d_stats) return fail(TACO_ERR_ARG, "null pointer");
  TRY(segnorm_check_buffers(d_grads, t->NP, (int)t->sm->spec.size(), d_norms, d_stats, d_argmax));
  if (!t->gn_plan) {      // one segment per spec tensor, in spec order = flat order; the BatchNorm moving statistics are no trainable variables
    const auto ends_with = [](const std::string& s, const char* tail) { const size_t k = strlen(tail); return s.size() >= k && s.compare(s.size() - k, k, tail) == 0; };
    std::vector<uint64_t> off; std::vector<uint8_t> skip;
    for (auto& s : t->sm->spec) {
      off.push_back(t->poff.at(s.first));
      skip.push_back(ends_with(s.first, "/moving_mean") || ends_with(s.first, "/moving_variance"));
    }
    off.push_back(t->NP);
    TRY(taco_segnorm_plan_create(off.data(), (int)skip.size(), skip.data(), t->sm->device, &t->gn_plan));
  }
  return taco_segment_norms(t->gn_plan, hip_stream, d_grads, t->NP, d_norms, d_stats, d_argmax);
}

// Timing hook: k_sumsq_partial alone, launched as taco_adam_step_f32 launches it -- the yardstick of taco_train_grad_norms (both read the same bytes once).
int taco_debug_sumsq_partial(void* hip_stream, const float* d_grads, size_t n, void* d_workspace, size_t workspace_bytes) {
  if (!d_grads || !d_workspace || n == 0) return fail(TACO_ERR_ARG, "bad argument");
  if (workspace_bytes < (size_t)TR_MAXBLK * sizeof(double)) return fail(TACO_ERR_STATE, "workspace too small");
  if ((reinterpret_cast<uintptr_t>(d_grads) & 15) != 0) return fail(TACO_ERR_ARG, "gradient buffer must be 16-byte aligned");
  const int nblk = (int)std::min<size_t>(TR_MAXBLK, (n + TR_NT * 16 - 1) / (TR_NT * 16));
  hipLaunchKernelGGL(k_sumsq_partial, dim3(nblk), dim3(TR_NT), 0, (hipStream_t)hip_stream, d_grads, n, (double*)d_workspace);
  HIPCHK(hipGetLastError());
  return 0;
}
