// taco_pack.h -- the model build (included by taco_lib.hip behind the model structs): everything between taco_model_create and the arena
// upload.  Host arithmetic only -- no HIP runtime call -- so that model_pack_host runs on a machine without a GPU (taco_debug_pack_host,
// tests/test_pack_host.py).  This is where the memory layouts the kernels read are DEFINED: each is described once, at its builder, with
// the kernel header that consumes it.  A wrong index here does not crash, it makes a slightly wrong model: the test holds every pack of
// nine models to recorded digests.
#pragma once

static size_t arena_put(taco_model* m, const float* src, size_t n) {
  size_t off = rup_sz(m->harena.size(), 16);
  m->harena.resize(off + rup_sz(std::max<size_t>(n, 1), 16), 0.f);
  if (src) memcpy(&m->harena[off], src, n * sizeof(float));
  return off + 1;
}
static size_t arena_put(taco_model* m, const std::vector<float>& v) { return arena_put(m, v.data(), v.size()); }
static size_t arena_put_u16(taco_model* m, const std::vector<unsigned short>& v) {      // bf16 planes ride in the float arena, two per element
  std::vector<float> f((v.size() + 1) / 2, 0.f);
  memcpy(f.data(), v.data(), v.size() * sizeof(unsigned short));
  return arena_put(m, f);
}

// A tensor of the model by name.  An unknown or unset name is a bug of a builder below (taco_model_finalize has checked the spec before):
// it ends the pack step with TACO_ERR_STATE (model_pack_host) instead of inserting an empty tensor that the next line reads past.
struct PackMissing { std::string name; };
static const HostTensor& T_(const taco_model* m, const std::string& n) {
  const auto it = m->raw.find(n);
  if (it == m->raw.end() || !it->second.set) throw PackMissing{n};
  return it->second;
}
static const std::vector<float>& TD(const taco_model* m, const std::string& n) { return T_(m, n).data; }
// kernels and biases of one direction of a CBHG's BiGRU
struct GruW { const std::vector<float>&gk, &gb, &ck, &cb; };
static GruW gru_w(const taco_model* m, const std::string& n) {
  return {TD(m, n + "/gates/kernel"), TD(m, n + "/gates/bias"), TD(m, n + "/candidate/kernel"), TD(m, n + "/candidate/bias")};
}
static GruW bigru_w(const taco_model* m, const std::string& sc, int dir) { return gru_w(m, sc + "/bigru/" + (dir ? "bw" : "fw")); }

static bool is_deepvoice(const taco_model* m) { return m->hp.num_speakers > 1 && m->hp.model_type == 2; }
static bool is_simple(const taco_model* m) { return m->hp.num_speakers > 1 && m->hp.model_type == 1; }
static int simple_S(const taco_model* m) { return is_simple(m) ? m->hp.speaker_embedding_size : 0; }

// ---- GEMM and skinny packs ----
// W32 pack of a [kw, cin, N] kernel (dense: kw = 1): see taco_kernels.h.
static size_t pack_w32(taco_model* m, const float* W, int kw, int cin, int N, int* cin_pad_out) {
  const int cin_pad = rup(cin, 8), Kq = kw * cin_pad / 4, NT = cdiv(N, 32);
  std::vector<float> p((size_t)NT * Kq * 32 * 4, 0.f);
  for (int nt = 0; nt < NT; ++nt)
    for (int kq = 0; kq < Kq; ++kq)
      for (int j = 0; j < 32; ++j)
        for (int e = 0; e < 4; ++e) {
          const int k = 4 * kq + e, tap = k / cin_pad, c = k % cin_pad, n = 32 * nt + j;
          if (c < cin && n < N) p[(((size_t)nt * Kq + kq) * 32 + j) * 4 + e] = W[((size_t)tap * cin + c) * N + n];
        }
  *cin_pad_out = cin_pad;
  return arena_put(m, p);
}
// split-bf16 pack of a [kw, cin, N] kernel for k_gemm_bf3: hi = bf16(w), lo = bf16(w - hi), k16-major layout in taco_kernels.h
static unsigned short bf16_rne_host(float x) {
  unsigned u; memcpy(&u, &x, 4);
  return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
static float bf16_to_float(unsigned short b) { unsigned u = (unsigned)b << 16; float f; memcpy(&f, &u, 4); return f; }
static void pack_bf3(taco_model* m, const float* W, int kw, int cin, int N, size_t* hi_out, size_t* lo_out, int* K16_out, int* cp16_out, size_t* l3_out = nullptr) {
  const int cp16 = rup(cin, 32), K16 = kw * cp16 / 16, NT = cdiv(N, 32);   // multiple of 32: k_gemm_bf3 walks k16 groups in pairs
  std::vector<unsigned short> hi((size_t)NT * K16 * 2 * 32 * 8, 0), lo(hi.size(), 0);
  std::vector<unsigned> idx(m->tp ? hi.size() : 0, 0u);
  const bool want_l3 = l3_out && !m->tp && *l3_out == (size_t)1;     // inference model, caller asks (*l3_out preset to 1) for the third plane too
  std::vector<unsigned short> l3v(want_l3 ? hi.size() : 0, 0);
  for (int nt = 0; nt < NT; ++nt)
    for (int k16 = 0; k16 < K16; ++k16)
      for (int h = 0; h < 2; ++h)
        for (int j = 0; j < 32; ++j)
          for (int e = 0; e < 8; ++e) {
            const int k = 16 * k16 + 8 * h + e, tap = k / cp16, c = k % cp16, n = 32 * nt + j;
            if (c >= cin || n >= N) continue;
            const float w = W[((size_t)tap * cin + c) * N + n];
            const size_t o = ((((size_t)k16 * NT + nt) * 2 + h) * 32 + j) * 8 + e;
            if (m->tp) { idx[o] = (unsigned)w; continue; }       // shadow model: `w` is 1 + a parameter index (k_bf3_gather splits the live value)
            const float hf = bf16_to_float(hi[o] = bf16_rne_host(w));
            lo[o] = bf16_rne_host(w - hf);
            if (want_l3) l3v[o] = bf16_rne_host(w - hf - bf16_to_float(lo[o]));
          }
  *hi_out = arena_put_u16(m, hi); *lo_out = arena_put_u16(m, lo); *K16_out = K16; *cp16_out = cp16;
  if (want_l3) *l3_out = arena_put_u16(m, l3v);
  else if (l3_out && !m->tp) *l3_out = 0;
  if (m->tp) {
    // third plane (zeros here: k_bf3_gather fills all three from the live parameters): the operand of the six-product instantiation
    const size_t l3 = arena_put_u16(m, std::vector<unsigned short>(hi.size(), 0));
    if (l3_out) *l3_out = l3;
    m->bf3_segs.push_back(Bf3Seg{(unsigned)m->bf3_idx.size(), (unsigned)idx.size(), (unsigned long long)(*hi_out - 1), (unsigned long long)(*lo_out - 1), (unsigned long long)(l3 - 1)});
    m->bf3_idx.insert(m->bf3_idx.end(), idx.begin(), idx.end());
  }
}

// W16 pack of rows [r0, r0+K) and columns [c0, c0+N) of a row-major [*, ldw] matrix.
static SkW pack_w16(taco_model* m, const float* W, int ldw, int r0, int K, int c0, int N, const float* bias) {
  SkW s; s.K = K; s.N = N;
  const int Kpad = rup(K, 16), NT = cdiv(N, 16);
  s.Kq = Kpad / 4;
  std::vector<float> p((size_t)NT * s.Kq * 16 * 4, 0.f);
  for (int nt = 0; nt < NT; ++nt)
    for (int kq = 0; kq < s.Kq; ++kq)
      for (int j = 0; j < 16; ++j)
        for (int e = 0; e < 4; ++e) {
          const int k = 4 * kq + e, n = 16 * nt + j;
          if (k < K && n < N) p[(((size_t)nt * s.Kq + kq) * 16 + j) * 4 + e] = W[(size_t)(r0 + k) * ldw + c0 + n];
        }
  s.wp = arena_put(m, p);
  if (bias) s.bias = arena_put(m, bias + c0, N);
  return s;
}
// a whole [K, N] matrix (+ bias) by name
static SkW pack_w16_named(taco_model* m, const std::string& name, int K, int N, bool bias = true) {
  return pack_w16(m, TD(m, name + "/kernel").data(), N, 0, K, 0, N, bias ? TD(m, name + "/bias").data() : nullptr);
}

// fp32 pack and (bf3) split-bf16 planes of one [kw, cin, N] matrix; on an inference model the third plane too (*l3 preset to 1: every
// layer can run the six-product instantiation, taco_debug_set_bf3 bit 64)
static void pack_gemm_weights(taco_model* m, ConvL& L, const float* W, bool bf3) {
  L.wp = pack_w32(m, W, L.kw, L.cin, L.N, &L.cin_pad);
  if (bf3 && !m->tp) L.bl3 = 1;
  if (bf3) pack_bf3(m, W, L.kw, L.cin, L.N, &L.bh, &L.bl, &L.K16, &L.cin_pad16, &L.bl3);
}
static ConvL make_conv(taco_model* m, const std::string& name, bool bn, bool has_bias = true, bool bf3 = false, bool x6 = false) {
  const HostTensor& k = T_(m, name + "/kernel");
  const int conv = k.shape.size() == 3;      // [kw, cin, N], or a dense [cin, N]
  ConvL L; L.kw = conv ? (int)k.shape[0] : 1; L.cin = (int)k.shape[conv]; L.N = (int)k.shape[conv + 1];
  L.x6 = x6;                                 // this layer runs the six-product instantiation by default
  pack_gemm_weights(m, L, k.data.data(), bf3);
  if (bf3 && L.kw == 1 && L.N >= 512 && L.N % 32 > 0 && L.N % 32 <= 4 && (L.cin == 256 || L.cin == 512)) {
    L.ntail = L.N % 32;
    std::vector<float> wt((size_t)L.ntail * L.cin);
    for (int t = 0; t < L.ntail; ++t)
      for (int kk = 0; kk < L.cin; ++kk) wt[(size_t)t * L.cin + kk] = k.data[(size_t)kk * L.N + (L.N - L.ntail + t)];
    L.wtail = arena_put(m, wt);
  }
  if (has_bias) L.bias = arena_put(m, TD(m, name + "/bias").data(), L.N);
  if (bn) {  // BatchNorm inference folded to y*scale + shift (A.2; epsilon 1e-3 = tf.layers default)
    const auto& g = TD(m, name + "/gamma"); const auto& b = TD(m, name + "/beta");
    const auto& mu = TD(m, name + "/moving_mean"); const auto& var = TD(m, name + "/moving_variance");
    std::vector<float> sc(L.N), sh(L.N);
    for (int i = 0; i < L.N; ++i) {
      const double s = (double)g[i] / std::sqrt((double)var[i] + 1e-3);
      sc[i] = (float)s; sh[i] = (float)((double)b[i] - (double)mu[i] * s);
    }
    L.bns = arena_put(m, sc.data(), L.N); L.bnb = arena_put(m, sh.data(), L.N);
  }
  return L;
}

static GruDec make_grudec(taco_model* m, const std::string& name, int I, int H) {
  GruDec g; g.I = I; g.H = H;
  const GruW w = gru_w(m, name);
  // one [I+H, 3H] matrix: columns [0,2H) = gates/kernel, columns [2H,3H) = candidate/kernel rows of x
  // (rows of h zero: the candidate's h part needs r first and runs in the second launch)
  std::vector<float> W((size_t)(I + H) * 3 * H, 0.f), b(3 * H, 0.f);
  for (int i = 0; i < I + H; ++i) {
    for (int j = 0; j < 2 * H; ++j) W[(size_t)i * 3 * H + j] = w.gk[(size_t)i * 2 * H + j];
    if (i < I) for (int j = 0; j < H; ++j) W[(size_t)i * 3 * H + 2 * H + j] = w.ck[(size_t)i * H + j];
  }
  for (int j = 0; j < 2 * H; ++j) b[j] = w.gb[j];
  g.gx = pack_w16(m, W.data(), 3 * H, 0, I + H, 0, 3 * H, b.data());
  g.ch = pack_w16(m, w.ck.data(), H, I, H, 0, H, w.cb.data());    // h rows of candidate/kernel (+ candidate bias)
  return g;
}

// ---- register packs of the persistent kernels ----
// Every persistent kernel keeps its weights in registers: 512 threads (8 waves of 64 lanes), thread tid reads register r of block `member`
// from pack[(member * nreg + r) * 512 + tid].  Two mappings of a matrix onto lanes exist, and these two functions are the only code that
// spells them out:
//   fill_cols (forward kernels): a wave owns a COLUMN, a lane kw consecutive rows of it:      reg0 + e = W[row0 + kw lane + e][col(wave)]
//   fill_rows (backward kernels): a wave owns a ROW, a lane kw consecutive columns of it:     reg0 + e = W[row(wave)][col0 + kw lane + e]
// col(wave) / row(wave) < 0: the wave holds nothing (zeros); fill_rows leaves columns from ncols on zero.
#define PK_NT 512
static_assert(PK_NT == DX_NT, "the register packs are laid out for 512 threads");
template <class ColFn>
static void fill_cols(std::vector<float>& pack, int nreg, int member, int reg0, int kw, const float* W, int ldw, int row0, ColFn col) {
  for (int tid = 0; tid < PK_NT; ++tid) {
    const int wave = tid >> 6, lane = tid & 63, n = col(wave);
    if (n < 0) continue;
    for (int e = 0; e < kw; ++e)
      pack[((size_t)member * nreg + reg0 + e) * PK_NT + tid] = W[(size_t)(row0 + kw * lane + e) * ldw + n];
  }
}
template <class RowFn>
static void fill_rows(std::vector<float>& pack, int nreg, int member, int reg0, int kw, const float* W, int ldw, RowFn row, int col0, int ncols) {
  for (int tid = 0; tid < PK_NT; ++tid) {
    const int wave = tid >> 6, lane = tid & 63, r = row(wave);
    if (r < 0) continue;
    for (int e = 0; e < kw; ++e) {
      const int c = col0 + kw * lane + e;
      if (c < ncols) pack[((size_t)member * nreg + reg0 + e) * PK_NT + tid] = W[(size_t)r * ldw + c];
    }
  }
}

// The persistent decoder exists for 256-wide cells and memory, two decoder layers, and the attention widths / prenet depths of the presets of
// hparams.py:71-117: attention_size 128 / 256 / 512, dec_prenet_sizes [256, 128] or [256, 128, 64].
static int dx_prenet_depth(const taco_model* m) {
  const taco_hparams& hp = m->hp;
  if (hp.dec_prenet_n == 2 && hp.dec_prenet[0] == DX_W && hp.dec_prenet[1] == DX_P2) return 2;
  if (hp.dec_prenet_n == 3 && hp.dec_prenet[0] == DX_W && hp.dec_prenet[1] == DX_P2 && hp.dec_prenet[2] == DX_P3) return 3;
  return 0;
}
static bool dx_reference_widths(const taco_model* m) { return m->hp.attention_size == DX_W && dx_prenet_depth(m) == 2; }
static bool dx_widths_ok(const taco_model* m) {
  const taco_hparams& hp = m->hp;
  const bool aw = hp.attention_size == 128 || hp.attention_size == 256 || hp.attention_size == 512;
  return hp.attention_state_size == DX_W && hp.dec_rnn_size == DX_W && aw && 2 * hp.enc_rnn_size == DX_W && dx_prenet_depth(m) != 0 &&
         hp.dec_layer_num == 2 && hp.num_mels * hp.reduction_factor <= 16 * DX_GROUP &&
         (dx_reference_widths(m) || !m->tp);       // the training forward / BPTT kernels: reference widths only
}
// k_decoder_xcd (taco_decoder_xcd.h, DXR_*): [32 members][DX_NREG][512], columns (fill_cols) -- wave w of member m owns column 8m + w of a
// 256-wide output (4m + w on waves 0-3 of a 128-wide one), a lane four input rows per register quad.
// Wc/bc: composite prenet layer 1 of the next step ([o | ctx] rows); Wf/bf: GRU 1 with the concat projection folded in
// ([h_att | ctx | h1] rows x [r | u | candidate-x | o0] columns): compose_prenet1_next / compose_gru1_fold, or their shadow-model forms
struct Composite { std::vector<float> W, b; };
static void dx_build_pack(taco_model* m, const Composite& p1, const Composite& g1) {
  if (!dx_widths_ok(m)) return;
  const taco_hparams& hp = m->hp;
  const std::vector<float>&Wc = p1.W, &Wf = g1.W;
  const int H = DX_W, rM = hp.num_mels * hp.reduction_factor, NCF = cdiv(rM, DX_GROUP);
  const int S = simple_S(m);                                      // 'simple': S speaker rows behind the prenet output / behind [h_att | ctx]
  const int PD = dx_prenet_depth(m), AW = hp.attention_size;
  const int IA = (PD == 3 ? DX_P3 : DX_P2) + S, Z = 2 * H + S;    // first h row of the attention GRU kernels / of the folded GRU 1 matrix
  std::vector<float> pack((size_t)DX_GROUP * DX_NREG * DX_NT, 0.f);
  const auto& W2 = TD(m, "decoder/prenet/dense_2/kernel");
  const auto& agk = TD(m, "decoder/attention_gru/gates/kernel"); const auto& ack = TD(m, "decoder/attention_gru/candidate/kernel");
  const auto& wq = TD(m, "attention/query_layer/kernel");
  const auto& c1k = TD(m, "decoder/gru_1/candidate/kernel");
  const auto& g2k = TD(m, "decoder/gru_2/gates/kernel"); const auto& c2k = TD(m, "decoder/gru_2/candidate/kernel");
  const auto& fk = TD(m, "decoder/frame_projection/kernel");
  for (int mem = 0; mem < DX_GROUP; ++mem) {
    auto c8 = [&](int w) { return mem * 8 + w; };
    auto cu = [&](int w) { return H + mem * 8 + w; };                       // update-gate column (A.6: gates kernel = r | u)
    auto c4 = [&](int w) { return w < 4 ? mem * 4 + w : -1; };
    auto f0 = [&](int w) { const int n = mem * NCF + w; return (w < NCF && n < rM) ? n : -1; };
    auto f1 = [&](int w) { const int n = mem * NCF + w + 8; return (w + 8 < NCF && n < rM) ? n : -1; };
    auto put = [&](int reg0, int kw, const std::vector<float>& W, int ldw, int row0, auto col) { fill_cols(pack, DX_NREG, mem, reg0, kw, W.data(), ldw, row0, col); };
    put(DXR_P2, 4, W2, DX_P2, 0, c4);
    put(DXR_AGH, 4, agk, 2 * H, IA, c8); put(DXR_AGH + 4, 4, agk, 2 * H, IA, cu);                  // h rows
    if (PD == 3) {      // 64 input rows, one per lane: r, u, candidate-x in one register each; behind them prenet layer 3 (p2 -> column 2m + w, waves 0-1)
      put(DXR_AGX, 1, agk, 2 * H, 0, c8); put(DXR_AGX + 1, 1, agk, 2 * H, 0, cu); put(DXR_AGX + 2, 1, ack, H, 0, c8);
      put(DXR_AGX + 3, 2, TD(m, "decoder/prenet/dense_3/kernel"), DX_P3, 0, [&](int w) { return w < 2 ? mem * 2 + w : -1; });
    } else {
      put(DXR_AGX, 2, agk, 2 * H, 0, c8); put(DXR_AGX + 2, 2, agk, 2 * H, 0, cu); put(DXR_AGX + 4, 2, ack, H, 0, c8);
    }
    put(DXR_AC, 4, ack, H, IA, c8);
    auto fx = [&](int w) { return 2 * H + mem * 8 + w; };
    auto fo = [&](int w) { return 3 * H + mem * 8 + w; };
    put(DXR_G1H, 4, Wf, 4 * H, Z, c8); put(DXR_G1H + 4, 4, Wf, 4 * H, Z, cu);                        // h1 rows
    put(DXR_G1A, 4, Wf, 4 * H, 0, c8); put(DXR_G1A + 4, 4, Wf, 4 * H, 0, cu);                        // h_att rows
    put(DXR_G1A + 8, 4, Wf, 4 * H, 0, fx); put(DXR_G1A + 12, 4, Wf, 4 * H, 0, fo);
    put(DXR_G1B, 4, Wf, 4 * H, H, c8); put(DXR_G1B + 4, 4, Wf, 4 * H, H, cu);                        // context rows
    put(DXR_G1B + 8, 4, Wf, 4 * H, H, fx); put(DXR_G1B + 12, 4, Wf, 4 * H, H, fo);
    put(DXR_G1C, 4, c1k, H, H, c8);
    put(DXR_G2H, 4, g2k, 2 * H, H, c8); put(DXR_G2H + 4, 4, g2k, 2 * H, H, cu);
    put(DXR_G2X, 4, g2k, 2 * H, 0, c8); put(DXR_G2X + 4, 4, g2k, 2 * H, 0, cu); put(DXR_G2X + 8, 4, c2k, H, 0, c8);
    put(DXR_G2C, 4, c2k, H, H, c8);
    put(DXR_P1C, 4, Wc, DX_W, H, c8);                                                                // context rows of [o | ctx]
    put(DXR_P1O, 4, Wc, DX_W, 0, c8);
    put(DXR_F, 4, fk, rM, 0, f0); put(DXR_F + 4, 4, fk, rM, 0, f1);
  }
  m->dx_pack = arena_put(m, pack);
  if (!m->tp && dx_reference_widths(m)) {
    // teacher-forced decoding on an inference model (taco_decoder_forward with teacher frames): the TAPE instantiation reads the teacher's
    // frame with the RAW frame rows of prenet layer 1 where this pack holds the frame-projection composite -- four registers per thread
    const auto& W1 = TD(m, "decoder/prenet/dense_1/kernel");
    std::vector<float> raw((size_t)DX_W * DX_W, 0.f), alt((size_t)DX_GROUP * 4 * DX_NT, 0.f);
    for (int k = 0; k < hp.num_mels; ++k) for (int q = 0; q < DX_W; ++q) raw[(size_t)k * DX_W + q] = W1[(size_t)k * DX_W + q];
    for (int mem = 0; mem < DX_GROUP; ++mem) fill_cols(alt, 4, mem, 0, 4, raw.data(), DX_W, 0, [&](int w) { return mem * 8 + w; });
    m->dx_p1o_raw = arena_put(m, alt);
  }
  if (S) {   // speaker rows: [k][slot][n], slots in DXRB_* order
    std::vector<float> sw((size_t)S * DXRB_N * H);
    for (int k = 0; k < S; ++k)
      for (int n = 0; n < H; ++n) {
        float* o = &sw[(size_t)k * DXRB_N * H + n];
        const int px = IA - S;                                      // prenet output rows in front of the speaker rows
        o[DXRB_AR * H] = agk[(size_t)(px + k) * 2 * H + n]; o[DXRB_AU * H] = agk[(size_t)(px + k) * 2 * H + H + n];
        o[DXRB_AX * H] = ack[(size_t)(px + k) * H + n];
        const float* wf = &Wf[(size_t)(2 * H + k) * 4 * H];
        o[DXRB_G1R * H] = wf[n]; o[DXRB_G1U * H] = wf[H + n]; o[DXRB_G1X * H] = wf[2 * H + n]; o[DXRB_O0 * H] = wf[3 * H + n];
      }
    m->dx_spkw = arena_put(m, sw);
  }
  // query layer: slot s of a row (s = member % Pr) scores channel block s % Pc and holds columns (s % Pc)*DS + w*QC + i of it; one pack
  // per rows-per-group
  for (int q = 0; q < 4; ++q) {
    const int RG = 1 << q, Pr = DX_GROUP / RG, Pc = dx_score_blocks(RG), DS = AW / Pc, QC = DS / 8, QR = dx_q_regs(RG, AW);
    if (DS < 8 || DS > 64) continue;                                // (no instantiation: attention_size 512 at 8 rows per group)
    std::vector<float> qp((size_t)DX_GROUP * QR * DX_NT, 0.f);
    for (int mem = 0; mem < DX_GROUP; ++mem)
      for (int i = 0; i < QC; ++i) {
        const int cb = (mem % Pr) % Pc;
        fill_cols(qp, QR, mem, 4 * i, 4, wq.data(), AW, 0, [&](int w) { return cb * DS + w * QC + i; });
      }
    m->dx_qpack[q] = arena_put(m, qp);
  }
  m->dx_b_p1_0 = arena_put(m, TD(m, "decoder/prenet/dense_1/bias"));
  m->dx_b_p1c = arena_put(m, p1.b);
  m->dx_b_p2 = arena_put(m, TD(m, "decoder/prenet/dense_2/bias"));
  if (PD == 3) m->dx_b_p3 = arena_put(m, TD(m, "decoder/prenet/dense_3/bias"));
  m->dx_b_ag = arena_put(m, TD(m, "decoder/attention_gru/gates/bias"));
  m->dx_b_ac = arena_put(m, TD(m, "decoder/attention_gru/candidate/bias"));
  m->dx_b_g1f = arena_put(m, g1.b);
  m->dx_b_g1c = arena_put(m, TD(m, "decoder/gru_1/candidate/bias"));
  m->dx_b_g2g = arena_put(m, TD(m, "decoder/gru_2/gates/bias"));
  m->dx_b_g2c = arena_put(m, TD(m, "decoder/gru_2/candidate/bias"));
  m->dx_b_f = arena_put(m, TD(m, "decoder/frame_projection/bias"));
}

// k_decoder_bwd_xcd (taco_decoder_bwd_xcd.h, DBR_*): [32 members][DB_NREG][512], ROWS (fill_rows) of every matrix a gradient is pulled back
// through -- wave w of member m owns row 8m + w (128-wide inputs: row 4m + w on waves 0-3), a lane inputs 4 lane .. 4 lane + 3 per register quad.
static void dbx_build_pack(taco_model* m) {
  if (!dx_widths_ok(m)) return;
  const taco_hparams& hp = m->hp;
  const int H = DX_W, Mm = hp.num_mels;
  // 'simple': S speaker rows sit between the prenet rows and the h rows of the attention GRU kernels (and behind [h_att | ctx] in the
  // concat projection).  The embedding is constant over the loop, so its gradient is a sum over steps of products with those rows --
  // formed once after the launch from the time-summed pre-activation gradients (decoder_backward); the kernel only skips the rows.
  const int IA = DX_P2 + simple_S(m);
  std::vector<float> pack((size_t)DX_GROUP * DB_NREG * DX_NT, 0.f);
  const auto& g2k = TD(m, "decoder/gru_2/gates/kernel"); const auto& c2k = TD(m, "decoder/gru_2/candidate/kernel");
  const auto& g1k = TD(m, "decoder/gru_1/gates/kernel"); const auto& c1k = TD(m, "decoder/gru_1/candidate/kernel");
  const auto& cck = TD(m, "decoder/concat_projection/kernel");
  const auto& wq = TD(m, "attention/query_layer/kernel");
  const auto& agk = TD(m, "decoder/attention_gru/gates/kernel"); const auto& ack = TD(m, "decoder/attention_gru/candidate/kernel");
  const auto& W2 = TD(m, "decoder/prenet/dense_2/kernel"); const auto& W1 = TD(m, "decoder/prenet/dense_1/kernel");
  for (int mem = 0; mem < DX_GROUP; ++mem) {
    // row r0 + 8m + w of a matrix with `cols` columns: four registers for columns [0, 256), four more for [256, 512) of a gates kernel
    auto rows = [&](int reg0, const std::vector<float>& W, int cols, int r0) {
      for (int half = 0; half * H < cols; ++half)
        fill_rows(pack, DB_NREG, mem, reg0 + 4 * half, 4, W.data(), cols, [&](int w) { return r0 + mem * 8 + w; }, half * H, cols);
    };
    auto en2 = [&](int w) { return w < 4 ? mem * 4 + w : -1; };         // the prenet-output rows of the attention GRU (128)
    rows(DBR_C2X, c2k, H, 0); rows(DBR_C2H, c2k, H, H);
    rows(DBR_G2X, g2k, 2 * H, 0); rows(DBR_G2H, g2k, 2 * H, H);
    rows(DBR_C1X, c1k, H, 0); rows(DBR_C1H, c1k, H, H);
    rows(DBR_G1X, g1k, 2 * H, 0); rows(DBR_G1H, g1k, 2 * H, H);
    rows(DBR_CCA, cck, H, 0); rows(DBR_CCC, cck, H, H);
    rows(DBR_Q, wq, H, 0);
    fill_rows(pack, DB_NREG, mem, DBR_CAX, 4, ack.data(), H, en2, 0, H); rows(DBR_CAH, ack, H, IA);
    fill_rows(pack, DB_NREG, mem, DBR_GAX, 4, agk.data(), 2 * H, en2, 0, 2 * H); fill_rows(pack, DB_NREG, mem, DBR_GAX + 4, 4, agk.data(), 2 * H, en2, H, 2 * H);
    rows(DBR_GAH, agk, 2 * H, IA);
    fill_rows(pack, DB_NREG, mem, DBR_P2, 2, W2.data(), DX_P2, [&](int w) { return mem * 8 + w; }, 0, DX_P2);
    rows(DBR_P1C, W1, H, Mm);
  }
  m->dbx_pack = arena_put(m, pack);
}

// ---- CBHG ----
static void cbhg_dims(Cbhg& c, int in_dim, int K, int C, int maxpool, int depth, int rnn, const int* projs, int nproj, int pw) {
  c.in_dim = in_dim; c.K = K; c.C = C; c.maxpool = maxpool; c.depth = depth; c.rnn = rnn; c.pw = pw; c.nproj = nproj;
  for (int i = 0; i < nproj; ++i) c.proj_dim[i] = projs[i];
}
// Forward scans k_bigru_oct<UPW> and k_bigru_duo (taco_bigru_xcd.h): [2 dirs][32 / UPW members][12 UPW][512], columns (fill_cols) of the
// recurrent (h-row) kernels.  Wave w of member mem owns units 8 UPW mem + UPW w + i of BOTH directions; a lane holds h rows 4 lane .. 4 lane + 3
// of the gate columns r_0, u_0, r_1, u_1, ... (registers 8i + 4g + e) and then of the candidates c_i (8 UPW + 4i + e).
// k_bigru_duo reads the UPW = 1 pack: one unit per wave, registers r | u | c.
static size_t bigru_fwd_pack(taco_model* m, const std::string& sc, int H, int UPW) {
  const int MB = DX_GROUP / UPW, NR = 12 * UPW;
  std::vector<float> p((size_t)2 * MB * NR * PK_NT, 0.f);
  for (int dir = 0; dir < 2; ++dir) {
    const GruW w = bigru_w(m, sc, dir);
    for (int mem = 0; mem < MB; ++mem)
      for (int i = 0; i < UPW; ++i) {
        auto r = [&](int wv) { return mem * 8 * UPW + wv * UPW + i; };
        auto u = [&](int wv) { return H + r(wv); };
        fill_cols(p, NR, dir * MB + mem, 8 * i, 4, w.gk.data(), 2 * H, H, r);
        fill_cols(p, NR, dir * MB + mem, 8 * i + 4, 4, w.gk.data(), 2 * H, H, u);
        fill_cols(p, NR, dir * MB + mem, 8 * UPW + 4 * i, 4, w.ck.data(), H, H, r);
      }
  }
  return arena_put(m, p);
}
// Backward scans (training): ROWS (fill_rows) of the recurrent kernels, a lane inputs 4 lane .. 4 lane + 3 of its wave's units.
// UPW = 1, k_bigru_duo_bwd: [2 dirs][32 members][12][512], wave w owns unit 8 mem + w: its row of Wc_h, then of Wg_h (r half, u half).
// UPW = GOB_UPW = 4, k_bigru_oct_bwd: [2 dirs][8 members][48][512], wave w owns units 32 mem + 4w + i: registers 4i + e = Wc_h row of unit i,
// 16 + 8i + e / 16 + 8i + 4 + e = Wg_h row of unit i, r half / u half.
static size_t bigru_bwd_pack(taco_model* m, const std::string& sc, int H, int UPW) {
  const int MB = DX_GROUP / UPW, NR = 12 * UPW;
  std::vector<float> p((size_t)2 * MB * NR * PK_NT, 0.f);
  for (int dir = 0; dir < 2; ++dir) {
    const GruW w = bigru_w(m, sc, dir);
    for (int mem = 0; mem < MB; ++mem)
      for (int i = 0; i < UPW; ++i) {
        auto row = [&](int wv) { return H + mem * 8 * UPW + wv * UPW + i; };
        fill_rows(p, NR, dir * MB + mem, 4 * i, 4, w.ck.data(), H, row, 0, H);
        fill_rows(p, NR, dir * MB + mem, 4 * UPW + 8 * i, 4, w.gk.data(), 2 * H, row, 0, 2 * H);
        fill_rows(p, NR, dir * MB + mem, 4 * UPW + 8 * i + 4, 4, w.gk.data(), 2 * H, row, H, 2 * H);
      }
  }
  return arena_put(m, p);
}
static_assert(GD_MEMBERS == DX_GROUP && DX_GROUP / GOB_UPW * GOB_UPM == GX_H, "the scan packs share the decoder's 32-member groups");

static void make_cbhg(taco_model* m, Cbhg& c, const std::string& sc, int in_dim, int K, int C, int maxpool,
                      int depth, int rnn, const int* projs, int nproj, int pw, bool bf3 = false) {
  cbhg_dims(c, in_dim, K, C, maxpool, depth, rnn, projs, nproj, pw);
  for (int k = K; k >= 1; --k) {
    const std::string n = sc + "/conv_bank/conv1d_" + std::to_string(k);
    c.bank.push_back(m->convs[n] = make_conv(m, n, true, true, bf3));
  }
  for (int i = 0; i < nproj; ++i) {
    const std::string n = sc + "/proj_" + std::to_string(i + 1);
    c.proj.push_back(m->convs[n] = make_conv(m, n, true, true, bf3));
  }
  c.has_dense = projs[nproj - 1] != rnn;
  if (c.has_dense) c.dense = m->convs[sc + "/dense"] = make_conv(m, sc + "/dense", false, true, bf3);
  for (int i = 0; i < depth; ++i) {
    const std::string n = sc + "/highway_" + std::to_string(i + 1);
    ConvL L = make_conv(m, n + "/H", false, true, bf3);
    const ConvL Tt = make_conv(m, n + "/T", false, true, bf3);
    L.wp2 = Tt.wp; L.bias2 = Tt.bias; L.bh2 = Tt.bh; L.bl2 = Tt.bl; L.bl3_2 = Tt.bl3;
    c.hw.push_back(m->convs[n] = L);
  }
  // BiGRU: hoisted input projection [rnn, 2*(2H+H)] = [fw gates(r|u) | fw cand | bw gates | bw cand]
  const int H = rnn, I = rnn;
  std::vector<float> Wx((size_t)I * 6 * H), bx(6 * H);
  for (int dir = 0; dir < 2; ++dir) {
    const GruW w = bigru_w(m, sc, dir);
    const auto &gk = w.gk, &ck = w.ck;
    for (int i = 0; i < I; ++i) {
      for (int j = 0; j < 2 * H; ++j) Wx[(size_t)i * 6 * H + dir * 3 * H + j] = gk[(size_t)i * 2 * H + j];
      for (int j = 0; j < H; ++j) Wx[(size_t)i * 6 * H + dir * 3 * H + 2 * H + j] = ck[(size_t)i * H + j];
    }
    for (int j = 0; j < 2 * H; ++j) bx[dir * 3 * H + j] = w.gb[j];
    for (int j = 0; j < H; ++j) bx[dir * 3 * H + 2 * H + j] = w.cb[j];
    c.gh[dir] = pack_w16(m, gk.data(), 2 * H, I, H, 0, 2 * H, nullptr);
    c.ch[dir] = pack_w16(m, ck.data(), H, I, H, 0, H, nullptr);
    c.raw_gh[dir] = arena_put(m, gk.data() + (size_t)I * 2 * H, (size_t)H * 2 * H);
    c.raw_ch[dir] = arena_put(m, ck.data() + (size_t)I * H, (size_t)H * H);
    std::vector<float> g2((size_t)H * H * 2);
    for (int k = 0; k < H; ++k)
      for (int j = 0; j < H; ++j) { g2[((size_t)k * H + j) * 2] = gk[(size_t)(I + k) * 2 * H + j]; g2[((size_t)k * H + j) * 2 + 1] = gk[(size_t)(I + k) * 2 * H + H + j]; }
    c.res_g2[dir] = arena_put(m, g2);
    if (H == 256) {
      std::vector<float> g2p(g2.size()), c1p((size_t)H * H);
      for (int k = 0; k < H; ++k)
        for (int jb = 0; jb < 64; ++jb)
          for (int u = 0; u < 4; ++u) {
            const int j = jb + 64 * u, cp = jb * 4 + u;
            g2p[((size_t)k * H + cp) * 2] = g2[((size_t)k * H + j) * 2]; g2p[((size_t)k * H + cp) * 2 + 1] = g2[((size_t)k * H + j) * 2 + 1];
            c1p[(size_t)k * H + cp] = ck[(size_t)(I + k) * H + j];
          }
      c.res_g2p[dir] = arena_put(m, g2p);
      c.res_c1p[dir] = arena_put(m, c1p);
    }
  }
  if (H == GX_H) {      // the whole-chip scans (gd_pack and go_pack[0] are the same bytes twice: the arena's order is kept as it was)
    c.gd_pack = bigru_fwd_pack(m, sc, H, 1);
    for (int lg = 0; lg < 3; ++lg) c.go_pack[lg] = bigru_fwd_pack(m, sc, H, 1 << lg);
    if (m->tp) { c.gb_pack = bigru_bwd_pack(m, sc, H, 1); c.gob_pack = bigru_bwd_pack(m, sc, H, GOB_UPW); }
  }
  ConvL X; X.kw = 1; X.cin = I; X.N = 6 * H;
  pack_gemm_weights(m, X, Wx.data(), bf3);
  X.bias = arena_put(m, bx);
  c.xproj = X;
  // fused front (taco_front.h): inference models only (the training forward needs the bank tensor for its batch statistics)
  c.front_kind = 0;
  if (bf3 && !m->tp && maxpool == 2 && pw == 3 && nproj >= 1 && C % FR_CH == 0 && K * (C / FR_CH) <= FR_MAXCH && K <= FR_MAXW) {
    const int cinp = rup(in_dim, 16), N1 = projs[0];
    // (N1 % 32: k_front_combine and the chain's fused entry read the partial sums, bias and BatchNorm operands as float4 at n = i % N1 and
    // consume them in 32-column tiles -- a custom first projection size such as 250 takes the two-launch path)
    if (cinp == 80 && K <= 8 && N1 <= 256 && N1 % 32 == 0) c.front_kind = 1;
    else if (cinp == 128 && K <= 16 && N1 <= 128 && N1 % 32 == 0) c.front_kind = 2;
    if (c.front_kind) {
      for (const ConvL& L : c.bank) {
        const auto& kt = TD(m, sc + "/conv_bank/conv1d_" + std::to_string(L.kw) + "/kernel");
        const int ns = rup(cdiv(L.kw * cinp, 32), 2), nct = C / 16;     // even: the kernel walks the steps in pairs (a padding step has zero weights)
        std::vector<unsigned short> hi((size_t)ns * nct * 512, 0), lo(hi.size(), 0);
        for (int st = 0; st < ns; ++st)
          for (int ct = 0; ct < nct; ++ct)
            for (int q = 0; q < 4; ++q)
              for (int i = 0; i < 16; ++i)
                for (int e = 0; e < 8; ++e) {
                  const int kk = 32 * st + 8 * q + e, tap = kk / cinp, cc = kk % cinp;
                  if (tap >= L.kw || cc >= in_dim) continue;
                  const float w = kt[((size_t)tap * in_dim + cc) * C + 16 * ct + i];
                  const size_t o = (((size_t)st * nct + ct) * 64 + q * 16 + i) * 8 + e;
                  lo[o] = bf16_rne_host(w - bf16_to_float(hi[o] = bf16_rne_host(w)));
                }
        c.fr_wh.push_back(arena_put_u16(m, hi)); c.fr_wl.push_back(arena_put_u16(m, lo)); c.fr_ns.push_back(ns);
      }
    }
  }
}

static int add_var(taco_model* m, ConvL& L, int coff) {
  GemmVar v;
  memset(&v, 0, sizeof v);
  // pointers are resolved after the arena upload (model_upload): store offsets for now
  v.wp = (const float*)L.wp; v.wp2 = (const float*)L.wp2; v.bias = (const float*)L.bias; v.bias2 = (const float*)L.bias2;
  v.bn_scale = (const float*)L.bns; v.bn_shift = (const float*)L.bnb;
  v.bh = (const unsigned short*)L.bh; v.bl = (const unsigned short*)L.bl; v.bh2 = (const unsigned short*)L.bh2; v.bl2 = (const unsigned short*)L.bl2;
  v.bl3 = (const unsigned short*)L.bl3; v.bl3_2 = (const unsigned short*)L.bl3_2;
  v.K16 = L.K16; v.cin_pad16 = L.cin_pad16;
  v.kw = L.kw; v.padl = (L.kw - 1) / 2; v.Kq = L.kw * L.cin_pad / 4; v.NT = cdiv(L.N, 32); v.N = L.N; v.coff = coff;
  L.var_index = (int)m->hvars.size();
  m->hvars.push_back(v);
  return L.var_index;
}

// ---- composite weights of the decoder loop: products formed in double and rounded once ----
// Prenet layer 1 of the NEXT step, fed with this step's outputs (helpers.py:31 feeds back the last of the r frames):
//   relu([frame, ctx] . W1 + b1), frame = o . Wf[:, rM-M:] + bf[rM-M:]   =>   relu([o, ctx] . [Wf_last . W1a ; W1b] + (b1 + bf_last . W1a))
// computed in the same launch as the frame projection: one dependent launch less per decoder step.  Rows [o (Hd) | ctx (D)], P0 columns.
static Composite compose_prenet1_next(const std::vector<float>& Wf, const std::vector<float>& bf, const std::vector<float>& W1, const std::vector<float>& b1,
                                      int Hd, int D, int Mm, int rM, int P0) {
  Composite c; c.W.assign((size_t)(Hd + D) * P0, 0.f); c.b.assign(P0, 0.f);
  for (int k = 0; k < Hd; ++k)
    for (int q = 0; q < P0; ++q) {
      double acc = 0;
      for (int j = 0; j < Mm; ++j) acc += (double)Wf[(size_t)k * rM + (rM - Mm) + j] * (double)W1[(size_t)j * P0 + q];
      c.W[(size_t)k * P0 + q] = (float)acc;
    }
  for (int k = 0; k < D; ++k)
    for (int q = 0; q < P0; ++q) c.W[(size_t)(Hd + k) * P0 + q] = W1[(size_t)(Mm + k) * P0 + q];
  for (int q = 0; q < P0; ++q) {
    double acc = b1[q];
    for (int j = 0; j < Mm; ++j) acc += (double)bf[(rM - Mm) + j] * (double)W1[(size_t)j * P0 + q];
    c.b[q] = (float)acc;
  }
  return c;
}
// ... on a training shadow model, in TEACHER form: the next step's prenet layer 1 reads the teacher's frame, so the same rows hold the raw
// kernel (frame rows k < num_mels, zero up to Hd; then the context rows) and the raw bias -- index-valued like every shadow "weight"
static Composite compose_prenet1_teacher(const std::vector<float>& W1, const std::vector<float>& b1, int Hd, int D, int Mm, int P0) {
  Composite c; c.W.assign((size_t)(Hd + D) * P0, 0.f); c.b = b1;
  for (int k = 0; k < Mm; ++k) for (int q = 0; q < P0; ++q) c.W[(size_t)k * P0 + q] = W1[(size_t)k * P0 + q];
  for (int k = 0; k < D; ++k) for (int q = 0; q < P0; ++q) c.W[(size_t)(Hd + k) * P0 + q] = W1[(size_t)(Mm + k) * P0 + q];
  return c;
}
// Decoder GRU 1 with the concat projection folded in.  o0 = z . Wc + bc is linear in z = [h_att | ctx (| spk)] (Z rows), so
//   gates:      [o0, h] . Wg + bg = z . (Wc . Wg_x) + h . Wg_h + (bg + bc . Wg_x)
//   candidate x: o0 . Wk_x       = z . (Wc . Wk_x) + bc . Wk_x
// and o0 itself (the ResidualWrapper input, tacotron.py:172) comes out of the same launch as Hd extra columns: one dependent launch less
// per decoder step.  [Z + Hd rows (z | h)] x [r | u | candidate-x | o0] (4 Hd columns); the h rows hold Wg_h under r | u only.
static Composite compose_gru1_fold(const std::vector<float>& Wc, const std::vector<float>& bcv, const GruW& g, int Z, int Hd) {
  const int N4 = 4 * Hd;
  Composite c; c.W.assign((size_t)(Z + Hd) * N4, 0.f); c.b.assign(N4, 0.f);
  std::vector<double> row(3 * Hd);
  for (int z = 0; z <= Z; ++z) {      // row Z of this loop = the bias row (z . Wc replaced by bc)
    std::fill(row.begin(), row.end(), 0.0);
    for (int k = 0; k < Hd; ++k) {
      const double w = (z < Z) ? (double)Wc[(size_t)z * Hd + k] : (double)bcv[k];
      for (int j = 0; j < 2 * Hd; ++j) row[j] += w * (double)g.gk[(size_t)k * 2 * Hd + j];
      for (int j = 0; j < Hd; ++j) row[2 * Hd + j] += w * (double)g.ck[(size_t)k * Hd + j];
    }
    if (z < Z) {
      for (int j = 0; j < 3 * Hd; ++j) c.W[(size_t)z * N4 + j] = (float)row[j];
      for (int j = 0; j < Hd; ++j) c.W[(size_t)z * N4 + 3 * Hd + j] = Wc[(size_t)z * Hd + j];
    } else {
      for (int j = 0; j < 2 * Hd; ++j) c.b[j] = (float)(row[j] + (double)g.gb[j]);
      for (int j = 0; j < Hd; ++j) { c.b[2 * Hd + j] = (float)row[2 * Hd + j]; c.b[3 * Hd + j] = bcv[j]; }
    }
  }
  for (int k = 0; k < Hd; ++k)
    for (int j = 0; j < 2 * Hd; ++j) c.W[(size_t)(Z + k) * N4 + j] = g.gk[(size_t)(Hd + k) * 2 * Hd + j];
  return c;
}
// ... on a training shadow model the products are computed on the device after every optimizer step (k_dx_fold) into a buffer of
// (Z + 1) * 3 Hd floats that the index map addresses behind the NP parameters: element (z, j) of [products | bias row] is index NP + 1 + i.
// The copied parts (o0 columns, Wg_h rows) stay parameter indices.
static Composite compose_gru1_fold_index(const std::vector<float>& Wc, const std::vector<float>& bcv, const GruW& g, int Z, int Hd, size_t NP) {
  const int N4 = 4 * Hd;
  Composite c; c.W.assign((size_t)(Z + Hd) * N4, 0.f); c.b.assign(N4, 0.f);
  for (int z = 0; z <= Z; ++z)
    for (int j = 0; j < 3 * Hd; ++j) {
      const float idx = (float)(NP + 1 + (size_t)z * 3 * Hd + j);
      if (z < Z) c.W[(size_t)z * N4 + j] = idx; else c.b[j] = idx;
    }
  for (int z = 0; z < Z; ++z) for (int j = 0; j < Hd; ++j) c.W[(size_t)z * N4 + 3 * Hd + j] = Wc[(size_t)z * Hd + j];
  for (int j = 0; j < Hd; ++j) c.b[3 * Hd + j] = bcv[j];
  for (int k = 0; k < Hd; ++k) for (int j = 0; j < 2 * Hd; ++j) c.W[(size_t)(Z + k) * N4 + j] = g.gk[(size_t)(Hd + k) * 2 * Hd + j];
  return c;
}

// ---- the model build ----
static int build_train_packs(taco_model* m);   // taco_train.h
static int pack_model(taco_model* m) {
  const taco_hparams& hp = m->hp;
  m->harena.clear(); m->hvars.clear();
  m->emb = arena_put(m, TD(m, "embedding"));
  for (int i = 0; i < hp.enc_prenet_n; ++i) m->enc_prenet.push_back(make_conv(m, "prenet/dense_" + std::to_string(i + 1), false, true, true));
  make_cbhg(m, m->enc, "encoder_cbhg", hp.enc_prenet[hp.enc_prenet_n - 1], hp.enc_bank_size, hp.enc_bank_channels,
            hp.enc_maxpool, hp.enc_highway_depth, hp.enc_rnn_size, hp.enc_proj, hp.enc_proj_n, hp.enc_proj_width, true);
  // fp32-grade: the keys feed the alignment argmax, the one output held to "bit-identical".  Rounds 1-3: the exact-fp32 MFMA (k_gemm, +35 us per
  // C2 forward over the three-product split); round 4: the SIX-product split (operands split three ways, 2^-24 per product) on the bf16 pipe
  m->memory_layer = make_conv(m, "attention/memory_layer", false, false, true, true);
  make_cbhg(m, m->post, "post_cbhg", hp.num_mels, hp.post_bank_size, hp.post_bank_channels, hp.post_maxpool,
            hp.post_highway_depth, hp.post_rnn_size, hp.post_proj, hp.post_proj_n, hp.post_proj_width, true);
  const int S = simple_S(m);
  if (is_simple(m)) {
    // linear head input = concat(speaker_embed, post_outputs) (tacotron.py:226-235): rows [0,S) of the kernel
    // multiply the per-utterance embedding -> a per-batch-row vector; rows [S,..) stay a GEMM over the frames
    const int F = hp.num_freq;
    const HostTensor k = T_(m, "linear/kernel");
    m->lin_spk = pack_w16(m, k.data.data(), F, 0, S, 0, F, nullptr);
    auto rows = [&](int64_t r0, int64_t r1) { HostTensor t; t.shape = {r1 - r0, (int64_t)F}; t.data.assign(k.data.begin() + r0 * F, k.data.begin() + r1 * F); t.set = true; return t; };
    m->raw["linear/kernel_spk"] = rows(0, S);     // (explicit inserts) kept for the training packs: transposed speaker rows
    m->raw["linear/kernel"] = rows(S, k.shape[0]);
    m->spk_emb = arena_put(m, TD(m, "speaker_embedding"));
  }
  m->linear = make_conv(m, "linear", false, true, true);
  // decoder (skinny packs)
  const int D = 2 * hp.enc_rnn_size, As = hp.attention_state_size, Hd = hp.dec_rnn_size, A = hp.attention_size;
  const int Mm = hp.num_mels, rM = Mm * hp.reduction_factor, P0 = hp.dec_prenet[0], Z = As + D + S;
  int d = Mm + D;
  for (int i = 0; i < hp.dec_prenet_n; ++i) {
    const std::string n = "decoder/prenet/dense_" + std::to_string(i + 1);
    m->dec_prenet.push_back(m->skinny[n] = pack_w16_named(m, n, d, hp.dec_prenet[i]));
    d = hp.dec_prenet[i];
  }
  m->grus["decoder/attention_gru"] = m->att_gru = make_grudec(m, "decoder/attention_gru", d + S, As);   // simple: input = concat(prenet_out, speaker_embed)
  m->skinny["attention/query_layer"] = m->query = pack_w16_named(m, "attention/query_layer", As, A, false);
  m->raw_wq = arena_put(m, TD(m, "attention/query_layer/kernel").data(), (size_t)As * A);
  m->skinny["decoder/concat_projection"] = m->concat_proj = pack_w16_named(m, "decoder/concat_projection", Z, Hd);
  for (int i = 0; i < hp.dec_layer_num; ++i) {
    const std::string n = "decoder/gru_" + std::to_string(i + 1);
    m->dec_gru.push_back(m->grus[n] = make_grudec(m, n, Hd, Hd));
  }
  m->skinny["decoder/frame_projection"] = m->frame_proj = pack_w16_named(m, "decoder/frame_projection", Hd, rM);
  const auto& W1 = TD(m, "decoder/prenet/dense_1/kernel"); const auto& b1 = TD(m, "decoder/prenet/dense_1/bias");
  const auto& Wcc = TD(m, "decoder/concat_projection/kernel"); const auto& bcc = TD(m, "decoder/concat_projection/bias");
  const Composite p1 = compose_prenet1_next(TD(m, "decoder/frame_projection/kernel"), TD(m, "decoder/frame_projection/bias"), W1, b1, Hd, D, Mm, rM, P0);
  m->prenet1_next = pack_w16(m, p1.W.data(), P0, 0, Hd + D, 0, P0, p1.b.data());
  if (!m->tp) {      // (the fold is not built for the training shadow model)
    const GruW g1 = gru_w(m, "decoder/gru_1");
    const Composite f = compose_gru1_fold(Wcc, bcc, g1, Z, Hd);
    m->gru1_fold.I = Z; m->gru1_fold.H = Hd;
    m->gru1_fold.gx = pack_w16(m, f.W.data(), 4 * Hd, 0, Z + Hd, 0, 4 * Hd, f.b.data());
    m->gru1_fold.ch = pack_w16(m, g1.ck.data(), Hd, Hd, Hd, 0, Hd, g1.cb.data());
    m->fuse_concat = 1;
    if (hp.dec_layer_num == 2) dx_build_pack(m, p1, f);
  } else if (hp.dec_layer_num == 2 && dx_widths_ok(m)) {
    // Training shadow model: every "weight" here is 1 + the flat index of a parameter, and the arena doubles as the index map of
    // taco_train_refresh.  The persistent decoder's pack is built from the teacher / index forms of the two composites.
    size_t NP = 0;
    for (auto& sp : m->spec) { size_t c = 1; for (int64_t dd : sp.second) c *= (size_t)dd; NP += c; }
    m->dx_fold_n = (size_t)(Z + 1) * 3 * Hd;
    if (NP + m->dx_fold_n >= (1u << 24)) return fail(TACO_ERR_UNSUPPORTED, "parameter + fold indices exceed 2^24");
    dx_build_pack(m, compose_prenet1_teacher(W1, b1, Hd, D, Mm, P0), compose_gru1_fold_index(Wcc, bcc, gru_w(m, "decoder/gru_1"), Z, Hd, NP));
    dbx_build_pack(m);
  }
  std::vector<float> v = TD(m, "attention/attention_v");      // attention vectors; bah_norm: v_hat = g * v / |v| (A.9)
  if (hp.attention_type == 1) {
    double nrm = 0; for (float x : v) nrm += (double)x * x;
    const double sc = (double)TD(m, "attention/attention_g")[0] / std::sqrt(nrm);
    for (float& x : v) x = (float)(x * sc);
    m->att_b = arena_put(m, TD(m, "attention/attention_b").data(), A);
  }
  m->att_v = arena_put(m, v.data(), A);
  if (hp.attention_type == 2) m->att_sb = arena_put(m, TD(m, "attention/attention_score_bias").data(), 1);
  if (is_deepvoice(m)) {      // speaker tables (speaker_embedding_size 1) or dense layers on the embedding
    if (hp.speaker_embedding_size != 1) m->spk_emb = arena_put(m, TD(m, "speaker_embedding"));
    for (auto& n : spk_vector_names(hp)) {
      if (hp.speaker_embedding_size == 1) { m->spk_table.push_back(arena_put(m, TD(m, "spk/" + n + "/table"))); continue; }
      const HostTensor& k = T_(m, "spk/" + n + "/kernel");
      m->spk_dense.push_back(pack_w16_named(m, "spk/" + n, (int)k.shape[0], (int)k.shape[1]));
    }
  }
  // GemmVar table (bank variants must be contiguous)
  for (int i = 0; i < hp.enc_prenet_n; ++i) add_var(m, m->enc_prenet[i], 0);
  for (Cbhg* c : {&m->enc, &m->post}) {
    for (size_t i = 0; i < c->bank.size(); ++i) add_var(m, c->bank[i], (c->bank[i].kw - 1) * c->C);
    for (auto& L : c->proj) add_var(m, L, 0);
    if (c->has_dense) add_var(m, c->dense, 0);
    for (auto& L : c->hw) add_var(m, L, 0);
    add_var(m, c->xproj, 0);
  }
  add_var(m, m->memory_layer, 0);
  add_var(m, m->linear, 0);
  // stand-alone copies for the op-level entry points (coff 0)
  for (auto& kv : m->convs) add_var(m, kv.second, 0);
  for (int i = 0; i < hp.enc_prenet_n; ++i) m->convs["prenet/dense_" + std::to_string(i + 1)] = m->enc_prenet[i];
  m->convs["attention/memory_layer"] = m->memory_layer;
  m->convs["linear"] = m->linear;
  return m->tp ? build_train_packs(m) : 0;
}
// Everything of taco_model_finalize that needs no device: the arena (m->harena), the GemmVar table with arena offsets (+1; 0 = absent) in
// its pointer fields, and on a shadow model (m->tp) the split-bf16 index lists and the backward packs.
static int model_pack_host(taco_model* m) {
  try {
    return pack_model(m);
  } catch (const PackMissing& e) {
    return fail(TACO_ERR_STATE, "model build: weight '%s' is unknown or was never set", e.name.c_str());
  }
}
