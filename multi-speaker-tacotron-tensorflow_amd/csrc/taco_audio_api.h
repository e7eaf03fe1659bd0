// taco_audio_api.h -- C ABI of the spectrogram -> waveform step and of the waveform -> training targets step; included inside extern "C".
// Shared by the entry points: gl_iterate (the Griffin-Lim loop of both flavours), gl_carved_bytes, wav_frame_energies (trim and split).

// The handle of either flavour.  GL_LIBROSA centres the window in n_fft (lpad = (n_fft - win) / 2: librosa pads the window, and the frame with
// it); GL_TF leaves it at the start (lpad = 0: tf.contrib.signal.stft multiplies the win samples by the window and zero-pads at the END
// to n_fft, and inverse_stft keeps irfft(X, n_fft)[:win]).  Both are the same two packs: X_k = sum_n f[n] w[n] e^{-2 pi i k (n + lpad) / N}
// and its transpose with the irfft weights, win columns, in double with the angle reduced exactly.  upload = false (taco_debug_gl_create_host)
// stops before the device is touched: such a handle serves the argument and state checks only.
static int gl_create(const taco_audio_hparams* hp, int device, int flavor, bool upload, taco_gl** out) {
  if (!hp || !out) return fail(TACO_ERR_ARG, "null argument");
  taco_gl* g = new taco_gl();
  g->hp = *hp;
  g->flavor = flavor;
  g->F = hp->num_freq; g->n_fft = (hp->num_freq - 1) * 2;                       // audio/__init__.py:118-122
  g->hop = (int)(hp->frame_shift_ms / 1000.0 * hp->sample_rate);
  g->win = (int)(hp->frame_length_ms / 1000.0 * hp->sample_rate);
  if (g->F < 2 || g->hop < 1 || g->win < 2 || g->win > g->n_fft) { delete g; return fail(TACO_ERR_ARG, "bad STFT parameters"); }
  g->lpad = flavor == GL_TF ? 0 : (g->n_fft - g->win) / 2;
  const int N = g->n_fft, F = g->F, W = g->win;
  const double PI2 = 6.283185307179586476925286766559;
  std::vector<double> w(W);
  for (int n = 0; n < W; ++n) w[n] = 0.5 - 0.5 * std::cos(PI2 * n / W);          // periodic Hann (fftbins=True)
  std::vector<float> fw((size_t)W * 2 * F), iv((size_t)2 * F * W), w2(N, 0.f);
  for (int n = 0; n < W; ++n) {
    w2[g->lpad + n] = (float)(w[n] * w[n]);
    for (int k = 0; k < F; ++k) {
      const long q = ((long)k * (n + g->lpad)) % N;                               // exact angle reduction
      const double c = std::cos(PI2 * q / N), s = std::sin(PI2 * q / N);
      fw[(size_t)n * 2 * F + k] = (float)(w[n] * c);                              // Re X_k =  sum f w cos
      fw[(size_t)n * 2 * F + F + k] = (float)(-w[n] * s);                         // Im X_k = -sum f w sin
      const double ck = (k == 0 || k == N / 2) ? 1.0 : 2.0;                       // irfft: Hermitian half counted twice
      iv[(size_t)k * W + n] = (float)(ck / N * c * w[n]);
      iv[(size_t)(F + k) * W + n] = (float)((k == 0 || k == N / 2) ? 0.0 : -ck / N * s * w[n]);
    }
  }
  taco_model* gm = new taco_model();
  gm->device = device; gm->bf3 = 1;
  g->gm = gm;
  g->fwd.kw = 1; g->fwd.cin = W; g->fwd.N = 2 * F;
  g->fwd.wp = pack_w32(gm, fw.data(), 1, W, 2 * F, &g->fwd.cin_pad);
  pack_bf3(gm, fw.data(), 1, W, 2 * F, &g->fwd.bh, &g->fwd.bl, &g->fwd.K16, &g->fwd.cin_pad16);
  g->inv.kw = 1; g->inv.cin = 2 * F; g->inv.N = W;
  g->inv.wp = pack_w32(gm, iv.data(), 1, 2 * F, W, &g->inv.cin_pad);
  pack_bf3(gm, iv.data(), 1, 2 * F, W, &g->inv.bh, &g->inv.bl, &g->inv.K16, &g->inv.cin_pad16);
  g->w2 = arena_put(gm, w2.data(), w2.size());
  add_var(gm, g->fwd, 0); add_var(gm, g->inv, 0);
  if (!upload) { *out = g; return 0; }
  if (hipSetDevice(device) != hipSuccess || hipMalloc((void**)&gm->darena, gm->harena.size() * sizeof(float)) != hipSuccess ||
      hipMemcpy(gm->darena, gm->harena.data(), gm->harena.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    delete gm; delete g; return fail(TACO_ERR_HIP, "could not upload the DFT packs");
  }
  for (auto& v : gm->hvars) {
    v.wp = AP(gm, (size_t)v.wp); v.wp2 = nullptr; v.bias = nullptr; v.bias2 = nullptr; v.bn_scale = nullptr; v.bn_shift = nullptr;
    v.bh = (const unsigned short*)AP(gm, (size_t)v.bh); v.bl = (const unsigned short*)AP(gm, (size_t)v.bl); v.bh2 = nullptr; v.bl2 = nullptr;
  }
  gm->harena.clear(); gm->harena.shrink_to_fit();
  if (const int rc = gemm_set_attributes()) { (void)hipFree(gm->darena); delete gm; delete g; return rc; }      // (this model does not pass through taco_model_finalize)
  gm->finalized = true;
  *out = g;
  return 0;
}

int taco_gl_create(const taco_audio_hparams* hp, int device, taco_gl** out) { return gl_create(hp, device, GL_LIBROSA, true, out); }
int taco_gl_create_tf(const taco_audio_hparams* hp, int device, taco_gl** out) { return gl_create(hp, device, GL_TF, true, out); }
int taco_debug_gl_create_host(const taco_audio_hparams* hp, int tf_flavor, taco_gl** out) {
  return gl_create(hp, -1, tf_flavor ? GL_TF : GL_LIBROSA, false, out);
}

void taco_gl_destroy(taco_gl* g) {
  if (!g) return;
  if (g->gm) { if (g->gm->darena) (void)hipFree(g->gm->darena); delete g->gm; }
  if (g->mel_band) (void)hipFree(g->mel_band);
  if (g->mel_w) (void)hipFree(g->mel_w);
  if (g->inv_mel) (void)hipFree(g->inv_mel);
  delete g;
}

int taco_gl_num_samples(const taco_gl* g, int T) { return (g && T > 0) ? g->hop * (T - 1) : 0; }

int taco_gl_min_frames(const taco_gl* g) { return g ? g->n_fft / 2 / g->hop + 2 : 0; }    // smallest T with hop*(T-1) > n_fft/2

// The Griffin-Lim workspace of either flavour (carve_gl); the exported sizes differ in the fewest frames they serve
static size_t gl_carved_bytes(const taco_gl* g, int B, int T) { Carver cv(nullptr, 0); GlWs w; carve_gl(cv, g, B, T, w); return cv.off; }
size_t taco_gl_workspace_bytes(const taco_gl* g, int B, int T) { return (!g || B <= 0 || T <= 1) ? 0 : gl_carved_bytes(g, B, T); }
size_t taco_gl_rows_workspace_bytes(const taco_gl* g, int B, int T) { return taco_gl_workspace_bytes(g, B, T); }   // same slot layout

// Fast Griffin-Lim: host state of the handle, read by gl_iterate and by carve_gl (the three workspace sizes above and below)
int taco_gl_set_momentum(taco_gl* g, float momentum) {
  if (!g) return fail(TACO_ERR_ARG, "null argument");
  if (!(momentum >= 0.f && momentum <= 1.f)) return fail(TACO_ERR_ARG, "momentum = %g: must be finite and in [0, 1]", (double)momentum);
  g->momentum = momentum;
  return 0;
}
float taco_gl_momentum(const taco_gl* g) { return g ? g->momentum : 0.f; }

// The Griffin-Lim iteration of either flavour, on a workspace whose S and X the flavour's prologue has filled: y = istft(X), then
// `iters` times est = stft(y), X = project(est, S), y = istft(X).  The two matrix products are the same for both; overlap_add()
// launches the flavour's overlap-add of the frames w.Y into w.ypad, `project` is its projection kernel.
// With the handle's momentum a != 0 (taco_gl_set_momentum) the projection is of z = est - c * prev, c = a / (1 + a), prev the
// estimate of the iteration before: the forward product writes into w.est and w.est2 in turn and k_gl_project_fast reads "this
// one" and "the other one".  The first iteration has no previous estimate and takes `project` as it stands.  At a = 0 the
// launches are the plain loop's, on w.est alone.
static void gl_launch_project_fast(hipStream_t st, bool tf, const float* est, const float* prev, const float* S, float* X, float c, size_t R, int F) {
  const bool pair = F % 2 == 0 && !((reinterpret_cast<uintptr_t>(est) | reinterpret_cast<uintptr_t>(prev) | reinterpret_cast<uintptr_t>(S) |
                                     reinterpret_cast<uintptr_t>(X)) & 7);
  if (pair) {
    if (tf) hipLaunchKernelGGL((k_gl_project_fast<true, 2>), EWGRID(R * F / 2), 0, st, est, prev, S, X, c, R, F);
    else hipLaunchKernelGGL((k_gl_project_fast<false, 2>), EWGRID(R * F / 2), 0, st, est, prev, S, X, c, R, F);
  } else {
    if (tf) hipLaunchKernelGGL((k_gl_project_fast<true, 1>), EWGRID(R * F), 0, st, est, prev, S, X, c, R, F);
    else hipLaunchKernelGGL((k_gl_project_fast<false, 1>), EWGRID(R * F), 0, st, est, prev, S, X, c, R, F);
  }
}
static int gl_iterate(taco_gl* g, hipStream_t st, const GlWs& w, size_t R, int iters, void (*project)(const float*, const float*, float*, size_t, int),
                      const std::function<void()>& overlap_add) {
  const int F = g->F;
  const float mc = g->momentum / (1.0f + g->momentum);
  float *cur = w.est, *other = w.est2;
  auto synth = [&]() -> int {     // frames = X . IDFT_w (win columns), then the flavour's overlap-add
    GemmCall c; c.x = w.X; c.ldx = 2 * F; c.M = (int)R; c.out = w.Y; c.ldo = g->win;
    TRY(run_gemm(g->gm, st, &g->inv, 1, false, c));
    overlap_add();
    HIPCHK(hipGetLastError());
    return 0;
  };
  TRY(synth());
  for (int it = 0; it < iters; ++it) {
    // est = stft(y): row (b, t) of the frame matrix is the hop-strided window ypad[b*slot + t*hop + lpad ...][0 .. win) (lpad = 0 on a TF
    // handle: pad_end=False, the utterance's hop*(f-1) + win samples hold exactly f frames); rows past an utterance's own frames read
    // whatever its slot holds there and are multiplied by S = 0 in the projection
    GemmCall c; c.x = w.ypad + g->lpad; c.ldx = g->hop; c.M = (int)R; c.out = cur; c.ldo = 2 * F;
    TRY(run_gemm(g->gm, st, &g->fwd, 1, false, c));
    if (other && it > 0) gl_launch_project_fast(st, g->flavor == GL_TF, cur, other, w.S, w.X, mc, R, F);
    else hipLaunchKernelGGL(project, EWGRID(R * F), 0, st, cur, w.S, w.X, R, F);
    HIPCHK(hipGetLastError());
    if (other) std::swap(cur, other);
    TRY(synth());
  }
  return 0;
}

// The librosa-flavour vocoder behind taco_gl_inv_spectrogram_rows (d_mel NULL: magnitudes from d_spec by k_gl_magnitude) and
// taco_gl_inv_melspectrogram_rows (d_mel: by k_gl_mel_magnitude); everything after the magnitudes is shared.
// d_frames NULL: every utterance keeps T frames (taco_gl_inv_spectrogram); else the kernels read each utterance's count from it,
// clamped to [taco_gl_min_frames, T]
static int gl_vocode_rows(taco_gl* g, void* hip_stream, const float* d_spec, const float* d_mel, const int32_t* d_frames,
                          const float* d_init_uniform, unsigned long long seed, int B, int T, int iters, float* d_wav, int32_t* d_num_samples,
                          void* d_workspace, size_t workspace_bytes) {
  if (!g || !(d_spec || d_mel) || !d_wav || !d_workspace || B <= 0 || T <= 1) return fail(TACO_ERR_ARG, "bad argument");
  if (g->flavor != GL_LIBROSA) return fail(TACO_ERR_STATE, "a handle of taco_gl_create_tf serves taco_gl_inv_spectrogram_tf only");
  if (d_mel && !g->inv_mels) return fail(TACO_ERR_STATE, "the mel vocoder needs the inverse basis: call taco_gl_set_inv_mel_basis first");
  const int L = g->hop * (T - 1), half = g->n_fft / 2, fmin = taco_gl_min_frames(g);
  if (L <= half) return fail(TACO_ERR_SHAPE, "utterance too short for reflect padding: hop*(T-1) = %d <= n_fft/2 = %d", L, half);
  HIPCHK(hipSetDevice(g->gm->device));
  hipStream_t st = (hipStream_t)hip_stream;
  Carver cv(d_workspace, workspace_bytes);
  GlWs w; carve_gl(cv, g, B, T, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes, have %zu", cv.off, workspace_bytes);
  const int Tr = gl_rows(g, T), F = g->F;
  const size_t R = (size_t)B * Tr, slot = gl_slot(g, T);
  if (iters < 0) iters = g->hp.griffin_lim_iters;
  HIPCHK(zero_async(w.ypad, ((size_t)B * slot + 2 * g->n_fft + g->win) * sizeof(float), st));
  hipLaunchKernelGGL(k_gl_wss, EWGRID((size_t)L + g->n_fft), 0, st, AP(g->gm, g->w2), w.wss, T, g->n_fft, g->hop);
  if (d_mel)
    hipLaunchKernelGGL(k_gl_mel_magnitude, dim3(cdiv(Tr, MELMAG_ROWS), B), dim3(256), mel_lds_bytes(g->inv_mels), st, d_mel, g->inv_mel, w.S, d_frames, fmin, T,
                       Tr, F, g->inv_mels, g->hp.min_level_db, g->hp.power, 1);
  else
    hipLaunchKernelGGL(k_gl_magnitude, EWGRID(R * F), 0, st, d_spec, w.S, d_frames, fmin, B, T, Tr, F, g->hp.min_level_db, g->hp.ref_level_db,
                       g->hp.power);
  hipLaunchKernelGGL(k_gl_init_phase, EWGRID(R * F), 0, st, w.S, d_init_uniform, seed, w.X, d_frames, fmin, B, T, Tr, F);
  HIPCHK(hipGetLastError());
  // y = istft(X): overlap-add / window sum-square with the reflect pad for the next stft
  TRY(gl_iterate(g, st, w, R, iters, k_gl_project, [&] {
    hipLaunchKernelGGL(k_gl_overlap_add, dim3((L + 255) / 256, B), dim3(256), 0, st, w.Y, w.wss, AP(g->gm, g->w2), w.ypad, d_frames, fmin, T, Tr,
                       g->win, g->hop, g->lpad, g->n_fft, slot);
  }));
  hipLaunchKernelGGL(k_inv_preemphasis, dim3(B), dim3(1024), 0, st, w.ypad, d_wav, d_frames, fmin, T, g->hop, d_num_samples, L, half, slot,
                     g->hp.preemphasis);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_gl_inv_spectrogram_rows(taco_gl* g, void* hip_stream, const float* d_spec, const int32_t* d_frames, const float* d_init_uniform,
                                 unsigned long long seed, int B, int T, int iters, float* d_wav, int32_t* d_num_samples, void* d_workspace,
                                 size_t workspace_bytes) {
  if (!d_spec) return fail(TACO_ERR_ARG, "bad argument");
  return gl_vocode_rows(g, hip_stream, d_spec, nullptr, d_frames, d_init_uniform, seed, B, T, iters, d_wav, d_num_samples, d_workspace,
                        workspace_bytes);
}

int taco_gl_inv_spectrogram(taco_gl* g, void* hip_stream, const float* d_spec, const float* d_init_uniform, unsigned long long seed,
                            int B, int T, int iters, float* d_wav, void* d_workspace, size_t workspace_bytes) {
  return taco_gl_inv_spectrogram_rows(g, hip_stream, d_spec, nullptr, d_init_uniform, seed, B, T, iters, d_wav, nullptr, d_workspace,
                                      workspace_bytes);
}

// ---- inv_melspectrogram (audio/__init__.py:70-72,136-140) ----
int taco_gl_set_inv_mel_basis(taco_gl* g, const float* host_inv, int num_mels) {
  if (!g || !host_inv || num_mels <= 0) return fail(TACO_ERR_ARG, "bad argument");
  if (mel_lds_bytes(num_mels) > 64 * 1024)
    return fail(TACO_ERR_UNSUPPORTED, "num_mels = %d: k_gl_mel_magnitude keeps %d rows of amplitudes in 64 KB of LDS", num_mels, MELMAG_ROWS);
  const int F = g->F;
  std::vector<float> t((size_t)num_mels * F);          // [num_freq, num_mels] as np.linalg.pinv returns it -> mel-major
  for (int f = 0; f < F; ++f)
    for (int m = 0; m < num_mels; ++m) t[(size_t)m * F + f] = host_inv[(size_t)f * num_mels + m];
  HIPCHK(hipSetDevice(g->gm->device));
  float* d = nullptr;
  if (hipMalloc((void**)&d, t.size() * sizeof(float)) != hipSuccess ||
      hipMemcpy(d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    if (d) (void)hipFree(d);
    return fail(TACO_ERR_HIP, "could not upload the inverse mel basis");
  }
  if (g->inv_mel) (void)hipFree(g->inv_mel);           // (hipFree waits for the launches that still read the basis it replaces)
  g->inv_mel = d; g->inv_mels = num_mels;
  return 0;
}

int taco_gl_mel_to_linear(taco_gl* g, void* hip_stream, const float* d_mel, int B, int T, float* d_out) {
  if (!g || !d_mel || !d_out || B <= 0 || B > 65535 || T <= 0) return fail(TACO_ERR_ARG, "bad argument");
  if (!g->inv_mels) return fail(TACO_ERR_STATE, "mel to linear needs the inverse basis: call taco_gl_set_inv_mel_basis first");
  HIPCHK(hipSetDevice(g->gm->device));
  hipLaunchKernelGGL(k_gl_mel_magnitude, dim3(cdiv(T, MELMAG_ROWS), B), dim3(256), mel_lds_bytes(g->inv_mels), (hipStream_t)hip_stream, d_mel,
                     g->inv_mel, d_out, nullptr, 0, T, T, g->F, g->inv_mels, g->hp.min_level_db, 1.0f, 0);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_gl_inv_melspectrogram_rows(taco_gl* g, void* hip_stream, const float* d_mel, const int32_t* d_frames, const float* d_init_uniform,
                                    unsigned long long seed, int B, int T, int iters, float* d_wav, int32_t* d_num_samples, void* d_workspace,
                                    size_t workspace_bytes) {
  if (!d_mel) return fail(TACO_ERR_ARG, "bad argument");
  return gl_vocode_rows(g, hip_stream, nullptr, d_mel, d_frames, d_init_uniform, seed, B, T, iters, d_wav, d_num_samples, d_workspace,
                        workspace_bytes);
}

// ---- inv_spectrogram_tensorflow (audio/__init__.py:59-61,87-96,109-116,152-153,167-168; synthesizer.py:53-54) ----
int taco_gl_tf_num_samples(const taco_gl* g, int T) { return (g && T > 0) ? g->hop * (T - 1) + g->win : 0; }

// (the slot layout of the librosa flavour, without its wss table in use)
size_t taco_gl_tf_workspace_bytes(const taco_gl* g, int B, int T) { return (!g || B <= 0 || T <= 0) ? 0 : gl_carved_bytes(g, B, T); }

int taco_gl_inv_spectrogram_tf(taco_gl* g, void* hip_stream, const float* d_spec, const int32_t* d_frames, int B, int T, int iters, float* d_wav,
                               int32_t* d_num_samples, void* d_workspace, size_t workspace_bytes) {
  if (!g || !d_spec || !d_wav || !d_workspace || B <= 0 || B > 65535 || T <= 0) return fail(TACO_ERR_ARG, "bad argument");
  if (g->flavor != GL_TF) return fail(TACO_ERR_STATE, "taco_gl_inv_spectrogram_tf needs a handle of taco_gl_create_tf");
  HIPCHK(hipSetDevice(g->gm->device));
  hipStream_t st = (hipStream_t)hip_stream;
  Carver cv(d_workspace, workspace_bytes);
  GlWs w; carve_gl(cv, g, B, T, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes, have %zu", cv.off, workspace_bytes);
  const int Tr = gl_rows(g, T), F = g->F, L = taco_gl_tf_num_samples(g, T);
  const size_t R = (size_t)B * Tr, slot = gl_slot(g, T);
  if (iters < 0) iters = g->hp.griffin_lim_iters;
  // every slot starts as zeros: an utterance's overlap-add writes its own samples only, and what a tail row of the frame matrix reads
  // behind them must be finite (it is multiplied by S = 0).  est is filled with zeros to serve as the "uniform" of zero phase:
  // k_gl_init_phase then writes X = [S cos 0 | S sin 0] = [S | 0] exactly (audio/__init__.py:90-91, S cast to complex64)
  HIPCHK(zero_async(w.ypad, ((size_t)B * slot + 2 * g->n_fft + g->win) * sizeof(float), st));
  HIPCHK(zero_async(w.est, R * 2 * F * sizeof(float), st));
  hipLaunchKernelGGL(k_gl_magnitude, EWGRID(R * F), 0, st, d_spec, w.S, d_frames, 1, B, T, Tr, F, g->hp.min_level_db, g->hp.ref_level_db,
                     g->hp.power);
  hipLaunchKernelGGL(k_gl_init_phase, EWGRID(R * F), 0, st, w.S, w.est, 0ull, w.X, d_frames, 1, B, T, Tr, F);
  HIPCHK(hipGetLastError());
  // y = inverse_stft(X): plain overlap-add to the start of each slot
  TRY(gl_iterate(g, st, w, R, iters, k_gl_project_tf, [&] {
    hipLaunchKernelGGL(k_gl_overlap_add_tf, dim3((L + 255) / 256, B), dim3(256), 0, st, w.Y, w.ypad, d_frames, T, Tr, g->win, g->hop, slot);
  }));
  hipLaunchKernelGGL(k_gl_output_tf, dim3((L + 255) / 256, B), dim3(256), 0, st, w.ypad, d_wav, d_frames, T, g->win, g->hop, d_num_samples, L, slot);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_wav_to_pcm16(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int L, int16_t* d_pcm) {
  if (!d_wav || !d_pcm || B <= 0 || L <= 0) return fail(TACO_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(k_wav_to_pcm16, dim3(B), dim3(1024), 0, (hipStream_t)hip_stream, d_wav, d_num_samples, L, d_pcm);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- silence trimming (librosa.effects.trim, synthesizer.py:266-269) ----
size_t taco_wav_trim_workspace_bytes(int B, int L, int frame_length, int hop_length) {
  (void)frame_length;
  if (B <= 0 || L <= 0 || hop_length < 1) return 0;
  Carver cv(nullptr, 0);
  cv.f((size_t)B * (1 + L / hop_length));                // mse [B, Fmax]
  return cv.off;
}

// The front of taco_wav_trim and taco_wav_split: their shared argument checks in one order, then the frame energies mse [B, Fmax]
// into the workspace (k_trim_energy).  outputs: the entry point's own result pointers are all there; max_intervals: taco_wav_split's
// table rows, checked where it always was (NULL: taco_wav_trim has none).
static int wav_frame_energies(hipStream_t st, const float* d_wav, const int32_t* d_num_samples, bool outputs, int B, int L, int frame_length,
                              int hop_length, int energy, const int* max_intervals, void* d_workspace, size_t workspace_bytes, float** mse,
                              int* Fmax) {
  if (!d_wav || !outputs || !d_workspace || B <= 0 || B > 65535 || L <= 0) return fail(TACO_ERR_ARG, "bad argument");
  if (hop_length < 1 || frame_length < 2) return fail(TACO_ERR_ARG, "bad frame parameters: frame_length %d, hop_length %d", frame_length, hop_length);
  if (max_intervals && *max_intervals < 1) return fail(TACO_ERR_ARG, "max_intervals = %d", *max_intervals);
  if (energy != TACO_TRIM_SPECTRAL && energy != TACO_TRIM_TIME) return fail(TACO_ERR_ARG, "unknown energy convention %d", energy);
  const size_t need = taco_wav_trim_workspace_bytes(B, L, frame_length, hop_length);
  if (workspace_bytes < need) return fail(TACO_ERR_ARG, "workspace too small: need %zu bytes, have %zu", need, workspace_bytes);
  if (frame_length & 1) return fail(TACO_ERR_UNSUPPORTED, "frame_length = %d: the one-sided spectrum sum is written for an even length", frame_length);
  const int fpt = trim_frames_per_tile(frame_length, hop_length, energy);
  if (fpt < 1)
    return fail(TACO_ERR_UNSUPPORTED, "frame_length = %d: k_trim_energy keeps a frame%s in %d KB of LDS", frame_length,
                energy == TACO_TRIM_SPECTRAL ? " and its window" : "", TRIM_LDS_BYTES / 1024);
  *Fmax = 1 + L / hop_length;
  *mse = (float*)d_workspace;
  hipLaunchKernelGGL(k_trim_energy, dim3(cdiv(*Fmax, fpt), B), dim3(TRIM_THREADS), trim_lds_bytes(frame_length, hop_length, fpt, energy), st, d_wav,
                     d_num_samples, L, frame_length, hop_length, fpt, *Fmax, energy, *mse);
  return 0;
}

int taco_wav_trim(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int L, float top_db, int frame_length,
                  int hop_length, int energy, int32_t* d_index, float* d_frame_db, void* d_workspace, size_t workspace_bytes) {
  hipStream_t st = (hipStream_t)hip_stream;
  float* mse; int Fmax;
  TRY(wav_frame_energies(st, d_wav, d_num_samples, d_index, B, L, frame_length, hop_length, energy, nullptr, d_workspace, workspace_bytes, &mse, &Fmax));
  hipLaunchKernelGGL(k_trim_index, dim3(B), dim3(256), 0, st, mse, d_num_samples, L, hop_length, Fmax, top_db, d_index, d_frame_db);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- splitting on silence (librosa.effects.split and remove_breath, audio/silence.py:21-31,44-45,53-54) ----
size_t taco_wav_split_workspace_bytes(int B, int L, int frame_length, int hop_length) {
  return taco_wav_trim_workspace_bytes(B, L, frame_length, hop_length);      // the same mse [B, Fmax]
}

int taco_wav_split(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int L, float top_db, int frame_length,
                   int hop_length, int energy, int max_intervals, int32_t* d_intervals, int32_t* d_counts, float* d_frame_db, void* d_workspace,
                   size_t workspace_bytes) {
  hipStream_t st = (hipStream_t)hip_stream;
  float* mse; int Fmax;
  TRY(wav_frame_energies(st, d_wav, d_num_samples, d_intervals && d_counts, B, L, frame_length, hop_length, energy, &max_intervals, d_workspace,
                         workspace_bytes, &mse, &Fmax));
  hipLaunchKernelGGL(k_split_edges, dim3(B), dim3(SPLIT_THREADS), 0, st, mse, d_num_samples, L, hop_length, Fmax, top_db, max_intervals, d_intervals,
                     d_counts, d_frame_db);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_wav_breath_mute(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int S, int L, const int32_t* d_intervals,
                         const int32_t* d_counts, int max_intervals, float threshold, float* d_out, int32_t* d_muted, float* d_abs_mean) {
  if (!d_wav || !d_intervals || !d_counts || !d_out || S <= 0 || L <= 0) return fail(TACO_ERR_ARG, "bad argument");
  if (max_intervals < 1) return fail(TACO_ERR_ARG, "max_intervals = %d", max_intervals);
  hipLaunchKernelGGL(k_breath_mute, dim3(S), dim3(MUTE_THREADS), 0, (hipStream_t)hip_stream, d_wav, d_num_samples, L, d_intervals, d_counts,
                     max_intervals, threshold, d_out, d_muted, d_abs_mean);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- waveform -> linear and mel targets ----
int taco_gl_set_mel_basis(taco_gl* g, const float* host_basis, int num_mels) {
  if (!g || !host_basis || num_mels <= 0) return fail(TACO_ERR_ARG, "bad argument");
  const int F = g->F;
  std::vector<int> band((size_t)3 * num_mels, 0);
  std::vector<float> w;
  for (int m = 0; m < num_mels; ++m) {               // the band of a filter: from its first to its last non-zero bin (a dense row: all of them)
    const float* row = host_basis + (size_t)m * F;
    int lo = F, hi = 0;
    for (int k = 0; k < F; ++k) if (row[k] != 0.f) { lo = std::min(lo, k); hi = k + 1; }
    if (hi == 0) lo = 0;
    band[m] = lo; band[num_mels + m] = hi; band[2 * num_mels + m] = (int)w.size();
    w.insert(w.end(), row + lo, row + hi);
  }
  if (w.empty()) w.push_back(0.f);
  HIPCHK(hipSetDevice(g->gm->device));
  int* d_band = nullptr; float* d_w = nullptr;
  if (hipMalloc((void**)&d_band, band.size() * sizeof(int)) != hipSuccess || hipMalloc((void**)&d_w, w.size() * sizeof(float)) != hipSuccess ||
      hipMemcpy(d_band, band.data(), band.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    if (d_band) (void)hipFree(d_band);
    if (d_w) (void)hipFree(d_w);
    return fail(TACO_ERR_HIP, "could not upload the mel filter bank");
  }
  if (g->mel_band) (void)hipFree(g->mel_band);       // (hipFree waits for the launches that still read the basis it replaces)
  if (g->mel_w) (void)hipFree(g->mel_w);
  g->mel_band = d_band; g->mel_w = d_w; g->num_mels = num_mels;
  return 0;
}

int taco_spec_num_mels(const taco_gl* g) { return g ? g->num_mels : 0; }

int taco_spec_num_frames(const taco_audio_hparams* hp, int n_samples) {      // host arithmetic only: needs no handle and no device
  const int hop = hp ? (int)(hp->frame_shift_ms / 1000.0 * hp->sample_rate) : 0;      // as taco_gl_create
  return (hop >= 1 && n_samples >= 0) ? 1 + n_samples / hop : 0;
}

size_t taco_spec_workspace_bytes(const taco_gl* g, int B, int Lmax) {
  if (!g || B <= 0 || Lmax <= 0) return 0;
  Carver cv(nullptr, 0);
  SpecWs w; carve_spec(cv, g, B, 1 + Lmax / g->hop, w);
  return cv.off;
}

// what k_spec_targets needs of the handle: a filter bank when there is a mel output, SPEC_ROWS rows of magnitudes within 64 KB of LDS
static int spec_check(const taco_gl* g, const float* d_mel) {
  if (d_mel && !g->num_mels) return fail(TACO_ERR_STATE, "the mel output needs a filter bank: call taco_gl_set_mel_basis first");
  if ((size_t)SPEC_ROWS * g->F * sizeof(float) > 64 * 1024)
    return fail(TACO_ERR_UNSUPPORTED, "num_freq = %d: k_spec_targets keeps %d rows of magnitudes in 64 KB of LDS", g->F, SPEC_ROWS);
  return 0;
}
// (the caller has passed spec_check)
static int spec_epilogue(taco_gl* g, hipStream_t st, const float* est, const int* nframes, int B, int T, int Tr, float* d_linear, float* d_mel) {
  const size_t lds = (size_t)SPEC_ROWS * g->F * sizeof(float);
  hipLaunchKernelGGL(k_spec_targets, dim3(cdiv(T, SPEC_ROWS), B), dim3(256), lds, st, est, nframes, T, Tr, g->F, g->mel_band, g->mel_w, g->num_mels,
                     d_linear, d_mel, g->hp.min_level_db, g->hp.ref_level_db);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_spec_targets(taco_gl* g, void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int Lmax, float* d_linear,
                      float* d_mel, int32_t* d_num_frames, void* d_workspace, size_t workspace_bytes) {
  if (!g || !d_wav || !d_linear || !d_workspace || B <= 0 || B > 65535 || Lmax <= 0) return fail(TACO_ERR_ARG, "bad argument");
  if (g->flavor != GL_LIBROSA) return fail(TACO_ERR_STATE, "a handle of taco_gl_create_tf serves taco_gl_inv_spectrogram_tf only");
  const int half = g->n_fft / 2, T = 1 + Lmax / g->hop, Tr = gl_rows(g, T), F = g->F;
  if (Lmax <= half) return fail(TACO_ERR_SHAPE, "utterance too short for reflect padding: Lmax = %d <= n_fft/2 = %d", Lmax, half);
  TRY(spec_check(g, d_mel));      // before anything is launched
  if ((size_t)B * Tr > (size_t)0x7fffffff) return fail(TACO_ERR_SHAPE, "too many frame rows: %zu", (size_t)B * Tr);
  HIPCHK(hipSetDevice(g->gm->device));
  hipStream_t st = (hipStream_t)hip_stream;
  Carver cv(d_workspace, workspace_bytes);
  SpecWs w; carve_spec(cv, g, B, T, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes, have %zu", cv.off, workspace_bytes);
  const size_t slot = gl_slot(g, T), tail = spec_tail(g);
  hipLaunchKernelGGL(k_spec_prepare, dim3((unsigned)((slot + tail + 255) / 256), B), dim3(256), 0, st, d_wav, d_num_samples, w.ypad, w.nf, d_num_frames,
                     B, Lmax, g->hop, half, slot, tail, g->hp.preemphasis);
  HIPCHK(hipGetLastError());
  // D = stft(p): the product the Griffin-Lim loop issues, row (b, t) = ypad[b*slot + t*hop + lpad ...][0 .. win); rows past an utterance's
  // own frames read zeros or the next slot and are stored as zeros by k_spec_targets
  GemmCall c; c.x = w.ypad + g->lpad; c.ldx = g->hop; c.M = B * Tr; c.out = w.est; c.ldo = 2 * F;
  TRY(run_gemm(g->gm, st, &g->fwd, 1, false, c));
  return spec_epilogue(g, st, w.est, w.nf, B, T, Tr, d_linear, d_mel);
}

int taco_debug_spec_epilogue(taco_gl* g, void* hip_stream, const float* d_est, int R, float* d_linear, float* d_mel) {
  if (!g || !d_est || !d_linear || R <= 0) return fail(TACO_ERR_ARG, "bad argument");
  TRY(spec_check(g, d_mel));
  HIPCHK(hipSetDevice(g->gm->device));
  return spec_epilogue(g, (hipStream_t)hip_stream, d_est, nullptr, 1, R, R, d_linear, d_mel);
}

// ---- spectral convergence of a vocoder's output against its target ----
size_t taco_gl_convergence_workspace_bytes(const taco_gl* g, int B, int T) {
  if (!g || B <= 0 || T <= 1) return 0;
  Carver cv(nullptr, 0);
  ConvWs w; carve_conv(cv, g, B, T, w);
  return cv.off;
}

// The analysis of taco_spec_targets on the vocoder's own output rectangle -- k_spec_prepare (its pre-emphasis undoes the vocoder's
// inverse pre-emphasis; reflect padding at each utterance's own ends), the forward product -- then the two convergence kernels on
// the estimate matrix.  Every check comes before the first HIP call.
int taco_gl_convergence(taco_gl* g, void* hip_stream, const float* d_target, int target_kind, const int32_t* d_frames, const float* d_wav, int B,
                        int T, float* d_sc, void* d_workspace, size_t workspace_bytes) {
  if (!g || !d_target || !d_wav || !d_sc || !d_workspace || B <= 0 || B > 65535 || T <= 1) return fail(TACO_ERR_ARG, "bad argument");
  if (target_kind != 0 && target_kind != 1) return fail(TACO_ERR_ARG, "unknown target kind %d", target_kind);
  if (g->flavor != GL_LIBROSA) return fail(TACO_ERR_STATE, "a handle of taco_gl_create_tf serves taco_gl_inv_spectrogram_tf only");
  const int L = g->hop * (T - 1), half = g->n_fft / 2, Tr = gl_rows(g, T), F = g->F, fmin = taco_gl_min_frames(g);
  if (L <= half) return fail(TACO_ERR_SHAPE, "utterance too short for reflect padding: hop*(T-1) = %d <= n_fft/2 = %d", L, half);
  if ((size_t)B * Tr > (size_t)0x7fffffff) return fail(TACO_ERR_SHAPE, "too many frame rows: %zu", (size_t)B * Tr);
  Carver cv(d_workspace, workspace_bytes);
  ConvWs w; carve_conv(cv, g, B, T, w);
  if (!cv.ok()) return fail(TACO_ERR_STATE, "workspace too small: need %zu bytes, have %zu", cv.off, workspace_bytes);
  HIPCHK(hipSetDevice(g->gm->device));
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t slot = gl_slot(g, T), tail = spec_tail(g);
  if (d_frames) hipLaunchKernelGGL(k_gl_frames_to_samples, EWGRID(B), 0, st, d_frames, fmin, T, g->hop, B, w.ns);
  // row b keeps hop*(frames_b - 1) > n_fft/2 samples, so k_spec_prepare's own clamp changes nothing and nf = 1 + n/hop = frames_b
  hipLaunchKernelGGL(k_spec_prepare, dim3((unsigned)((slot + tail + 255) / 256), B), dim3(256), 0, st, d_wav, d_frames ? w.ns : nullptr, w.spec.ypad,
                     w.spec.nf, (int*)nullptr, B, L, g->hop, half, slot, tail, g->hp.preemphasis);
  HIPCHK(hipGetLastError());
  GemmCall c; c.x = w.spec.ypad + g->lpad; c.ldx = g->hop; c.M = B * Tr; c.out = w.spec.est; c.ldo = 2 * F;      // as taco_spec_targets
  TRY(run_gemm(g->gm, st, &g->fwd, 1, false, c));
  const int P = cdiv(T, CONV_ROWS);
  hipLaunchKernelGGL(k_gl_convergence_partial, dim3(P, B), dim3(256), 0, st, w.spec.est, d_target, target_kind, w.spec.nf, T, Tr, F, g->hp.min_level_db,
                     g->hp.ref_level_db, g->hp.power, w.part);
  hipLaunchKernelGGL(k_gl_convergence_final, dim3(B), dim3(64), 0, st, w.part, P, d_sc);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_debug_gl_project(taco_gl* g, void* hip_stream, const float* d_est, const float* d_prev, const float* d_S, float* d_X, float c, int R) {
  if (!g || !d_est || !d_S || !d_X || R <= 0) return fail(TACO_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(g->gm->device));
  hipStream_t st = (hipStream_t)hip_stream;
  const bool tf = g->flavor == GL_TF;
  if (d_prev) gl_launch_project_fast(st, tf, d_est, d_prev, d_S, d_X, c, (size_t)R, g->F);
  else hipLaunchKernelGGL(tf ? k_gl_project_tf : k_gl_project, EWGRID((size_t)R * g->F), 0, st, d_est, d_S, d_X, (size_t)R, g->F);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- the stages of the Griffin-Lim path alone (include/taco_debug.h): the launches of gl_vocode_rows / taco_gl_inv_spectrogram_tf / gl_iterate on caller data ----
int taco_debug_gl_info(const taco_gl* g, int T, int* out, int n) {
  if (!g || !out || n < 0 || T < 1) return fail(TACO_ERR_ARG, "bad argument");
  const bool tf = g->flavor == GL_TF;
  const long long v[8] = {gl_rows(g, T), (long long)gl_slot(g, T), g->n_fft / 2, g->lpad, (long long)spec_tail(g), (long long)g->hop * (T - 1) + g->n_fft,
                          tf ? 1 : taco_gl_min_frames(g), tf ? taco_gl_tf_num_samples(g, T) : taco_gl_num_samples(g, T)};
  for (int i = 0; i < std::min(n, 8); ++i) out[i] = (int)v[i];
  return 0;
}
// A handle of taco_debug_gl_create_host has no device arena: nothing may be launched on it
static int gl_debug_device(const taco_gl* g) {
  if (!g->gm->darena) return fail(TACO_ERR_STATE, "a host-only handle (taco_debug_gl_create_host) serves the argument checks only");
  HIPCHK(hipSetDevice(g->gm->device));
  return 0;
}

int taco_debug_gl_prologue(taco_gl* g, void* hip_stream, const float* d_spec, const int32_t* d_frames, const float* d_init_uniform,
                           unsigned long long seed, int B, int T, float* d_S, float* d_X) {
  if (!g || !d_spec || !d_S || !d_X || B <= 0 || B > 65535) return fail(TACO_ERR_ARG, "bad argument");
  const bool tf = g->flavor == GL_TF;
  if (T < (tf ? 1 : 2)) return fail(TACO_ERR_ARG, "T = %d", T);
  const int Tr = gl_rows(g, T), F = g->F, fmin = tf ? 1 : taco_gl_min_frames(g);
  const size_t R = (size_t)B * Tr;
  if (R * 2 * F > (size_t)0x7fffffff) return fail(TACO_ERR_SHAPE, "too many elements: %zu", R * 2 * F);
  TRY(gl_debug_device(g));
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(k_gl_magnitude, EWGRID(R * F), 0, st, d_spec, d_S, d_frames, fmin, B, T, Tr, F, g->hp.min_level_db, g->hp.ref_level_db, g->hp.power);
  hipLaunchKernelGGL(k_gl_init_phase, EWGRID(R * F), 0, st, d_S, d_init_uniform, seed, d_X, d_frames, fmin, B, T, Tr, F);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_debug_gl_overlap_add(taco_gl* g, void* hip_stream, const float* d_Y, const int32_t* d_frames, int B, int T, float* d_ypad, float* d_wss) {
  if (!g || !d_Y || !d_ypad || B <= 0 || B > 65535) return fail(TACO_ERR_ARG, "bad argument");
  const bool tf = g->flavor == GL_TF;
  if (T < (tf ? 1 : 2)) return fail(TACO_ERR_ARG, "T = %d", T);
  if (!tf && !d_wss) return fail(TACO_ERR_ARG, "the librosa flavour needs the window-sum table");
  const int half = g->n_fft / 2, Tr = gl_rows(g, T), L = tf ? taco_gl_tf_num_samples(g, T) : g->hop * (T - 1);
  if (!tf && L <= half) return fail(TACO_ERR_SHAPE, "utterance too short for reflect padding: hop*(T-1) = %d <= n_fft/2 = %d", L, half);
  const size_t slot = gl_slot(g, T);
  TRY(gl_debug_device(g));
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHK(zero_async(d_ypad, ((size_t)B * slot + spec_tail(g)) * sizeof(float), st));
  if (tf) {
    hipLaunchKernelGGL(k_gl_overlap_add_tf, dim3((L + 255) / 256, B), dim3(256), 0, st, d_Y, d_ypad, d_frames, T, Tr, g->win, g->hop, slot);
  } else {
    hipLaunchKernelGGL(k_gl_wss, EWGRID((size_t)L + g->n_fft), 0, st, AP(g->gm, g->w2), d_wss, T, g->n_fft, g->hop);
    hipLaunchKernelGGL(k_gl_overlap_add, dim3((L + 255) / 256, B), dim3(256), 0, st, d_Y, d_wss, AP(g->gm, g->w2), d_ypad, d_frames, taco_gl_min_frames(g), T,
                       Tr, g->win, g->hop, g->lpad, g->n_fft, slot);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_debug_gl_inv_preemphasis(void* hip_stream, const float* d_x, const int32_t* d_frames, int fmin, int T, int hop, int B, float a,
                                  float* d_wav, int32_t* d_num_samples) {
  if (!d_x || !d_wav || B <= 0 || B > 65535) return fail(TACO_ERR_ARG, "bad argument");
  if (T < 2 || hop < 1 || fmin < 1 || fmin > T) return fail(TACO_ERR_ARG, "bad frame parameters: T %d, hop %d, fmin %d", T, hop, fmin);
  if ((long long)hop * (T - 1) > 0x7fffffffLL) return fail(TACO_ERR_ARG, "hop*(T-1) = %lld does not fit an int", (long long)hop * (T - 1));
  if (!std::isfinite(a)) return fail(TACO_ERR_ARG, "a = %g", (double)a);
  const int L = hop * (T - 1);
  hipLaunchKernelGGL(k_inv_preemphasis, dim3(B), dim3(1024), 0, (hipStream_t)hip_stream, d_x, d_wav, d_frames, fmin, T, hop, d_num_samples, L, 0, (size_t)L, a);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_debug_gl_dft(taco_gl* g, void* hip_stream, int which, int exact, const float* d_rows, size_t rows_floats, int M, int ld, float* d_out) {
  if (!g || !d_rows || !d_out || M <= 0 || ld < 1) return fail(TACO_ERR_ARG, "bad argument");
  if ((which != 0 && which != 1) || (exact != 0 && exact != 1)) return fail(TACO_ERR_ARG, "which = %d, exact = %d: each is 0 or 1", which, exact);
  const ConvL& pack = which ? g->inv : g->fwd;
  if ((size_t)(M - 1) * ld + pack.cin > rows_floats)
    return fail(TACO_ERR_ARG, "%d rows of %d at stride %d need %zu floats, d_rows holds %zu", M, pack.cin, ld, (size_t)(M - 1) * ld + pack.cin, rows_floats);
  if ((size_t)M * std::max(pack.N, ld) > (size_t)0x7fffffff) return fail(TACO_ERR_SHAPE, "too many elements");
  TRY(gl_debug_device(g));
  GemmCall c; c.x = d_rows; c.ldx = ld; c.M = M; c.out = d_out; c.ldo = pack.N;
  c.force = exact ? GEMM_FORCE_EXACT : GEMM_FORCE_NONE;
  TRY(run_gemm(g->gm, (hipStream_t)hip_stream, &pack, 1, false, c));
  return 0;
}

// ---- splitting and levelling 16-bit PCM on silence: pydub.silence.detect_nonsilent (audio/silence.py:81-117, app.py:27-53) ----
// The workspace of taco_pcm_nonsilent: the energies E [B, Mmax] first (taco_pcm_range_sumsq reads them from there), then the flags
struct PcmWs { unsigned long long* E; unsigned char* silent; };
static void carve_pcm(Carver& cv, int B, int Mmax, PcmWs& w) {
  w.E = (unsigned long long*)cv.raw((size_t)B * Mmax * sizeof(unsigned long long));
  w.silent = (unsigned char*)cv.raw((size_t)B * Mmax);
}
// Milliseconds of a row of L frames (every row's M_b is at most this); -1 where it passes what an int32 table can hold
static long long pcm_len_max(int L, int sample_rate) {
  const double m = rint(1000.0 * ((double)L / (double)sample_rate));
  return m <= 2.0e9 ? (long long)m : -1;
}
// The front of the three entry points: the shape of the rectangle and the grid of milliseconds, in one order.  The rate rule: with
// r = fl(sr/1000.0) >= sr/1000, fl(j*r) is never below an integral j*sr/1000 and stays within 1/1000 of any other while j*sr/1000 <
// 2^52/1000, so pydub's int(j * (sr/1000.0)) equals floor(j*sr/1000) at every millisecond of any row; with r below sr/1000 (1001 Hz
// at j = 1000) it does not, and such a rate is refused.  fma forms r*1000 - sr with one rounding: its sign is exact.
static int pcm_grid(int B, int L, int channels, int sample_rate, int max_ranges, int* Mmax) {
  if (B < 1 || B > 65535 || L < 1 || channels < 1 || sample_rate < 1)
    return fail(TACO_ERR_ARG, "bad argument: B %d, L %d, channels %d, sample_rate %d", B, L, channels, sample_rate);
  if (max_ranges < 1) return fail(TACO_ERR_ARG, "max_ranges = %d", max_ranges);
  const long long m = pcm_len_max(L, sample_rate);
  if (m < 0) return fail(TACO_ERR_SHAPE, "L = %d frames at %d Hz: more milliseconds than an int32 table holds", L, sample_rate);
  *Mmax = (int)m;
  return 0;
}
static int pcm_rate_check(int sample_rate) {
  if (!taco_pcm_rate_supported(sample_rate))
    return fail(TACO_ERR_UNSUPPORTED, "sample_rate = %d: sample_rate/1000.0 rounds below the quotient, where pydub's int(j * (sr/1000.0)) "
                "and floor(j*sr/1000) part", sample_rate);
  return 0;
}

int taco_pcm_rate_supported(int sample_rate) {      // host arithmetic only: needs no device
  return sample_rate >= 1 && std::fma((double)sample_rate / 1000.0, 1000.0, -(double)sample_rate) >= 0.0;
}

// k_pcm_energy on a rectangle the caller has checked (pcm_grid, pcm_rate_check, ept >= 1, Mmax > 0)
static void pcm_launch_energy(hipStream_t st, const int16_t* d_pcm, const int32_t* d_num_frames, int B, int L, int channels, int sample_rate, int ept,
                              int Mmax, unsigned long long* E) {
  hipLaunchKernelGGL(k_pcm_energy, dim3(cdiv(Mmax, ept), B), dim3(PCM_THREADS), (pcm_energy_span_words(ept, channels, sample_rate) + 16) * sizeof(short),
                     st, d_pcm, d_num_frames, L, channels, sample_rate, ept, Mmax, E);
}

size_t taco_pcm_nonsilent_workspace_bytes(int B, int L, int sample_rate) {
  if (B < 1 || L < 1 || sample_rate < 1) return 0;
  const long long m = pcm_len_max(L, sample_rate);
  if (m < 0) return 0;
  Carver cv(nullptr, 0);
  PcmWs w; carve_pcm(cv, B, (int)m, w);
  return cv.off;
}

int taco_pcm_nonsilent(void* hip_stream, const int16_t* d_pcm, const int32_t* d_num_frames, int B, int L, int channels, int sample_rate,
                       int min_silence_len, int k, int max_ranges, int32_t* d_ranges, int32_t* d_counts, int32_t* d_len_ms,
                       uint64_t* d_window_sumsq, void* d_workspace, size_t workspace_bytes) {
  if (!d_pcm || !d_ranges || !d_counts || !d_workspace) return fail(TACO_ERR_ARG, "null argument");
  int Mmax;
  TRY(pcm_grid(B, L, channels, sample_rate, max_ranges, &Mmax));
  if (min_silence_len < 1) return fail(TACO_ERR_ARG, "min_silence_len = %d", min_silence_len);
  if (k < 0) return fail(TACO_ERR_ARG, "k = %d: the bound floor(10^(dB/20) * 32768) is not negative", k);
  if ((reinterpret_cast<uintptr_t>(d_pcm) & 1) || (reinterpret_cast<uintptr_t>(d_workspace) & 7) || (reinterpret_cast<uintptr_t>(d_window_sumsq) & 7))
    return fail(TACO_ERR_ARG, "misaligned pointer: d_pcm holds 2-byte words, the workspace and d_window_sumsq 8-byte words");
  const size_t need = taco_pcm_nonsilent_workspace_bytes(B, L, sample_rate);
  if (workspace_bytes < need) return fail(TACO_ERR_ARG, "workspace too small: need %zu bytes, have %zu", need, workspace_bytes);
  TRY(pcm_rate_check(sample_rate));
  if (k > 32768) k = 32768;      // no rms passes 32768: a larger bound means what 32768 does
  const int W = min_silence_len, ept = pcm_energy_tile(channels, sample_rate);
  if (ept < 1)
    return fail(TACO_ERR_UNSUPPORTED, "sample_rate %d x %d channels: k_pcm_energy keeps a millisecond of samples in %d KB of LDS", sample_rate, channels,
                PCM_E_LDS_WORDS * 2 / 1024);
  const size_t wlds = ((size_t)PCM_W_TILE + W) * sizeof(unsigned long long);
  if (wlds + 256 > PCM_W_LDS_BYTES)
    return fail(TACO_ERR_UNSUPPORTED, "min_silence_len = %d: k_pcm_windows keeps %d + min_silence_len energies in %d KB of LDS", W, PCM_W_TILE,
                PCM_W_LDS_BYTES / 1024);
  const unsigned __int128 kk = (unsigned __int128)(k + 1LL) * (unsigned __int128)(k + 1LL);
  const unsigned __int128 cmax = (unsigned __int128)((long long)W * sample_rate / 1000 + 1) * (unsigned)channels;
  if (kk * cmax >= ((unsigned __int128)1 << 52))
    return fail(TACO_ERR_UNSUPPORTED, "(k + 1)^2 times the samples of a window reaches 2^52 (k %d, min_silence_len %d, sample_rate %d, channels %d): "
                "the integer comparison stands for audioop.rms's double only below that", k, W, sample_rate, channels);
  hipStream_t st = (hipStream_t)hip_stream;
  Carver cv(d_workspace, workspace_bytes);
  PcmWs w; carve_pcm(cv, B, Mmax, w);
  if (Mmax > 0) {      // (a rectangle shorter than half a millisecond has no energies and no windows: every row is [[0, 0]])
    pcm_launch_energy(st, d_pcm, d_num_frames, B, L, channels, sample_rate, ept, Mmax, w.E);
    hipLaunchKernelGGL(k_pcm_windows, dim3(cdiv(Mmax, PCM_W_TILE), B), dim3(PCM_THREADS), wlds, st, w.E, d_num_frames, L, channels, sample_rate, W,
                       (unsigned long long)kk, Mmax, w.silent, (unsigned long long*)d_window_sumsq);
  }
  hipLaunchKernelGGL(k_pcm_ranges, dim3(B), dim3(PCM_THREADS), 0, st, w.silent, d_num_frames, L, sample_rate, W, Mmax, max_ranges, d_ranges, d_counts,
                     d_len_ms);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_pcm_range_sumsq(void* hip_stream, const uint64_t* d_energy, const int32_t* d_num_frames, int B, int L, int channels, int sample_rate,
                         const int32_t* d_ranges, const int32_t* d_counts, int max_ranges, uint64_t* d_sumsq, int64_t* d_samples) {
  if (!d_energy || !d_ranges || !d_counts || !d_sumsq || !d_samples) return fail(TACO_ERR_ARG, "null argument");
  int Mmax;
  TRY(pcm_grid(B, L, channels, sample_rate, max_ranges, &Mmax));
  if ((reinterpret_cast<uintptr_t>(d_energy) & 7) || (reinterpret_cast<uintptr_t>(d_sumsq) & 7) || (reinterpret_cast<uintptr_t>(d_samples) & 7))
    return fail(TACO_ERR_ARG, "misaligned pointer: d_energy, d_sumsq and d_samples hold 8-byte words");
  TRY(pcm_rate_check(sample_rate));
  hipLaunchKernelGGL(k_pcm_range_sumsq, dim3(cdiv(max_ranges, PCM_THREADS / 64), B), dim3(PCM_THREADS), 0, (hipStream_t)hip_stream,
                     (const unsigned long long*)d_energy, d_num_frames, L, channels, sample_rate, Mmax, d_ranges, d_counts, max_ranges,
                     (unsigned long long*)d_sumsq, (long long*)d_samples);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_pcm_apply_gains(void* hip_stream, const int16_t* d_pcm, const int32_t* d_num_frames, int B, int L, int channels, int sample_rate,
                         const int32_t* d_ranges, const int32_t* d_counts, int max_ranges, const double* d_gains, int16_t* d_out, int L_out,
                         int32_t* d_out_frames) {
  if (!d_pcm || !d_ranges || !d_counts || !d_gains || !d_out) return fail(TACO_ERR_ARG, "null argument");
  int Mmax;
  TRY(pcm_grid(B, L, channels, sample_rate, max_ranges, &Mmax));
  if (L_out < 1) return fail(TACO_ERR_ARG, "L_out = %d", L_out);
  if ((reinterpret_cast<uintptr_t>(d_pcm) & 1) || (reinterpret_cast<uintptr_t>(d_out) & 1) || (reinterpret_cast<uintptr_t>(d_gains) & 7))
    return fail(TACO_ERR_ARG, "misaligned pointer: d_pcm and d_out hold 2-byte words, d_gains 8-byte words");
  TRY(pcm_rate_check(sample_rate));
  hipLaunchKernelGGL(k_pcm_apply_gains, dim3(cdiv(L_out, PCM_THREADS), B), dim3(PCM_THREADS), 0, (hipStream_t)hip_stream, d_pcm, d_num_frames, L,
                     channels, sample_rate, d_ranges, d_counts, max_ranges, d_gains, d_out, L_out, d_out_frames);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_debug_pcm_energy(void* hip_stream, const int16_t* d_pcm, const int32_t* d_num_frames, int B, int L, int channels, int sample_rate,
                          uint64_t* d_energy) {
  if (!d_pcm || !d_energy) return fail(TACO_ERR_ARG, "null argument");
  int Mmax;
  TRY(pcm_grid(B, L, channels, sample_rate, 1, &Mmax));
  if ((reinterpret_cast<uintptr_t>(d_pcm) & 1) || (reinterpret_cast<uintptr_t>(d_energy) & 7))
    return fail(TACO_ERR_ARG, "misaligned pointer: d_pcm holds 2-byte words, d_energy 8-byte words");
  TRY(pcm_rate_check(sample_rate));
  const int ept = pcm_energy_tile(channels, sample_rate);
  if (ept < 1) return fail(TACO_ERR_UNSUPPORTED, "sample_rate %d x %d channels: k_pcm_energy keeps a millisecond of samples in %d KB of LDS", sample_rate, channels,
                           PCM_E_LDS_WORDS * 2 / 1024);
  if (Mmax > 0) pcm_launch_energy((hipStream_t)hip_stream, d_pcm, d_num_frames, B, L, channels, sample_rate, ept, Mmax, (unsigned long long*)d_energy);
  HIPCHK(hipGetLastError());
  return 0;
}
