// taco_envelope_api.h -- C ABI of the spectral envelope and the pitch / formant shift (kernels in taco_envelope.h); included inside extern "C".

// The two tables on the host in double, in the order include/taco_abi.h states, rounded once.  The cosines come from the caller: no libm
// call of this library decides a bit (the precedent of taco_resample_create and taco_gl_set_mel_basis).
int taco_envelope_create(int W, int Q, const double* host_basis, const double* host_lifter, int device, taco_envelope** out) {
#pragma clang fp contract(off)
  if (!host_basis || !out) return fail(TACO_ERR_ARG, "null argument");
  if (W < 3 || Q < 1 || Q > W - 1) return fail(TACO_ERR_ARG, "W >= 3 and 1 <= Q <= W - 1 are required, got W = %d, Q = %d", W, Q);
  for (size_t x = 0; x < (size_t)Q * W; ++x)
    if (!std::isfinite(host_basis[x]) || std::fabs(host_basis[x]) > 1.0)
      return fail(TACO_ERR_ARG, "host_basis[%zu, %zu] = %g is no cosine: not finite, or above 1 in magnitude", x / W, x % W, host_basis[x]);
  if (host_lifter)
    for (int n = 0; n < Q; ++n)
      if (!std::isfinite(host_lifter[n])) return fail(TACO_ERR_ARG, "host_lifter[%d] is not finite", n);
  if (Q > EV_MAX_Q) return fail(TACO_ERR_UNSUPPORTED, "Q = %d: the kernels keep at most %d cepstral coefficients", Q, EV_MAX_Q);
  if (W > EV_MAX_W)
    return fail(TACO_ERR_UNSUPPORTED, "W = %d: %d frames of v and of the envelope fit the LDS up to W = %d", W, EV_ROWS_WIDE, EV_MAX_W);
  taco_envelope* h = new taco_envelope();
  h->W = W; h->Q = Q; h->device = device;
  h->A.resize((size_t)Q * W); h->S.resize((size_t)Q * W);
  const double M = (double)(W - 1);
  for (int n = 0; n < Q; ++n) {
    const double al = (n == 0 ? 1.0 : 2.0) * (host_lifter ? host_lifter[n] : 1.0);
    for (int k = 0; k < W; ++k) {
      const double b = host_basis[(size_t)n * W + k], wk = (k == 0 || k == W - 1) ? 0.5 : 1.0;
      h->A[(size_t)n * W + k] = (float)((wk * b) / M);
      h->S[(size_t)n * W + k] = (float)(al * b);
    }
  }
  *out = h;
  return 0;
}

void taco_envelope_destroy(taco_envelope* e) {
  if (!e) return;
  if (e->d_tab) (void)hipFree(e->d_tab);
  delete e;
}

int taco_envelope_width(const taco_envelope* e) { return e ? e->W : 0; }
int taco_envelope_order(const taco_envelope* e) { return e ? e->Q : 0; }

int taco_envelope_tables(const taco_envelope* e, float* host_A, float* host_S) {
  if (!e || !host_A || !host_S) return fail(TACO_ERR_ARG, "null argument");
  memcpy(host_A, e->A.data(), e->A.size() * sizeof(float));
  memcpy(host_S, e->S.data(), e->S.size() * sizeof(float));
  return 0;
}

// the tables stay on the host until the first call that needs them on the device: A [QP, WP], then S^T [WP, QP], zero filled
static int ev_upload(taco_envelope* e) {
  std::lock_guard<std::mutex> lock(e->mu);
  if (e->d_tab) return 0;
  const EvDims d = ev_dims(e->W, e->Q);
  const size_t half = (size_t)d.QP * d.WP;
  std::vector<float> t(2 * half, 0.f);
  for (int n = 0; n < e->Q; ++n)
    for (int k = 0; k < e->W; ++k) {
      t[(size_t)n * d.WP + k] = e->A[(size_t)n * e->W + k];
      t[half + (size_t)k * d.QP + n] = e->S[(size_t)n * e->W + k];
    }
  float* p = nullptr;
  if (hipMalloc((void**)&p, t.size() * sizeof(float)) != hipSuccess ||
      hipMemcpy(p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    if (p) (void)hipFree(p);
    return fail(TACO_ERR_HIP, "could not upload the envelope tables");
  }
  e->d_tab = p;
  return 0;
}

// the instantiation for QP / 16 coefficient tiles
#define EV_PICK(K, nt) ((nt) == 1 ? K<1> : (nt) == 2 ? K<2> : (nt) == 3 ? K<3> : (nt) == 4 ? K<4> : (nt) == 5 ? K<5> : (nt) == 6 ? K<6> : (nt) == 7 ? K<7> : K<8>)

// what both calls do after their checks: the device, the tables, the LDS the kernel asks for.  -> the grid
static int ev_prepare(taco_envelope* e, const void* kernel, long long rows, EvDims& d, size_t& lds, unsigned& grid) {
  d = ev_dims(e->W, e->Q);
  lds = ev_lds_floats(d) * sizeof(float);
  HIPCHK(hipSetDevice(e->device));
  TRY(ev_upload(e));
  // (asked every time, as k_yin does: no state between calls; for what the launch takes and no more -- the kernel's barrier-with-vote keeps
  // a few static words of its own, and the two together must fit the 160 KB)
  if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  grid = (unsigned)std::min<long long>((rows + d.R - 1) / d.R, 0x7fffffffLL);
  return 0;
}

int taco_spec_envelope(taco_envelope* e, void* hip_stream, const float* d_spec, const int32_t* d_frames, int B, int T, float* d_env, float* d_cep) {
  if (!e || !d_spec || !d_env) return fail(TACO_ERR_ARG, "null pointer");
  if (B < 1 || T < 1) return fail(TACO_ERR_ARG, "B and T must be >= 1, got %d, %d", B, T);
  const u128 nb = (u128)(unsigned)B, nspec = nb * (unsigned)T * (unsigned)e->W * sizeof(float);
  TRY(no_overlap({{d_env, nspec, "d_env"}, {d_cep, nb * (unsigned)T * (unsigned)e->Q * sizeof(float), "d_cep"}, {d_spec, nspec, "d_spec"},
                  {d_frames, nb * sizeof(int32_t), "d_frames"}}, 2));
  EvDims d; size_t lds; unsigned grid;
  const long long rows = (long long)B * T;
  const auto kernel = EV_PICK(k_spec_envelope, cdiv(e->Q, EV_TILE));
  TRY(ev_prepare(e, reinterpret_cast<const void*>(kernel), rows, d, lds, grid));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(EV_NT), lds, (hipStream_t)hip_stream, d_spec, d_frames, e->d_tab,
                     e->d_tab + (size_t)d.QP * d.WP, T, e->W, e->Q, rows, d_env, d_cep);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_spec_warp_formant(taco_envelope* e, void* hip_stream, const float* d_spec, const int32_t* d_frames, const int32_t* d_src,
                           const int32_t* d_frac, const int32_t* d_out_frames, const float* d_pitch_scale, const float* d_formant_scale, int B,
                           int T, int T_out, float* d_out) {
  if (!e || !d_spec || !d_src || !d_frac || !d_out_frames || !d_out) return fail(TACO_ERR_ARG, "null pointer");
  if (B < 1 || T < 1 || T_out < 1) return fail(TACO_ERR_ARG, "B, T and T_out must be >= 1, got %d, %d, %d", B, T, T_out);
  const u128 nb = (u128)(unsigned)B, nmap = nb * (unsigned)T_out * sizeof(int32_t);
  TRY(no_overlap({{d_out, nb * (unsigned)T_out * (unsigned)e->W * sizeof(float), "d_out"},
                  {d_spec, nb * (unsigned)T * (unsigned)e->W * sizeof(float), "d_spec"}, {d_frames, nb * sizeof(int32_t), "d_frames"},
                  {d_src, nmap, "d_src"}, {d_frac, nmap, "d_frac"}, {d_out_frames, nb * sizeof(int32_t), "d_out_frames"},
                  {d_pitch_scale, nb * sizeof(float), "d_pitch_scale"}, {d_formant_scale, nb * sizeof(float), "d_formant_scale"}}, 1));
  EvDims d; size_t lds; unsigned grid;
  const long long rows = (long long)B * T_out;
  const auto kernel = EV_PICK(k_spec_warp_formant, cdiv(e->Q, EV_TILE));
  TRY(ev_prepare(e, reinterpret_cast<const void*>(kernel), rows, d, lds, grid));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(EV_NT), lds, (hipStream_t)hip_stream, d_spec, d_frames, d_src, d_frac, d_out_frames,
                     d_pitch_scale, d_formant_scale, e->d_tab, e->d_tab + (size_t)d.QP * d.WP, T, e->W, e->Q, T_out, rows, d_out);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_debug_envelope_info(int* out, int n) {
  if (!out || n < 0) return fail(TACO_ERR_ARG, "null pointer or negative count");
  const int v[8] = {EV_ROWS, 64, EV_TILE, EV_KSTEP, EV_MAX_W, EV_W16, EV_ROWS_WIDE, EV_MAX_Q};
  for (int k = 0; k < n && k < 8; ++k) out[k] = v[k];
  return 0;
}
