// taco_resample_api.h -- C ABI of resampling to the model's sample rate; included inside extern "C".

static int rs_gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }
// the most inputs a tile of k_resample stages: those under RS_TILE consecutive outputs, and the filter's reach around them
static size_t rs_span(int P, int Q, int taps) { return (size_t)((long long)(RS_TILE - 1) * Q / P) + 1 + taps; }

// The polyphase bank of resampy.resample's interpolated filter, in double with the reference's operations in the reference's order
// (include/taco_abi.h); `win + eta*delta` must round twice as NumPy's does, so contraction is off for this function.
int taco_resample_create(int orig_sr, int target_sr, const double* host_half_window, int n_window, int num_table, int device, taco_resample** out) {
#pragma clang fp contract(off)
  if (!host_half_window || !out) return fail(TACO_ERR_ARG, "null argument");
  if (orig_sr <= 0 || target_sr <= 0) return fail(TACO_ERR_ARG, "bad sample rates: orig_sr %d, target_sr %d", orig_sr, target_sr);
  if (num_table < 1 || n_window < 2) return fail(TACO_ERR_ARG, "bad filter table: n_window %d, num_table %d", n_window, num_table);
  const double ratio = (double)target_sr / orig_sr, scale = std::min(1.0, ratio);
  const int step = (int)(scale * num_table);
  if (step == 0)
    return fail(TACO_ERR_ARG, "int(scale*num_table) = 0: a table of %d entries per zero crossing cannot serve the ratio %d/%d", num_table, target_sr, orig_sr);
  const int g = rs_gcd(orig_sr, target_sr), P = target_sr / g, Q = orig_sr / g, nwin = n_window;
  std::vector<double> win(nwin), delta(nwin, 0.0);
  for (int i = 0; i < nwin; ++i) win[i] = ratio < 1.0 ? host_half_window[i] * ratio : host_half_window[i];
  for (int i = 0; i + 1 < nwin; ++i) delta[i] = win[i + 1] - win[i];
  // offset into the table, interpolation weight and tap count of one wing at one phase
  auto wing = [&](double frac, int& off, double& eta) {
    const double f = frac * num_table;
    off = (int)f; eta = f - off;
    return std::max(0, nwin - off) / step;
  };
  int LW = 0, RW = 0;
  for (int r = 0; r < P; ++r) {
    const double frac = scale * ((double)r / P);
    int off; double eta;
    LW = std::max(LW, wing(frac, off, eta));
    RW = std::max(RW, wing(scale - frac, off, eta));
  }
  const int taps = LW + RW;
  if (taps < 1) return fail(TACO_ERR_ARG, "the filter has no taps: n_window %d, num_table %d", n_window, num_table);
  if ((size_t)P * taps > RS_BANK_CAP)
    return fail(TACO_ERR_ARG, "filter bank too large: %d phases x %d taps = %zu entries, the cap is %u (%d -> %d Hz reduces to %d/%d)", P, taps,
                (size_t)P * taps, RS_BANK_CAP, orig_sr, target_sr, P, Q);
  if (rs_span(P, Q, taps) > RS_LDS_FLOATS)
    return fail(TACO_ERR_UNSUPPORTED, "%d -> %d Hz: k_resample keeps the %zu inputs of %d outputs and %d taps in %d KB of LDS", orig_sr, target_sr,
                rs_span(P, Q, taps), RS_TILE, taps, RS_LDS_FLOATS * 4 / 1024);
  taco_resample* h = new taco_resample();
  h->orig_sr = orig_sr; h->target_sr = target_sr; h->device = device; h->P = P; h->Q = Q; h->LW = LW; h->RW = RW; h->ratio = ratio;
  h->bank.assign((size_t)P * taps, 0.f);
  for (int r = 0; r < P; ++r) {
    float* row = h->bank.data() + (size_t)r * taps;
    const double frac = scale * ((double)r / P);
    int off; double eta;
    int cnt = wing(frac, off, eta);
    for (int i = 0; i < cnt; ++i) row[LW - 1 - i] = (float)(win[off + i * step] + eta * delta[off + i * step]);      // x[n - i]
    cnt = wing(scale - frac, off, eta);
    for (int k = 0; k < cnt; ++k) row[LW + k] = (float)(win[off + k * step] + eta * delta[off + k * step]);          // x[n + k + 1]
  }
  *out = h;
  return 0;
}

void taco_resample_destroy(taco_resample* r) {
  if (!r) return;
  if (r->d_bank) (void)hipFree(r->d_bank);
  delete r;
}

int taco_resample_out_len(const taco_resample* r, int n) { return (r && n > 0) ? (int)std::ceil((double)n * r->ratio) : 0; }
int taco_resample_computed_len(const taco_resample* r, int n) { return (r && n > 0) ? (int)((double)n * r->ratio) : 0; }
int taco_resample_phases(const taco_resample* r) { return r ? r->P : 0; }
int taco_resample_taps(const taco_resample* r) { return r ? r->LW + r->RW : 0; }
int taco_resample_left_taps(const taco_resample* r) { return r ? r->LW : 0; }
int taco_resample_tile(const taco_resample* r) { return r ? RS_TILE : 0; }

int taco_resample_bank(const taco_resample* r, float* host_out) {
  if (!r || !host_out) return fail(TACO_ERR_ARG, "null argument");
  memcpy(host_out, r->bank.data(), r->bank.size() * sizeof(float));
  return 0;
}

// the bank stays on the host until the first call that needs it on the device (a handle can be made and queried without one)
static int rs_upload(taco_resample* r) {
  std::lock_guard<std::mutex> lock(r->mu);
  if (r->d_bank) return 0;
  const int P = r->P, taps = r->LW + r->RW;
  std::vector<float> t((size_t)taps * P);
  for (int p = 0; p < P; ++p)
    for (int j = 0; j < taps; ++j) t[(size_t)j * P + p] = r->bank[(size_t)p * taps + j];
  float* d = nullptr;
  if (hipMalloc((void**)&d, t.size() * sizeof(float)) != hipSuccess ||
      hipMemcpy(d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    if (d) (void)hipFree(d);
    return fail(TACO_ERR_HIP, "could not upload the resampling filter bank");
  }
  r->d_bank = d;
  return 0;
}

int taco_wav_resample(taco_resample* r, void* hip_stream, const void* d_in, int in_format, int channels, const int32_t* d_num_samples, int B,
                      int L, float* d_out, int L_out, int32_t* d_out_samples) {
  if (!r || !d_in || !d_out || B <= 0 || B > 65535 || L <= 0) return fail(TACO_ERR_ARG, "bad argument");
  if (in_format != TACO_WAV_F32 && in_format != TACO_WAV_PCM16) return fail(TACO_ERR_ARG, "unknown input format %d", in_format);
  if (channels < 1) return fail(TACO_ERR_ARG, "channels = %d", channels);
  if ((double)L * r->ratio > 2147483647.0) return fail(TACO_ERR_ARG, "L = %d: the resampled row would pass 2^31 - 1 samples", L);
  const int need = taco_resample_out_len(r, L);
  if (L_out < need) return fail(TACO_ERR_ARG, "L_out = %d: %d samples at %d Hz give %d at %d Hz", L_out, L, r->orig_sr, need, r->target_sr);
  HIPCHK(hipSetDevice(r->device));
  TRY(rs_upload(r));
  const int taps = r->LW + r->RW;
  hipLaunchKernelGGL(k_resample, dim3(cdiv(L_out, RS_TILE), B), dim3(RS_THREADS), rs_span(r->P, r->Q, taps) * sizeof(float), (hipStream_t)hip_stream,
                     d_in, in_format, channels, d_num_samples, L, r->d_bank, r->P, r->Q, r->LW, taps, r->ratio, d_out, L_out, d_out_samples);
  HIPCHK(hipGetLastError());
  return 0;
}
