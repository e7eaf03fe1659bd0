// taco_f0_api.h -- C ABI of pitch tracking (kernels in taco_f0.h); included inside extern "C".

// every check of taco_f0_yin, before any HIP call; fills the lag range, the column count and the plan
static int f0_yin_check(const float* d_wav, const int32_t* d_num_samples, int B, int L, int sample_rate, int hop, int window, float fmin, float fmax,
                        float threshold, float* d_f0, float* d_aper, int32_t* d_lag, int* tau_min, int* tau_max, int* F, YinPlan* pl) {
  if (!d_wav || !d_f0) return fail(TACO_ERR_ARG, "null pointer");
  if (B < 1 || L < 1 || hop < 1 || window < 1) return fail(TACO_ERR_ARG, "B, L, hop and window must be >= 1, got %d, %d, %d, %d", B, L, hop, window);
  if (sample_rate < 1) return fail(TACO_ERR_ARG, "sample_rate = %d", sample_rate);
  if (!(fmin > 0.f) || !(fmax > fmin)) return fail(TACO_ERR_ARG, "fmin = %g, fmax = %g: 0 < fmin < fmax is required", (double)fmin, (double)fmax);
  const double lo = std::floor((double)sample_rate / (double)fmax), hi = std::ceil((double)sample_rate / (double)fmin);
  if (lo < 2.0) return fail(TACO_ERR_ARG, "fmax = %g at %d Hz: the shortest lag floor(sample_rate / fmax) must be >= 2", (double)fmax, sample_rate);
  if (!(threshold > 0.f) || !(threshold <= 1.f)) return fail(TACO_ERR_ARG, "threshold = %g is outside (0, 1]", (double)threshold);
  const int nf = 1 + L / hop;
  *F = nf;
  const u128 nb = (u128)(unsigned)B, nout = nb * (unsigned)nf * sizeof(float);
  TRY(no_overlap({{d_f0, nout, "d_f0"}, {d_aper, nout, "d_aper"}, {d_lag, nout, "d_lag"},                         // three outputs, then two inputs
                  {d_wav, nb * (unsigned)L * sizeof(float), "d_wav"}, {d_num_samples, nb * sizeof(int32_t), "d_num_samples"}}, 3));
  if (hi + (double)window + 2.0 > (double)YIN_FRAME_MAX)
    return fail(TACO_ERR_UNSUPPORTED, "a frame of window + tau_max + 2 = %d + %.0f + 2 floats: k_yin holds a frame and its lag sums in LDS, up to %d",
                window, hi, YIN_FRAME_MAX);
  *tau_min = (int)lo;
  *tau_max = (int)hi;
  *pl = yin_plan(window, *tau_max, hop);
  return 0;
}

// plain: k_yin<true>, the form that walks j (taco_debug_f0_yin_plain: the benchmark and one equality test)
static int f0_yin(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int L, int sample_rate, int hop, int window, float fmin,
                  float fmax, float threshold, float* d_f0, float* d_aper, int32_t* d_lag, bool plain) {
  int tau_min, tau_max, F;
  YinPlan pl;
  TRY(f0_yin_check(d_wav, d_num_samples, B, L, sample_rate, hop, window, fmin, fmax, threshold, d_f0, d_aper, d_lag, &tau_min, &tau_max, &F, &pl));
  const auto launch = !plain ? yin_launch<false> : yin_launch<true>;      // k_yin<false> is instantiated first: the order of the code object
  return launch((hipStream_t)hip_stream, pl, d_wav, d_num_samples, B, L, F, hop, window, tau_min, tau_max, (float)sample_rate, threshold, d_f0, d_aper,
                d_lag);
}

int taco_f0_yin(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int L, int sample_rate, int hop, int window, float fmin,
                float fmax, float threshold, float* d_f0, float* d_aper, int32_t* d_lag) {
  return f0_yin(hip_stream, d_wav, d_num_samples, B, L, sample_rate, hop, window, fmin, fmax, threshold, d_f0, d_aper, d_lag, false);
}

int taco_debug_f0_yin_plain(void* hip_stream, const float* d_wav, const int32_t* d_num_samples, int B, int L, int sample_rate, int hop, int window,
                            float fmin, float fmax, float threshold, float* d_f0, float* d_aper, int32_t* d_lag) {
  return f0_yin(hip_stream, d_wav, d_num_samples, B, L, sample_rate, hop, window, fmin, fmax, threshold, d_f0, d_aper, d_lag, true);
}

int taco_f0_path_stats(void* hip_stream, const float* d_f0_a, int Fa, const float* d_f0_b, int Fb, const int32_t* d_path, const int32_t* d_path_len,
                       int B, int path_cap, float* d_stats) {
  if (!d_f0_a || !d_f0_b || !d_path || !d_path_len || !d_stats) return fail(TACO_ERR_ARG, "null pointer");
  if (B < 1 || Fa < 1 || Fb < 1 || path_cap < 1) return fail(TACO_ERR_ARG, "B, Fa, Fb and path_cap must be >= 1, got %d, %d, %d, %d", B, Fa, Fb, path_cap);
  const u128 nb = (u128)(unsigned)B;
  TRY(no_overlap({{d_stats, nb * 4 * sizeof(float), "d_stats"}, {d_f0_a, nb * (unsigned)Fa * sizeof(float), "d_f0_a"},
                  {d_f0_b, nb * (unsigned)Fb * sizeof(float), "d_f0_b"}, {d_path, nb * (unsigned)path_cap * 2 * sizeof(int32_t), "d_path"},
                  {d_path_len, nb * sizeof(int32_t), "d_path_len"}}, 1));
  hipLaunchKernelGGL(k_f0_path_stats, dim3((unsigned)std::min(B, YIN_MAXGRID)), dim3(F0S_NT), 0, (hipStream_t)hip_stream, d_f0_a, Fa, d_f0_b, Fb,
                     d_path, d_path_len, B, path_cap, d_stats);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_debug_f0_info(int* out, int n) {
  if (!out || n < 0) return fail(TACO_ERR_ARG, "null pointer or negative count");
  const int v[7] = {64, YIN_LB, YIN_JC, YIN_FPW, YIN_NT, YIN_FRAME_MAX, YIN_LDS_FLOATS};
  for (int k = 0; k < n && k < 7; ++k) out[k] = v[k];
  return 0;
}

// the layout k_yin runs a (window, tau_max, hop) with: out = {lag blocks, j parts, j per part, frames per workgroup, LDS floats}
int taco_debug_f0_plan(int window, int tau_max, int hop, int* out) {
  if (!out || window < 1 || tau_max < 2 || hop < 1 || (long long)window + tau_max + 2 > YIN_FRAME_MAX) return fail(TACO_ERR_ARG, "bad argument");
  const YinPlan p = yin_plan(window, tau_max, hop);
  out[0] = p.nblk; out[1] = p.P; out[2] = p.JP; out[3] = p.fpw; out[4] = (int)p.lds_floats;
  return 0;
}
