// taco_warp_api.h -- C ABI of rate, duration and pitch control on the spectrogram (kernels in taco_warp.h); included inside extern "C".

size_t taco_spec_warp_workspace_bytes(int B, int T) {
  if (B < 1 || T < 1) return 0;
  return (size_t)B * wm_ws_row_bytes(T);                          // C [B, T] int64, then the steps' tokens [B, T] int32
}

int taco_spec_warp_map(void* hip_stream, const float* d_alignments, const int32_t* d_frames, const float* d_row_stretch,
                       const float* d_token_stretch, int B, int T_in, int n_steps, int reduction_factor, int T, int T_out, int32_t* d_src,
                       int32_t* d_frac, int32_t* d_out_frames, int32_t* d_token_frames, void* d_workspace, size_t workspace_bytes) {
  if (!d_src || !d_frac || !d_out_frames || !d_workspace) return fail(TACO_ERR_ARG, "null pointer");
  if (B < 1 || T < 1 || T_out < 1 || reduction_factor < 1)
    return fail(TACO_ERR_ARG, "B, T, T_out and reduction_factor must be >= 1, got %d, %d, %d, %d", B, T, T_out, reduction_factor);
  if (d_alignments) {
    if (T_in < 1 || n_steps < 1) return fail(TACO_ERR_ARG, "T_in and n_steps must be >= 1, got %d, %d", T_in, n_steps);
    if ((long long)n_steps * reduction_factor != T)
      return fail(TACO_ERR_ARG, "T = %d is not n_steps * reduction_factor = %d * %d", T, n_steps, reduction_factor);
  } else {
    if (d_token_stretch) return fail(TACO_ERR_ARG, "d_token_stretch needs d_alignments: without them no frame has a token");
    if (d_token_frames) return fail(TACO_ERR_ARG, "d_token_frames needs d_alignments: without them no frame has a token");
    T_in = n_steps = 1;                                           // not used below; the byte counts of absent buffers stay defined
  }
  if ((uintptr_t)d_workspace & 7) return fail(TACO_ERR_ARG, "d_workspace must be 8-byte aligned");
  const size_t need = taco_spec_warp_workspace_bytes(B, T);
  const u128 nb = (u128)(unsigned)B, nmap = nb * (unsigned)T_out * sizeof(int32_t), ntok = nb * (unsigned)T_in * sizeof(int32_t);
  TRY(no_overlap({{d_src, nmap, "d_src"}, {d_frac, nmap, "d_frac"}, {d_out_frames, nb * sizeof(int32_t), "d_out_frames"},
                  {d_token_frames, ntok, "d_token_frames"}, {d_workspace, (u128)need, "d_workspace"},       // five outputs, then four inputs
                  {d_alignments, nb * (unsigned)T_in * (unsigned)n_steps * sizeof(float), "d_alignments"},
                  {d_frames, nb * sizeof(int32_t), "d_frames"}, {d_row_stretch, nb * sizeof(float), "d_row_stretch"},
                  {d_token_stretch, ntok, "d_token_stretch"}}, 5));
  if (workspace_bytes < need)
    return fail(TACO_ERR_STATE, "workspace of %zu bytes, taco_spec_warp_workspace_bytes asks for %zu", workspace_bytes, need);
  long long* C = (long long*)d_workspace;
  hipLaunchKernelGGL(k_warp_map, dim3((unsigned)B), dim3(WM_NT), 0, (hipStream_t)hip_stream, d_alignments, d_frames, d_row_stretch, d_token_stretch,
                     T_in, n_steps, reduction_factor, T, T_out, d_src, d_frac, d_out_frames, d_token_frames, C, (int*)(C + (size_t)B * T));
  HIPCHK(hipGetLastError());
  return 0;
}

// direct: the frequency gather reads the source rows from the cache at every width (taco_debug_spec_warp_direct: the benchmark and one equality test)
static int spec_warp(void* hip_stream, const float* d_spec, const int32_t* d_frames, const int32_t* d_src, const int32_t* d_frac,
                     const int32_t* d_out_frames, const float* d_freq_scale, int B, int T, int W, int T_out, float* d_out, bool direct) {
  if (!d_spec || !d_src || !d_frac || !d_out_frames || !d_out) return fail(TACO_ERR_ARG, "null pointer");
  if (B < 1 || T < 1 || W < 1 || T_out < 1) return fail(TACO_ERR_ARG, "B, T, W and T_out must be >= 1, got %d, %d, %d, %d", B, T, W, T_out);
  if (W >= (1 << 24)) return fail(TACO_ERR_UNSUPPORTED, "W = %d: a bin index must be exact in fp32 (below 2^24)", W);
  const u128 nb = (u128)(unsigned)B, nmap = nb * (unsigned)T_out * sizeof(int32_t);
  TRY(no_overlap({{d_out, nb * (unsigned)T_out * (unsigned)W * sizeof(float), "d_out"}, {d_spec, nb * (unsigned)T * (unsigned)W * sizeof(float), "d_spec"},
                  {d_frames, nb * sizeof(int32_t), "d_frames"}, {d_src, nmap, "d_src"}, {d_frac, nmap, "d_frac"},
                  {d_out_frames, nb * sizeof(int32_t), "d_out_frames"}, {d_freq_scale, nb * sizeof(float), "d_freq_scale"}}, 1));
  const int groups = cdiv(T_out, SW_ROWS);
  const long long total = (long long)B * groups;
  const dim3 grid((unsigned)std::min(total, SW_MAXGRID)), block(SW_NT);
  const int mode = !d_freq_scale ? 0 : (direct || W > SW_STAGE_W) ? 1 : 2;
  const auto kernel = mode == 0 ? k_spec_warp<0> : mode == 1 ? k_spec_warp<1> : k_spec_warp<2>;
  const size_t lds = mode == 2 ? (size_t)(SW_NT / 64) * (W + 1) * sizeof(float) : 0;                     // at most 32 KB: no attribute to set
  hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)hip_stream, d_spec, d_frames, d_src, d_frac, d_out_frames, d_freq_scale, T, W, T_out,
                     groups, total, d_out);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_spec_warp(void* hip_stream, const float* d_spec, const int32_t* d_frames, const int32_t* d_src, const int32_t* d_frac,
                   const int32_t* d_out_frames, const float* d_freq_scale, int B, int T, int W, int T_out, float* d_out) {
  return spec_warp(hip_stream, d_spec, d_frames, d_src, d_frac, d_out_frames, d_freq_scale, B, T, W, T_out, d_out, false);
}

int taco_debug_spec_warp_direct(void* hip_stream, const float* d_spec, const int32_t* d_frames, const int32_t* d_src, const int32_t* d_frac,
                                const int32_t* d_out_frames, const float* d_freq_scale, int B, int T, int W, int T_out, float* d_out) {
  return spec_warp(hip_stream, d_spec, d_frames, d_src, d_frac, d_out_frames, d_freq_scale, B, T, W, T_out, d_out, true);
}

int taco_debug_warp_info(int* out, int n) {
  if (!out || n < 0) return fail(TACO_ERR_ARG, "null pointer or negative count");
  const int v[4] = {WM_NT, 64, SW_ROWS, SW_STAGE_W};
  for (int k = 0; k < n && k < 4; ++k) out[k] = v[k];
  return 0;
}
