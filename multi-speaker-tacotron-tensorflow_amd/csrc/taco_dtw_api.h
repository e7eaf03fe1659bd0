// taco_dtw_api.h -- C ABI of dynamic time warping (kernels in taco_dtw.h); included inside extern "C".

// the boundary column of a strip for every pair; nothing when one strip covers Tb.  0 for sizes taco_dtw refuses.
size_t taco_dtw_workspace_bytes(int B, int Ta, int Tb, int D) {
  if (B < 1 || Ta < 1 || Tb < 1 || D < 1) return 0;
  return Tb > DTW_STRIP ? (size_t)B * (size_t)Ta * sizeof(float) : 0;
}

int taco_dtw(void* hip_stream, const float* d_a, const int32_t* d_len_a, const float* d_b, const int32_t* d_len_b, int B, int Ta, int Tb, int D,
             int cost_kind, float* d_dist, float* d_total, uint8_t* d_dir, void* d_workspace, size_t workspace_bytes) {
  if (!d_a || !d_b || !d_dist) return fail(TACO_ERR_ARG, "null pointer");
  if (B < 1 || Ta < 1 || Tb < 1 || D < 1) return fail(TACO_ERR_ARG, "B, Ta, Tb and D must be >= 1, got %d, %d, %d, %d", B, Ta, Tb, D);
  if (cost_kind != 0 && cost_kind != 1) return fail(TACO_ERR_ARG, "cost_kind = %d: accepted are 0 (mean absolute) and 1 (Euclidean)", cost_kind);
  const size_t need = taco_dtw_workspace_bytes(B, Ta, Tb, D);
  if (need && !d_workspace) return fail(TACO_ERR_ARG, "null workspace");
  const u128 nb = (u128)(unsigned)B;
  TRY(no_overlap({{d_dist, nb * sizeof(float), "d_dist"}, {d_total, nb * sizeof(float), "d_total"}, {d_dir, nb * (unsigned)Ta * (unsigned)Tb, "d_dir"},
                  {d_workspace, (u128)need, "d_workspace"},                                                        // four outputs, then four inputs
                  {d_a, nb * (unsigned)Ta * (unsigned)D * sizeof(float), "d_a"}, {d_b, nb * (unsigned)Tb * (unsigned)D * sizeof(float), "d_b"},
                  {d_len_a, nb * sizeof(int32_t), "d_len_a"}, {d_len_b, nb * sizeof(int32_t), "d_len_b"}}, 4));
  if (D > DTW_DMAX) return fail(TACO_ERR_UNSUPPORTED, "D = %d: taco_dtw keeps a column's features in registers, up to D = %d", D, DTW_DMAX);
  if (workspace_bytes < need) return fail(TACO_ERR_STATE, "workspace of %zu bytes, taco_dtw_workspace_bytes asks for %zu", workspace_bytes, need);
  hipStream_t st = (hipStream_t)hip_stream;
  float* seam = need ? (float*)d_workspace : nullptr;
#define DTW_CASE(DP) \
  case DP: return dtw_launch<DP>(st, d_a, d_len_a, d_b, d_len_b, B, Ta, Tb, D, cost_kind, d_dist, d_total, d_dir, seam);
  switch (rup(D, DTW_DSTEP)) {
    DTW_CASE(16) DTW_CASE(32) DTW_CASE(48) DTW_CASE(64) DTW_CASE(80) DTW_CASE(96) DTW_CASE(112) DTW_CASE(128)
  }
#undef DTW_CASE
  return fail(TACO_ERR_UNSUPPORTED, "D = %d has no instantiation", D);
}

int taco_dtw_path(void* hip_stream, const uint8_t* d_dir, const int32_t* d_len_a, const int32_t* d_len_b, int B, int Ta, int Tb, int32_t* d_path,
                  int32_t* d_path_len) {
  if (!d_dir || !d_path || !d_path_len) return fail(TACO_ERR_ARG, "null pointer");
  if (B < 1 || Ta < 1 || Tb < 1) return fail(TACO_ERR_ARG, "B, Ta and Tb must be >= 1, got %d, %d, %d", B, Ta, Tb);
  const u128 nb = (u128)(unsigned)B;
  TRY(no_overlap({{d_path, nb * ((u128)(unsigned)Ta + (unsigned)Tb - 1) * 2 * sizeof(int32_t), "d_path"}, {d_path_len, nb * sizeof(int32_t), "d_path_len"},
                  {d_dir, nb * (unsigned)Ta * (unsigned)Tb, "d_dir"},                                              // two outputs, then three inputs
                  {d_len_a, nb * sizeof(int32_t), "d_len_a"}, {d_len_b, nb * sizeof(int32_t), "d_len_b"}}, 2));
  hipLaunchKernelGGL(k_dtw_path, dim3((unsigned)std::min(B, DTW_MAXGRID)), dim3(64), 0, (hipStream_t)hip_stream, d_dir, d_len_a, d_len_b, B, Ta, Tb,
                     d_path, d_path_len);
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_debug_dtw_info(int* out, int n) {
  if (!out || n < 0) return fail(TACO_ERR_ARG, "null pointer or negative count");
  const int v[6] = {DTW_STRIP, DTW_CH, DTW_DMAX, DTW_DSTEP, 64 * DTW_COLS, DTW_ROWS};
  for (int k = 0; k < n && k < 6; ++k) out[k] = v[k];
  return 0;
}
