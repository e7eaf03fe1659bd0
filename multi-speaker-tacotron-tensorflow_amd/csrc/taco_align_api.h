// taco_align_api.h -- C ABI of matching recognised text to script lines (kernels in taco_align.h); included inside extern "C".

// cols: 0 = the one-column kernel for len(b) <= 64 and the four-column one above; TA_WIDE = the four-column kernel for every length
static int ta_matches(void* hip_stream, const int32_t* d_chars, long long n_chars, const int32_t* d_offsets, int n_texts, const int32_t* d_pairs,
                      int n_pairs, int32_t* d_matches, int cols) {
  if (!d_offsets || !d_pairs || !d_matches || (!d_chars && n_chars != 0)) return fail(TACO_ERR_ARG, "null pointer");
  if (n_chars < 0 || n_texts < 0 || n_pairs < 0)
    return fail(TACO_ERR_ARG, "n_chars, n_texts and n_pairs must be >= 0, got %lld, %d, %d", n_chars, n_texts, n_pairs);
  if (cols != 0 && cols != TA_WIDE) return fail(TACO_ERR_ARG, "cols = %d: accepted are 0 (by length) and %d", cols, TA_WIDE);
  TRY(no_overlap({{d_matches, (u128)(unsigned)n_pairs * sizeof(int32_t), "d_matches"},
                  {d_chars, (u128)(unsigned long long)n_chars * sizeof(int32_t), "d_chars"},
                  {d_offsets, ((u128)(unsigned)n_texts + 1) * sizeof(int32_t), "d_offsets"},
                  {d_pairs, (u128)(unsigned)n_pairs * 2 * sizeof(int32_t), "d_pairs"}}, 1));
  if (n_pairs == 0) return 0;
  const dim3 grid((unsigned)cdiv(n_pairs, TA_WAVES)), block(TA_WAVES * 64);
  hipStream_t st = (hipStream_t)hip_stream;
  if (cols == 0) {
    hipLaunchKernelGGL(k_text_matches<1>, grid, block, 0, st, d_chars, n_chars, d_offsets, n_texts, d_pairs, n_pairs, d_matches, 0, 64);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_text_matches<TA_WIDE>, grid, block, 0, st, d_chars, n_chars, d_offsets, n_texts, d_pairs, n_pairs, d_matches, 65, TA_BMAX);
  } else {
    hipLaunchKernelGGL(k_text_matches<TA_WIDE>, grid, block, 0, st, d_chars, n_chars, d_offsets, n_texts, d_pairs, n_pairs, d_matches, 0, TA_BMAX);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int taco_text_matches(void* hip_stream, const int32_t* d_chars, long long n_chars, const int32_t* d_offsets, int n_texts, const int32_t* d_pairs,
                      int n_pairs, int32_t* d_matches) {
  return ta_matches(hip_stream, d_chars, n_chars, d_offsets, n_texts, d_pairs, n_pairs, d_matches, 0);
}

int taco_debug_text_matches_cols(void* hip_stream, const int32_t* d_chars, long long n_chars, const int32_t* d_offsets, int n_texts,
                                 const int32_t* d_pairs, int n_pairs, int32_t* d_matches, int cols) {
  return ta_matches(hip_stream, d_chars, n_chars, d_offsets, n_texts, d_pairs, n_pairs, d_matches, cols);
}

int taco_text_best_two(void* hip_stream, const int32_t* d_matches, const int32_t* d_pairs, const int32_t* d_offsets, int n_texts,
                       const int32_t* d_group_offsets, int n_groups, int32_t* d_best) {
  if (!d_matches || !d_pairs || !d_offsets || !d_group_offsets || !d_best) return fail(TACO_ERR_ARG, "null pointer");
  if (n_texts < 0 || n_groups < 0) return fail(TACO_ERR_ARG, "n_texts and n_groups must be >= 0, got %d, %d", n_texts, n_groups);
  // the pair count is not an argument: of d_matches and d_pairs the first element is what can be checked
  TRY(no_overlap({{d_best, (u128)(unsigned)n_groups * 4 * sizeof(int32_t), "d_best"},
                  {d_offsets, ((u128)(unsigned)n_texts + 1) * sizeof(int32_t), "d_offsets"},
                  {d_group_offsets, ((u128)(unsigned)n_groups + 1) * sizeof(int32_t), "d_group_offsets"},
                  {d_matches, sizeof(int32_t), "d_matches"}, {d_pairs, 2 * sizeof(int32_t), "d_pairs"}}, 1));
  if (n_groups == 0) return 0;
  hipLaunchKernelGGL(k_text_best_two, dim3((unsigned)cdiv(n_groups, TA_WAVES)), dim3(TA_WAVES * 64), 0, (hipStream_t)hip_stream, d_matches, d_pairs,
                     d_offsets, n_texts, d_group_offsets, n_groups, d_best);
  HIPCHK(hipGetLastError());
  return 0;
}
