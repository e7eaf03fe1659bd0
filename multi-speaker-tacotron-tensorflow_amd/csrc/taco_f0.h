// taco_f0.h -- pitch tracking on the GPU: the YIN estimator (de Cheveigne and Kawahara 2002, steps 2 to 5) per frame of a batch of
// waveforms, and F0 error statistics along a warping path.  Not in the reference: its synthesizer is judged by ear.  With the cepstral
// distortion of metrics.py these are the objective numbers of a synthesiser -- the spectral envelope, the intonation (F0 RMSE in cents)
// and the voicing decisions (V/UV error), the last two taken along the path taco_dtw_path produces.  Included from taco_lib.hip; the
// definition is in include/taco_abi.h and, as NumPy, in tests/yin_reference.py.
//
// k_yin<PLAIN>: a workgroup of YIN_NT threads takes `fpw` (at most YIN_FPW) consecutive frames of one row.  Neighbouring frames overlap
// by (frame - hop) samples -- four fifths at the model's framing -- so the workgroup stages ONE span of the row, zero outside [0, n),
// and frame f reads it from offset f * hop.  The frames are then worked one after the other by all threads:
//
//   difference function, d(tau) = sum_j (x[j] - x[j + tau])^2, tau = 0 .. tau_max + 1, the squares added by fmaf.  A lag per thread
//   walking j (the PLAIN form, kept for the benchmark and one equality test) reads two LDS words per multiply-add and runs at the LDS's
//   pace.  The blocked form gives a thread YIN_LB consecutive lags and a part of the j range: per YIN_JC values of j it loads x[j ..
//   j + JC) and the run x[j + tau0 .. j + tau0 + JC + LB - 1) once, 40 words, and makes JC * LB = 144 pairs out of registers.  Threads
//   next to each other own neighbouring lag blocks, so their runs start YIN_LB = 9 words apart: an odd stride, every ds_read_b32 of a
//   wave falls on 32 different banks (the x[j ..] words are one address per j part: a broadcast).  Where the lags need fewer than
//   YIN_NT blocks the j range is cut into P = YIN_NT / blocks parts so that no thread idles; the parts' sums go to LDS and are added
//   in the order p = 0 .. P - 1, one fixed order.  Lags past tau_max + 1 in the last block are computed and dropped.
//   Left alone, the compiler packs the pairs of the unrolled block two by two into v_pk_add_f32 / v_pk_fma_f32 -- no faster per element
//   on this chip than the plain forms -- with register shuffles and overlapping re-reads of the run around them (58 words read for the
//   40 needed, 103 registers).  Each difference and each running sum is therefore pinned (DX_PIN, an empty asm): the block compiles to
//   144 v_sub_f32 + 144 v_fmac_f32 behind 20 ds_read2_b32, in 87 registers.
//
//   a frame that read a NaN or an infinity is found by its own test of the W + tau_max + 1 words it reads, not through the sums.
//
// After the last frame wave w finishes frame w from its d() in LDS, with no further workgroup barrier: lane l owns the lags
// [l * C, (l + 1) * C), C = ceil((tau_max + 2) / 64); S(tau) is the lane's running sum on top of a wave scan of the lanes' totals
// (shuffles; the exclusive value is the left lane's inclusive one, no subtraction), d'(tau) replaces d(tau) in place; the first lag
// under the threshold is each lane's first, minimised over the wave (dx_allmax of taco_xchg.h on the negated index), the argmin of
// the unvoiced case a (value, index) butterfly; the descent and the parabola are a few dependent steps every lane repeats.  Product,
// quotient and each operation of the parabola are _rn intrinsics: the compiler contracts nothing there.
//
// k_f0_path_stats: one workgroup per pair, thread t takes the path entries t, t + NT, ...; the four partial results are added by one
// LDS tree.  No atomics in either kernel: two calls give the same bits.
#pragma once

#define YIN_NT 256                        // threads of k_yin
#define YIN_FPW 4                         // frames of one workgroup = its waves: wave w finishes frame w
#define YIN_LB 9                          // lags of a thread's block (odd: neighbouring threads' runs start on different LDS banks)
#define YIN_JC 16                         // values of j per register block
#define YIN_FRAME_MAX 8192                // W + tau_max + 2 at most: with its lag sums and their parts a frame stays below YIN_LDS_FLOATS
#define YIN_LDS_FLOATS 36864              // 144 KB of the 160 KB of a CU
#define YIN_MAXGRID 65536                 // workgroups of either kernel; they loop over the work beyond
#define F0S_NT 256                        // threads of k_f0_path_stats

struct YinPlan {
  int NL, nblk, NLP, P, JP, fpw;          // lags, lag blocks, lags padded to whole blocks, j parts, j per part, frames per workgroup
  long long lds_floats;
};
// where the pieces of a workgroup's LDS start (floats): the span at 0, the parts' sums, d() of every frame
__host__ __device__ static inline int yin_span(int fpw, int hop, int W, int NLP) { return (fpw - 1) * hop + W + NLP - 1; }
__host__ __device__ static inline int yin_part_off(int span) { return (span + 3) & ~3; }

// host: the layout for a frame of W + tau_max + 2 <= YIN_FRAME_MAX floats (checked by the caller)
static YinPlan yin_plan(int W, int tau_max, int hop) {
  YinPlan p;
  p.NL = tau_max + 2;
  p.nblk = (p.NL + YIN_LB - 1) / YIN_LB;
  p.NLP = p.nblk * YIN_LB;
  p.P = p.nblk < YIN_NT ? YIN_NT / p.nblk : 1;
  p.JP = (W + p.P - 1) / p.P;
  p.fpw = 1;
  for (int f = YIN_FPW; f >= 1; --f) {
    const long long span = (long long)(f - 1) * hop + W + p.NLP - 1;
    const long long tot = ((span + 3) & ~3LL) + (long long)p.P * p.NLP + (long long)f * p.NLP;
    if (tot <= YIN_LDS_FLOATS || f == 1) { p.fpw = f; p.lds_floats = tot; break; }
  }
  return p;
}

__device__ __forceinline__ bool yin_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

template <bool PLAIN>
__global__ __launch_bounds__(YIN_NT) void k_yin(const float* __restrict__ wav, const int* __restrict__ num, int B, int L, int F, int hop, int W,
                                                int tau_min, int tau_max, float srf, float thr, int fpw, float* __restrict__ f0,
                                                float* __restrict__ aper, int* __restrict__ lag) {
  extern __shared__ __attribute__((aligned(16))) float yin_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NL = tau_max + 2, nblk = (NL + YIN_LB - 1) / YIN_LB, NLP = nblk * YIN_LB;
  const int P = nblk < YIN_NT ? YIN_NT / nblk : 1, JP = (W + P - 1) / P;
  float* xs = yin_lds;                                          // the span: frame f starts at xs + f * hop
  float* part = xs + yin_part_off(yin_span(fpw, hop, W, NLP));  // [P][NLP]: d() of the frame in work, by j part
  float* dl = part + P * NLP;                                   // [fpw][NLP]: d(), then d'()
  const int groups = (F + fpw - 1) / fpw;
  const long long total = (long long)B * groups;
  for (long long g = blockIdx.x; g < total; g += gridDim.x) {
    const int b = (int)(g / groups), t0 = (int)(g - (long long)b * groups) * fpw;
    const int n = num ? min(max(num[b], 0), L) : L;
    const int cnt = min(fpw, F - t0);                           // columns of this group
    const int live = max(0, min(cnt, 1 + n / hop - t0));        // of them the row's own frames
    const size_t o0 = (size_t)b * F + t0;
    if (tid >= live && tid < cnt) {                             // columns past the row's frames
      f0[o0 + tid] = 0.f;
      if (aper) aper[o0 + tid] = 0.f;
      if (lag) lag[o0 + tid] = 0;
    }
    if (live == 0) continue;
    const long long g0 = (long long)t0 * hop - (W + tau_max) / 2;
    const int need = yin_span(live, hop, W, NLP);
    const float* row = wav + (size_t)b * L;
    for (int p = tid; p < need; p += YIN_NT) {
      const long long s = g0 + p;
      xs[p] = (s >= 0 && s < n) ? row[s] : 0.f;
    }
    __syncthreads();
    unsigned badmask = 0;
    for (int f = 0; f < live; ++f) {
      const float* x = xs + f * hop;
      bool bad = false;
      for (int k = tid; k <= W + tau_max; k += YIN_NT) bad = bad || !yin_finite(x[k]);
      if (PLAIN) {
        for (int tau = tid; tau < NL; tau += YIN_NT) {
          float acc = 0.f;
          for (int j = 0; j < W; ++j) {
            const float df = x[j] - x[j + tau];
            acc = fmaf(df, df, acc);
          }
          dl[f * NLP + tau] = acc;
        }
      } else {
        for (int item = tid; item < nblk * P; item += YIN_NT) {
          const int p = item / nblk, tau0 = (item - p * nblk) * YIN_LB;
          const int je = min(W, p * JP + JP);
          const float* xa = x + tau0;
          float acc[YIN_LB];
#pragma unroll
          for (int l = 0; l < YIN_LB; ++l) acc[l] = 0.f;
          int j = p * JP;
          for (; j + YIN_JC <= je; j += YIN_JC) {
            float a[YIN_JC], w[YIN_JC + YIN_LB - 1];
#pragma unroll
            for (int c = 0; c < YIN_JC; ++c) a[c] = x[j + c];
#pragma unroll
            for (int r = 0; r < YIN_JC + YIN_LB - 1; ++r) w[r] = xa[j + r];
#pragma unroll
            for (int c = 0; c < YIN_JC; ++c)
#pragma unroll
              for (int l = 0; l < YIN_LB; ++l) {
                float df = a[c] - w[c + l];
                DX_PIN(df);                                     // one v_sub, one v_fmac per pair: the note on packed forms above
                acc[l] = fmaf(df, df, acc[l]);
                DX_PIN(acc[l]);
              }
          }
          for (; j < je; ++j) {
            const float a = x[j];
#pragma unroll
            for (int l = 0; l < YIN_LB; ++l) {
              const float df = a - xa[j + l];
              acc[l] = fmaf(df, df, acc[l]);
            }
          }
#pragma unroll
          for (int l = 0; l < YIN_LB; ++l) part[p * NLP + tau0 + l] = acc[l];
        }
      }
      if (__syncthreads_or(bad ? 1 : 0)) badmask |= 1u << f;    // also: the parts are written
      if (!PLAIN) {
        for (int tau = tid; tau < NL; tau += YIN_NT) {
          float s = part[tau];
          for (int p = 1; p < P; ++p) s += part[p * NLP + tau];
          dl[f * NLP + tau] = s;
        }
        __syncthreads();                                        // the parts are free for the next frame; after the last one, d() is complete
      }
    }
    if (wave < live) {                                          // wave w finishes frame w
      float* d = dl + wave * NLP;
      const int C = (NL + 63) / 64, k0 = lane * C, k1 = min(NL, k0 + C);
      float loc = 0.f;
      for (int k = max(k0, 1); k < k1; ++k) loc += d[k];
      float inc = loc;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const float v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
      }
      float S = __shfl_up(inc, 1, 64);                          // the lanes to the left: S(k0 - 1)
      if (lane == 0) S = 0.f;
      const int lo = max(k0, tau_min), hi = min(k1 - 1, tau_max);      // the lane's share of the search range
      float first = __builtin_inff(), best = __builtin_inff();
      int besti = 0x7fffffff;
      for (int k = k0; k < k1; ++k) {
        float dp = 1.f;
        if (k > 0) {
          const float dk = d[k];
          S += dk;
          if (S != 0.f) dp = __fdiv_rn(__fmul_rn(dk, (float)k), S);
        }
        d[k] = dp;
        if (k >= lo && k <= hi) {
          if (dp < thr && first == __builtin_inff()) first = (float)k;
          if (dp < best) { best = dp; besti = k; }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");    // d'() of every lane, read below by all of them
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      first = -dx_allmax(-first);                               // lags are far below 2^24: exact as floats
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(besti, off, 64);
        if (ov < best || (ov == best && oi < besti)) { best = ov; besti = oi; }
      }
      const bool voiced = first != __builtin_inff();
      int tau = voiced ? (int)first : besti;
      tau = min(max(tau, tau_min), tau_max);                    // (an all-NaN d'() leaves no argmin: stay inside the array)
      if (voiced)
        while (tau + 1 <= tau_max && d[tau + 1] < d[tau]) ++tau;
      if (lane == 0) {
        const float y0 = d[tau - 1], y1 = d[tau], y2 = d[tau + 1];
        const float q = __fadd_rn(__fsub_rn(y0, __fmul_rn(2.f, y1)), y2);
        float delta = 0.f;
        if (q > 0.f) delta = fminf(fmaxf(__fdiv_rn(__fmul_rn(0.5f, __fsub_rn(y0, y2)), q), -0.5f), 0.5f);
        const bool isbad = (badmask >> wave & 1u) != 0;
        const float nanv = __builtin_nanf("");
        f0[o0 + wave] = isbad ? nanv : (voiced ? __fdiv_rn(srf, __fadd_rn((float)tau, delta)) : 0.f);
        if (aper) aper[o0 + wave] = isbad ? nanv : y1;
        if (lag) lag[o0 + wave] = isbad ? -1 : tau;
      }
    }
    __syncthreads();                                            // before the next group's span overwrites this one
  }
}

__global__ __launch_bounds__(F0S_NT) void k_f0_path_stats(const float* __restrict__ fa, int Fa, const float* __restrict__ fb, int Fb,
                                                          const int* __restrict__ path, const int* __restrict__ path_len, int B, int cap,
                                                          float* __restrict__ stats) {
  __shared__ float sh_s[F0S_NT];
  __shared__ int sh_n[3][F0S_NT];
  const int tid = threadIdx.x;
  for (long long p = blockIdx.x; p < B; p += gridDim.x) {
    const int n = min(max(path_len[p], 0), cap);
    const int* e = path + (size_t)p * cap * 2;
    const float* a = fa + (size_t)p * Fa;
    const float* bq = fb + (size_t)p * Fb;
    float s = 0.f;
    int both = 0, vuv = 0, used = 0;
    bool bad = false;
    for (int k = tid; k < n; k += F0S_NT) {
      const int i = e[2 * k], j = e[2 * k + 1];
      if (i < 0 || i >= Fa || j < 0 || j >= Fb) continue;
      const float va = a[i], vb = bq[j];
      ++used;
      if (va != va || vb != vb) { bad = true; continue; }
      const bool ua = va > 0.f, ub = vb > 0.f;
      if (ua && ub) {
        const float c = __fmul_rn(1200.f, log2f(__fdiv_rn(va, vb)));
        s = __fadd_rn(s, __fmul_rn(c, c));
        ++both;
      } else if (ua != ub) {
        ++vuv;
      }
    }
    sh_s[tid] = s; sh_n[0][tid] = both; sh_n[1][tid] = vuv; sh_n[2][tid] = used;
    const int anybad = __syncthreads_or(bad ? 1 : 0);
    for (int h = F0S_NT / 2; h > 0; h >>= 1) {
      if (tid < h) {
        sh_s[tid] = __fadd_rn(sh_s[tid], sh_s[tid + h]);
        sh_n[0][tid] += sh_n[0][tid + h]; sh_n[1][tid] += sh_n[1][tid + h]; sh_n[2][tid] += sh_n[2][tid + h];
      }
      __syncthreads();
    }
    if (tid == 0) {
      float* o = stats + (size_t)p * 4;
      o[0] = anybad ? __builtin_nanf("") : sh_s[0];
      o[1] = (float)sh_n[0][0]; o[2] = (float)sh_n[1][0]; o[3] = (float)sh_n[2][0];
    }
    __syncthreads();                                            // the tree's cells, before the next pair fills them
  }
}

// host: one launch of k_yin<PLAIN> on st
template <bool PLAIN>
static int yin_launch(hipStream_t st, const YinPlan& pl, const float* d_wav, const int32_t* d_num, int B, int L, int F, int hop, int W,
                      int tau_min, int tau_max, float srf, float thr, float* d_f0, float* d_aper, int32_t* d_lag) {
  const size_t lds = (size_t)pl.lds_floats * sizeof(float);
  // More than 64 KB of dynamic LDS has to be asked for (on the current device, which is the stream's: include/taco_abi.h).  Only long
  // frames or long hops get there -- the model's framing takes 24 KB -- and those calls ask every time: no state is kept between calls.
  if (lds > 64 * 1024)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_yin<PLAIN>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(YIN_LDS_FLOATS * sizeof(float))));
  const long long total = (long long)B * ((F + pl.fpw - 1) / pl.fpw);
  hipLaunchKernelGGL(k_yin<PLAIN>, dim3((unsigned)std::min<long long>(total, YIN_MAXGRID)), dim3(YIN_NT), lds, st, d_wav, d_num, B, L, F, hop, W,
                     tau_min, tau_max, srf, thr, pl.fpw, d_f0, d_aper, d_lag);
  HIPCHK(hipGetLastError());
  return 0;
}
