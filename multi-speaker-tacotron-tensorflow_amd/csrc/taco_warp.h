// taco_warp.h -- rate, per-token duration and pitch control on the spectrogram the forward produced, before any vocoder runs.  Not in
// the reference: its synthesizer says a sentence at the speed and pitch the model chose.  The forward gives a MAGNITUDE spectrogram
// (normalised dB) and Griffin-Lim invents the phase afterwards, so speed is a resampling of the frame axis and pitch a resampling of the
// bin axis; there are no phases to keep coherent.  The alignments attribute every decoder step to an input token, so the stretch can
// differ per token.  Included from taco_lib.hip; the definition is in include/taco_abi.h and, as NumPy, in tests/warp_reference.py.
//
// k_warp_map: one workgroup of WM_NT threads per batch row, one launch, integers throughout.
//   f = clamp(frames[b], 1, T).  tok(s) = argmax over e of alignments[b, e, s]: the first maximum wins, a NaN counts as the maximum and the
//   first NaN wins (ma_wins of taco_kernels.h, the rule of k_manual_alignments); lanes own consecutive s, so the loads along e are
//   coalesced, as in k_attention_trim, and the four waves take a quarter of the tokens each, their bests meeting in LDS (the loads are
//   round trips to memory: four times as many are in flight).  Source frame t < f belongs to step t / r; its duration in units of 2^-16 output frame is
//   d_t = clamp(lrint(fp32(row_stretch[b] * token_stretch[b, tok(t / r)]) * 65536), 2^12, 2^20), 2^12 for a NaN or a non-positive product.
//   C_t = d_0 + .. + d_t in int64 (C_-1 = 0): chunks of WM_NT frames, a shuffle scan per wave, the waves' totals through LDS, the carry
//   of the chunks before in a register; integer sums are associative, so the shape of the scan does not show in the bits.  C lives in
//   the workspace, T is not bounded by the LDS.  out_frames = clamp((C_{f-1} + 2^15) >> 16, 1, T_out).  Output frame j < out_frames sits
//   at tau = j << 16: src = the t with C_{t-1} <= tau < C_t (binary search), frac = ((tau - C_{src-1}) << 16) / d_src in [0, 65536).
//   j >= out_frames: src = f - 1, frac = 0.  token_frames[b, e] = the frames t < f of the steps with tok(s) == e: thread e walks the steps,
//   every element is written once, nothing is cleared beforehand.
//
// k_spec_warp: the gather and the two interpolations, one launch.  A wave owns an output row (b, j) at a time and its lanes run along k, so
// both source rows are read coalesced, once per output row; a workgroup takes SW_ROWS consecutive rows of one batch row, which mostly share
// their source rows (L1 / L2 serve the second reader).  THE ORDER IS: time first, then frequency, every operation rounded on its own
// (sw_lerp: nothing contracted) -- the bound of tests/test_gpu_warp.py is derived from this order:
//   t0 = src, t1 = min(t0 + 1, f - 1), w_t = frac * 2^-16 (exact);  v(k) = x[t0, k] if frac == 0 (the bits are copied: a NaN in the
//   next frame never leaks), else x[t0, k] + w_t * (x[t1, k] - x[t0, k]);  v(k) = +0 for k >= W.
//   no scale: out[j, k] = v(k).  scale c: q = fp32(k * c), k0 = (int)q, w_f = q - k0; out = v(k0) if w_f == 0, else
//   v(k0) + w_f * (v(k0 + 1) - v(k0)); a q that is not in [0, W) (a NaN or a negative c among them) gives +0.
// Rows j >= out_frames are +0; every element of out is written exactly once; no frame >= f of the input is read (src is clamped to
// [0, f - 1], frac to [0, 65535]: a garbage map gives a wrong picture, nothing worse).  The frequency gather has two forms that give
// the same bits: v(0 .. W) of the row staged once in the wave's own LDS and gathered from there (rows up to SW_STAGE_W bins; no workgroup
// barrier, a wave synchronises with itself), or the four values an output needs read straight from the cache (wider rows, and
// taco_debug_spec_warp_direct for the comparison).  DESIGN.md has the measurement the choice rests on.
#pragma once

#define WM_NT 256                         // threads of k_warp_map = frames of one scan chunk
#define WM_DMIN (1 << 12)                 // shortest and longest duration of a source frame, in 2^-16 output frame: 1/16 and 16
#define WM_DMAX (1 << 20)
#define SW_NT 256                         // threads of k_spec_warp: four waves, a row each at a time
#define SW_ROWS 8                         // output rows of one workgroup
#define SW_STAGE_W 2048                   // widest row the frequency gather stages in LDS (W + 1 floats a wave: 32 KB a workgroup at most)
#define SW_MAXGRID 0x7fffffffLL

__host__ __device__ static inline size_t wm_ws_row_bytes(int T) { return (size_t)T * (sizeof(long long) + sizeof(int)); }

// the duration of a frame whose stretches multiply to p (one correctly rounded fp32 product), in 2^-16 output frame
__device__ __forceinline__ int wm_duration(float p) {
  if (!(p > 0.f)) return WM_DMIN;                                 // NaN, zero, negative
  if (p >= 16.f) return WM_DMAX;                                  // (also keeps an infinity away from the conversion)
  const int d = (int)rintf(p * 65536.f);                          // an exact scaling, then round half to even like lrint
  return min(max(d, WM_DMIN), WM_DMAX);
}

__device__ __forceinline__ long long wm_shfl_up(long long v, int off) {
  const int lo = __shfl_up((int)(v & 0xffffffffLL), off, 64), hi = __shfl_up((int)(v >> 32), off, 64);
  return ((long long)hi << 32) | (unsigned int)lo;
}

__global__ __launch_bounds__(WM_NT) void k_warp_map(const float* __restrict__ align, const int* __restrict__ frames,
                                                    const float* __restrict__ row_stretch, const float* __restrict__ tok_stretch, int T_in,
                                                    int n_steps, int r, int T, int T_out, int* __restrict__ src, int* __restrict__ frac,
                                                    int* __restrict__ out_frames, int* __restrict__ tok_frames, long long* __restrict__ wsC,
                                                    int* __restrict__ wsTok) {
  __shared__ long long wtot[WM_NT / 64];
  __shared__ float wbest[WM_NT];
  __shared__ int warg[WM_NT];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = frames ? min(max(frames[b], 1), T) : T;
  long long* C = wsC + (size_t)b * T;                             // [T]: the inclusive prefix sums of the durations, the first f are used
  int* tok = wsTok + (size_t)b * T;                               // [n_steps <= T]: the token of every decoder step
  const int used = align ? (f + r - 1) / r : 0;                   // steps that own a frame t < f (T == n_steps * r: used <= n_steps)
  if (align) {
    const float* a = align + (size_t)b * T_in * n_steps;
    // 64 steps at a time, a lane each; the four waves share the tokens, a contiguous quarter each, and wave 0 takes the best of the four
    // (ma_wins is a total order -- greater value, then smaller index -- so the split does not show).  A wave whose quarter is empty holds
    // (-inf, INT_MAX), which loses to every real element: to -inf by its index, to a NaN by ma_beats.
    const int part = (T_in + WM_NT / 64 - 1) / (WM_NT / 64), e0 = min(wave * part, T_in), e1 = min(e0 + part, T_in);
    for (int s0 = 0; s0 < used; s0 += 64) {
      const int s = s0 + lane;
      float best = -INFINITY; int arg = INT_MAX;
      if (s < used) {
#pragma unroll 8
        for (int e = e0; e < e1; ++e) {                           // ascending e: the first maximum, the first NaN stays
          const float v = a[(size_t)e * n_steps + s];
          const bool take = ma_wins(v, e, best, arg);
          best = take ? v : best; arg = take ? e : arg;
        }
      }
      wbest[tid] = best; warg[tid] = arg;
      __syncthreads();
      if (wave == 0 && s < used) {
#pragma unroll
        for (int w = 1; w < WM_NT / 64; ++w) {
          const float ov = wbest[w * 64 + lane]; const int oa = warg[w * 64 + lane];
          const bool take = ma_wins(ov, oa, best, arg);
          best = take ? ov : best; arg = take ? oa : arg;
        }
        tok[s] = arg;                                             // wave 0's quarter holds token 0: arg is a real index
      }
      __syncthreads();                                            // the cells are free again; tok[], written to global memory, is read by all below
    }
    if (tok_frames)
      for (int e = tid; e < T_in; e += WM_NT) {
        int cnt = 0;
        for (int s = 0; s < used; ++s) cnt += tok[s] == e ? min(r, f - s * r) : 0;
        tok_frames[(size_t)b * T_in + e] = cnt;
      }
  }
  const float rs = row_stretch ? row_stretch[b] : 1.f;
  long long carry = 0;                                            // C of the last frame of the chunk before, the same in every thread
  for (int t0 = 0; t0 < f; t0 += WM_NT) {
    const int t = t0 + tid;
    long long inc = 0;
    if (t < f) inc = wm_duration(__fmul_rn(rs, tok_stretch ? tok_stretch[(size_t)b * T_in + tok[t / r]] : 1.f));
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long v = wm_shfl_up(inc, off);
      if (lane >= off) inc += v;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    long long before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < WM_NT / 64; ++w) {
      const long long v = wtot[w];
      if (w < wave) before += v;
      all += v;
    }
    if (t < f) C[t] = before + inc;
    carry += all;
    __syncthreads();                                              // wtot is free for the next chunk; after the last one C[] is complete
  }
  const long long of64 = (carry + (1 << 15)) >> 16;               // carry == C_{f-1}
  const int of = (int)min(max(of64, 1LL), (long long)T_out);
  if (tid == 0) out_frames[b] = of;
  for (int j = tid; j < T_out; j += WM_NT) {
    int s = f - 1, fr = 0;
    if (j < of) {
      // tau < C_{f-1}: j <= out_frames - 1 <= ((C_{f-1} + 2^15) >> 16) - 1, so tau = j << 16 <= C_{f-1} + 2^15 - 2^16 < C_{f-1}
      // (where the lower clamp raised out_frames to 1, j = 0 and tau = 0 < 2^12 <= C_0).  The search therefore ends inside [0, f).
      // (Four searches of a thread run side by side, a fixed number of steps each, were measured at the C2 shape: no faster, C sits in L1.)
      const long long tau = (long long)j << 16;
      int lo = 0, hi = f - 1;                                     // the smallest t with C_t > tau
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (C[mid] > tau) hi = mid; else lo = mid + 1;
      }
      const long long prev = lo > 0 ? C[lo - 1] : 0;
      s = lo;
      fr = (int)(((tau - prev) << 16) / (C[lo] - prev));
    }
    src[(size_t)b * T_out + j] = s;
    frac[(size_t)b * T_out + j] = fr;
  }
}

// a + w * (b - a), three fp32 operations rounded one by one.  (The _rn intrinsics are plain operators to this compiler and would be
// contracted into an fma under its default -ffp-contract=fast; the pragma is what keeps the product and the sum apart.)
__device__ __forceinline__ float sw_lerp(float a, float b, float w) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float p = w * d;
  return a + p;
}

// v(k) of the header: the time interpolation of bin k < W of one output row
__device__ __forceinline__ float sw_time(const float* __restrict__ x0, const float* __restrict__ x1, int k, bool copy, float wt) {
  const float a = x0[k];
  return copy ? a : sw_lerp(a, x1[k], wt);
}

// what a wave wrote to its part of the LDS, before its other lanes read it (and the other way round before the next row overwrites it)
__device__ __forceinline__ void sw_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// MODE 0: no frequency scale.  1: the scale, v(k0) and v(k0 + 1) formed from the source rows in the cache.  2: the scale, v(0 .. W) of the
// row staged once in the wave's own W + 1 floats of LDS (W <= SW_STAGE_W) and gathered from there.  1 and 2 give the same bits.
template <int MODE>
__global__ __launch_bounds__(SW_NT) void k_spec_warp(const float* __restrict__ spec, const int* __restrict__ frames, const int* __restrict__ src,
                                                     const int* __restrict__ frac, const int* __restrict__ out_frames,
                                                     const float* __restrict__ freq_scale, int T, int W, int T_out, int groups,
                                                     long long total, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float sw_lds[];
  constexpr bool SCALE = MODE != 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* vs = sw_lds + (size_t)wave * (W + 1);                    // MODE 2 only
  for (long long g = blockIdx.x; g < total; g += gridDim.x) {
    const int b = (int)(g / groups), j0 = (int)(g - (long long)b * groups) * SW_ROWS;
    const int f = frames ? min(max(frames[b], 1), T) : T;
    const int of = min(max(out_frames[b], 0), T_out);
    const float c = SCALE ? freq_scale[b] : 1.f;
    const float* xb = spec + (size_t)b * T * W;
    for (int j = j0 + wave; j < min(j0 + SW_ROWS, T_out); j += SW_NT / 64) {
      float* o = out + ((size_t)b * T_out + j) * W;
      if (j >= of) {
        for (int k = lane; k < W; k += 64) o[k] = 0.f;
        continue;
      }
      const int t0 = min(max(src[(size_t)b * T_out + j], 0), f - 1), t1 = min(t0 + 1, f - 1);
      const int fr = min(max(frac[(size_t)b * T_out + j], 0), 65535);
      const bool copy = fr == 0;
      const float wt = (float)fr * (1.f / 65536.f);
      const float* x0 = xb + (size_t)t0 * W;
      const float* x1 = copy ? x0 : xb + (size_t)t1 * W;          // (a copied row never touches its neighbour)
      if (!SCALE) {
#pragma unroll 4
        for (int k = lane; k < W; k += 64) o[k] = sw_time(x0, x1, k, copy, wt);
      } else if (MODE == 2) {
        for (int k = lane; k < W; k += 64) vs[k] = sw_time(x0, x1, k, copy, wt);
        if (lane == 0) vs[W] = 0.f;                               // v(W) = +0
        sw_wave_sync();
#pragma unroll 2
        for (int k = lane; k < W; k += 64) {
#pragma clang fp contract(off)                                    // q is the rounded product: w_f = q - k0 is no fma of k, c and k0
          const float q = (float)k * c;
          float res = 0.f;
          if (q >= 0.f && q < (float)W) {
            const int k0 = (int)q;
            const float wf = q - (float)k0;
            const float v0 = vs[k0];
            res = wf == 0.f ? v0 : sw_lerp(v0, vs[k0 + 1], wf);
          }
          o[k] = res;
        }
        sw_wave_sync();                                           // before the wave's next row overwrites vs[]
      } else {
#pragma unroll 2
        for (int k = lane; k < W; k += 64) {
#pragma clang fp contract(off)                                    // q is the rounded product: w_f = q - k0 is no fma of k, c and k0
          const float q = (float)k * c;
          float res = 0.f;
          if (q >= 0.f && q < (float)W) {                         // (W < 2^24 is checked by the caller: (float)W is exact)
            const int k0 = (int)q;
            const float wf = q - (float)k0;
            const float v0 = sw_time(x0, x1, k0, copy, wt);
            if (wf == 0.f) res = v0;
            else {
              const float v1 = k0 + 1 < W ? sw_time(x0, x1, k0 + 1, copy, wt) : 0.f;
              res = sw_lerp(v0, v1, wf);
            }
          }
          o[k] = res;
        }
      }
    }
  }
}
