// taco_envelope.h -- the spectral envelope of every frame of a log-magnitude spectrogram, and the pitch / formant shift that rests on it.
// Not in the reference.  The model's linear output is normalised dB, affine in log|D|, so the real cepstrum of a frame is a DCT-I of the
// frame and its envelope the low-quefrency part of it: with M = W - 1 and Q coefficients kept,
//     c_n = sum_k A[n, k] v_k,   env_k = sum_n S[n, k] c_n,   e_k = v_k - env_k        (A, S: the two fp32 tables of taco_envelope_create)
// -- two small dense products per frame, [R, W] x [W, Q] and [R, Q] x [Q, W] over a tile of R frames.  Included from taco_lib.hip; the
// definition is in include/taco_abi.h and, as NumPy, in tests/envelope_reference.py.
//
// Both products run on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32 (a k-ordered fp32 fma chain: the bound of
// tests/test_gpu_envelope.py is an fp32 bound in any order), which leaves the VALU to the interpolations.  One workgroup of EV_NT threads
// (eight waves) owns EV_ROWS whole frames -- EV_ROWS_WIDE of them where W > EV_W16, the rows above staying zero in the 16-row tile --:
//   1. stage v [R, W] in LDS: the frames themselves (k_spec_envelope) or taco_spec_warp's time interpolation of them, to the bit
//      (k_spec_warp_formant: sw_time of taco_warp.h); a wave takes a row at a time, its lanes run along k.  Bins W .. WP (W rounded up to 16)
//      are zero, and so are rows that are not live (t >= f, j >= out_frames, past the last row).
//   2. analysis: the sum over k is cut into groups of 16 bins, the waves take the groups in turn; lane (i, g) of a wave holds frame i and,
//      in step s of a group, bin 16 * group + 4 g + s -- the order of a sum is the kernel's to choose, and this one makes the operand of four
//      steps ONE 16-byte load: from row n of the table A [QP, WP] (Q and W rounded up to 16, zero filled) and from row i of v in LDS.  Every
//      wave holds QP / 16 accumulators, which are independent chains; the eight partial sums meet in LDS (in the array that will hold env)
//      and are added in the order of the waves: c [16, QP].
//   3. synthesis: the waves take the 16-bin tiles of the frame in turn, the sum over n in groups of 16 the same way, the table as
//      S^T [WP, QP].  The accumulator has the bin on the lane and four frames in its registers: env goes to LDS, e = v - env (one fp32
//      subtraction) over v in place.
//   4. k_spec_envelope writes env (and c) out, rows along k; k_spec_warp_formant gathers out[k] = G(env, formant)[k] + G(e, pitch)[k] with
//      the expressions of k_spec_warp (ev_gather), one fp32 addition.
// A tile with no live row skips 2 and 3.  No K split across workgroups, no atomics, no workspace: two calls give the same bits.
// The tables are read through L2 by every workgroup: 2 * QP * WP * 4 bytes (533 KB at W = 1025, Q = 49) against the 2 * R * W * 4 bytes
// of spectrogram a workgroup moves (131 KB at R = 16): DESIGN.md says why R is 16.
#pragma once

#define EV_NT 512                         // threads of both kernels: eight waves
#define EV_NW (EV_NT / 64)
#define EV_ROWS 16                        // frames of one workgroup = rows of the matrix tile
#define EV_ROWS_WIDE 8                    // frames of one workgroup where W > EV_W16: two arrays of 16 such rows do not fit the LDS
#define EV_TILE 16                        // v_mfma_f32_16x16x4_f32: 16 x 16 outputs,
#define EV_KSTEP 4                        // four terms of the sum an instruction
#define EV_W16 1152                       // the widest frame a workgroup takes 16 of
#define EV_MAX_W 2304                     // the widest frame at all: 2 * 8 * (2304 + 4) + 16 * (128 + 4) floats = 152.5 KB of the 160 KB
#define EV_MAX_Q 128

typedef float ev_f32x4 __attribute__((ext_vector_type(4)));

struct EvDims { int W, Q, WP, QP, LS, CS, R; };      // LS, CS: the row strides of v / env and of c in LDS, in floats

__host__ __device__ static inline EvDims ev_dims(int W, int Q) {
  EvDims d;
  d.W = W; d.Q = Q;
  d.WP = (W + 15) / 16 * 16; d.QP = (Q + 15) / 16 * 16;
  d.LS = d.WP + 4; d.CS = d.QP + 4;       // a multiple of 4 (16-byte operand reads) that is 4 mod 16 (the four frame groups of a tile store to different banks)
  d.R = W > EV_W16 ? EV_ROWS_WIDE : EV_ROWS;
  return d;
}
// floats of dynamic LDS: v, then env (which first holds the waves' partial sums [EV_NW, 16, QP]), then c [16, CS]
__host__ __device__ static inline size_t ev_second(const EvDims& d) {
  const size_t a = (size_t)d.R * d.LS, p = (size_t)EV_NW * EV_TILE * d.QP;
  return a > p ? a : p;
}
__host__ __device__ static inline size_t ev_lds_floats(const EvDims& d) { return (size_t)d.R * d.LS + ev_second(d) + (size_t)EV_TILE * d.CS; }

struct taco_envelope {
  int W = 0, Q = 0, device = 0;
  std::vector<float> A, S;       // host [Q, W] each, as taco_envelope_tables returns them
  float* d_tab = nullptr;        // device: A [QP, WP], then S^T [WP, QP], zero filled
  std::mutex mu;                 // guards the upload at first use
};

// G(y, c)[k] of include/taco_abi.h, the expressions of k_spec_warp: y is a row of W floats in LDS, y(W) = +0
__device__ __forceinline__ float ev_gather(const float* y, int k, float c, int W) {
#pragma clang fp contract(off)                                    // q is the rounded product: w_f = q - k0 is no fma of k, c and k0
  const float q = (float)k * c;
  float res = 0.f;
  if (q >= 0.f && q < (float)W) {
    const int k0 = (int)q;
    const float wf = q - (float)k0;
    const float v0 = y[k0];
    if (wf == 0.f) res = v0;
    else res = sw_lerp(v0, k0 + 1 < W ? y[k0 + 1] : 0.f, wf);
  }
  return res;
}

// Steps 2 and 3 of the header on the tile staged in va, NT = QP / 16 a template parameter (the accumulators are registers); all threads of the workgroup, which leave behind a barrier: c in cc [16, CS],
// env in vb [R, LS] (bins >= W: +0) and, where WANT_E, e over v in va.
template <int NT, bool WANT_E>
__device__ __forceinline__ void ev_tile(float* __restrict__ va, float* __restrict__ vb, float* __restrict__ cc, const float* __restrict__ tabA,
                                        const float* __restrict__ tabS, const EvDims d) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  {
    ev_f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = ev_f32x4{0.f, 0.f, 0.f, 0.f};
    const float* trow = tabA + (size_t)i * d.WP + 4 * g;          // table row n = 16 * tile + i, bins 16 * group + 4 g ..
    const size_t tstep = (size_t)EV_TILE * d.WP;
    for (int grp = wave; grp < d.WP / 16; grp += EV_NW) {
      const int k = grp * 16 + 4 * g;
      const ev_f32x4 a = i < d.R ? *reinterpret_cast<const ev_f32x4*>(va + (size_t)i * d.LS + k) : ev_f32x4{0.f, 0.f, 0.f, 0.f};
      ev_f32x4 b[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) b[n] = *reinterpret_cast<const ev_f32x4*>(trow + n * tstep + grp * 16);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[n][s], acc[n], 0, 0, 0);
    }
    float* part = vb + (size_t)wave * EV_TILE * d.QP;             // [16 frames, QP]: coefficient on the lane, four frames in the registers
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[(size_t)(4 * g + r) * d.QP + n * EV_TILE + i] = acc[n][r];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < EV_TILE * d.QP; idx += EV_NT) {
    float s = vb[idx];
#pragma unroll
    for (int w = 1; w < EV_NW; ++w) s += vb[(size_t)w * EV_TILE * d.QP + idx];
    cc[(size_t)(idx / d.QP) * d.CS + idx % d.QP] = s;
  }
  __syncthreads();                                                // c is whole, and the partial sums are read: vb may take env
  for (int t = wave; t < d.WP / EV_TILE; t += EV_NW) {
    ev_f32x4 acc = ev_f32x4{0.f, 0.f, 0.f, 0.f};
    const int col = t * EV_TILE + i;
    const float* srow = tabS + (size_t)col * d.QP + 4 * g;        // S^T row of bin col, coefficients 16 * group + 4 g ..
    const float* crow = cc + (size_t)i * d.CS + 4 * g;
#pragma unroll
    for (int grp = 0; grp < NT; ++grp) {
      const ev_f32x4 b = *reinterpret_cast<const ev_f32x4*>(srow + grp * 16);
      const ev_f32x4 a = *reinterpret_cast<const ev_f32x4*>(crow + grp * 16);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * g + r;
      if (row < d.R) {
        const bool in = col < d.W;
        const float env = in ? acc[r] : 0.f;
        vb[(size_t)row * d.LS + col] = env;
        if (WANT_E) {
          float* p = va + (size_t)row * d.LS + col;
          *p = in ? *p - env : 0.f;
        }
      }
    }
  }
  __syncthreads();
}

template <int NT>
__global__ __launch_bounds__(EV_NT) void k_spec_envelope(const float* __restrict__ spec, const int* __restrict__ frames,
                                                         const float* __restrict__ tabA, const float* __restrict__ tabS, int T, int W, int Q,
                                                         long long rows, float* __restrict__ env, float* __restrict__ cep) {
  extern __shared__ __attribute__((aligned(16))) float ev_lds[];
  const EvDims d = ev_dims(W, Q);
  float* va = ev_lds; float* vb = va + (size_t)d.R * d.LS; float* cc = vb + ev_second(d);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long g0 = (long long)blockIdx.x * d.R; g0 < rows; g0 += (long long)gridDim.x * d.R) {
    int any = 0;
    for (int r = wave; r < d.R; r += EV_NW) {
      const long long g = g0 + r;
      bool live = false;
      if (g < rows) {
        const int b = (int)(g / T), t = (int)(g - (long long)b * T);
        live = t < (frames ? min(max(frames[b], 1), T) : T);
      }
      const float* x = spec + (size_t)g * W;
      float* v = va + (size_t)r * d.LS;
      for (int k = lane; k < d.WP; k += 64) v[k] = live && k < W ? x[k] : 0.f;
      any |= live;
    }
    any = __syncthreads_or(any);                                  // also: v is staged
    if (any) ev_tile<NT, false>(va, vb, cc, tabA, tabS, d);
    for (int r = wave; r < d.R; r += EV_NW) {
      const long long g = g0 + r;
      if (g >= rows) continue;
      const int b = (int)(g / T), t = (int)(g - (long long)b * T);
      const bool live = t < (frames ? min(max(frames[b], 1), T) : T);         // a live row makes `any`: vb and cc hold its results
      const float* y = vb + (size_t)r * d.LS;
      float* o = env + (size_t)g * W;
      for (int k = lane; k < W; k += 64) o[k] = live ? y[k] : 0.f;
      if (cep)
        for (int n = lane; n < Q; n += 64) cep[(size_t)g * Q + n] = live ? cc[(size_t)r * d.CS + n] : 0.f;
    }
    __syncthreads();                                              // before the next tile overwrites the three arrays
  }
}

template <int NT>
__global__ __launch_bounds__(EV_NT) void k_spec_warp_formant(const float* __restrict__ spec, const int* __restrict__ frames,
                                                             const int* __restrict__ src, const int* __restrict__ frac,
                                                             const int* __restrict__ out_frames, const float* __restrict__ pitch_scale,
                                                             const float* __restrict__ formant_scale, const float* __restrict__ tabA,
                                                             const float* __restrict__ tabS, int T, int W, int Q, int T_out, long long rows,
                                                             float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float ev_lds[];
  const EvDims d = ev_dims(W, Q);
  float* va = ev_lds; float* vb = va + (size_t)d.R * d.LS; float* cc = vb + ev_second(d);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long g0 = (long long)blockIdx.x * d.R; g0 < rows; g0 += (long long)gridDim.x * d.R) {
    int any = 0;
    for (int r = wave; r < d.R; r += EV_NW) {
      const long long g = g0 + r;
      float* v = va + (size_t)r * d.LS;
      bool live = false;
      if (g < rows) {
        const int b = (int)(g / T_out), j = (int)(g - (long long)b * T_out);
        live = j < min(max(out_frames[b], 0), T_out);
        if (live) {                                               // the time interpolation of k_spec_warp
          const int f = frames ? min(max(frames[b], 1), T) : T;
          const int t0 = min(max(src[g], 0), f - 1), t1 = min(t0 + 1, f - 1);
          const int fr = min(max(frac[g], 0), 65535);
          const bool copy = fr == 0;
          const float wt = (float)fr * (1.f / 65536.f);
          const float* x0 = spec + ((size_t)b * T + t0) * W;
          const float* x1 = copy ? x0 : spec + ((size_t)b * T + t1) * W;      // (a copied row never touches its neighbour)
          for (int k = lane; k < W; k += 64) v[k] = sw_time(x0, x1, k, copy, wt);
          for (int k = W + lane; k < d.WP; k += 64) v[k] = 0.f;
        }
      }
      if (!live)
        for (int k = lane; k < d.WP; k += 64) v[k] = 0.f;
      any |= live;
    }
    any = __syncthreads_or(any);
    if (any) ev_tile<NT, true>(va, vb, cc, tabA, tabS, d);
    for (int r = wave; r < d.R; r += EV_NW) {
      const long long g = g0 + r;
      if (g >= rows) continue;
      const int b = (int)(g / T_out), j = (int)(g - (long long)b * T_out);
      float* o = out + (size_t)g * W;
      if (j >= min(max(out_frames[b], 0), T_out)) {
        for (int k = lane; k < W; k += 64) o[k] = 0.f;
        continue;
      }
      const float* ye = vb + (size_t)r * d.LS;                    // env
      const float* yx = va + (size_t)r * d.LS;                    // e
      const float cp = pitch_scale ? pitch_scale[b] : 1.f, cf = formant_scale ? formant_scale[b] : 1.f;
#pragma unroll 2
      for (int k = lane; k < W; k += 64) {
        const float ge = formant_scale ? ev_gather(ye, k, cf, W) : ye[k];
        const float gx = pitch_scale ? ev_gather(yx, k, cp, W) : yx[k];
        o[k] = ge + gx;
      }
    }
    __syncthreads();
  }
}
