// taco_resample.h -- recordings to the model's sample rate on the GPU: band-limited sinc interpolation, the algorithm of
// resampy.resample that librosa.core.load / librosa.core.resample run (audio/__init__.py:12-20,30-32; recognition/google.py:48),
// restated; UNPINNED on resampy and librosa (include/taco_abi.h).  Output t of a row sits at input position t*orig_sr/target_sr
// EXACTLY: with g = gcd, P = target_sr/g, Q = orig_sr/g it is n = (t*Q) div P plus the phase r = (t*Q) mod P, and the interpolated
// filter an output sees depends on r alone -- a polyphase bank of P rows, built once per rate pair on the host in double
// (taco_resample_create) and rounded to fp32.  Included from taco_lib.hip.
#pragma once

#define RS_THREADS 256         // four waves per workgroup of k_resample
#define RS_PER 4               // outputs per thread
#define RS_TILE (RS_THREADS * RS_PER)      // consecutive outputs of one row per workgroup
#define RS_LDS_FLOATS 16384    // 64 KB: the dynamic LDS a launch gets without opting in to more
#define RS_BANK_CAP (1u << 22) // bank entries (16 MB of fp32) a handle may hold

struct taco_resample {
  int orig_sr = 0, target_sr = 0, device = 0;
  int P = 0, Q = 0;              // phases, and input samples per P outputs
  int LW = 0, RW = 0;            // taps at and left of n (x[n], x[n-1], ...), taps right of it (x[n+1], ...): the most any phase has
  double ratio = 0.0;            // (double)target_sr / orig_sr, as the reference forms it
  std::vector<float> bank;       // host [P, LW + RW]: tap j of row r weighs x[n - (LW - 1) + j]
  float* d_bank = nullptr;       // device [LW + RW, P] (tap-major: the lanes of a wave gather one tap's weights from one row of P words)
  std::mutex mu;                 // guards the upload at first use
};

// Samples row b keeps: L, or num_samples[b] (device memory) clamped to [0, L]
__device__ __forceinline__ int rs_samples(const int* num_samples, int b, int L) { return num_samples ? min(max(num_samples[b], 0), L) : L; }
// Sample `pos` of row b as the reference's decoder and librosa.to_mono deliver it: 16-bit PCM times 1/32768 (audioread's buf_to_float),
// the mean over channels.  The channel sum is formed in double and rounded to fp32 once; one channel passes through as its own bits.
__device__ __forceinline__ float rs_fetch(const void* in, int fmt, int channels, size_t frame) {
  if (fmt == TACO_WAV_PCM16) {
    const short* p = (const short*)in + frame * channels;
    if (channels == 1) return (float)p[0] * (1.0f / 32768.0f);
    double s = 0.0;
    for (int c = 0; c < channels; ++c) s += (double)p[c] * (1.0 / 32768.0);
    return (float)(s / (double)channels);
  }
  const float* p = (const float*)in + frame * channels;
  if (channels == 1) return p[0];
  double s = 0.0;
  for (int c = 0; c < channels; ++c) s += (double)p[c];
  return (float)(s / (double)channels);
}
// grid (tiles of RS_TILE outputs, B).  A workgroup owns outputs [t0, t0 + RS_TILE) of row b.  Those below the row's computed length
// (int)(n_b*ratio) are sums over taps; the rest, up to L_out, are stored as exact zeros; block 0 of a row writes out_samples[b] =
// (int)ceil(n_b*ratio) -- both in double from the expressions of the host queries.  The tile's inputs x[n(t0) - (LW - 1) ..
// n(t_last) + RW] are staged in LDS once, converted and averaged over channels on the way, zeros outside [0, n_b): a tap outside
// the row contributes nothing, as the bounds of the reference's loops have it.  Thread i then owns outputs t0 + i, t0 + i + 256, ...
// (stores of a wave are one line): output t reads LDS from n(t) - n(t0) on and tap j's weight from bank[j*P + r(t)] -- consecutive
// outputs' phases step by Q mod P inside one row of P words, which the L1 holds.  Taps are summed j = 0, 1, ... by fmaf: one order,
// independent of the tile, the batch and whatever runs beside it.
__global__ __launch_bounds__(RS_THREADS) void k_resample(const void* in, int fmt, int channels, const int* num_samples, int L,
                                                         const float* __restrict__ bank, int P, int Q, int LW, int taps, double ratio,
                                                         float* out, int L_out, int* out_samples) {
  extern __shared__ __attribute__((aligned(16))) float rs_x[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = rs_samples(num_samples, b, L);
  const double len = (double)n * ratio;
  const long long computed = min((long long)len, (long long)L_out);
  if (blockIdx.x == 0 && tid == 0 && out_samples) out_samples[b] = (int)ceil(len);
  const long long t0 = (long long)blockIdx.x * RS_TILE;
  float* y = out + (size_t)b * L_out;
  if (t0 >= computed) {
    for (int k = 0; k < RS_PER; ++k) {
      const long long t = t0 + k * RS_THREADS + tid;
      if (t < L_out) y[t] = 0.f;
    }
    return;
  }
  const long long t_last = min(t0 + RS_TILE, computed) - 1;
  const long long n0 = t0 * Q / P, lo = n0 - (LW - 1);
  const int span = (int)(t_last * Q / P - n0) + taps;
  const size_t row = (size_t)b * L;
  for (int i = tid; i < span; i += RS_THREADS) {
    const long long pos = lo + i;
    rs_x[i] = (pos >= 0 && pos < n) ? rs_fetch(in, fmt, channels, row + (size_t)pos) : 0.f;
  }
  __syncthreads();
  int off[RS_PER], ph[RS_PER];
  float acc[RS_PER];
#pragma unroll
  for (int k = 0; k < RS_PER; ++k) {
    const long long t = min(t0 + k * RS_THREADS + tid, t_last);      // (an output past the computed length repeats the last one's reads)
    const long long tq = t * Q;
    off[k] = (int)(tq / P - n0); ph[k] = (int)(tq % P); acc[k] = 0.f;
  }
#pragma unroll 2
  for (int j = 0; j < taps; ++j) {
    const float* w = bank + (size_t)j * P;
#pragma unroll
    for (int k = 0; k < RS_PER; ++k) acc[k] = fmaf(w[ph[k]], rs_x[off[k] + j], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < RS_PER; ++k) {
    const long long t = t0 + k * RS_THREADS + tid;
    if (t < L_out) y[t] = t < computed ? acc[k] : 0.f;
  }
}
