// taco_audio.h -- spectrogram -> waveform on the GPU (audio/__init__.py:54-56,76-96,118-122,149-165;
// synthesizer.py:264 `inv_spectrogram(wav.T)`): denormalise, dB -> amplitude, ^power, Griffin-Lim, inverse pre-emphasis.
// librosa's stft/istft are restated as what they are for this window: a hop-strided gather of win_length samples, one
// windowed-DFT matrix product per direction (on the matrix cores through the same implicit-GEMM kernels as the model,
// 3-term split-bf16), overlap-add with the window sum-square normalisation, reflect padding.  Included from taco_lib.hip.
// The analysis direction (waveform -> the linear and mel targets training consumes) uses the same pack, slots and frame rows:
// k_spec_prepare, the forward product, k_spec_targets.
#pragma once

enum GlFlavor { GL_LIBROSA = 0, GL_TF = 1 };
struct taco_gl {
  taco_audio_hparams hp;
  int n_fft = 0, hop = 0, win = 0, lpad = 0, F = 0;
  taco_model* gm = nullptr;      // container for the two DFT weight packs (GemmVar table + arena)
  ConvL fwd, inv;                // [win -> 2F] analysis, [2F -> win] synthesis (window folded into both)
  size_t w2 = 0;                 // squared padded window [n_fft] (arena offset)
  // analysis (taco_spec_targets): the mel filter bank as bands, device memory of its own (taco_gl_set_mel_basis; 0 filters = not set)
  int num_mels = 0;
  int* mel_band = nullptr;       // [3, num_mels]: first bin, one past the last bin, offset of the filter's weights in mel_w
  float* mel_w = nullptr;        // the weights of every filter's [lo, hi), packed one filter after the other
  // the two other vocoders of audio/__init__.py
  int flavor = GL_LIBROSA;       // GL_TF (taco_gl_create_tf): tf.contrib.signal's uncentred STFT, lpad = 0, w2 unused
  int inv_mels = 0;              // inv_mel_basis: filters of the pseudo-inverse in use (taco_gl_set_inv_mel_basis; 0 = not set)
  float* inv_mel = nullptr;      // [inv_mels, F] mel-major: consecutive lanes read consecutive bins
  // Fast Griffin-Lim (taco_gl_set_momentum): 0 = the reference's loop.  Host state, read when a call is issued; non-zero adds the
  // second estimate buffer to the workspace (carve_gl)
  float momentum = 0.f;
};

// ---- kernels ----
// Frames utterance b keeps: T, or frames[b] (device memory, taco_gl_inv_spectrogram_rows) clamped to [fmin, T].  Every kernel that
// depends on an utterance's length takes the nullable `frames` and calls this; with NULL each one computes what it did before.
__device__ __forceinline__ int gl_frames(const int* frames, int b, int T, int fmin) { return frames ? min(max(frames[b], fmin), T) : T; }
// The magnitude a normalised linear bin x stands for: (10^((clip(x,0,1) * -min_db + min_db + ref_db) / 20))^power.  Written once:
// k_gl_magnitude fills the loop's target with it and k_gl_convergence_partial judges the result against it
__device__ __forceinline__ float gl_magnitude_of(float v, float min_db, float ref_db, float power) {
  const float x = fminf(fmaxf(v, 0.f), 1.f);
  const float db = x * -min_db + min_db + ref_db;
  return powf(powf(10.f, db * 0.05f), power);
}
// S = gl_magnitude_of(spec) ; rows t >= the utterance's frames of every slot are zero
__global__ void k_gl_magnitude(const float* spec, float* S, const int* frames, int fmin, int B, int T, int Tr, int F, float min_db,
                               float ref_db, float power) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * Tr * F) return;
  const int f = (int)(i % F); const size_t row = i / F; const int t = (int)(row % Tr), b = (int)(row / Tr);
  float v = 0.f;
  if (t < gl_frames(frames, b, T, fmin)) v = gl_magnitude_of(spec[((size_t)b * T + t) * F + f], min_db, ref_db, power);
  S[i] = v;
}
__device__ __forceinline__ float gl_hash_uniform(unsigned long long seed, size_t i) {   // counter-based: splitmix64 -> [0,1)
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}
// X = S * exp(2 pi i u): u from the caller ([B,T,F], np.random.rand of audio/__init__.py:77) or from the counter hash
__global__ void k_gl_init_phase(const float* S, const float* u, unsigned long long seed, float* X, const int* frames, int fmin, int B,
                                int T, int Tr, int F) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * Tr * F) return;
  const int f = (int)(i % F); const size_t row = i / F; const int t = (int)(row % Tr), b = (int)(row / Tr);
  float re = 0.f, im = 0.f;
  if (t < gl_frames(frames, b, T, fmin)) {
    const float uu = u ? u[((size_t)b * T + t) * F + f] : gl_hash_uniform(seed, i);
    float sn, cs; sincosf(6.283185307179586f * uu, &sn, &cs);
    re = S[i] * cs; im = S[i] * sn;
  }
  X[row * 2 * F + f] = re; X[row * 2 * F + F + f] = im;
}
// angles = exp(i * angle(est)) (np.angle(0) = 0); X = S * angles
__global__ void k_gl_project(const float* est, const float* S, float* X, size_t rows, int F) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * F) return;
  const size_t row = i / F; const int f = (int)(i % F);
  const float re = est[row * 2 * F + f], im = est[row * 2 * F + F + f];
  const float mag = sqrtf(re * re + im * im), s = S[i];
  X[row * 2 * F + f] = mag > 0.f ? s * re / mag : s;
  X[row * 2 * F + F + f] = mag > 0.f ? s * im / mag : 0.f;
}
// 1 / window-sum-square where it exceeds tiny, else 1 (librosa istft), in padded coordinates [hop*(T-1) + n_fft]
__global__ void k_gl_wss(const float* w2, float* inv, int T, int n_fft, int hop) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int Lp = hop * (T - 1) + n_fft;
  if (p >= Lp) return;
  float s = 0.f;
  const int t1 = min(T - 1, p / hop);
  for (int t = t1; t >= 0 && p - t * hop < n_fft; --t) s += w2[p - t * hop];
  inv[p] = s > 1.17549435e-38f ? 1.0f / s : 1.0f;
}
// y[s] = v, and v again where np.pad mode="reflect" mirrors sample s of y[0 .. n) within `half` of either end (y[-k] = y[k],
// y[n-1+k] = y[n-1-k], k = 1 .. half): the thread that owns a sample writes its reflections
__device__ __forceinline__ void store_reflected(float* y, int s, int n, int half, float v) {
  y[s] = v;
  if (s >= 1 && s <= half) y[-s] = v;
  if (s >= n - 1 - half && s <= n - 2) y[2 * (n - 1) - s] = v;
}
// overlap-add of the windowed frames Y [B, Tr, win] -> centre part of ypad [B, slot], and the reflect padding of n_fft/2 on both sides
// (store_reflected).
// An utterance that keeps fewer than T frames is written up to its own L = hop*(frames-1) samples and reflected there (what lies
// beyond in its slot is read only by STFT frames whose magnitude is 0); it divides by the window sum-square of its own frames,
// summed here from w2 alongside the samples, while one that keeps all T uses the table of k_gl_wss.
// grid (blocks of a row, B): the utterance is uniform in a workgroup.
__global__ void k_gl_overlap_add(const float* Y, const float* wss_inv, const float* w2, float* ypad, const int* frames, int fmin,
                                 int T, int Tr, int win, int hop, int lpad, int n_fft, size_t slot) {
  const int half = n_fft / 2;
  const int b = blockIdx.y, s = blockIdx.x * blockDim.x + threadIdx.x, p = s + half;
  const int fb = gl_frames(frames, b, T, fmin), L = hop * (fb - 1);          // L > n_fft/2 by the clamp to fmin
  if (s >= L) return;
  const bool own = fb < T;
  float acc = 0.f, ws = 0.f;
  const int t1 = min(fb - 1, (p - lpad) / hop);
  for (int t = t1; t >= 0; --t) {
    const int off = p - t * hop - lpad;
    if (off >= win) break;
    acc += Y[((size_t)b * Tr + t) * win + off];
    if (own) ws += w2[lpad + off];
  }
  const float v = acc * (own ? (ws > 1.17549435e-38f ? 1.0f / ws : 1.0f) : wss_inv[p]);
  store_reflected(ypad + (size_t)b * slot + half, s, L, half, v);      // y[0 .. L)
}
// scipy.signal.lfilter([1], [1, -a], x): out[n] = x[n] + a*out[n-1]; one workgroup per utterance, chunked scan.  The utterance's
// own hop*(frames-1) samples are filtered, the rest of its row of L is zero; num_samples (nullable) receives that count.
__global__ __launch_bounds__(1024) void k_inv_preemphasis(const float* ypad, float* wav, const int* frames, int fmin, int T, int hop,
                                                          int* num_samples, int L, int half, size_t slot, float a) {
  __shared__ float ends[1024];
  __shared__ float carry[1024];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* x = ypad + (size_t)b * slot + half;
  float* out = wav + (size_t)b * L;
  const int Lb = hop * (gl_frames(frames, b, T, fmin) - 1);
  if (num_samples && tid == 0) num_samples[b] = Lb;
  const int C = (L + 1023) / 1024, i0 = tid * C, i1 = min(Lb, i0 + C);
  for (int i = max(i0, Lb); i < min(L, i0 + C); ++i) out[i] = 0.f;
  float acc = 0.f;
  for (int i = i0; i < i1; ++i) { acc = x[i] + a * acc; out[i] = acc; }
  ends[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    const float aC = powf(a, (float)C);
    float c = 0.f;
    for (int k = 0; k < 1024; ++k) { carry[k] = c; c = ends[k] + aC * c; }   // carry[k] = out[k*C - 1]
  }
  __syncthreads();
  const float c = carry[tid];
  float f = a;
  for (int i = i0; i < i1; ++i) { out[i] += f * c; f *= a; }
}
// save_audio's scaling (audio/__init__.py:23-24): x * 32767 / max(0.01, max|x|) truncated to int16, per utterance over its first
// num_samples[b] (NULL: L) samples, zeros after.  One workgroup per utterance: the peak (a max: the same in any order), then the scaling.
__global__ __launch_bounds__(1024) void k_wav_to_pcm16(const float* wav, const int* num_samples, int L, short* pcm) {
  __shared__ float part[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* x = wav + (size_t)b * L;
  short* out = pcm + (size_t)b * L;
  const int n = num_samples ? min(max(num_samples[b], 0), L) : L;
  float peak = 0.f;
  for (int i = tid; i < n; i += 1024) peak = fmaxf(peak, fabsf(x[i]));
  for (int o = 32; o > 0; o >>= 1) peak = fmaxf(peak, __shfl_xor(peak, o));
  if ((tid & 63) == 0) part[tid >> 6] = peak;
  __syncthreads();
  peak = part[0];
  for (int k = 1; k < 16; ++k) peak = fmaxf(peak, part[k]);
  const float scale = 32767.0f / fmaxf(0.01f, peak);
  for (int i = tid; i < L; i += 1024) out[i] = i < n ? (short)(int)fminf(fmaxf(truncf(x[i] * scale), -32767.f), 32767.f) : (short)0;
}

// ---- inv_spectrogram_tensorflow (audio/__init__.py:59-61,87-96,109-116): tf.contrib.signal.stft / inverse_stft restated; UNPINNED on TensorFlow ----
// X = S * est / max(1e-8, |est|) (audio/__init__.py:94): a bin whose estimate is zero gives 0, not S as k_gl_project does
__global__ void k_gl_project_tf(const float* est, const float* S, float* X, size_t rows, int F) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * F) return;
  const size_t row = i / F; const int f = (int)(i % F);
  const float re = est[row * 2 * F + f], im = est[row * 2 * F + F + f], s = S[i];
  const float d = fmaxf(1e-8f, sqrtf(re * re + im * im));
  // (rows past an utterance's frames have S = 0 and are written as exact zeros whatever their estimate is)
  X[row * 2 * F + f] = s != 0.f ? s * (re / d) : 0.f;
  X[row * 2 * F + F + f] = s != 0.f ? s * (im / d) : 0.f;
}
// Fast Griffin-Lim (Perraudin, Balazs, Sondergaard 2013; librosa.griffinlim's loop): the projection of z = est - c * prev, prev the
// estimate of the iteration before and c = momentum / (1 + momentum).  TF = false: X = S * exp(i angle(z)) with angle(0) = 0, as
// k_gl_project; TF = true: X = S * z / max(1e-8, |z|), as k_gl_project_tf.  The forward product writes its estimates into two
// buffers in turn, so est and prev are "this one" and "the other one" and nothing is copied.  A bin with S = 0 -- every bin of a
// row past its utterance's frames, whose est and prev hold whatever the slot's slack gave the product -- is written as exact
// zeros without looking at z, so nothing that is not finite there can reach X.
// V bins per thread: 2 where F is even -- then every offset below is even and est, prev, S and X (8-byte aligned) are read and
// written as 8-byte words; with F odd (every n_fft that is a multiple of 4, the reference's included) the Im plane of a row starts
// at an odd word, no pair of both planes is aligned, and V = 1 reads consecutive 4-byte words from consecutive lanes.
// 28 bytes per bin (est, prev, X: 8 each; S: 4) against k_gl_project's 20.
template <bool TF, int V>
__global__ void k_gl_project_fast(const float* est, const float* prev, const float* S, float* X, float c, size_t rows, int F) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= rows * F) return;
  const size_t row = i / F; const int f = (int)(i % F);
  const size_t o = row * 2 * F + f;
  float re[V], im[V], pr[V], pi[V], s[V], xr[V], xi[V];
  if constexpr (V == 2) {
    const float2 a = *reinterpret_cast<const float2*>(est + o), b = *reinterpret_cast<const float2*>(est + o + F);
    const float2 p = *reinterpret_cast<const float2*>(prev + o), q = *reinterpret_cast<const float2*>(prev + o + F);
    const float2 m = *reinterpret_cast<const float2*>(S + i);
    re[0] = a.x; re[1] = a.y; im[0] = b.x; im[1] = b.y; pr[0] = p.x; pr[1] = p.y; pi[0] = q.x; pi[1] = q.y; s[0] = m.x; s[1] = m.y;
  } else {
    re[0] = est[o]; im[0] = est[o + F]; pr[0] = prev[o]; pi[0] = prev[o + F]; s[0] = S[i];
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const float zr = re[v] - c * pr[v], zi = im[v] - c * pi[v];
    const float mag = sqrtf(zr * zr + zi * zi);
    xr[v] = 0.f; xi[v] = 0.f;
    if (s[v] != 0.f) {
      if (TF) {
        const float d = fmaxf(1e-8f, mag);
        xr[v] = s[v] * (zr / d); xi[v] = s[v] * (zi / d);
      } else {
        xr[v] = mag > 0.f ? s[v] * zr / mag : s[v];
        xi[v] = mag > 0.f ? s[v] * zi / mag : 0.f;
      }
    }
  }
  if constexpr (V == 2) {
    *reinterpret_cast<float2*>(X + o) = make_float2(xr[0], xr[1]);
    *reinterpret_cast<float2*>(X + o + F) = make_float2(xi[0], xi[1]);
  } else {
    X[o] = xr[0]; X[o + F] = xi[0];
  }
}
// inverse_stft's overlap-add: y[s] = sum over the frames t that cover s of Y[t, s - t*hop], Y [B, Tr, win] the windowed irfft frames.  No
// window sum-square and no reflect padding; the frames are visited in the order of k_gl_overlap_add.  Utterance b writes its own
// hop*(frames-1) + win samples from the START of its slot of ypad, where the next forward product reads frame t at t*hop (ldx = hop);
// the rest of the slot keeps the zeros it was filled with.  grid (blocks of a row, B).
__global__ void k_gl_overlap_add_tf(const float* Y, float* ypad, const int* frames, int T, int Tr, int win, int hop, size_t slot) {
  const int b = blockIdx.y, s = blockIdx.x * blockDim.x + threadIdx.x;
  const int fb = gl_frames(frames, b, T, 1);
  if (s >= hop * (fb - 1) + win) return;
  float acc = 0.f;
  for (int t = min(fb - 1, s / hop); t >= 0; --t) {
    const int off = s - t * hop;
    if (off >= win) break;
    acc += Y[((size_t)b * Tr + t) * win + off];
  }
  ypad[(size_t)b * slot + s] = acc;
}
// The utterance's own samples out of its slot, exact zeros after in its row of L; num_samples (nullable) receives the count
__global__ void k_gl_output_tf(const float* ypad, float* wav, const int* frames, int T, int win, int hop, int* num_samples, int L, size_t slot) {
  const int b = blockIdx.y, s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= L) return;
  const int Lb = hop * (gl_frames(frames, b, T, 1) - 1) + win;
  if (num_samples && s == 0) num_samples[b] = Lb;
  wav[(size_t)b * L + s] = s < Lb ? ypad[(size_t)b * slot + s] : 0.f;
}

// ---- inv_melspectrogram (audio/__init__.py:70-72,136-140): mel -> linear magnitudes through the pseudo-inverse of the filter bank ----
#define MELMAG_ROWS 8          // frame rows per workgroup of k_gl_mel_magnitude: a weight of the inverse basis is fetched once for eight rows
// out[b, t, f] = max(1e-10, sum_m inv[m, f] * amp[b, t, m]) (then ^power with apply_pow), amp = 10^((clip(mel,0,1) * -min_db + min_db) / 20):
// _mel_to_linear(_db_to_amp(_denormalize(mel))) -- no ref_level_db, melspectrogram never subtracts it.  A workgroup stages the
// amplitudes of its MELMAG_ROWS rows in LDS ([m][row], so a thread reads the eight of one m as two 16-byte words); the exponent and
// the power of ten are formed in double there (num_mels values per row: nothing beside the sum), so an amplitude carries one
// rounding.  Each thread owns bins f = tid, tid + 256, ... and sums m = 0 .. M-1 in that order with fmaf in fp32: the pseudo-inverse
// has entries of both signs and the sum cancels heavily, so it does NOT go through the split-bf16 product; in this fixed order it
// has the dot-product bound tests/test_gpu_vocoder.py holds it to.  Rows t >= the utterance's frames (and the slot's tail rows
// t >= T) are zero.  out has Tr rows per utterance (the S buffer of the Griffin-Lim workspace; Tr = T for taco_gl_mel_to_linear).
// grid (blocks of MELMAG_ROWS rows, B), 256 threads, MELMAG_ROWS * M floats of LDS.
__global__ __launch_bounds__(256) void k_gl_mel_magnitude(const float* mel, const float* inv, float* out, const int* frames, int fmin, int T,
                                                          int Tr, int F, int M, float min_db, float power, int apply_pow) {
  extern __shared__ __attribute__((aligned(16))) float melmag_amp[];      // [M, MELMAG_ROWS]
  const int b = blockIdx.y, t0 = blockIdx.x * MELMAG_ROWS, tid = threadIdx.x;
  const int fb = gl_frames(frames, b, T, fmin);
  for (int i = tid; i < MELMAG_ROWS * M; i += 256) {
    const int r = i / M, m = i - r * M, t = t0 + r;
    float a = 0.f;
    if (t < fb) {
      const double x = (double)fminf(fmaxf(mel[((size_t)b * T + t) * M + m], 0.f), 1.f);
      a = (float)pow(10.0, (x * -(double)min_db + (double)min_db) * 0.05);
    }
    melmag_amp[m * MELMAG_ROWS + r] = a;
  }
  __syncthreads();
  const float4* amp4 = reinterpret_cast<const float4*>(melmag_amp);
  for (int f = tid; f < F; f += 256) {
    float acc[MELMAG_ROWS];
#pragma unroll
    for (int r = 0; r < MELMAG_ROWS; ++r) acc[r] = 0.f;
    for (int m = 0; m < M; ++m) {
      const float w = inv[(size_t)m * F + f];
      const float4 a0 = amp4[2 * m], a1 = amp4[2 * m + 1];
      acc[0] = fmaf(w, a0.x, acc[0]); acc[1] = fmaf(w, a0.y, acc[1]); acc[2] = fmaf(w, a0.z, acc[2]); acc[3] = fmaf(w, a0.w, acc[3]);
      acc[4] = fmaf(w, a1.x, acc[4]); acc[5] = fmaf(w, a1.y, acc[5]); acc[6] = fmaf(w, a1.z, acc[6]); acc[7] = fmaf(w, a1.w, acc[7]);
    }
#pragma unroll
    for (int r = 0; r < MELMAG_ROWS; ++r) {
      const int t = t0 + r;
      if (t < Tr) {
        float v = 0.f;
        if (t < fb) {
          v = fmaxf(1e-10f, acc[r]);
          if (apply_pow) v = powf(v, power);
        }
        out[((size_t)b * Tr + t) * F + f] = v;
      }
    }
  }
}
static_assert(MELMAG_ROWS == 8, "k_gl_mel_magnitude reads a mel's eight amplitudes as two float4");

// ---- silence trimming: librosa.effects.trim (synthesizer.py:266-269), restated; UNPINNED on librosa (include/taco_abi.h) ----
#define TRIM_THREADS 256       // four waves per workgroup of k_trim_energy
#define TRIM_FRAMES 16         // frames per tile at most; trim_frames_per_tile lowers it until the tile fits TRIM_LDS_BYTES
#define TRIM_LDS_BYTES 65536   // dynamic LDS a launch gets without opting in to more
// Samples row b keeps: L, or num_samples[b] (device memory) clamped to [0, L]
__device__ __forceinline__ int trim_samples(const int* num_samples, int b, int L) { return num_samples ? min(max(num_samples[b], 0), L) : L; }
// np.pad(y, N/2, mode="reflect") as an index map: padded position j - N/2 -> a sample in [0, n), period 2(n - 1), n >= 2.  A row
// shorter than N/2 is reflected more than once; 64-bit because 2(n - 1) and a padded position can pass 2^31.
__device__ __forceinline__ int trim_reflect(long long j, int n) {
  if (j >= 0 && j < n) return (int)j;
  const long long P = 2LL * (n - 1);
  long long m = j % P;
  if (m < 0) m += P;
  return (int)(m < n ? m : P - m);
}
// Frame energies of B rows.  Frame t of row b is the N samples of the reflect-padded row from t*hop; a row has 1 + n_b/hop frames.
//   TACO_TRIM_SPECTRAL  mse = mean over the N/2 + 1 one-sided bins of |rfft(hann * frame)|^2, without a transform: for a real frame
//                       of even length, sum_{k=0..N/2} |X_k|^2 = (N sum xw^2 + (sum xw)^2 + (sum (-1)^i xw)^2) / 2  (Parseval; DC and
//                       Nyquist count once in the full spectrum and are added back) -- every term is positive
//   TACO_TRIM_TIME      mse = sum x^2 / N, no window
// grid (tiles of fpt frames, B), TRIM_THREADS threads.  A workgroup stages its tile's (ft - 1)*hop + N samples in LDS once, each
// through trim_reflect from wav[b, :n_b] (nothing at or past n_b is read), and the periodic Hann table beside them; its waves take
// the tile's frames round-robin.  Lane l sums i = l, l + 64, ... in that order, so its (-1)^i is one sign, and a butterfly of fixed
// shape joins the 64 partial sums: one order per sum, two calls give the same bits.  Frames at or past the row's own count are
// not written (k_trim_index does not read them).
__global__ __launch_bounds__(TRIM_THREADS) void k_trim_energy(const float* wav, const int* num_samples, int L, int N, int hop, int fpt,
                                                              int Fmax, int energy, float* mse) {
  extern __shared__ __attribute__((aligned(16))) float trim_lds[];      // samples [(fpt - 1)*hop + N] | window [N] (spectral only)
  const int b = blockIdx.y, t0 = blockIdx.x * fpt, tid = threadIdx.x;
  const int n = trim_samples(num_samples, b, L);
  if (n < 2) return;
  const int nf = 1 + n / hop;
  if (t0 >= nf) return;
  const int ft = min(fpt, nf - t0), span = (ft - 1) * hop + N;
  float* xs = trim_lds;
  float* win = trim_lds + (size_t)(fpt - 1) * hop + N;
  const float* x = wav + (size_t)b * L;
  const long long j0 = (long long)t0 * hop - N / 2;
  for (int i = tid; i < span; i += TRIM_THREADS) xs[i] = x[trim_reflect(j0 + i, n)];
  if (energy == TACO_TRIM_SPECTRAL)
    for (int i = tid; i < N; i += TRIM_THREADS) win[i] = 0.5f - 0.5f * cospif((float)(2 * i) / (float)N);      // periodic Hann
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int f = wave; f < ft; f += TRIM_THREADS / 64) {
    const float* fx = xs + f * hop;
    float s2 = 0.f, s1 = 0.f;
    if (energy == TACO_TRIM_SPECTRAL) {
      for (int i = lane; i < N; i += 64) { const float v = fx[i] * win[i]; s2 = fmaf(v, v, s2); s1 += v; }
    } else {
      for (int i = lane; i < N; i += 64) { const float v = fx[i]; s2 = fmaf(v, v, s2); }
    }
    float sa = (lane & 1) ? -s1 : s1;                     // sum (-1)^i xw: i = lane mod 2 on this lane
    for (int o = 32; o > 0; o >>= 1) { s2 += __shfl_xor(s2, o); s1 += __shfl_xor(s1, o); sa += __shfl_xor(sa, o); }
    if (lane == 0)
      mse[(size_t)b * Fmax + t0 + f] = energy == TACO_TRIM_SPECTRAL ? ((float)N * s2 + s1 * s1 + sa * sa) * 0.5f / (float)(N / 2 + 1)
                                                                    : s2 / (float)N;
  }
}
// The frame dB law of k_trim_index and k_split_edges, written once so that the two agree by construction (tests/test_gpu_split.py).
// trim_db_ref: 10 log10(max(1e-10, max_t e[t])) over a row's nf energies, by a workgroup of 256 threads (four waves), the same
// value in every thread; a maximum is the same in any order.
__device__ __forceinline__ float trim_db_ref(const float* e, int nf) {
  __shared__ float pmax[4];
  const int tid = threadIdx.x;
  float mx = 0.f;                                          // energies are >= 0
  for (int t = tid; t < nf; t += 256) mx = fmaxf(mx, e[t]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((tid & 63) == 0) pmax[tid >> 6] = mx;
  __syncthreads();
  return 10.f * log10f(fmaxf(1e-10f, fmaxf(fmaxf(pmax[0], pmax[1]), fmaxf(pmax[2], pmax[3]))));
}
// One frame's dB below ref
__device__ __forceinline__ float trim_db(float e, float ref) {
#pragma clang fp contract(off)      // the product is rounded before the subtraction, as ref was: the loudest frame is exactly 0 dB
  return 10.f * log10f(fmaxf(1e-10f, e)) - ref;
}
// logamplitude(ref_power=np.max) and the index: db[t] = 10 log10(max(1e-10, mse[t])) - 10 log10(max(1e-10, max_t mse)); a frame is
// non-silent where db > -top_db; index[b] = {first*hop, min(n_b, (last + 1)*hop)}, {0, 0} when no frame is, {0, n_b} for a row of
// fewer than two samples (it has no frames).  frame_db (nullable) receives db for the row's own frames and zeros after.  One
// workgroup per row; a maximum and a minimum are the same in any order.
__global__ __launch_bounds__(256) void k_trim_index(const float* mse, const int* num_samples, int L, int hop, int Fmax, float top_db,
                                                    int* index, float* frame_db) {
  __shared__ int pfirst[4], plast[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = trim_samples(num_samples, b, L), nf = n < 2 ? 0 : 1 + n / hop;
  const float* e = mse + (size_t)b * Fmax;
  const float ref = trim_db_ref(e, nf);
  int first = 0x7fffffff, last = -1;
  for (int t = tid; t < Fmax; t += 256) {
    float db = 0.f;
    if (t < nf) {
      db = trim_db(e[t], ref);
      if (db > -top_db) { first = min(first, t); last = max(last, t); }
    }
    if (frame_db) frame_db[(size_t)b * Fmax + t] = db;
  }
  for (int o = 32; o > 0; o >>= 1) { first = min(first, __shfl_xor(first, o)); last = max(last, __shfl_xor(last, o)); }
  if ((tid & 63) == 0) { pfirst[tid >> 6] = first; plast[tid >> 6] = last; }
  __syncthreads();
  if (tid == 0) {
    first = min(min(pfirst[0], pfirst[1]), min(pfirst[2], pfirst[3]));
    last = max(max(plast[0], plast[1]), max(plast[2], plast[3]));
    int start = 0, end = n < 2 ? n : 0;
    if (last >= 0) { start = (int)min((long long)first * hop, (long long)n); end = (int)min((long long)n, (long long)(last + 1) * hop); }
    index[2 * b] = start; index[2 * b + 1] = end;
  }
}

// ---- splitting on silence: librosa.effects.split and remove_breath (audio/silence.py:21-31,44-45,53-54), restated; UNPINNED on librosa ----
#define SPLIT_THREADS 256      // four waves: a chunk of k_split_edges is 256 frames
static_assert(SPLIT_THREADS == 256, "trim_db_ref joins the maxima of four waves");
// The maximal runs of non-silent frames of row b, in order, from the mse table k_trim_energy wrote.  db[t] is k_trim_index's: the same
// trim_db_ref and trim_db, non-silent where db > -top_db.  An EDGE is a frame t in [0, nf] whose
// state differs from frame t - 1's, with frames -1 and nf counted as silent: that is flatnonzero(diff(non_silent)) + 1 with the 0
// prepended when frame 0 is non-silent and len(non_silent) appended when the last frame is.  Edge number k (even: a run starts, odd:
// one ends) goes to word k of the row's table as min(n, t*hop) -- so run r is {s*hop, min(n, e*hop)}, and {n, n} when n % hop == 0
// and only the last frame is non-silent.  k comes from a block-wide prefix count: ballot and popcount inside a wave, the four wave
// totals through LDS, and a running count carried across the 256-frame chunks of a long row -- no atomics, so the order does not
// depend on scheduling and two calls return the same bits.  counts[b] receives the true number of runs; only the first
// max_intervals are written and every other word of the row's table is an exact zero.  frame_db as in k_trim_index.  One workgroup
// per row; a row of fewer than two samples has no frames and count 0.
__global__ __launch_bounds__(SPLIT_THREADS) void k_split_edges(const float* mse, const int* num_samples, int L, int hop, int Fmax, float top_db,
                                                               int max_intervals, int* intervals, int* counts, float* frame_db) {
  __shared__ unsigned long long wmask[4];
  __shared__ int wedges[4];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = trim_samples(num_samples, b, L), nf = n < 2 ? 0 : 1 + n / hop;
  const float* e = mse + (size_t)b * Fmax;
  int* tab = intervals + (size_t)b * max_intervals * 2;
  const long long cap = 2LL * max_intervals;
  const float ref = trim_db_ref(e, nf);
  const int last = max(nf, frame_db ? Fmax - 1 : 0);       // frames 0 .. last are visited: nf itself closes a run that reaches the end
  long long seen = 0;                                      // edges in the chunks before this one (the same in every thread)
  bool carry = false;                                      // the state of the last frame of the chunk before this one
  for (int t0 = 0; t0 <= last; t0 += SPLIT_THREADS) {
    const int t = t0 + tid;
    float db = 0.f;
    bool loud = false;
    if (t < nf) {
      db = trim_db(e[t], ref);
      loud = db > -top_db;
    }
    if (frame_db && t < Fmax) frame_db[(size_t)b * Fmax + t] = db;
    const unsigned long long m = __ballot(loud);
    if (lane == 0) wmask[wave] = m;
    __syncthreads();
    const bool before = lane ? (m >> (lane - 1)) & 1 : (wave ? (wmask[wave - 1] >> 63) & 1 : carry);
    carry = (wmask[3] >> 63) & 1;
    const bool edge = t <= nf && loud != before;
    const unsigned long long em = __ballot(edge);
    if (lane == 0) wedges[wave] = __popcll(em);
    __syncthreads();
    long long k = seen + __popcll(em & ((1ull << lane) - 1));
    for (int w = 0; w < wave; ++w) k += wedges[w];
    if (edge && k < cap) tab[k] = (int)min((long long)n, (long long)t * hop);
    seen += wedges[0] + wedges[1] + wedges[2] + wedges[3];
  }
  if (tid == 0) counts[b] = (int)(seen / 2);               // every run that starts also ends: frame nf is silent
  for (long long i = min(seen, cap) + tid; i < cap; i += SPLIT_THREADS) tab[i] = 0;
}
#define MUTE_THREADS 1024      // sixteen waves per row of k_breath_mute
#define MUTE_BATCH 1024        // intervals whose sums are held in LDS at a time
// remove_breath (audio/silence.py:21-31) on row s of a rectangle [S, L], given the row's interval table (k_split_edges at 128 / 32)
// and count: interval k is muted iff abs_mean(audio[start:end]) < abs_mean(audio) - threshold, and since the reference mutes in
// place, abs_mean(audio) is re-evaluated after every mute.  Restated with sums: total = sum |x| over the row's n samples, sum_k over
// interval k (the intervals are disjoint, so muting one changes no other's sum); ONE thread walks the intervals in order with a
// running total: muted iff len_k > 0 and sum_k/len_k < total/n - threshold, and a muted interval's sum leaves the total.  An empty
// interval is never muted (NumPy's mean of nothing is NaN and the comparison is false).  Every sum has one order: thread i of the
// row's 1024 (lane i of an interval's wave) adds its samples i, i + stride, ... in that order, and butterflies and a fixed chain
// join the partial sums.  The row is first copied to out (zeros past n; out may alias wav, the copy is then each thread's own word),
// then the table is taken MUTE_BATCH intervals at a time -- sums by the waves round-robin, the walk, the zeros of the muted ones by
// the waves round-robin -- so a table of any length is served from a fixed LDS footprint, bounded, without a spin.  Only the first
// max_intervals intervals of a row exist for it; bounds are clamped to [0, n] and nothing at or past n is read.
// muted [S, max_intervals] and abs_mean [S, 1 + max_intervals] (both nullable): the flags, and total/n (0 for an empty row) followed
// by every interval's mean (NaN for an empty one, as NumPy's); entries past the row's count are zero.
__global__ __launch_bounds__(MUTE_THREADS) void k_breath_mute(const float* wav, const int* num_samples, int L, const int* intervals,
                                                              const int* counts, int max_intervals, float threshold, float* out, int* muted,
                                                              float* abs_mean) {
#pragma clang fp contract(off)      // the means are rounded before they are compared, as the reported ones are
  __shared__ float part[MUTE_THREADS / 64];
  __shared__ float isum[MUTE_BATCH];
  __shared__ int ilo[MUTE_BATCH], ihi[MUTE_BATCH];
  __shared__ int iflag[MUTE_BATCH];
  __shared__ float total_s;
  const int s = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = trim_samples(num_samples, s, L);
  const int cnt = min(max(counts[s], 0), max_intervals);
  const float* x = wav + (size_t)s * L;
  float* y = out + (size_t)s * L;
  const int* tab = intervals + (size_t)s * max_intervals * 2;
  float acc = 0.f;
  for (int i = tid; i < L; i += MUTE_THREADS) {
    const float v = i < n ? x[i] : 0.f;
    acc += fabsf(v);
    y[i] = v;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < MUTE_THREADS / 64; ++w) t += part[w];
    total_s = t;
    if (abs_mean) abs_mean[(size_t)s * (1 + max_intervals)] = n > 0 ? t / (float)n : 0.f;
  }
  for (int k0 = 0; k0 < cnt; k0 += MUTE_BATCH) {
    const int kb = min(MUTE_BATCH, cnt - k0);
    for (int j = wave; j < kb; j += MUTE_THREADS / 64) {
      const int lo = min(max(tab[2 * (k0 + j)], 0), n), hi = min(max(tab[2 * (k0 + j) + 1], lo), n);
      float a = 0.f;
      for (int i = lo + lane; i < hi; i += 64) a += fabsf(x[i]);
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
      if (lane == 0) { isum[j] = a; ilo[j] = lo; ihi[j] = hi; }
    }
    __syncthreads();                                       // (also orders the copy above before the zeros below)
    if (tid == 0) {
      float total = total_s;
      const float fn = (float)n;
      for (int j = 0; j < kb; ++j) {
        const int len = ihi[j] - ilo[j];
        const bool m = len > 0 && isum[j] / (float)len < total / fn - threshold;
        if (m) total -= isum[j];
        iflag[j] = m;
      }
      total_s = total;
    }
    __syncthreads();
    for (int j = tid; j < kb; j += MUTE_THREADS) {
      if (muted) muted[(size_t)s * max_intervals + k0 + j] = iflag[j];
      if (abs_mean) abs_mean[(size_t)s * (1 + max_intervals) + 1 + k0 + j] = isum[j] / (float)(ihi[j] - ilo[j]);
    }
    for (int j = wave; j < kb; j += MUTE_THREADS / 64)
      if (iflag[j])
        for (int i = ilo[j] + lane; i < ihi[j]; i += 64) y[i] = 0.f;
    __syncthreads();                                       // the next batch overwrites isum / ilo / ihi
  }
  for (int k = cnt + tid; k < max_intervals; k += MUTE_THREADS) {
    if (muted) muted[(size_t)s * max_intervals + k] = 0;
    if (abs_mean) abs_mean[(size_t)s * (1 + max_intervals) + 1 + k] = 0.f;
  }
}

// ---- waveform -> linear and mel targets (audio/__init__.py:48-51,64-67,142-147,155-156,161-162; datasets/generate_data.py:151-158) ----
#define SPEC_ROWS 4            // frame rows per workgroup of k_spec_targets: the band table is fetched once for four rows
// Samples utterance b keeps: Lmax, or num_samples[b] (device memory) clamped to [n_fft/2 + 1, Lmax] -- reflect padding needs n > n_fft/2
__device__ __forceinline__ int spec_samples(const int* num_samples, int b, int Lmax, int half) {
  return num_samples ? min(max(num_samples[b], half + 1), Lmax) : Lmax;
}
// Pre-emphasis p[i] = y[i] - a*y[i-1], y[-1] = 0 (scipy.signal.lfilter([1, -a], [1], y)) of wav [B, Lmax] into the centre of each
// utterance's slot of ypad, and the reflect padding of n_fft/2 at the utterance's OWN ends (store_reflected,
// as k_gl_overlap_add).  Everything else of the slot -- and, behind the last slot, the slack the tail rows of
// the frame matrix read -- is zeroed, so no frame row reads another call's data.  nf_ws [B] and num_frames [B] (nullable) receive
// 1 + n_b / hop.  grid (blocks of a slot, B).
__global__ void k_spec_prepare(const float* wav, const int* num_samples, float* ypad, int* nf_ws, int* num_frames, int B, int Lmax, int hop,
                               int half, size_t slot, size_t tail, float a) {
  const int b = blockIdx.y;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= slot + (b == B - 1 ? tail : 0)) return;
  const int n = spec_samples(num_samples, b, Lmax, half);
  if (i == 0) { nf_ws[b] = 1 + n / hop; if (num_frames) num_frames[b] = 1 + n / hop; }
  float* y = ypad + (size_t)b * slot + half;             // y[0 .. n)
  if (i < (size_t)n) {
    const int s = (int)i;
    const float* x = wav + (size_t)b * Lmax;
    store_reflected(y, s, n, half, s ? x[s] - a * x[s - 1] : x[0]);
  }
  if (i >= (size_t)n + 2 * half) y[(ptrdiff_t)i - half] = 0.f;
}
// clip((20 log10(max(1e-5, amp)) - sub_db - min_db) / -min_db, 0, 1): _normalize(_amp_to_db(amp) - sub_db)
__device__ __forceinline__ float spec_normalize(float amp, float sub_db, float min_db) {
  const float db = 20.f * log10f(fmaxf(1e-5f, amp));
  return fminf(fmaxf((db - sub_db - min_db) / -min_db, 0.f), 1.f);
}
// The back end of the analysis, fused: per frame row of est [B*Tr, 2F] (Re | Im) the magnitude |D| goes to LDS once; the linear row
// is written from it, and the num_mels filter sums are formed from the same LDS copy -- the magnitude never goes to memory.
// A filter is its band [lo, hi) of bins and hi - lo packed weights.  Sixteen lanes share one (row, filter): lane l sums bins lo + l,
// lo + l + 16, ... in that order and the sixteen partial sums meet in a butterfly of fixed shape, so a sum has one order whatever
// runs beside it (no atomics).  Rows t >= the utterance's frames (nframes [B], NULL: T) are stored as zeros.
// grid (blocks of SPEC_ROWS frames, B), 256 threads, SPEC_ROWS * F floats of LDS.
__global__ __launch_bounds__(256) void k_spec_targets(const float* est, const int* nframes, int T, int Tr, int F, const int* band,
                                                      const float* mw, int M, float* lin, float* mel, float min_db, float ref_db) {
  extern __shared__ float spec_mag[];      // [SPEC_ROWS, F]
  const int b = blockIdx.y, t0 = blockIdx.x * SPEC_ROWS, tid = threadIdx.x;
  const int Tb = nframes ? min(nframes[b], T) : T;
#pragma unroll
  for (int r = 0; r < SPEC_ROWS; ++r) {
    const int t = t0 + r;
    if (t >= T) break;
    float* lo = lin + ((size_t)b * T + t) * F;
    if (t < Tb) {
      const float* e = est + ((size_t)b * Tr + t) * 2 * F;
      for (int f = tid; f < F; f += 256) {
        const float re = e[f], im = e[F + f];
        const float m = sqrtf(re * re + im * im);
        spec_mag[r * F + f] = m;
        lo[f] = spec_normalize(m, ref_db, min_db);
      }
    } else {
      for (int f = tid; f < F; f += 256) lo[f] = 0.f;
    }
  }
  if (!mel) return;
  __syncthreads();
  const int g = tid >> 4, l = tid & 15;
  for (int r = 0; r < SPEC_ROWS; ++r) {
    const int t = t0 + r;
    if (t >= T) break;
    float* mo = mel + ((size_t)b * T + t) * M;
    if (t >= Tb) {
      for (int m = tid; m < M; m += 256) mo[m] = 0.f;
      continue;
    }
    const float* mg = spec_mag + r * F;
    for (int m = g; m < M; m += 16) {                    // (the sixteen lanes of a group take every branch together)
      const int k0 = band[m], k1 = band[M + m];
      const float* w = mw + band[2 * M + m] - k0;
      float acc = 0.f;
      for (int k = k0 + l; k < k1; k += 16) acc = fmaf(w[k], mg[k], acc);
      acc += __shfl_xor(acc, 8, 16); acc += __shfl_xor(acc, 4, 16); acc += __shfl_xor(acc, 2, 16); acc += __shfl_xor(acc, 1, 16);
      if (l == 0) mo[m] = spec_normalize(acc, 0.f, min_db);
    }
  }
}

// ---- spectral convergence of a waveform against its target (taco_gl_convergence) ----
#define CONV_ROWS 8            // frame rows per workgroup of k_gl_convergence_partial
// hop * (frames - 1) per utterance, frames clamped as the vocoder clamps them: the sample counts k_spec_prepare takes
__global__ void k_gl_frames_to_samples(const int* frames, int fmin, int T, int hop, int B, int* num_samples) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) num_samples[b] = hop * (gl_frames(frames, b, T, fmin) - 1);
}
// Stage one of sc[b] = ||  |est| - S || / || S || over utterance b's own frames t < nframes[b] and all F bins: the workgroup of
// (tile, b) sums num = (|est| - S)^2 and den = S^2 over its CONV_ROWS frame rows of est [B*Tr, 2F] (Re | Im) into part[b, tile] =
// {num, den}; a tile past the utterance's frames writes zeros.  S is formed on the fly: kind 0, target [B, T, F] is a normalised
// linear spectrogram and S = gl_magnitude_of(target), the law of k_gl_magnitude; kind 1, target holds the magnitudes themselves.
// One order per sum and no atomics: thread i adds the bins i, i + 256, ... of the tile's rows in ascending row with one fmaf each, a
// butterfly of fixed shape joins the 64 lanes of a wave, and thread 0 adds the four wave sums in ascending order.
// grid (tiles of CONV_ROWS rows, B), 256 threads.
__global__ __launch_bounds__(256) void k_gl_convergence_partial(const float* est, const float* target, int kind, const int* nframes, int T, int Tr,
                                                                int F, float min_db, float ref_db, float power, float* part) {
  __shared__ float wsum[4][2];
  const int b = blockIdx.y, t0 = blockIdx.x * CONV_ROWS, tid = threadIdx.x;
  const int Tb = min(nframes[b], T);
  float num = 0.f, den = 0.f;
  for (int r = 0; r < CONV_ROWS; ++r) {
    const int t = t0 + r;
    if (t >= Tb) break;
    const float* e = est + ((size_t)b * Tr + t) * 2 * F;
    const float* g = target + ((size_t)b * T + t) * F;
    for (int f = tid; f < F; f += 256) {
      const float re = e[f], im = e[F + f];
      const float s = kind ? g[f] : gl_magnitude_of(g[f], min_db, ref_db, power);
      const float d = sqrtf(re * re + im * im) - s;
      num = fmaf(d, d, num); den = fmaf(s, s, den);
    }
  }
  for (int o = 32; o > 0; o >>= 1) { num += __shfl_xor(num, o); den += __shfl_xor(den, o); }
  if ((tid & 63) == 0) { wsum[tid >> 6][0] = num; wsum[tid >> 6][1] = den; }
  __syncthreads();
  if (tid == 0) {
    float* p = part + ((size_t)b * gridDim.x + blockIdx.x) * 2;
    p[0] = ((wsum[0][0] + wsum[1][0]) + wsum[2][0]) + wsum[3][0];
    p[1] = ((wsum[0][1] + wsum[1][1]) + wsum[2][1]) + wsum[3][1];
  }
}
// Stage two: sc[b] = sqrt(num / den) from the utterance's P partial pairs, 0 where den == 0 (a silent target).  One wave per
// utterance: lane l adds the pairs l, l + 64, ... in that order, a butterfly of fixed shape joins the lanes.
__global__ __launch_bounds__(64) void k_gl_convergence_final(const float* part, int P, float* sc) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* p = part + (size_t)b * P * 2;
  float num = 0.f, den = 0.f;
  for (int i = lane; i < P; i += 64) { num += p[2 * i]; den += p[2 * i + 1]; }
  for (int o = 32; o > 0; o >>= 1) { num += __shfl_xor(num, o); den += __shfl_xor(den, o); }
  if (lane == 0) sc[b] = den > 0.f ? sqrtf(num / den) : 0.f;
}

// ---- host ----
static int gl_rows(const taco_gl* g, int T) { return T + cdiv(g->n_fft, g->hop); }                 // frames per utterance slot (tail frames read the slack)
static size_t gl_slot(const taco_gl* g, int T) { return (size_t)gl_rows(g, T) * g->hop; }          // samples per utterance slot >= hop*(T-1) + n_fft
struct GlWs { float *S, *X, *est, *Y, *ypad, *wss, *est2; };      // est2: the other estimate buffer of the fast loop, NULL at momentum 0
static void carve_gl(Carver& cv, const taco_gl* g, int B, int T, GlWs& w) {
  const size_t R = (size_t)B * gl_rows(g, T);
  w.S = cv.f(R * g->F); w.X = cv.f(R * 2 * g->F); w.est = cv.f(R * 2 * g->F); w.Y = cv.f(R * g->win);
  w.ypad = cv.f((size_t)B * gl_slot(g, T) + 2 * g->n_fft + g->win);
  w.wss = cv.f((size_t)g->hop * (T - 1) + g->n_fft);
  w.est2 = g->momentum != 0.f ? cv.f(R * 2 * g->F) : nullptr;      // last, and only then: at momentum 0 the layout and its size are what they were
}
static size_t mel_lds_bytes(int num_mels) { return (size_t)MELMAG_ROWS * num_mels * sizeof(float); }   // k_gl_mel_magnitude's amplitudes
// analysis: T = 1 + Lmax / hop frames per utterance in the slot geometry above (a padded utterance is Lmax + n_fft <= gl_slot samples)
struct SpecWs { float *ypad, *est; int* nf; };
static size_t spec_tail(const taco_gl* g) { return (size_t)2 * g->n_fft + g->win; }                // slack behind the last slot
static void carve_spec(Carver& cv, const taco_gl* g, int B, int T, SpecWs& w) {
  w.ypad = cv.f((size_t)B * gl_slot(g, T) + spec_tail(g));
  w.est = cv.f((size_t)B * gl_rows(g, T) * 2 * g->F);
  w.nf = cv.i(B);
}
// convergence: the analysis workspace, the sample counts k_spec_prepare reads and the partial pairs of k_gl_convergence_partial
struct ConvWs { SpecWs spec; int* ns; float* part; };
static void carve_conv(Carver& cv, const taco_gl* g, int B, int T, ConvWs& w) {
  carve_spec(cv, g, B, T, w.spec);
  w.ns = cv.i(B);
  w.part = cv.f((size_t)B * cdiv(T, CONV_ROWS) * 2);
}
// silence trimming: frames per tile of k_trim_energy, the most (<= TRIM_FRAMES) whose samples and window fit TRIM_LDS_BYTES; 0 = not even one
static size_t trim_lds_bytes(int N, int hop, int fpt, int energy) {
  return ((size_t)(fpt - 1) * hop + N + (energy == TACO_TRIM_SPECTRAL ? N : 0)) * sizeof(float);
}
static int trim_frames_per_tile(int N, int hop, int energy) {
  int fpt = TRIM_FRAMES;
  while (fpt > 0 && trim_lds_bytes(N, hop, fpt, energy) > TRIM_LDS_BYTES) --fpt;
  return fpt;
}

// ---- splitting and levelling 16-bit PCM on silence: pydub.silence.detect_nonsilent (audio/silence.py:81-117, app.py:27-53), restated;
// UNPINNED on pydub (include/taco_abi.h).  Everything below is integer arithmetic: any order of a sum gives the same bits. ----
#define PCM_THREADS 256        // four waves per workgroup of every kernel below
#define PCM_E_MS 64            // milliseconds per tile of k_pcm_energy at most; pcm_energy_tile lowers it until the span fits PCM_E_LDS_WORDS
#define PCM_E_LDS_WORDS 24576  // 16-bit words of LDS a tile's span may take (48 KB)
#define PCM_W_TILE 256         // window starts per tile of k_pcm_windows: one per thread
#define PCM_W_LDS_BYTES 65536  // dynamic LDS a launch gets without opting in to more: PCM_W_TILE + W energies of 8 bytes
// Frame at which millisecond j starts: floor(j*sr/1000), pydub's int(j * (sr/1000.0)) (tests/test_pydub_host.py holds the two equal)
__host__ __device__ __forceinline__ long long pcm_frame_of_ms(long long j, int sr) { return j * sr / 1000; }
// Length in milliseconds of n frames: pydub's round(1000 * (n / sr)), Python's round (half to even), in double as pydub forms it.
// One multiplication after one division: nothing to contract, and both are correctly rounded on the host and on the device.
__host__ __device__ __forceinline__ int pcm_len_ms(int n, int sr) { return (int)rint(1000.0 * ((double)n / (double)sr)); }
// Frames row b keeps: L, or num_frames[b] (device memory) clamped to [0, L]
__device__ __forceinline__ int pcm_frames(const int* num_frames, int b, int L) { return num_frames ? min(max(num_frames[b], 0), L) : L; }

// E[b, j] = sum of squares over frames [p(j), min(p(j + 1), n_b)) x channels of row b, for the row's own j < M_b = pcm_len_ms(n_b);
// entries at or past M_b are not written (nothing reads them).  The only pass over the samples.  grid (tiles of ept milliseconds,
// B), PCM_THREADS threads.  A workgroup stages its tile's span -- the words [(p(j0) - 0)*C, min(p(j0 + jt), n_b)*C) of the row -- in
// LDS once: whole 16-byte lines of global memory by one 16-byte load each, the words before the first whole line and after the
// last one by one 2-byte load each, so nothing before the row's first word and nothing at or past n_b is read.  The LDS image is
// shifted by the span's offset within its 16-byte line, which makes every 16-byte store to LDS aligned as well.  Sixteen lanes then
// take one millisecond: lane l adds the squares of words l, l + 16, ... and a butterfly joins the sixteen sums.
__global__ __launch_bounds__(PCM_THREADS) void k_pcm_energy(const short* pcm, const int* num_frames, int L, int C, int sr, int ept, int Mmax,
                                                            unsigned long long* E) {
  extern __shared__ __attribute__((aligned(16))) short pcm_lds[];      // [8 + span + 8]
  const int b = blockIdx.y, j0 = blockIdx.x * ept, tid = threadIdx.x;
  const int n = pcm_frames(num_frames, b, L), M = pcm_len_ms(n, sr);
  if (j0 >= M) return;
  const int jt = min(ept, M - j0);
  const long long f0 = min(pcm_frame_of_ms(j0, sr), (long long)n), f1 = min(pcm_frame_of_ms(j0 + jt, sr), (long long)n);
  const short* src = pcm + ((size_t)b * L + (size_t)f0) * C;            // the span's first word
  const int span = (int)(f1 - f0) * C;
  const int shift = (int)((reinterpret_cast<uintptr_t>(src) & 15) >> 1);  // words between the 16-byte line and src
  const int head = min((8 - shift) & 7, span), nvec = (span - head) >> 3, tail0 = head + (nvec << 3);
  short* xs = pcm_lds + shift;                                            // xs[i] = src[i]; xs + head is 16-byte aligned
  for (int i = tid; i < head; i += PCM_THREADS) xs[i] = src[i];
  for (int v = tid; v < nvec; v += PCM_THREADS)
    *reinterpret_cast<uint4*>(xs + head + (v << 3)) = *reinterpret_cast<const uint4*>(src + head + (v << 3));
  for (int i = tail0 + tid; i < span; i += PCM_THREADS) xs[i] = src[i];
  __syncthreads();
  const int sub = tid >> 4, l = tid & 15;
  for (int j = sub; j < jt; j += PCM_THREADS / 16) {
    const long long a = min(pcm_frame_of_ms(j0 + j, sr), (long long)n), e = min(pcm_frame_of_ms(j0 + j + 1, sr), (long long)n);
    const int lo = (int)(a - f0) * C, hi = (int)(e - f0) * C;
    unsigned long long s = 0;
    for (int i = lo + l; i < hi; i += 16) { const int v = xs[i]; s += (unsigned long long)(unsigned)(v * v); }
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
    if (l == 0) E[(size_t)b * Mmax + j0 + j] = s;
  }
}

// The silence flag of every window of W milliseconds on the millisecond grid.  Window i of row b, 0 <= i <= M_b - W, covers
// frames [p(i), p(i + W)) over all channels: S_i = E[i] + ... + E[i + W - 1], c_i = (p(i + W) - p(i))*C samples -- a frame at or past
// n_b is a zero frame that still counts -- and it is silent iff c_i == 0 or S_i < kk*c_i, kk = (k + 1)^2: audioop.rms's
// (unsigned)sqrt(S/c) <= k (and its 0 for an empty fragment) as an integer comparison.  grid (tiles of PCM_W_TILE starts, B).  A
// tile takes its PCM_W_TILE + W energies into LDS (zeros at and past M_b) and turns them into their exclusive prefix sums there --
// every thread its own run of consecutive entries, the 256 run totals through a scan of shuffles and four wave totals -- so
// S_i = P[i + W] - P[i] with no scan across tiles.  silent [B, Mmax] receives the flags of the row's own windows; window_sumsq
// [B, Mmax] (nullable) S_i for them and zeros in every other word.
__global__ __launch_bounds__(PCM_THREADS) void k_pcm_windows(const unsigned long long* E, const int* num_frames, int L, int C, int sr, int W,
                                                             unsigned long long kk, int Mmax, unsigned char* silent,
                                                             unsigned long long* window_sumsq) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long pcm_pre[];      // [PCM_W_TILE + W]
  __shared__ unsigned long long wtot[PCM_THREADS / 64];
  const int b = blockIdx.y, i0 = blockIdx.x * PCM_W_TILE, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = pcm_frames(num_frames, b, L), M = pcm_len_ms(n, sr);
  const int nwin = M >= W ? M - W + 1 : 0, i = i0 + tid;
  if (i0 >= nwin) {                                        // (the whole workgroup: no window of the row starts in this tile)
    if (window_sumsq && i < Mmax) window_sumsq[(size_t)b * Mmax + i] = 0;
    return;
  }
  const int items = PCM_W_TILE + W, q = (items + PCM_THREADS - 1) / PCM_THREADS;
  const unsigned long long* e = E + (size_t)b * Mmax;
  for (int m = tid; m < items; m += PCM_THREADS) pcm_pre[m] = i0 + m < M ? e[i0 + m] : 0ull;
  __syncthreads();
  const int m0 = min(tid * q, items), m1 = min(m0 + q, items);
  unsigned long long run = 0;
  for (int m = m0; m < m1; ++m) run += pcm_pre[m];
  unsigned long long inc = run;                            // inclusive scan of the run totals inside the wave
  for (int o = 1; o < 64; o <<= 1) { const unsigned long long up = __shfl_up(inc, o); if (lane >= o) inc += up; }
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  unsigned long long base = inc - run;
  for (int w = 0; w < wave; ++w) base += wtot[w];
  for (int m = m0; m < m1; ++m) { const unsigned long long v = pcm_pre[m]; pcm_pre[m] = base; base += v; }
  __syncthreads();
  unsigned long long S = 0;
  if (i < nwin) {
    S = pcm_pre[tid + W] - pcm_pre[tid];
    const unsigned long long c = (unsigned long long)(pcm_frame_of_ms((long long)i + W, sr) - pcm_frame_of_ms(i, sr)) * (unsigned long long)C;
    silent[(size_t)b * Mmax + i] = (c == 0 || S < kk * c) ? 1 : 0;
  }
  if (window_sumsq && i < Mmax) window_sumsq[(size_t)b * Mmax + i] = S;
}

// detect_silence and detect_nonsilent of row b from the flags k_pcm_windows wrote, in milliseconds and in order.  pydub joins the
// silent starts into ranges [a, b + W] and opens a new one only at a start a > b_prev + W, b_prev the silent start before it; the
// non-silent ranges are the gaps.  Restated per window start i, with `prev` the last silent start before i (none: -1): i OPENS a
// silent range iff it is silent and (prev is none or i - prev > W), and the non-silent range that ends there is [0, i] for the first
// opening (dropped when i == 0: pydub's removed [0, 0]) and [prev + W, i] for every later one.  After the last window: no silent
// start at all gives [0, M] (also when M < W); otherwise [last + W, M] unless last + W == M.  So every range is written whole by one
// thread from a look BACK alone: prev comes from the ballots of the chunk's four waves and a value carried across the 256-start
// chunks of a long row, the range's position from a prefix count of the openings as k_split_edges counts its edges -- no atomics,
// two calls return the same bits.  counts[b] receives the true number of ranges; only the first max_ranges are written and every
// other word of the row's table is an exact zero.  len_ms[b] (nullable) receives M.  One workgroup per row.
__global__ __launch_bounds__(PCM_THREADS) void k_pcm_ranges(const unsigned char* silent, const int* num_frames, int L, int sr, int W, int Mmax,
                                                            int max_ranges, int* ranges, int* counts, int* len_ms) {
  __shared__ unsigned long long wmask[4];
  __shared__ int wopen[4];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = pcm_frames(num_frames, b, L), M = pcm_len_ms(n, sr);
  const int nwin = M >= W ? M - W + 1 : 0;
  const unsigned char* f = silent + (size_t)b * Mmax;
  int* tab = ranges + (size_t)b * max_ranges * 2;
  long long seen = 0;                                      // ranges of the chunks before this one (the same in every thread)
  int last = -1;                                           // the last silent start of the chunks before this one
  for (int t0 = 0; t0 < nwin; t0 += PCM_THREADS) {
    const int i = t0 + tid;
    const bool s = i < nwin && f[i] != 0;
    const unsigned long long m = __ballot(s);
    if (lane == 0) wmask[wave] = m;
    __syncthreads();
    int prev = last;
    const unsigned long long below = m & ((1ull << lane) - 1);
    if (below) prev = t0 + wave * 64 + 63 - __clzll(below);
    else
      for (int w = wave - 1; w >= 0; --w)
        if (wmask[w]) { prev = t0 + w * 64 + 63 - __clzll(wmask[w]); break; }
    const bool open = s && i > 0 && (prev < 0 || i - prev > W);      // (i == 0 opens the range whose gap [0, 0] pydub removes)
    const unsigned long long om = __ballot(open);
    if (lane == 0) wopen[wave] = __popcll(om);
    __syncthreads();
    long long k = seen + __popcll(om & ((1ull << lane) - 1));
    for (int w = 0; w < wave; ++w) k += wopen[w];
    if (open && k < max_ranges) { tab[2 * k] = prev < 0 ? 0 : prev + W; tab[2 * k + 1] = i; }
    seen += wopen[0] + wopen[1] + wopen[2] + wopen[3];
    for (int w = 3; w >= 0; --w)
      if (wmask[w]) { last = t0 + w * 64 + 63 - __clzll(wmask[w]); break; }
    __syncthreads();                                       // wmask and wopen are rewritten by the next chunk
  }
  if (last < 0 || last + W != M) {                         // the range that runs to the end of the row
    if (tid == 0 && seen < max_ranges) { tab[2 * seen] = last < 0 ? 0 : last + W; tab[2 * seen + 1] = M; }
    seen += 1;
  }
  if (tid == 0) { counts[b] = (int)seen; if (len_ms) len_ms[b] = M; }
  for (long long w = 2 * min(seen, (long long)max_ranges) + tid; w < 2LL * max_ranges; w += PCM_THREADS) tab[w] = 0;
}

// The exact sum of squares and the number of samples of every range of a table [B, max_ranges, 2] in milliseconds, from the energies
// k_pcm_energy wrote: range k of row b = [s, e) clamped to 0 <= s <= e <= M_b has sumsq = E[s] + ... + E[e - 1] -- the frames
// [p(s), p(e)) over all channels, zero frames at or past n_b -- and samples = (p(e) - p(s))*C.  Ranges at or past counts[b] give zeros.
// grid (groups of four ranges, B): a wave per range, lane l adds entries l, l + 64, ..., a butterfly joins them.
__global__ __launch_bounds__(PCM_THREADS) void k_pcm_range_sumsq(const unsigned long long* E, const int* num_frames, int L, int C, int sr, int Mmax,
                                                                 const int* ranges, const int* counts, int max_ranges,
                                                                 unsigned long long* sumsq, long long* samples) {
  const int b = blockIdx.y, k = blockIdx.x * (PCM_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= max_ranges) return;
  const int n = pcm_frames(num_frames, b, L), M = pcm_len_ms(n, sr);
  unsigned long long acc = 0;
  long long c = 0;
  if (k < counts[b]) {
    const int* r = ranges + ((size_t)b * max_ranges + k) * 2;
    const int s = min(max(r[0], 0), M), e = min(max(r[1], s), M);
    const unsigned long long* row = E + (size_t)b * Mmax;
    for (int j = s + lane; j < e; j += 64) acc += row[j];
    c = (pcm_frame_of_ms(e, sr) - pcm_frame_of_ms(s, sr)) * C;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) { sumsq[(size_t)b * max_ranges + k] = acc; samples[(size_t)b * max_ranges + k] = c; }
}

// audioop.mul per range, and the cut app.py's amplify makes: row b of out [B, L_out, C] receives the frames [p(s_0), p(M_b)) of row
// b of pcm -- s_0 the start of its first range; zero frames at or past n_b -- where a sample x of a frame inside range k becomes
// clip(floor((double)x * gains[b, k]), -32768, 32767) and a sample between ranges is copied.  A frame f lies in millisecond
// j(f) = ((f + 1)*1000 - 1) / sr, the largest j with p(j) <= f, so f is inside [p(s), p(e)) iff s <= j(f) < e: the range is found by
// bisection over the row's first min(counts[b], max_ranges) starts, which are in order.  out_frames[b] receives the row's true length
// p(M_b) - p(s_0), 0 without a range; frames past it, and past L_out, are zeros resp. not written.  grid (tiles of 256 frames, B).
__global__ __launch_bounds__(PCM_THREADS) void k_pcm_apply_gains(const short* pcm, const int* num_frames, int L, int C, int sr, const int* ranges,
                                                                 const int* counts, int max_ranges, const double* gains, short* out, int L_out,
                                                                 int* out_frames) {
  const int b = blockIdx.y, fo = blockIdx.x * PCM_THREADS + threadIdx.x;
  const int n = pcm_frames(num_frames, b, L), M = pcm_len_ms(n, sr);
  const int cnt = min(max(counts[b], 0), max_ranges);
  const int* tab = ranges + (size_t)b * max_ranges * 2;
  const long long first = cnt > 0 ? pcm_frame_of_ms(min(max(tab[0], 0), M), sr) : 0;
  const long long len = cnt > 0 ? pcm_frame_of_ms(M, sr) - first : 0;
  if (fo == 0 && out_frames) out_frames[b] = (int)len;
  if (fo >= L_out) return;
  short* y = out + ((size_t)b * L_out + fo) * C;
  const long long f = first + fo;
  if (fo >= len || f >= n) {                               // past the row's output, or a zero frame: floor(0 * g) = 0
    for (int c = 0; c < C; ++c) y[c] = 0;
    return;
  }
  const int j = (int)(((f + 1) * 1000 - 1) / sr);
  int lo = 0, hi = cnt;                                    // the last range with start <= j, if any: lo - 1
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (tab[2 * mid] <= j) lo = mid + 1; else hi = mid; }
  const bool inside = lo > 0 && j < tab[2 * lo - 1];
  const short* x = pcm + ((size_t)b * L + (size_t)f) * C;
  if (!inside) {
    for (int c = 0; c < C; ++c) y[c] = x[c];
    return;
  }
  const double g = gains[(size_t)b * max_ranges + lo - 1];
  for (int c = 0; c < C; ++c) y[c] = (short)fmin(fmax(floor((double)x[c] * g), -32768.0), 32767.0);
}

// Milliseconds per tile of k_pcm_energy: the most, up to PCM_E_MS, whose span fits PCM_E_LDS_WORDS; 0 = not even one
static size_t pcm_energy_span_words(int ept, int C, int sr) { return (size_t)(((long long)ept * sr + 999) / 1000 + 1) * C; }
static int pcm_energy_tile(int C, int sr) {
  int ept = PCM_E_MS;
  while (ept > 0 && pcm_energy_span_words(ept, C, sr) + 16 > PCM_E_LDS_WORDS) --ept;
  return ept;
}
