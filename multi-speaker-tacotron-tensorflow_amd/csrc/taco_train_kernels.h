// taco_train_kernels.h -- training-side kernels that need no backward pass:
//   k_l1_partial / k_loss_final   add_loss (tacotron.py:274-302): coefficient-weighted L1 means
//   k_sumsq_partial + k_adam      clip_by_global_norm(1.0) + tf.train.AdamOptimizer + LR schedule (tacotron.py:305-336)
// All streaming (HBM-bound): 16-byte loads, grid-stride, one partial per workgroup, deterministic final pass.
#pragma once
#include <hip/hip_runtime.h>

#define TR_NT 256
#define TR_MAXBLK 1024

__device__ __forceinline__ double tr_block_sum(double x, double* sm) {
  const int tid = threadIdx.x;
  sm[tid] = x;
  __syncthreads();
  for (int o = TR_NT / 2; o > 0; o >>= 1) { if (tid < o) sm[tid] += sm[tid + o]; __syncthreads(); }
  return sm[0];
}

// partial[blk*4 + {0,1,2}] = sum |a-b|, sum |a-b|*coeff[row/T], sum over the priority band of |a-b|*coeff; [3] = band plain
// a, b: [B*T, C]; band [c_lo, c_hi) (empty when c_lo >= c_hi)
__global__ __launch_bounds__(TR_NT) void k_l1_partial(const float* a, const float* b, const float* coeff, int rows, int T, int C,
                                                     int c_lo, int c_hi, double* partial) {
  __shared__ double sm[TR_NT];
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  const size_t total = (size_t)rows * C;
  for (size_t i = (size_t)blockIdx.x * TR_NT + threadIdx.x; i < total; i += (size_t)gridDim.x * TR_NT) {
    const int row = (int)(i / C), c = (int)(i % C);
    const float d = fabsf(a[i] - b[i]);
    const float w = coeff ? coeff[row / T] : 1.f;
    s0 += d; s1 += (double)d * w;
    if (c >= c_lo && c < c_hi) { s2 += (double)d * w; s3 += d; }
  }
  const double r0 = tr_block_sum(s0, sm); __syncthreads();
  const double r1 = tr_block_sum(s1, sm); __syncthreads();
  const double r2 = tr_block_sum(s2, sm); __syncthreads();
  const double r3 = tr_block_sum(s3, sm);
  if (threadIdx.x == 0) { double* p = partial + (size_t)blockIdx.x * 4; p[0] = r0; p[1] = r1; p[2] = r2; p[3] = r3; }
}

// losses[0..3] = loss, mel_loss, linear_loss, loss_without_coeff
// (one workgroup of TR_NT threads: strided partial sums, then a fixed tree -- deterministic; a single thread walking the 2 x 1024 partials
// one dependent load at a time was 0.2 ms on the step's critical path)
__global__ __launch_bounds__(TR_NT) void k_loss_final(const double* pm, int nbm, const double* pl, int nbl, double n_mel, double n_lin, double n_band,
                                                     int prioritize, float* losses) {
  __shared__ double sm[TR_NT];
  if (blockIdx.x != 0) return;
  double m0 = 0, m1 = 0, l0 = 0, l1 = 0, l2 = 0, l3 = 0;
  for (int i = threadIdx.x; i < nbm; i += TR_NT) { m0 += pm[i * 4]; m1 += pm[i * 4 + 1]; }
  for (int i = threadIdx.x; i < nbl; i += TR_NT) { l0 += pl[i * 4]; l1 += pl[i * 4 + 1]; l2 += pl[i * 4 + 2]; l3 += pl[i * 4 + 3]; }
  m0 = tr_block_sum(m0, sm); __syncthreads(); m1 = tr_block_sum(m1, sm); __syncthreads();
  l0 = tr_block_sum(l0, sm); __syncthreads(); l1 = tr_block_sum(l1, sm); __syncthreads();
  l2 = tr_block_sum(l2, sm); __syncthreads(); l3 = tr_block_sum(l3, sm);
  if (threadIdx.x != 0) return;
  const double mel_loss = m0 / n_mel;
  double loss, lin_loss;
  if (prioritize) {
    loss = m1 / n_mel + 0.5 * l1 / n_lin + 0.5 * l2 / n_band;
    lin_loss = 0.5 * (l0 / n_lin + l3 / n_band);
  } else {
    loss = m1 / n_mel + l1 / n_lin;
    lin_loss = l0 / n_lin;
  }
  losses[0] = (float)loss; losses[1] = (float)mel_loss; losses[2] = (float)lin_loss; losses[3] = (float)(mel_loss + lin_loss);
}

// see taco_train_forward_backward: the sticky device error word -> NaN losses and one NaN gradient element
__global__ void k_train_latch(const unsigned* err, float* losses, float* grads) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && err && err[0] != 0u) {
    const float nan = __uint_as_float(0x7FC00000u);
    if (losses) { losses[0] = nan; losses[1] = nan; losses[2] = nan; losses[3] = nan; }
    if (grads) grads[0] = nan;
  }
}

__global__ __launch_bounds__(TR_NT) void k_sumsq_partial(const float* g, size_t n, double* partial) {
  __shared__ double sm[TR_NT];
  double s = 0;
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * TR_NT + threadIdx.x; i < n4; i += (size_t)gridDim.x * TR_NT) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    s += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { const float v = g[n4 * 4 + threadIdx.x]; s += (double)v * v; }
  const double r = tr_block_sum(s, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// every workgroup re-reduces the (<= TR_MAXBLK) partials -> global norm; then the fused clip + Adam update.
// TF form (A.14): lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m = b1*m+(1-b1)*g; v = b2*v+(1-b2)*g^2; p -= lr_t*m/(sqrt(v)+eps)
__global__ __launch_bounds__(TR_NT) void k_adam(float* p, const float* g, float* m, float* v, size_t n, const double* partial,
                                               int nblk, float lr_t, float b1, float b2, float eps, float clip, float* gnorm_out) {
  __shared__ double sm[TR_NT];
  double s = 0;
  for (int i = threadIdx.x; i < nblk; i += TR_NT) s += partial[i];
  const double gn = sqrt(tr_block_sum(s, sm));
  const float scale = (float)((double)clip / fmax(gn, (double)clip));      // tf.clip_by_global_norm
  if (blockIdx.x == 0 && threadIdx.x == 0 && gnorm_out) *gnorm_out = (float)gn;
  // a non-finite global norm (a gradient poisoned by k_train_latch after a device fault, or a genuine overflow) skips the update:
  // parameters and moments stay as they are.  (tf.clip_by_global_norm would turn every parameter into NaN here; nothing can be
  // learned from such a step either way, and a data-parallel job stays consistent because all ranks see the same reduced norm.)
  if (!(gn < 1.7976931348623157e308)) return;
  for (size_t i = (size_t)blockIdx.x * TR_NT + threadIdx.x; i < n; i += (size_t)gridDim.x * TR_NT) {
    const float gi = g[i] * scale;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) + eps);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Segmented sum of squares over a flat fp32 buffer: per-variable gradient norms, their maximum and the global norm
// (the 'train' branch of add_stats, train.py:50-77: max_gradient_norm = reduce_max([tf.norm(g) for g in model.gradients])).
// Caveat: train.py:156 calls add_stats(model, scope_name='stats'), so in the reference as run that branch never executes; the function
// is reproduced as it stands (as the speaker-mixture branch that never ran was), and 'train' is the useful scope.
// Work table (taco_segnorm.h, built on the host once per plan): ascending pieces of at most SEGN_P floats, none across a segment
// boundary, none inside a skipped segment.  Three launches, the buffer read once by the first:
//   k_segsq_piece     one workgroup per piece      -> one double partial per piece
//   k_segsq_segment   one wave per segment         -> the segment's double sum (its pieces in ascending order, lane-strided, fixed
//                                                     shuffle tree: no thread walks a list alone, cf. k_loss_final) and its fp32 norm
//   k_segnorm_stats   one workgroup                -> max norm, its index, the norm over all counted segments
// Squares and sums are doubles (an fp32 product is exact in double); every order of summation is fixed by the table and the
// launch shapes, nothing is accumulated through atomics: the same input gives the same bits on every call, stream and graph replay.
// ---------------------------------------------------------------------------------------------------------------
#define SEGN_P 4096                        // floats per piece (taco_segnorm_piece_floats)
#define SEGN_V (SEGN_P / 4 / TR_NT)        // 16-byte loads per thread that cover a whole piece
struct SegPiece { unsigned long long begin; int len; int seg; };      // elements [begin, begin + len) of segment seg, len in [1, SEGN_P]

__device__ __forceinline__ double segn_wave_sum(double x) {            // fixed tree over the 64 lanes; the total is in lane 0
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  return x;
}

// The piece's 16-byte-aligned interior goes through 16-byte loads (all of a thread's loads issued before the first use), the up to 3
// elements in front of it and behind it through scalar loads: variable offsets are no multiples of 4 (biases, scalars, 1025-wide rows).
__global__ __launch_bounds__(TR_NT) void k_segsq_piece(const float* __restrict__ x, const SegPiece* __restrict__ pieces, double* __restrict__ partial) {
  __shared__ double sm[TR_NT / 64];
  const SegPiece pc = pieces[blockIdx.x];
  const float* p = x + pc.begin;
  const int tid = threadIdx.x;
  const int head = min(pc.len, (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u));
  const int nv = (pc.len - head) >> 2, tail = (pc.len - head) & 3;
  const float4* q = reinterpret_cast<const float4*>(p + head);
  float4 v[SEGN_V];
#pragma unroll
  for (int k = 0; k < SEGN_V; ++k) {
    const int i = tid + k * TR_NT;
    v[k] = i < nv ? q[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float e0 = 0.f, e1 = 0.f;
  if (tid < head) e0 = p[tid];
  if (tid < tail) e1 = p[head + 4 * nv + tid];
  double s = 0;
#pragma unroll
  for (int k = 0; k < SEGN_V; ++k)
    s += (double)v[k].x * v[k].x + (double)v[k].y * v[k].y + (double)v[k].z * v[k].z + (double)v[k].w * v[k].w;
  s += (double)e0 * e0 + (double)e1 * e1;
  s = segn_wave_sum(s);
  if ((tid & 63) == 0) sm[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double r = sm[0];
    for (int w = 1; w < TR_NT / 64; ++w) r += sm[w];
    partial[blockIdx.x] = r;
  }
}

// pfirst[s] .. pfirst[s + 1]: the pieces of segment s (none: an empty or a skipped segment, whose sum and norm are 0).
// A norm beyond the fp32 range becomes +inf in the conversion.
__global__ __launch_bounds__(TR_NT) void k_segsq_segment(const double* __restrict__ partial, const int* __restrict__ pfirst, int n_seg,
                                                        double* __restrict__ segsum, float* __restrict__ norms) {
  const int s = blockIdx.x * (TR_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= n_seg) return;
  const int a = pfirst[s], b = pfirst[s + 1];
  double acc = 0;
  for (int i = a + lane; i < b; i += 64) acc += partial[i];
  acc = segn_wave_sum(acc);
  if (lane == 0) { segsum[s] = acc; norms[s] = (float)sqrt(acc); }
}

// stats[0] = the largest norm of a counted (not skipped) segment, *argmax = its index: ties go to the first index; if any counted
// norm is NaN the maximum is NaN and the index is that of the first NaN segment -- a step poisoned by k_train_latch (NaN in
// grads[0]) stays visible, where tf.reduce_max's treatment of NaN is unspecified and not imitated.  stats[1] = sqrt of the sum of
// the counted segments' sums.  No counted segment at all: 0, 0 and index -1.
__global__ __launch_bounds__(TR_NT) void k_segnorm_stats(const double* __restrict__ segsum, const float* __restrict__ norms,
                                                        const unsigned char* __restrict__ skip, int n_seg, float* __restrict__ stats,
                                                        int* __restrict__ argmax) {
  __shared__ double sm[TR_NT];
  __shared__ float bv[TR_NT];
  __shared__ int bi[TR_NT], ni[TR_NT];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x, none = 0x7fffffff;
  double tot = 0;
  float best = 0.f; int besti = none, nani = none;
  for (int s = tid; s < n_seg; s += TR_NT) {
    if (skip[s]) continue;
    tot += segsum[s];
    const float v = norms[s];
    if (v != v) { if (nani == none) nani = s; }
    else if (besti == none || v > best) { best = v; besti = s; }
  }
  tot = tr_block_sum(tot, sm);
  bv[tid] = best; bi[tid] = besti; ni[tid] = nani;
  __syncthreads();
  for (int o = TR_NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      ni[tid] = min(ni[tid], ni[tid + o]);
      const float v = bv[tid + o]; const int i = bi[tid + o];
      if (i != none && (bi[tid] == none || v > bv[tid] || (v == bv[tid] && i < bi[tid]))) { bv[tid] = v; bi[tid] = i; }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const bool anynan = ni[0] != none;
  stats[0] = anynan ? __uint_as_float(0x7FC00000u) : (bi[0] == none ? 0.f : bv[0]);
  stats[1] = (float)sqrt(tot);
  if (argmax) *argmax = anynan ? ni[0] : (bi[0] == none ? -1 : bi[0]);
}
