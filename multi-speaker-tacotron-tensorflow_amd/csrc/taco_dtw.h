// taco_dtw.h -- dynamic time warping of two feature sequences on the GPU: the cost of the cheapest monotone alignment of A[p, :n] and
// Bm[p, :m], normalised by n + m, with the direction map and the warping path as optional outputs.  Not in the reference: it is the number
// that says how far a free-running decoder's mel frames are from their targets once the drift in time is taken out (tacotron.py:274-302
// compares frame t with frame t).  Included from taco_lib.hip; tests/dtw_reference.py is the definition in float64 NumPy.
//
// Frame cost c(i, j), summed over d ascending in fp32: kind 0 (1/D) * sum |a - b|, kind 1 sqrt(sum (a - b)^2) (the squares by fmaf).
// Symmetric step pattern, diagonal weight 2:  G(i,j) = min(G(i-1,j-1) + 2c, G(i-1,j) + c, G(i,j-1) + c), G(0,0) = 2c(0,0); the diagonal is
// tried first, then (i-1,j), then (i,j-1), a later candidate wins under strict '<' only.  total = G(n-1,m-1), dist = total / (n + m).
//
// k_dtw<DP>: one workgroup of DTW_NT threads per pair (the grid loops over pairs), walking anti-diagonals.  Thread t of a strip owns the
// DTW_COLS consecutive columns j = j0 + t * DTW_COLS + c of Bm with their D features in registers (DP = D rounded up to 16, the pad is 0
// on both sides and adds exact zeros); at step s it handles row i = s - t of them, left to right, from ONE read of row i of A.  For its
// first column G(i,j-1) is the left lane's last column of the step before and G(i-1,j-1) the one of two steps before: one DPP shift per
// step (ta_from_left) and a register that remembers the last shift; everything else a cell needs is the lane's own.  Across the wave seams
// lane 63 of a wave leaves its last column in LDS (two buffers by step parity) for lane 0 of the next wave; one workgroup barrier per step
// orders that.  The barrier and the hand-off are what a step costs at small D (profiles/r22_dtw.json), which is why a lane takes two
// columns: half the steps for a given Tb, and half the LDS reads per cell.  No cost matrix exists: costs are formed on the fly and G
// lives in registers as the rolling anti-diagonal.
//
// The rows of A pass through an LDS ring of DTW_NT + DTW_CH rows, DTW_CH rows staged at a time with coalesced loads.  Row stride DP + 4
// words: rows stay 16-byte aligned for ds_read_b128 and (DP + 4) / 4 is odd, so the 16 lanes that one LDS cycle serves, which read 16
// consecutive rows, cover all 64 banks.  DP = 128 takes 152 KB of the 160 KB of a CU.
//
// Tb beyond DTW_STRIP columns runs as strips one after the other.  The last column of a strip, G(i, j0 + DTW_STRIP - 1) for every i, goes
// to the workspace ([B, Ta] floats) and the next strip reads it back DTW_CH rows at a time with the rows of A; a row is read before the
// same strip overwrites it DTW_NT - 1 steps later.  Ta and Tb have no cap.
//
// Non-finite input: every used element is tested where it is loaded; the flag is OR-ed over the workgroup and turns the pair's total
// and dist into NaN.  The recurrence is not relied on to carry it.  Slack past the lengths is never loaded.
//
// k_dtw_path: one wave per pair.  Lane 0 walks dir backwards from (n-1, m-1), writing from the end of the pair's path rows; the wave
// then moves the entries to the front and fills the rest with -1.  Every move lowers i + j and stays in the rectangle whatever the
// byte says (above 2 counts as 0; in row 0 the move is (i, j-1), in column 0 (i-1, j)), so n + m - 1 entries bound the walk.
#pragma once

#define DTW_NT 256                        // threads of k_dtw
#define DTW_WAVES (DTW_NT / 64)
#define DTW_COLS 2                        // columns of Bm per thread
#define DTW_STRIP (DTW_NT * DTW_COLS)     // columns of a strip
#define DTW_CH 32                         // rows of A staged at a time (a power of two)
#define DTW_ROWS (DTW_NT + DTW_CH)        // rows of the LDS ring: a row leaves DTW_NT - 1 steps after it came
#define DTW_DSTEP 16                      // D is rounded up to a multiple of this
#define DTW_DMAX 128                      // largest D: DTW_COLS * 128 feature registers per lane, and the ring of DP = 128 is 152 KB
#define DTW_MAXGRID 4096                  // workgroups of either kernel; they loop over the pairs beyond

static size_t dtw_lds_bytes(int DP) { return ((size_t)DTW_ROWS * (DP + 4) + DTW_CH + 2 * DTW_WAVES + 4) * sizeof(float); }

__device__ __forceinline__ float dtw_from_left(float v) { return __int_as_float(ta_from_left(__float_as_int(v))); }
__device__ __forceinline__ bool dtw_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
// the length of pair p clamped to [1, T]; a null array means full rows
__device__ __forceinline__ int dtw_len(const int* len, long long p, int T) { return len ? min(max(len[p], 1), T) : T; }

template <int DP>
__global__ __launch_bounds__(DTW_NT) void k_dtw(const float* __restrict__ A, const int* __restrict__ len_a, const float* __restrict__ Bm,
                                                const int* __restrict__ len_b, int B, int Ta, int Tb, int D, int cost_kind,
                                                float* __restrict__ dist, float* __restrict__ total, unsigned char* __restrict__ dir,
                                                float* seam) {
  constexpr int LD = DP + 4;
  extern __shared__ __attribute__((aligned(16))) float dtw_lds[];
  float* ring = dtw_lds;                        // [DTW_ROWS][LD]: row i of A at slot i % DTW_ROWS
  float* bnd = ring + DTW_ROWS * LD;            // [DTW_CH]: G(i, j0 - 1) of the staged rows, +inf in the first strip
  float* wlast = bnd + DTW_CH;                  // [2][DTW_WAVES]: lane 63's last column of the step, by step parity
  float* res = wlast + 2 * DTW_WAVES;           // G(n-1, m-1)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inf = __builtin_inff();
  for (int e = tid; e < DTW_ROWS * LD; e += DTW_NT) ring[e] = 0.f;      // the pad columns d >= D stay 0 from here on
  const float inv_d = 1.0f / (float)D;
  for (long long p = blockIdx.x; p < B; p += gridDim.x) {
    const int n = dtw_len(len_a, p, Ta), m = dtw_len(len_b, p, Tb);
    const float* a = A + (size_t)p * Ta * D;
    const float* bp = Bm + (size_t)p * Tb * D;
    bool bad = false;
    for (int j0 = 0; j0 < m; j0 += DTW_STRIP) {
      const int jb = j0 + tid * DTW_COLS;         // the lane's first column
      float b[DTW_COLS][DP];
#pragma unroll
      for (int c = 0; c < DTW_COLS; ++c) {
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const float v = (jb + c < m && d < D) ? bp[(size_t)(jb + c) * D + d] : 0.f;
          bad = bad || !dtw_finite(v);
          b[c][d] = v;
        }
      }
      if (tid < 2 * DTW_WAVES) wlast[tid] = inf;
      const int nsteps = n + (min(DTW_STRIP, m - j0) + DTW_COLS - 1) / DTW_COLS - 1;      // rows + lanes with a column - 1
      const bool hand = j0 + DTW_STRIP < m;       // another strip follows: the last column goes to the workspace
      float g[DTW_COLS], left1 = inf;
#pragma unroll
      for (int c = 0; c < DTW_COLS; ++c) g[c] = inf;
      int slot = tid == 0 ? 0 : DTW_ROWS - tid;   // (0 - tid) mod DTW_ROWS
      __syncthreads();                            // the zero fill, wlast, and the reads of the strip before
      for (int s = 0; s < nsteps; ++s) {
        if ((s & (DTW_CH - 1)) == 0) {            // rows s .. s + DTW_CH - 1: their slots held rows last read at step s - 2
          const int cnt = min(DTW_CH, n - s) * D;
          for (int e = tid; e < cnt; e += DTW_NT) {
            const int r = e / D;
            const float v = a[(size_t)s * D + e];
            bad = bad || !dtw_finite(v);
            ring[((s + r) % DTW_ROWS) * LD + (e - r * D)] = v;
          }
          if (tid < DTW_CH) bnd[tid] = (j0 > 0 && s + tid < n) ? seam[(size_t)p * Ta + s + tid] : inf;
          __syncthreads();
        }
        const int i = s - tid;
        const bool rowok = i >= 0 && i < n;
        const float4* ar = reinterpret_cast<const float4*>(ring + slot * LD);
        float cst[DTW_COLS];
#pragma unroll
        for (int c = 0; c < DTW_COLS; ++c) cst[c] = 0.f;
        if (cost_kind == 0) {
#pragma unroll
          for (int q = 0; q < DP / 4; ++q) {
            const float4 v = ar[q];
#pragma unroll
            for (int c = 0; c < DTW_COLS; ++c) {
              cst[c] += fabsf(v.x - b[c][4 * q]);
              cst[c] += fabsf(v.y - b[c][4 * q + 1]);
              cst[c] += fabsf(v.z - b[c][4 * q + 2]);
              cst[c] += fabsf(v.w - b[c][4 * q + 3]);
            }
          }
#pragma unroll
          for (int c = 0; c < DTW_COLS; ++c) cst[c] *= inv_d;
        } else {
#pragma unroll
          for (int q = 0; q < DP / 4; ++q) {
            const float4 v = ar[q];
#pragma unroll
            for (int c = 0; c < DTW_COLS; ++c) {
              const float t0 = v.x - b[c][4 * q], t1 = v.y - b[c][4 * q + 1], t2 = v.z - b[c][4 * q + 2], t3 = v.w - b[c][4 * q + 3];
              cst[c] = fmaf(t0, t0, cst[c]);
              cst[c] = fmaf(t1, t1, cst[c]);
              cst[c] = fmaf(t2, t2, cst[c]);
              cst[c] = fmaf(t3, t3, cst[c]);
            }
          }
#pragma unroll
          for (int c = 0; c < DTW_COLS; ++c) cst[c] = sqrtf(cst[c]);
        }
        float fl = dtw_from_left(g[DTW_COLS - 1]);      // G(i, jb-1): the left lane's last column of the step before
        if (lane == 0) fl = wave == 0 ? bnd[s & (DTW_CH - 1)] : wlast[((s + 1) & 1) * DTW_WAVES + wave - 1];
        float diag = (i == 0 && jb == 0) ? 0.f : left1; // G(i-1, jb-1): what the shift brought a step ago
        left1 = fl;
        float lf = fl;
#pragma unroll
        for (int c = 0; c < DTW_COLS; ++c) {            // left to right: a column's new value is the next one's left neighbour
          const float up = g[c];                        // G(i-1, j), and the next column's diagonal
          float best = diag + 2.f * cst[c];
          int dr = 0;
          const float vu = up + cst[c], vl = lf + cst[c];
          if (vu < best) { best = vu; dr = 1; }
          if (vl < best) { best = vl; dr = 2; }
          if (rowok && jb + c < m) {
            g[c] = best;
            if (dir) dir[((size_t)p * Ta + i) * Tb + jb + c] = (unsigned char)dr;
          }
          diag = up;
          lf = g[c];
        }
        if (hand && tid == DTW_NT - 1 && rowok) seam[(size_t)p * Ta + i] = g[DTW_COLS - 1];
        if (lane == 63) wlast[(s & 1) * DTW_WAVES + wave] = g[DTW_COLS - 1];
        slot = slot + 1 == DTW_ROWS ? 0 : slot + 1;
        __syncthreads();
      }
#pragma unroll
      for (int c = 0; c < DTW_COLS; ++c)
        if (jb + c == m - 1) res[0] = g[c];
    }
    const int anybad = __syncthreads_or(bad ? 1 : 0);
    if (tid == 0) {
      const float tot = anybad ? __builtin_nanf("") : res[0];
      if (total) total[p] = tot;
      dist[p] = tot / (float)(n + m);
    }
  }
}

__global__ __launch_bounds__(64) void k_dtw_path(const unsigned char* __restrict__ dir, const int* __restrict__ len_a,
                                                 const int* __restrict__ len_b, int B, int Ta, int Tb, int* path, int* __restrict__ path_len) {
  const int lane = threadIdx.x;
  const int cap = Ta + Tb - 1;
  for (long long p = blockIdx.x; p < B; p += gridDim.x) {
    const int n = dtw_len(len_a, p, Ta), m = dtw_len(len_b, p, Tb);
    int2* out = reinterpret_cast<int2*>(path) + (size_t)p * cap;
    int L = 0;
    if (lane == 0) {
      const unsigned char* dp = dir + (size_t)p * Ta * Tb;
      int i = n - 1, j = m - 1;
      for (int k = 0; k < n + m - 1; ++k) {
        out[cap - 1 - k] = make_int2(i, j);
        L = k + 1;
        if (i == 0 && j == 0) break;
        int d = dp[(size_t)i * Tb + j];
        if (d > 2) d = 0;
        if (i == 0) d = 2;
        else if (j == 0) d = 1;
        if (d != 2) --i;
        if (d != 1) --j;
      }
    }
    L = __shfl(L, 0, 64);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // lane 0's entries, read by every lane of the wave
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const int shift = cap - L;
    if (shift > 0) {                                              // to the front: a round reads 64 entries, then writes them lower down
      for (int base = 0; base < L; base += 64) {
        const int k = base + lane;
        int2 v = make_int2(-1, -1);
        if (k < L) v = out[k + shift];
        if (k < L) out[k] = v;
      }
      for (int k = L + lane; k < cap; k += 64) out[k] = make_int2(-1, -1);
    }
    if (lane == 0) path_len[p] = L;
  }
}

// host: one launch of k_dtw<DP> on st (the entry point taco_dtw in taco_dtw_api.h picks DP)
template <int DP>
static int dtw_launch(hipStream_t st, const float* d_a, const int32_t* d_len_a, const float* d_b, const int32_t* d_len_b, int B, int Ta, int Tb,
                      int D, int cost_kind, float* d_dist, float* d_total, uint8_t* d_dir, float* seam) {
  const size_t lds = dtw_lds_bytes(DP);
  // > 64 KB of dynamic LDS has to be asked for, per kernel and device; there is no handle to do it in, so the first call on a device does
  static unsigned long long asked = 0;      // one bit per device ordinal (setting it twice is harmless)
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev >= 64 || !(asked >> dev & 1)) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dtw<DP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (dev < 64) asked |= 1ull << dev;
  }
  hipLaunchKernelGGL(k_dtw<DP>, dim3((unsigned)std::min(B, DTW_MAXGRID)), dim3(DTW_NT), lds, st, d_a, d_len_a, d_b, d_len_b, B, Ta, Tb, D,
                     cost_kind, d_dist, d_total, d_dir, seam);
  HIPCHK(hipGetLastError());
  return 0;
}
