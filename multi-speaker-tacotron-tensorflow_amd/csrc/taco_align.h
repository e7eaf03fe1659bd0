// taco_align.h -- matching recognised text to script lines on the GPU: the matched-character count M of
// difflib.SequenceMatcher(None, a, b).ratio() = 2*M/(len(a)+len(b)), which recognition/alignment.py:21-26 evaluates for every
// (script line, recognised utterance) pair, and the top-two decision of :107-113.  Included from taco_lib.hip.
//
// M is Ratcliff/Obershelp: take the longest common substring of a[alo:ahi] and b[blo:bhi], add its length, do the same to the piece
// left of it in both strings and to the piece right of it.  Among the longest blocks difflib takes the one that starts earliest in a,
// among those the one that starts earliest in b; M depends on that rule.  Restated densely: L[i][j] = L[i-1][j-1] + 1 where
// a[i] == b[j], else 0, evaluated inside the current sub-rectangle only (a run never crosses alo or blo), the best taken as largest L,
// then smallest start in a, then smallest start in b.  tests/align_reference.py is that restatement in NumPy.
//
// The restatement equals difflib for len(b) <= 199.  From len(b) = 200 on difflib's autojunk drops the characters of b that occur more
// than 1 + len(b)/100 times from its index, and the two part ways; such pairs are refused (-1), not approximated.
//
// k_text_matches<COLS>: one wavefront per pair, TA_WAVES independent waves per workgroup and no workgroup barrier.  Lane l holds the COLS
// consecutive columns j = l*COLS + c of b, so the diagonal L[i-1][j-1] is the lane's own register for c > 0 and ONE shift by a lane per
// row for c = 0 (DPP wave_shr:1; lane 0 receives 0, which is the column left of b).  The wave walks the rows of a; a[i] is wave-uniform: 64
// rows are loaded by the 64 lanes at once and handed out with v_readlane.  Per row and column: a compare, the shifted add, two selects
// for the run and three for the lane's best -- VALU and cross-lane issue, no memory.  A lane keeps its best under strict '>' with the
// rows ascending and its columns ascending, which orders equal lengths by start in a, then start in b; the wave then takes the maximum
// of a packed key (length, then the complements of the two starts).  Pending sub-rectangles sit on a per-wave stack in LDS; they have
// non-empty, disjoint ranges of b, so len(b) entries suffice.  a has no length cap (its bounds are 32-bit; b's pack into one word).
#pragma once

#define TA_WAVES 4                 // pairs per workgroup of k_text_matches, groups per workgroup of k_text_best_two
#define TA_BMAX 199                // longest b the device scores (difflib's autojunk starts at 200)
#define TA_STACK (TA_BMAX + 1)     // stack entries per wave; 3 words each: 9.4 KB of LDS per workgroup
#define TA_WIDE 4                  // columns per lane of the wide instantiation: 256 >= TA_BMAX

__device__ __forceinline__ int ta_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// lane l gets lane l-1's value, lane 0 gets 0
__device__ __forceinline__ int ta_from_left(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, true); }

// the pool ranges [*a0, *a1) and [*b0, *b1) of pair p, or false where the pair is to be refused: a text index outside [0, n_texts),
// offsets that decrease or leave the pool
__device__ __forceinline__ bool ta_ranges(const int* offsets, int n_texts, long long n_chars, const int* pairs, long long p, int* a0, int* a1,
                                          int* b0, int* b1) {
  const int ia = ta_uniform(pairs[2 * p]), ib = ta_uniform(pairs[2 * p + 1]);
  if (ia < 0 || ia >= n_texts || ib < 0 || ib >= n_texts) return false;
  *a0 = ta_uniform(offsets[ia]); *a1 = ta_uniform(offsets[ia + 1]);
  *b0 = ta_uniform(offsets[ib]); *b1 = ta_uniform(offsets[ib + 1]);
  return *a0 >= 0 && *a0 <= *a1 && *a1 <= n_chars && *b0 >= 0 && *b0 <= *b1 && *b1 <= n_chars;
}

// Scores the pairs whose len(b) lies in [lb_lo, lb_hi] (lb_hi <= 64*COLS and <= TA_BMAX); the launch with lb_lo == 0 also writes the -1 of
// every refused pair.  Two launches with complementary ranges write every element of matches exactly once.
template <int COLS>
__global__ __launch_bounds__(TA_WAVES * 64) void k_text_matches(const int* __restrict__ chars, long long n_chars, const int* __restrict__ offsets,
                                                                int n_texts, const int* __restrict__ pairs, int n_pairs, int* __restrict__ matches,
                                                                int lb_lo, int lb_hi) {
  __shared__ unsigned stk[TA_WAVES][TA_STACK][3];     // alo, ahi, blo | bhi << 16
  const int lane = threadIdx.x & 63, wave = ta_uniform(threadIdx.x >> 6);
  const long long p = (long long)blockIdx.x * TA_WAVES + wave;
  if (p >= n_pairs) return;
  int a0 = 0, a1 = 0, b0 = 0, b1 = 0;
  const bool ok = ta_ranges(offsets, n_texts, n_chars, pairs, p, &a0, &a1, &b0, &b1) && b1 - b0 <= TA_BMAX;
  if (!ok) {
    if (lb_lo == 0 && lane == 0) matches[p] = -1;
    return;
  }
  const int la = a1 - a0, lb = b1 - b0;
  if (lb < lb_lo || lb > lb_hi) return;
  const int* a = chars + a0;
  int bch[COLS];
#pragma unroll
  for (int c = 0; c < COLS; ++c) {
    const int j = lane * COLS + c;
    bch[c] = j < lb ? chars[(size_t)b0 + j] : 0;
  }
  int M = 0, sp = 0;
  int alo = 0, ahi = la, blo = 0, bhi = lb;
  bool more = la > 0 && lb > 0;
  while (more) {
    bool col[COLS];                                   // columns outside [blo, bhi) never match: what lies next to the range stays out
    int run[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
      const int j = lane * COLS + c;
      col[c] = j >= blo && j < bhi;
      run[c] = 0;
    }
    int bestL = 0, bestI = 0, bestJ = 0;
    for (int base = alo, n = 0; base < ahi; base += n) {
      n = min(64, ahi - base);
      const int av = lane < n ? a[(size_t)base + lane] : 0;
      for (int r = 0; r < n; ++r) {
        const int ai = __builtin_amdgcn_readlane(av, r), i = base + r;
        const int left = ta_from_left(run[COLS - 1]);
#pragma unroll
        for (int c = COLS - 1; c > 0; --c) run[c] = (col[c] && bch[c] == ai) ? run[c - 1] + 1 : 0;
        run[0] = (col[0] && bch[0] == ai) ? left + 1 : 0;
#pragma unroll
        for (int c = 0; c < COLS; ++c)
          if (run[c] > bestL) { bestL = run[c]; bestI = i; bestJ = lane * COLS + c; }
      }
    }
    // largest length, then smallest start in a, then smallest start in b: the maximum of one packed key
    unsigned long long key = 0;
    if (bestL > 0)
      key = ((unsigned long long)bestL << 40) | ((unsigned long long)(0x7fffffff - (bestI - bestL + 1)) << 8) |
            (unsigned long long)(255 - (bestJ - bestL + 1));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_xor(key, d, 64);
      key = o > key ? o : key;
    }
    const int L = ta_uniform((int)(key >> 40));
    int nalo = 0, nahi = 0, nblo = 0, nbhi = 0;
    bool have = false;
    if (L > 0) {
      const int si = 0x7fffffff - ta_uniform((int)((key >> 8) & 0x7fffffffu)), sj = 255 - ta_uniform((int)(key & 255u));
      M += L;
      const bool lft = si > alo && sj > blo, rgt = si + L < ahi && sj + L < bhi;
      if (lft && rgt) {                               // the right piece waits; at most len(b) wait at a time
        if (lane == 0) {
          stk[wave][sp][0] = (unsigned)(si + L);
          stk[wave][sp][1] = (unsigned)ahi;
          stk[wave][sp][2] = (unsigned)(sj + L) | ((unsigned)bhi << 16);
        }
        ++sp;
      }
      if (lft) { nalo = alo; nahi = si; nblo = blo; nbhi = sj; have = true; }
      else if (rgt) { nalo = si + L; nahi = ahi; nblo = sj + L; nbhi = bhi; have = true; }
    }
    if (!have && sp > 0) {
      --sp;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // lane 0's entries, read by every lane of the same wave
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const unsigned e0 = stk[wave][sp][0], e1 = stk[wave][sp][1], e2 = stk[wave][sp][2];
      nalo = ta_uniform((int)e0); nahi = ta_uniform((int)e1);
      nblo = ta_uniform((int)(e2 & 0xffffu)); nbhi = ta_uniform((int)(e2 >> 16));
      have = true;
    }
    alo = nalo; ahi = nahi; blo = nblo; bhi = nbhi;
    more = have;
  }
  if (lane == 0) matches[p] = M;
}

// 2*M/T as the fraction rm/rt in lowest-effort form: T == 0 (both texts empty) is ratio 1 = 2*1/2
__device__ __forceinline__ void ta_ratio(int m, long long T, unsigned long long* rm, unsigned long long* rt) {
  *rm = T == 0 ? 1ull : (unsigned long long)m;
  *rt = T == 0 ? 2ull : (unsigned long long)T;
}

// M and T = len(a) + len(b) of pair p, or false for a refused pair (M < 0, or ranges ta_ranges refuses)
__device__ __forceinline__ bool ta_scored(const int* matches, const int* pairs, const int* offsets, int n_texts, long long p, int* m, long long* T) {
  *m = matches[p];
  const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
  if (*m < 0 || ia < 0 || ia >= n_texts || ib < 0 || ib >= n_texts) return false;
  const long long la = (long long)offsets[ia + 1] - offsets[ia], lb = (long long)offsets[ib + 1] - offsets[ib];
  *T = la + lb;
  return la >= 0 && lb >= 0;
}

// One wave per group (the pairs [group_offsets[g], group_offsets[g+1]) of one utterance): best[g] = {pair of the largest ratio (the first
// such pair), its M, its T, 1 if every other pair's ratio is strictly smaller and the group holds no refused pair}.  Ratios 2*M/T compare
// as M1*T2 against M2*T1 in 64-bit integers.  An empty group, or one whose pairs are all refused, gives {-1, 0, 0, 0}.
__global__ __launch_bounds__(TA_WAVES * 64) void k_text_best_two(const int* __restrict__ matches, const int* __restrict__ pairs,
                                                                 const int* __restrict__ offsets, int n_texts, const int* __restrict__ group_offsets,
                                                                 int n_groups, int* __restrict__ best) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * TA_WAVES + ta_uniform(threadIdx.x >> 6);
  if (g >= n_groups) return;
  const long long p0 = ta_uniform(group_offsets[g]), p1 = ta_uniform(group_offsets[g + 1]);
  unsigned long long bm = 0, bt = 1;
  long long bp = -1;
  bool refused = false;
  for (long long p = p0 + lane; p0 >= 0 && p < p1; p += 64) {
    int m; long long T;
    if (!ta_scored(matches, pairs, offsets, n_texts, p, &m, &T)) { refused = true; continue; }
    unsigned long long rm, rt;
    ta_ratio(m, T, &rm, &rt);
    if (bp < 0 || rm * bt > bm * rt) { bm = rm; bt = rt; bp = p; }       // strict: the first pair of equal ratios stays
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long om = __shfl_xor(bm, d, 64), ot = __shfl_xor(bt, d, 64);
    const long long op = __shfl_xor(bp, d, 64);
    const bool take = op >= 0 && (bp < 0 || om * bt > bm * ot || (om * bt == bm * ot && op < bp));
    if (take) { bm = om; bt = ot; bp = op; }
  }
  bool rival = false;                                 // another pair whose ratio is not strictly smaller
  for (long long p = p0 + lane; bp >= 0 && p < p1; p += 64) {
    int m; long long T;
    if (p == bp || !ta_scored(matches, pairs, offsets, n_texts, p, &m, &T)) continue;
    unsigned long long rm, rt;
    ta_ratio(m, T, &rm, &rt);
    rival = rival || rm * bt >= bm * rt;
  }
  const bool spoiled = __any(rival || refused);
  if (lane == 0) {
    int m = 0; long long T = 0;
    if (bp >= 0) (void)ta_scored(matches, pairs, offsets, n_texts, bp, &m, &T);
    best[4 * g + 0] = (int)bp;
    best[4 * g + 1] = bp >= 0 ? m : 0;
    best[4 * g + 2] = bp >= 0 ? (int)T : 0;
    best[4 * g + 3] = bp >= 0 && !spoiled ? 1 : 0;
  }
}
