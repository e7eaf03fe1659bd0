// taco_xchg.h -- what the whole-chip persistent kernels share: k_decoder_xcd (taco_decoder_xcd.h), k_decoder_bwd_xcd (taco_decoder_bwd_xcd.h),
// k_bigru_duo / k_bigru_oct and their backward twins (taco_bigru_xcd.h), and the micro-benchmarks tools/ubench_rowsets, ubench_mfma_stage and
// ubench_mfma_scan.  Nothing here knows a model layer: register maps, LDS layouts and stage code live with their kernel.
//
// The exchange.  256 workgroups of 512 threads, one per CU; the 32 CUs of one XCD form a group.  Between two stages of a step the members of a group
// hand each other their column slices through the XCD's own L2 as 8-byte {value, tag = step + 1} granules -- the data is the flag: the producer
// stores (dx_publish*), the consumer polls with L1-bypassing loads until every granule it needs carries the step's tag (dx_poll*, dx_gather*: into
// LDS; XgPoll / xg_*: a gather whose loads are requested a compute phase ahead).  When every XCD hosts exactly one group -- dx_census counts
// HW_REG_XCC_ID at the start of the launch -- the stores stay in the shared L2 (sc0); otherwise, or with force_wt, they are write-through (sc1)
// and the protocol holds for any placement (MI355X_MICROARCH.md, inter-workgroup visibility).  Every spin is bounded: a timeout raises the
// launch's error word (DxRt::err) and all pollers drain.
//
// Next to it, the arithmetic every such kernel builds its stages from: the weight-stationary pass (dx_pass), the wave reductions on DPP and
// permlane swaps (dx_allsum .. dx_reduce), and the 4-bytes-per-lane load from global memory straight into LDS (dx_load_lds4).
#pragma once
#include <hip/hip_runtime.h>

typedef __attribute__((address_space(1))) unsigned long long dx_gu64;
typedef __attribute__((address_space(1))) unsigned dx_gu32;

#define DX_NT 512
#define DX_NW 8
#define DX_GROUP 32          // members (CUs) per group
#define DX_NGROUP 8          // groups (XCDs)
#define DX_SPIN_LIMIT (1u << 21)
#define DX_TRACE_STEPS 8
#define DX_TRACE_SLOTS 16

#define DX_DPP0(v, ctrl) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), (ctrl), 0xF, 0xF, false))
#define DX_DPPZ(v, ctrl, rmask, bmask) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), (ctrl), (rmask), (bmask), true))
// sum over the wave; every lane of a row of 16 first gets its row's total, the row totals are chained into lane 63 and read back
// as a wave-uniform value
__device__ __forceinline__ float dx_allsum(float v) {
  v += DX_DPP0(v, 0xB1);                 // quad_perm [1,0,3,2]
  v += DX_DPP0(v, 0x4E);                 // quad_perm [2,3,0,1]
  v += DX_DPP0(v, 0x141);                // row_half_mirror
  v += DX_DPP0(v, 0x140);                // row_mirror
  v += DX_DPPZ(v, 0x142, 0xA, 0xF);      // row_bcast:15 -> rows 1, 3
  v += DX_DPPZ(v, 0x143, 0xC, 0xF);      // row_bcast:31 -> rows 2, 3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float dx_allmax(float v) {
  v = fmaxf(v, DX_DPP0(v, 0xB1)); v = fmaxf(v, DX_DPP0(v, 0x4E)); v = fmaxf(v, DX_DPP0(v, 0x141)); v = fmaxf(v, DX_DPP0(v, 0x140));
  const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)), d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return fmaxf(fmaxf(a, b), fmaxf(c, d));
}
__device__ __forceinline__ float dx_quadsum(float v) { v += DX_DPP0(v, 0xB1); v += DX_DPP0(v, 0x4E); return v; }

// one pass: acc[c][r] += sum_e W[REG0 + 4c + e] * x[r][4*lane + e]   (W: the thread's NW weight registers; x: LDS, row stride LD)
template <int REG0, int NCOLS, int RG, int NW, int LD>
__device__ __forceinline__ void dx_pass(const float (&W)[NW], const float* x, int lane, float (&acc)[NCOLS][RG]) {
#pragma unroll
  for (int r = 0; r < RG; ++r) {
    const float4 xv = *reinterpret_cast<const float4*>(x + r * LD + 4 * lane);
#pragma unroll
    for (int c = 0; c < NCOLS; ++c) {
      acc[c][r] = fmaf(W[REG0 + 4 * c + 0], xv.x, acc[c][r]);
      acc[c][r] = fmaf(W[REG0 + 4 * c + 1], xv.y, acc[c][r]);
      acc[c][r] = fmaf(W[REG0 + 4 * c + 2], xv.z, acc[c][r]);
      acc[c][r] = fmaf(W[REG0 + 4 * c + 3], xv.w, acc[c][r]);
    }
  }
}
template <int NCOLS, int RG>
__device__ __forceinline__ void dx_zero(float (&acc)[NCOLS][RG]) {
#pragma unroll
  for (int c = 0; c < NCOLS; ++c)
#pragma unroll
    for (int r = 0; r < RG; ++r) acc[c][r] = 0.f;
}
// Wave reduction of NC columns x RG rows of per-lane partial sums.  A plain tree costs 6 cross-lane (DPP) adds per value and DPP
// adds are the expensive instruction here (about four times a plain VALU op), so the first two levels are a butterfly that also
// distributes the ROWS over the lanes of a quad: at each level a lane keeps half of its rows, sends the other half to its
// partner and adds what the partner sends -- the number of live values halves.  After two levels lane l holds, per column, the
// RG/4 rows  (l&1)*RG/2 + ((l>>1)&1)*RG/4 + q  summed over its quad; row_ror 4 / 8 finish the row of 16 lanes and two
// permlane swaps the four rows of the wave, all lane-position preserving.  Every lane ends with the wave totals of its rows.
template <int RG> struct DxRL { static constexpr int value = RG >= 4 ? RG / 4 : 1; };
template <int RG>
__device__ __forceinline__ int dx_row(int lane, int q) {
  if (RG >= 4) return (lane & 1) * (RG / 2) + ((lane >> 1) & 1) * (RG / 4) + q;
  if (RG == 2) return lane & 1;
  return 0;
}
__device__ __forceinline__ float dx_xrow16(float v) {
  const unsigned u = __float_as_uint(v);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float dx_xrow32(float v) {
  const unsigned u = __float_as_uint(v);
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
template <int NC, int RG>
__device__ __forceinline__ void dx_reduce(const float (&a)[NC][RG], float (&out)[NC][DxRL<RG>::value], int lane) {
  constexpr int RL = DxRL<RG>::value;
  const bool b0 = (lane & 1) != 0, b1 = (lane & 2) != 0;
  float d[NC][RL];
  if (RG >= 4) {
    constexpr int H = RG / 2, Q = RG / 4;
    float b[NC][H];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int p = 0; p < H; ++p) {
        const float keep = b0 ? a[c][H + p] : a[c][p], send = b0 ? a[c][p] : a[c][H + p];
        b[c][p] = keep + DX_DPP0(send, 0xB1);
      }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const float keep = b1 ? b[c][Q + q] : b[c][q], send = b1 ? b[c][q] : b[c][Q + q];
        d[c][q] = keep + DX_DPP0(send, 0x4E);
      }
  } else if (RG == 2) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float keep = b0 ? a[c][1] : a[c][0], send = b0 ? a[c][0] : a[c][1];
      const float t = keep + DX_DPP0(send, 0xB1);
      d[c][0] = t + DX_DPP0(t, 0x4E);
    }
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float t = a[c][0] + DX_DPP0(a[c][0], 0xB1);
      d[c][0] = t + DX_DPP0(t, 0x4E);
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int q = 0; q < RL; ++q) d[c][q] += DX_DPP0(d[c][q], 0x124);     // row_ror:4
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int q = 0; q < RL; ++q) d[c][q] += DX_DPP0(d[c][q], 0x128);     // row_ror:8
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int q = 0; q < RL; ++q) d[c][q] = dx_xrow16(d[c][q]);
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int q = 0; q < RL; ++q) out[c][q] = dx_xrow32(d[c][q]);
}

struct DxRt {     // run-time state of a thread
  dx_gu32* err; bool wt; bool dead;
#ifdef DX_DLY_RT
  int dly[12];       // this wave's table (waves 0-3 / 4-7 may differ in the A/B build)
#endif
};
// The sleep in front of a gather's FIRST poll (template parameter DLY of dx_poll* / dx_gather*, s_sleep units of 64 clocks): a poll that reaches the L2
// ahead of the stores it waits for comes back stale and costs a second round trip (~500 clocks); a short sleep lets the group's stores land first.
// The values are per kernel and per site: dx_site_delay (taco_decoder_xcd.h), db_site_delay (taco_decoder_bwd_xcd.h).  In the sweep build -DDX_DLY_RT
// a DLY of 100 + site reads the wave's table instead.  (A sleep between two polls of a stale granule, on top of this one: 1 unit +-0, 2 units +2 %,
// 4 units +6.6 % of the decoder loop; profiles/HISTORY.md 3.1d.)
template <int DLY>
__device__ __forceinline__ void dx_first_poll_sleep(const DxRt& rt) {
#ifdef DX_DLY_RT
  if constexpr (DLY >= 100) { const int n = __builtin_amdgcn_readfirstlane(rt.dly[DLY - 100]); for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(1); return; }
#endif
  if constexpr (DLY > 0 && DLY < 100) __builtin_amdgcn_s_sleep(DLY);
  (void)rt;
}
// How an XCD-local granule leaves the lane: global_store_dwordx2 sc0.  A non-temporal and a plain store measured the same on a stage in isolation
// (tools/ubench_mfma_stage: 1564 / 2418 clocks per stage), a workgroup-scope atomic swap with the result dropped six times as long: the L2
// serialises the 8 K atomics of a stage (profiles/HISTORY.md 3.1d).
__device__ __forceinline__ void dx_store_local(dx_gu64* p, unsigned long long g) {
  __hip_atomic_store(p, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);           // sc0: stays in this XCD's L2
}
// Granule `idx` of a group's exchange buffer as the buffer's (wave-uniform) base + a 32-bit byte offset (round 7): the access is one instruction
// with the base in an SGPR pair and the offset in one VGPR.  As X + xl.field + index the compiler kept a 64-bit base per exchange field in SGPRs
// (spilled to VGPR lanes and read back with v_readlane inside the step) and built every address with 64-bit VALU adds.  The buffer is far below 4 GB.
__device__ __forceinline__ dx_gu64* dx_at(const dx_gu64* X, unsigned idx) {
  return (dx_gu64*)((__attribute__((address_space(1))) char*)X + (size_t)(idx * 8u));
}
// WTC: the protocol as a compile-time constant (0: XCD-local, 1: write-through) where the kernel body is instantiated per protocol -- the
// run-time test (-1) costs a branch per publish, ~30 clocks each on the chain (round 5: 11 % of a post-net scan step, measured)
template <int WTC = -1>
__device__ __forceinline__ void dx_publish(dx_gu64* p, float v, unsigned tag, const DxRt& rt) {
  const unsigned long long g = ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v);
  if (WTC == 1 || (WTC < 0 && rt.wt)) __hip_atomic_store(p, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);         // sc1: write-through, any placement
  else dx_store_local(p, g);
}
// N granules of one lane at once (p + u*stride): ONE uniform branch on the protocol around all stores, so that the epilogue that
// produced the values stays a single basic block (a branch per value kept the compiler from interleaving the exp/rcp chains of
// independent units)
template <int N, int WTC = -1>
__device__ __forceinline__ void dx_publish_n(dx_gu64* p, int stride, const float (&v)[N], unsigned tag, const DxRt& rt) {
  unsigned long long g[N];
#pragma unroll
  for (int u = 0; u < N; ++u) g[u] = ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v[u]);
  if (WTC == 1 || (WTC < 0 && rt.wt)) {
#pragma unroll
    for (int u = 0; u < N; ++u) __hip_atomic_store(p + u * stride, g[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
#pragma unroll
    for (int u = 0; u < N; ++u) dx_store_local(p + u * stride, g[u]);
  }
}
// keeps a value's computation where it is written (LLVM otherwise sinks an expensive operand of a select into a branch)
#define DX_PIN(x) asm("" : "+v"(x))
// Poll N granules (p0 + u*stride) until every one carries `tag` (L1-bypassing loads).  All N are re-requested together on every
// round, so a late producer costs one L2 round trip after its store lands, not one per granule.  Bounded.
template <int N, int DLY = 0>
__device__ __forceinline__ void dx_poll_at(const dx_gu64* X, unsigned idx0, unsigned stride, unsigned tag, float (&v)[N], DxRt& rt) {
  // (keeping a second round of requests in flight behind the one being examined was measured: 11.8 -> 14.2 us per decoder step at
  // C2 -- the extra L2 requests of 16 K pollers delay the very stores they are waiting for)
  unsigned long long g[N];
  unsigned spins = 0;
  dx_first_poll_sleep<DLY>(rt);
  for (;;) {
    bool ok = true;
#pragma unroll
    for (int u = 0; u < N; ++u) g[u] = __hip_atomic_load(dx_at(X, idx0 + (unsigned)u * stride), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int u = 0; u < N; ++u) ok = ok && ((unsigned)(g[u] >> 32) == tag);
    if (ok || rt.dead) break;
    if ((++spins & 1023u) == 0) {
      if (spins >= DX_SPIN_LIMIT || __hip_atomic_load(rt.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        __hip_atomic_store(rt.err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rt.dead = true;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < N; ++u) v[u] = __uint_as_float((unsigned)g[u]);
}
template <int N, int DLY = 0>
__device__ __forceinline__ void dx_poll(const dx_gu64* p0, size_t stride, unsigned tag, float (&v)[N], DxRt& rt) {
  dx_poll_at<N, DLY>(p0, 0u, (unsigned)stride, tag, v, rt);
}
// all-gather of a published [RG][N] vector (granules X[base ..]) into the LDS state vector at column offset `off` (N a power of two);
// RES: dst2[r][n] = value + res[r][n] as well (ResidualWrapper output, tacotron.py:172)
// Two ADJACENT granules with one 16-byte request (each 8-byte half is one producer's single 8-byte store; a half that has not landed
// fails its own tag test and the pair is asked for again).  Used where a thread collects four or more granules per gather (eight rows
// per group; the 512-wide gate-gradient vectors of the BPTT kernel): measured on the exchange stage in isolation
// (tools/ubench_rowsets, variant T) 13.96 -> 12.63 us per step at eight rows, and nothing at two granules per thread (C2's decoder).
typedef unsigned long long dx_u64x2 __attribute__((ext_vector_type(2)));
template <int NP, int DLY = 0>
__device__ __forceinline__ void dx_poll_pairs(const dx_gu64* X, unsigned idx0, unsigned stride, unsigned tag, float (&v)[2 * NP], DxRt& rt) {
  dx_u64x2 g[NP];
  unsigned spins = 0;
  dx_first_poll_sleep<DLY>(rt);
  for (;;) {
    bool ok = true;
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const dx_gu64* p = dx_at(X, idx0 + (unsigned)u * stride);
      asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(g[u]) : "v"(p) : "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int u = 0; u < NP; ++u) ok = ok && ((unsigned)(g[u][0] >> 32) == tag) && ((unsigned)(g[u][1] >> 32) == tag);
    if (ok || rt.dead) break;
    if ((++spins & 1023u) == 0) {
      if (spins >= DX_SPIN_LIMIT || __hip_atomic_load(rt.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        __hip_atomic_store(rt.err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rt.dead = true;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < NP; ++u) { v[2 * u] = __uint_as_float((unsigned)g[u][0]); v[2 * u + 1] = __uint_as_float((unsigned)g[u][1]); }
}
template <int RG, int N, bool RES, int LD, int NT = DX_NT, int DLY = 0>
__device__ __forceinline__ void dx_gather_at(const dx_gu64* X, unsigned base, unsigned tag, float* st, int off, int off_res, int off2, int tid, DxRt& rt) {
  constexpr int NI = (RG * N + NT - 1) / NT;
  if constexpr (NI >= 4 && NI % 2 == 0 && (RG * N) % (2 * NT) == 0 && N % 2 == 0) {
    constexpr int NP = NI / 2;
    float v[NI];
    dx_poll_pairs<NP, DLY>(X, base + 2u * (unsigned)tid, 2u * NT, tag, v, rt);
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const unsigned i = 2u * ((unsigned)(u * NT) + (unsigned)tid), r = i / (unsigned)N, n = i % (unsigned)N;
      *reinterpret_cast<float2*>(st + r * LD + off + n) = make_float2(v[2 * u], v[2 * u + 1]);
      if (RES) {
        const float2 rs = *reinterpret_cast<const float2*>(st + r * LD + off_res + n);
        *reinterpret_cast<float2*>(st + r * LD + off2 + n) = make_float2(v[2 * u] + rs.x, v[2 * u + 1] + rs.y);
      }
    }
    return;
  }
  const bool act = (RG * N >= NT) || tid < RG * N;
  if (act) {
    float v[NI];
    dx_poll_at<NI, DLY>(X, base + (unsigned)tid, NT, tag, v, rt);
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      const unsigned i = (unsigned)(u * NT) + (unsigned)tid;      // (unsigned: a shift and a mask; the signed forms cost five instructions each)
      const unsigned r = i / (unsigned)N, n = i % (unsigned)N;
      st[r * LD + off + n] = v[u];
      if (RES) st[r * LD + off2 + n] = v[u] + st[r * LD + off_res + n];
    }
  }
}
template <int RG, int N, bool RES, int LD, int NT = DX_NT, int DLY = 0>
__device__ __forceinline__ void dx_gather(const dx_gu64* X, unsigned tag, float* st, int off, int off_res, int off2, int tid, DxRt& rt) {
  dx_gather_at<RG, N, RES, LD, NT, DLY>(X, 0u, tag, st, off, off_res, off2, tid, rt);
}

// The loads of a gather of N granules by NT threads, requested now and examined later (dx_gather split in two).  Both forward scans (N = RG * GX_H)
// and both backward scans (N = RG * W: the d c_pre and the d gates vectors) use it.
template <int N, int NT>
struct XgPoll {
  static constexpr int NI = (N + NT - 1) / NT;
  unsigned long long g[NI];
};
template <int N, int NT>
__device__ __forceinline__ void xg_request(const dx_gu64* X, int tid, XgPoll<N, NT>& p) {
  constexpr int NI = XgPoll<N, NT>::NI;
  if ((N >= NT) || tid < N) {
#pragma unroll
    for (int u = 0; u < NI; ++u) p.g[u] = __hip_atomic_load(X + tid + u * NT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// Makes the requested granules "used" at this point of the program: hipcc places the wait for the loads HERE.  Called right before a
// phase publishes, so that the wait sees only the loads (requested a whole compute phase ago: landed) and not the publish stores
// issued after them -- vmcnt counts in issue order, and a wait behind the stores would also wait for their acknowledgement.
// `after` ties the statement to a value of the phase's epilogue, so that the scheduler cannot hoist it (and the wait) above the
// phase's arithmetic.
template <int N, int NT>
__device__ __forceinline__ void xg_landed(XgPoll<N, NT>& p, float& after) {
#pragma unroll
  for (int u = 0; u < XgPoll<N, NT>::NI; ++u) asm volatile("" : "+v"(p.g[u]), "+v"(after));
}
template <int N, int NT>
__device__ __forceinline__ void xg_collect(const dx_gu64* X, unsigned tag, float* st, int tid, XgPoll<N, NT>& p, DxRt& rt) {
  constexpr int NI = XgPoll<N, NT>::NI;
  if ((N >= NT) || tid < N) {
    bool ok = true;
#pragma unroll
    for (int u = 0; u < NI; ++u) ok = ok && ((unsigned)(p.g[u] >> 32) == tag);
    float v[NI];
    if (ok) {
#pragma unroll
      for (int u = 0; u < NI; ++u) v[u] = __uint_as_float((unsigned)p.g[u]);
    } else {
      dx_poll<NI>(X + tid, NT, tag, v, rt);       // a producer was late: the ordinary bounded poll
    }
#pragma unroll
    for (int u = 0; u < NI; ++u) st[u * NT + tid] = v[u];      // granule order: [rows][width] row-major
  }
}

typedef __attribute__((address_space(3))) float dx_lds_float;
// 4 bytes per lane from global memory straight into LDS: the wave's 64 floats land at LDS byte address lds_dst (wave-uniform) + 4 * lane.
// Not counted by hipcc: the consumer waits (any later s_waitcnt vmcnt(0) of the issuing wave covers it: loads retire in order).
__device__ __forceinline__ void dx_load_lds4(const float* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// Census of a persistent launch of 256 (or 512: two per CU) workgroups: every workgroup reports the XCD it runs on (HW_REG_XCC_ID)
// and takes the next slot there; when all have arrived and every XCD hosts exactly gridDim.x / 8 of them, the XCD-local protocol is used (exchange stores stay
// in the XCD's L2) and a workgroup's place is (xcc, slot); otherwise -- or with force_wt -- places follow blockIdx and the stores
// are write-through.  out[0] = xcc or blockIdx % 8, out[1] = slot (0..31) or blockIdx / 8, out[2] = write-through?, out[3] = failed?
// errw[info0..info0+8] report the protocol and the per-XCD counts to the host.  Called by all threads; ends with a barrier.
__device__ __forceinline__ void dx_census(dx_gu32* ctl, dx_gu32* errw, int force_wt, int* out, int tid, int info0) {
  if (tid == 0) {
    const unsigned xcc = __builtin_amdgcn_s_getreg(6164) & 7u;      // HW_REG_XCC_ID (id 20), bits [3:0]
    const unsigned slot = __hip_atomic_fetch_add(ctl + xcc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(ctl + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0; bool ok = true;
    while (__hip_atomic_load(ctl + 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x) {
      __builtin_amdgcn_s_sleep(2);
      if (++spins > (DX_SPIN_LIMIT << 2) || __hip_atomic_load(errw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { ok = false; break; }
    }
    bool even = ok;
    for (int i = 0; i < DX_NGROUP; ++i)
      even = even && (__hip_atomic_load(ctl + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x / DX_NGROUP);
    const bool fast = even && !force_wt;
    if (!ok) __hip_atomic_store(errw, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    out[0] = fast ? (int)xcc : (int)(blockIdx.x & 7);
    out[1] = fast ? (int)slot : (int)(blockIdx.x >> 3);
    out[2] = fast ? 0 : 1;
    out[3] = ok ? 0 : 1;
    if (blockIdx.x == 0) {   // reported to the host (taco_debug_decoder_info): protocol used, workgroups seen per XCD
      errw[info0] = fast ? 1u : 2u;
      for (int i = 0; i < DX_NGROUP; ++i) errw[info0 + 1 + i] = __hip_atomic_load(ctl + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
}
