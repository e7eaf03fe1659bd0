// taco_chain.h -- the point-wise tail of a CBHG (modules.py:72-77 + the hoisted input projection of the BiGRU, :82-96) as ONE
// launch: [dense ->] highway x depth -> BiGRU input projection, for a tile of 64 frames at a time.
//
// As separate launches (k_gemm_bf3) every link writes its [B*T, W] activation to HBM and the next one stages it again: 6 launches
// and 5 round trips of 16 MB at the post-net of C2 for layers of only 4 GFLOP each (30 us per highway layer, 150 TF-equivalent).
// Here a workgroup of 8 waves keeps the tile's activations on the CU from the first layer to the last:
//   * the tile [64, W] lives in LDS as two bf16 planes (hi = bf16(x), lo = bf16(x - hi): the split-bf16 operand of k_gemm_bf3,
//     same arithmetic, same weight packs) -- the A operand of every layer;
//   * wave (wm, wn) owns rows 64/WM * wm .. and the 32 columns 32 wn .. of every W-wide layer, streams its weight fragments from
//     the layer's pack (L2) one k16 step ahead, and keeps its own 32 x 32 (x TM) slice of the layer's fp32 output in registers:
//     the highway carry  y = H*T + x*(1-T)  needs x exactly where the lane produced it one layer earlier;
//   * between layers (a seam): the lanes write their outputs into a SECOND plane set, one barrier, the sets swap.  Round 18 (profiles/r18_*):
//     until then a seam was barrier ("every wave has read the planes") - 64 ds_write_b16 per lane - barrier.  Now (1) layer l reads one set and
//     writes the other, so only "all writes done before anyone reads" is left to wait for; (2) the first weight fragments and the biases of the
//     product loop behind the seam are requested before the epilogue in front of it (ch_request), the entry's first proj_2 block and per-column
//     operands before the wait for the partial sums; (3) the last link runs its passes from the upper column groups down and no longer waits
//     for each time-reversed store to be acknowledged (store_group).  Tried and left out, with their numbers where they stood: 32-bit plane
//     writes by lane pairs (ch_write_planes), four parts' sums in flight at W = 128 (the entry).  No FMA chain, summation order or K rotation
//     moved: tests/test_gpu_chain_seams.py holds the forward to the bits of the build before;
//   * the last link (N = 6H columns) loops over column groups of W and stores straight to the projection buffer, the backward
//     direction's columns time-reversed per row (tf.reverse_sequence, A.7) exactly as k_gemm_bf3's epilogue does.
//
// Round 5: the same kernel also runs the ENCODER PRENET (taco_lib.hip: run_prenet_chain) -- the embedding rows gathered straight into the planes
// (ChainArgs.gather), a 256-wide ReLU layer, and the second layer as the chain's last link with a ReLU on its way out (ChainLayer.act) --, and the
// workgroups of that launch that own no tile clear the words the forward's persistent kernels poll (ChainArgs.ntiles, zp, znw).  The workgroups of
// an XCD walk every layer's K loop from different starting steps (ChainArgs::krot).
#pragma once
#include "taco_kernels.h"

#define CH_MAXL 8
// Register sets of weight fragments per wave (ch_mma_loop): two, at W = 256 and at W = 128 (deeper rings: profiles/r05_ab_runs.txt, call L, and below).  What bounds the product loops, measured at C2 in round 4
// (tools/trace_chain.py on ablated builds): a k16 step of a highway layer takes ~1040 ticks for ~650 of matrix work.  Rings 2, 3, 4, 5 deep,
// the activation fragments requested a step ahead of their MFMAs, four or eight independent accumulator chains per cluster: no change.
// Every step re-reading the FIRST step's weight fragments (L1 hits, same instruction stream): 16.2 K -> 10.5 K ticks per layer.  So the loops
// are bound by the stream of weight fragments out of L2: 32 CUs of an XCD x 32 KB per step = 1 MB per step through an L2 that returns ~1 KB
// per clock -- bandwidth, not latency.  Rows per workgroup set that ratio (every workgroup streams all 3.6 MB of the stage's weights): 128-row
// tiles would halve the stream but leave half the CUs idle at M = 16384 and double the matrix time per CU, which is the larger term.
constexpr int CH_PF = 2;
#define CH_BM 64
constexpr int CH_RIDERS = 4;       // regions a launch's spare workgroups clear (ChainArgs::zp / znw): the words a forward's persistent kernels poll (forward_pass lists them)
enum { CH_DENSE = 0, CH_HIGHWAY = 1, CH_XPROJ = 2 };
struct ChainLayer {
  const unsigned short* bh; const unsigned short* bl; const unsigned short* bh2; const unsigned short* bl2;   // split-bf16 packs (pack_bf3)
  const float* bias; const float* bias2;
  int type, K16, NT, N, act;       // k16 steps of the layer's K (padded input width / 16), 32-column tiles in the pack, columns
};
// Fused entry (the CBHG's second projection in front of the chain, modules.py:55-69): instead of reading its input rows, the workgroup
// forms them -- proj_1's output from the partial sums of k_cbhg_front (sum over the parts in a fixed order, + bias -> ReLU -> BatchNorm:
// what k_front_combine did as a launch of its own), then the width-3 projection conv proj_2 (+ bias -> BatchNorm affine, no activation)
// on the matrix cores, + the residual input (+ the deepvoice per-row vector).  Saves two launches and the round trip of two activations.
struct ChainEntry {
  const float* part; int P; size_t MN; int N1;           // partial sums [P][M][N1]
  const float* b1; const float* s1; const float* h1; int relu1;       // proj_1: bias, BatchNorm scale / shift (nullable), ReLU?
  const unsigned short* bh; const unsigned short* bl; int NT2, K16tap, N2;   // proj_2 pack (pack_bf3), k16 groups per tap, columns
  const float* b2; const float* s2; const float* h2;     // proj_2: bias, BatchNorm scale / shift (nullable)
  const float* res; int ldres;                           // residual rows [M, ldres] (the CBHG's input)
  const float* rowvec; int ldrv;                         // optional per-batch-row vector [M / T, ldrv]
};
struct ChainArgs {
  ChainEntry e;                    // e.part != null: fused entry (x unused)
  const float* x; int ldx, Cin;    // input rows [M, ldx], Cin columns used
  const int* gather;               // optional: row m of the input is x[gather[m]] (the embedding lookup in front of the encoder prenet, tacotron.py:38-39)
  float* out; int ldo;             // projection output [M, ldo]
  float* y; int ldy;               // optional: the last highway output [M, W] (null: not stored)
  const int* rev_len; int rev_col0;
  int M, T, nlayers;
  int krot;                        // 1: workgroups start their K loops at different steps (the default; 133.6 -> 130.6 and 60.9 -> 58.9 us at C2, profiles/r05_ab_runs.txt, call J); 0: every tile walks K from step 0
  // riders: with ntiles > 0 the workgroups ntiles .. gridDim.x - 1 own no tile; they clear up to CH_RIDERS regions of 32-bit words (the words the
  // persistent kernels of the same forward poll: a launch of its own otherwise -- the encoder prenet's chain leaves three quarters of the CUs free)
  int ntiles; unsigned* zp[CH_RIDERS]; unsigned long long znw[CH_RIDERS];
  ChainLayer L[CH_MAXL];
};

// One product loop of a wave: a layer's K for its TM row tiles and one 32-column tile nt of the pack (bhA, blA); dual: a second product that
// shares the A fragments -- the T matrix of a highway layer at the same column tile, or column tile nt2 of the same matrix.  rot: the
// workgroup's first k16 step: the CUs of an XCD walk the layer's K in the same order but from different starts, so that at any moment
// they ask the L2 for DIFFERENT 8 KB slices of the pack instead of all 32 for the same one
struct ChProd {
  const unsigned short* bhA; const unsigned short* blA; const unsigned short* bhB; const unsigned short* blB;
  int K16, NT, nt, nt2, rot; bool dual;
};
// the register sets of weight fragments (hi, lo; h2, l2: the second product's) that a product loop rotates through
struct ChFrag { uint4 h[CH_PF], l[CH_PF], h2[CH_PF], l2[CH_PF]; };
__device__ __forceinline__ int ch_kstep(const ChProd& p, int g) { const int gg = min(g, p.K16 - 1) + p.rot; return gg >= p.K16 ? gg - p.K16 : gg; }
__device__ __forceinline__ size_t ch_boff(const ChProd& p, int g, int t, int l31, int lh) { return ((((size_t)ch_kstep(p, g) * p.NT + t) * 2 + lh) * 32 + l31) * 8; }
// The loads a product loop needs before its first MFMA -- steps 0 .. CH_PF - 1 into sets 0 .. CH_PF - 1 -- as a call of their own: the
// product (ChProd) depends on the layer alone, not on the activations, so the kernel asks for them BEFORE the epilogue and the barrier of
// the seam in front of the loop, and the L2 round trip runs under the seam instead of behind it.  ch_mma_loop takes the sets as loaded here.
__device__ __forceinline__ void ch_request(const ChProd& p, int l31, int lh, ChFrag& fr) {
#pragma unroll
  for (int i = 0; i < CH_PF; ++i) {
    const size_t o = ch_boff(p, i, p.nt, l31, lh);
    fr.h[i] = *reinterpret_cast<const uint4*>(p.bhA + o); fr.l[i] = *reinterpret_cast<const uint4*>(p.blA + o);
    fr.h2[i] = fr.l2[i] = make_uint4(0, 0, 0, 0);
    if (p.dual) { const size_t o2 = ch_boff(p, i, p.nt2, l31, lh); fr.h2[i] = *reinterpret_cast<const uint4*>(p.bhB + o2); fr.l2[i] = *reinterpret_cast<const uint4*>(p.blB + o2); }
  }
}
// the loop itself (DUAL == p.dual): weight fragments one k16 step ahead in two register sets that swap roles (K16 is even: pack_bf3 pads K to
// a multiple of 32); fr holds steps 0 .. CH_PF - 1 on entry (ch_request)
template <int TM, int LDSW, bool DUAL>
__device__ __forceinline__ void ch_mma_loop(const ChProd& p, ChFrag& fr, const unsigned short* xhi, const unsigned short* xlo, int row0,
                                            int l31, int lh, f32x16 (&acc)[TM], f32x16 (&acc2)[TM]) {
  const int K16 = p.K16;
  auto kstep = [&](int g) { return ch_kstep(p, g); };
  auto loadb = [&](int g, uint4& h, uint4& l, uint4& h2, uint4& l2) {
    const size_t o = ch_boff(p, g, p.nt, l31, lh);
    h = *reinterpret_cast<const uint4*>(p.bhA + o); l = *reinterpret_cast<const uint4*>(p.blA + o);
    if constexpr (DUAL) { const size_t o2 = ch_boff(p, g, p.nt2, l31, lh); h2 = *reinterpret_cast<const uint4*>(p.bhB + o2); l2 = *reinterpret_cast<const uint4*>(p.blB + o2); }
  };
  auto mma = [&](int g, const uint4& h, const uint4& l, const uint4& h2, const uint4& l2) {
    const bf16x8 bh = __builtin_bit_cast(bf16x8, h), bl = __builtin_bit_cast(bf16x8, l);
    bf16x8 ah[TM], al[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const int off = (row0 + tm * 32 + l31) * LDSW + 16 * kstep(g) + 8 * lh;
      ah[tm] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(xhi + off));
      al[tm] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(xlo + off));
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) acc[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[tm], bh, acc[tm], 0, 0, 0);      // small terms first
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) acc[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[tm], bl, acc[tm], 0, 0, 0);
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) acc[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[tm], bh, acc[tm], 0, 0, 0);
    if constexpr (DUAL) {
      const bf16x8 bh2 = __builtin_bit_cast(bf16x8, h2), bl2 = __builtin_bit_cast(bf16x8, l2);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) acc2[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[tm], bh2, acc2[tm], 0, 0, 0);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) acc2[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[tm], bl2, acc2[tm], 0, 0, 0);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) acc2[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[tm], bh2, acc2[tm], 0, 0, 0);
    }
  };
  // steps 0 and 1 are in the sets already: the first round asks for step 2 only
  __builtin_amdgcn_sched_barrier(0);
  mma(0, fr.h[0], fr.l[0], fr.h2[0], fr.l2[0]);
  __builtin_amdgcn_sched_barrier(0);
  loadb(2, fr.h[0], fr.l[0], fr.h2[0], fr.l2[0]);
  __builtin_amdgcn_sched_barrier(0);
  mma(1, fr.h[1], fr.l[1], fr.h2[1], fr.l2[1]);
  __builtin_amdgcn_sched_barrier(0);
  for (int g = 2; g < K16; g += 2) {
    loadb(g + 1, fr.h[1], fr.l[1], fr.h2[1], fr.l2[1]);
    __builtin_amdgcn_sched_barrier(0);
    mma(g, fr.h[0], fr.l[0], fr.h2[0], fr.l2[0]);
    __builtin_amdgcn_sched_barrier(0);
    loadb(g + 2, fr.h[0], fr.l[0], fr.h2[0], fr.l2[0]);
    __builtin_amdgcn_sched_barrier(0);
    mma(g + 1, fr.h[1], fr.l[1], fr.h2[1], fr.l2[1]);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// The lane's slice of a layer's output -> the (hi, lo) planes: a lane holds ONE column (col) of 16 rows per row tile and writes 2-byte elements.
// row0: first row of the lane's C elements (row tile 0, register 0); on: the lane's column lies inside the planes.
// (Round 18 tried 32-bit writes: a lane pair swaps half of its values with one DPP move each, quad_perm [1,0,3,2], and each lane writes words of
// two neighbouring columns -- half the ds_write count and packed conversions.  Same bits; k_pointwise_chain<256> 118.6 / 118.4 us without it
// against 119.5 / 118.2 with it, <128> 50.9 / 51.4 against 51.1 / 50.9: the writes of a wave are not what the seam's one barrier waits for.  Left out.)
template <int TM, int LDSW>
__device__ __forceinline__ void ch_write_planes(unsigned short* xhi, unsigned short* xlo, int row0, int col, const float (&x)[TM][16], bool on) {
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float f = x[tm][r];
      const unsigned hp = taco_pk_bf16(f, 0.f) & 0xffffu;
      const unsigned lp = taco_pk_bf16(f - __uint_as_float(hp << 16), 0.f) & 0xffffu;
      const int off = (row0 + tm * 32 + (r & 3) + 8 * (r >> 2)) * LDSW + col;
      if (on) { xhi[off] = (unsigned short)hp; xlo[off] = (unsigned short)lp; }
    }
}

#ifdef TACO_TRACE
__device__ long long taco_trace_chain[64];      // slots: 0 entry, 1 partial sums in planes, 2 proj_2 products done, 3 entry epilogue done, 4 first barrier; then per layer:
#define CTRC(i) do { if (trc && (i) < 64) taco_trace_chain[i] = clock64(); } while (0)      // products done, epilogue done, plane writes issued, barrier passed; per pass of the last link: products done, stores issued
#else
#define CTRC(i) do {} while (0)
#endif
// (Round 5: the ring depth was tried again where only 64 workgroups run -- the encoder prenet's chain and the encoder's own, 4096 rows: six sets
// instead of two made the prenet chain 17.6 -> 22.9 us and the encoder chain 61 -> 71 us (four sets: 63).  A deeper ring issues its last sets'
// requests again past the end of every short K loop; the loops are paced by the bytes a CU can pull from L2 (~26-31 B per clock and CU
// measured, all CUs streaming), not by the round trip, so more requests in flight only add bytes.  profiles/r05_*.)
template <int W>
__global__ __launch_bounds__(512) void k_pointwise_chain(const ChainArgs a_in) {
  constexpr int WN = W / 32, WM = 8 / WN, TM = CH_BM / 32 / WM;      // W = 256: 1 x 8 waves of 64 x 32; W = 128: 2 x 4 waves of 32 x 32
  constexpr int LDSW = W + 8;                                          // bf16 elements per plane row: (W + 8) * 2 bytes = odd multiple of 16
  extern __shared__ __attribute__((aligned(16))) unsigned short ch_smem[];
  // two plane sets: a hidden layer reads (xhi, xlo) and writes its output into (yhi, ylo), then the two swap -- one barrier per seam
  unsigned short* xhi = ch_smem;
  unsigned short* xlo = ch_smem + CH_BM * LDSW;
  unsigned short* yhi = ch_smem + 2 * CH_BM * LDSW;
  unsigned short* ylo = ch_smem + 3 * CH_BM * LDSW;
  struct { const float* x; float* out; float* y; const int* rev_len; int ldx, Cin, ldo, ldy, rev_col0, M, T, nlayers; } a =
      {a_in.x, a_in.out, a_in.y, a_in.rev_len, a_in.ldx, a_in.Cin, a_in.ldo, a_in.ldy, a_in.rev_col0, a_in.M, a_in.T, a_in.nlayers};
  PIN(a.x); PIN(a.out); PIN(a.y); PIN(a.rev_len); PIN(a.ldx); PIN(a.Cin); PIN(a.ldo); PIN(a.ldy); PIN(a.rev_col0); PIN(a.M); PIN(a.T);
  PIN(a.nlayers);
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  if (a_in.ntiles > 0 && (int)blockIdx.x >= a_in.ntiles) {
    const size_t i0 = (size_t)((int)blockIdx.x - a_in.ntiles) * 512 + tid, stride = (size_t)((int)gridDim.x - a_in.ntiles) * 512;
    for (int rg = 0; rg < CH_RIDERS; ++rg) {
      unsigned* p = a_in.zp[rg];
      const size_t nw = a_in.znw[rg];
      if (!p || !nw) continue;
      const size_t n16 = (reinterpret_cast<uintptr_t>(p) & 15) ? 0 : nw / 4;
      uint4* q = reinterpret_cast<uint4*>(p);
      for (size_t i = i0; i < n16; i += stride) q[i] = make_uint4(0u, 0u, 0u, 0u);
      for (size_t i = n16 * 4 + i0; i < nw; i += stride) p[i] = 0u;
    }
    return;
  }
  const int m0 = blockIdx.x * CH_BM;
  // first k16 step of this workgroup's K loops, in 32nds of a layer's K (ChainArgs::krot = 0 switches it off at run time: every row's fp32
  // accumulation order is then the same whichever tile the row lands in -- bit-invariance under batch permutation / sharding at any size)
  const int krot = a_in.krot ? ((int)(blockIdx.x >> 3) & 31) : 0;
#ifdef TACO_TRACE
  const bool trc = (blockIdx.x == (a_in.ntiles > 0 ? a_in.ntiles : gridDim.x) / 2) && threadIdx.x == 0;
  int trci = 5;
  CTRC(0);
#endif

  const int l31_outer = l31, lh_outer = lh;
  // column group of pass ps of the last link.  Two groups per pass share the A fragments; an odd group left over (6H = 3 W at W = 256: the backward
  // direction's last columns) goes first, and the pairs follow from the LAST to the first: the time-reversed columns (>= rev_col0, the upper groups)
  // are the slow stores, so they drain behind the products of the passes after them and the kernel ends on a pass of plain stores (at W = 128 the
  // passes ran (0,1) (2,3) (4,5) until round 18, and the reversed stores of (4,5) were the kernel's tail).  Groups are independent of each other.
  auto pass_group = [](int ngroups, int ps) { return ((ngroups & 1) && ps == 0) ? ngroups - 1 : 2 * ((ngroups + 1) / 2 - 1 - ps); };
  // this wave's product of a hidden layer, or of pass ps of the last link
  auto make_prod = [&](const ChainLayer& L, int ps) {
    ChProd p;
    p.bhA = p.bhB = L.bh; p.blA = p.blB = L.bl; p.K16 = L.K16; p.NT = L.NT; p.rot = krot * L.K16 >> 5; p.nt = p.nt2 = wn; p.dual = false;
    if (L.type == CH_XPROJ) {
      const int ngroups = (L.N + W - 1) / W, ng = pass_group(ngroups, ps);
      p.nt = min(ng * WN + wn, L.NT - 1);      // tiles past the pack are clamped, never stored
      p.dual = ng + 1 < ngroups;
      p.nt2 = p.dual ? min((ng + 1) * WN + wn, L.NT - 1) : p.nt;
    } else if (L.type == CH_HIGHWAY) { p.bhB = L.bh2; p.blB = L.bl2; p.dual = true; }
    return p;
  };
  ChFrag fr;                               // first weight fragments of the NEXT product loop, requested ahead of the seam in front of it (ch_request)
  float nbia = 0.f, nbia2 = 0.f;               // ... and the biases of the next hidden layer
  auto request_layer = [&](int li, int l31r, int lhr) {
    const ChainLayer Ln = a_in.L[li];
    ch_request(make_prod(Ln, 0), l31r, lhr, fr);
    if (Ln.type != CH_XPROJ) {
      const int c = wn * 32 + l31r;
      nbia = Ln.bias ? Ln.bias[c] : 0.f;
      nbia2 = (Ln.type == CH_HIGHWAY && Ln.bias2) ? Ln.bias2[c] : 0.f;
    }
  };
  float xreg[TM][16];                          // the lane's slice of the current activation in fp32 (highway carry)
  bool have_x = false;
  if (a_in.e.part) {
    // ---- fused entry: proj_1's epilogue over the partial sums -> planes [CH_BM + 2][N1]; proj_2 (width 3) -> the chain's input ----
    const ChainEntry E = a_in.e;
    const float* gpart = E.part; const float* gb1 = E.b1; const float* gs1 = E.s1; const float* gh1 = E.h1;
    const unsigned short* gbh = E.bh; const unsigned short* gbl = E.bl;
    const float* gres = E.res; const float* grv = E.rowvec; const float* gb2 = E.b2; const float* gs2 = E.s2; const float* gh2 = E.h2;
    PIN(gpart); PIN(gb1); PIN(gs1); PIN(gh1); PIN(gbh); PIN(gbl); PIN(gres); PIN(grv); PIN(gb2); PIN(gs2); PIN(gh2);
    constexpr int N1 = W;                                                  // (= E.N1: ff_plan admits the entry only where proj_1 is as wide as the chain)
    constexpr int LDE = N1 + 8;                                            // bf16 per plane row (N1 = 128 / 256: odd multiple of 16 bytes)
    // behind the first plane set, over the second: the entry's planes are dead once proj_2's products are done, and the first hidden layer writes
    // plane set B only behind the barrier that ends the entry
    unsigned short* ehi = ch_smem + 2 * CH_BM * LDSW;
    unsigned short* elo = ehi + (CH_BM + 2) * LDE;
    constexpr int nq = N1 / 4;
    constexpr int NSTG = ((CH_BM + 2) * nq + 511) / 512;                   // float4 per thread and part: 9 at N1 = 256, 5 at 128
    constexpr int NPART = 2;                                               // parts whose loads are in flight together
    // proj_2's plan: wave (wm, wn) owns its TM row tiles x the 32 columns 32 wn .. (waves past the last column tile idle).
    // W = 256 (one row of eight waves): N2 = 80 columns are three column tiles -- alone, three waves would run the whole contraction on
    // three SIMDs, one wave each, while five wait (31 K of the workgroup's 220 K clocks at C2).  The contraction is cut in two K halves
    // instead: waves NT2 .. 2 NT2 - 1 take the second half of the k16 steps of column tile wn - NT2 and hand their partial tile over
    // through LDS (the chain's own planes are not written yet)
    const int K0 = a_in.L[0].K16 * 16;                                     // columns of the chain's input planes (>= N2, zero padded)
    const int col = wn * 32 + l31;
    const bool cin = col < E.N2;
    const int KSPL = (WM == 1 && 2 * E.NT2 <= WN) ? 2 : 1;
    const bool mact = wn < E.NT2 * KSPL;
    const int ect = mact ? wn % E.NT2 : 0, kp = mact ? wn / E.NT2 : 0;
    const int nk = (3 * E.K16tap) / KSPL, kbeg = kp * nk, kend = kbeg + nk;      // k16 steps (tap, group) of this wave
    auto boff = [&](int k) { return ((((size_t)k * E.NT2 + ect) * 2 + lh) * 32 + l31) * 8; };
    // few waves per SIMD here, so the weight stream is requested a whole block of NB k16 steps ahead (two register
    // sets that swap roles; nk = 3 N1 / 16 [/ 2] is a multiple of 2 NB): one step ahead left every step waiting ~800 clocks for L2
    constexpr int NB = 6;                            // nk = 48, 24 (K halves) or 24: a multiple of 2 NB (the host admits N1 = 256 with W = 256, 128 with 128)
    uint4 pH[NB], pL[NB], qH[NB], qL[NB];
    auto loadblk = [&](int k0, uint4 (&H)[NB], uint4 (&Lo)[NB]) {
#pragma unroll
      for (int i = 0; i < NB; ++i) { const size_t o = boff(min(k0 + i, kend - 1)); H[i] = *reinterpret_cast<const uint4*>(gbh + o); Lo[i] = *reinterpret_cast<const uint4*>(gbl + o); }
    };
    // Requested BEFORE the wait for the partial sums, none of it depends on them: proj_2's first weight block and the per-column operands of both
    // epilogues (proj_1's are the same four columns for every float4 of a thread: 512 is a multiple of nq).  They were one L2 round trip each
    // behind the sums / behind the products.
    if (mact) loadblk(kbeg, pH, pL);
    const int c1 = 4 * (tid % nq);
    const float4 bi1 = gb1 ? *reinterpret_cast<const float4*>(gb1 + c1) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 sc1 = gs1 ? *reinterpret_cast<const float4*>(gs1 + c1) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 sh1 = gh1 ? *reinterpret_cast<const float4*>(gh1 + c1) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float bi2 = (cin && gb2) ? gb2[col] : 0.f, sc2 = (cin && gs2) ? gs2[col] : 1.f, sh2 = (cin && gh2) ? gh2[col] : 0.f;
    __builtin_amdgcn_sched_barrier(0);
    {
      float4 f[NSTG];
      const float* src[NSTG];
#pragma unroll
      for (int u = 0; u < NSTG; ++u) {
        const int i = tid + 512 * u, r = i / nq, c = 4 * (i - r * nq), row = m0 - 1 + r;
        f[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        src[u] = (i < (CH_BM + 2) * nq && row >= 0 && row < a.M) ? gpart + (size_t)row * N1 + c : nullptr;
      }
      // parts in a fixed order (part q before part q + 1: bit-reproducible); the loads of NPART parts are in flight together -- a part's loads
      // alone left a full memory round trip exposed per part (2 at the post-net, 8 at the encoder).  (Round 18: FOUR parts in flight at N1 = 128,
      // where a part is 5 float4 per thread, i.e. two dependent round trips instead of four at the encoder: k_pointwise_chain<128> 51.1 / 50.9 us
      // against 51.5 / 51.8 with two, inside the 0.8 us the launches of one run scatter by.  Left at two.)
      for (int q = 0; q < E.P; q += NPART) {
        float4 g[NPART][NSTG];
#pragma unroll
        for (int j = 0; j < NPART; ++j)
          if (q + j < E.P) {
#pragma unroll
            for (int u = 0; u < NSTG; ++u) g[j][u] = src[u] ? *reinterpret_cast<const float4*>(src[u] + (size_t)(q + j) * E.MN) : make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
        for (int j = 0; j < NPART; ++j)
          if (q + j < E.P) {
#pragma unroll
            for (int u = 0; u < NSTG; ++u) { f[u].x += g[j][u].x; f[u].y += g[j][u].y; f[u].z += g[j][u].z; f[u].w += g[j][u].w; }
          }
      }
#pragma unroll
      for (int u = 0; u < NSTG; ++u) {
        const int i = tid + 512 * u, r = i / nq, c = 4 * (i - r * nq);
        if (i >= (CH_BM + 2) * nq) continue;
        float4 v = f[u];
        if (src[u]) {
          const float4 bi = bi1, sc = sc1, sh = sh1;
          v.x += bi.x; v.y += bi.y; v.z += bi.z; v.w += bi.w;
          if (E.relu1) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
          v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
        }
        uint2 h4, l4;
        taco_split_bf16x4(v, h4, l4);
        *reinterpret_cast<uint2*>(ehi + r * LDE + c) = h4;
        *reinterpret_cast<uint2*>(elo + r * LDE + c) = l4;
      }
    }
    CTRC(1);
    __syncthreads();
    // proj_2 (the plan above): SAME padding and the batch-row boundary by masking the A fragment per (row, tap) as k_gemm_bf3 does
    // (requested BEFORE the MFMA loop, whose duration hides them; all residual values of the lane are requested before the first is used: left in one loop with the LDS stores, every element
    // waited for its own load -- 32 memory round trips)
    float rs[TM][16];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, row = min(m0 + rl, a.M - 1);
        float v = 0.f;
        if (cin) {
          v = gres[(size_t)row * E.ldres + col];
          if (grv) v += grv[(size_t)(row / a.T) * E.ldrv + col];
        }
        rs[tm][r] = v;
      }
    f32x16 acc[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
      for (int r = 0; r < 16; ++r) acc[tm][r] = 0.f;
    if (mact) {
      int tloc[TM];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) tloc[tm] = (m0 + (wm * TM + tm) * 32 + l31) % a.T;
      auto mmablk = [&](int k0, const uint4 (&H)[NB], const uint4 (&Lo)[NB]) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const int k = k0 + i, j = k / E.K16tap, g = k - j * E.K16tap;
          const bf16x8 bh8 = __builtin_bit_cast(bf16x8, H[i]), bl8 = __builtin_bit_cast(bf16x8, Lo[i]);
#pragma unroll
          for (int tm = 0; tm < TM; ++tm) {
            const int off = ((wm * TM + tm) * 32 + l31 + j) * LDE + 16 * g + 8 * lh;
            uint4 xh = *reinterpret_cast<const uint4*>(ehi + off), xl = *reinterpret_cast<const uint4*>(elo + off);
            const int tt = tloc[tm] + j - 1;
            const unsigned keep = ((tt >= 0) && (tt < a.T)) ? 0xffffffffu : 0u;
            xh.x &= keep; xh.y &= keep; xh.z &= keep; xh.w &= keep; xl.x &= keep; xl.y &= keep; xl.z &= keep; xl.w &= keep;
            const bf16x8 ah = __builtin_bit_cast(bf16x8, xh), al = __builtin_bit_cast(bf16x8, xl);
            acc[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh8, acc[tm], 0, 0, 0);
            acc[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl8, acc[tm], 0, 0, 0);
            acc[tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh8, acc[tm], 0, 0, 0);
          }
        }
      };
      for (int k0 = kbeg; k0 < kend; k0 += 2 * NB) {      // (block kbeg was requested in front of the partial sums)
        loadblk(k0 + NB, qH, qL);
        __builtin_amdgcn_sched_barrier(0);
        mmablk(k0, pH, pL);
        __builtin_amdgcn_sched_barrier(0);
        loadblk(k0 + 2 * NB, pH, pL);
        __builtin_amdgcn_sched_barrier(0);
        mmablk(k0 + NB, qH, qL);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    request_layer(0, l31, lh);                         // the first layer's weights and biases travel under the hand-over and the epilogue
    __builtin_amdgcn_sched_barrier(0);
    if (KSPL == 2) {                                   // the second K half's partial tile -> the first half's wave (fixed order: bit-reproducible)
      float* red = reinterpret_cast<float*>(ch_smem);
      if (mact && kp == 1) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int r = 0; r < 16; ++r) red[((ect * TM + tm) * 16 + r) * 64 + lane] = acc[tm][r];
      }
      __syncthreads();
      if (mact && kp == 0) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[tm][r] += red[((ect * TM + tm) * 16 + r) * 64 + lane];
      } else {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
          for (int r = 0; r < 16; ++r) acc[tm][r] = 0.f;
      }
      __syncthreads();                                 // ... before the epilogue below writes the planes over the partial tiles
    }
    CTRC(2);
    // epilogue: + bias -> BatchNorm affine -> + residual (+ per-row vector); the chain's input planes (zero beyond N2) and the carry registers
    {
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(rs[tm][r]));
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) xreg[tm][r] = cin ? (acc[tm][r] + bi2) * sc2 + sh2 + rs[tm][r] : 0.f;
      ch_write_planes<TM, LDSW>(xhi, xlo, wm * TM * 32 + 4 * lh, col, xreg, col < K0);
      have_x = true;
    }
    CTRC(3);
  } else
  // ---- stage the input rows: fp32 -> (hi, lo) planes, zero padded to the first layer's K ----
  {
    request_layer(0, l31, lh);                 // the first layer's weights and biases travel under the staging
    __builtin_amdgcn_sched_barrier(0);
    const int K0 = a_in.L[0].K16 * 16;
    for (int i = tid; i < CH_BM * (K0 / 4); i += 512) {
      const int r = i / (K0 / 4), c = 4 * (i % (K0 / 4));
      float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
      const int row = m0 + r;
      if (row < a.M && c < a.Cin) {
        const float* p = a.x + (size_t)(a_in.gather ? a_in.gather[row] : row) * a.ldx + c;
        if (c + 3 < a.Cin && (a.ldx & 3) == 0) f = *reinterpret_cast<const float4*>(p);
        else { f.x = p[0]; if (c + 1 < a.Cin) f.y = p[1]; if (c + 2 < a.Cin) f.z = p[2]; if (c + 3 < a.Cin) f.w = p[3]; }
      }
      uint2 h4, l4;
      taco_split_bf16x4(f, h4, l4);
      *reinterpret_cast<uint2*>(xhi + r * LDSW + c) = h4;
      *reinterpret_cast<uint2*>(xlo + r * LDSW + c) = l4;
    }
  }
  const bool full = m0 + CH_BM <= a.M;         // every row of the tile exists: the stores need no guards (the common case)
  __syncthreads();
  CTRC(4);

  for (int li = 0; li < a.nlayers; ++li) {
    const ChainLayer L = a_in.L[li];
    // opaque per-layer copies of the lane coordinates: otherwise every address below (32 carry loads, 32 stores, 64 LDS writes per
    // lane) is computed once before the loop and kept -- and spilled -- across all layers (same effect as in taco_decoder_xcd.h)
    int l31 = l31_outer, lh = lh_outer;
    asm volatile("" : "+v"(l31), "+v"(lh));
    // row of the lane's C element r of row tile tm (C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5))
    auto rloc = [&](int tm, int r) { return (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh; };
    const int col = wn * 32 + l31;
    if (L.type == CH_XPROJ) {
      // ---- last link: N = 6H columns in groups of W, stored straight to the projection buffer ----
      const int ngroups = (L.N + W - 1) / W;
      const int bb0 = m0 / a.T;                // a tile of 64 rows spans at most two batch rows when T >= 64: their lengths once, not once per stored element
      const int nbrow = (a.M - 1) / a.T;
      const int Lb0 = a.rev_len ? a.rev_len[min(bb0, nbrow)] : a.T, Lb1 = a.rev_len ? a.rev_len[min(bb0 + 1, nbrow)] : a.T;
      auto store_group = [&](int ng, const f32x16 (&acc)[TM], float bia) {
        const int ocol = ng * W + col;
        if (ocol >= L.N) return;
        const bool rev = a.rev_col0 >= 0 && ocol >= a.rev_col0;
        const bool relu_out = L.act == ACT_RELU;                       // (a chain that ends in a ReLU layer: the encoder prenet; otherwise the value passes as it is, a NaN included)
        if (full && !rev) {
#pragma unroll
          for (int tm = 0; tm < TM; ++tm) {
            float* po = a.out + (size_t)(m0 + rloc(tm, 0)) * a.ldo + ocol;
#pragma unroll
            for (int r = 0; r < 16; ++r) { const float v = acc[tm][r] + bia; po[(size_t)((r & 3) + 8 * (r >> 2)) * a.ldo] = relu_out ? fmaxf(v, 0.f) : v; }
          }
        } else {                               // the backward direction's columns go to the time-reversed row of the batch row
          int lhs = lh;                        // (opaque per call: the 32 reversed row indices are formed here, not kept -- and spilled -- across the column groups)
          asm volatile("" : "+v"(lhs));
          // Two copies of the loop.  T >= 64: the tile's two lengths are in registers, no load on the way to a store.  T < 64: a length is loaded
          // per element.  As ONE loop every element's code joined a path with a load pending, the compiler put a wait for ALL vector-memory
          // traffic in front of every store, and each reversed store waited for the one before it to be acknowledged (32 round trips: the
          // 13 - 17 K clocks of "stores" behind the encoder's reversed pass in the timelines up to round 18)
          if (a.T >= CH_BM) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int row = m0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhs;
                int orow = row;
                if (rev) {
                  const int bb = bb0 + (row >= (bb0 + 1) * a.T ? 1 : 0);
                  const int tt = row - bb * a.T, Lb = bb == bb0 ? Lb0 : Lb1;
                  orow = tt < Lb ? bb * a.T + (Lb - 1 - tt) : row;
                }
                if (row < a.M) { const float v = acc[tm][r] + bia; a.out[(size_t)orow * a.ldo + ocol] = relu_out ? fmaxf(v, 0.f) : v; }
              }
          } else {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int row = m0 + (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhs;
                int orow = row;
                if (rev) {
                  const int bb = row / a.T;
                  const int tt = row - bb * a.T, Lb = a.rev_len ? a.rev_len[min(bb, (a.M - 1) / a.T)] : a.T;
                  orow = tt < Lb ? bb * a.T + (Lb - 1 - tt) : row;
                }
                if (row < a.M) { const float v = acc[tm][r] + bia; a.out[(size_t)orow * a.ldo + ocol] = relu_out ? fmaxf(v, 0.f) : v; }
              }
          }
        }
      };
      // the passes in pass_group's order.  The first pass's fragments were requested before the last seam; a later pass's are requested BEHIND
      // the stores of the pass in front of it: the wait for a load covers every store issued before it, and in front of them it would hold
      // the next products until those stores are acknowledged instead of letting them drain behind the products.  A pass's biases are
      // requested before its products, and they and the tile's lengths are waited for ONCE, before the first store.
      const int npass = (ngroups + 1) / 2;
      for (int ps = 0; ps < npass; ++ps) {
        const int ng = pass_group(ngroups, ps);
        const ChProd pr = make_prod(L, ps);
        const float biaA = (L.bias && ng * W + col < L.N) ? L.bias[ng * W + col] : 0.f;
        const float biaB = (L.bias && pr.dual && (ng + 1) * W + col < L.N) ? L.bias[(ng + 1) * W + col] : 0.f;
        f32x16 acc[TM], acc2[TM];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
          for (int r = 0; r < 16; ++r) { acc[tm][r] = 0.f; acc2[tm][r] = 0.f; }
        if (pr.dual) ch_mma_loop<TM, LDSW, true>(pr, fr, xhi, xlo, wm * TM * 32, l31, lh, acc, acc2);
        else ch_mma_loop<TM, LDSW, false>(pr, fr, xhi, xlo, wm * TM * 32, l31, lh, acc, acc2);     // the odd group: one matrix
#ifdef TACO_TRACE
        CTRC(trci); ++trci;
#endif
        asm volatile("" :: "v"(biaA), "v"(biaB), "v"(Lb0), "v"(Lb1));
        store_group(ng, acc, biaA);
        if (pr.dual) store_group(ng + 1, acc2, biaB);
#ifdef TACO_TRACE
        CTRC(trci); ++trci;
#endif
        __builtin_amdgcn_sched_barrier(0);
        if (ps + 1 < npass) ch_request(make_prod(L, ps + 1), l31, lh, fr);
        else if (li + 1 < a.nlayers) request_layer(li + 1, l31, lh);
      }
      continue;
    }
    // ---- a W-wide hidden layer: dense or highway ----
    const bool dual = L.type == CH_HIGHWAY;
    if (dual && !have_x) {                     // a chain that starts with a highway layer: the carry comes from the input itself
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) xreg[tm][r] = a.x[(size_t)min(m0 + rloc(tm, r), a.M - 1) * a.ldx + col];
    }
    have_x = true;
    {
      f32x16 acc[TM], acc2[TM];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
        for (int r = 0; r < 16; ++r) { acc[tm][r] = 0.f; acc2[tm][r] = 0.f; }
      const float bia = nbia, bia2 = nbia2;      // (request_layer, in front of the seam before this layer)
      const ChProd pr = make_prod(L, 0);
      if (dual) {
        ch_mma_loop<TM, LDSW, true>(pr, fr, xhi, xlo, wm * TM * 32, l31, lh, acc, acc2);
#ifdef TACO_TRACE
        CTRC(trci); ++trci;
#endif
        if (li + 1 < a.nlayers) request_layer(li + 1, l31, lh);      // the next layer's first fragments and biases: under this epilogue and the barrier
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int r = 0; r < 16; ++r) {       // modules.py:105-120: H = relu(.), T = sigmoid(.), y = H*T + x*(1-T)
            const float Hh = fmaxf(acc[tm][r] + bia, 0.f);
            const float Tg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * (acc2[tm][r] + bia2)));
            xreg[tm][r] = Hh * Tg + xreg[tm][r] * (1.f - Tg);
          }
      } else {
        ch_mma_loop<TM, LDSW, false>(pr, fr, xhi, xlo, wm * TM * 32, l31, lh, acc, acc2);
#ifdef TACO_TRACE
        CTRC(trci); ++trci;
#endif
        if (li + 1 < a.nlayers) request_layer(li + 1, l31, lh);
        __builtin_amdgcn_sched_barrier(0);
        const bool relu = L.act == ACT_RELU;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int r = 0; r < 16; ++r) { const float v = acc[tm][r] + bia; xreg[tm][r] = relu ? fmaxf(v, 0.f) : v; }
      }
    }
    const bool last_hidden = (li + 1 == a.nlayers) || a_in.L[li + 1].type == CH_XPROJ;
    if (last_hidden && a.y) {
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + rloc(tm, r);
          if (row < a.M) a.y[(size_t)row * a.ldy + col] = xreg[tm][r];
        }
    }
#ifdef TACO_TRACE
    CTRC(trci); ++trci;
#endif
    // The seam: the output goes into the OTHER plane set, so nobody has to wait until every wave has read this layer's planes; one barrier -- all
    // writes of the new set done before anyone reads it.  When the layer after next writes back into this set, every wave is past that barrier,
    // and a wave passes it only behind its own reads of this layer's planes (its MFMAs have consumed them).
    ch_write_planes<TM, LDSW>(yhi, ylo, wm * TM * 32 + 4 * lh, col, xreg, true);
#ifdef TACO_TRACE
    CTRC(trci); ++trci;
#endif
    __syncthreads();
    { unsigned short* t = xhi; xhi = yhi; yhi = t; t = xlo; xlo = ylo; ylo = t; }
#ifdef TACO_TRACE
    CTRC(trci); ++trci;
#endif
  }
}
