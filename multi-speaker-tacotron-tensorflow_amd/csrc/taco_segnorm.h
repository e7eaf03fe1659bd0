// taco_segnorm.h -- the work table of the segmented norms (k_segsq_piece / k_segsq_segment / k_segnorm_stats, taco_train_kernels.h), included by
// taco_lib.hip in front of taco_train.h.  The builder is host arithmetic only -- no HIP runtime call -- so that it runs on a machine
// without a GPU (taco_debug_segnorm_pieces, tests/test_grad_stats_host.py).  The table DEFINES the order of summation: a piece is
// at most SEGN_P consecutive floats of ONE counted segment, the pieces of a segment tile it exactly, and all pieces ascend; a
// skipped segment and an empty one have none.
#pragma once

// Pieces of segments [off[s], off[s + 1]), s < n_seg, appended to `pieces`; pfirst[s] .. pfirst[s + 1] are those of segment s.
// Returns null, or the text of an argument error (nothing of the inputs is trusted: this runs before any device call).
static const char* segnorm_pieces(const uint64_t* off, int n_seg, const uint8_t* skip, std::vector<SegPiece>& pieces, std::vector<int>& pfirst) {
  if (!off) return "null offsets";
  if (n_seg < 1) return "n_seg must be >= 1";
  for (int s = 0; s < n_seg; ++s)
    if (off[s + 1] < off[s]) return "segment offsets must ascend";
  pieces.clear(); pfirst.assign((size_t)n_seg + 1, 0);
  for (int s = 0; s < n_seg; ++s) {
    pfirst[s] = (int)pieces.size();
    if (skip && skip[s]) continue;
    for (uint64_t b = off[s], left = off[s + 1] - off[s]; left;) {      // (counted down: an end near 2^64 cannot wrap the position)
      if (pieces.size() >= (size_t)0x7fffffff) return "more than 2^31 - 1 pieces";
      const int len = (int)std::min<uint64_t>(SEGN_P, left);
      pieces.push_back(SegPiece{(unsigned long long)b, len, s});
      b += (uint64_t)len; left -= (uint64_t)len;
    }
  }
  pfirst[n_seg] = (int)pieces.size();
  return nullptr;
}

// A plan: the table on the device and every buffer a call writes besides its outputs.  Calls on one plan share `partial` and `segsum`:
// they must be ordered among themselves (one stream, or events between streams).
struct taco_segnorm_plan {
  int device = 0, n_seg = 0, n_pieces = 0;
  uint64_t end = 0;                    // off[n_seg]: the buffer of a call holds at least this many floats
  SegPiece* d_pieces = nullptr; int* d_pfirst = nullptr; unsigned char* d_skip = nullptr;
  double* d_partial = nullptr;         // [n_pieces]
  double* d_segsum = nullptr;          // [n_seg]
};
