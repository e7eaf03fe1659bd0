// taco_feed.h -- a ragged training batch gathered out of a device-resident corpus: taco_collate (include/taco_abi.h), the device twin
// of feeder.collate (_pad_target / _prepare_inputs of datasets/datafeeder.py:289-328).  Included by taco_lib.hip before its extern "C" block.
//
// Shape of the work.  An item of a stream is ONE contiguous run of rows * width words in the pack and its batch row is one contiguous
// run of rows_out * width words of the output, so whatever the width (1025 is odd) the copy is linear in memory: out[b][j] = item[j] for
// j < c * width, 0 after.  A C4-shard batch reads 70 MB and writes 71 MB; to fill 256 CUs every output row is cut into chunks of
// FEED_CHUNK words (16 KB) and (stream, row, chunk) is flattened into ONE grid: 4000 workgroups for the linear stream of that batch, 320
// for mel, 32 each for the small streams, all in the same launch.  The descriptors travel by value in the kernel arguments.
//
// Which side is aligned.  Source and destination differ in alignment modulo 16 bytes in general (item starts are arbitrary word offsets,
// and a batch row starts at b * rows_out * width words).  The STORES get the aligned 16-byte accesses: a store that covers only part of
// a line is a read-modify-write further out, and narrow stores cost several times the 16-byte store's time per byte, while a 16-byte
// load that is only dword-aligned is one instruction that touches at most one more line, which the neighbouring lane's load needs
// anyway (it stays in the L1/L2).  So per output row: up to 3 head words until the destination is 16-byte aligned (dword stores),
// then 16-byte stores fed by dword-aligned 16-byte loads (global_load_dwordx4 with 4-byte alignment), then up to 3 tail words.  The group
// that straddles the item's end is put together word by word, so no word past c * width is ever read, and everything after it is
// a store of zeros that reads nothing.  A lane issues its four loads before its four stores (4 x 16 B in flight per lane).
// Offsets are 64-bit throughout (a pack of linear targets passes 2^31 words at about 8 hours of audio).
#pragma once

#define FEED_NT 256
#define FEED_VEC_PER_LANE 4
#define FEED_CHUNK (FEED_NT * FEED_VEC_PER_LANE * 4)    // words of an output row per workgroup: 4096 (16 KB)

struct FeedArgs {
  taco_collate_stream s[TACO_COLLATE_MAX_STREAMS];
  int blk_end[TACO_COLLATE_MAX_STREAMS];     // first workgroup past stream s
  int nchunks[TACO_COLLATE_MAX_STREAMS];     // chunks per output row of stream s
  int n_streams, N;
};

typedef uint32_t feed_w4 __attribute__((ext_vector_type(4)));
typedef feed_w4 feed_w4u __attribute__((aligned(4)));                             // 16 bytes at dword alignment

__global__ __launch_bounds__(FEED_NT) void k_collate(const FeedArgs a, const int32_t* __restrict__ index) {
  const int blk = (int)blockIdx.x;
  int s = 0;
#pragma unroll
  for (int k = 0; k < TACO_COLLATE_MAX_STREAMS - 1; ++k)
    if (k + 1 < a.n_streams && blk >= a.blk_end[k]) s = k + 1;
  // select the stream's descriptor without indexing the argument block dynamically (that would put it in scratch)
  taco_collate_stream d = a.s[0];
  int first = 0, nch = a.nchunks[0];
#pragma unroll
  for (int k = 1; k < TACO_COLLATE_MAX_STREAMS; ++k)
    if (s == k) { d = a.s[k]; first = a.blk_end[k - 1]; nch = a.nchunks[k]; }
  const int rel = blk - first;
  const int b = rel / nch, chunk = rel - b * nch;
  const long long row_words = (long long)d.rows_out * d.width;
  const int i = index[b];
  int c = 0;
  long long src0 = 0;
  if (i >= 0 && i < a.N) {                     // an index outside the corpus reads nothing: an all-zero row, count 0
    c = d.rows ? d.rows[i] : d.rows_out;
    c = c < 0 ? 0 : (c > d.rows_out ? d.rows_out : c);
    src0 = d.start ? d.start[i] : (long long)i * row_words;
  }
  const long long ncopy = (long long)c * d.width;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(d.pack) + src0;
  uint32_t* dst = reinterpret_cast<uint32_t*>(d.out) + (long long)b * row_words;
  const int tid = (int)threadIdx.x;
  if (chunk == 0 && tid == 0 && d.counts) d.counts[b] = c;
  long long head = (long long)((0 - (reinterpret_cast<uintptr_t>(dst) >> 2)) & 3);     // words until dst is 16-byte aligned
  if (head > row_words) head = row_words;
  if (chunk == 0 && tid < head) dst[tid] = tid < ncopy ? src[tid] : 0u;
  const long long lo = head + (long long)chunk * FEED_CHUNK;
  const long long hi = lo + FEED_CHUNK < row_words ? lo + FEED_CHUNK : row_words;
  feed_w4 v[FEED_VEC_PER_LANE];
#pragma unroll
  for (int it = 0; it < FEED_VEC_PER_LANE; ++it) {
    const long long j = lo + 4 * (long long)(tid + it * FEED_NT);
    v[it] = (feed_w4)(0u);
    if (j + 4 <= ncopy && j + 4 <= hi) {
      v[it] = *reinterpret_cast<const feed_w4u*>(src + j);
    } else if (j < ncopy && j < hi) {          // the group that straddles the item's end (or the row's): word by word
      v[it].x = src[j];
      if (j + 1 < ncopy && j + 1 < hi) v[it].y = src[j + 1];
      if (j + 2 < ncopy && j + 2 < hi) v[it].z = src[j + 2];
    }
  }
#pragma unroll
  for (int it = 0; it < FEED_VEC_PER_LANE; ++it) {
    const long long j = lo + 4 * (long long)(tid + it * FEED_NT);
    if (j + 4 <= hi) {
      *reinterpret_cast<feed_w4*>(dst + j) = v[it];
    } else if (j < hi) {                       // the row's last 1..3 words
      dst[j] = v[it].x;
      if (j + 1 < hi) dst[j + 1] = v[it].y;
      if (j + 2 < hi) dst[j + 2] = v[it].z;
    }
  }
}

extern "C" int taco_collate(void* hip_stream, const taco_collate_stream* streams, int n_streams, const int32_t* d_index, int B, int N) {
  if (!streams || !d_index) return fail(TACO_ERR_ARG, "taco_collate: null streams or d_index");
  if (n_streams < 1 || n_streams > TACO_COLLATE_MAX_STREAMS)
    return fail(TACO_ERR_ARG, "taco_collate: n_streams %d outside [1, %d]", n_streams, TACO_COLLATE_MAX_STREAMS);
  if (B < 1 || N < 1) return fail(TACO_ERR_ARG, "taco_collate: B %d, N %d must be >= 1", B, N);
  FeedArgs a;
  memset(&a, 0, sizeof a);
  a.n_streams = n_streams;
  a.N = N;
  long long blocks = 0;
  for (int s = 0; s < n_streams; ++s) {
    const taco_collate_stream& d = streams[s];
    if (!d.pack || !d.out) return fail(TACO_ERR_ARG, "taco_collate: stream %d has a null pack or out", s);
    if (d.width < 1 || d.rows_out < 1) return fail(TACO_ERR_ARG, "taco_collate: stream %d: width %d, rows_out %d must be >= 1", s, d.width, d.rows_out);
    if (!d.start && d.rows) return fail(TACO_ERR_ARG, "taco_collate: stream %d: rows without start (the fixed-size form has neither)", s);
    if ((reinterpret_cast<uintptr_t>(d.pack) | reinterpret_cast<uintptr_t>(d.out)) & 3)
      return fail(TACO_ERR_ARG, "taco_collate: stream %d: pack and out must be 4-byte aligned", s);
    const long long row_words = (long long)d.rows_out * d.width;
    const long long nch = (row_words + FEED_CHUNK - 1) / FEED_CHUNK;
    blocks += nch * B;
    if (blocks > 0x7fffffffLL) return fail(TACO_ERR_ARG, "taco_collate: the batch needs more than 2^31 - 1 workgroups");
    a.s[s] = d;
    a.nchunks[s] = (int)nch;
    a.blk_end[s] = (int)blocks;
  }
  for (int s = n_streams; s < TACO_COLLATE_MAX_STREAMS; ++s) { a.blk_end[s] = (int)blocks; a.nchunks[s] = 1; }
  hipLaunchKernelGGL(k_collate, dim3((unsigned)blocks), dim3(FEED_NT), 0, (hipStream_t)hip_stream, a, d_index);
  HIPCHK(hipGetLastError());
  return 0;
}
