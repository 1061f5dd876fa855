// prt_sort.hpp -- the stable counting sort that every image pass of the frame begins with: the
// rows are cut into contiguous runs, a wave each; every wave counts its rows per bucket, the counts are scanned into
// each wave's place inside each bucket, and every wave writes its rows there in row order.  A bucket is a group, a
// (group, wavelength), a (group, zone) or a (group, state): the pass says which.  Here is the sort and nothing of the
// sums: the plan of the runs (sort_plan), a wave's run (sort_run), the ballot loop (sort_turns, and sort_tally and
// sort_place on it), the scan (sort_scan) and the fixed tree that the sums' workgroups end with (sort_tree).
//
//   k_sort_positions   one workgroup: the waves' totals scanned into the rows before each wave
//   k_sort_offsets     per bucket: the waves' counts scanned into each wave's offset inside the bucket; its total
//   k_sort_starts      one workgroup: the buckets' totals scanned into each bucket's start
// Everything here is integer arithmetic: the same on every run, and the same however the rows are cut.  The order of a
// bucket's rows is the rows' own, so rows that no pass selects change nothing.
// (included by prt_wavefront.hpp, below kWfRowsPerWave and kWfMaxWaves)
#pragma once

static const int kSortScanBlock = 512;  // threads of a scan workgroup

// ---- host: the runs ---------------------------------------------------------------------------------------------------
// n_rows items in waves of contiguous runs: kWfRowsPerWave items a wave at least, kWfMaxWaves waves at most, and no more
// waves than the (wave, bucket) cells of cell_bytes each fit in cap_bytes; a run is whole 64-item steps; the launch is
// whole workgroups of PRT_BLOCK / 64 waves (the ones past the items count nothing)
struct SortPlan {
  int64_t per_wave, all_waves;
  unsigned grid;
  size_t count_bytes;
};
static SortPlan sort_plan(int64_t n_rows, int64_t buckets, size_t cell_bytes, size_t cap_bytes) {
  SortPlan p;
  int64_t waves = (n_rows + kWfRowsPerWave - 1) / kWfRowsPerWave;
  waves = std::min<int64_t>(std::max<int64_t>(waves, 1), kWfMaxWaves);
  waves = std::max<int64_t>(1, std::min<int64_t>(waves, (int64_t)(cap_bytes / ((size_t)buckets * cell_bytes))));
  const int64_t per_wave = ((n_rows + waves - 1) / waves + 63) / 64 * 64;
  const unsigned grid = (unsigned)((waves + PRT_BLOCK / 64 - 1) / (PRT_BLOCK / 64));
  const int64_t all_waves = (int64_t)grid * (PRT_BLOCK / 64);
  p.per_wave = per_wave, p.all_waves = all_waves, p.grid = grid;
  p.count_bytes = (size_t)all_waves * buckets * cell_bytes;
  return p;
}

// ---- device: a wave's run and the ballot loop -------------------------------------------------------------------------
// the run [first, last) of this wave of a PRT_BLOCK workgroup among n items, per_wave a wave
struct SortRun { int lane; int64_t wave, first, last; };
__device__ __forceinline__ int64_t sort_wave() { return (int64_t)blockIdx.x * (PRT_BLOCK / 64) + (threadIdx.x >> 6); }
__device__ __forceinline__ SortRun sort_run(int64_t per_wave, int64_t n) {
  SortRun r;
  r.lane = threadIdx.x & 63;
  r.wave = sort_wave();
  r.first = r.wave * per_wave;
  r.last = r.first + per_wave < n ? r.first + per_wave : n;
  return r;
}

// a wave's 64 rows, `key` < 0 for a row left out: one turn per key present, in the order of the keys' first rows --
// almost always exactly one turn.  body(k, take): k the key, take the ballot of its rows, both wave-uniform
template <class Body>
__device__ __forceinline__ void sort_turns(int key, Body body) {
  unsigned long long pending = __ballot(key >= 0);
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    const int k = __shfl(key, leader);
    const unsigned long long take = __ballot(key == k);
    body(k, take);
    pending &= ~take;
  }
}

// mine[k] += the rows of key k (mine: this wave's cells, which no other wave touches)
__device__ __forceinline__ void sort_tally(int lane, int key, int64_t* mine) {
  sort_turns(key, [&](int k, unsigned long long take) {
    if (lane == 0) mine[k] += __popcll(take);
  });
}

// put(place) for every row kept, place = bucket_start[k] + the wave's offset mine[k] + the rows of k in lower lanes;
// mine[k] advances by the rows taken, so that the rows of a bucket keep their order from step to step
template <class Put>
__device__ __forceinline__ void sort_place(int lane, int key, int64_t* mine, const int64_t* __restrict__ bucket_start,
                                           Put put) {
  sort_turns(key, [&](int k, unsigned long long take) {
    int64_t at = lane == 0 ? mine[k] : 0;
    at = __shfl(at, 0);
    if (key == k) put(bucket_start[k] + at + __popcll(take & ((1ull << lane) - 1ull)));
    if (lane == 0) mine[k] = at + __popcll(take);
  });
}

// ---- device: the scan and the tree ------------------------------------------------------------------------------------
// an exclusive scan of n int64 values by one workgroup of kSortScanBlock threads, each owning a contiguous run:
// get(k) reads value k, put(k, before) receives the sum of the values before it; returns the total
template <class Get, class Put>
__device__ int64_t sort_scan(int64_t n, Get get, Put put, int64_t* __restrict__ scan) {
  const int64_t per = (n + kSortScanBlock - 1) / kSortScanBlock;
  const int64_t lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  int64_t mine = 0;
  for (int64_t k = lo; k < hi; ++k) mine += get(k);
  __syncthreads();  // (scan may still be read by a previous call)
  scan[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < kSortScanBlock; off <<= 1) {
    const int64_t add = (int)threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
    __syncthreads();
    scan[threadIdx.x] += add;
    __syncthreads();
  }
  int64_t at = scan[threadIdx.x] - mine;
  for (int64_t k = lo; k < hi; ++k) {
    const int64_t v = get(k);
    put(k, at);
    at += v;
  }
  return scan[kSortScanBlock - 1];
}

// red[k][0] = red[k][0 .. BLOCK) joined for every k, in a fixed tree: join(k, red[k][t], red[k][t + half]) folds the
// second into the first
template <int N, int BLOCK, class T, class Join>
__device__ __forceinline__ void sort_tree(T (&red)[N][BLOCK], int t, Join join) {
  for (int half = BLOCK / 2; half > 0; half >>= 1) {
    __syncthreads();
    if (t < half)
      for (int k = 0; k < N; ++k) join(k, red[k][t], red[k][t + half]);
  }
  __syncthreads();
}
// ... the sum of each
template <int N, int BLOCK, class T>
__device__ __forceinline__ void sort_tree(T (&red)[N][BLOCK], int t) {
  sort_tree(red, t, [](int, T& a, T b) { a += b; });
}

// ---- the kernels ------------------------------------------------------------------------------------------------------
// wave_before[w] = the rows of the waves before w (it may be wave_rows itself)
__global__ void __launch_bounds__(kSortScanBlock)
k_sort_positions(int waves, const int64_t* wave_rows, int64_t* wave_before) {
  __shared__ int64_t scan[kSortScanBlock];
  sort_scan(
      waves, [&](int64_t w) { return wave_rows[w]; }, [&](int64_t w, int64_t before) { wave_before[w] = before; }, scan);
}

// per bucket (one workgroup each): counts[wave][b] -> the wave's first position inside the bucket, in place
__global__ void __launch_bounds__(kSortScanBlock)
k_sort_offsets(int waves, int buckets, int64_t* __restrict__ counts, int64_t* __restrict__ bucket_total) {
  __shared__ int64_t scan[kSortScanBlock];
  const int b = blockIdx.x;
  const int64_t total = sort_scan(
      waves, [&](int64_t w) { return counts[w * buckets + b]; },
      [&](int64_t w, int64_t before) { counts[w * buckets + b] = before; }, scan);
  if (threadIdx.x == 0) bucket_total[b] = total;
}

__global__ void __launch_bounds__(kSortScanBlock)
k_sort_starts(int buckets, const int64_t* __restrict__ bucket_total, int64_t* __restrict__ bucket_start) {
  __shared__ int64_t scan[kSortScanBlock];
  sort_scan(
      buckets, [&](int64_t b) { return bucket_total[b]; }, [&](int64_t b, int64_t before) { bucket_start[b] = before; },
      scan);
}

// the two launches between a pass's tally and its scatter, where it needs no more than the buckets' starts
static void sort_offsets(hipStream_t st, int waves, int buckets, int64_t* counts, int64_t* bucket_total,
                         int64_t* bucket_start) {
  hipLaunchKernelGGL(k_sort_offsets, dim3((unsigned)buckets), dim3(kSortScanBlock), 0, st, waves, buckets, counts,
                     bucket_total);
  hipLaunchKernelGGL(k_sort_starts, dim3(1), dim3(kSortScanBlock), 0, st, buckets, bucket_total, bucket_start);
}
