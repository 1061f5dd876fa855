// prt_histogram.hpp -- histograms of the result frame on the device.
//
// What a spot diagram, an irradiance map or the lens-design notebook's `ray_set.hist('y1')` (cell 19) does with the
// frame: bin one or two quantities of the selected rows, optionally weighted by a column.  The bin rule is numpy's
// (np.histogram / np.histogram2d): bin i takes v when edges[i] <= v < edges[i+1], the last bin also takes
// v == edges[n]; values outside [edges[0], edges[n]], NaN and +-inf are not counted, and a row counts in 2-D only
// when both of its values fall in a bin.  The edges themselves come from numpy on the host, so that the result is
// numpy's to the count.
//
// k_frame_histogram privatises the histogram in LDS: one or two 1024-thread workgroups per CU walk the rows
// grid-stride and add into a window of up to 65 536 16-bit counts (when a workgroup's share of the rows is below
// 2^16), 32 768 uint32 counts, or 10 922 uint32 counts with as many float64 weight sums, with LDS atomics, then
// flushes the window: by one global add per non-zero bin, or -- counts only, where a uniform spread would touch most
// of a large window -- by storing the window to a slab of its own that k_frame_histogram_fold adds up.  Either way
// (CUs x window) words leave LDS, not one global atomic per row.  A histogram larger than the window
// (n_groups * nx * ny bins) is tiled: one launch per window of the flattened bin space, each re-reading the columns
// it needs.  Counts are integer adds: exact and the same on every run.  Weight sums are float64 adds in an order that
// depends on the schedule: exact whenever the weights are integers and the sums stay below 2^53 (every built-in
// source emits intensity 100), otherwise equal up to the last bits.
#pragma once

static const int kHistBlock = 1024;                   // threads per workgroup: 16 waves
static const int kHistLdsBytes = 128 * 1024;          // the LDS window of one workgroup (of 160 KiB per CU)
static const int kHistMaxBlocksPerCu = 2;             // two 16-wave workgroups fill a CU's 32 wave slots

__device__ __forceinline__ double frame_value(const double* __restrict__ rows, int64_t ld, int64_t j, int quantity) {
  if (quantity == FRAME_AXIS_INTERCEPT)
    return rows[PRT_COL_X0 * ld + j] - rows[PRT_COL_XTILT * ld + j] * rows[PRT_COL_Y0 * ld + j] / rows[PRT_COL_YTILT * ld + j];
  return rows[(int64_t)quantity * ld + j];
}

// The bin of v among n bins with edges e[0..n] (non-decreasing), or -1.  Uniform edges: numpy's fast path -- a guess
// by arithmetic, corrected by comparing with the edges themselves, so the answer is the edges' and not the guess's.
// Otherwise a binary search for the largest i < n with e[i] <= v (= searchsorted(e, v, "right") - 1, with v == e[n]
// in the last bin).
__device__ __forceinline__ int hist_bin(double v, const double* __restrict__ e, int n, int uniform) {
  if (!(v >= e[0] && v <= e[n])) return -1;  // (NaN fails both)
  int i;
  if (uniform) {
    const double f = (v - e[0]) * ((double)n / (e[n] - e[0]));
    i = f >= (double)(n - 1) ? n - 1 : (f > 0.0 ? (int)f : 0);  // (NaN / inf guesses land on an end)
    while (i > 0 && v < e[i]) --i;
    while (i < n - 1 && v >= e[i + 1]) ++i;
  } else {
    int lo = 0, hi = n;  // e[lo] <= v; the answer is below hi
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (e[mid] <= v) lo = mid; else hi = mid;
    }
    i = lo;
  }
  return i;
}

// One window [first_bin, first_bin + window) of the flattened (n_groups, nx, ny) histogram.  y_quantity < 0: 1-D
// (ny = 1).  weights: null for counts only, else the window's float64 sums of rows[weight_column].
__global__ void __launch_bounds__(kHistBlock)
k_frame_histogram(const double* __restrict__ rows, int64_t ld, int64_t n_rows, double surface, double generation,
                  double rays_per_source, int n_groups, int x_quantity, const double* __restrict__ x_edges, int nx,
                  int x_uniform, int y_quantity, const double* __restrict__ y_edges, int ny, int y_uniform,
                  int weight_column, int64_t first_bin, int window, int packed, unsigned long long* __restrict__ counts,
                  double* __restrict__ weights, unsigned* __restrict__ slab) {
  extern __shared__ double hist_lds[];
  double* const sums = hist_lds;                                          // window doubles (weights only)
  unsigned* const tally = (unsigned*)(hist_lds + (weights ? window : 0));  // window uint32, or two uint16 a word
  const int words = packed ? (window + 1) >> 1 : window;
  for (int k = threadIdx.x; k < words; k += kHistBlock) tally[k] = 0u;
  if (weights)
    for (int k = threadIdx.x; k < window; k += kHistBlock) sums[k] = 0.0;
  __syncthreads();
  const bool any_surface = surface != surface, any_generation = generation != generation;  // NaN = no filter
  const int64_t stride = (int64_t)gridDim.x * kHistBlock;
  for (int64_t j = (int64_t)blockIdx.x * kHistBlock + threadIdx.x; j < n_rows; j += stride) {
    if (!any_surface && rows[PRT_COL_SURFACE * ld + j] != surface) continue;
    if (!any_generation && rows[PRT_COL_GENERATION * ld + j] != generation) continue;
    int group = 0;
    if (rays_per_source > 0) {
      const double g = floor(rows[PRT_COL_ID * ld + j] / rays_per_source);  // _pyrayt.py:352
      if (!(g >= 0 && g < (double)n_groups)) continue;
      group = (int)g;
    }
    const int ix = hist_bin(frame_value(rows, ld, j, x_quantity), x_edges, nx, x_uniform);
    if (ix < 0) continue;
    int iy = 0;
    if (y_quantity >= 0) {
      iy = hist_bin(frame_value(rows, ld, j, y_quantity), y_edges, ny, y_uniform);
      if (iy < 0) continue;
    }
    const int64_t b = ((int64_t)group * nx + ix) * ny + iy - first_bin;
    if (b < 0 || b >= window) continue;
    if (packed) atomicAdd(tally + (b >> 1), 1u << ((b & 1) << 4));  // (a half never carries: < 65536 rows a workgroup)
    else atomicAdd(tally + b, 1u);
    if (weights) atomicAdd(sums + b, rows[(int64_t)weight_column * ld + j]);
  }
  __syncthreads();
  if (slab) {  // counts only: the window's words as they are, into this workgroup's slab (k_frame_histogram_fold adds them)
    unsigned* const mine = slab + (size_t)blockIdx.x * words;
    for (int k = threadIdx.x; k < words; k += kHistBlock) mine[k] = tally[k];
    return;
  }
  // flush: consecutive lanes read consecutive bins and add the non-zero ones (a workgroup counts at most
  // ceil(n_rows / grid) rows, far below 2^32)
  for (int k = threadIdx.x; k < window; k += kHistBlock) {
    const unsigned c = packed ? (tally[k >> 1] >> ((k & 1) << 4)) & 0xffffu : tally[k];
    if (c) {
      atomicAdd(counts + first_bin + k, (unsigned long long)c);
      if (weights) atomicAdd(weights + first_bin + k, sums[k]);
    }
  }
}

// The slabs of one window added up: thread t sums word t % words over the workgroups of chunk t / words and adds the
// sum (two sums for packed tallies) to the output -- kHistFoldChunks contiguous integer adds a bin.
static const int kHistFoldChunks = 8;
__global__ void __launch_bounds__(PRT_BLOCK)
k_frame_histogram_fold(const unsigned* __restrict__ slab, int blocks, int words, int window, int packed,
                       unsigned long long* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (t >= (int64_t)words * kHistFoldChunks) return;
  const int w = (int)(t % words), chunk = (int)(t / words);
  const int per = (blocks + kHistFoldChunks - 1) / kHistFoldChunks;
  const int b1 = (chunk + 1) * per < blocks ? (chunk + 1) * per : blocks;
  unsigned long long lo = 0, hi = 0;
  for (int b = chunk * per; b < b1; ++b) {
    const unsigned v = slab[(size_t)b * words + w];
    if (packed) { lo += v & 0xffffu; hi += v >> 16; } else lo += v;
  }
  if (!packed) {
    if (lo) atomicAdd(counts + w, lo);
  } else {
    if (lo) atomicAdd(counts + 2 * w, lo);
    if (hi && 2 * w + 1 < window) atomicAdd(counts + 2 * w + 1, hi);
  }
}

// ---- the automatic range: min / max of the finite values of one quantity over the selected rows ----------------
// Reduced per lane and per wave, then combined with integer atomics on an order-preserving image of the double
// (sign-magnitude -> two's complement): the result does not depend on the order of arrival.
__device__ __forceinline__ long long ordered_key(double v) {
  const long long bits = __double_as_longlong(v);
  return bits >= 0 ? bits : bits ^ 0x7fffffffffffffffll;
}

__device__ __forceinline__ double key_value(long long key) {
  return __longlong_as_double(key >= 0 ? key : key ^ 0x7fffffffffffffffll);
}

__global__ void k_frame_range_init(long long* keys) {
  keys[0] = 0x7fffffffffffffffll;   // min of nothing
  keys[1] = -0x7fffffffffffffffll - 1;
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_frame_range(const double* __restrict__ rows, int64_t ld, int64_t n_rows, double surface, double generation,
              int quantity, long long* __restrict__ keys) {
  const bool any_surface = surface != surface, any_generation = generation != generation;
  long long lo = 0x7fffffffffffffffll, hi = -0x7fffffffffffffffll - 1;
  const int64_t stride = (int64_t)gridDim.x * PRT_BLOCK;
  for (int64_t j = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x; j < n_rows; j += stride) {
    if (!any_surface && rows[PRT_COL_SURFACE * ld + j] != surface) continue;
    if (!any_generation && rows[PRT_COL_GENERATION * ld + j] != generation) continue;
    const double v = frame_value(rows, ld, j, quantity);
    if (!(v == v && fabs(v) < PRT_INF)) continue;
    const long long k = ordered_key(v);
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long a = __shfl_xor(lo, off), b = __shfl_xor(hi, off);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  // ... and across the workgroup's waves: one atomic pair a workgroup (every atomic goes to the same two words, and
  // same-address atomics serialise: one a wave cost 96 us at 1M rows)
  __shared__ long long wave_lo[PRT_BLOCK / 64], wave_hi[PRT_BLOCK / 64];
  if ((threadIdx.x & 63) == 0) { wave_lo[threadIdx.x >> 6] = lo; wave_hi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < PRT_BLOCK / 64; ++w) {
      lo = wave_lo[w] < lo ? wave_lo[w] : lo;
      hi = wave_hi[w] > hi ? wave_hi[w] : hi;
    }
    if (lo != 0x7fffffffffffffffll) atomicMin(keys, lo);
    if (hi != -0x7fffffffffffffffll - 1) atomicMax(keys + 1, hi);
  }
}

__global__ void k_frame_range_finish(double* minmax) {  // the keys, in place, back to doubles (+inf, -inf: nothing)
  long long* keys = (long long*)minmax;
  const long long lo = keys[0], hi = keys[1];
  minmax[0] = lo == 0x7fffffffffffffffll ? PRT_INF : key_value(lo);
  minmax[1] = hi == -0x7fffffffffffffffll - 1 ? -PRT_INF : key_value(hi);
}

static int hist_cus(int device, int* cus) {
  HIP_TRY(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device));
  if (*cus < 1) *cus = 1;
  return PRT_OK;
}

extern "C" int prt_frame_range(int device, const double* rows, int64_t ld, int64_t n_rows, double surface,
                               double generation, int quantity, double* minmax_out, void* stream) {
  if (n_rows < 0 || ld < n_rows || !minmax_out || (n_rows && !rows)) return fail(PRT_ERR_ARG, "bad buffers");
  if (quantity < 0 || quantity > FRAME_AXIS_INTERCEPT)
    return fail(PRT_ERR_ARG, "quantity: a frame column 0..14 or 15 (axis intercept)");
  int rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  long long* keys = (long long*)minmax_out;
  hipLaunchKernelGGL(k_frame_range_init, dim3(1), dim3(1), 0, st, keys);
  if (n_rows > 0) {
    int cus = 1;
    rc = hist_cus(device, &cus);
    if (rc) return rc;
    const int64_t blocks = (n_rows + PRT_BLOCK - 1) / PRT_BLOCK;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks, (int64_t)cus);
    hipLaunchKernelGGL(k_frame_range, dim3(grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, surface, generation,
                       quantity, keys);
  }
  hipLaunchKernelGGL(k_frame_range_finish, dim3(1), dim3(1), 0, st, minmax_out);
  HIP_TRY(hipGetLastError());
  return PRT_OK;
}

static int64_t hist_edges_count(int nx, int ny) { return (int64_t)nx + 1 + (ny >= 1 ? (int64_t)ny + 1 : 0); }

extern "C" int64_t prt_frame_histogram_workspace_bytes(int n_groups, int nx, int ny, int with_weights) {
  (void)with_weights;  // (the weight sums live in LDS and in weights_out: nothing more to hold)
  if (n_groups < 1 || nx < 1) return PRT_ERR_ARG;
  return hist_edges_count(nx, ny) * (int64_t)sizeof(double);
}

static bool edges_ok(const double* e, int n) {
  if (!e) return false;
  for (int i = 0; i <= n; ++i)
    if (!std::isfinite(e[i]) || (i > 0 && e[i] < e[i - 1])) return false;
  return true;
}

extern "C" int prt_frame_histogram(int device, const double* rows, int64_t ld, int64_t n_rows, double surface,
                                   double generation, double rays_per_source, int n_groups, int x_quantity,
                                   const double* x_edges, int nx, int x_uniform, int y_quantity, const double* y_edges,
                                   int ny, int y_uniform, int weight_column, int64_t* counts_out, double* weights_out,
                                   void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  if (n_rows < 0 || ld < n_rows || n_groups < 1 || !counts_out || !workspace || (n_rows && !rows))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (!(rays_per_source > 0) && n_groups != 1) return fail(PRT_ERR_ARG, "one group without rays_per_source");
  const bool two_d = y_quantity >= 0;
  if (x_quantity < 0 || x_quantity > FRAME_AXIS_INTERCEPT || y_quantity > FRAME_AXIS_INTERCEPT || y_quantity < -1)
    return fail(PRT_ERR_ARG, "quantity: a frame column 0..14 or 15 (axis intercept); y_quantity -1: one dimension");
  if (nx < 1 || (two_d && ny < 1)) return fail(PRT_ERR_ARG, "nx, ny: at least one bin");
  if (!edges_ok(x_edges, nx) || (two_d && !edges_ok(y_edges, ny)))
    return fail(PRT_ERR_ARG, "edges: finite and monotonically increasing, host memory");
  if (weight_column < -1 || weight_column >= PRT_RECORD_COLS) return fail(PRT_ERR_ARG, "weight_column: 0..14 or -1");
  if ((weight_column >= 0) != (weights_out != nullptr)) return fail(PRT_ERR_ARG, "weights_out goes with weight_column");
  if (!two_d) ny = 1;
  const int64_t bins = (int64_t)n_groups * nx * ny;
  if (bins / n_groups / nx != ny || bins > ((int64_t)1 << 40)) return fail(PRT_ERR_ARG, "too many bins");
  int rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  double* x_dev = (double*)workspace;
  double* y_dev = x_dev + nx + 1;
  HIP_TRY(hipMemcpyAsync(x_dev, x_edges, (size_t)(nx + 1) * sizeof(double), hipMemcpyHostToDevice, st));
  if (two_d) HIP_TRY(hipMemcpyAsync(y_dev, y_edges, (size_t)(ny + 1) * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(counts_out, 0, (size_t)bins * sizeof(int64_t), st));
  if (weights_out) HIP_TRY(hipMemsetAsync(weights_out, 0, (size_t)bins * sizeof(double), st));
  if (n_rows == 0) return PRT_OK;
  int cus = 1;
  rc = hist_cus(device, &cus);
  if (rc) return rc;
  // counts only, and a workgroup's share of the rows below 2^16 (1M rows: 4 096 a workgroup): two 16-bit tallies a
  // word, so the window holds 65 536 bins -- a 256 x 256 histogram in one pass over the rows
  const int64_t blocks = (n_rows + kHistBlock - 1) / kHistBlock;
  const int64_t one_per_cu = std::min<int64_t>(blocks, cus);
  const int64_t per_thread = (n_rows + one_per_cu * kHistBlock - 1) / (one_per_cu * kHistBlock);
  const int packed = !weights_out && per_thread * kHistBlock < 65536;
  const int window = (int)std::min<int64_t>(bins, packed ? 2 * kHistLdsBytes / 4 : kHistLdsBytes / (weights_out ? 12 : 4));
  const size_t lds = weights_out ? (size_t)window * 12 : packed ? (size_t)((window + 1) / 2) * 4 : (size_t)window * 4;
  HIP_TRY(hipFuncSetAttribute((const void*)k_frame_histogram, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // (packed tallies need every workgroup's share of the rows below 2^16: one workgroup per CU then)
  const int per_cu = packed ? 1 : (int)std::max<size_t>(1, std::min<size_t>(kHistMaxBlocksPerCu, (size_t)(160 * 1024) / std::max<size_t>(lds, 1)));
  const unsigned grid = (unsigned)std::min<int64_t>(blocks, (int64_t)cus * per_cu);
  // The flush.  Atomic: every workgroup adds its window's non-zero bins to the output, one global add each; what that
  // costs is the 64-byte segments of the output it touches.  Slab: every workgroup stores its window's words (plain
  // stores) and k_frame_histogram_fold adds them up in eight chunks of workgroups, with contiguous adds.  Measured at
  // 1M rows (profiles/histogram/): 256 x 256 bins, uniform spread 54 us atomic / 38 us slab, concentrated spot 19 / 31;
  // 64 x 64 bins 16 / 20; 1024 x 1024 bins (16 windows, few rows in each) 17 / 33 us a window.  So the slab is taken
  // where a uniform spread -- the worst case for the atomic flush -- would touch a large share of a big window's
  // segments: atomic ~ 90 us x touched share x (window / 65 536), slab ~ 10 + 20 x (window / 65 536).  Weight sums
  // always flush by atomics (their order is free anyway, and a float64 slab would be four times the bytes).
  const int words = packed ? (window + 1) / 2 : window;
  const double per_window_rows = (double)n_rows / grid * ((double)window / (double)bins);  // a workgroup's, if spread
  const double touched = 1.0 - std::exp(-8.0 * per_window_rows / window), share = window / 65536.0;
  unsigned* slab = nullptr;
  if (!weights_out && 90.0 * touched * share > 10.0 + 20.0 * share)
    HIP_TRY(hipMallocAsync((void**)&slab, (size_t)grid * words * sizeof(unsigned), st));
  for (int64_t first = 0; first < bins; first += window) {
    const int this_window = (int)std::min<int64_t>(window, bins - first);
    hipLaunchKernelGGL(k_frame_histogram, dim3(grid), dim3(kHistBlock), lds, st, rows, ld, n_rows, surface, generation,
                       rays_per_source, n_groups, x_quantity, x_dev, nx, x_uniform, two_d ? y_quantity : -1, y_dev,
                       ny, y_uniform, weight_column, first, this_window, packed, (unsigned long long*)counts_out,
                       weights_out, slab);
    if (slab) {
      const int this_words = packed ? (this_window + 1) / 2 : this_window;
      const int64_t threads = (int64_t)this_words * kHistFoldChunks;
      hipLaunchKernelGGL(k_frame_histogram_fold, dim3((unsigned)((threads + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK),
                         0, st, slab, (int)grid, this_words, this_window, packed,
                         (unsigned long long*)counts_out + first);
    }
  }
  if (slab) HIP_TRY(hipFreeAsync(slab, st));
  HIP_TRY(hipGetLastError());
  return PRT_OK;
}
