// prt_wavefront.hpp -- optical path, wavefront error (OPD) and its Zernike fit, on the device.
//
// The frame's rows (pyrayt/_pyrayt.py:168-186) hold every segment a ray ran: its start (x0..z0, relaunch offset
// included, _pyrayt.py:449), its end (x1..z1), its unit direction and the index of the medium.  A ray's optical path
// length up to a surface is the sum of index * |x1 - x0| over its rows of that generation and every earlier one.
//
// k_frame_optical_path: one launch per generation, in generation order on one stream, over a dense per-id accumulator
//   (ids in [id0, id0 + n_ids)).  A stamp per id says which generation wrote the accumulator last, so a row adds the
//   previous generation's value only when that generation held the same id, and an id seen twice in one generation
//   (an integer exchange on the stamp) or outside the range sets a status bit.  No id repeats within a generation,
//   so no two lanes touch the same accumulator: no races, no floating-point atomics.
// The wavefront at surface S, per group of rows (id // rays_per_source):
//   k_frame_wavefront_locate     pass 1: per wave, in-order sums of the rows' end and start points and the group's
//                                first row, into a slab of its own; the wave's count of selected rows
//   k_frame_wavefront_reference  folds the slab in wave order: the reference sphere (P, R) and the pivot per group;
//                                one more workgroup scans the waves' counts into output offsets (sort_scan)
//   k_frame_wavefront_pupil      pass 2: per row E, OPD and the pupil point, written compacted in row order; per
//                                group the largest pupil radius, the OPD's range and the misses (integer atomics on
//                                order-preserving images: the same on every run)
//   k_frame_zernike              the basis by recurrence in registers, a tile of rows in LDS, the normal-equation
//                                entries owned by threads and accumulated in a fixed order into a slab per workgroup
//   k_frame_zernike_fold         the slab added up in workgroup order; the group records finished
//   k_frame_wavefront_piston     the group's (weighted) mean OPD taken off the per-row OPD
// Every floating-point sum is formed in an order fixed by the data and the launch shape: bit-identical run to run.
#pragma once

static const int kWfMaxWaves = 2048;           // waves of the row passes (each walks a contiguous run of rows)
static const int kWfRowsPerWave = 1024;        // ... at least this many rows a wave
static const int kWfZBlock = 256;              // threads of a k_frame_zernike workgroup = rows of its LDS tile
static const int kWfMaxZBlocks = 512;
static const size_t kWfSlabBytes = 64u << 20;  // cap on a slab of per-wave / per-workgroup partial sums
enum { WF_LOC = 8, WF_GROUP = 12, WF_MAX_TERMS = 36 };
#include "prt_sort.hpp"  // (the runs of the row passes and the scan: it reads kWfMaxWaves and kWfRowsPerWave)
// group record (n_groups, 12) float64: [0..2] P  [3] R  [4] pivot  [5] pupil radius  [6] rows  [7] rows that miss
// the sphere  [8] largest and [9] smallest OPD about the pivot  [10] first row  [11] largest radial extent
// (during the passes [7] is an int64 count, [8] / [9] order-preserving keys, [11] the bits of a non-negative double)

__host__ __device__ constexpr int wf_entries(int terms) { return terms * (terms + 1) / 2 + terms + 3; }

// Noll (1976): j = 1.. -> (n, m), m > 0 for cos(m theta) (even j), m < 0 for sin (odd j)
__host__ __device__ constexpr int noll_n(int j) {
  int n = 0, k = j - 1;
  while (k > n) { ++n; k -= n; }
  return n;
}
__host__ __device__ constexpr int noll_m(int j) {
  int n = 0, k = j - 1;
  while (k > n) { ++n; k -= n; }
  const int m = (n % 2) + 2 * ((k + ((n + 1) % 2)) / 2);
  return (j % 2) ? -m : m;
}

struct NollTable { int n[WF_MAX_TERMS], m[WF_MAX_TERMS]; };
__host__ __device__ constexpr NollTable noll_table() {
  NollTable t{};
  for (int j = 1; j <= WF_MAX_TERMS; ++j) { t.n[j - 1] = noll_n(j); t.m[j - 1] = noll_m(j); }
  return t;
}

__device__ __forceinline__ bool wf_selected(const double* __restrict__ rows, int64_t ld, int64_t j, double surface,
                                            double generation) {
  return (surface != surface || rows[PRT_COL_SURFACE * ld + j] == surface) &&
         (generation != generation || rows[PRT_COL_GENERATION * ld + j] == generation);
}

__device__ __forceinline__ int wf_group(const double* __restrict__ rows, int64_t ld, int64_t j, double rays_per_source,
                                        int n_groups) {
  if (!(rays_per_source > 0)) return 0;
  const double g = floor(rows[PRT_COL_ID * ld + j] / rays_per_source);  // _pyrayt.py:352
  return (g >= 0 && g < (double)n_groups) ? (int)g : -1;
}

// ---- optical path -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PRT_BLOCK)
k_frame_optical_path(const double* __restrict__ rows, int64_t ld, int64_t start, int64_t count, int generation,
                     double id0, int64_t n_ids, double* __restrict__ acc, int* __restrict__ stamp,
                     double* __restrict__ opl, int* __restrict__ status) {
  const int64_t j = start + (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (j >= start + count) return;
  const double dx = rows[PRT_COL_X1 * ld + j] - rows[PRT_COL_X0 * ld + j];
  const double dy = rows[PRT_COL_Y1 * ld + j] - rows[PRT_COL_Y0 * ld + j];
  const double dz = rows[PRT_COL_Z1 * ld + j] - rows[PRT_COL_Z0 * ld + j];
  const double segment = rows[PRT_COL_INDEX * ld + j] * sqrt(dx * dx + dy * dy + dz * dz);
  const int64_t i = join_id(rows, ld, j, id0, n_ids);
  if (i < 0) {
    atomicOr(status, JOIN_BAD_ID);
    opl[j] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const int bits = join_status(join_claim(stamp, i, generation), generation);  // (0: acc[i] is generation - 1's)
  if (bits & JOIN_REPEATED_ID) atomicOr(status, JOIN_REPEATED_ID);
  // (a missing generation is not refused here: the sum starts again)
  const double cumulative = (generation > 0 && !bits ? acc[i] : 0.0) + segment;
  acc[i] = cumulative;
  opl[j] = cumulative;
}

// ---- pass 1: where each group's rows are ---------------------------------------------------------------------------
// per wave and group: [0] rows  [1..3] sum (x1, y1, z1)  [4..6] sum (x0, y0, z0)  [7] n_rows - (first row)  (max)
__device__ __forceinline__ void wf_locate_flush(double (&acc)[WF_LOC], int group, double* __restrict__ mine) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < WF_LOC; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(v, off);
      v = k == 7 ? fmax(v, o) : v + o;
    }
    if (lane == 0) {
      double* slot = mine + (size_t)group * WF_LOC + k;
      *slot = k == 7 ? fmax(*slot, v) : *slot + v;
    }
    acc[k] = 0.0;
  }
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_frame_wavefront_locate(const double* __restrict__ rows, int64_t ld, int64_t n_rows, double surface,
                         double generation, double rays_per_source, int n_groups, int64_t per_wave,
                         double* __restrict__ slab, int64_t* __restrict__ wave_rows) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (PRT_BLOCK / 64) + (threadIdx.x >> 6);
  const int64_t first = wave * per_wave;
  const int64_t last = first + per_wave < n_rows ? first + per_wave : n_rows;
  double* const mine = slab + (size_t)wave * n_groups * WF_LOC;  // (only this wave writes here)
  double acc[WF_LOC] = {0, 0, 0, 0, 0, 0, 0, 0};
  int current = -1;
  int64_t selected = 0;
  for (int64_t base = first; base < last; base += 64) {
    const int64_t j = base + lane;
    int group = -1;
    if (j < last && wf_selected(rows, ld, j, surface, generation)) group = wf_group(rows, ld, j, rays_per_source, n_groups);
    double v[WF_LOC] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (group >= 0) {
      v[0] = 1.0;
      v[1] = rows[PRT_COL_X1 * ld + j]; v[2] = rows[PRT_COL_Y1 * ld + j]; v[3] = rows[PRT_COL_Z1 * ld + j];
      v[4] = rows[PRT_COL_X0 * ld + j]; v[5] = rows[PRT_COL_Y0 * ld + j]; v[6] = rows[PRT_COL_Z0 * ld + j];
      v[7] = (double)(n_rows - j);
    }
    unsigned long long pending = __ballot(group >= 0);
    selected += __popcll(pending);
    while (pending) {  // one turn per group present in the slice: almost always exactly one
      const int leader = __ffsll((long long)pending) - 1;
      const int g = __shfl(group, leader);
      if (g != current) {
        if (current >= 0) wf_locate_flush(acc, current, mine);
        current = g;
      }
      const bool take = group == g;
      if (take) {
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[k] += v[k];
        acc[7] = fmax(acc[7], v[7]);
      }
      pending &= ~__ballot(take);
    }
  }
  if (current >= 0) wf_locate_flush(acc, current, mine);
  if (lane == 0) wave_rows[wave] = selected;
}

// E = Q - s u on the sphere (P, R), the larger root s; false when the ray's line misses the sphere
__device__ __forceinline__ bool wf_extend(const double* __restrict__ rows, int64_t ld, int64_t j,
                                          const double* __restrict__ p, double radius, double& s, double (&e)[3]) {
  const double q[3] = {rows[PRT_COL_X1 * ld + j], rows[PRT_COL_Y1 * ld + j], rows[PRT_COL_Z1 * ld + j]};
  const double u[3] = {rows[PRT_COL_XTILT * ld + j], rows[PRT_COL_YTILT * ld + j], rows[PRT_COL_ZTILT * ld + j]};
  const double d[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
  const double a = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
  const double b = d[0] * u[0] + d[1] * u[1] + d[2] * u[2];
  const double c = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) - radius * radius;
  const double disc = b * b - a * c;
  if (!(disc >= 0.0 && a > 0.0)) return false;
  const double root = sqrt(disc);
  s = b >= 0.0 ? (b + root) / a : -c / (root - b);  // (the larger root, without cancellation)
  if (!(s == s && fabs(s) < PRT_INF)) return false;
  for (int k = 0; k < 3; ++k) e[k] = q[k] - s * u[k];
  return true;
}

// ---- the reference sphere and the pivot; the output offsets ------------------------------------------------------
static const int kWfRefBlock = 512;  // 8 waves: one per pass-1 statistic
static_assert(kWfRefBlock == kSortScanBlock, "the last workgroup of k_frame_wavefront_reference runs sort_scan");
__global__ void __launch_bounds__(kWfRefBlock)
k_frame_wavefront_reference(const double* __restrict__ rows, int64_t ld, int64_t n_rows,
                            const double* __restrict__ opl, double surface, double generation, double rays_per_source,
                            int n_groups, int waves, const double* __restrict__ slab,
                            const double* __restrict__ reference, const double* __restrict__ radius,
                            double* __restrict__ group_out, const int64_t* __restrict__ wave_rows,
                            int64_t* __restrict__ wave_offset, int64_t* __restrict__ total) {
  __shared__ double stat[WF_LOC];
  __shared__ int64_t scan[kWfRefBlock];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if ((int)blockIdx.x == n_groups) {  // the last workgroup: exclusive scan of the waves' selected rows
    const int64_t all = sort_scan(
        waves, [&](int64_t k) { return wave_rows[k]; }, [&](int64_t k, int64_t before) { wave_offset[k] = before; }, scan);
    if (threadIdx.x == 0) *total = all;
    return;
  }
  const int g = blockIdx.x;
  {  // wave w folds statistic w over the waves of pass 1: lane-strided, then a fixed butterfly
    double v = 0.0;
    for (int k = lane; k < waves; k += 64) {
      const double x = slab[((size_t)k * n_groups + g) * WF_LOC + w];
      v = w == 7 ? fmax(v, x) : v + x;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(v, off);
      v = w == 7 ? fmax(v, o) : v + o;
    }
    if (lane == 0) stat[w] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double* o = group_out + (size_t)g * WF_GROUP;
  const double count = stat[0];
  o[6] = count;
  ((long long*)o)[7] = 0;                        // misses (int64 until the end)
  ((long long*)o)[8] = -0x7fffffffffffffffll - 1;  // largest OPD (key)
  ((long long*)o)[9] = 0x7fffffffffffffffll;       // smallest OPD (key)
  ((unsigned long long*)o)[11] = 0ull;             // largest radial extent (bits)
  if (count == 0) {
    for (int k = 0; k < 6; ++k) o[k] = nan;
    o[10] = nan;
    return;
  }
  double p[3];
  for (int k = 0; k < 3; ++k) p[k] = reference ? reference[3 * g + k] : stat[1 + k] / count;
  double r = radius ? radius[g] : nan;
  if (!(r > 0.0 && r < PRT_INF)) {  // default: from P to the mean start of the segments that end at S
    const double dx = stat[4] / count - p[0], dy = stat[5] / count - p[1], dz = stat[6] / count - p[2];
    r = sqrt(dx * dx + dy * dy + dz * dz);
  }
  // the pivot: the first row of the group, in row order, whose line meets the sphere (almost always the first row)
  const int64_t j = n_rows - (int64_t)stat[7];
  double s, e[3], pivot = nan;
  for (int64_t k = j; k < n_rows; ++k) {
    if (!wf_selected(rows, ld, k, surface, generation) || wf_group(rows, ld, k, rays_per_source, n_groups) != g) continue;
    if (wf_extend(rows, ld, k, p, r, s, e)) {
      pivot = opl[k] - rows[PRT_COL_INDEX * ld + k] * s;
      break;
    }
  }
  o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = r; o[4] = pivot; o[5] = nan;
  o[10] = (double)j;
}

// ---- pass 2: per row E, OPD and the pupil point ------------------------------------------------------------------
struct WfAxes { double a[3], e1[3], e2[3]; };

__global__ void __launch_bounds__(PRT_BLOCK)
k_frame_wavefront_pupil(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const double* __restrict__ opl,
                        double surface, double generation, double rays_per_source, int n_groups, int64_t per_wave,
                        WfAxes axes, int weight_column, double* __restrict__ group_out,
                        const int64_t* __restrict__ wave_offset, double* __restrict__ opd_out,
                        double* __restrict__ pupil_out, int* __restrict__ group_of, double* __restrict__ weight_of) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (PRT_BLOCK / 64) + (threadIdx.x >> 6);
  const int64_t first = wave * per_wave;
  const int64_t last = first + per_wave < n_rows ? first + per_wave : n_rows;
  if (first >= last) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  int64_t at = wave_offset[wave];
  int current = -1;
  long long missed = 0, hi = -0x7fffffffffffffffll - 1, lo = 0x7fffffffffffffffll;
  unsigned long long extent = 0ull;
  auto flush = [&](int group) {  // (integer max / min / add: exact in any order)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      missed += __shfl_xor(missed, off);
      const long long h = __shfl_xor(hi, off), l = __shfl_xor(lo, off);
      const unsigned long long x = __shfl_xor(extent, off);
      hi = h > hi ? h : hi; lo = l < lo ? l : lo; extent = x > extent ? x : extent;
    }
    if (lane == 0) {
      long long* o = (long long*)(group_out + (size_t)group * WF_GROUP);
      if (missed) atomicAdd((unsigned long long*)(o + 7), (unsigned long long)missed);
      atomicMax(o + 8, hi);
      atomicMin(o + 9, lo);
      atomicMax((unsigned long long*)(o + 11), extent);
    }
    missed = 0; hi = -0x7fffffffffffffffll - 1; lo = 0x7fffffffffffffffll; extent = 0ull;
  };
  for (int64_t base = first; base < last; base += 64) {
    const int64_t j = base + lane;
    int group = -1;
    if (j < last && wf_selected(rows, ld, j, surface, generation)) group = wf_group(rows, ld, j, rays_per_source, n_groups);
    const unsigned long long chosen = __ballot(group >= 0);
    double opd = nan, p1 = nan, p2 = nan;
    bool hit = false;
    if (group >= 0) {
      const double* g = group_out + (size_t)group * WF_GROUP;
      double s, e[3];
      if (wf_extend(rows, ld, j, g, g[3], s, e)) {
        opd = (opl[j] - rows[PRT_COL_INDEX * ld + j] * s) - g[4];
        const double v[3] = {e[0] - g[0], e[1] - g[1], e[2] - g[2]};
        p1 = v[0] * axes.e1[0] + v[1] * axes.e1[1] + v[2] * axes.e1[2];
        p2 = v[0] * axes.e2[0] + v[1] * axes.e2[1] + v[2] * axes.e2[2];
        hit = opd == opd && p1 == p1 && p2 == p2;
      }
      const int64_t pos = at + __popcll(chosen & ((1ull << lane) - 1ull));
      opd_out[pos] = hit ? opd : nan;
      pupil_out[2 * pos] = hit ? p1 : nan;
      pupil_out[2 * pos + 1] = hit ? p2 : nan;
      group_of[pos] = group;
      if (weight_of) weight_of[pos] = rows[(int64_t)weight_column * ld + j];
    }
    at += __popcll(chosen);
    unsigned long long pending = chosen;
    while (pending) {
      const int leader = __ffsll((long long)pending) - 1;
      const int g = __shfl(group, leader);
      if (g != current) {
        if (current >= 0) flush(current);
        current = g;
      }
      const bool take = group == g;
      if (take) {
        if (hit) {
          const long long k = ordered_key(opd);
          hi = k > hi ? k : hi; lo = k < lo ? k : lo;
          const unsigned long long x = (unsigned long long)__double_as_longlong(sqrt(p1 * p1 + p2 * p2));
          extent = x > extent ? x : extent;
        } else {
          ++missed;
        }
      }
      pending &= ~__ballot(take);
    }
  }
  if (current >= 0) flush(current);
}

// ---- the Zernike normal equations ----------------------------------------------------------------------------------
// Z_j(rho, theta) for j = 1..36 (Noll's order, RMS-normalised) into z[0..35]: radial polynomials by Kintner's
// three-term recurrence in n for each m, cos / sin (m theta) by the complex power of (x + iy) / rho.
__device__ __forceinline__ void wf_zernike(double x, double y, double (&z)[WF_MAX_TERMS]) {
  const double rho2 = x * x + y * y, rho = sqrt(rho2);
  const double c1 = rho > 0.0 ? x / rho : 1.0, s1 = rho > 0.0 ? y / rho : 0.0;
  double cm[8], sm[8], rm[8];  // cos(m theta), sin(m theta), rho^m
  cm[0] = 1.0; sm[0] = 0.0; rm[0] = 1.0;
#pragma unroll
  for (int m = 1; m < 8; ++m) {
    cm[m] = cm[m - 1] * c1 - sm[m - 1] * s1;
    sm[m] = sm[m - 1] * c1 + cm[m - 1] * s1;
    rm[m] = rm[m - 1] * rho;
  }
  double radial[8][8];  // radial[n][m], n - m even
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    radial[m][m] = rm[m];
    if (m + 2 < 8) radial[m + 2][m] = (m + 2) * rm[m + 2] - (m + 1) * rm[m];
#pragma unroll
    for (int n = m + 4; n < 8; n += 2) {
      const double k1 = 0.5 * (n + m) * (n - m) * (n - 2), k2 = 2.0 * n * (n - 1) * (n - 2);
      const double k3 = -(double)m * m * (n - 1) - (double)n * (n - 1) * (n - 2), k4 = -0.5 * n * (n + m - 2) * (n - m - 2);
      radial[n][m] = ((k2 * rho2 + k3) * radial[n - 2][m] + k4 * radial[n - 4][m]) / k1;
    }
  }
  constexpr NollTable noll = noll_table();  // (constants once the loop is unrolled: radial, cm, sm stay in registers)
#pragma unroll
  for (int j = 1; j <= WF_MAX_TERMS; ++j) {
    const int n = noll.n[j - 1], m = noll.m[j - 1], am = m < 0 ? -m : m;
    const double norm = am == 0 ? sqrt((double)(n + 1)) : sqrt(2.0 * (n + 1));
    z[j - 1] = norm * radial[n][am] * (m > 0 ? cm[am] : m < 0 ? sm[am] : 1.0);
  }
}

// entry e of a group's (terms (terms + 1) / 2 + terms + 3) sums: the upper triangle of Z^T W Z row by row, then
// Z^T W opd, then sum w, sum w opd, sum w opd^2
__device__ __forceinline__ void wf_entry(int e, int terms, int& i, int& j) {
  const int tri = terms * (terms + 1) / 2;
  if (e < tri) {
    i = 0;
    while (e >= terms - i) { e -= terms - i; ++i; }
    j = i + e;
  } else if (e < tri + terms) {
    i = e - tri; j = -1;                 // Z_i opd
  } else {
    i = -1 - (e - tri - terms); j = -1;  // -1: w, -2: w opd, -3: w opd^2
  }
}

static const int kWfEntriesPerThread = (wf_entries(WF_MAX_TERMS) + kWfZBlock - 1) / kWfZBlock;
__global__ void __launch_bounds__(kWfZBlock)
k_frame_zernike(int64_t capacity, const int64_t* __restrict__ total, const double* __restrict__ opd,
                double* __restrict__ pupil, const int* __restrict__ group_of, const double* __restrict__ weight_of,
                const double* __restrict__ group_out, double pupil_radius, int terms, int n_groups,
                double* __restrict__ slab) {
  extern __shared__ double zt[];          // [kWfZBlock][terms + 1]: the tile's basis values (+1: bank spread)
  __shared__ double wl[kWfZBlock], ol[kWfZBlock];
  __shared__ int red[kWfZBlock / 64];
  const int t = threadIdx.x, stride = terms + 1;
  const int entries = wf_entries(terms);
  const int64_t n = *total < capacity ? *total : capacity;
  const int64_t per = ((n + gridDim.x - 1) / gridDim.x + kWfZBlock - 1) / kWfZBlock * kWfZBlock;
  const int64_t first = (int64_t)blockIdx.x * per, last = first + per < n ? first + per : n;
  int ei[kWfEntriesPerThread], ej[kWfEntriesPerThread];
  double acc[kWfEntriesPerThread];
#pragma unroll
  for (int q = 0; q < kWfEntriesPerThread; ++q) {
    const int e = t + q * kWfZBlock;
    ei[q] = ej[q] = -100;
    if (e < entries) wf_entry(e, terms, ei[q], ej[q]);
    acc[q] = 0.0;
  }
  double* const mine = slab + (size_t)blockIdx.x * n_groups * entries;  // (only this workgroup writes here)
  int current = -1;
  for (int64_t base = first; base < last; base += kWfZBlock) {
    const int64_t r = base + t;
    int group = -1;
    double w = 0.0, v = 0.0;
    double z[WF_MAX_TERMS];
#pragma unroll
    for (int k = 0; k < WF_MAX_TERMS; ++k) z[k] = 0.0;
    if (r < last) {
      group = group_of[r];
      v = opd[r];
      if (v == v) {  // (a row that missed the sphere: NaN, weight 0, basis 0)
        const double* g = group_out + (size_t)group * WF_GROUP;
        const double extent = __longlong_as_double((long long)((const unsigned long long*)g)[11]);
        const double scale = pupil_radius > 0.0 ? pupil_radius : extent;
        const double x = scale > 0.0 ? pupil[2 * r] / scale : 0.0, y = scale > 0.0 ? pupil[2 * r + 1] / scale : 0.0;
        pupil[2 * r] = x;
        pupil[2 * r + 1] = y;
        wf_zernike(x, y, z);
        w = weight_of ? weight_of[r] : 1.0;
      } else {
        v = 0.0;
      }
    }
#pragma unroll
    for (int k = 0; k < WF_MAX_TERMS; ++k)
      if (k < terms) zt[t * stride + k] = z[k];
    ol[t] = v;
    bool pending = group >= 0;
    for (;;) {  // one turn per group present in the tile (block-uniform): almost always exactly one
      int m = pending ? group : 0x7fffffff;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(m, off); m = o < m ? o : m; }
      __syncthreads();  // (also: the tile and the previous turn's weights are in place / read)
      if ((t & 63) == 0) red[t >> 6] = m;
      __syncthreads();
      int g = red[0];
      for (int k = 1; k < kWfZBlock / 64; ++k) g = red[k] < g ? red[k] : g;
      if (g == 0x7fffffff) break;
      if (g != current) {
        if (current >= 0) {
#pragma unroll
          for (int q = 0; q < kWfEntriesPerThread; ++q)
            if (ei[q] != -100) { mine[(size_t)current * entries + t + q * kWfZBlock] += acc[q]; acc[q] = 0.0; }
        }
        current = g;
      }
      const bool take = pending && group == g;
      wl[t] = take ? w : 0.0;
      pending = pending && !take;
      __syncthreads();
      const int rows_here = (int)(last - base < kWfZBlock ? last - base : kWfZBlock);
#pragma unroll
      for (int q = 0; q < kWfEntriesPerThread; ++q) {
        const int i = ei[q], j = ej[q];
        if (i == -100) continue;
        double c = acc[q];
        for (int k = 0; k < rows_here; ++k) {
          const double a = i >= 0 ? zt[k * stride + i] : 1.0;
          const double b = j >= 0 ? zt[k * stride + j] : (i >= 0 || i == -2 ? ol[k] : i == -3 ? ol[k] * ol[k] : 1.0);
          c += wl[k] * a * b;
        }
        acc[q] = c;
      }
    }
  }
  if (current >= 0) {
#pragma unroll
    for (int q = 0; q < kWfEntriesPerThread; ++q)
      if (ei[q] != -100) mine[(size_t)current * entries + t + q * kWfZBlock] += acc[q];
  }
}

// one wave per (group, entry): the workgroups' partials in a fixed order; the last workgroup finishes the group
// records (keys and counts back to doubles, the pupil radius used)
__global__ void __launch_bounds__(PRT_BLOCK)
k_frame_zernike_fold(const double* __restrict__ slab, int blocks, int n_groups, int entries,
                     double* __restrict__ normal_out, double* __restrict__ group_out, double pupil_radius) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * (PRT_BLOCK / 64) + (threadIdx.x >> 6);
  if (item < (int64_t)n_groups * entries) {
    double v = 0.0;
    for (int k = lane; k < blocks; k += 64) v += slab[(size_t)k * n_groups * entries + item];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) normal_out[item] = v;
    return;
  }
  if (item != (int64_t)n_groups * entries) return;  // (one wave more than the entries: the group records)
  for (int g = lane; g < n_groups; g += 64) {
    double* o = group_out + (size_t)g * WF_GROUP;
    const long long missed = ((const long long*)o)[7], hi = ((const long long*)o)[8], lo = ((const long long*)o)[9];
    const double extent = __longlong_as_double((long long)((const unsigned long long*)o)[11]);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    o[7] = (double)missed;
    o[8] = hi == -0x7fffffffffffffffll - 1 ? nan : key_value(hi);
    o[9] = lo == 0x7fffffffffffffffll ? nan : key_value(lo);
    o[11] = o[6] > (double)missed ? extent : nan;
    o[5] = pupil_radius > 0.0 ? pupil_radius : o[11];
  }
}

// the group's mean OPD (sum w opd / sum w) off every row's OPD: piston removed
__global__ void __launch_bounds__(PRT_BLOCK)
k_frame_wavefront_piston(int64_t capacity, const int64_t* __restrict__ total, const int* __restrict__ group_of,
                         const double* __restrict__ normal, int entries, double* __restrict__ opd) {
  const int64_t r = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  const int64_t n = *total < capacity ? *total : capacity;
  if (r >= n) return;
  const double* s = normal + (size_t)group_of[r] * entries + entries - 3;
  opd[r] -= s[1] / s[0];
}

// ---- entry points ---------------------------------------------------------------------------------------------------
extern "C" int prt_frame_optical_path(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                                      int n_generations, double id0, int64_t n_ids, double* opl_out, void* stream) {
  const int64_t n_rows = join_rows(rows_per_generation, n_generations, ld);
  if (n_rows < 0) return (int)n_rows;
  if (n_rows && (!rows || !opl_out)) return fail(PRT_ERR_ARG, "bad buffers");
  int rc = join_ids(id0, n_ids);
  if (rc) return rc;
  if (n_rows == 0) return PRT_OK;
  rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* scratch = nullptr;
  const size_t acc_bytes = (size_t)n_ids * sizeof(double), stamp_bytes = (size_t)n_ids * sizeof(int);
  HIP_TRY(hipMallocAsync((void**)&scratch, acc_bytes + stamp_bytes + sizeof(int), st));
  double* acc = (double*)scratch;
  int* stamp = (int*)(scratch + acc_bytes);
  int* status = stamp + n_ids;
  HIP_TRY(hipMemsetAsync(stamp, 0, stamp_bytes + sizeof(int), st));
  int64_t start = 0;
  for (int g = 0; g < n_generations; ++g) {
    const int64_t count = rows_per_generation[g];
    if (count)
      hipLaunchKernelGGL(k_frame_optical_path, dim3((unsigned)((count + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0,
                         st, rows, ld, start, count, g, id0, n_ids, acc, stamp, opl_out, status);
    start += count;
  }
  int host_status = 0;
  HIP_TRY(hipMemcpyAsync(&host_status, status, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipFreeAsync(scratch, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return join_refusal(host_status, "optical path");
}

extern "C" int64_t prt_frame_wavefront_workspace_bytes(int64_t n_rows, int n_groups, int n_terms, int with_weights) {
  if (n_rows < 0 || n_groups < 1 || n_terms < 1 || n_terms > WF_MAX_TERMS) return PRT_ERR_ARG;
  return (int64_t)(2 * kWfMaxWaves + 1) * 8 + n_rows * (int64_t)(sizeof(int) + (with_weights ? sizeof(double) : 0)) + 8;
}

extern "C" int prt_frame_wavefront(int device, const double* rows, int64_t ld, int64_t n_rows, const double* opl,
                                   double surface, double generation, double rays_per_source, int n_groups,
                                   const double* reference, const double* radius, const double* axes,
                                   double pupil_radius, int n_terms, int weight_column, double* opd_out,
                                   double* pupil_out, double* group_out, double* normal_out, void* workspace,
                                   void* stream) {
  // (everything is checked before a device is touched)
  if (n_rows < 0 || ld < n_rows || n_groups < 1 || !group_out || !normal_out || !workspace || !axes ||
      (n_rows && (!rows || !opl || !opd_out || !pupil_out)))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (!(rays_per_source > 0) && n_groups != 1) return fail(PRT_ERR_ARG, "one group without rays_per_source");
  if (n_terms < 1 || n_terms > WF_MAX_TERMS) return fail(PRT_ERR_ARG, "zernike: 1 to 36 terms");
  if (weight_column < -1 || weight_column >= PRT_RECORD_COLS) return fail(PRT_ERR_ARG, "weight_column: 0..14 or -1");
  if (!(pupil_radius == pupil_radius) || pupil_radius < 0 || !(pupil_radius < PRT_INF))
    return fail(PRT_ERR_ARG, "pupil_radius: > 0, or 0 for the largest radial extent");
  WfAxes ax;
  for (int k = 0; k < 3; ++k) { ax.a[k] = axes[k]; ax.e1[k] = axes[3 + k]; ax.e2[k] = axes[6 + k]; }
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(axes[k])) return fail(PRT_ERR_ARG, "axes: finite");
  const int entries = wf_entries(n_terms);
  int rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  int64_t* wave_rows = (int64_t*)workspace;
  int64_t* wave_offset = wave_rows + kWfMaxWaves;
  int64_t* total = wave_offset + kWfMaxWaves;
  int* group_of = (int*)(total + 1);
  double* weight_of = nullptr;
  if (weight_column >= 0) weight_of = (double*)(((uintptr_t)(group_of + n_rows) + 7) & ~(uintptr_t)7);
  // row passes: waves of contiguous rows, as many as the slab of pass 1, WF_LOC doubles a (wave, group), allows
  const SortPlan plan = sort_plan(n_rows, n_groups, WF_LOC * sizeof(double), kWfSlabBytes);
  const int64_t per_wave = plan.per_wave, all_waves = plan.all_waves;
  const unsigned grid = plan.grid;
  const size_t loc_bytes = plan.count_bytes;
  double* loc = nullptr;
  HIP_TRY(hipMallocAsync((void**)&loc, loc_bytes, st));
  HIP_TRY(hipMemsetAsync(loc, 0, loc_bytes, st));
  hipLaunchKernelGGL(k_frame_wavefront_locate, dim3(grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, surface,
                     generation, rays_per_source, n_groups, per_wave, loc, wave_rows);
  hipLaunchKernelGGL(k_frame_wavefront_reference, dim3(n_groups + 1), dim3(kWfRefBlock), 0, st, rows, ld, n_rows, opl,
                     surface, generation, rays_per_source, n_groups, (int)all_waves, loc, reference, radius, group_out, wave_rows, wave_offset, total);
  HIP_TRY(hipFreeAsync(loc, st));
  hipLaunchKernelGGL(k_frame_wavefront_pupil, dim3(grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, opl, surface,
                     generation, rays_per_source, n_groups, per_wave, ax, weight_column, group_out, wave_offset,
                     opd_out, pupil_out, group_of, weight_of);
  int cus = 1;
  rc = hist_cus(device, &cus);
  if (rc) return rc;
  const int64_t tiles = (n_rows + kWfZBlock * 4 - 1) / (kWfZBlock * 4);
  int64_t zblocks = std::min<int64_t>(std::max<int64_t>(tiles, 1), std::min<int64_t>(kWfMaxZBlocks, 2 * (int64_t)cus));
  zblocks = std::max<int64_t>(1, std::min<int64_t>(zblocks, (int64_t)(kWfSlabBytes / ((size_t)n_groups * entries * 8))));
  const size_t zslab_bytes = (size_t)zblocks * n_groups * entries * sizeof(double);
  double* zslab = nullptr;
  HIP_TRY(hipMallocAsync((void**)&zslab, zslab_bytes, st));
  HIP_TRY(hipMemsetAsync(zslab, 0, zslab_bytes, st));
  const size_t lds = (size_t)kWfZBlock * (n_terms + 1) * sizeof(double);
  HIP_TRY(hipFuncSetAttribute((const void*)k_frame_zernike, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_frame_zernike, dim3((unsigned)zblocks), dim3(kWfZBlock), lds, st, n_rows, total, opd_out,
                     pupil_out, group_of, weight_of, group_out, pupil_radius, n_terms, n_groups, zslab);
  const int64_t items = (int64_t)n_groups * entries + 1;
  hipLaunchKernelGGL(k_frame_zernike_fold, dim3((unsigned)((items + PRT_BLOCK / 64 - 1) / (PRT_BLOCK / 64))),
                     dim3(PRT_BLOCK), 0, st, zslab, (int)zblocks, n_groups, entries, normal_out, group_out, pupil_radius);
  HIP_TRY(hipFreeAsync(zslab, st));
  if (n_rows)
    hipLaunchKernelGGL(k_frame_wavefront_piston, dim3((unsigned)((n_rows + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK),
                       0, st, n_rows, total, group_of, normal_out, entries, opd_out);
  HIP_TRY(hipGetLastError());
  return PRT_OK;
}
