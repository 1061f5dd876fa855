// prt_aberrations.hpp -- ray-aberration curves of the frame, on the device: each ray's row at
// a surface joined by ray id with the row where it was launched, its transverse and longitudinal aberration against
// its pupil coordinate, their sums, a Zernike fit of the fans and the zonal curve.  Definitions: include/prt.h.
//
//   k_aberration_table     the join, pass 1: generation 0 writes its row numbers into a dense per-id table
//   k_aberration_gather    the join, pass 2: every row reads its launch row from the table
//   k_aberration_extent    per wave of a contiguous run of rows: per group the largest |h|, the smallest |h|^2 and the
//                          rays left out (integer atomics on order-preserving images)
//   k_aberration_count     per wave: the rays kept per (group, zone) bucket and in all; the chief ray's row (the
//                          smallest row among the rays that attain the smallest |h|^2: an integer atomic)
//   (k_sort_positions, k_sort_offsets of prt_sort.hpp: the waves' totals scanned into each wave's place in the row-order
//   outputs, the waves' counts scanned per bucket; k_mtf_starts of prt_mtf.hpp: bucket and chunk starts)
//   k_aberration_scatter   the stable counting sort: every wave writes its rays, in row order, at its offsets
//   (k_mtf_centre<AbRaw> of prt_mtf.hpp: per (bucket, chunk of 4096 rays) sum w and sum w Q in a fixed tree)
//   k_aberration_record    per group: the chunks folded in order into the centroid (or the given point, or the chief
//                          ray's Q), rho, the counts
//   k_aberration_stage     per (bucket, chunk): each ray's (p, eps, s, la) into ray_out / row_out at its row-order
//                          place; the chunk's twelve sums in a fixed tree
//   k_aberration_normal    per (bucket, chunk): the Zernike basis by the wavefront's recurrence, a tile of rays in LDS,
//                          the normal-equation entries owned by threads and accumulated in ray order
//   k_aberration_fold      per output: the chunks of a group (of a bucket, for the zones) added in chunk order
// A bucket's chunks depend only on its count of rays used, never on n_rows, and the sort is stable: a frame with more
// rows that are not selected gives the same bits.  No floating-point atomics: every output is the same, bit for bit,
// on every run.
#pragma once

enum { AB_RECORD = 16, AB_RAY = 7, AB_ZONE = 6, AB_MAX_ZONES = 1024, AB_SUMS = 12 };
static const int kAbBlock = 256;                  // threads of a chunk workgroup = rays of its LDS tile
static_assert(kAbBlock == kMtfBlock, "k_mtf_centre<AbRaw> sums a chunk of this pass's rays");
static const size_t kAbCountBytes = 64u << 20;    // cap on the sort's (wave, bucket) counts
static const size_t kAbSlabBytes = 256u << 20;    // cap on the chunks' partial sums
static const int kAbEntriesPerThread = (WF_MAX_TERMS * (WF_MAX_TERMS + 1) / 2 + 4 * WF_MAX_TERMS + 1 + kAbBlock - 1) / kAbBlock;

__host__ __device__ constexpr int ab_entries(int terms) { return terms * (terms + 1) / 2 + 4 * terms + 1; }

// ---- the join: launch rows by ray id ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(PRT_BLOCK)
k_aberration_table(const double* __restrict__ rows, int64_t ld, int64_t n_launch_rows, double id0, int64_t n_ids,
                   unsigned long long* __restrict__ table, int* __restrict__ status) {
  const int64_t j = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (j >= n_launch_rows) return;
  const int64_t i = join_id(rows, ld, j, id0, n_ids);
  if (i < 0) {
    atomicOr(status, JOIN_BAD_ID);
    return;
  }
  // (the table starts as all ones: an entry taken before is an id seen twice in generation 0)
  if (atomicCAS(table + i, ~0ull, (unsigned long long)j) != ~0ull) atomicOr(status, JOIN_REPEATED_ID);
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_aberration_gather(const double* __restrict__ rows, int64_t ld, int64_t n_rows, double id0, int64_t n_ids,
                    const unsigned long long* __restrict__ table, int64_t* __restrict__ index_out,
                    int* __restrict__ status) {
  const int64_t j = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (j >= n_rows) return;
  const int64_t i = join_id(rows, ld, j, id0, n_ids);
  if (i < 0) {
    atomicOr(status, JOIN_BAD_ID);
    index_out[j] = -1;
    return;
  }
  index_out[j] = (int64_t)table[i];  // (all ones: -1, no launch row)
}

extern "C" int prt_frame_launch_index(int device, const double* rows, int64_t ld, int64_t n_rows, int64_t n_launch_rows,
                                      double id0, int64_t n_ids, int64_t* index_out, void* stream) {
  if (n_rows < 0 || ld < n_rows || n_launch_rows < 0 || n_launch_rows > n_rows || (n_rows && (!rows || !index_out)))
    return fail(PRT_ERR_ARG, "bad buffers");
  int rc = join_ids(id0, n_ids);
  if (rc) return rc;
  if (n_rows == 0) return PRT_OK;
  rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* scratch = nullptr;
  const size_t table_bytes = (size_t)n_ids * sizeof(unsigned long long);
  HIP_TRY(hipMallocAsync((void**)&scratch, table_bytes + sizeof(int), st));
  unsigned long long* table = (unsigned long long*)scratch;
  int* status = (int*)(scratch + table_bytes);
  HIP_TRY(hipMemsetAsync(table, 0xff, table_bytes, st));
  HIP_TRY(hipMemsetAsync(status, 0, sizeof(int), st));
  if (n_launch_rows)
    hipLaunchKernelGGL(k_aberration_table, dim3((unsigned)((n_launch_rows + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK),
                       0, st, rows, ld, n_launch_rows, id0, n_ids, table, status);
  hipLaunchKernelGGL(k_aberration_gather, dim3((unsigned)((n_rows + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                     rows, ld, n_rows, id0, n_ids, table, index_out, status);
  int host_status = 0;
  HIP_TRY(hipMemcpyAsync(&host_status, status, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipFreeAsync(scratch, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  if (host_status & JOIN_BAD_ID) return join_refusal(JOIN_BAD_ID, "launch index");
  if (host_status & JOIN_REPEATED_ID) return fail(PRT_ERR_ARG, "launch index: an id repeats within generation 0");
  return PRT_OK;
}

// ---- the aberration pass ------------------------------------------------------------------------------------------
struct AbSelect {
  double surface, generation, rays_per_source, pupil_radius, origin[3];
  int n_groups, n_zones, weight_column, pupil_mode;
  MtfAxes ax;
};
struct AbRaw { double q[3], u[3], h1, h2, w, la; int64_t row, pos; };  // (96 bytes)
struct AbOut { double p1, p2, e1, e2, s1, s2; };

__device__ __forceinline__ double ab_dot(const double (&v)[3], const double (&e)[3]) {
  return v[0] * e[0] + v[1] * e[1] + v[2] * e[2];
}

// the ray of row j if it is used: end point, direction, launch coordinate h, weight, longitudinal aberration
__device__ __forceinline__ bool ab_ray(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t j,
                                       const int64_t* __restrict__ launch, const AbSelect& a, AbRaw& r) {
  const int64_t l = launch[j];
  if (l < 0 || l >= n_rows) return false;
  r.q[0] = rows[PRT_COL_X1 * ld + j]; r.q[1] = rows[PRT_COL_Y1 * ld + j]; r.q[2] = rows[PRT_COL_Z1 * ld + j];
  r.u[0] = rows[PRT_COL_XTILT * ld + j]; r.u[1] = rows[PRT_COL_YTILT * ld + j]; r.u[2] = rows[PRT_COL_ZTILT * ld + j];
  r.w = a.weight_column >= 0 ? rows[(int64_t)a.weight_column * ld + j] : 1.0;
  bool ok = r.w >= 0.0 && r.w < PRT_INF;
  for (int k = 0; k < 3; ++k) ok = ok && fabs(r.q[k]) < PRT_INF && fabs(r.u[k]) < PRT_INF;
  const double ua = ab_dot(r.u, a.ax.a);
  const double s1 = ab_dot(r.u, a.ax.e1) / ua, s2 = ab_dot(r.u, a.ax.e2) / ua;
  ok = ok && ua != 0.0 && fabs(s1) < PRT_INF && fabs(s2) < PRT_INF;
  if (a.pupil_mode == 0) {  // position: h = ((L - O).e1, (L - O).e2)
    const double d[3] = {rows[PRT_COL_X0 * ld + l] - a.origin[0], rows[PRT_COL_Y0 * ld + l] - a.origin[1],
                         rows[PRT_COL_Z0 * ld + l] - a.origin[2]};
    r.h1 = ab_dot(d, a.ax.e1);
    r.h2 = ab_dot(d, a.ax.e2);
    for (int k = 0; k < 3; ++k) ok = ok && fabs(d[k]) < PRT_INF;
  } else {                  // direction: h = (v.e1, v.e2) / (v.a)
    const double v[3] = {rows[PRT_COL_XTILT * ld + l], rows[PRT_COL_YTILT * ld + l], rows[PRT_COL_ZTILT * ld + l]};
    const double va = ab_dot(v, a.ax.a);
    r.h1 = ab_dot(v, a.ax.e1) / va;
    r.h2 = ab_dot(v, a.ax.e2) / va;
    for (int k = 0; k < 3; ++k) ok = ok && fabs(v[k]) < PRT_INF;
    ok = ok && va != 0.0;
  }
  ok = ok && fabs(r.h1) < PRT_INF && fabs(r.h2) < PRT_INF;
  const double la = frame_value(rows, ld, j, FRAME_AXIS_INTERCEPT);  // (the one definition: prt_histogram.hpp)
  r.la = fabs(la) < PRT_INF ? la : __longlong_as_double(0x7ff8000000000000ll);
  r.row = j;
  return ok;
}

// rho: the given pupil radius, or the group's largest |h| (0: 1)
__device__ __forceinline__ double ab_rho(double pupil_radius, unsigned long long extent_bits) {
  if (pupil_radius > 0.0) return pupil_radius;
  const double extent = __longlong_as_double((long long)extent_bits);
  return extent > 0.0 ? extent : 1.0;
}

// zone = min(floor(|p| n_zones), n_zones - 1), p = h / rho (0 without zones)
__device__ __forceinline__ int ab_zone(double h1, double h2, double rho, int n_zones) {
  if (n_zones < 1) return 0;
  const double p1 = h1 / rho, p2 = h2 / rho;
  const double z = floor(sqrt(p1 * p1 + p2 * p2) * (double)n_zones);
  return z < (double)(n_zones - 1) ? (int)z : n_zones - 1;
}

// the group and the ray of row j of a wave's slice: group -1 when the row is not selected; used = the ray counts
__device__ __forceinline__ int ab_select(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t j,
                                         int64_t last, const int64_t* __restrict__ launch, const AbSelect& a, AbRaw& r,
                                         bool& used) {
  int group = -1;
  used = false;
  if (j < last && wf_selected(rows, ld, j, a.surface, a.generation))
    group = wf_group(rows, ld, j, a.rays_per_source, a.n_groups);
  if (group >= 0) used = ab_ray(rows, ld, n_rows, j, launch, a, r);
  return group;
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_aberration_extent(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const int64_t* __restrict__ launch,
                    AbSelect a, int64_t per_wave, unsigned long long* __restrict__ extent,
                    unsigned long long* __restrict__ hmin, unsigned long long* __restrict__ missed) {
  const SortRun run = sort_run(per_wave, n_rows);
  for (int64_t base = run.first; base < run.last; base += 64) {
    const int64_t j = base + run.lane;
    AbRaw r;
    bool used;
    const int group = ab_select(rows, ld, n_rows, j, run.last, launch, a, r, used);
    if (group >= 0 && !used) atomicAdd(missed + group, 1ull);  // (integer: the same total in any order)
    const int kept = used ? group : -1;
    // (a non-negative double's bits order as the double does)
    const double hh = used ? r.h1 * r.h1 + r.h2 * r.h2 : 0.0;
    const unsigned long long e_bits = used ? (unsigned long long)__double_as_longlong(sqrt(hh)) : 0ull;
    const unsigned long long m_bits = used ? (unsigned long long)__double_as_longlong(hh) : ~0ull;
    sort_turns(kept, [&](int g, unsigned long long) {
      const bool take = kept == g;
      unsigned long long e = take ? e_bits : 0ull, m = take ? m_bits : ~0ull;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long eo = __shfl_xor(e, off), mo = __shfl_xor(m, off);
        e = eo > e ? eo : e;
        m = mo < m ? mo : m;
      }
      if (run.lane == 0) {
        atomicMax(extent + g, e);
        atomicMin(hmin + g, m);
      }
    });
  }
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_aberration_count(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const int64_t* __restrict__ launch,
                   AbSelect a, int64_t per_wave, const unsigned long long* __restrict__ extent,
                   const unsigned long long* __restrict__ hmin, int n_buckets, int64_t* __restrict__ counts,
                   int64_t* __restrict__ wave_total, long long* __restrict__ chief) {
  const SortRun run = sort_run(per_wave, n_rows);
  const int nz = a.n_zones < 1 ? 1 : a.n_zones;
  int64_t* const mine = counts + run.wave * n_buckets;  // (only this wave writes here)
  int64_t total = 0;
  for (int64_t base = run.first; base < run.last; base += 64) {
    const int64_t j = base + run.lane;
    AbRaw r;
    bool used;
    const int group = ab_select(rows, ld, n_rows, j, run.last, launch, a, r, used);
    int bucket = -1;
    long long candidate = 0x7fffffffffffffffll;
    if (used) {
      bucket = group * nz + ab_zone(r.h1, r.h2, ab_rho(a.pupil_radius, extent[group]), a.n_zones);
      if ((unsigned long long)__double_as_longlong(r.h1 * r.h1 + r.h2 * r.h2) == hmin[group]) candidate = j;
    }
    total += __popcll(__ballot(bucket >= 0));
    const bool candidates = __ballot(candidate != 0x7fffffffffffffffll) != 0ull;  // (wave-uniform; rarely true)
    sort_turns(bucket, [&](int b, unsigned long long take) {
      long long c = bucket == b ? candidate : 0x7fffffffffffffffll;
      if (candidates) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const long long o = __shfl_xor(c, off);
          c = o < c ? o : c;
        }
      }
      if (run.lane == 0) {
        mine[b] += __popcll(take);
        if (candidates && c != 0x7fffffffffffffffll) atomicMin(chief + b / nz, c);  // (integer: the same in any order)
      }
    });
  }
  if (run.lane == 0) wave_total[run.wave] = total;
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_aberration_scatter(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const int64_t* __restrict__ launch,
                     AbSelect a, int64_t per_wave, const unsigned long long* __restrict__ extent, int n_buckets,
                     int64_t* __restrict__ offsets, const int64_t* __restrict__ wave_pos,
                     const int64_t* __restrict__ bucket_start, int64_t capacity, AbRaw* __restrict__ sorted) {
  const auto [lane, wave, first, last] = sort_run(per_wave, n_rows);
  if (first >= last) return;
  const int nz = a.n_zones < 1 ? 1 : a.n_zones;
  int64_t* const mine = offsets + wave * n_buckets;  // (only this wave reads and writes here)
  int64_t pos = wave_pos[wave];
  for (int64_t base = first; base < last; base += 64) {
    const int64_t j = base + lane;
    AbRaw r;
    bool used;
    const int group = ab_select(rows, ld, n_rows, j, last, launch, a, r, used);
    int bucket = -1;
    if (used) bucket = group * nz + ab_zone(r.h1, r.h2, ab_rho(a.pupil_radius, extent[group]), a.n_zones);
    const unsigned long long kept = __ballot(bucket >= 0);
    r.pos = pos + __popcll(kept & ((1ull << lane) - 1ull));
    pos += __popcll(kept);
    sort_place(lane, bucket, mine, bucket_start, [&](int64_t slot) {
      if (slot < capacity) sorted[slot] = r;  // (the host has checked the total against the capacity)
    });
  }
}

// per group: C_g (reference_mode 0: the chunks folded in order; 1: the given point; 2: the chief ray's Q), rho, counts
__global__ void __launch_bounds__(PRT_BLOCK)
k_aberration_record(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int n_groups, int nz,
                    int reference_mode, double pupil_radius, const int64_t* __restrict__ chunk_start,
                    const int64_t* __restrict__ bucket_start, const double* __restrict__ slab,
                    const double* __restrict__ reference, const unsigned long long* __restrict__ extent,
                    const unsigned long long* __restrict__ missed, const long long* __restrict__ chief,
                    double* __restrict__ record_out) {
  const int g = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (g >= n_groups) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int64_t b0 = (int64_t)g * nz, b1 = b0 + nz;
  const int64_t used = bucket_start[b1] - bucket_start[b0];
  const long long row = chief[g];
  const bool has_chief = row >= 0 && row < n_rows;
  double c[3] = {nan, nan, nan};
  if (reference_mode == 1) {
    for (int k = 0; k < 3; ++k) c[k] = reference[3 * g + k];
  } else if (reference_mode == 2) {
    if (has_chief) { c[0] = rows[PRT_COL_X1 * ld + row]; c[1] = rows[PRT_COL_Y1 * ld + row]; c[2] = rows[PRT_COL_Z1 * ld + row]; }
  } else {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t q = chunk_start[b0]; q < chunk_start[b1]; ++q)
      for (int k = 0; k < 4; ++k) s[k] += slab[q * 4 + k];
    for (int k = 0; k < 3; ++k) c[k] = s[1 + k] / s[0];  // (no rays, or sum w = 0: NaN)
  }
  double* o = record_out + (size_t)g * AB_RECORD;
  for (int k = 0; k < 3; ++k) o[k] = c[k];
  o[3] = ab_rho(pupil_radius, extent[g]);
  o[4] = (double)used;
  o[5] = (double)missed[g];
  o[7] = has_chief ? (double)row : -1.0;
}

// p = h / rho, eps = ((Q - C).e1, (Q - C).e2), s = (u.e1, u.e2) / (u.a)
__device__ __forceinline__ AbOut ab_out(const AbRaw& r, const double* __restrict__ record, const MtfAxes& ax) {
  const double d[3] = {r.q[0] - record[0], r.q[1] - record[1], r.q[2] - record[2]};
  const double ua = ab_dot(r.u, ax.a);
  return AbOut{r.h1 / record[3], r.h2 / record[3], ab_dot(d, ax.e1), ab_dot(d, ax.e2), ab_dot(r.u, ax.e1) / ua,
               ab_dot(r.u, ax.e2) / ua};
}

// per (bucket, chunk): the per-ray outputs at their row-order places; the chunk's sums [0] w  [1, 2] w eps  [3, 4] w s
// [5] w |eps|^2  [6] w eps.s  [7] w |s|^2  [8] rays with finite la  [9] w  [10] w la  [11] w la^2 (9..11 over those rays)
__global__ void __launch_bounds__(kAbBlock)
k_aberration_stage(int n_buckets, int nz, const int64_t* __restrict__ chunk_start,
                   const int64_t* __restrict__ bucket_total, const int64_t* __restrict__ bucket_start,
                   const AbRaw* __restrict__ sorted, const double* __restrict__ record, MtfAxes ax, int64_t capacity,
                   double* __restrict__ ray_out, int64_t* __restrict__ row_out, double* __restrict__ slab) {
  __shared__ double red[AB_SUMS][kAbBlock];
  const int t = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int b = mtf_owner(chunk_start, n_buckets, chunk);
  if (b < 0) return;
  int64_t lo, hi;
  mtf_chunk(chunk_start, bucket_total, bucket_start, b, chunk, lo, hi);
  const double* rec = record + (size_t)(b / nz) * AB_RECORD;
  double s[AB_SUMS];
#pragma unroll
  for (int k = 0; k < AB_SUMS; ++k) s[k] = 0.0;
  for (int64_t r = lo + t; r < hi; r += kAbBlock) {
    const AbRaw ray = sorted[r];
    const AbOut v = ab_out(ray, rec, ax);
    if (ray.pos >= 0 && ray.pos < capacity) {
      double* o = ray_out + ray.pos * AB_RAY;
      o[0] = v.p1; o[1] = v.p2; o[2] = v.e1; o[3] = v.e2; o[4] = v.s1; o[5] = v.s2; o[6] = ray.la;
      row_out[ray.pos] = ray.row;
    }
    const double w = ray.w;
    s[0] += w;
    s[1] += w * v.e1; s[2] += w * v.e2; s[3] += w * v.s1; s[4] += w * v.s2;
    s[5] += w * (v.e1 * v.e1 + v.e2 * v.e2);
    s[6] += w * (v.e1 * v.s1 + v.e2 * v.s2);
    s[7] += w * (v.s1 * v.s1 + v.s2 * v.s2);
    if (ray.la == ray.la) { s[8] += 1.0; s[9] += w; s[10] += w * ray.la; s[11] += w * (ray.la * ray.la); }
  }
#pragma unroll
  for (int k = 0; k < AB_SUMS; ++k) red[k][t] = s[k];
  sort_tree(red, t);
  if (t < AB_SUMS) slab[chunk * AB_SUMS + t] = red[t][0];
}

// entry e of a group's (terms (terms + 1) / 2 + 4 terms + 1) sums: the upper triangle of Z^T W Z row by row (i <= j),
// then Z^T W t for the targets t = eps1, eps2, s1, s2 (j = -1 - target), then sum w (i = -1)
__device__ __forceinline__ void ab_entry(int e, int terms, int& i, int& j) {
  const int tri = terms * (terms + 1) / 2;
  if (e < tri) {
    i = 0;
    while (e >= terms - i) { e -= terms - i; ++i; }
    j = i + e;
  } else if (e < tri + 4 * terms) {
    const int target = (e - tri) / terms;
    i = (e - tri) - target * terms;
    j = -1 - target;
  } else {
    i = -1; j = -1;
  }
}

// per (bucket, chunk): the chunk's normal-equation sums, each entry by its own thread over the rays in order
__global__ void __launch_bounds__(kAbBlock)
k_aberration_normal(int n_buckets, int nz, int terms, const int64_t* __restrict__ chunk_start,
                    const int64_t* __restrict__ bucket_total, const int64_t* __restrict__ bucket_start,
                    const AbRaw* __restrict__ sorted, const double* __restrict__ record, MtfAxes ax,
                    double* __restrict__ slab) {
  extern __shared__ double ab_lds[];  // [kAbBlock][terms + 1] basis values (+1: bank spread), 4 targets, the weights
  const int t = threadIdx.x, stride = terms + 1;
  double* const zt = ab_lds;
  double* const tl = zt + kAbBlock * stride;
  double* const wl = tl + 4 * kAbBlock;
  const int entries = ab_entries(terms);
  const int64_t chunk = blockIdx.x;
  const int b = mtf_owner(chunk_start, n_buckets, chunk);
  if (b < 0) return;
  int64_t lo, hi;
  mtf_chunk(chunk_start, bucket_total, bucket_start, b, chunk, lo, hi);
  const double* rec = record + (size_t)(b / nz) * AB_RECORD;
  int ei[kAbEntriesPerThread], ej[kAbEntriesPerThread];
  double acc[kAbEntriesPerThread];
#pragma unroll
  for (int q = 0; q < kAbEntriesPerThread; ++q) {
    const int e = t + q * kAbBlock;
    ei[q] = ej[q] = -100;
    if (e < entries) ab_entry(e, terms, ei[q], ej[q]);
    acc[q] = 0.0;
  }
  for (int64_t base = lo; base < hi; base += kAbBlock) {
    const int64_t r = base + t;
    double z[WF_MAX_TERMS];
#pragma unroll
    for (int k = 0; k < WF_MAX_TERMS; ++k) z[k] = 0.0;
    AbOut v = AbOut{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double w = 0.0;
    if (r < hi) {
      const AbRaw ray = sorted[r];
      v = ab_out(ray, rec, ax);
      w = ray.w;
      wf_zernike(v.p1, v.p2, z);  // (the wavefront's recurrence: prt_wavefront.hpp)
    }
    __syncthreads();  // (the previous tile is read)
#pragma unroll
    for (int k = 0; k < WF_MAX_TERMS; ++k)
      if (k < terms) zt[t * stride + k] = z[k];
    tl[t] = v.e1; tl[kAbBlock + t] = v.e2; tl[2 * kAbBlock + t] = v.s1; tl[3 * kAbBlock + t] = v.s2;
    wl[t] = w;
    __syncthreads();
    const int rays_here = (int)(hi - base < kAbBlock ? hi - base : kAbBlock);
#pragma unroll
    for (int q = 0; q < kAbEntriesPerThread; ++q) {
      const int i = ei[q], j = ej[q];
      if (i == -100) continue;
      double c = acc[q];
      for (int k = 0; k < rays_here; ++k) {
        const double za = i >= 0 ? zt[k * stride + i] : 1.0;
        const double zb = j >= 0 ? zt[k * stride + j] : (i >= 0 ? tl[(-1 - j) * kAbBlock + k] : 1.0);
        c += wl[k] * za * zb;
      }
      acc[q] = c;
    }
  }
#pragma unroll
  for (int q = 0; q < kAbEntriesPerThread; ++q)
    if (ei[q] != -100) slab[(size_t)chunk * entries + t + q * kAbBlock] = acc[q];
}

// per output: its chunks in chunk order.  Items: (group, normal entry); (group, sum 0..8) into the record's slots
// 8..15 and 6; (bucket, zone slot)
__global__ void __launch_bounds__(PRT_BLOCK)
k_aberration_fold(int n_groups, int nz, int n_zones, int entries, const int64_t* __restrict__ chunk_start,
                  const int64_t* __restrict__ bucket_total, const double* __restrict__ sums_slab,
                  const double* __restrict__ normal_slab, double* __restrict__ normal_out,
                  double* __restrict__ record_out, double* __restrict__ zone_out) {
  int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  const int64_t n_normal = (int64_t)n_groups * entries, n_record = (int64_t)n_groups * 9;
  const int64_t n_zone = n_zones > 0 ? (int64_t)n_groups * n_zones * AB_ZONE : 0;
  if (item < n_normal) {
    const int64_t g = item / entries, e = item - g * entries;
    double v = 0.0;
    for (int64_t q = chunk_start[g * nz]; q < chunk_start[(g + 1) * nz]; ++q) v += normal_slab[(size_t)q * entries + e];
    normal_out[item] = v;
    return;
  }
  item -= n_normal;
  if (item < n_record) {
    const int64_t g = item / 9;
    const int k = (int)(item - g * 9);
    double v = 0.0;
    for (int64_t q = chunk_start[g * nz]; q < chunk_start[(g + 1) * nz]; ++q) v += sums_slab[(size_t)q * AB_SUMS + k];
    record_out[(size_t)g * AB_RECORD + (k == 8 ? 6 : 8 + k)] = v;
    return;
  }
  item -= n_record;
  if (item >= n_zone) return;
  const int64_t b = item / AB_ZONE;  // (with zones a bucket is a (group, zone))
  const int slot = (int)(item - b * AB_ZONE);
  if (slot == 0) {
    zone_out[item] = (double)bucket_total[b];
    return;
  }
  const int k = slot == 1 ? 9 : slot == 2 ? 10 : slot == 3 ? 11 : slot == 4 ? 5 : 8;
  double v = 0.0;
  for (int64_t q = chunk_start[b]; q < chunk_start[b + 1]; ++q) v += sums_slab[(size_t)q * AB_SUMS + k];
  zone_out[item] = v;
}

// ---- entry points ---------------------------------------------------------------------------------------------------
static bool ab_sizes_ok(int64_t capacity, int n_groups, int n_terms, int n_zones) {
  if (capacity < 0 || n_groups < 1 || n_terms < 1 || n_terms > WF_MAX_TERMS || n_zones < 0 || n_zones > AB_MAX_ZONES)
    return false;
  return (size_t)n_groups * (size_t)(n_zones < 1 ? 1 : n_zones) * 8 <= kAbCountBytes;
}

extern "C" int64_t prt_frame_ray_aberrations_workspace_bytes(int64_t capacity, int n_groups, int n_terms, int n_zones) {
  if (!ab_sizes_ok(capacity, n_groups, n_terms, n_zones)) return PRT_ERR_ARG;
  const int64_t n_buckets = (int64_t)n_groups * (n_zones < 1 ? 1 : n_zones);
  // bucket totals and starts, chunk and slice starts (n_buckets + 1 each); per group the extent, the smallest |h|^2,
  // the chief ray's row and the misses; the sorted rays
  return (4 * (n_buckets + 1) + 4 * (int64_t)n_groups) * 8 + capacity * (int64_t)sizeof(AbRaw) + 64;
}

extern "C" int prt_frame_ray_aberrations(int device, const double* rows, int64_t ld, int64_t n_rows,
                                         const int64_t* launch_index, double surface, double generation,
                                         double rays_per_source, int n_groups, const double* reference,
                                         int reference_mode, const double* axes, int pupil_mode,
                                         const double* launch_origin, double pupil_radius, int n_terms, int n_zones,
                                         int weight_column, int64_t capacity, double* ray_out, int64_t* row_out,
                                         double* record_out, double* normal_out, double* zone_out, void* workspace,
                                         void* stream) {
  // (everything is checked before a device is touched)
  if (n_rows < 0 || ld < n_rows || capacity < 0 || n_groups < 1 || !record_out || !normal_out || !workspace || !axes ||
      (n_rows && (!rows || !launch_index)) || (capacity && (!ray_out || !row_out)))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (!(rays_per_source > 0) && n_groups != 1) return fail(PRT_ERR_ARG, "one group without rays_per_source");
  if (n_terms < 1 || n_terms > WF_MAX_TERMS) return fail(PRT_ERR_ARG, "zernike: 1 to 36 terms");
  if (n_zones < 0 || n_zones > AB_MAX_ZONES) return fail(PRT_ERR_ARG, "zones: 0 to 1024");
  if (n_zones > 0 && !zone_out) return fail(PRT_ERR_ARG, "bad buffers");
  if (!ab_sizes_ok(capacity, n_groups, n_terms, n_zones))
    return fail(PRT_ERR_ARG, "ray aberrations: n_groups * n_zones * 8 bytes above the 64 MiB count cap");
  if (weight_column < -1 || weight_column >= PRT_RECORD_COLS) return fail(PRT_ERR_ARG, "weight_column: 0..14 or -1");
  if (pupil_mode < 0 || pupil_mode > 1) return fail(PRT_ERR_ARG, "pupil_mode: 0 position, 1 direction");
  if (reference_mode < 0 || reference_mode > 2 || (reference_mode == 1) != (reference != nullptr))
    return fail(PRT_ERR_ARG, "reference_mode: 0 centroid, 1 the given points, 2 chief ray");
  if (!(pupil_radius == pupil_radius) || pupil_radius < 0 || !(pupil_radius < PRT_INF))
    return fail(PRT_ERR_ARG, "pupil_radius: > 0, or 0 for the largest extent");
  AbSelect a;
  if (const int rc = mtf_axes(axes, a.ax)) return rc;
  a.surface = surface; a.generation = generation; a.rays_per_source = rays_per_source; a.pupil_radius = pupil_radius;
  for (int k = 0; k < 3; ++k) {
    a.origin[k] = launch_origin ? launch_origin[k] : 0.0;
    if (!std::isfinite(a.origin[k])) return fail(PRT_ERR_ARG, "launch_origin: finite");
  }
  a.n_groups = n_groups; a.n_zones = n_zones; a.weight_column = weight_column; a.pupil_mode = pupil_mode;
  const int nz = n_zones < 1 ? 1 : n_zones;
  const int n_buckets = n_groups * nz;
  const int entries = ab_entries(n_terms);
  if (n_rows / 64 + 1 > 0x7fffffff) return fail(PRT_ERR_ARG, "ray aberrations: too many rows for one launch");
  int rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_ray_aberrations_workspace_bytes)
  int64_t* bucket_total = (int64_t*)workspace;
  int64_t* bucket_start = bucket_total + (n_buckets + 1);
  int64_t* chunk_start = bucket_start + (n_buckets + 1);
  int64_t* slice_start = chunk_start + (n_buckets + 1);
  unsigned long long* extent = (unsigned long long*)(slice_start + (n_buckets + 1));
  unsigned long long* hmin = extent + n_groups;
  long long* chief = (long long*)(hmin + n_groups);
  unsigned long long* missed = (unsigned long long*)(chief + n_groups);
  AbRaw* sorted = (AbRaw*)(((uintptr_t)(missed + n_groups) + 31) & ~(uintptr_t)31);
  // row passes: waves of contiguous rows, as many as the (wave, bucket) counts allow
  const SortPlan plan = sort_plan(n_rows, n_buckets, 8, kAbCountBytes);
  const int64_t per_wave = plan.per_wave, all_waves = plan.all_waves;
  const unsigned grid = plan.grid;
  const size_t count_bytes = plan.count_bytes, total_bytes = (size_t)all_waves * 8;
  char* scratch = nullptr;
  HIP_TRY(hipMallocAsync((void**)&scratch, count_bytes + total_bytes, st));
  int64_t* counts = (int64_t*)scratch;
  int64_t* wave_pos = (int64_t*)(scratch + count_bytes);
  HIP_TRY(hipMemsetAsync(scratch, 0, count_bytes + total_bytes, st));
  HIP_TRY(hipMemsetAsync(extent, 0, (size_t)n_groups * 8, st));
  HIP_TRY(hipMemsetAsync(hmin, 0xff, (size_t)n_groups * 8, st));
  HIP_TRY(hipMemsetAsync(chief, 0x7f, (size_t)n_groups * 8, st));  // (a row no frame reaches: no chief ray yet)
  HIP_TRY(hipMemsetAsync(missed, 0, (size_t)n_groups * 8, st));
  hipLaunchKernelGGL(k_aberration_extent, dim3(grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, launch_index, a,
                     per_wave, extent, hmin, missed);
  hipLaunchKernelGGL(k_aberration_count, dim3(grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, launch_index, a, per_wave,
                     extent, hmin, n_buckets, counts, wave_pos, chief);
  hipLaunchKernelGGL(k_sort_positions, dim3(1), dim3(kSortScanBlock), 0, st, (int)all_waves, wave_pos, wave_pos);
  hipLaunchKernelGGL(k_sort_offsets, dim3((unsigned)n_buckets), dim3(kSortScanBlock), 0, st, (int)all_waves, n_buckets,
                     counts, bucket_total);
  hipLaunchKernelGGL(k_mtf_starts, dim3(1), dim3(kSortScanBlock), 0, st, n_buckets, (int64_t)1, bucket_total,
                     bucket_start, chunk_start, slice_start);
  // the rays used and the chunks they make: read back, so that the slabs are sized by the chunks there are
  int64_t used = 0, chunks = 0;
  HIP_TRY(hipMemcpyAsync(&used, bucket_start + n_buckets, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&chunks, chunk_start + n_buckets, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (used > capacity || chunks > 0x7fffffff || (size_t)chunks * (size_t)(entries + AB_SUMS + 4) * 8 > kAbSlabBytes) {
    HIP_TRY(hipFreeAsync(scratch, st));
    if (used > capacity) return fail(PRT_ERR_ARG, "ray aberrations: more rays used than the outputs' capacity");
    return fail(PRT_ERR_ARG, "ray aberrations: the chunks' partial sums pass the 256 MiB slab cap");
  }
  char* slabs = nullptr;
  const size_t centre_bytes = (size_t)chunks * 4 * 8, sums_bytes = (size_t)chunks * AB_SUMS * 8;
  const size_t normal_bytes = (size_t)chunks * entries * 8;
  HIP_TRY(hipMallocAsync((void**)&slabs, centre_bytes + sums_bytes + normal_bytes + 8, st));
  double* centre_slab = (double*)slabs;
  double* sums_slab = (double*)(slabs + centre_bytes);
  double* normal_slab = (double*)(slabs + centre_bytes + sums_bytes);
  hipLaunchKernelGGL(k_aberration_scatter, dim3(grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, launch_index, a,
                     per_wave, extent, n_buckets, counts, wave_pos, bucket_start, capacity, sorted);
  if (chunks && reference_mode == 0)
    hipLaunchKernelGGL(k_mtf_centre<AbRaw>, dim3((unsigned)chunks), dim3(kMtfBlock), 0, st, n_buckets, chunk_start,
                       bucket_total, bucket_start, sorted, centre_slab);
  hipLaunchKernelGGL(k_aberration_record, dim3((unsigned)((n_groups + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0,
                     st, rows, ld, n_rows, n_groups, nz, reference_mode, pupil_radius, chunk_start, bucket_start,
                     centre_slab, reference, extent, missed, chief, record_out);
  if (chunks) {
    hipLaunchKernelGGL(k_aberration_stage, dim3((unsigned)chunks), dim3(kAbBlock), 0, st, n_buckets, nz, chunk_start,
                       bucket_total, bucket_start, sorted, record_out, a.ax, capacity, ray_out, row_out, sums_slab);
    const size_t lds = (size_t)kAbBlock * (n_terms + 1 + 5) * sizeof(double);
    HIP_TRY(hipFuncSetAttribute((const void*)k_aberration_normal, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_aberration_normal, dim3((unsigned)chunks), dim3(kAbBlock), lds, st, n_buckets, nz, n_terms,
                       chunk_start, bucket_total, bucket_start, sorted, record_out, a.ax, normal_slab);
  }
  const int64_t items = (int64_t)n_groups * (entries + 9) + (n_zones > 0 ? (int64_t)n_buckets * AB_ZONE : 0);
  hipLaunchKernelGGL(k_aberration_fold, dim3((unsigned)((items + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                     n_groups, nz, n_zones, entries, chunk_start, bucket_total, sums_slab, normal_slab, normal_out,
                     record_out, zone_out);
  HIP_TRY(hipFreeAsync(slabs, st));
  HIP_TRY(hipFreeAsync(scratch, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return PRT_OK;
}
