// prt_mtf.hpp -- the geometric MTF of the frame through focus, on the device.  It needs only
// each ray's end point and direction at the detector, so it runs on any frame that holds those rows.  Definitions:
// include/prt.h.
//
// The first part is the core that the geometric image passes stand on (this one, the MTF sensitivities, the enclosed
// energy): on the host the checks and the plan of the outputs (mtf_plan), the plan of the row passes (mtf_row_plan), the
// staging pass (mtf_stage_rows: the seven launches k_mtf_count to k_mtf_stage) and an entry's tail (mtf_finish); on the
// device the rule for keeping a ray, a chunk's and a slice's rays, a ray about its centre and the fp32 phasor.  The
// stable counting sort under the staging pass (the runs, the ballot loop, the scan, the tree) is prt_sort.hpp's.
//
//   k_mtf_count     per wave of a contiguous run of rows: the rays kept per group; rays left out counted per group
//                   (integer atomics)
//   (k_sort_offsets of prt_sort.hpp: the waves' counts scanned per group into each wave's offset inside the bucket)
//   k_mtf_starts    one workgroup: each bucket's start, and where each group's centre chunks and sum slices begin
//   k_mtf_scatter   the stable counting sort: every wave writes its rays (Q, u, w), in row order, at its offsets
//   k_mtf_centre    per (group, chunk of 4096 rays): sum w and sum w Q in a fixed tree
//   k_mtf_record    per group: the chunks folded in order into the centroid (or the given reference)
//   k_mtf_stage     per ray of a bucket: (p1, p2, s1, s2, w) about the group's centre
//   k_mtf_sum       per (ray slice of a group, output tile): sum w cos / sin (2 pi k.x(delta)) over the slice's rays,
//                   read through LDS, into a slab of partial sums of its own
//   k_mtf_fold      per (group, output): the slices added in slice order, normalised by sum w in the same order
// Every partition of the rays (chunks, slices) depends only on the group's count of rays kept, on the output count
// and on n_groups, never on n_rows: a frame holding only the detector's rows gives the same bits as the whole frame.
// No floating-point atomics: every output is the same, bit for bit, on every run.
#pragma once

#include <vector>

enum { MTF_MAX_FREQUENCIES = 4096, MTF_MAX_AZIMUTHS = 16, MTF_MAX_FOCUS = 256, MTF_RECORD = 6 };
static const int kMtfBlock = 256;                 // threads of a sum workgroup = rays of its LDS tile
static const int kMtfOut = 4;                     // outputs a thread owns (fp64 complex accumulators in registers)
static const int kMtfChunk = 4096;                // rays of a centroid / staging chunk
static const int kMtfMinSlice = 2048;             // rays a sum slice holds at least (while the group has them)
static const int kMtfMaxSlices = 256;             // slices of a group at most (the fold walks them in series)
static const size_t kMtfSlabBytes = 256u << 20;   // cap on the (slice, output) partial sums
static const size_t kMtfCountBytes = 64u << 20;   // cap on the sort's (wave, group) counts

struct MtfAxes { double a[3], e1[3], e2[3]; };
struct MtfRaw { double q[3], u[3], w; };
struct MtfRay { double p1, p2, s1, s2, w, pad; };  // (48 bytes: three 16-byte LDS reads)

// ---- the core, host side --------------------------------------------------------------------------------------------
static int mtf_axes(const double* axes, MtfAxes& ax) {
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(axes[k])) return fail(PRT_ERR_ARG, "axes: finite");
  for (int k = 0; k < 3; ++k) { ax.a[k] = axes[k]; ax.e1[k] = axes[3 + k]; ax.e2[k] = axes[6 + k]; }
  return PRT_OK;
}

// The outputs of a pass that sums phasors: `name` is the entry point's prefix of its messages; cell_bytes a (slice,
// output) of its slab of partial sums as the slices are capped; a sum workgroup has `block` threads, each owning `out`
// outputs.  max_slices decides the order of the slice fold, and with it the bits.
struct MtfPlan {
  MtfAxes ax;
  int n_k, lanes;
  int64_t n_out, max_slices, tiles;
  std::vector<double> host;  // (kc, ks) per (azimuth, frequency), then the planes
};
static int mtf_plan(const char* name, const double* frequencies, int n_frequencies, const double* azimuths_deg,
                    int n_azimuths, const double* focus, int n_focus, const double* axes, int n_groups,
                    size_t cell_bytes, int out, int block, MtfPlan& p) {
  const std::string at = std::string(name) + ": ";
  if (!frequencies || n_frequencies < 1 || n_frequencies > MTF_MAX_FREQUENCIES)
    return fail(PRT_ERR_ARG, at + "1 to 4096 frequencies");
  if (!azimuths_deg || n_azimuths < 1 || n_azimuths > MTF_MAX_AZIMUTHS) return fail(PRT_ERR_ARG, at + "1 to 16 azimuths");
  if (!focus || n_focus < 1 || n_focus > MTF_MAX_FOCUS) return fail(PRT_ERR_ARG, at + "1 to 256 focus shifts");
  for (int k = 0; k < n_frequencies; ++k)
    if (!(frequencies[k] >= 0 && frequencies[k] < PRT_INF)) return fail(PRT_ERR_ARG, at + "frequencies finite and >= 0");
  for (int k = 0; k < n_azimuths; ++k)
    if (!std::isfinite(azimuths_deg[k])) return fail(PRT_ERR_ARG, at + "azimuths finite");
  for (int k = 0; k < n_focus; ++k)
    if (!std::isfinite(focus[k])) return fail(PRT_ERR_ARG, at + "focus shifts finite");
  if (const int rc = mtf_axes(axes, p.ax)) return rc;
  p.n_k = n_azimuths * n_frequencies;
  const int64_t n_out = p.n_out = (int64_t)n_focus * p.n_k;
  const size_t cells = (size_t)n_groups * n_out * cell_bytes;
  if (cells > kMtfSlabBytes)
    return fail(PRT_ERR_ARG, at + "n_groups * n_focus * n_azimuths * n_frequencies * " +
                                 (cell_bytes > 16 ? std::to_string(cell_bytes / 16) + " * 16" : std::string("16")) +
                                 " bytes above the 256 MiB slab cap");
  // slices are launched for the most the rows could need; each group's share follows from its own count
  p.max_slices = std::max<int64_t>(1, std::min<int64_t>(kMtfMaxSlices, (int64_t)(kMtfSlabBytes / cells)));
  const int lanes = n_out <= out * block / 4 ? 4 : (n_out <= out * block / 2 ? 2 : 1);
  const int64_t tile = (int64_t)out * (block / lanes), tiles = (n_out + tile - 1) / tile;
  p.lanes = lanes, p.tiles = tiles;
  // k = nu (cos theta, sin theta), theta in degrees from e1 towards e2; then the planes
  p.host.resize(2 * (size_t)p.n_k + n_focus);
  for (int a = 0; a < n_azimuths; ++a) {
    const double theta = azimuths_deg[a] * (M_PI / 180.0), c = std::cos(theta), s = std::sin(theta);
    for (int f = 0; f < n_frequencies; ++f) {
      p.host[2 * ((size_t)a * n_frequencies + f)] = frequencies[f] * c;
      p.host[2 * ((size_t)a * n_frequencies + f) + 1] = frequencies[f] * s;
    }
  }
  for (int k = 0; k < n_focus; ++k) p.host[2 * (size_t)p.n_k + k] = focus[k];
  return PRT_OK;
}

// The staging pass (mtf_stage_rows) over n_rows rows in n_groups groups.  Row passes: waves of contiguous rows, as many
// as the (wave, group) counts allow; chunks and slices are launched for the most the rows could need.
struct MtfRowPlan {
  int64_t per_wave, all_waves, chunk_grid, slice_grid;
  unsigned grid;
  size_t count_bytes, centre_bytes;
};
static MtfRowPlan mtf_row_plan(int64_t n_rows, int n_groups, int64_t max_slices) {
  MtfRowPlan p;
  const SortPlan sort = sort_plan(n_rows, n_groups, 8, kMtfCountBytes);
  p.per_wave = sort.per_wave, p.grid = sort.grid, p.all_waves = sort.all_waves, p.count_bytes = sort.count_bytes;
  p.chunk_grid = (n_rows + kMtfChunk - 1) / kMtfChunk + n_groups;
  p.slice_grid = std::min<int64_t>((int64_t)n_groups * max_slices, n_rows / kMtfMinSlice + n_groups);
  p.centre_bytes = (size_t)p.chunk_grid * 4 * sizeof(double);
  return p;
}

// what the staging pass reads and writes: the head of an entry's workspace (mtf_staging_words), the entry's own centre,
// record, sorted and staged rays, and in its scratch the sort's counts and the centre chunks
struct MtfStaging {
  int64_t *bucket_total, *bucket_start, *chunk_start, *slice_start, *counts;
  unsigned long long* missed;
  double *centre, *record, *centre_slab;
  MtfRaw* sorted; MtfRay* stage;
};
// bucket totals and starts, chunk and slice starts (n_groups + 1 each), then the misses; returns what follows them
static void* mtf_staging_words(void* workspace, int n_groups, MtfStaging& s) {
  s.bucket_total = (int64_t*)workspace;
  s.bucket_start = s.bucket_total + (n_groups + 1);
  s.chunk_start = s.bucket_start + (n_groups + 1);
  s.slice_start = s.chunk_start + (n_groups + 1);
  s.missed = (unsigned long long*)(s.slice_start + (n_groups + 1));
  return s.missed + n_groups;
}

// the tail of an entry: the scratch freed, the stream drained
static int mtf_finish(hipStream_t st, void* scratch) {
  HIP_TRY(hipFreeAsync(scratch, st));
  HIP_TRY(hipStreamSynchronize(st));  // (the host table outlives its copy)
  HIP_TRY(hipGetLastError());
  return PRT_OK;
}

// ---- the core, device side ------------------------------------------------------------------------------------------
// the ray of row j if it is kept: end point, direction, weight; false if a value it needs is not finite, u.a == 0 or
// the weight is not finite and >= 0
__device__ __forceinline__ bool mtf_ray(const double* __restrict__ rows, int64_t ld, int64_t j, const MtfAxes& ax,
                                        int weight_column, MtfRaw& r) {
  r.q[0] = rows[PRT_COL_X1 * ld + j]; r.q[1] = rows[PRT_COL_Y1 * ld + j]; r.q[2] = rows[PRT_COL_Z1 * ld + j];
  r.u[0] = rows[PRT_COL_XTILT * ld + j]; r.u[1] = rows[PRT_COL_YTILT * ld + j]; r.u[2] = rows[PRT_COL_ZTILT * ld + j];
  r.w = weight_column >= 0 ? rows[(int64_t)weight_column * ld + j] : 1.0;
  bool ok = r.w >= 0.0 && r.w < PRT_INF;
  for (int k = 0; k < 3; ++k) ok = ok && fabs(r.q[k]) < PRT_INF && fabs(r.u[k]) < PRT_INF;
  const double ua = r.u[0] * ax.a[0] + r.u[1] * ax.a[1] + r.u[2] * ax.a[2];
  const double s1 = (r.u[0] * ax.e1[0] + r.u[1] * ax.e1[1] + r.u[2] * ax.e1[2]) / ua;
  const double s2 = (r.u[0] * ax.e2[0] + r.u[1] * ax.e2[1] + r.u[2] * ax.e2[2]) / ua;
  return ok && ua != 0.0 && fabs(s1) < PRT_INF && fabs(s2) < PRT_INF;
}

// the slices of a group of `count` rays: at least kMtfMinSlice rays each while the group has them, max_slices at most
__host__ __device__ __forceinline__ int64_t mtf_slices(int64_t count, int64_t max_slices) {
  const int64_t s = (count + kMtfMinSlice - 1) / kMtfMinSlice;
  return s < 1 ? 1 : (s > max_slices ? max_slices : s);
}

// the group whose run [start[g], start[g + 1]) holds item (start: n_groups + 1 non-decreasing entries); -1 past the end
__device__ __forceinline__ int mtf_owner(const int64_t* __restrict__ start, int n_groups, int64_t item) {
  if (item >= start[n_groups]) return -1;
  int lo = 0, hi = n_groups - 1;
  while (lo < hi) {  // the last g with start[g] <= item: the one non-empty run that holds it
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= item) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the rays [lo, hi) of a group's chunk
__device__ __forceinline__ void mtf_chunk(const int64_t* __restrict__ chunk_start,
                                          const int64_t* __restrict__ bucket_total,
                                          const int64_t* __restrict__ bucket_start, int g, int64_t chunk, int64_t& lo,
                                          int64_t& hi) {
  lo = bucket_start[g] + (chunk - chunk_start[g]) * kMtfChunk;
  const int64_t end = bucket_start[g] + bucket_total[g];
  hi = lo + kMtfChunk < end ? lo + kMtfChunk : end;
}

// the rays [lo, hi) of slice s of group g, whose `count` rays begin at first[g]
__device__ __forceinline__ void mtf_slice(const int64_t* __restrict__ slice_start, const int64_t* __restrict__ first,
                                          int64_t count, int g, int64_t s, int64_t& lo, int64_t& hi) {
  const int64_t slices = slice_start[g + 1] - slice_start[g], per = (count + slices - 1) / slices;
  lo = first[g] + (s - slice_start[g]) * per;
  hi = lo + per < first[g] + count ? lo + per : first[g] + count;
}

// a ray about the centre c: d = Q - C, s = (u.e1, u.e2) / u.a, p = (d.e1, d.e2) - s (d.a); also s, da = d.a and ua = u.a
__device__ __forceinline__ MtfRay mtf_stage_ray(const MtfRaw& ray, const double c[3], const MtfAxes& ax, double& s1,
                                                double& s2, double& da, double& ua) {
  const double d[3] = {ray.q[0] - c[0], ray.q[1] - c[1], ray.q[2] - c[2]};
  ua = ray.u[0] * ax.a[0] + ray.u[1] * ax.a[1] + ray.u[2] * ax.a[2];
  s1 = (ray.u[0] * ax.e1[0] + ray.u[1] * ax.e1[1] + ray.u[2] * ax.e1[2]) / ua;
  s2 = (ray.u[0] * ax.e2[0] + ray.u[1] * ax.e2[1] + ray.u[2] * ax.e2[2]) / ua;
  da = d[0] * ax.a[0] + d[1] * ax.a[1] + d[2] * ax.a[2];
  const double d1 = d[0] * ax.e1[0] + d[1] * ax.e1[1] + d[2] * ax.e1[2];
  const double d2 = d[0] * ax.e2[0] + d[1] * ax.e2[1] + d[2] * ax.e2[2];
  return MtfRay{d1 - s1 * da, d2 - s2 * da, s1, s2, ray.w, 0.0};
}

// k.x(delta) = kc p1 + ks p2 + delta (kc s1 + ks s2), in cycles; the cosine and sine of its fraction from
// v_cos_f32 / v_sin_f32 (they take turns).  Returns the angle that the conversion to fp32 drops: the caller corrects
// (c, sn) for it to first order, each sum kernel in its own way
__device__ __forceinline__ double mtf_phasor(double kc, double ks, double kcd, double ksd, const MtfRay& ray, double& c,
                                             double& sn) {
  const double phase = fma(kc, ray.p1, fma(ks, ray.p2, fma(kcd, ray.s1, ksd * ray.s2)));
  const double turn = __builtin_amdgcn_fract(phase);
  const float tf = (float)turn;
  c = (double)__builtin_amdgcn_cosf(tf);
  sn = (double)__builtin_amdgcn_sinf(tf);
  return 6.283185307179586 * (turn - (double)tf);
}

// ---- the staging pass -----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PRT_BLOCK)
k_mtf_count(const double* __restrict__ rows, int64_t ld, int64_t n_rows, double surface, double generation,
            double rays_per_source, int n_groups, MtfAxes ax, int weight_column, int64_t per_wave,
            int64_t* __restrict__ counts, unsigned long long* __restrict__ missed) {
  const auto [lane, wave, first, last] = sort_run(per_wave, n_rows);
  int64_t* const mine = counts + wave * n_groups;  // (only this wave writes here)
  for (int64_t base = first; base < last; base += 64) {
    const int64_t j = base + lane;
    int group = -1;
    if (j < last && wf_selected(rows, ld, j, surface, generation)) group = wf_group(rows, ld, j, rays_per_source, n_groups);
    int kept = -1;
    if (group >= 0) {
      MtfRaw r;
      if (mtf_ray(rows, ld, j, ax, weight_column, r)) kept = group;
      else atomicAdd(missed + group, 1ull);  // (integer: the same total in any order)
    }
    sort_tally(lane, kept, mine);
  }
}

// one workgroup: bucket starts, and the first centre chunk and first sum slice of each group (n_groups + 1 entries)
__global__ void __launch_bounds__(kSortScanBlock)
k_mtf_starts(int n_groups, int64_t max_slices, const int64_t* __restrict__ bucket_total,
             int64_t* __restrict__ bucket_start, int64_t* __restrict__ chunk_start, int64_t* __restrict__ slice_start) {
  __shared__ int64_t scan[kSortScanBlock];
  const int64_t rays = sort_scan(
      n_groups, [&](int64_t g) { return bucket_total[g]; }, [&](int64_t g, int64_t v) { bucket_start[g] = v; }, scan);
  const int64_t chunks = sort_scan(
      n_groups, [&](int64_t g) { return (bucket_total[g] + kMtfChunk - 1) / kMtfChunk; },
      [&](int64_t g, int64_t v) { chunk_start[g] = v; }, scan);
  const int64_t slices = sort_scan(
      n_groups, [&](int64_t g) { return mtf_slices(bucket_total[g], max_slices); },
      [&](int64_t g, int64_t v) { slice_start[g] = v; }, scan);
  if (threadIdx.x == 0) {
    bucket_start[n_groups] = rays;
    chunk_start[n_groups] = chunks;
    slice_start[n_groups] = slices;
  }
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_mtf_scatter(const double* __restrict__ rows, int64_t ld, int64_t n_rows, double surface, double generation,
              double rays_per_source, int n_groups, MtfAxes ax, int weight_column, int64_t per_wave,
              int64_t* __restrict__ offsets, const int64_t* __restrict__ bucket_start, MtfRaw* __restrict__ sorted) {
  const auto [lane, wave, first, last] = sort_run(per_wave, n_rows);
  int64_t* const mine = offsets + wave * n_groups;  // (only this wave reads and writes here)
  for (int64_t base = first; base < last; base += 64) {
    const int64_t j = base + lane;
    int group = -1, kept = -1;
    MtfRaw r;
    if (j < last && wf_selected(rows, ld, j, surface, generation)) group = wf_group(rows, ld, j, rays_per_source, n_groups);
    if (group >= 0 && mtf_ray(rows, ld, j, ax, weight_column, r)) kept = group;
    sort_place(lane, kept, mine, bucket_start, [&](int64_t slot) { sorted[slot] = r; });
  }
}

// per (group, chunk): [0] sum w  [1..3] sum w Q -- each thread over its strided rays in order, then a fixed tree.
// Ray: the sorted rays of the pass, with a weight .w and an end point .q (MtfRaw; the aberrations' AbRaw)
template <class Ray>
__global__ void __launch_bounds__(kMtfBlock)
k_mtf_centre(int n_groups, const int64_t* __restrict__ chunk_start, const int64_t* __restrict__ bucket_total,
             const int64_t* __restrict__ bucket_start, const Ray* __restrict__ sorted, double* __restrict__ slab) {
  __shared__ double red[4][kMtfBlock];
  const int t = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int g = mtf_owner(chunk_start, n_groups, chunk);
  if (g < 0) return;
  int64_t lo, hi;
  mtf_chunk(chunk_start, bucket_total, bucket_start, g, chunk, lo, hi);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = lo + t; r < hi; r += kMtfBlock) {
    const double w = sorted[r].w;
    s[0] += w;
    for (int k = 0; k < 3; ++k) s[1 + k] = fma(w, sorted[r].q[k], s[1 + k]);
  }
  for (int k = 0; k < 4; ++k) red[k][t] = s[k];
  sort_tree(red, t);
  if (t < 4) slab[chunk * 4 + t] = red[t][0];
}

// per group: the centre (the chunks folded in order, or the given reference) into centre and record_out[0..2]
__global__ void __launch_bounds__(PRT_BLOCK)
k_mtf_record(int n_groups, const int64_t* __restrict__ chunk_start, const double* __restrict__ slab,
             const double* __restrict__ reference, double* __restrict__ centre, double* __restrict__ record_out) {
  const int g = blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (g >= n_groups) return;
  double c[3];
  if (reference) {
    for (int k = 0; k < 3; ++k) c[k] = reference[3 * g + k];
  } else {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t q = chunk_start[g]; q < chunk_start[g + 1]; ++q)
      for (int k = 0; k < 4; ++k) s[k] += slab[q * 4 + k];
    for (int k = 0; k < 3; ++k) c[k] = s[1 + k] / s[0];  // (no rays, or sum w = 0: NaN)
  }
  for (int k = 0; k < 3; ++k) {
    centre[3 * g + k] = c[k];
    record_out[(size_t)g * MTF_RECORD + k] = c[k];
  }
}

// per (group, chunk), each ray: mtf_stage_ray about the group's centre
__global__ void __launch_bounds__(kMtfBlock)
k_mtf_stage(int n_groups, const int64_t* __restrict__ chunk_start, const int64_t* __restrict__ bucket_total,
            const int64_t* __restrict__ bucket_start, const MtfRaw* __restrict__ sorted, const double* __restrict__ centre,
            MtfAxes ax, MtfRay* __restrict__ stage) {
  const int64_t chunk = blockIdx.x;
  const int g = mtf_owner(chunk_start, n_groups, chunk);
  if (g < 0) return;
  int64_t lo, hi;
  mtf_chunk(chunk_start, bucket_total, bucket_start, g, chunk, lo, hi);
  const double c[3] = {centre[3 * g], centre[3 * g + 1], centre[3 * g + 2]};
  for (int64_t r = lo + threadIdx.x; r < hi; r += kMtfBlock) {
    double s1, s2, da, ua;
    stage[r] = mtf_stage_ray(sorted[r], c, ax, s1, s2, da, ua);
  }
}

// The staging pass: per group, in row order, each kept ray's (p1, p2, s1, s2, w) about the group's centre into s.stage,
// the centre into s.centre and s.record[0..2], the rays left out into s.missed.  `cleared` bytes from s.missed on are
// zeroed (an entry's own counters may follow the misses).
static int mtf_stage_rows(hipStream_t st, const MtfRowPlan& p, const MtfStaging& s, size_t cleared, const double* rows,
                          int64_t ld, int64_t n_rows, double surface, double generation, double rays_per_source,
                          int n_groups, const double* reference, const MtfAxes& ax, int weight_column,
                          int64_t max_slices) {
  HIP_TRY(hipMemsetAsync(s.counts, 0, p.count_bytes, st));
  HIP_TRY(hipMemsetAsync(s.missed, 0, cleared, st));
  hipLaunchKernelGGL(k_mtf_count, dim3(p.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, surface, generation,
                     rays_per_source, n_groups, ax, weight_column, p.per_wave, s.counts, s.missed);
  hipLaunchKernelGGL(k_sort_offsets, dim3((unsigned)n_groups), dim3(kSortScanBlock), 0, st, (int)p.all_waves, n_groups,
                     s.counts, s.bucket_total);
  hipLaunchKernelGGL(k_mtf_starts, dim3(1), dim3(kSortScanBlock), 0, st, n_groups, max_slices, s.bucket_total,
                     s.bucket_start, s.chunk_start, s.slice_start);
  hipLaunchKernelGGL(k_mtf_scatter, dim3(p.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, surface, generation,
                     rays_per_source, n_groups, ax, weight_column, p.per_wave, s.counts, s.bucket_start, s.sorted);
  if (!reference)
    hipLaunchKernelGGL(k_mtf_centre<MtfRaw>, dim3((unsigned)p.chunk_grid), dim3(kMtfBlock), 0, st, n_groups, s.chunk_start,
                       s.bucket_total, s.bucket_start, s.sorted, s.centre_slab);
  hipLaunchKernelGGL(k_mtf_record, dim3((unsigned)((n_groups + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st,
                     n_groups, s.chunk_start, s.centre_slab, reference, s.centre, s.record);
  hipLaunchKernelGGL(k_mtf_stage, dim3((unsigned)p.chunk_grid), dim3(kMtfBlock), 0, st, n_groups, s.chunk_start,
                     s.bucket_total, s.bucket_start, s.sorted, s.centre, ax, s.stage);
  return PRT_OK;
}

// ---- the MTF's own kernels ------------------------------------------------------------------------------------------
// A workgroup is `lanes` lanes of kMtfBlock / lanes threads; each thread owns kMtfOut outputs of the tile.  With
// lanes > 1 the lanes (whole waves) split the LDS tile's rays between them -- one ray per wave per step, an LDS
// broadcast -- and their sums are added in lane order.  table: (kc, ks) per (azimuth, frequency); focus: delta per plane.
__global__ void __launch_bounds__(kMtfBlock)
k_mtf_sum(int n_groups, const int64_t* __restrict__ slice_start, const int64_t* __restrict__ bucket_total,
          const int64_t* __restrict__ bucket_start, const MtfRay* __restrict__ stage, const double* __restrict__ table,
          const double* __restrict__ focus, int n_k, int64_t n_out, int lanes, double* __restrict__ slab,
          double* __restrict__ weight_slab) {
  __shared__ double lds[kMtfBlock * 2 * kMtfOut];  // the ray tile (6 doubles a ray), then the lanes' sums
  MtfRay* const tile = (MtfRay*)lds;
  const int t = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int g = mtf_owner(slice_start, n_groups, s);
  if (g < 0) return;
  const int threads = kMtfBlock / lanes, lane = t / threads, me = t - lane * threads;
  double kc[kMtfOut], ks[kMtfOut], kcd[kMtfOut], ksd[kMtfOut], re[kMtfOut], im[kMtfOut];
#pragma unroll
  for (int q = 0; q < kMtfOut; ++q) {
    const int64_t o = (int64_t)blockIdx.y * threads * kMtfOut + q * threads + me;
    const int64_t oo = o < n_out ? o : 0;
    const int64_t f = oo / n_k, k = oo - f * n_k;
    kc[q] = table[2 * k];
    ks[q] = table[2 * k + 1];
    kcd[q] = kc[q] * focus[f];
    ksd[q] = ks[q] * focus[f];
    re[q] = im[q] = 0.0;
  }
  double sw = 0.0;
  int64_t lo, hi;
  mtf_slice(slice_start, bucket_start, bucket_total[g], g, s, lo, hi);
  for (int64_t base = lo; base < hi; base += kMtfBlock) {
    __syncthreads();  // (the previous tile is read)
    if (base + t < hi) tile[t] = stage[base + t];
    __syncthreads();
    const int count = hi - base < kMtfBlock ? (int)(hi - base) : kMtfBlock;
    for (int r = lane; r < count; r += lanes) {
      const MtfRay ray = tile[r];
      sw += ray.w;
#pragma unroll
      for (int q = 0; q < kMtfOut; ++q) {
        // the phasor corrected to first order for what the conversion to fp32 drops (mtf_phasor)
        double c, sn;
        const double wd = ray.w * mtf_phasor(kc[q], ks[q], kcd[q], ksd[q], ray, c, sn);
        re[q] = fma(-wd, sn, fma(ray.w, c, re[q]));
        im[q] = fma(wd, c, fma(ray.w, sn, im[q]));
      }
    }
  }
  if (lanes > 1) {  // the lanes' sums added in lane order
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMtfOut; ++q) {
      lds[(2 * q) * kMtfBlock + t] = re[q];
      lds[(2 * q + 1) * kMtfBlock + t] = im[q];
    }
    __syncthreads();
    if (lane == 0)
      for (int l = 1; l < lanes; ++l)
#pragma unroll
        for (int q = 0; q < kMtfOut; ++q) {
          re[q] += lds[(2 * q) * kMtfBlock + l * threads + me];
          im[q] += lds[(2 * q + 1) * kMtfBlock + l * threads + me];
        }
    __syncthreads();
    if (me == 0) lds[t] = sw;  // (lane l's sum of w at lds[l * threads])
    __syncthreads();
    if (lane == 0)
      for (int l = 1; l < lanes; ++l) sw += lds[l * threads];
  }
  if (lane != 0) return;
#pragma unroll
  for (int q = 0; q < kMtfOut; ++q) {
    const int64_t o = (int64_t)blockIdx.y * threads * kMtfOut + q * threads + me;
    if (o < n_out) {
      double* p = slab + ((size_t)s * n_out + o) * 2;
      p[0] = re[q];
      p[1] = im[q];
    }
  }
  if (blockIdx.y == 0 && me == 0) weight_slab[s] = sw;
}

// per (group, output): the slices in slice order; OTF = (sum w cos, -sum w sin) / sum w; the record's sums and counts
__global__ void __launch_bounds__(PRT_BLOCK)
k_mtf_fold(int n_groups, int64_t n_out, const int64_t* __restrict__ slice_start, const double* __restrict__ slab,
           const double* __restrict__ weight_slab, const int64_t* __restrict__ bucket_total,
           const unsigned long long* __restrict__ missed, double* __restrict__ otf_out, double* __restrict__ record_out) {
  const int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item >= (int64_t)n_groups * n_out) return;
  const int g = (int)(item / n_out);
  const int64_t o = item - (int64_t)g * n_out;
  double re = 0.0, im = 0.0, sw = 0.0;
  for (int64_t s = slice_start[g]; s < slice_start[g + 1]; ++s) {
    const double* p = slab + ((size_t)s * n_out + o) * 2;
    re += p[0];
    im += p[1];
    sw += weight_slab[s];
  }
  otf_out[item * 2] = re / sw;  // (a group without rays, or with sum w = 0: 0 / 0, NaN)
  otf_out[item * 2 + 1] = -im / sw;
  if (o == 0) {
    double* r = record_out + (size_t)g * MTF_RECORD;
    r[3] = sw;
    r[4] = (double)bucket_total[g];
    r[5] = (double)missed[g];
  }
}

// ---- entry points ---------------------------------------------------------------------------------------------------
extern "C" int64_t prt_frame_mtf_workspace_bytes(int64_t n_rows, int n_groups, int n_frequencies, int n_azimuths,
                                                 int n_focus) {
  if (n_rows < 0 || n_groups < 1 || n_frequencies < 1 || n_frequencies > MTF_MAX_FREQUENCIES || n_azimuths < 1 ||
      n_azimuths > MTF_MAX_AZIMUTHS || n_focus < 1 || n_focus > MTF_MAX_FOCUS)
    return PRT_ERR_ARG;
  // bucket totals and starts, chunk and slice starts (n_groups + 1 each), misses, centres, the (kc, ks) table and the
  // planes, the sorted and the staged rays
  return (4 * ((int64_t)n_groups + 1) + 4 * (int64_t)n_groups) * 8 +
         (int64_t)(2 * n_frequencies * n_azimuths + n_focus) * 8 + n_rows * (int64_t)(sizeof(MtfRaw) + sizeof(MtfRay)) +
         64;
}

extern "C" int prt_frame_mtf(int device, const double* rows, int64_t ld, int64_t n_rows, double surface,
                             double generation, double rays_per_source, int n_groups, const double* reference,
                             const double* axes, int weight_column, const double* frequencies, int n_frequencies,
                             const double* azimuths_deg, int n_azimuths, const double* focus, int n_focus,
                             double* otf_out, double* record_out, void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  if (n_rows < 0 || ld < n_rows || n_groups < 1 || !otf_out || !record_out || !workspace || !axes || (n_rows && !rows))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (!(rays_per_source > 0) && n_groups != 1) return fail(PRT_ERR_ARG, "one group without rays_per_source");
  if (weight_column < -1 || weight_column >= PRT_RECORD_COLS) return fail(PRT_ERR_ARG, "weight_column: 0..14 or -1");
  MtfPlan plan;
  int rc = mtf_plan("mtf", frequencies, n_frequencies, azimuths_deg, n_azimuths, focus, n_focus, axes, n_groups, 16,
                    kMtfOut, kMtfBlock, plan);
  if (rc) return rc;
  const int64_t n_out = plan.n_out;
  const MtfRowPlan row = mtf_row_plan(n_rows, n_groups, plan.max_slices);
  if (row.chunk_grid > 0x7fffffff || row.slice_grid > 0x7fffffff || plan.tiles > 65535)
    return fail(PRT_ERR_ARG, "mtf: too many rows or outputs for one launch");
  rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_mtf_workspace_bytes)
  MtfStaging s;
  s.centre = (double*)mtf_staging_words(workspace, n_groups, s);
  s.record = record_out;
  double* table = s.centre + 3 * (size_t)n_groups;
  double* planes = table + 2 * (size_t)plan.n_k;
  s.sorted = (MtfRaw*)(((uintptr_t)(planes + n_focus) + 31) & ~(uintptr_t)31);
  s.stage = (MtfRay*)(s.sorted + n_rows);
  const size_t weight_bytes = (size_t)row.slice_grid * sizeof(double);
  const size_t slab_bytes = (size_t)row.slice_grid * n_out * 2 * sizeof(double);
  char* scratch = nullptr;
  HIP_TRY(hipMallocAsync((void**)&scratch, row.count_bytes + row.centre_bytes + weight_bytes + slab_bytes, st));
  s.counts = (int64_t*)scratch;
  s.centre_slab = (double*)(scratch + row.count_bytes);
  double* weight_slab = (double*)(scratch + row.count_bytes + row.centre_bytes);
  double* slab = (double*)(scratch + row.count_bytes + row.centre_bytes + weight_bytes);
  HIP_TRY(hipMemcpyAsync(table, plan.host.data(), plan.host.size() * sizeof(double), hipMemcpyHostToDevice, st));
  rc = mtf_stage_rows(st, row, s, (size_t)n_groups * 8, rows, ld, n_rows, surface, generation, rays_per_source, n_groups,
                      reference, plan.ax, weight_column, plan.max_slices);
  if (rc) return rc;
  hipLaunchKernelGGL(k_mtf_sum, dim3((unsigned)row.slice_grid, (unsigned)plan.tiles), dim3(kMtfBlock), 0, st, n_groups,
                     s.slice_start, s.bucket_total, s.bucket_start, s.stage, table, planes, plan.n_k, n_out, plan.lanes,
                     slab, weight_slab);
  hipLaunchKernelGGL(k_mtf_fold, dim3((unsigned)(((int64_t)n_groups * n_out + PRT_BLOCK - 1) / PRT_BLOCK)),
                     dim3(PRT_BLOCK), 0, st, n_groups, n_out, s.slice_start, slab, weight_slab, s.bucket_total, s.missed,
                     otf_out, record_out);
  return mtf_finish(st, scratch);
}
