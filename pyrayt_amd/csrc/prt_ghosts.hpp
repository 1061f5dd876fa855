// prt_ghosts.hpp -- ghost rays spawned from the frame, on the device: at every refraction a ray's
// rows describe, at the surfaces the caller lists, the energy the Fresnel pass says did not go through leaves as one
// reflected child ray.  The children are an ordinary (13, n) ray set for prt_trace; nothing of the trace is touched.
// The pass has prt_fresnel.hpp's shape -- the join by ray id (prt_join.hpp), one launch per generation, one row a thread
// -- and then the stable counting sort of prt_sort.hpp, which orders the children by (parent group, surface) and so
// makes every ghost path a "source" of the per-source passes.  Definitions: include/prt.h.
//
//   ghost_child     the child of an interface, written once for the two kernels that need it (the same bits in both)
//   k_ghost_mark    one launch per generation: a row finds its ray's previous row p, reads the interface as fresnel_row
//                   does and writes p's bucket (or leaves -1) and its own number beside it; then the counters
//   k_ghost_tally   the sort's count over the marks, a wave a contiguous run of rows
//   k_ghost_groups  one workgroup: the buckets' starts, the non-empty buckets numbered, the largest count
//   k_ghost_emit    the sort's scatter: a marked row computes its child again and writes it where the sort puts it
// The host has to size the ray set between counting and writing: prt_frame_ghosts_count runs the first three and keeps
// what the fourth needs in its workspace, prt_frame_ghosts_emit runs the fourth.
// No two lanes write one row's mark (ids do not repeat within a generation, so no two rows share a previous row); there
// are no floating-point atomics and no floating-point sums across rows; the counters are integers, summed by ballot and
// LDS and added with one atomic per workgroup (fresnel_count), into one of GHOST_STRIPES copies.  Every output is the
// same bits on every run.  The library is built with -ffp-contract=off: every product and sum below is rounded on its
// own, in the order written, which tests/ghost_reference.py follows operation for operation.
#pragma once

enum { GHOST_BAD_GROUP = JOIN_OWN_BIT };  // (after the join's bits: a ray's group is not in [0, n_groups))
// counters: spawned, dropped, dark, invalid children; rows that end on a listed surface, and those of them with a
// successor (the difference: the open rows)
enum { GHOST_MAX_SURFACES = 64, GHOST_MAX_BUCKETS = 65535, GHOST_COUNTERS = 6, GHOST_RECORD = 8, GHOST_STRIPES = 64 };
enum { GHOST_HEAD_MAGIC = 0, GHOST_HEAD_ROWS, GHOST_HEAD_BUCKETS, GHOST_HEAD_CHILDREN, GHOST_HEAD_GROUPS,
       GHOST_HEAD_STRIDE, GHOST_HEAD = 8 };
static const int64_t kGhostMagic = 0x0073'7473'6f68'6721ll;
static const size_t kGhostCountBytes = (size_t)64 << 20;  // cap of the (wave, bucket) counts

// The counters of this pass are not rare events, as the Fresnel pass's are: nearly every workgroup adds to three of them.
// One copy of the words would take every workgroup's atomics on one cache line, which then costs more than the rows'
// bytes; a workgroup adds to copy blockIdx.x mod GHOST_STRIPES, a cache line each, and the host adds the copies up.
struct alignas(64) GhostWords { u64 count[GHOST_COUNTERS]; int status; };  // (cleared together, read back together)
struct GhostArgs {
  double surface[GHOST_MAX_SURFACES];
  double rays_per_group, min_intensity, ray_offset;
  int n_surfaces, n_groups;
};
struct GhostChild { FrVec origin, ur; double e, wavelength, ni; };

// the position of `surface` in the list, or -1
__device__ __forceinline__ int ghost_listed(const GhostArgs& a, double surface) {
  int at = -1;
  for (int s = a.n_surfaces - 1; s >= 0; --s) at = surface == a.surface[s] ? s : at;
  return at;
}

// the child spawned at the end of row p of a ray whose next row is j (t: the Fresnel pass's transmittance per row)
__device__ __forceinline__ GhostChild ghost_child(const double* __restrict__ rows, int64_t ld,
                                                  const double* __restrict__ t, int64_t p, int64_t j, double ray_offset) {
  GhostChild c;
  const FrVec ui = fr_unit(fr_tilt(rows, ld, p)), ut = fr_unit(fr_tilt(rows, ld, j));
  const double ni = rows[PRT_COL_INDEX * ld + p], nt = rows[PRT_COL_INDEX * ld + j];
  const FrVec n = fr_unit({ni * ui.x - nt * ut.x, ni * ui.y - nt * ut.y, ni * ui.z - nt * ut.z});
  const double twice = 2.0 * fr_dot(ui, n);
  c.ur = {ui.x - twice * n.x, ui.y - twice * n.y, ui.z - twice * n.z};  // (not renormalised)
  c.origin = {rows[PRT_COL_X1 * ld + p] + ray_offset * c.ur.x, rows[PRT_COL_Y1 * ld + p] + ray_offset * c.ur.y,
              rows[PRT_COL_Z1 * ld + p] + ray_offset * c.ur.z};
  c.e = rows[PRT_COL_INTENSITY * ld + p] * (t[p] - t[j]);
  c.wavelength = rows[PRT_COL_WAVELENGTH * ld + p];
  c.ni = ni;
  return c;
}

__device__ __forceinline__ bool ghost_finite(double v) { return fabs(v) < PRT_INF; }  // (false for NaN)

__global__ void __launch_bounds__(kFresnelBlock)
k_ghost_mark(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t start, int64_t count, int generation,
             double id0, int64_t n_ids, GhostArgs args, const double* __restrict__ t, int64_t* __restrict__ last_row,
             int* __restrict__ stamp, GhostWords* __restrict__ words, int* __restrict__ mark, int64_t* __restrict__ next) {
  const int64_t j = start + (int64_t)blockIdx.x * kFresnelBlock + threadIdx.x;
  bool flag[GHOST_COUNTERS] = {};
  words += blockIdx.x & (GHOST_STRIPES - 1);
  if (j < start + count) {
    const int64_t i = join_id(rows, ld, j, id0, n_ids);
    bool joined = false;
    if (i < 0) {
      atomicOr(&words->status, JOIN_BAD_ID);
    } else {
      const int bits = join_status(join_claim(stamp, i, generation), generation);
      joined = !bits;
      if (bits) atomicOr(&words->status, bits);
    }
    flag[4] = ghost_listed(args, rows[PRT_COL_SURFACE * ld + j]) >= 0;
    if (joined && generation > 0) {
      const int64_t p = last_row[i];  // (written by the launch of generation - 1: the stamp said so)
      const int at = p >= 0 && p < n_rows ? ghost_listed(args, rows[PRT_COL_SURFACE * ld + p]) : -1;
      flag[5] = at >= 0;
      if (at >= 0) {
        const double ni = rows[PRT_COL_INDEX * ld + p], nt = rows[PRT_COL_INDEX * ld + j];
        const double tp = t[p], tj = t[j];
        const bool refraction = ni > 0.0 && ni < PRT_INF && nt > 0.0 && nt < PRT_INF && ni != nt;
        if (refraction && ghost_finite(tp) && ghost_finite(tj)) {
          const double group = args.rays_per_group > 0 ? floor((double)i / args.rays_per_group) : 0.0;
          const GhostChild c = ghost_child(rows, ld, t, p, j, args.ray_offset);
          if (!(group < (double)args.n_groups)) {
            atomicOr(&words->status, GHOST_BAD_GROUP);
          } else if (c.e <= 0.0) {
            flag[2] = true;
          } else if (c.e < args.min_intensity) {
            flag[1] = true;
          } else if (ghost_finite(c.e) && ghost_finite(c.wavelength) && ghost_finite(c.origin.x) &&
                     ghost_finite(c.origin.y) && ghost_finite(c.origin.z) && ghost_finite(c.ur.x) &&
                     ghost_finite(c.ur.y) && ghost_finite(c.ur.z)) {
            flag[0] = true;
            mark[p] = (int)group * args.n_surfaces + at;
            next[p] = j;
          } else {
            flag[3] = true;
          }
        }
      }
    }
    if (i >= 0) last_row[i] = j;  // (also for a row the status word refuses: what the next generation reads is this launch's)
  }
  fresnel_count(flag, words->count);
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_ghost_tally(const int* __restrict__ mark, int64_t n_rows, int64_t per_wave, int n_buckets, int64_t* __restrict__ counts) {
  const SortRun run = sort_run(per_wave, n_rows);
  int64_t* const mine = counts + run.wave * n_buckets;  // (only this wave writes here)
  for (int64_t base = run.first; base < run.last; base += 64) {
    const int64_t j = base + run.lane;
    sort_tally(run.lane, j < run.last ? mark[j] : -1, mine);
  }
}

// bucket_start[0 .. n_buckets] (the last: all children); group_of[b]: the number of bucket b among the non-empty ones;
// the head's three results
__global__ void __launch_bounds__(kSortScanBlock)
k_ghost_groups(int n_buckets, int64_t n_rows, const int64_t* __restrict__ bucket_total, int64_t* __restrict__ bucket_start,
               int64_t* __restrict__ group_of, int64_t* __restrict__ head) {
  __shared__ int64_t scan[kSortScanBlock];
  const int64_t children = sort_scan(
      n_buckets, [&](int64_t b) { return bucket_total[b]; }, [&](int64_t b, int64_t before) { bucket_start[b] = before; },
      scan);
  const int64_t groups = sort_scan(
      n_buckets, [&](int64_t b) { return (int64_t)(bucket_total[b] > 0); },
      [&](int64_t b, int64_t before) { group_of[b] = before; }, scan);
  int64_t most = 0;
  for (int b = threadIdx.x; b < n_buckets; b += kSortScanBlock) most = bucket_total[b] > most ? bucket_total[b] : most;
  __syncthreads();  // (scan is read by the calls above)
  scan[threadIdx.x] = most;
  for (int half = kSortScanBlock / 2; half > 0; half >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < half && scan[threadIdx.x + half] > scan[threadIdx.x]) scan[threadIdx.x] = scan[threadIdx.x + half];
  }
  if (threadIdx.x == 0) {
    bucket_start[n_buckets] = children;
    head[GHOST_HEAD_MAGIC] = kGhostMagic; head[GHOST_HEAD_ROWS] = n_rows; head[GHOST_HEAD_BUCKETS] = n_buckets;
    head[GHOST_HEAD_CHILDREN] = children; head[GHOST_HEAD_GROUPS] = groups; head[GHOST_HEAD_STRIDE] = scan[0];
    head[6] = head[7] = 0;
  }
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_ghost_emit(const double* __restrict__ rows, int64_t ld, int64_t n_rows, const double* __restrict__ t, double ray_offset,
             int64_t per_wave, int n_buckets, const int* __restrict__ mark, const int64_t* __restrict__ next,
             int64_t* __restrict__ offsets, const int64_t* __restrict__ bucket_start, const int64_t* __restrict__ group_of,
             const int64_t* __restrict__ head, int64_t n_children, int64_t ld_rays, double* __restrict__ rays,
             int64_t* __restrict__ parent_row) {
  const SortRun run = sort_run(per_wave, n_rows);
  if (run.first >= run.last) return;
  int64_t* const mine = offsets + run.wave * n_buckets;  // (only this wave reads and writes here)
  const double stride = (double)head[GHOST_HEAD_STRIDE];
  for (int64_t base = run.first; base < run.last; base += 64) {
    const int64_t p = base + run.lane;
    int bucket = p < run.last ? mark[p] : -1;
    bucket = bucket < n_buckets ? bucket : -1;
    if (__ballot(bucket >= 0) == 0ull) continue;
    GhostChild c = {};
    if (bucket >= 0) {
      const int64_t j = next[p];
      if (j >= 0 && j < n_rows) c = ghost_child(rows, ld, t, p, j, ray_offset);
    }
    sort_place(run.lane, bucket, mine, bucket_start, [&](int64_t slot) {
      if (slot >= n_children) return;  // (the host has checked n_children against the head)
      const double id = (double)group_of[bucket] * stride + (double)(slot - bucket_start[bucket]);
      rays[PRT_ROW_OX * ld_rays + slot] = c.origin.x; rays[PRT_ROW_OY * ld_rays + slot] = c.origin.y;
      rays[PRT_ROW_OZ * ld_rays + slot] = c.origin.z; rays[PRT_ROW_OW * ld_rays + slot] = 1.0;
      rays[PRT_ROW_DX * ld_rays + slot] = c.ur.x; rays[PRT_ROW_DY * ld_rays + slot] = c.ur.y;
      rays[PRT_ROW_DZ * ld_rays + slot] = c.ur.z; rays[PRT_ROW_DW * ld_rays + slot] = 0.0;
      rays[PRT_ROW_GENERATION * ld_rays + slot] = 0.0; rays[PRT_ROW_INTENSITY * ld_rays + slot] = c.e;
      rays[PRT_ROW_WAVELENGTH * ld_rays + slot] = c.wavelength; rays[PRT_ROW_INDEX * ld_rays + slot] = c.ni;
      rays[PRT_ROW_ID * ld_rays + slot] = id;
      parent_row[slot] = p;
    });
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------
struct GhostWork {
  GhostWords* words; int64_t *head, *bucket_total, *bucket_start, *group_of, *next, *last_row, *counts; int *mark, *stamp;
};

static bool ghost_sizes_ok(int64_t n_rows, int n_buckets) {
  return n_rows >= 0 && n_buckets >= 1 && n_buckets <= GHOST_MAX_BUCKETS && n_rows / 64 + 1 <= 0x7fffffff;
}
static SortPlan ghost_plan(int64_t n_rows, int n_buckets) { return sort_plan(n_rows, n_buckets, 8, kGhostCountBytes); }

static GhostWork ghost_carve(void* workspace, int64_t n_rows, int64_t n_ids, int n_buckets) {
  GhostWork w;
  w.words = (GhostWords*)(((uintptr_t)workspace + 63) & ~(uintptr_t)63);
  w.head = (int64_t*)(w.words + GHOST_STRIPES);
  w.bucket_total = w.head + GHOST_HEAD;
  w.bucket_start = w.bucket_total + (n_buckets + 1);
  w.group_of = w.bucket_start + (n_buckets + 1);
  w.next = w.group_of + (n_buckets + 1);
  w.last_row = w.next + n_rows;
  w.counts = w.last_row + n_ids;
  w.mark = (int*)((char*)w.counts + ghost_plan(n_rows, n_buckets).count_bytes);
  w.stamp = w.mark + n_rows;
  return w;
}

extern "C" int64_t prt_frame_ghosts_count_workspace_bytes(int64_t n_rows, int64_t n_ids, int n_buckets) {
  if (!ghost_sizes_ok(n_rows, n_buckets) || !join_n_ids_ok(n_ids)) return PRT_ERR_ARG;
  return 64 + GHOST_STRIPES * (int64_t)sizeof(GhostWords) + (GHOST_HEAD + 3 * ((int64_t)n_buckets + 1) + n_rows + n_ids) * 8 +
         (int64_t)ghost_plan(n_rows, n_buckets).count_bytes + (n_rows + n_ids) * 4;
}

extern "C" int prt_frame_ghosts_count(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                                      int n_generations, double id0, int64_t n_ids, const double* transmittance,
                                      const int64_t* surfaces, int n_surfaces, double rays_per_group, int n_groups,
                                      double min_intensity, double ray_offset, int64_t* bucket_count_out,
                                      int64_t* record_out, void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  const int64_t n_rows = join_rows(rows_per_generation, n_generations, ld, kFresnelBlock, "ghosts");
  if (n_rows < 0) return (int)n_rows;
  if (!record_out || !bucket_count_out || !workspace || (n_rows && (!rows || !transmittance)))
    return fail(PRT_ERR_ARG, "bad buffers");
  int rc = join_ids(id0, n_ids);
  if (rc) return rc;
  if (n_surfaces < 1 || n_surfaces > GHOST_MAX_SURFACES || !surfaces)
    return fail(PRT_ERR_ARG, "ghosts: 1 to 64 surfaces");
  if (n_groups < 1 || (int64_t)n_groups * n_surfaces > GHOST_MAX_BUCKETS)
    return fail(PRT_ERR_ARG, "ghosts: n_groups * n_surfaces in [1, 65535]");
  if (!(rays_per_group > 0) && n_groups != 1) return fail(PRT_ERR_ARG, "one group without rays_per_group");
  if (!(min_intensity >= 0.0 && min_intensity < PRT_INF) || !(std::fabs(ray_offset) < PRT_INF))
    return fail(PRT_ERR_ARG, "ghosts: min_intensity finite and >= 0, ray_offset finite");
  const int n_buckets = n_groups * n_surfaces;
  if (!ghost_sizes_ok(n_rows, n_buckets)) return fail(PRT_ERR_ARG, "ghosts: too many rows for one launch");
  GhostArgs args;
  std::memset(&args, 0, sizeof(args));
  for (int k = 0; k < n_surfaces; ++k) {
    args.surface[k] = (double)surfaces[k];
    for (int q = 0; q < k; ++q)
      if (surfaces[q] == surfaces[k]) return fail(PRT_ERR_ARG, "ghosts: a surface is listed twice");
  }
  args.rays_per_group = rays_per_group > 0 ? rays_per_group : 0.0;
  args.min_intensity = min_intensity; args.ray_offset = ray_offset;
  args.n_surfaces = n_surfaces; args.n_groups = n_groups;
  for (int k = 0; k < GHOST_RECORD; ++k) record_out[k] = 0;
  for (int b = 0; b < n_buckets; ++b) bucket_count_out[b] = 0;
  if (!n_rows) return PRT_OK;
  rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const GhostWork w = ghost_carve(workspace, n_rows, n_ids, n_buckets);
  const SortPlan plan = ghost_plan(n_rows, n_buckets);
  HIP_TRY(hipMemsetAsync(w.words, 0, GHOST_STRIPES * sizeof(GhostWords) + GHOST_HEAD * 8, st));  // (and the head)
  HIP_TRY(hipMemsetAsync(w.stamp, 0, (size_t)n_ids * sizeof(int), st));
  HIP_TRY(hipMemsetAsync(w.mark, 0xff, (size_t)n_rows * sizeof(int), st));
  HIP_TRY(hipMemsetAsync(w.counts, 0, plan.count_bytes, st));
  int64_t start = 0;
  for (int g = 0; g < n_generations; ++g) {
    const int64_t count = rows_per_generation[g];
    if (count)
      hipLaunchKernelGGL(k_ghost_mark, dim3((unsigned)((count + kFresnelBlock - 1) / kFresnelBlock)), dim3(kFresnelBlock), 0,
                         st, rows, ld, n_rows, start, count, g, id0, n_ids, args, transmittance, w.last_row, w.stamp,
                         w.words, w.mark, w.next);
    start += count;
  }
  hipLaunchKernelGGL(k_ghost_tally, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, w.mark, n_rows, plan.per_wave, n_buckets,
                     w.counts);
  hipLaunchKernelGGL(k_sort_offsets, dim3((unsigned)n_buckets), dim3(kSortScanBlock), 0, st, (int)plan.all_waves, n_buckets,
                     w.counts, w.bucket_total);
  hipLaunchKernelGGL(k_ghost_groups, dim3(1), dim3(kSortScanBlock), 0, st, n_buckets, n_rows, w.bucket_total,
                     w.bucket_start, w.group_of, w.head);
  GhostWords stripes[GHOST_STRIPES], host_words = {};
  int64_t head[GHOST_HEAD];
  HIP_TRY(hipMemcpyAsync(stripes, w.words, sizeof(stripes), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(head, w.head, sizeof(head), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(bucket_count_out, w.bucket_total, (size_t)n_buckets * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  for (const GhostWords& stripe : stripes) {
    host_words.status |= stripe.status;
    for (int k = 0; k < GHOST_COUNTERS; ++k) host_words.count[k] += stripe.count[k];
  }
  rc = join_refusal(host_words.status, "ghosts");
  if (!rc && (host_words.status & GHOST_BAD_GROUP))
    rc = fail(PRT_ERR_ARG, "ghosts: a ray's group, floor((id - id0) / rays_per_group), is not below n_groups");
  if (rc) {
    for (int b = 0; b < n_buckets; ++b) bucket_count_out[b] = 0;
    return rc;
  }
  for (int k = 0; k < 4; ++k) record_out[k] = (int64_t)host_words.count[k];
  record_out[4] = (int64_t)(host_words.count[4] - host_words.count[5]);
  record_out[5] = head[GHOST_HEAD_GROUPS];
  record_out[6] = head[GHOST_HEAD_STRIDE];
  return PRT_OK;
}

extern "C" int64_t prt_frame_ghosts_emit_workspace_bytes(int64_t n_rows, int n_buckets) {
  if (!ghost_sizes_ok(n_rows, n_buckets)) return PRT_ERR_ARG;
  return (int64_t)ghost_plan(n_rows, n_buckets).count_bytes + 64;
}

extern "C" int prt_frame_ghosts_emit(int device, const double* rows, int64_t ld, int64_t n_rows, int64_t n_ids,
                                     const double* transmittance, double ray_offset, int n_buckets, int64_t n_children,
                                     const void* count_workspace, double* rays_out, int64_t ld_rays,
                                     int64_t* parent_row_out, void* workspace, void* stream) {
  if (!ghost_sizes_ok(n_rows, n_buckets) || ld < n_rows || !join_n_ids_ok(n_ids) || n_children < 0 ||
      ld_rays < n_children || !workspace || !count_workspace || (n_rows && (!rows || !transmittance)) ||
      (n_children && (!rays_out || !parent_row_out)))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (!(std::fabs(ray_offset) < PRT_INF)) return fail(PRT_ERR_ARG, "ghosts: ray_offset finite");
  if (!n_rows) return n_children ? fail(PRT_ERR_ARG, "ghosts: n_children is not what the count found") : PRT_OK;
  int rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const GhostWork w = ghost_carve(const_cast<void*>(count_workspace), n_rows, n_ids, n_buckets);
  int64_t head[GHOST_HEAD];
  HIP_TRY(hipMemcpyAsync(head, w.head, sizeof(head), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (head[GHOST_HEAD_MAGIC] != kGhostMagic || head[GHOST_HEAD_ROWS] != n_rows || head[GHOST_HEAD_BUCKETS] != n_buckets)
    return fail(PRT_ERR_ARG, "ghosts: count_workspace is not that of a count of this frame");
  if (head[GHOST_HEAD_CHILDREN] != n_children) return fail(PRT_ERR_ARG, "ghosts: n_children is not what the count found");
  if (!n_children) return PRT_OK;
  const SortPlan plan = ghost_plan(n_rows, n_buckets);
  int64_t* offsets = (int64_t*)(((uintptr_t)workspace + 63) & ~(uintptr_t)63);
  // (the scatter advances the waves' offsets: on a copy, so that the count's workspace serves another emit)
  HIP_TRY(hipMemcpyAsync(offsets, w.counts, plan.count_bytes, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_ghost_emit, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_rows, transmittance, ray_offset,
                     plan.per_wave, n_buckets, w.mark, w.next, offsets, w.bucket_start, w.group_of, w.head, n_children,
                     ld_rays, rays_out, parent_row_out);
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return PRT_OK;
}
