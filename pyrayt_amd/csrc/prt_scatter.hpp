// prt_scatter.hpp -- stray light by surface scatter, spawned from the frame on the device: every
// row that lands on a listed surface sends N child rays back into the half space it came from, each with the energy its
// surface's BSDF gives the direction drawn for it.  The children are an ordinary (13, n) ray set for prt_trace; nothing
// of the trace is touched.  The pass has prt_ghosts.hpp's shape with items (row, child) in place of rows -- item
// p * N + c is child c of row p -- and needs no join: a row spawns whatever happens to its ray afterwards.
// Definitions: include/prt.h.
//
//   scatter_child   the child of an item, written once for the two kernels that need it (the same bits in both): the
//                   Philox4x32-10 sample of (seed, id, generation, child), the surface's normal from the trace's own
//                   world_normal_len turned against the ray, the direction (cosine-weighted, or towards a point of
//                   the target disk), the BSDF table's value and the energy
//   k_scatter_mark  one item a thread: a row whose surface is not listed leaves -1 before any arithmetic; otherwise the
//                   child's fate, and its bucket in mark[item]; then the counters
//   k_ghost_tally, k_sort_offsets, k_ghost_groups   the ghost pass's, as they are, over the item marks
//   k_scatter_emit  the sort's scatter: a marked item computes its child again and writes it where the sort puts it
// The N lanes of a row read its columns at one address.  The listed surfaces' primitives (SensSurface, at most 64, in
// the order of the list) and the BSDF tables lie in the count's workspace and are read through the caches.  There are
// no floating-point atomics and no floating-point sums across items; the counters are integers, summed by ballot and
// LDS and added with one atomic per workgroup into one of GHOST_STRIPES copies.  Every output is the same bits on every
// run.  The library is built with -ffp-contract=off: every product and sum below is rounded on its own, in the order
// written (the fma calls of world_normal_len are the trace's own), which tests/scatter_reference.py follows operation
// for operation.
// (included below prt_ghosts.hpp and prt_sensitivity.hpp)
#pragma once

enum { SCATTER_BAD_ID = 1, SCATTER_BAD_GROUP = 2 };
// counters: spawned, rejected, below the horizon, dark, dropped, invalid
enum { SCATTER_MAX_MODELS = 16, SCATTER_KNOTS = 1024, SCATTER_MAX_CHILDREN = 64, SCATTER_COUNTERS = 6, SCATTER_RECORD = 8 };
static const int64_t kScatterMagic = 0x0072'6574'7461'6373ll;

struct ScatterArgs {
  double surface[GHOST_MAX_SURFACES];
  int model[GHOST_MAX_SURFACES];
  double centre[3], normal[3], e1[3], e2[3], radius, four_r2;  // the target disk (toward: 1)
  double rays_per_group, min_intensity, ray_offset, n_children;  // n_children: N as a double
  uint32_t key[2];
  int n_surfaces, n_groups, rays_per_hit, toward;
};
// what the count leaves for the emit, in front of its workspace
struct alignas(64) ScatterKeep { int64_t magic, n_rows; ScatterArgs args; };
enum { SCATTER_SPAWNED = 0, SCATTER_REJECTED, SCATTER_BELOW, SCATTER_DARK, SCATTER_DROPPED, SCATTER_INVALID };
struct ScatterChild { FrVec origin, uo; double e, wavelength, ni; };

// Philox4x32-10 (Salmon et al. 2011): the four words of counter c under key k
__device__ __forceinline__ void scatter_philox(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t y0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, y2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = y0; c[2] = y2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
__device__ __forceinline__ double scatter_uniform(uint32_t hi, uint32_t lo) {  // in [0, 1)
  return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1p-53;
}

// the orthonormal basis of a unit vector n (Duff et al. 2017): one division, products and sums
__device__ __forceinline__ void scatter_basis(const FrVec& n, FrVec& t1, FrVec& t2) {
  const double sign = copysign(1.0, n.z);
  const double a = -1.0 / (sign + n.z);
  const double b = (n.x * n.y) * a;
  const double sx = sign * n.x;
  t1 = {1.0 + (sx * n.x) * a, sign * b, -sx};
  t2 = {b, sign + (n.y * n.y) * a, -n.y};
}

// the table's value at b = |beta - beta0|; NaN where b is not a number
__device__ __forceinline__ double scatter_bsdf(const double* __restrict__ tab, double b) {
  const double q = sqrt(0.5 * b) * (double)SCATTER_KNOTS;
  if (!(q >= 0.0)) return __builtin_nan("");
  const int k = q < (double)(SCATTER_KNOTS - 1) ? (int)q : SCATTER_KNOTS - 1;
  const double lo = tab[k];
  return lo + (q - (double)k) * (tab[k + 1] - lo);
}

// child c of row p: its fate as far as the sample and the horizon decide it (SCATTER_SPAWNED: not decided yet), and
// the child.  surfaces: the listed surfaces' primitives in list order; at: the row's place in the list
__device__ __forceinline__ int scatter_child(const double* __restrict__ rows, int64_t ld, int64_t p, uint32_t c,
                                             const ScatterArgs& args, const SensSurface* __restrict__ surfaces,
                                             const double* __restrict__ tables, int at, ScatterChild& out) {
  const int64_t id = (int64_t)rows[PRT_COL_ID * ld + p];
  uint32_t word[4] = {(uint32_t)id, (uint32_t)((uint64_t)id >> 32), (uint32_t)(int64_t)rows[PRT_COL_GENERATION * ld + p], c};
  scatter_philox(word, args.key[0], args.key[1]);
  const double a = 2.0 * scatter_uniform(word[0], word[1]) - 1.0, b = 2.0 * scatter_uniform(word[2], word[3]) - 1.0;
  const double s = a * a + b * b;
  if (!(s < 1.0)) return SCATTER_REJECTED;
  const FrVec x = {rows[PRT_COL_X1 * ld + p], rows[PRT_COL_Y1 * ld + p], rows[PRT_COL_Z1 * ld + p]};
  const FrVec ui = fr_unit(fr_tilt(rows, ld, p));
  FrVec n;
  double len;
  world_normal_len(surfaces + at, x.x, x.y, x.z, 1.0, n.x, n.y, n.z, len);
  if (fr_dot(n, ui) > 0.0) n = {-n.x, -n.y, -n.z};
  const double intensity = rows[PRT_COL_INTENSITY * ld + p];
  FrVec uo;
  double cos_o = 1.0, cos_t = 1.0, r2 = 1.0;
  if (args.toward) {
    const double ha = args.radius * (a * args.e1[0] + b * args.e2[0]), hb = args.radius * (a * args.e1[1] + b * args.e2[1]),
                 hc = args.radius * (a * args.e1[2] + b * args.e2[2]);
    const FrVec v = {(args.centre[0] + ha) - x.x, (args.centre[1] + hb) - x.y, (args.centre[2] + hc) - x.z};
    r2 = fr_dot(v, v);
    const double r = sqrt(r2);
    uo = {v.x / r, v.y / r, v.z / r};
    cos_o = fr_dot(n, uo);
    if (cos_o <= 0.0) return SCATTER_BELOW;
    cos_t = fabs(fr_dot({args.normal[0], args.normal[1], args.normal[2]}, uo));
  } else {
    const double cz = sqrt(1.0 - s);
    if (!(cz > 0.0)) return SCATTER_REJECTED;
    FrVec t1, t2;
    scatter_basis(n, t1, t2);
    uo = {(a * t1.x + b * t2.x) + cz * n.x, (a * t1.y + b * t2.y) + cz * n.y, (a * t1.z + b * t2.z) + cz * n.z};
  }
  const FrVec d = {uo.x - ui.x, uo.y - ui.y, uo.z - ui.z};
  const double dn = fr_dot(d, n);
  const FrVec across = {d.x - dn * n.x, d.y - dn * n.y, d.z - dn * n.z};
  const double f = scatter_bsdf(tables + (int64_t)args.model[at] * (SCATTER_KNOTS + 1), sqrt(fr_dot(across, across)));
  out.e = args.toward ? ((((intensity * f) * cos_o) * cos_t) * args.four_r2) / (args.n_children * r2)
                      : ((4.0 * intensity) * f) / args.n_children;
  out.uo = uo;
  out.origin = {x.x + args.ray_offset * uo.x, x.y + args.ray_offset * uo.y, x.z + args.ray_offset * uo.z};
  out.wavelength = rows[PRT_COL_WAVELENGTH * ld + p];
  out.ni = rows[PRT_COL_INDEX * ld + p];
  return SCATTER_SPAWNED;
}

// the place of `surface` in the list, or -1
__device__ __forceinline__ int scatter_listed(const ScatterArgs& a, double surface) {
  int at = -1;
  for (int s = a.n_surfaces - 1; s >= 0; --s) at = surface == a.surface[s] ? s : at;
  return at;
}

__global__ void __launch_bounds__(kFresnelBlock)
k_scatter_mark(const double* __restrict__ rows, int64_t ld, int64_t n_items, ScatterArgs args,
               const SensSurface* __restrict__ surfaces, const double* __restrict__ tables,
               GhostWords* __restrict__ words, int* __restrict__ mark) {
  const int64_t item = (int64_t)blockIdx.x * kFresnelBlock + threadIdx.x;
  bool flag[SCATTER_COUNTERS] = {};
  words += blockIdx.x & (GHOST_STRIPES - 1);
  if (item < n_items) {
    const uint32_t n = (uint32_t)args.rays_per_hit;
    const int64_t p = (int64_t)((uint32_t)item / n);
    const int at = scatter_listed(args, rows[PRT_COL_SURFACE * ld + p]);
    int bucket = -1;
    if (at >= 0) {
      const double id = rows[PRT_COL_ID * ld + p], generation = rows[PRT_COL_GENERATION * ld + p];
      const double group = args.rays_per_group > 0 ? floor(id / args.rays_per_group) : 0.0;
      if (!(id >= 0.0 && id < 0x1p53 && id == floor(id) && generation >= 0.0 && generation < 0x1p31 &&
            generation == floor(generation))) {
        atomicOr(&words->status, SCATTER_BAD_ID);
      } else if (!(group < (double)args.n_groups)) {
        atomicOr(&words->status, SCATTER_BAD_GROUP);
      } else {
        ScatterChild c;
        int fate = scatter_child(rows, ld, p, (uint32_t)item - (uint32_t)p * n, args, surfaces, tables, at, c);
        if (fate == SCATTER_SPAWNED) {
          if (c.e <= 0.0) {
            fate = SCATTER_DARK;
          } else if (c.e < args.min_intensity) {
            fate = SCATTER_DROPPED;
          } else if (!(ghost_finite(c.e) && ghost_finite(c.wavelength) && ghost_finite(c.ni) && ghost_finite(c.origin.x) &&
                       ghost_finite(c.origin.y) && ghost_finite(c.origin.z) && ghost_finite(c.uo.x) &&
                       ghost_finite(c.uo.y) && ghost_finite(c.uo.z))) {
            fate = SCATTER_INVALID;
          } else {
            bucket = (int)group * args.n_surfaces + at;
          }
        }
#pragma unroll
        for (int k = 0; k < SCATTER_COUNTERS; ++k) flag[k] = fate == k;
      }
    }
    mark[item] = bucket;
  }
  fresnel_count(flag, words->count);
}

__global__ void __launch_bounds__(PRT_BLOCK)
k_scatter_emit(const double* __restrict__ rows, int64_t ld, int64_t n_items, ScatterArgs args,
               const SensSurface* __restrict__ surfaces, const double* __restrict__ tables, int64_t per_wave,
               int n_buckets, const int* __restrict__ mark, int64_t* __restrict__ offsets,
               const int64_t* __restrict__ bucket_start, const int64_t* __restrict__ group_of,
               const int64_t* __restrict__ head, int64_t n_children, int64_t ld_rays, double* __restrict__ rays,
               int64_t* __restrict__ parent_row, int* __restrict__ child) {
  const SortRun run = sort_run(per_wave, n_items);
  if (run.first >= run.last) return;
  int64_t* const mine = offsets + run.wave * n_buckets;  // (only this wave reads and writes here)
  const double stride = (double)head[GHOST_HEAD_STRIDE];
  const uint32_t n = (uint32_t)args.rays_per_hit;
  for (int64_t base = run.first; base < run.last; base += 64) {
    const int64_t item = base + run.lane;
    int bucket = item < run.last ? mark[item] : -1;
    bucket = bucket < n_buckets ? bucket : -1;
    if (__ballot(bucket >= 0) == 0ull) continue;
    ScatterChild c = {};
    const int64_t p = (int64_t)((uint32_t)item / n);
    const uint32_t which = (uint32_t)item - (uint32_t)p * n;
    if (bucket >= 0) {
      const int at = bucket % args.n_surfaces;
      if (rows[PRT_COL_SURFACE * ld + p] == args.surface[at])  // (as the mark found it; anything else writes zeros)
        scatter_child(rows, ld, p, which, args, surfaces, tables, at, c);
    }
    sort_place(run.lane, bucket, mine, bucket_start, [&](int64_t slot) {
      if (slot >= n_children) return;  // (the host has checked n_children against the head)
      const double id = (double)group_of[bucket] * stride + (double)(slot - bucket_start[bucket]);
      rays[PRT_ROW_OX * ld_rays + slot] = c.origin.x; rays[PRT_ROW_OY * ld_rays + slot] = c.origin.y;
      rays[PRT_ROW_OZ * ld_rays + slot] = c.origin.z; rays[PRT_ROW_OW * ld_rays + slot] = 1.0;
      rays[PRT_ROW_DX * ld_rays + slot] = c.uo.x; rays[PRT_ROW_DY * ld_rays + slot] = c.uo.y;
      rays[PRT_ROW_DZ * ld_rays + slot] = c.uo.z; rays[PRT_ROW_DW * ld_rays + slot] = 0.0;
      rays[PRT_ROW_GENERATION * ld_rays + slot] = 0.0; rays[PRT_ROW_INTENSITY * ld_rays + slot] = c.e;
      rays[PRT_ROW_WAVELENGTH * ld_rays + slot] = c.wavelength; rays[PRT_ROW_INDEX * ld_rays + slot] = c.ni;
      rays[PRT_ROW_ID * ld_rays + slot] = id;
      parent_row[slot] = p;
      child[slot] = (int)which;
    });
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------
struct ScatterWork {
  ScatterKeep* keep; GhostWords* words; int64_t *head, *bucket_total, *bucket_start, *group_of, *counts;
  SensSurface* surfaces; double* tables; int* mark;
};

static bool scatter_sizes_ok(int64_t n_rows, int rays_per_hit, int n_buckets, int n_models) {
  return n_rows >= 0 && rays_per_hit >= 1 && rays_per_hit <= SCATTER_MAX_CHILDREN && n_rows * rays_per_hit < 0x7fffffffll &&
         n_models >= 1 && n_models <= SCATTER_MAX_MODELS && ghost_sizes_ok(n_rows * rays_per_hit, n_buckets);
}

static ScatterWork scatter_carve(void* workspace, int64_t n_items, int n_buckets, int n_models) {
  ScatterWork w;
  w.keep = (ScatterKeep*)(((uintptr_t)workspace + 63) & ~(uintptr_t)63);
  w.words = (GhostWords*)(w.keep + 1);
  w.head = (int64_t*)(w.words + GHOST_STRIPES);
  w.bucket_total = w.head + GHOST_HEAD;
  w.bucket_start = w.bucket_total + (n_buckets + 1);
  w.group_of = w.bucket_start + (n_buckets + 1);
  w.counts = w.group_of + (n_buckets + 1);
  w.surfaces = (SensSurface*)((char*)w.counts + ghost_plan(n_items, n_buckets).count_bytes);
  w.tables = (double*)(w.surfaces + GHOST_MAX_SURFACES);
  w.mark = (int*)(w.tables + (int64_t)n_models * (SCATTER_KNOTS + 1));
  return w;
}

extern "C" int64_t prt_frame_scatter_count_workspace_bytes(int64_t n_rows, int rays_per_hit, int n_buckets, int n_models) {
  if (!scatter_sizes_ok(n_rows, rays_per_hit, n_buckets, n_models)) return PRT_ERR_ARG;
  const int64_t n_items = n_rows * rays_per_hit;
  return 64 + (int64_t)sizeof(ScatterKeep) + GHOST_STRIPES * (int64_t)sizeof(GhostWords) +
         (GHOST_HEAD + 3 * ((int64_t)n_buckets + 1)) * 8 + (int64_t)ghost_plan(n_items, n_buckets).count_bytes +
         GHOST_MAX_SURFACES * (int64_t)sizeof(SensSurface) + (int64_t)n_models * (SCATTER_KNOTS + 1) * 8 + n_items * 4;
}

extern "C" int prt_frame_scatter_count(int device, const double* rows, int64_t ld, int64_t n_rows, const prt_prim* prims,
                                       int n_prims, const int64_t* surfaces, const int* models, int n_surfaces,
                                       const double* tables, int n_models, const double* target, int rays_per_hit,
                                       uint64_t seed, double rays_per_group, int n_groups, double min_intensity,
                                       double ray_offset, int64_t* bucket_count_out, int64_t* record_out, void* workspace,
                                       void* stream) {
  // (everything is checked before a device is touched)
  if (n_rows < 0 || ld < n_rows || !record_out || !bucket_count_out || !workspace || (n_rows && !rows))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (rays_per_hit < 1 || rays_per_hit > SCATTER_MAX_CHILDREN) return fail(PRT_ERR_ARG, "scatter: 1 to 64 rays a hit");
  if (n_rows * rays_per_hit >= 0x7fffffffll) return fail(PRT_ERR_ARG, "scatter: rows x rays a hit below 2^31");
  if (n_surfaces < 1 || n_surfaces > GHOST_MAX_SURFACES || !surfaces || !models)
    return fail(PRT_ERR_ARG, "scatter: 1 to 64 surfaces");
  if (n_models < 1 || n_models > SCATTER_MAX_MODELS || !tables) return fail(PRT_ERR_ARG, "scatter: 1 to 16 models");
  if (n_groups < 1 || (int64_t)n_groups * n_surfaces > GHOST_MAX_BUCKETS)
    return fail(PRT_ERR_ARG, "scatter: n_groups * n_surfaces in [1, 65535]");
  if (!(rays_per_group > 0) && n_groups != 1) return fail(PRT_ERR_ARG, "one group without rays_per_group");
  if (!(min_intensity >= 0.0 && min_intensity < PRT_INF) || !(std::fabs(ray_offset) < PRT_INF))
    return fail(PRT_ERR_ARG, "scatter: min_intensity finite and >= 0, ray_offset finite");
  if (n_prims < 1 || n_prims > (1 << 20) || !prims) return fail(PRT_ERR_ARG, "scatter: 1 to 2^20 surfaces in the table");
  for (int s = 0; s < n_prims; ++s) {
    const prt_prim& pr = prims[s];
    if (pr.type < PRT_PRIM_SPHERE || pr.type > PRT_PRIM_PARABOLOID || (pr.normal_scale != 1 && pr.normal_scale != -1))
      return fail(PRT_ERR_ARG, "scatter: a surface of unknown kind or normal_scale");
    if (s && !(prims[s - 1].surface_id < pr.surface_id))
      return fail(PRT_ERR_ARG, "scatter: the surface table is sorted by id, ids distinct");
  }
  const int n_buckets = n_groups * n_surfaces;
  const int64_t n_items = n_rows * rays_per_hit;
  if (!ghost_sizes_ok(n_items, n_buckets)) return fail(PRT_ERR_ARG, "scatter: too many rows for one launch");
  ScatterKeep keep;
  std::memset(&keep, 0, sizeof(keep));
  ScatterArgs& args = keep.args;
  std::vector<SensSurface> listed((size_t)GHOST_MAX_SURFACES);
  std::memset(listed.data(), 0, listed.size() * sizeof(SensSurface));
  for (int k = 0; k < n_surfaces; ++k) {
    for (int q = 0; q < k; ++q)
      if (surfaces[q] == surfaces[k]) return fail(PRT_ERR_ARG, "scatter: a surface is listed twice");
    if (models[k] < 0 || models[k] >= n_models) return fail(PRT_ERR_ARG, "scatter: a surface's model is not in [0, n_models)");
    int lo = 0, hi = n_prims;  // (the bisection of sens_find, on the host: the device reads the entry by its place in the list)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (prims[mid].surface_id < surfaces[k]) lo = mid + 1; else hi = mid;
    }
    if (lo == n_prims || prims[lo].surface_id != surfaces[k])
      return fail(PRT_ERR_ARG, "scatter: a listed surface is not in the surface table");
    const prt_prim& pr = prims[lo];
    SensSurface& out = listed[(size_t)k];
    for (int i = 0; i < 16; ++i) {
      if (!(std::fabs(pr.minv[i]) < PRT_INF)) return fail(PRT_ERR_ARG, "scatter: a surface's minv is not finite");
      out.minv[i] = pr.minv[i];
    }
    for (int i = 0; i < 6; ++i) out.params[i] = pr.params[i];
    out.surface_id = (double)pr.surface_id;
    out.type = pr.type;
    out.normal_scale = pr.normal_scale;
    args.surface[k] = (double)surfaces[k];
    args.model[k] = models[k];
  }
  for (int64_t k = 0; k < (int64_t)n_models * (SCATTER_KNOTS + 1); ++k)
    if (!(tables[k] >= 0.0 && tables[k] < PRT_INF)) return fail(PRT_ERR_ARG, "scatter: a BSDF table is finite and >= 0");
  if (target) {
    for (int k = 0; k < 13; ++k)
      if (!(std::fabs(target[k]) < PRT_INF)) return fail(PRT_ERR_ARG, "scatter: the target is finite");
    const double nn = (target[3] * target[3] + target[4] * target[4]) + target[5] * target[5];
    if (!(target[12] > 0.0)) return fail(PRT_ERR_ARG, "scatter: the target's radius is > 0");
    if (!(std::fabs(nn - 1.0) <= 1e-12)) return fail(PRT_ERR_ARG, "scatter: the target's normal is a unit vector");
    for (int k = 0; k < 3; ++k) {
      args.centre[k] = target[k]; args.normal[k] = target[3 + k]; args.e1[k] = target[6 + k]; args.e2[k] = target[9 + k];
    }
    args.radius = target[12];
    args.four_r2 = 4.0 * (target[12] * target[12]);
    args.toward = 1;
  }
  args.rays_per_group = rays_per_group > 0 ? rays_per_group : 0.0;
  args.min_intensity = min_intensity; args.ray_offset = ray_offset; args.n_children = (double)rays_per_hit;
  args.key[0] = (uint32_t)seed; args.key[1] = (uint32_t)(seed >> 32);
  args.n_surfaces = n_surfaces; args.n_groups = n_groups; args.rays_per_hit = rays_per_hit;
  keep.magic = kScatterMagic; keep.n_rows = n_rows;
  for (int k = 0; k < SCATTER_RECORD; ++k) record_out[k] = 0;
  for (int b = 0; b < n_buckets; ++b) bucket_count_out[b] = 0;
  if (!n_rows) return PRT_OK;
  int rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const ScatterWork w = scatter_carve(workspace, n_items, n_buckets, n_models);
  const SortPlan plan = ghost_plan(n_items, n_buckets);
  HIP_TRY(hipMemsetAsync(w.words, 0, GHOST_STRIPES * sizeof(GhostWords) + GHOST_HEAD * 8, st));  // (and the head)
  HIP_TRY(hipMemsetAsync(w.counts, 0, plan.count_bytes, st));
  HIP_TRY(hipMemcpyAsync(w.keep, &keep, sizeof(keep), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.surfaces, listed.data(), listed.size() * sizeof(SensSurface), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.tables, tables, (size_t)n_models * (SCATTER_KNOTS + 1) * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_scatter_mark, dim3((unsigned)((n_items + kFresnelBlock - 1) / kFresnelBlock)), dim3(kFresnelBlock), 0,
                     st, rows, ld, n_items, args, w.surfaces, w.tables, w.words, w.mark);
  hipLaunchKernelGGL(k_ghost_tally, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, w.mark, n_items, plan.per_wave, n_buckets,
                     w.counts);
  hipLaunchKernelGGL(k_sort_offsets, dim3((unsigned)n_buckets), dim3(kSortScanBlock), 0, st, (int)plan.all_waves, n_buckets,
                     w.counts, w.bucket_total);
  hipLaunchKernelGGL(k_ghost_groups, dim3(1), dim3(kSortScanBlock), 0, st, n_buckets, n_items, w.bucket_total,
                     w.bucket_start, w.group_of, w.head);
  GhostWords stripes[GHOST_STRIPES], host_words = {};
  int64_t head[GHOST_HEAD];
  HIP_TRY(hipMemcpyAsync(stripes, w.words, sizeof(stripes), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(head, w.head, sizeof(head), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(bucket_count_out, w.bucket_total, (size_t)n_buckets * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (the host copies above are read by then: keep, listed)
  HIP_TRY(hipGetLastError());
  for (const GhostWords& stripe : stripes) {
    host_words.status |= stripe.status;
    for (int k = 0; k < SCATTER_COUNTERS; ++k) host_words.count[k] += stripe.count[k];
  }
  rc = PRT_OK;
  if (host_words.status & SCATTER_BAD_ID)
    rc = fail(PRT_ERR_ARG, "scatter: an id or a generation of a row on a listed surface is not an integer >= 0");
  else if (host_words.status & SCATTER_BAD_GROUP)
    rc = fail(PRT_ERR_ARG, "scatter: a ray's group, floor(id / rays_per_group), is not below n_groups");
  if (rc) {
    for (int b = 0; b < n_buckets; ++b) bucket_count_out[b] = 0;
    return rc;
  }
  for (int k = 0; k < SCATTER_COUNTERS; ++k) record_out[k] = (int64_t)host_words.count[k];
  record_out[6] = head[GHOST_HEAD_GROUPS];
  record_out[7] = head[GHOST_HEAD_STRIDE];
  return PRT_OK;
}

extern "C" int64_t prt_frame_scatter_emit_workspace_bytes(int64_t n_rows, int rays_per_hit, int n_buckets) {
  if (!scatter_sizes_ok(n_rows, rays_per_hit, n_buckets, 1)) return PRT_ERR_ARG;
  return (int64_t)ghost_plan(n_rows * rays_per_hit, n_buckets).count_bytes + 64;
}

extern "C" int prt_frame_scatter_emit(int device, const double* rows, int64_t ld, int64_t n_rows, int rays_per_hit,
                                      int n_buckets, int n_models, int64_t n_children, const void* count_workspace,
                                      double* rays_out, int64_t ld_rays, int64_t* parent_row_out, int* child_out,
                                      void* workspace, void* stream) {
  if (!scatter_sizes_ok(n_rows, rays_per_hit, n_buckets, n_models) || ld < n_rows || n_children < 0 || ld_rays < n_children ||
      !workspace || !count_workspace || (n_rows && !rows) || (n_children && (!rays_out || !parent_row_out || !child_out)))
    return fail(PRT_ERR_ARG, "bad buffers");
  if (!n_rows) return n_children ? fail(PRT_ERR_ARG, "scatter: n_children is not what the count found") : PRT_OK;
  int rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_items = n_rows * rays_per_hit;
  const ScatterWork w = scatter_carve(const_cast<void*>(count_workspace), n_items, n_buckets, n_models);
  int64_t head[GHOST_HEAD];
  ScatterKeep keep;
  HIP_TRY(hipMemcpyAsync(head, w.head, sizeof(head), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&keep, w.keep, sizeof(keep), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (keep.magic != kScatterMagic || keep.n_rows != n_rows || keep.args.rays_per_hit != rays_per_hit ||
      keep.args.n_surfaces < 1 || keep.args.n_surfaces > GHOST_MAX_SURFACES ||
      (int64_t)keep.args.n_surfaces * keep.args.n_groups != n_buckets || head[GHOST_HEAD_MAGIC] != kGhostMagic ||
      head[GHOST_HEAD_ROWS] != n_items || head[GHOST_HEAD_BUCKETS] != n_buckets)
    return fail(PRT_ERR_ARG, "scatter: count_workspace is not that of a count of this frame");
  for (int k = 0; k < keep.args.n_surfaces; ++k)
    if (keep.args.model[k] < 0 || keep.args.model[k] >= n_models)
      return fail(PRT_ERR_ARG, "scatter: count_workspace is not that of a count of this frame");
  if (head[GHOST_HEAD_CHILDREN] != n_children) return fail(PRT_ERR_ARG, "scatter: n_children is not what the count found");
  if (!n_children) return PRT_OK;
  const SortPlan plan = ghost_plan(n_items, n_buckets);
  int64_t* offsets = (int64_t*)(((uintptr_t)workspace + 63) & ~(uintptr_t)63);
  // (the scatter advances the waves' offsets: on a copy, so that the count's workspace serves another emit)
  HIP_TRY(hipMemcpyAsync(offsets, w.counts, plan.count_bytes, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_scatter_emit, dim3(plan.grid), dim3(PRT_BLOCK), 0, st, rows, ld, n_items, keep.args, w.surfaces,
                     w.tables, plan.per_wave, n_buckets, w.mark, offsets, w.bucket_start, w.group_of, w.head, n_children,
                     ld_rays, rays_out, parent_row_out, child_out);
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return PRT_OK;
}
