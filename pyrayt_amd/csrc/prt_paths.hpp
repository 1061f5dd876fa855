// prt_paths.hpp -- ray-path analysis of the frame, on the device: every ray's ordered sequence
// of surfaces put into a tree of prefixes, the rays and the energy through every node, ended there and absorbed there,
// per source group.  It is the third use of the join by ray id (k_frame_optical_path, k_aberration_table) and the most
// general one.  Definitions: include/prt.h.
//
//   k_paths_weight_max  the largest valid weight: one integer atomic max on the double's bits per workgroup
//   k_paths_step        one launch per generation, in generation order on one stream.  Per id: the generation that
//                       wrote it last + 1 (an atomic exchange, which also finds a repeated id and a missing generation),
//                       the slot of its node, its last row.  The tree is an open-addressing table of 64-bit keys
//                       (parent slot + 1, surface); a node's device-side name is the slot its key landed in, so an
//                       insert is one compare-and-swap and nothing is published after it: nobody waits for anybody.
//                       A wave loops over the distinct keys of its 64 rows (the leader probes, the slot is broadcast)
//                       and over the groups under a key; the rows and the scaled weights per (group, slot) are summed
//                       across the wave, held while the next slice of rows names the same cell, merged across the
//                       workgroup's waves, and added with 64-bit integer atomics
//   k_paths_end         over the ids: a ray with rows ended at its node; rays, dark rays and scaled weight of the last
//                       row per (group, slot), aggregated in the same way
//   (host)              the nodes' keys, in the order they were made, read back (12 bytes a node); parent, surface and
//                       depth rebuilt; the canonical order by a depth-first walk with children in ascending surface;
//                       subtree sizes; the slot -> node table
//   k_paths_remap       row_node_out and ray_node_out through the table; the per-slot tallies gathered into the
//                       (n_groups, max_paths, .) outputs; the integer energies converted to doubles, once
// Every loop has a bound known at launch (the probe: the table's capacity; the key and group loops: 64 turns), no wave
// reads a word that it waits for another wave to write, and every sum that reaches an output is an integer sum: the
// outputs are the same bits on every run and under any order of the rows inside a generation.
#pragma once

enum { PATHS_BAD_SURFACE = JOIN_OWN_BIT, PATHS_OVERFLOW = JOIN_OWN_BIT << 1 };  // (after the join's bits, prt_join.hpp)
enum { PATHS_MAX_PATHS = 65536, PATHS_TALLIES = 5 };  // tallies: through, energy through, ended, dark, energy ended
static const int kPathsBlock = 256;
static const int kPathsWaves = kPathsBlock / 64;
static const int64_t kPathsGrid = 512;                // workgroups a row pass aims at: fewer same-word atomics
static const size_t kPathsTableBytes = 256u << 20;    // cap on the per-(group, slot) tallies
static const u64 kPathsEmpty = ~0ull;                 // (no key: a surface is below 2^31)

struct PathsWords { u64 w_max, bad_weight, rays; int status, nodes; };  // (cleared together, read back together)
struct PathsHeld { long long cell; u64 a, b, c; };                      // tallies of one (group, slot), wave-uniform

// the table's capacity: the power of two that is at least 4 * max_paths
static int paths_capacity_bits(int max_paths) {
  int bits = 6;
  while (((int64_t)1 << bits) < 4 * (int64_t)max_paths) ++bits;
  return bits;
}

__device__ __forceinline__ int paths_shift(const PathsWords* __restrict__ words, int weight_column, int64_t n_rows) {
  // (without a weight column every weight is 1)
  return energy_shift(weight_column >= 0 ? words->w_max : 0x3ff0000000000000ull, (long long)(n_rows > 0 ? n_rows : 1));
}

// the weight of row j and whether it counts (finite and >= 0)
__device__ __forceinline__ double paths_weight(const double* __restrict__ rows, int64_t ld, int64_t j, int weight_column,
                                               bool& valid) {
  const double w = weight_column >= 0 ? rows[(int64_t)weight_column * ld + j] : 1.0;
  valid = w >= 0.0 && w < PRT_INF;
  return valid ? w : 0.0;
}

// the sum of v over the wave, in every lane (integers: the same in any order)
__device__ __forceinline__ u64 paths_wave_sum(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ void paths_flush(const PathsHeld& h, u64* __restrict__ ta, u64* __restrict__ tb,
                                            u64* __restrict__ tc) {
  if (h.cell < 0) return;
  if (h.a) atomicAdd(ta + h.cell, h.a);
  if (h.b) atomicAdd(tb + h.cell, h.b);
  if (tc && h.c) atomicAdd(tc + h.cell, h.c);
}

// add to the held cell, writing it out first when another cell comes (`writer`: the one lane that owns the atomics)
__device__ __forceinline__ void paths_hold(PathsHeld& h, long long cell, u64 a, u64 b, u64 c, u64* __restrict__ ta,
                                           u64* __restrict__ tb, u64* __restrict__ tc, bool writer) {
  if (cell != h.cell) {
    if (writer) paths_flush(h, ta, tb, tc);
    h.cell = cell;
    h.a = h.b = h.c = 0;
  }
  h.a += a;
  h.b += b;
  h.c += c;
}

// the waves' held cells merged in wave order and written out: one set of atomics per workgroup when they agree
__device__ __forceinline__ void paths_merge(const PathsHeld& held, PathsHeld* merge, u64* __restrict__ ta,
                                            u64* __restrict__ tb, u64* __restrict__ tc) {
  if ((threadIdx.x & 63) == 0) merge[threadIdx.x >> 6] = held;
  __syncthreads();
  if (threadIdx.x != 0) return;
  PathsHeld all = {-1, 0, 0, 0};
  for (int w = 0; w < kPathsWaves; ++w) paths_hold(all, merge[w].cell, merge[w].a, merge[w].b, merge[w].c, ta, tb, tc, true);
  paths_flush(all, ta, tb, tc);
}

// the slot of `key`, inserted if it is new; -1 (and the overflow bit) past max_paths nodes or once round the table
__device__ __forceinline__ int paths_insert(u64* __restrict__ keys, int capacity, int hash_shift, u64 key, int max_paths,
                                            PathsWords* __restrict__ words, u64* __restrict__ node_key,
                                            int* __restrict__ node_slot) {
  unsigned slot = (unsigned)((key * 0x9e3779b97f4a7c15ull) >> hash_shift);
  for (int probe = 0; probe < capacity; ++probe) {
    u64 seen = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == kPathsEmpty) {
      seen = atomicCAS(keys + slot, kPathsEmpty, key);
      if (seen == kPathsEmpty) {  // (this lane made the node: it numbers it, for the host's walk)
        const int n = atomicAdd(&words->nodes, 1);
        if (n >= max_paths) break;
        node_key[n] = key;
        node_slot[n] = (int)slot;
        return (int)slot;
      }
    }
    if (seen == key) return (int)slot;
    slot = (slot + 1) & (unsigned)(capacity - 1);
  }
  atomicOr(&words->status, PATHS_OVERFLOW);
  return -1;
}

__global__ void __launch_bounds__(kPathsBlock)
k_paths_weight_max(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int weight_column,
                   PathsWords* __restrict__ words) {
  __shared__ u64 red[kPathsWaves];
  u64 top = 0;
  for (int64_t j = (int64_t)blockIdx.x * kPathsBlock + threadIdx.x; j < n_rows; j += (int64_t)gridDim.x * kPathsBlock) {
    bool valid;
    const u64 bits = (u64)__double_as_longlong(paths_weight(rows, ld, j, weight_column, valid));
    top = bits > top ? bits : top;  // (weights are >= 0: the order of their bit images is their own)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = __shfl_xor(top, off);
    top = o > top ? o : top;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = top;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kPathsWaves; ++w) top = red[w] > top ? red[w] : top;
    if (top) atomicMax(&words->w_max, top);
  }
}

__global__ void __launch_bounds__(kPathsBlock)
k_paths_step(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t start, int64_t count, int generation,
             double id0, int64_t n_ids, double rays_per_source, int n_groups, int weight_column, int64_t per_wave,
             u64* __restrict__ keys, int capacity, int hash_shift, int max_paths, PathsWords* __restrict__ words,
             u64* __restrict__ node_key, int* __restrict__ node_slot, int* __restrict__ stamp, int* __restrict__ node_of,
             int64_t* __restrict__ last_row, int* __restrict__ row_node, u64* __restrict__ through,
             u64* __restrict__ energy_through) {
  __shared__ PathsHeld merge[kPathsWaves];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kPathsWaves + (threadIdx.x >> 6);
  const int64_t first = start + wave * per_wave;
  const int64_t last = first + per_wave < start + count ? first + per_wave : start + count;
  const int shift = paths_shift(words, weight_column, n_rows);
  PathsHeld held = {-1, 0, 0, 0};
  u64 held_key = kPathsEmpty, bad_weights = 0;
  int held_slot = -1;
  for (int64_t base = first; base < last; base += 64) {
    const int64_t j = base + lane;
    const bool live = j < last;
    u64 key = kPathsEmpty, q = 0;
    int group = -1;
    int64_t i = -1;
    bool weight_ok = true;
    if (live) {
      const int64_t id = join_id(rows, ld, j, id0, n_ids);
      const double s = rows[PRT_COL_SURFACE * ld + j];
      const bool surface_ok = s >= 0.0 && s < 2147483648.0 && s == floor(s);
      if (id < 0) atomicOr(&words->status, JOIN_BAD_ID);
      if (!surface_ok) atomicOr(&words->status, PATHS_BAD_SURFACE);
      if (id >= 0 && surface_ok) {  // (an id is claimed only by a row whose surface is good too)
        i = id;
        // (the stamp: the generation that wrote node_of[i] last, + 1)
        const int bits = join_status(join_claim(stamp, i, generation), generation);
        int parent = -1;
        bool ok = !bits;
        if (bits) atomicOr(&words->status, bits);
        if (ok && generation > 0) {
          parent = node_of[i];
          ok = parent >= 0 && parent < capacity;  // (-1: its node overflowed)
        }
        if (ok) key = ((u64)(unsigned)(parent + 1) << 32) | (u64)(unsigned)(int)s;
        last_row[i] = j;
      }
      q = energy_quantum(paths_weight(rows, ld, j, weight_column, weight_ok), shift);
      group = wf_group(rows, ld, j, rays_per_source, n_groups);
    }
    bad_weights += __popcll(__ballot(!weight_ok));
    int my_slot = -1;
    unsigned long long pending = __ballot(key != kPathsEmpty);
    for (int turn = 0; turn < 64 && pending; ++turn) {  // one turn per distinct key of the slice: very few
      const int leader = __ffsll((long long)pending) - 1;
      const u64 k = __shfl(key, leader);
      const bool mine = key == k;
      pending &= ~__ballot(mine);
      if (k != held_key) {
        int slot = -1;
        if (lane == leader) slot = paths_insert(keys, capacity, hash_shift, k, max_paths, words, node_key, node_slot);
        held_slot = __shfl(slot, leader);
        held_key = k;
      }
      const int slot = held_slot;
      if (mine) my_slot = slot;
      if (slot < 0) continue;
      unsigned long long grouped = __ballot(mine && group >= 0);
      for (int inner = 0; inner < 64 && grouped; ++inner) {  // one turn per group under the key
        const int g = __shfl(group, __ffsll((long long)grouped) - 1);
        const bool same = mine && group == g;
        const unsigned long long take = __ballot(same);
        const u64 sum = paths_wave_sum(same ? q : 0ull);
        paths_hold(held, (long long)g * capacity + slot, (u64)__popcll(take), sum, 0, through, energy_through, nullptr,
                   lane == 0);
        grouped &= ~take;
      }
    }
    if (live) row_node[j] = my_slot;
    if (i >= 0) node_of[i] = my_slot;
  }
  if (lane == 0 && bad_weights) atomicAdd(&words->bad_weight, bad_weights);
  paths_merge(held, merge, through, energy_through, nullptr);
}

__global__ void __launch_bounds__(kPathsBlock)
k_paths_end(const double* __restrict__ rows, int64_t ld, int64_t n_rows, int64_t n_ids, double rays_per_source,
            int n_groups, int weight_column, int64_t per_wave, int capacity, PathsWords* __restrict__ words,
            const int* __restrict__ stamp, const int* __restrict__ node_of, const int64_t* __restrict__ last_row,
            u64* __restrict__ ended, u64* __restrict__ dark, u64* __restrict__ energy_ended) {
  __shared__ PathsHeld merge[kPathsWaves];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kPathsWaves + (threadIdx.x >> 6);
  const int64_t first = wave * per_wave;
  const int64_t last = first + per_wave < n_ids ? first + per_wave : n_ids;
  const int shift = paths_shift(words, weight_column, n_rows);
  PathsHeld held = {-1, 0, 0, 0};
  u64 rays = 0;
  for (int64_t base = first; base < last; base += 64) {
    const int64_t i = base + lane;
    long long cell = -1;
    bool has_rows = false, is_dark = false;
    u64 q = 0;
    if (i < last && stamp[i] != 0) {
      const int slot = node_of[i];
      const int64_t j = last_row[i];
      has_rows = true;
      if (slot >= 0 && slot < capacity && j >= 0 && j < n_rows) {
        const int group = wf_group(rows, ld, j, rays_per_source, n_groups);
        if (group >= 0) cell = (long long)group * capacity + slot;
        const double tx = rows[PRT_COL_XTILT * ld + j], ty = rows[PRT_COL_YTILT * ld + j], tz = rows[PRT_COL_ZTILT * ld + j];
        is_dark = sqrt(tx * tx + ty * ty + tz * tz) <= 1e-8;  // (_pyrayt.py:415: np.isclose's absolute tolerance)
        bool weight_ok;
        q = energy_quantum(paths_weight(rows, ld, j, weight_column, weight_ok), shift);
      }
    }
    rays += __popcll(__ballot(has_rows));
    unsigned long long pending = __ballot(cell >= 0);
    for (int turn = 0; turn < 64 && pending; ++turn) {  // one turn per distinct (group, node) of the slice
      const long long c = __shfl(cell, __ffsll((long long)pending) - 1);
      const bool same = cell == c;
      const unsigned long long take = __ballot(same);
      const u64 sum = paths_wave_sum(same ? q : 0ull);
      paths_hold(held, c, (u64)__popcll(take), (u64)__popcll(__ballot(same && is_dark)), sum, ended, dark, energy_ended,
                 lane == 0);
      pending &= ~take;
    }
  }
  if (lane == 0 && rays) atomicAdd(&words->rays, rays);
  paths_merge(held, merge, ended, dark, energy_ended);
}

// items: the rows, the ids, then the (group, node) cells of the outputs
__global__ void __launch_bounds__(PRT_BLOCK)
k_paths_remap(int64_t n_rows, int64_t n_ids, int n_groups, int max_paths, int n_nodes, int capacity, int weight_column,
              const PathsWords* __restrict__ words, const int* __restrict__ lut, const int* __restrict__ slot_of,
              const u64* __restrict__ tallies, int* __restrict__ row_node, int* __restrict__ ray_node,
              int64_t* __restrict__ count_out, double* __restrict__ energy_out) {
  int64_t item = (int64_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
  if (item < n_rows + n_ids) {
    int* const at = item < n_rows ? row_node + item : ray_node + (item - n_rows);
    const int slot = *at;
    *at = slot >= 0 && slot < capacity ? lut[slot] : -1;
    return;
  }
  item -= n_rows + n_ids;
  if (item >= (int64_t)n_groups * max_paths) return;
  const int64_t g = item / max_paths;
  const int node = (int)(item - g * max_paths);
  u64 v[PATHS_TALLIES] = {0, 0, 0, 0, 0};
  if (node < n_nodes) {
    const int slot = slot_of[node];
    if (slot >= 0 && slot < capacity) {
      const size_t plane = (size_t)n_groups * capacity, cell = (size_t)g * capacity + slot;
#pragma unroll
      for (int k = 0; k < PATHS_TALLIES; ++k) v[k] = tallies[k * plane + cell];
    }
  }
  const int shift = paths_shift(words, weight_column, n_rows);
  count_out[item * 3] = (int64_t)v[0];
  count_out[item * 3 + 1] = (int64_t)v[2];
  count_out[item * 3 + 2] = (int64_t)v[3];
  energy_out[item * 2] = ldexp((double)v[1], -shift);
  energy_out[item * 2 + 1] = ldexp((double)v[4], -shift);
}

// ---- entry points ---------------------------------------------------------------------------------------------------
static bool paths_sizes_ok(int64_t n_rows, int64_t n_ids, int n_groups, int max_paths) {
  if (n_rows < 0 || n_groups < 1 || max_paths < 1 || max_paths > PATHS_MAX_PATHS) return false;
  if (!join_n_ids_ok(n_ids)) return false;
  return ((size_t)n_groups << paths_capacity_bits(max_paths)) * PATHS_TALLIES * 8 <= kPathsTableBytes;
}

extern "C" int64_t prt_frame_paths_workspace_bytes(int64_t n_rows, int64_t n_ids, int n_groups, int max_paths) {
  if (!paths_sizes_ok(n_rows, n_ids, n_groups, max_paths)) return PRT_ERR_ARG;
  const int64_t capacity = (int64_t)1 << paths_capacity_bits(max_paths);
  // the words; the table's keys; the tallies per (group, slot); the nodes' keys and slots in the order they were made;
  // the slot -> node table and its inverse; the stamp per id
  return 64 + capacity * 8 + (int64_t)n_groups * capacity * PATHS_TALLIES * 8 + (int64_t)max_paths * (8 + 4 + 4) +
         capacity * 4 + n_ids * 4 + 64;
}

extern "C" int prt_frame_paths(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                               int n_generations, double id0, int64_t n_ids, double rays_per_source, int n_groups,
                               int weight_column, int max_paths, int32_t* row_node_out, int32_t* ray_node_out,
                               int64_t* ray_last_row_out, int32_t* node_out, int64_t* count_out, double* energy_out,
                               int64_t* record_out, void* workspace, void* stream) {
  // (everything is checked before a device is touched)
  const int64_t n_rows = join_rows(rows_per_generation, n_generations, ld);
  if (n_rows < 0) return (int)n_rows;
  if (n_groups < 1 || !ray_node_out || !ray_last_row_out || !node_out || !count_out || !energy_out ||
      !record_out || !workspace || (n_rows && (!rows || !row_node_out)))
    return fail(PRT_ERR_ARG, "bad buffers");
  int rc = join_ids(id0, n_ids);
  if (rc) return rc;
  if (!(rays_per_source > 0) && n_groups != 1) return fail(PRT_ERR_ARG, "one group without rays_per_source");
  if (weight_column < -1 || weight_column >= PRT_RECORD_COLS) return fail(PRT_ERR_ARG, "weight_column: 0..14 or -1");
  if (max_paths < 1 || max_paths > PATHS_MAX_PATHS) return fail(PRT_ERR_ARG, "paths: max_paths in [1, 65536]");
  if (!paths_sizes_ok(n_rows, n_ids, n_groups, max_paths))
    return fail(PRT_ERR_ARG, "paths: n_groups * table capacity * 40 bytes above the 256 MiB table cap");
  const int bits = paths_capacity_bits(max_paths), capacity = 1 << bits;
  const int64_t items = n_rows + n_ids + (int64_t)n_groups * max_paths;
  if ((items + PRT_BLOCK - 1) / PRT_BLOCK > 0x7fffffff) return fail(PRT_ERR_ARG, "paths: too many rows for one launch");
  rc = ops_device(device);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the workspace (prt_frame_paths_workspace_bytes)
  PathsWords* words = (PathsWords*)(((uintptr_t)workspace + 63) & ~(uintptr_t)63);
  u64* keys = (u64*)((char*)words + 64);
  u64* tallies = keys + capacity;
  const size_t plane = (size_t)n_groups * capacity;
  u64* node_key = tallies + PATHS_TALLIES * plane;
  int* node_slot = (int*)(node_key + max_paths);
  int* slot_of = node_slot + max_paths;
  int* lut = slot_of + max_paths;
  int* stamp = lut + capacity;
  HIP_TRY(hipMemsetAsync(words, 0, 64, st));
  HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)capacity * 8, st));
  HIP_TRY(hipMemsetAsync(tallies, 0, PATHS_TALLIES * plane * 8, st));
  HIP_TRY(hipMemsetAsync(stamp, 0, (size_t)n_ids * 4, st));
  HIP_TRY(hipMemsetAsync(ray_node_out, 0xff, (size_t)n_ids * 4, st));
  HIP_TRY(hipMemsetAsync(ray_last_row_out, 0xff, (size_t)n_ids * 8, st));
  HIP_TRY(hipMemsetAsync(node_out, 0xff, (size_t)max_paths * 4 * 4, st));
  // a wave takes a contiguous run of 64-row slices: the workgroups of a launch stay near kPathsGrid
  const auto run = [](int64_t n) { return std::max<int64_t>(1, (n + kPathsGrid * kPathsBlock - 1) / (kPathsGrid * kPathsBlock)) * 64; };
  const auto grid = [](int64_t n, int64_t per_wave) { return (unsigned)((n + per_wave * kPathsWaves - 1) / (per_wave * kPathsWaves)); };
  if (n_rows && weight_column >= 0)
    hipLaunchKernelGGL(k_paths_weight_max, dim3((unsigned)std::min<int64_t>((n_rows + kPathsBlock - 1) / kPathsBlock, 1024)),
                       dim3(kPathsBlock), 0, st, rows, ld, n_rows, weight_column, words);
  int64_t start = 0;
  for (int g = 0; g < n_generations; ++g) {
    const int64_t count = rows_per_generation[g];
    if (count) {
      const int64_t per_wave = run(count);
      hipLaunchKernelGGL(k_paths_step, dim3(grid(count, per_wave)), dim3(kPathsBlock), 0, st, rows, ld, n_rows, start,
                         count, g, id0, n_ids, rays_per_source, n_groups, weight_column, per_wave, keys, capacity,
                         64 - bits, max_paths, words, node_key, node_slot, stamp, ray_node_out, ray_last_row_out,
                         row_node_out, tallies, tallies + plane);
    }
    start += count;
  }
  if (n_rows) {
    const int64_t per_wave = run(n_ids);
    hipLaunchKernelGGL(k_paths_end, dim3(grid(n_ids, per_wave)), dim3(kPathsBlock), 0, st, rows, ld, n_rows, n_ids,
                       rays_per_source, n_groups, weight_column, per_wave, capacity, words, stamp, ray_node_out,
                       ray_last_row_out, tallies + 2 * plane, tallies + 3 * plane, tallies + 4 * plane);
  }
  PathsWords host_words;
  HIP_TRY(hipMemcpyAsync(&host_words, words, sizeof(PathsWords), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  const int status = host_words.status;
  if (!(status & JOIN_BAD_ID) && (status & PATHS_BAD_SURFACE))  // (a bad id first, a bad surface before the join's others)
    return fail(PRT_ERR_ARG, "paths: a surface is not an integer in [0, 2^31)");
  rc = join_refusal(status, "paths");
  if (rc) return rc;
  if ((status & PATHS_OVERFLOW) || host_words.nodes > max_paths || host_words.nodes < 0)
    return fail(PRT_ERR_ARG, "paths: more than max_paths = " + std::to_string(max_paths) + " distinct nodes");
  // the nodes in the order they were made: a parent comes before its children (the generations ran in order)
  const int n_nodes = host_words.nodes;
  std::vector<u64> made_key((size_t)n_nodes);
  std::vector<int> made_slot((size_t)n_nodes), parent((size_t)n_nodes), depth((size_t)n_nodes), order, number((size_t)n_nodes);
  if (n_nodes) {
    HIP_TRY(hipMemcpyAsync(made_key.data(), node_key, (size_t)n_nodes * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(made_slot.data(), node_slot, (size_t)n_nodes * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  std::vector<int> host_lut((size_t)capacity, -1);  // (slot -> the order made, then slot -> node)
  for (int n = 0; n < n_nodes; ++n) {
    if (made_slot[n] < 0 || made_slot[n] >= capacity) return fail(PRT_ERR_HIP, "paths: a node's slot is out of range");
    host_lut[made_slot[n]] = n;
  }
  std::vector<std::vector<int>> children((size_t)n_nodes + 1);  // (the last: the first surfaces)
  int deepest = 0;
  for (int n = 0; n < n_nodes; ++n) {
    const int64_t parent_slot = (int64_t)(made_key[n] >> 32) - 1;
    parent[n] = parent_slot < 0 ? -1 : (parent_slot < capacity ? host_lut[parent_slot] : n);
    if (parent[n] >= n) return fail(PRT_ERR_HIP, "paths: a node came before its parent");
    depth[n] = parent[n] < 0 ? 0 : depth[parent[n]] + 1;
    deepest = std::max(deepest, depth[n] + 1);
    children[parent[n] < 0 ? n_nodes : parent[n]].push_back(n);
  }
  const auto surface_of = [&](int n) { return (int64_t)(made_key[n] & 0xffffffffull); };
  for (auto& c : children) std::sort(c.begin(), c.end(), [&](int a, int b) { return surface_of(a) > surface_of(b); });
  // depth-first, children in ascending surface (pushed descending): the order of the sequences compared as tuples
  order.reserve((size_t)n_nodes);
  std::vector<int> stack(children[n_nodes]);
  while (!stack.empty()) {
    const int n = stack.back();
    stack.pop_back();
    number[n] = (int)order.size();
    order.push_back(n);
    for (int c : children[n]) stack.push_back(c);
  }
  if ((int)order.size() != n_nodes) return fail(PRT_ERR_HIP, "paths: the nodes do not make a tree");
  std::vector<int32_t> table((size_t)n_nodes * 4);
  std::vector<int> host_slot_of((size_t)n_nodes);
  for (int k = n_nodes - 1; k >= 0; --k) {  // (descendants have larger numbers: their sizes are complete)
    const int n = order[k];
    table[4 * (size_t)k] = parent[n] < 0 ? -1 : number[parent[n]];
    table[4 * (size_t)k + 1] = (int32_t)surface_of(n);
    table[4 * (size_t)k + 2] = depth[n];
    table[4 * (size_t)k + 3] += 1;
    if (parent[n] >= 0) table[4 * (size_t)number[parent[n]] + 3] += table[4 * (size_t)k + 3];
    host_slot_of[k] = made_slot[n];
  }
  for (int n = 0; n < n_nodes; ++n) host_lut[made_slot[n]] = number[n];
  HIP_TRY(hipMemcpyAsync(lut, host_lut.data(), (size_t)capacity * 4, hipMemcpyHostToDevice, st));
  if (n_nodes) {
    HIP_TRY(hipMemcpyAsync(slot_of, host_slot_of.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(node_out, table.data(), (size_t)n_nodes * 16, hipMemcpyHostToDevice, st));
  }
  hipLaunchKernelGGL(k_paths_remap, dim3((unsigned)((items + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0, st, n_rows,
                     n_ids, n_groups, max_paths, n_nodes, capacity, weight_column, words, lut, slot_of, tallies,
                     row_node_out, ray_node_out, count_out, energy_out);
  HIP_TRY(hipStreamSynchronize(st));  // (the host tables outlive their copies)
  HIP_TRY(hipGetLastError());
  record_out[0] = n_nodes;
  record_out[1] = (int64_t)host_words.rays;
  record_out[2] = (int64_t)host_words.bad_weight;
  record_out[3] = deepest;
  return PRT_OK;
}
