// prt_join.hpp -- the join by ray id that the frame passes share: a row finds its ray's state in
// dense per-id arrays through k = id - id0, and a pass that runs one launch per generation, in order, keeps per id a
// stamp: the generation that wrote the ray's state last, + 1 (0: none yet).  Exchanging the stamp tells a row whether
// the ray's state is the previous generation's, and finds an id that repeats within a generation and a ray with a row
// in a generation and none in the one before.  Each pass reports the bits in its own word and keeps its own rules:
// k_frame_optical_path restarts its sum where a generation is missing, k_paths_step claims an id only when the row's
// surface is good too, k_aberration_table / k_aberration_gather use the id check alone.
#pragma once

// the shared bits of a pass's status word; a pass's own bits go from JOIN_OWN_BIT up
enum { JOIN_BAD_ID = 1, JOIN_REPEATED_ID = 2, JOIN_NOT_WHOLE = 4, JOIN_OWN_BIT = 8 };

// row j's id as an index in [0, n_ids), or -1
__device__ __forceinline__ int64_t join_id(const double* __restrict__ rows, int64_t ld, int64_t j, double id0,
                                           int64_t n_ids) {
  const double k = rows[PRT_COL_ID * ld + j] - id0;
  return k >= 0.0 && k < (double)n_ids && k == floor(k) ? (int64_t)k : -1;
}

// id i claimed for `generation`: the stamp that was there
__device__ __forceinline__ int join_claim(int* __restrict__ stamp, int64_t i, int generation) {
  return atomicExch(stamp + i, generation + 1);
}

// what that stamp says: 0 when the ray's state is that of generation - 1 (at generation 0: untouched)
__device__ __forceinline__ int join_status(int before, int generation) {
  return before == generation ? 0 : before == generation + 1 ? JOIN_REPEATED_ID : JOIN_NOT_WHOLE;
}

// ---- host side: the arguments every joined pass takes, and the shared refusals -------------------------------------------
static bool join_n_ids_ok(int64_t n_ids) { return n_ids >= 1 && n_ids <= ((int64_t)1 << 31); }

// the rows of a frame given by generation: their number, or PRT_ERR_ARG with the message set.  block: the rows a
// workgroup takes in a pass that launches one grid per generation and refuses (as `pass`) what one grid cannot hold;
// 0 in a pass without that bound
static int64_t join_rows(const int64_t* rows_per_generation, int n_generations, int64_t ld, int block = 0,
                         const char* pass = "") {
  if (n_generations < 0 || (n_generations && !rows_per_generation) || ld < 0) return fail(PRT_ERR_ARG, "bad buffers");
  int64_t n_rows = 0;
  for (int g = 0; g < n_generations; ++g) {
    if (rows_per_generation[g] < 0) return fail(PRT_ERR_ARG, "rows_per_generation: counts >= 0");
    if (block && (rows_per_generation[g] + block - 1) / block > 0x7fffffff)
      return fail(PRT_ERR_ARG, std::string(pass) + ": too many rows in a generation for one launch");
    n_rows += rows_per_generation[g];
  }
  if (ld < n_rows) return fail(PRT_ERR_ARG, "bad buffers");
  return n_rows;
}

static int join_ids(double id0, int64_t n_ids) {
  if (!join_n_ids_ok(n_ids) || !(id0 == id0 && std::fabs(id0) < 9.0e15))
    return fail(PRT_ERR_ARG, "ids: n_ids in [1, 2^31], id0 finite");
  return PRT_OK;
}

// the shared bits of a status word as `pass` refuses them; PRT_OK when none is set
static int join_refusal(int status, const char* pass) {
  const std::string who = std::string(pass) + ": ";
  if (status & JOIN_BAD_ID) return fail(PRT_ERR_ARG, who + "an id is not an integer in [id0, id0 + n_ids)");
  if (status & JOIN_REPEATED_ID) return fail(PRT_ERR_ARG, who + "an id repeats within a generation");
  if (status & JOIN_NOT_WHOLE)
    return fail(PRT_ERR_ARG, who + "a ray has a row in a generation and none in the one before: the frame is not whole");
  return PRT_OK;
}
