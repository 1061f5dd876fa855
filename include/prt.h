/*
 * prt.h -- C-ABI of libprt_hip.so, the MI355X (gfx950) ray-propagation engine that sits
 * under PyRayT's RayTracer.trace() hot path.
 *
 * Every entry point is plain C: pointers, sizes, ints.  No torch / C++ types cross this
 * boundary.  Device pointers are raw HIP device addresses (e.g. torch.Tensor.data_ptr()).
 * Streams are passed as void* (a hipStream_t; NULL = the default stream).
 *
 * Each function cites the reference interface (path:line under the PyRayT tree) it replaces.
 * The reference has no FFI layer of its own (it is pure Python + numpy), so the seam is the
 * duck-typed Python interface of pyrayt/_pyrayt.py, tinygfx/g3d/world_objects.py,
 * tinygfx/g3d/csg.py and pyrayt/materials.py.  INTEGRATION.md shows the ctypes stubs a
 * maintainer would add on the reference side.
 *
 * Ownership: the caller owns every buffer.  The library copies the scene description at
 * prt_scene_create() and never retains caller pointers beyond a call (stream-ordered work
 * excepted: buffers must stay alive until the stream has drained).
 * Errors: 0 = OK, negative = error; prt_last_error() returns a thread-local message.
 * Threads: the stateless entry points (prt_reflect ... prt_generate_rays, prt_place_rows,
 * prt_frame_reduce) may be called from any thread; a prt_scene (like the reference's RayTracer,
 * _pyrayt.py:227-246, which holds its state between trace() calls) carries per-scene state between
 * calls -- trace statistics, the dense-mode hints, the host mirror the kernels publish to -- and
 * serves one caller at a time.  Concurrent traces use one scene object per host thread
 * (tools/two_stream_probe.py); a prt_comm likewise belongs to one thread.
 */
#ifndef PRT_H
#define PRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRT_VERSION 240 /* 0.2.4: prt_frame_optical_path, prt_frame_wavefront_workspace_bytes, prt_frame_wavefront; added since without a change to what was there: prt_frame_psf, prt_frame_vector_psf, prt_frame_mtf, prt_frame_launch_index, prt_frame_ray_aberrations, prt_frame_energy, prt_frame_paths, prt_frame_fresnel, prt_frame_fresnel_coated, prt_frame_sensitivity, prt_frame_design_sensitivity, prt_frame_opd_sensitivity, prt_frame_launch_sensitivity, prt_frame_mtf_gradient, prt_frame_psf_gradient, prt_frame_psf_focus and their workspace functions (prt_frame_psf_gradient_workspace_bytes and prt_frame_psf_focus_workspace_bytes among them), prt_frame_tolerance and prt_frame_tolerance_moments with theirs, prt_frame_mtf_tolerance with its own, prt_frame_energy_tolerance with its own, prt_frame_ghosts_count and prt_frame_ghosts_emit with theirs, prt_frame_scatter_count and prt_frame_scatter_emit with theirs.  0.2.3: prt_frame_range, prt_frame_histogram_workspace_bytes, prt_frame_histogram.  0.2.2: record plans (prt_record_plan, prt_trace_set_plan); per-tile records retired (PRT_TRACE_NO_TILE_RECORDS ignored, telemetry slots 8 / 9 count plan launches / misses). 0.2.1: prt_frame_mean_square, PRT_TRACE_BUSY / prt_trace_batch_busy, prt_comm_info.  0.2.0: prt_interact takes the caller-shaded state, PRT_MAT_TABLE / PRT_MAT_HOST,
                           prt_scene_set_index_tables, prt_gather_hits / prt_scatter_shaded, prt_unique_values,
                           prt_frame_stats_sharded / prt_frame_pivots / prt_frame_finish, prt_trace_telemetry fills 12 slots.  A caller built against another version must not load this library:
                           prt_version() is there to be compared with this constant (pyrayt_amd.engine.library does). */

/* ---- ray buffer layout: pyrayt/_pyrayt.py:13-144 (RaySet) -------------------------------
 * A ray set is a row-major (13, n) float64 matrix with leading dimension `ld` (elements
 * between consecutive rows, ld >= n): one contiguous row per field, i.e. SoA. */
enum {
  PRT_ROW_OX = 0, PRT_ROW_OY = 1, PRT_ROW_OZ = 2, PRT_ROW_OW = 3,
  PRT_ROW_DX = 4, PRT_ROW_DY = 5, PRT_ROW_DZ = 6, PRT_ROW_DW = 7,
  PRT_ROW_GENERATION = 8, PRT_ROW_INTENSITY = 9, PRT_ROW_WAVELENGTH = 10,
  PRT_ROW_INDEX = 11, PRT_ROW_ID = 12,
  PRT_RAY_ROWS = 13
};

/* ---- result rows: pyrayt/_pyrayt.py:154-165 (_RayTraceDataframe.df_columns) --------------
 * A record block is a row-major (15, cap) float64 matrix (one contiguous row per DataFrame
 * column) with leading dimension ld_rows. */
enum {
  PRT_COL_GENERATION = 0, PRT_COL_INTENSITY = 1, PRT_COL_WAVELENGTH = 2, PRT_COL_INDEX = 3,
  PRT_COL_ID = 4, PRT_COL_SURFACE = 5, PRT_COL_X0 = 6, PRT_COL_Y0 = 7, PRT_COL_Z0 = 8,
  PRT_COL_X1 = 9, PRT_COL_Y1 = 10, PRT_COL_Z1 = 11, PRT_COL_XTILT = 12, PRT_COL_YTILT = 13,
  PRT_COL_ZTILT = 14,
  PRT_RECORD_COLS = 15
};

/* ---- scene snapshot ---------------------------------------------------------------------- */

/* primitive kinds: tinygfx/g3d/primitives.py (Sphere :220, Cylinder :621, Plane :422,
 * Cube :501, Paraboloid :299) */
enum {
  PRT_PRIM_SPHERE = 0,     /* params: radius */
  PRT_PRIM_CYLINDER = 1,   /* params: radius, h_min, h_max */
  PRT_PRIM_PLANE = 2,      /* params: width (x), length (y) */
  PRT_PRIM_CUBE = 3,       /* params: xmin, xmax, ymin, ymax, zmin, zmax */
  PRT_PRIM_PARABOLOID = 4  /* params: focus, height */
};

/* material kinds: pyrayt/materials.py (:41 absorber, :53 mirror, :102 BasicRefractor,
 * :121 SellmeierRefractor).  PRT_MAT_NONE is a surface whose material has no trace()
 * (the reference's default GoochMaterial, world_objects.py:341): hitting it is an error. */
enum {
  PRT_MAT_NONE = 0,
  PRT_MAT_ABSORBER = 1,
  PRT_MAT_MIRROR = 2,
  PRT_MAT_CONST_INDEX = 3, /* coef[0] = n */
  PRT_MAT_SELLMEIER = 4,   /* coef = b1, b2, b3, c1, c2, c3 (wavelength in um) */
  /* The reference's extension points (pyrayt/materials.py:26-37, :88-99, docs/source/reference/materials.rst:17-19):
   * a user's Glass subclass supplies index_at(wavelength), a user's TracableMaterial subclass supplies trace(). */
  PRT_MAT_TABLE = 5,       /* a glass (Glass.trace, materials.py:70-75) whose index_at() is arbitrary host code: the
                              caller evaluates it on the distinct wavelengths of its rays and hands the library the
                              sorted (wavelength, index) pairs (prt_scene_set_index_tables); the kernels look a ray's
                              wavelength up by exact value.  coef[3] = the index for a NaN wavelength; the rest of
                              coef is owned by the library.  A wavelength that is not in the table is an error
                              (PRT_ERR_WAVELENGTH), never a guess. */
  PRT_MAT_HOST = 6         /* a material whose trace() is arbitrary host code: the caller shades the rays that hit it
                              itself (prt_gather_hits -> its trace() -> prt_scatter_shaded) and prt_interact takes
                              their post-interaction state as given.  prt_trace cannot serve such a surface: a ray
                              that hits one there is PRT_ERR_UNTRACABLE. */
};

/* CSG operations: tinygfx/g3d/csg.py:7-10 (Operation) */
enum { PRT_NODE_LEAF = 0, PRT_NODE_UNION = 1, PRT_NODE_INTERSECT = 2, PRT_NODE_DIFFERENCE = 3 };

/* one TracerSurface (world_objects.py:338-422): primitive + cached world->object matrix */
typedef struct prt_prim {
  int32_t type;          /* PRT_PRIM_* */
  int32_t material;      /* index into the material table */
  int32_t normal_scale;  /* +1 / -1: Intersectable._normal_scale (world_objects.py:305,319) */
  int32_t reserved;
  int64_t surface_id;    /* CountedObject id (world_objects.py:26-40); written to `surface` */
  double params[6];
  double minv[16];       /* row-major _object_coordinate_transform (world_objects.py:122) */
} prt_prim;

/* one node of a component tree: leaf = TracerSurface, inner = CSGSurface (csg.py:64-91) */
typedef struct prt_node {
  int32_t op;            /* PRT_NODE_* */
  int32_t left, right;   /* child node indices (inner nodes) */
  int32_t prim;          /* primitive index (leaf nodes) */
  double aabb[6];        /* inner nodes: world-space CSGSurface._aobb axis spans
                            xmin,xmax,ymin,ymax,zmin,zmax (csg.py:93-116) */
} prt_node;

typedef struct prt_material {
  int32_t kind;          /* PRT_MAT_* */
  int32_t reserved;
  double coef[6];
} prt_material;

typedef struct prt_scene prt_scene; /* opaque */

/* ---- library ------------------------------------------------------------------------------ */

int prt_version(void);
const char* prt_last_error(void);
/* number of visible HIP devices (0 if none / no driver) */
int prt_device_count(void);

/* How a scene is compiled and which kernels serve it.  Every field's zero is the default (and the
 * product's choice); the others exist for A/B measurements and for the tests, which run the parity
 * suites under each of them.  None of them changes a result.  No counterpart upstream.  The library
 * reads nothing from the environment: these options and the PRT_TRACE_* flags are all there is. */
typedef struct prt_scene_options {
  int32_t struct_size;  /* sizeof(prt_scene_options) as the caller knows it */
  int32_t no_chain;     /* 1: components run on the step interpreter, none as a register-only chain step */
  int32_t no_cull;      /* 1: no component cull steps in the trace program, no line-of-sight steps in the render program */
  int32_t cull_min;     /* components from which cull steps are compiled in (0 = the default, 3) */
  int32_t no_groups;    /* 1: no hierarchy of cull steps over groups of components */
  int32_t no_implied;   /* 1: every CSG node evaluates upstream's cull box (csg.py:126-128) exactly */
  int32_t hit_lanes;    /* nearest-hit kernel of prt_propagate and of PRT_TRACE_UNFUSED: lanes per ray,
                           0 / 1 = one ray per lane (default), 4 / 8 / 16 = surface-parallel with a
                           wavefront shuffle (t, component order) min-reduce */
  int32_t hit_staged;   /* 1: those kernels read the program from an LDS copy instead of the scalar cache */
  int32_t list_order_groups; /* 1: the cull-step hierarchy groups components in list order only (the
                           round-2 form); 0: by position in space when that is tighter */
  int32_t one_direction;     /* 1: a grouped trace program is stored once, not also in mirror image */
  int32_t no_intervals;      /* 1: chain steps whose nodes are all INTERSECT run the general CSG node algebra instead of
                                the interval form (an intersection of the leaves' [enter, exit] intervals) */
  int32_t no_clearance;      /* 1: the cylinder that cuts a lens chain to its aperture is evaluated for every wave (0: not for a
                                wave all of whose chords run inside it by a margin: a convexity argument) */
  int32_t no_plane_bound;    /* 1: a bare plane of a trace program (a detector, a baffle) evaluates its two slabs for every wave (0: only
                                for a wave in which some lane's crossing t is positive and beats its nearest hit so far: the slabs
                                can only remove that t) */
  int32_t reserved[3];
} prt_scene_options;

/* Build a scene from a snapshot.  roots[] lists the node index of every top-level component
 * in RayTracer._components order (pyrayt/_pyrayt.py:229-239); the surface look-up table of
 * _pyrayt.py:257-260 is the depth-first leaf order of those roots.  options: NULL = defaults. */
int prt_scene_create(const prt_prim* prims, int n_prims, const prt_node* nodes, int n_nodes,
                     const int32_t* roots, int n_roots, const prt_material* mats, int n_mats,
                     const prt_scene_options* options, prt_scene** out);
void prt_scene_destroy(prt_scene* scene);
/* The same components with other numbers in them -- a part moved, a radius or a glass changed: what a
 * design loop does between two RayTracer.trace() calls (examples/lens_design.ipynb; upstream simply
 * walks the mutated Python objects again, _pyrayt.py:377).  Recompiles on the host and overwrites the
 * scene's tables in place: device buffers, pinned memory, events and what the scene learnt from its
 * previous trace stay.  Returns 0, or 1 -- scene untouched -- when the snapshot does not have the old
 * one's shape (a table or program would change size): build a new scene then.  Synchronises the
 * device (the previous trace may still be reading the tables); refused while a trace is in flight.  The record plans
 * of the scene's tickets (prt_trace_set_plan) stay in force and are resolved again against the new snapshot: they
 * name surfaces by id, so after a reordered component list they still pass the rows of the same surfaces, and an id
 * the new snapshot no longer has (a part replaced by a new one) passes no row.
 * options: NULL = keep the scene's. */
int prt_scene_update(prt_scene* scene, const prt_prim* prims, int n_prims, const prt_node* nodes, int n_nodes,
                     const int32_t* roots, int n_roots, const prt_material* mats, int n_mats,
                     const prt_scene_options* options);
/* Index tables of the scene's PRT_MAT_TABLE materials (Glass.index_at of a user-defined glass,
 * pyrayt/materials.py:88-99, evaluated by the caller): material m looks wavelengths up in entries
 * [ranges[2m], ranges[2m] + ranges[2m+1]) of the two HOST arrays (`total` entries each), ascending in wavelength
 * without duplicates inside a material's range; ranges of other kinds of material are ignored.  Copied; replaces
 * the previous tables; a TABLE material without entries misses every look-up.  Synchronises the device (a trace
 * may still be reading the old tables); refused while a trace is in flight. */
int prt_scene_set_index_tables(prt_scene* scene, const int64_t* ranges, int n_mats, const double* wavelengths,
                               const double* indices, int64_t total);
/* rows of the hit list component `root` returns from intersect(): 2 * (#leaves under it) */
int prt_scene_component_rows(const prt_scene* scene, int root);
/* what the scene compiled to (no counterpart upstream; host-only, needs no GPU):
 * out10 = { primitives, components, step slots of the trace program, LDS hit-list slots per ray of the
 * trace program, component cull steps in it, steps / slots of the render program, components of the
 * trace program compiled to a single register-only chain step, 1 if the cull steps are grouped by the
 * components' position in space rather than by their place in the list, 1 if the trace program is stored
 * in both directions (waves that run against its axis take the mirror image) } */
int prt_scene_info(const prt_scene* scene, int64_t* out10);

/* ---- per-state entry points (drop-ins for the reference's Python methods) ------------------ */

/* component.intersect(rays) -> (hits (m,n) sorted ascending, inf = miss ; surface ids (m,n)):
 * TracerSurface.intersect world_objects.py:360-383, CSGSurface.intersect csg.py:118-160.
 * rays: device (8+, n) matrix, rows 0-7 used.  hits_out / ids_out: device (m, n) with leading
 * dimension ld_out, m = prt_scene_component_rows().  ids are defined where the hit is finite
 * and -1 elsewhere. */
int prt_intersect(prt_scene* scene, int device, int root, const double* rays, int64_t n,
                  int64_t ld, double* hits_out, int64_t* ids_out, int64_t ld_out, void* stream);

/* RayTracer._st_propagate (pyrayt/_pyrayt.py:370-392): nearest positive hit over all
 * components.  t_out (n) float64 (inf = no hit), surf_out (n) int64 surface id (-1 = none). */
int prt_propagate(prt_scene* scene, int device, const double* rays, int64_t n, int64_t ld,
                  double* t_out, int64_t* surf_out, void* stream);

/* TracerSurface.get_world_normals (world_objects.py:401-418) for primitive `prim`:
 * points (4,k) -> normals (4,k), both device, row-major with leading dimension ld. */
int prt_world_normals(prt_scene* scene, int device, int prim, const double* points, int64_t k,
                      int64_t ld, double* normals_out, void* stream);

/* surface.material.trace(surface, ray_set) (pyrayt/materials.py:47-50, :58-62, :70-75):
 * shades, in place, every ray of the (13,k) set as having hit primitive `prim` at its current
 * origin. */
int prt_material_trace(prt_scene* scene, int device, int prim, double* rays, int64_t k,
                       int64_t ld, void* stream);

/* RayTracer._st_interact (pyrayt/_pyrayt.py:394-452) + _RayTraceDataframe.insert (:168-186):
 * advance hit rays to their hit point, shade, drop dead rays (order preserving), append one
 * record row per live ray, set generation+1, and (unless generation+1 == generation_limit)
 * re-launch by ray_offset along the new direction.
 *   rays_in (13,n) ld_in ; t/surf from prt_propagate ; rays_out (13, >= n) ld_out
 *   rows_out (15, >= n) ld_rows ; n_live_out: device int64[1] (a negative PRT_ERR_* if the device raised one)
 *   shaded (13, n) ld_shaded, or NULL: column i holds the state of ray i as the caller's own material.trace()
 *     left it (_pyrayt.py:408-410 assigns what trace() returns to all 13 rows); read only for rays that hit a
 *     PRT_MAT_HOST surface -- origin, direction, intensity, wavelength, index and id of the next state are taken
 *     from it, the generation is set as for any ray (:437) -- and ignored elsewhere
 *   workspace: device scratch of prt_interact_workspace_bytes(n) bytes
 * If every ray is dead nothing is written and *n_live_out = 0 (_pyrayt.py:424-425). */
int64_t prt_interact_workspace_bytes(int64_t n);
int prt_interact(prt_scene* scene, int device, const double* rays_in, int64_t n, int64_t ld_in,
                 const double* t, const int64_t* surf, double* rays_out, int64_t ld_out,
                 int generation, int generation_limit, double ray_offset, double* rows_out,
                 int64_t ld_rows, int64_t* n_live_out, const double* shaded, int64_t ld_shaded,
                 void* workspace, void* stream);

/* The two halves of a host-shaded interaction (pyrayt/_pyrayt.py:401-410: `surface.material.trace(surface,
 * next_ray_set[..., surface_mask])` with a user-defined trace()).
 *   prt_gather_hits     the rays whose nearest hit (surf from prt_propagate) is `surface_id`, in ray order, all 13
 *                       rows, origins advanced to the hit point (o += d t, :404-407) -> subset_out (13, >= count)
 *                       ld_subset; index_out (>= count): their columns in `rays`; *count_out: HOST, how many
 *                       (the call synchronises the stream).  subset_out / index_out may hold n columns at most.
 *                       workspace: prt_interact_workspace_bytes(n) device bytes.
 *   prt_scatter_shaded  column j of subset (13, k) -> column index[j] of shaded (13, >= max index + 1): the block
 *                       prt_interact reads.  Stream-ordered. */
int prt_gather_hits(int device, const double* rays, int64_t n, int64_t ld, const double* t, const int64_t* surf,
                    int64_t surface_id, double* subset_out, int64_t ld_subset, int64_t* index_out,
                    int64_t* count_out, void* workspace, void* stream);
int prt_scatter_shaded(int device, const double* subset, int64_t k, int64_t ld_subset, const int64_t* index,
                       double* shaded, int64_t ld_shaded, void* stream);

/* The distinct values of a device array of doubles (the wavelength row of a ray set: what Glass.index_at of a
 * user-defined glass has to be evaluated on, pyrayt/materials.py:70-75), compared bit for bit, in no particular
 * order: out (cap) device, *count_out HOST = how many there are (the call synchronises the stream); when that
 * exceeds cap only the first cap found are in `out`.  workspace: prt_unique_workspace_bytes(cap) device bytes. */
int64_t prt_unique_workspace_bytes(int64_t cap);
int prt_unique_values(int device, const double* values, int64_t n, double* out, int64_t cap, int64_t* count_out,
                      void* workspace, void* stream);

/* ---- ray sources (next to the hot path) --------------------------
 * Source.generate_rays(n) (pyrayt/components.py:481-496): object-space pattern -> 4x4 world
 * transform -> unit directions, written straight into a device ray set so that the initial
 * RaySet never crosses PCIe.  Patterns: LineOfRays :511-530, CircleOfRays :533-558,
 * ConeOfRays :561-585, WedgeOfRays :588-613 (closed form, same arithmetic as upstream) and
 * Lamp :616-654 (upstream draws from numpy's global RNG; here a counter-based generator keyed
 * by `seed` and the ray number: same distribution, not the same stream). */
enum {
  PRT_SRC_LINE = 0,   /* params: spacing */
  PRT_SRC_CIRCLE = 1, /* params: diameter */
  PRT_SRC_CONE = 2,   /* params: half angle (radians) */
  PRT_SRC_WEDGE = 3,  /* params: full angle (radians) */
  PRT_SRC_LAMP = 4    /* params: width, length, max angle (radians) */
};
typedef struct prt_source {
  int32_t kind;      /* PRT_SRC_* */
  int32_t reserved;
  double params[4];
  double wavelength; /* um */
  double world[16];  /* row-major _world_coordinate_transform (world_objects.py:97-99) */
  uint64_t seed;     /* PRT_SRC_LAMP only */
} prt_source;

/* Write rays [first, first+count) of the n_total rays this source emits into columns
 * [col_offset, col_offset+count) of the device (13, >= col_offset+count) ray set `rays_out`
 * (leading dimension ld); ray k gets id id_first + (k - first), generation 0, index 1,
 * intensity 100 (Lamp: 100 cos(theta)). */
int prt_generate_rays(int device, const prt_source* source, int64_t n_total, int64_t first,
                      int64_t count, int64_t id_first, double* rays_out, int64_t ld,
                      int64_t col_offset, void* stream);

/* ---- the whole hot loop -------------------------------------------------------------------
 * RayTracer.trace() minus source generation and DataFrame construction
 * (pyrayt/_pyrayt.py:329-339 driving :370-452).  Runs every generation on the device.
 *   rays (13,n) ld: initial ray set (read only)
 *   rows_out (15, rows_cap) ld_rows = rows_cap: generation-major record rows
 *   rows_per_generation: HOST int64[generation_limit], rows recorded by each generation
 *   workspace: device scratch of prt_trace_workspace_bytes(n) bytes.  A scene that is traced again
 *     with the same workspace address, ray count and generation limit finds the control words in it as
 *     its previous trace left them and does not re-initialise them; the library notices when another
 *     scene traced with that address in between (then it does), but not when something else wrote
 *     there: do not hand the block to anything but prt_trace between two traces
 *   flags: PRT_TRACE_* bits
 * Returns the total number of rows (>= 0) or a negative error.  PRT_ERR_ROWS_CAP if rows_cap
 * is too small (n * generation_limit rows always suffices).
 * On return the COUNTS are on the host; the record rows and the workspace are only stream-ordered: the
 * generation kernels publish their counts to host-mapped memory themselves, and the call returns as
 * soon as it has seen them -- possibly while the last kernel is still storing rows.  Whatever consumes
 * rows_out (or frees / reuses rows_out, rays or the workspace) must run on `stream` or synchronise with
 * it first; PRT_TRACE_SYNC makes the call do that itself before it returns. */
#define PRT_TRACE_KEEP_ABSORBED 1 /* carry zero-direction (absorbed) rays into the next
                                     generation exactly like _pyrayt.py:415-428 (Q3) instead of
                                     dropping them when they are absorbed; the rows are
                                     identical either way */
#define PRT_TRACE_UNFUSED 2       /* run the generation as propagate + interact kernels */
#define PRT_TRACE_NO_HINTS 4      /* do not use the dense-mode hints of the scene's previous trace
                                     (every generation runs the general look-back path, as in a first trace) */
#define PRT_TRACE_FULL_ROWS 8     /* carry all 13 state rows between generations (see "compact state") */
#define PRT_TRACE_PUBLISH_KERNEL 16 /* counts reach the host through a one-block kernel behind each batch
                                     instead of from inside the generation kernels (A/B, tests) */
#define PRT_TRACE_TEST_STALL 32   /* test hook: one tile reports an expired look-back, so that the
                                     fallback to the three-kernel path can be exercised */
#define PRT_TRACE_SYNC 64         /* hipStreamSynchronize(stream) before returning */
#define PRT_TRACE_NO_TIMING 256   /* do not bracket the generation launches with HIP events (prt_trace_stats then
                                     reports 0 ms of kernel time): two event records and one event query less per
                                     trace, which is most of what a 125k-ray trace costs the host */
/* (512 was PRT_TRACE_NO_TILE_RECORDS: the per-tile records were retired in 0.2.2 -- worth under 2 % wherever they applied
 * once the sparse-loss forms existed, profiles/r6/ab_round6.txt; the bit is ignored) */
#define PRT_TRACE_BUSY 2048         /* prt_trace_batch only: bracket every job's launches with a pair of HIP events of its own (on the job's stream) and merge the intervals behind the batch: prt_trace_batch_busy */
#define PRT_TRACE_NO_SPARSE_KEEP 1024 /* do not launch sparse-loss generations dense with their absorbed rays kept
                                     (see prt_trace_telemetry); A/B, tests */
#define PRT_TRACE_COUNT_PATHS 128 /* count, in prt_trace_telemetry, the rays that are not well formed and
                                     the CSG node evaluations that took an exact path (see there) */
int64_t prt_trace_workspace_bytes(int64_t n);
int64_t prt_trace(prt_scene* scene, int device, const double* rays, int64_t n, int64_t ld,
                  int generation_limit, double ray_offset, double* rows_out, int64_t rows_cap,
                  int64_t* rows_per_generation, void* workspace, int flags, void* stream);

/* The same in two halves, so that host work and GPU work overlap (no counterpart upstream:
 * pyrayt/_pyrayt.py:329-339 is a blocking loop).  prt_trace_begin enqueues the generations the scene's
 * previous trace needed (a first trace: a batch of four) and returns at once; prt_trace_end waits for
 * their counts, enqueues whatever the trace still needs (more generations; a repeat when a hint did
 * not hold) and returns what prt_trace returns.  prt_trace is begin + end on ticket 0.
 * A scene has PRT_TRACE_TICKETS tickets per device: traces of different tickets may be in flight
 * together.  Every ticket in flight needs its own workspace and its own record block; on one stream they
 * execute one after the other, on two streams their kernels overlap on the device (the workgroups of a
 * generation leave the chip partly idle while they start up and drain).  rays, rows_out and the
 * workspace must stay valid until prt_trace_end.  Results are those of prt_trace, bit for bit. */
#define PRT_TRACE_TICKETS 4
int prt_trace_begin(prt_scene* scene, int device, int ticket, const double* rays, int64_t n, int64_t ld,
                    int generation_limit, double ray_offset, double* rows_out, int64_t rows_cap,
                    void* workspace, int flags, void* stream);
int64_t prt_trace_end(prt_scene* scene, int device, int ticket, int64_t* rows_per_generation);

/* A sequence of traces of one scene -- a tolerance run, a source sweep, the shards of a rank -- with `depth`
 * of them in flight: job k runs on ticket k % depth with workspaces[k % depth] and on streams[k % depth]
 * (NULL: all on the null stream), exactly as a caller of prt_trace_begin / prt_trace_end would run them,
 * without the caller's interpreter between two launches (no counterpart upstream: pyrayt/_pyrayt.py:329-339
 * traces one ray set per call).  It is a convenience and keeps a caller's interpreter out of the loop; it is
 * not faster than a tight loop over the two entry points (125k-ray traces, three in flight: 25 us each either
 * way -- what bounds them is the chain of dependent launches on the device, not the host).
 *   jobs: per trace the ray set, its record block and HOST rows_per_generation[generation_limit]; `total`
 *     receives what prt_trace would have returned for it.  Jobs `depth` apart may share a record block if
 *     the caller wants only the last results (jobs in flight together may not).
 *   workspaces: `depth` blocks, each of prt_trace_workspace_bytes(largest n it will see) bytes.
 *   The ray sets must be complete before the call, or be produced on the stream their job runs on.
 * Returns the rows of all jobs together, or the first error (jobs already in flight are collected, later
 * ones are not started).  As with prt_trace the counts are on the host on return and the rows are ordered
 * on their job's stream (PRT_TRACE_SYNC: every job synchronises its stream when it is collected). */
typedef struct prt_trace_job {
  const double* rays;  /* (13, n) with leading dimension ld */
  int64_t n, ld;
  double* rows_out;    /* (15, rows_cap) */
  int64_t rows_cap;
  int64_t* rows_per_generation;
  int64_t total;       /* out */
} prt_trace_job;
int64_t prt_trace_batch(prt_scene* scene, int device, prt_trace_job* jobs, int64_t count, int generation_limit,
                        double ray_offset, int depth, void* const* workspaces, void* const* streams, int flags);
/* What the last prt_trace_batch of this scene on `device` that was given PRT_TRACE_BUSY measured (for bench.py's
 * roofline: traces in flight together overlap on the device, so the sum of their kernel times says nothing about
 * the region): out4[0] = milliseconds during which at least one of the batch's traces had launches in flight -- the
 * union of the jobs' [first launch enqueued ... last launch finished] intervals, HIP events on each job's own
 * stream --, out4[1] = the sum of those intervals, out4[2] = how many there were, out4[3] = from the earliest
 * start to the latest end.  Zeros if no such batch ran.  (A job that had to repeat an attempt is represented by its
 * last attempt.) */
int prt_trace_batch_busy(const prt_scene* scene, int device, double* out4);

/* ---- record plans: what a trace records (round 6) ------------------------------------------------------
 * The reference appends one row per live ray and generation (_RayTraceDataframe.insert, pyrayt/_pyrayt.py:168-186)
 * and the very next line of its users throws most of them away: `results.loc[results['surface'] ==
 * imager.get_id()]` (examples/lens_design.ipynb cells 11, 19, 38), `results.loc[results['generation'] ==
 * np.max(results['generation'])]` (cells 12, 15, 20) -- to look at a spot size, a focus, a merit function.  A plan
 * tells the generation kernel about it while the row is still in registers:
 *   n_surfaces > 0    only rows whose surface id is one of surfaces[] pass (0: the rows of every surface pass);
 *   store_rows        the rows that pass are stored in rows_out, generation-major / id-ascending as ever: the frame
 *                     is exactly frame.loc[frame.surface.isin(surfaces)] of the unfiltered trace, and
 *                     rows_per_generation / the return value count the stored rows; `columns` picks which of the fifteen
 *                     columns those rows write (the notebook's spot diagrams look at two).  0: nothing is stored at all
 *                     (rows_out may be NULL, rows_cap 0; the counts are 0) -- the caller wants the sums only;
 *   n_groups > 0      the rows that pass are also summed, per generation and per group (group = floor(id /
 *                     rays_per_source), pyrayt/_pyrayt.py:349-354; rays_per_source <= 0: one group), into
 *                     sums_out[(generation * n_groups + group) * PRT_SINK_STATS + k] (device memory, overwritten by
 *                     every trace of the ticket, complete when the trace's stream reaches the end of prt_trace_end):
 *                       k = 0..8  the sums of prt_frame_reduce -- count, sum (y1 - py), sum (z1 - pz), sum of their
 *                                 squares, sum (f - pf), sum (f - pf)^2 with f = the axis intercept x0 - x_tilt y0 /
 *                                 y_tilt over the rows that have one, sum wavelength, sum intensity, rows with an
 *                                 intercept -- about the caller's pivots (device (n_groups, 3): py, pz, pf; NULL:
 *                                 zeros.  A design loop passes the previous iteration's means: second moments about
 *                                 a point near the mean are well conditioned);
 *                       k = 9..11 the sums of prt_frame_mean_square for ms_quantity (a frame column 0..14 or
 *                                 PRT_FRAME_AXIS_INTERCEPT; < 0: none), ms_transform (0 none, 1 sin) and ms_about:
 *                                 rows with a finite v, sum v, sum v^2.
 *                     Sums are additive over generations (one set of pivots): "the rows of the last generation" are
 *                     the block of the highest generation whose count is not zero -- the last generation in which a row
 *                     passed the filter, which is lower than the frame's last generation when rays that miss the
 *                     listed surfaces live on; prt_frame_finish turns a block's first nine into the statistics of
 *                     prt_frame_stats.
 * A plan belongs to a ticket (prt_trace = ticket 0) of a scene on a device and stays in force until replaced; NULL
 * removes it.  Traces under a plan run on the fused path only (PRT_TRACE_UNFUSED / COUNT_PATHS: PRT_ERR_ARG) and
 * learn their own dense-mode hints; without a plan nothing changes -- those kernels do not know about plans.
 * generation_limit: the largest generation_limit a trace under this plan will be given (sizes sums_out). */
#define PRT_SINK_STATS 12
typedef struct prt_record_plan {
  int32_t struct_size;     /* sizeof(prt_record_plan) */
  int32_t n_surfaces;      /* 0 .. 8 */
  int32_t store_rows;
  int32_t n_groups;
  int64_t surfaces[8];     /* surface ids (TracerSurface.get_id()) */
  double rays_per_source;
  double* sums_out;        /* DEVICE (generation_limit, n_groups, PRT_SINK_STATS) float64, or NULL when n_groups == 0 */
  const double* pivots;    /* DEVICE (n_groups, 3) or NULL */
  int32_t ms_quantity, ms_transform;
  double ms_about;
  int32_t generation_limit;
  int32_t columns;         /* which record columns a stored row writes: bit k = column PRT_COL_k; 0 = all fifteen.  A caller
                              that will look at x1, y1 only -- a spot diagram -- asks for those (0x600): the other rows of the
                              (15, rows_cap) block are left as they were, and only two columns need to cross PCIe */
} prt_record_plan;
int prt_trace_set_plan(prt_scene* scene, int device, int ticket, const prt_record_plan* plan);

/* ---- frame re-assembly across the GPUs of a node ----------------------------
 * No counterpart upstream (pyrayt/_pyrayt.py:329-339 is one Python thread).  Rank r traces the
 * contiguous id range [r n/G, (r+1) n/G) with no communication; these entry points put the per-rank
 * record blocks back into the row order of pyrayt/_pyrayt.py:168-186 (generation-major, ascending
 * ray id = rank-major inside a generation).  One process per GPU; the communicator is RCCL's
 * (resolved with dlopen at first use), bootstrapped like any NCCL communicator: rank 0 draws a
 * 128-byte id, the caller broadcasts it (torch.distributed, MPI, a file ...), every rank creates.
 *   prt_allgather_counts   (limit) rows-per-generation of every rank -> counts_all[r * limit + g];
 *                          synchronises the stream (the host sizes the assembled frame from it)
 *   prt_allgather_rows     15 grouped ncclAllGather (one per record column, straight out of the
 *                          (15, ld_rows) block) + the placement kernel; stream-ordered, no host sync;
 *                          ld_rows must be >= the largest per-rank row total
 *   prt_place_rows         the placement kernel alone, for a staging area filled by another
 *                          transport: element (column k, rank r, position p) at
 *                          staging[k * stride_col + r * stride_rank + p]                              */
typedef struct prt_comm prt_comm;
int prt_comm_unique_id(char* id128);
int prt_comm_create(int device, int world, int rank, const char* id128, prt_comm** out);
void prt_comm_destroy(prt_comm* comm);
/* what RCCL reports about the communicator: out3 = { ncclCommCount, ncclCommUserRank, device } */
int prt_comm_info(const prt_comm* comm, int* out3);
int prt_allgather_counts(prt_comm* comm, const int64_t* counts_local, int limit, int64_t* counts_all,
                         void* stream);
int64_t prt_allgather_workspace_bytes(int world, int limit, int64_t pad_rows);
int prt_allgather_rows(prt_comm* comm, const double* rows, int64_t ld_rows, const int64_t* counts_all,
                       int limit, double* out, int64_t ld_out, void* workspace, void* stream);
int64_t prt_place_workspace_bytes(int world, int limit);
int prt_place_rows(int device, const double* staging, int64_t stride_rank, int64_t stride_col, int world,
                   const int64_t* counts_all, int limit, double* out, int64_t ld_out, void* workspace,
                   void* stream);

/* ---- result sink: reductions over the record block on the device ---------------------------------
 * The (15, R) record block is the frame of pyrayt/_pyrayt.py:147-186 in columns.  What upstream's
 * examples compute from that frame (examples/lens_design.ipynb cells 11-16, 19-20, 38) is: keep
 * the rows of one surface and / or generation, group them by source (id // rays_per_source,
 * _pyrayt.py:349-354), and reduce spot positions (y1, z1) and axis intercepts
 * x0 - x_tilt * y0 / y_tilt per group.  One pass over the block; out is (n_groups, 9) float64 on
 * the device: count, sum(y1 - py), sum(z1 - pz), sum((y1 - py)^2 + (z1 - pz)^2), sum(focus - pf),
 * sum((focus - pf)^2), sum(wavelength), sum(intensity), number of rows with a finite axis intercept (the
 * two focus sums run over those: a ray parallel to the axis has none, and pandas' mean skips such a
 * NaN), with pivots = DEVICE (n_groups, 3) float64, per
 * group the (py, pz, pf) its rows are measured from (a second pass about the first pass's means gives
 * well-conditioned second moments), or NULL for 0.
 * surface / generation: NaN selects every row; rays_per_source <= 0: a single group.
 * Every wave keeps the sums of the group it is in in registers (rows are ordered by id, so groups come
 * in runs) and adds them to the output when the group changes; with few groups the waves spread
 * those atomics over 64 copies of the output in a stream-ordered scratch block (hipMallocAsync) that
 * a second kernel folds.  Stream-ordered; no host synchronisation. */
int prt_frame_reduce(int device, const double* rows, int64_t ld, int64_t n_rows, double surface,
                     double generation, double rays_per_source, int n_groups, const double* pivots,
                     double* out, void* stream);
/* The statistics themselves in one stream-ordered call (two prt_frame_reduce passes, the second about
 * the first one's per-group means, computed on the device): out = (n_groups, 8) float64 on the device,
 * per group count, mean y1, mean z1, rms spot radius about that centroid, mean axis intercept, its
 * standard deviation (both over the rows that have an intercept, NaN if none has), mean wavelength, mean
 * intensity (NaN in 1..7 for a group without rows).
 * workspace: prt_frame_stats_workspace_bytes(n_groups) device bytes. */
int64_t prt_frame_stats_workspace_bytes(int n_groups);
int prt_frame_stats(int device, const double* rows, int64_t ld, int64_t n_rows, double surface,
                    double generation, double rays_per_source, int n_groups, double* out, void* workspace,
                    void* stream);
/* The same statistics of a frame that is spread over the ranks of a communicator -- a sharded trace whose rows were
 * NOT re-assembled (each rank holds the rows of its own id range): every rank reduces its own rows and the
 * (n_groups, 9) sums of each pass are added across the ranks with one ncclAllReduce (the second pass runs about the
 * whole frame's means, which every rank then holds).  Every rank receives the statistics of the whole frame; what
 * crosses xGMI is 72 bytes per group and pass instead of the frame (315 MB into every GPU for the north-star job).
 * Stream-ordered; same `out` and `workspace` as prt_frame_stats.  Row order plays no part: any partition of the
 * rows gives the same sums (up to the rounding of the additions). */
int prt_frame_stats_sharded(prt_comm* comm, const double* rows, int64_t ld, int64_t n_rows, double surface,
                            double generation, double rays_per_source, int n_groups, double* out, void* workspace,
                            void* stream);
/* The steps between and behind the two passes on their own, for sums added across ranks by another transport
 * (prt_frame_reduce on every rank -> add -> prt_frame_pivots -> prt_frame_reduce about them -> add ->
 * prt_frame_finish): pivots_out (n_groups, 3) = per group the means (y1, z1, axis intercept) of a first pass's sums;
 * out (n_groups, 8) = the statistics from a second pass's sums and the pivots it ran about.  All device pointers. */
int prt_frame_pivots(int device, const double* sums, int n_groups, double* pivots_out, void* stream);
int prt_frame_finish(int device, const double* sums, const double* pivots, int n_groups, double* out, void* stream);
/* Mean squares of one quantity of the frame: the merit functions of examples/lens_design.ipynb, all of the form
 * np.mean(np.square(f(rows) - c)) over a selection of rows (cell 20, the coma metric: np.sin(ray_set['y_tilt']) -
 * np.sin(angle) over the rows of the last generation; cells 28 / 32: the axis intercept minus the design focus).
 * quantity: a frame column (PRT_COL_*, 0..14) or PRT_FRAME_AXIS_INTERCEPT = x0 - x_tilt * y0 / y_tilt (cells 12, 15);
 * transform: 0 none, 1 sin; v = transform(quantity) - about.  out = (n_groups, 3) float64 on the device, per group
 * the rows counted, sum v, sum v^2, over the rows that pass the surface / generation filter (NaN = every row) and
 * whose v is finite (pandas' mean skips a NaN: a ray parallel to the axis has no intercept); the sums are additive
 * over any partition of the rows, so a sharded frame adds them across ranks before dividing.  rays_per_source <= 0:
 * one group.  Stream-ordered. */
#define PRT_FRAME_AXIS_INTERCEPT 15
int prt_frame_mean_square(int device, const double* rows, int64_t ld, int64_t n_rows, double surface,
                          double generation, double rays_per_source, int n_groups, int quantity, int transform,
                          double about, double* out, void* stream);
/* Histograms of the frame: what a spot diagram, an irradiance map or examples/lens_design.ipynb cell 19
 * (`ray_set.hist('y1')`) computes from the rows, with numpy's bin rule (np.histogram / np.histogram2d): bin i takes
 * v when edges[i] <= v < edges[i+1], the last bin also takes v == edges[n]; values outside [edges[0], edges[n]], NaN
 * and +-inf are not counted; in two dimensions a row counts only when both of its values fall in a bin.
 *
 * prt_frame_range: the smallest and the largest FINITE value of one quantity (a frame column 0..14 or
 * PRT_FRAME_AXIS_INTERCEPT) over the rows that pass the surface / generation filter (NaN = every row), into
 * minmax_out = 2 doubles of DEVICE memory; +inf, -inf when no value is finite.  Integer atomics on an
 * order-preserving image of the doubles: the same result on every run.  Stream-ordered.
 *
 * prt_frame_histogram: x_quantity (and y_quantity; -1: one dimension, y_edges / ny / y_uniform ignored) binned against
 * x_edges[0..nx] (y_edges[0..ny]): HOST arrays, finite and non-decreasing (else PRT_ERR_ARG), copied into the
 * workspace (prt_frame_histogram_workspace_bytes(n_groups, nx, ny, with_weights) device bytes; ny < 1 for one
 * dimension) before the call returns.  x_uniform / y_uniform: the edges are evenly spaced (np.linspace), and the bin
 * is guessed by arithmetic and then corrected against the edges, as numpy's own fast path does -- the answer is the
 * edges' either way.  Rows pass the same surface / generation filter as prt_frame_reduce and are grouped by
 * floor(id / rays_per_source) (rays_per_source <= 0: one group; a row whose group is outside [0, n_groups) is not
 * counted).  counts_out: DEVICE int64 (n_groups, nx, ny) (ny = 1 in one dimension), overwritten: exact, and the
 * same on every run.  weight_column 0..14: weights_out, DEVICE float64 of the same shape, overwritten with the sums
 * of that column per bin; -1 (and weights_out NULL): counts only.  The weight sums are float64 adds whose order
 * depends on the schedule: exact -- and then the same on every run -- when the weights are integers and every sum
 * stays below 2^53 (every built-in source emits intensity 100), otherwise equal up to the last bits.
 * The histogram is privatised in LDS (a window per workgroup of 65 536 bins counts only when a workgroup's share of
 * the rows is below 2^16 -- 16-bit tallies --, else 32 768, and 10 922 with weights; one global add per non-zero bin
 * and workgroup, or -- counts only, large windows -- per-workgroup slabs in a stream-ordered scratch block
 * (hipMallocAsync) added up by a second kernel); more bins than a window are done in several passes over the rows.
 * All arguments are checked before a device is touched.  Stream-ordered. */
int prt_frame_range(int device, const double* rows, int64_t ld, int64_t n_rows, double surface, double generation,
                    int quantity, double* minmax_out, void* stream);
int64_t prt_frame_histogram_workspace_bytes(int n_groups, int nx, int ny, int with_weights);
int prt_frame_histogram(int device, const double* rows, int64_t ld, int64_t n_rows, double surface, double generation,
                        double rays_per_source, int n_groups, int x_quantity, const double* x_edges, int nx,
                        int x_uniform, int y_quantity, const double* y_edges, int ny, int y_uniform,
                        int weight_column, int64_t* counts_out, double* weights_out, void* workspace, void* stream);
/* Optical path and wavefront error of the frame (no counterpart upstream: the examples study aberrations through spot
 * moments and axis intercepts, examples/lens_design.ipynb cells 11-20).  The rows are pyrayt/_pyrayt.py:168-186's:
 * segment start x0..z0, end x1..z1, unit direction x_tilt..z_tilt, the index of the medium it runs through, the ray id.
 *
 * Definitions.
 * Segment and OPL: a row's segment OPL is index * sqrt(dx*dx + dy*dy + dz*dz), d = (x1,y1,z1) - (x0,y0,z0), evaluated
 *   in that order.  A row's cumulative OPL is its own segment OPL plus the cumulative OPL of the same id's row in the
 *   previous generation; a generation-0 row has only its own.  The rows are the contract, so the 1e-6 relaunch offset
 *   (pyrayt/_pyrayt.py:449) is part of x0 as written and not added back.
 * Reference sphere: for a row Q = (x1,y1,z1) at surface S with direction u and index n, the ray is extended backwards to
 *   E = Q - s u on the sphere of centre P and radius R, s the larger real root (E on the side the light came from).
 *   OPL_E = OPL_Q - n s; OPD = OPL_E - pivot, positive when the ray's path is longer.  A ray whose line misses the
 *   sphere gets OPD = NaN and is counted apart.
 * Pupil: the component of E - P perpendicular to the unit axis a, in the basis (e1, e2) of the plane perpendicular to
 *   a, divided by the pupil radius (default: the group's largest radial extent); theta runs from e1 towards e2.
 * Zernike: Noll's order and RMS normalisation (Noll 1976), Z1 = 1, Z2 = 2 rho cos theta, Z3 = 2 rho sin theta,
 *   Z4 = sqrt(3) (2 rho^2 - 1), ..., Z11 = sqrt(5) (6 rho^4 - 6 rho^2 + 1); n_terms <= 36.
 * P: the mean of the group's Q, or given; R: given, or the distance from P to the mean of the group's (x0,y0,z0) at S
 *   (where the image-space segments start: a stand-in for the exit pupil).  Pivot: OPL_E of the group's first row at S
 *   in row order that meets the sphere.
 *
 * prt_frame_optical_path: the cumulative OPL of every row into opl_out (DEVICE, one double a row).  The frame is whole
 * and generation-major: rows_per_generation (HOST, n_generations counts) gives the generations' row runs; ids are
 * integers in [id0, id0 + n_ids) (a dense accumulator and a stamp per id, in a stream-ordered scratch block).  One
 * launch per generation, in order; an id outside the range or repeated within a generation gives PRT_ERR_ARG.  The
 * call reads one status word back and so returns when the stream has reached its end.
 *
 * prt_frame_wavefront: the wavefront at the rows that pass the surface / generation filter (NaN = every row), grouped
 * by floor(id / rays_per_source) (<= 0: one group), opl the rows' cumulative OPL (prt_frame_optical_path).  reference:
 * DEVICE (n_groups, 3) centres, or NULL for each group's centroid of Q; radius: DEVICE (n_groups) radii, or NULL (an
 * entry <= 0 or NaN: the default); axes: HOST 9 doubles a, e1, e2; pupil_radius 0: the group's largest radial extent.
 * Out, DEVICE, overwritten: opd_out / pupil_out (n_rows / (n_rows, 2) capacity) hold the selected rows in row order --
 * the OPD with the group's weighted mean taken off (piston removed) and the normalised pupil point (e1, e2); NaN for a
 * row that misses the sphere -- group_out (n_groups, 12): P (3), R, pivot, pupil radius, rows, rows that miss, largest
 * and smallest OPD about the pivot, first row, largest radial extent; normal_out (n_groups, n_terms (n_terms + 1) / 2
 * + n_terms + 3): the upper triangle of Z^T W Z by rows, Z^T W OPD, sum w, sum w OPD, sum w OPD^2 (OPD about the
 * pivot), W = 1 or the weight_column (0..14; -1: ones).  workspace: prt_frame_wavefront_workspace_bytes(n_rows,
 * n_groups, n_terms, with_weights) device bytes.  No floating-point atomics: every output is the same, bit for bit, on
 * every run.  All arguments are checked before a device is touched.  Stream-ordered. */
int prt_frame_optical_path(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                           int n_generations, double id0, int64_t n_ids, double* opl_out, void* stream);
int64_t prt_frame_wavefront_workspace_bytes(int64_t n_rows, int n_groups, int n_terms, int with_weights);
int prt_frame_wavefront(int device, const double* rows, int64_t ld, int64_t n_rows, const double* opl, double surface,
                        double generation, double rays_per_source, int n_groups, const double* reference,
                        const double* radius, const double* axes, double pupil_radius, int n_terms, int weight_column,
                        double* opd_out, double* pupil_out, double* group_out, double* normal_out, void* workspace,
                        void* stream);

/* Diffraction PSF and Strehl ratio of the frame: the Huygens sum over the rays that reach the reference sphere (no
 * counterpart upstream).  It takes the wavefront's own reference sphere and OPD, so there is one definition and not two.
 *
 * Definitions.
 * Rays: the rows prt_frame_wavefront selected with the same rows / ld / n_rows / surface / generation /
 *   rays_per_source / n_groups, in its order; opd, pupil and group_record are that call's opd_out, pupil_out and
 *   group_out.  For group g it gives P, R, the pupil radius rho and the axes (a, e1, e2).  A ray whose OPD is NaN (it
 *   missed the sphere), or whose weight is not finite and >= 0, is left out and counted.
 * Ray r contributes p1 = pupil_r[0] * rho and p2 = pupil_r[1] * rho (these are (E_r - P).e1 and (E_r - P).e2), OPD_r
 *   and an amplitude a_r = sqrt(w_r), w the weight_column (-1: ones).
 * Image plane: through P, perpendicular to a.  Pixel (i, j) lies at x = P + u_i e1 + v_j e2, where
 *   u_i = u0 + (i - (nx-1)/2) du and v_j = v0 + (j - (ny-1)/2) dv.
 * Distance: d_r(x) = sqrt(R^2 + u^2 + v^2 - 2 (u p1 + v p2)), exact when |E_r - P| = R; the formula is the contract.
 * Wavelengths are in micrometres, as upstream's are (components.py:472); world units are the caller's, so
 *   lambda_w = wavelength / world_unit_um (world_unit_um = 1000 for millimetres).
 * Phase: phi_r(x) = (OPD_r + d_r(x) - R) / lambda_w, in cycles.  Amplitude: U_l(x) = (1/lambda_w) sum over the rays
 *   r of wavelength l of a_r exp(2 pi i phi_r(x)).  Rays of one wavelength add coherently, wavelengths incoherently.
 * Normalised image: I(x) = sum_l |U_l(x)|^2 / sum_l (sum over r of l of a_r / lambda_w)^2.  A perfect wave on the same
 *   rays gives exactly 1 at P.
 * Strehl: I at P, (u, v) = (0, 0), whether or not P is a pixel centre:
 *   sum_l |sum a_r exp(2 pi i OPD_r / lambda_w)|^2 / lambda_w^2 / sum_l (sum a_r / lambda_w)^2; piston drops out.
 * Amplitude factors of the Huygens-Fresnel integral other than 1/lambda (the obliquity factor, 1/r) are taken as
 *   constant over the pupil: the error is of the order of NA^2 at the rim.  Each ray stands for an equal share of the
 *   pupil's area, or carries its share in w; random pupil samples give a noise floor of about 1 / (number of rays).
 * Accuracy: the phase is reduced in fp64 and its sine and cosine come from the fp32 instructions, so a ray's phasor is
 *   within eps = 3e-7 + 2 pi 2^-25 + 16 pi ulp(R / lambda_w) of the definition's (3e-7: twice the instructions' measured
 *   error) and a bucket's normalised intensity within 2 eps sqrt(I) + eps^2: about 1e-6 at the peak, 2e-13 where the
 *   image is dark.  The Strehl ratio is summed with fp64 sines and cosines: within 4 pi 2 ulp(R / lambda_w) and a few
 *   hundred ulps.  tests/diffraction_reference.py derives both and states what is counted.
 *
 * prt_frame_psf: wavelengths_um (HOST, n_wavelengths <= 16 distinct values, finite and > 0) lists every wavelength of
 * the selected rows (a row of another wavelength: PRT_ERR_ARG once the passes have run); nx, ny in 1..1024; du, dv
 * finite and > 0; centre_uv (HOST) = (u0, v0).  n_groups * n_wavelengths * nx * ny * 16 bytes may not pass the 256 MiB
 * cap of the partial-sum slab.  Out, DEVICE, overwritten: image_out (n_groups, n_wavelengths, nx, ny) -- the group's
 * normalised image per wavelength: the polychromatic image is their sum; NaN for a group without rays --; strehl_out
 * (n_groups); record_out (n_groups, n_wavelengths, 4): rays used, rays left out, sum a, and the Strehl numerator
 * |sum a exp(2 pi i OPD / lambda_w)|^2 / lambda_w^2.  workspace: prt_frame_psf_workspace_bytes(n_rows, n_groups,
 * n_wavelengths) device bytes.  The sum is a grid of (pixel tile, ray slice, (group, wavelength) bucket) workgroups
 * over rays sorted into buckets by a stable counting sort; partial sums are folded in slice order, with no
 * floating-point atomics: every output is the same, bit for bit, on every run.  All arguments are checked before a
 * device is touched.  Stream-ordered; the call reads one status word back and so returns when the stream has reached
 * its end. */
int64_t prt_frame_psf_workspace_bytes(int64_t n_rows, int n_groups, int n_wavelengths);
int prt_frame_psf(int device, const double* rows, int64_t ld, int64_t n_rows, double surface, double generation,
                  double rays_per_source, int n_groups, const double* opd, const double* pupil,
                  const double* group_record, int weight_column, const double* wavelengths_um, int n_wavelengths,
                  double world_unit_um, int nx, int ny, double du, double dv, const double* centre_uv,
                  double* image_out, double* strehl_out, double* record_out, void* workspace, void* stream);

/* Diffraction PSF and Strehl ratio through focus: the Huygens sum above on n_focus planes shifted along the axis, from
 * one wavefront and without a re-trace (no counterpart upstream).
 *
 * Definitions.
 * Everything of prt_frame_psf stays: the rays, p1, p2, OPD_r, a_r, lambda_w, the buckets, the normalisation (its
 *   denominator, which no plane moves) and record_out.
 * Sphere point: E_r = P + p1 e1 + p2 e2 + p3 a with p3 = (E_r - P).a, formed by extending the row to the sphere again
 *   as prt_frame_wavefront does (its sign is that of -(u.a), u the ray's direction).  A ray is kept under
 *   prt_frame_psf's rule and a finite p3: the same rays, buckets and order.
 * Planes: plane f lies through P + delta_f a, perpendicular to a; delta has the sign of prt_frame_mtf's focus.  Pixel
 *   (i, j) of plane f of group g lies at x = P + u e1 + v e2 + delta_f a with u = cu_gf + (i - (nx-1)/2) du and
 *   v = cv_gf + (j - (ny-1)/2) dv.
 * Distance: d_r(x) = sqrt(R^2 + u^2 + v^2 + delta^2 - 2 (u p1 + v p2 + delta p3)); phase and amplitude as above.
 * Chief line: the line through P and the weighted mean of the group's sphere points.  Per unit of delta it moves by
 *   t_i = (sum w_r p_i) / (sum w_r p3), i = 1, 2, the sums over the group's kept rays of all wavelengths (w_r = a_r^2):
 *   the slope (u.e_i) / (u.a) of a ray that runs from the mean sphere point to P.  track = 1: the centre of plane f
 *   is (cu, cv)_gf = (u0 + delta_f t1, v0 + delta_f t2), each one fma; track = 0: t = 0 and every centre is (u0, v0).
 * Strehl through focus: the normalised intensity at P + delta_f (t1 e1 + t2 e2 + a), whatever the grid:
 *   sum_l |sum a_r exp(2 pi i (OPD_r + d_r - R) / lambda_w)|^2 / lambda_w^2 over prt_frame_psf's denominator, d_r from
 *   a correctly rounded fp64 square root and the phasor from fp64 sincospi.
 * Bits: a plane with delta = 0.0 has the image, the Strehl ratio and the record of prt_frame_psf on the same arguments;
 *   a plane's bits do not depend on the other planes, their number or their order (the ray slices are those
 *   prt_frame_psf picks for one plane's grid; planes past the slab cap run in chunks of planes).
 * Accuracy: prt_frame_psf's eps with the roundings of the new terms; tests/psf_focus_reference.py derives it.
 *
 * prt_frame_psf_focus: the arguments of prt_frame_psf, and: axes HOST 9 doubles (a, e1, e2), the ones
 * prt_frame_wavefront was given; focus HOST n_focus (1..256) finite shifts; track 0 or 1.  Out, DEVICE, overwritten:
 * image_out (n_groups, n_focus, n_wavelengths, nx, ny); strehl_out (n_groups, n_focus); record_out (n_groups,
 * n_wavelengths, 4) as prt_frame_psf's; axial_out (n_rows; the first n_selected are written): p3 per selected row in
 * the wavefront's order, NaN where the pupil point is NaN; line_out (n_groups, 2): t1, t2 (NaN for a group without
 * rays under track = 1); centres_out (n_groups, n_focus, 2).  The cap of prt_frame_psf's slab holds for one plane.
 * workspace: prt_frame_psf_focus_workspace_bytes(n_rows, n_groups, n_wavelengths, n_focus) device bytes (-1 for
 * arguments the call would refuse).  All arguments are checked before a device is touched.  Stream-ordered; the call
 * reads one status word back and so returns when the stream has reached its end. */
int64_t prt_frame_psf_focus_workspace_bytes(int64_t n_rows, int n_groups, int n_wavelengths, int n_focus);
int prt_frame_psf_focus(int device, const double* rows, int64_t ld, int64_t n_rows, double surface, double generation,
                        double rays_per_source, int n_groups, const double* opd, const double* pupil,
                        const double* group_record, int weight_column, const double* wavelengths_um,
                        int n_wavelengths, double world_unit_um, int nx, int ny, double du, double dv,
                        const double* centre_uv, const double* axes, const double* focus, int n_focus, int track,
                        double* image_out, double* strehl_out, double* record_out, double* axial_out,
                        double* line_out, double* centres_out, void* workspace, void* stream);

/* Polarised diffraction PSF of the frame: the Huygens sum above with the Fresnel pass's complex field vectors as the
 * rays' amplitudes (no counterpart upstream).  The scalar PSF sees the Fresnel losses as apodisation only; this sum
 * also carries the phase a coating, a metal or a total internal reflection puts on s and p, the rotation of the field
 * across the pupil and the field's axial component.
 *
 * Definitions.
 * Everything of the scalar PSF stays: the wavefront's P, R, rho, axes (e1, e2, a) and OPD; the selected rows, the
 *   (group, wavelength) buckets and the pixel grid; d_r and the phase in cycles; the usable-ray rule.
 * States.  A Fresnel from polarised input (polarization not None) has one state, Ea.  From unpolarised input it has
 *   two, Ea and Eb, which add incoherently with weight 1/2 each.  The sum is coherent over the rays, so a state must be
 *   one state of the whole beam: prt_frame_fresnel launches an unpolarised ray in a basis made from the ray's own
 *   direction, and the caller recombines Ea and Eb per ray into states that are uniform across the beam before this
 *   call (the pass is linear in the launch field; pyrayt_amd does it in Fresnel.uniform_states).
 * Component amplitudes.  Ray r in state s has amplitude A_r = sqrt(w_r) E_r.  w_r is the weights column of the frame
 *   the Fresnel was computed on.  It is not the applied frame, so T does not enter twice.  E_r is the field on the
 *   selected row's segment.  The components are c_r = (A_r.e1, A_r.e2, A_r.a): plain dot products with the real axes,
 *   complex in general.  A ray whose field is not finite (one past an invalid interface) is left out and counted,
 *   like a ray without a usable weight; with two states it is left out of both when either field is not finite.
 * Field at a pixel.  U_{l,s,k}(u, v) = (1 / lambda_l) sum_r c_{r,k} exp(2 pi i phase_r(u, v)), for k = 1, 2, 3.
 * Per state and wavelength.  S0 = |U1|^2 + |U2|^2, S1 = |U1|^2 - |U2|^2, S2 = 2 Re(conj(U1) U2),
 *   S3 = 2 Im(conj(U1) U2), axial = |U3|^2.  This is the convention of Fresnel.stokes.  The image of a bucket is the
 *   mean over its states of S0 + axial.
 * Normalisation.  Divide by the scalar PSF's own denominator, D_g = sum_l (sum_r sqrt(w_r) / lambda_l)^2.  This is the
 *   perfect, lossless wave with parallel fields on the same rays.
 * Two Strehl ratios.  strehl is the image at P over D_g.  It is comparable to the scalar psf() of the bare frame and
 *   across coatings.  strehl_apodized is the image at P over D'_g = mean_s sum_l (sum_r |A_r| / lambda_l)^2, with
 *   |A_r| the complex 3-norm.  This is the strict ratio against the same amplitudes with phases and field directions
 *   aligned.  Both are evaluated at P with fp64 sincospi, as k_psf_strehl does, whether or not P is a pixel centre.
 * Throughput.  throughput_g = sum_r w_r |E_r|^2 / sum_r w_r, the mean over states, over the rays summed.
 * Accuracy: the phase path is the scalar kernel's, so |U~_k - U_k| <= eps sum_r |c_{r,k}| / lambda with the eps above;
 *   tests/vector_psf_reference.py derives from it the bound of every Stokes plane.
 *
 * prt_frame_vector_psf: the arguments of prt_frame_psf, and: field (DEVICE) -- (field_planes, field_ld) float64, the
 * block prt_frame_fresnel (field_planes = 6: Ea then Eb by component, real) or prt_frame_fresnel_coated (12: the six
 * real parts, then the six imaginary parts) wrote, offset to the first of the n_rows rows; field_ld >= n_rows, the
 * distance between two planes; n_states 1 (Ea alone) or 2; axes HOST 9 doubles (a, e1, e2), the ones
 * prt_frame_wavefront was given.  n_groups * n_wavelengths * n_states may not pass 65535, and
 * n_groups * n_wavelengths * n_states * nx * ny * 48 bytes may not pass the 256 MiB cap of the partial-sum slab.
 * Out, DEVICE, overwritten: stokes_out (n_groups, n_wavelengths, 5, nx, ny) -- S0, S1, S2, S3 and axial, the mean
 * over the states, over D_g; NaN for a group without rays --; strehl_out (n_groups, 4): strehl, strehl_apodized,
 * throughput, D_g; record_out (n_groups, n_wavelengths, n_states, 6): rays used, rays left out, sum sqrt(w), sum |A|,
 * the Strehl numerator sum_k |sum c_k exp(2 pi i OPD / lambda_w)|^2 / lambda_w^2, sum w |E|^2.  workspace:
 * prt_frame_vector_psf_workspace_bytes(n_rows, n_groups, n_wavelengths, n_states) device bytes (-1 for arguments the
 * call would refuse).  The sum is a grid of (pixel tile, ray slice, (group, wavelength, state) bucket) workgroups;
 * partial sums are folded in slice order, with no floating-point atomics: every output is the same, bit for bit, on
 * every run.  All arguments are checked before a device is touched.  Stream-ordered; the call reads one status word
 * back and so returns when the stream has reached its end. */
int64_t prt_frame_vector_psf_workspace_bytes(int64_t n_rows, int n_groups, int n_wavelengths, int n_states);
int prt_frame_vector_psf(int device, const double* rows, int64_t ld, int64_t n_rows, double surface, double generation,
                         double rays_per_source, int n_groups, const double* opd, const double* pupil,
                         const double* group_record, int weight_column, const double* wavelengths_um,
                         int n_wavelengths, double world_unit_um, int nx, int ny, double du, double dv,
                         const double* centre_uv, const double* field, int64_t field_ld, int field_planes,
                         int n_states, const double* axes, double* stokes_out, double* strehl_out, double* record_out,
                         void* workspace, void* stream);

/* Geometric MTF of the frame, through focus (no counterpart upstream).  It reads only each ray's end point and
 * direction at the surface, so it works on frames that hold the detector's rows alone.
 *
 * Definitions.
 * Rays: rows at surface (NaN: any), in generation (NaN: any), in group g = floor(id / rays_per_source) with
 *   0 <= g < n_groups (rays_per_source <= 0: one group).  Each ray has an end point Q = (x1, y1, z1), a direction
 *   u = (x_tilt, y_tilt, z_tilt) (which need not be unit length) and a weight w (weight_column, or ones for -1).
 * Rays left out: a ray is left out and counted (n_missed) when u.a == 0, when any value it needs is not finite, or when
 *   w is not finite and >= 0.
 * Axes: (a, e1, e2), the 9 doubles of frame.pupil_axes().  The default is a = x, e1 = y, e2 = z.
 * Centre C_g: the weighted centroid of the group's Q, or a given point per group (reference).
 * Plane at shift delta: the plane through C_g + delta a, perpendicular to a.  Ray r meets it at
 *   X_r(delta) = Q_r + u_r ((C_g + delta a - Q_r).a) / (u_r.a).  Its coordinates in that plane are
 *   x_r(delta) = ((X_r(delta) - C_g).e1, (X_r(delta) - C_g).e2).  These are linear in delta:
 *   x_r(delta) = p_r + delta s_r with s_r = (u.e1, u.e2) / (u.a).
 * Frequency vector: azimuth theta in degrees, measured from e1 towards e2, and frequency nu >= 0 in cycles per world
 *   unit (cycles/mm for a scene in mm).  Together they give k = nu (cos theta, sin theta).
 * OTF: OTF_g(delta, theta, nu) = sum_r w_r exp(-2 pi i k.x_r(delta)) / sum_r w_r.  Wavelengths are not separated: the
 *   geometric MTF is polychromatic through the weights.  The MTF is |OTF| and the PTF is arg OTF, about C_g.  A group
 *   with no rays, or with sum w = 0, gives NaN.
 * Accuracy: the phase k.x is formed and reduced in fp64, its sine and cosine come from the fp32 instructions with the
 *   conversion's rounding put back to first order: |OTF - definition| <= 3e-7 + 2e-14 + 2 pi 13 2^-53 T, T the weighted
 *   mean of the magnitudes of the phase's terms in cycles (3e-7: twice the instructions' measured error).
 *   tests/diffraction_reference.py derives it and states what is counted.
 *
 * prt_frame_mtf: reference DEVICE (n_groups, 3) or NULL for the centroids; axes HOST 9 doubles; frequencies (HOST,
 * 1..4096, finite and >= 0), azimuths_deg (HOST, 1..16, finite), focus (HOST, 1..256 shifts delta, finite);
 * n_groups * n_focus * n_azimuths * n_frequencies * 16 bytes may not pass the 256 MiB cap of the partial-sum slab.
 * Out, DEVICE, overwritten: otf_out (n_groups, n_focus, n_azimuths, n_frequencies, 2) -- real and imaginary part --;
 * record_out (n_groups, 6): C_g (3), sum w, rays used, rays left out.  workspace: prt_frame_mtf_workspace_bytes(n_rows,
 * n_groups, n_frequencies, n_azimuths, n_focus) device bytes.  The rays are sorted into group buckets in row order by a
 * stable counting sort; the sum is a grid of (ray slice, output tile) workgroups whose partial sums are folded in
 * slice order.  Every partition depends only on a group's count of rays used, on the output count and on n_groups,
 * never on n_rows, and there are no floating-point atomics: every output is the same, bit for bit, on every run and on
 * any frame that holds the same selected rows in the same order.  sum w is added in the order of the numerators, so
 * the OTF at nu = 0 is exactly 1.  All arguments are checked before a device is touched.  Stream-ordered; the call
 * returns when the stream has reached its end. */
int64_t prt_frame_mtf_workspace_bytes(int64_t n_rows, int n_groups, int n_frequencies, int n_azimuths, int n_focus);
int prt_frame_mtf(int device, const double* rows, int64_t ld, int64_t n_rows, double surface, double generation,
                  double rays_per_source, int n_groups, const double* reference, const double* axes, int weight_column,
                  const double* frequencies, int n_frequencies, const double* azimuths_deg, int n_azimuths,
                  const double* focus, int n_focus, double* otf_out, double* record_out, void* workspace, void* stream);

/* MTF sensitivities: d(OTF)/d(parameter) through focus, from the rows, jacobian_out and slopes_out of one
 * prt_frame_launch_sensitivity call (below; any kinds of parameter), without a re-trace.
 *
 * Definitions, with those of the geometric MTF above.
 * Rays: the selected rows of the sensitivity call, in its order (selected DEVICE n_selected int64 row numbers, ordered by
 *   group, generation and id; group_first HOST n_groups + 1 int64: group q is [group_first[q], group_first[q + 1]), a
 *   contiguous run, so nothing is sorted).  Weights: weight_column, or ones for -1.
 * Rays kept: a ray is kept if the MTF would keep it (the rule "Rays left out" above; a row number outside [0, n_rows)
 *   counts as left out too) and its 3 K entries of jacobian and its 3 K entries of slopes are all finite.  There is one
 *   kept set for all K.  The others are counted per group: n_missed by the MTF's rule, n_unfollowed by the second.  A ray
 *   that is left out contributes exactly nothing: it keeps its place in the order with w = 0 and zero derivatives.
 * Staged: uh = u / |u| (slopes is duh_k, the derivative of the unit direction), s = (uh.e1, uh.e2) / (uh.a),
 *   d = Q - C_g, p = (d.e1, d.e2) - s (d.a), x(delta) = p + delta s.  C_g is the weighted centroid of the kept rays' Q, or a
 *   given point per group (reference); it is HELD FIXED under the parameter.
 * Per parameter k, with dQ_k = jacobian and duh_k = slopes:
 *   ds_k = ((duh_k.e1, duh_k.e2) - s (duh_k.a)) / (uh.a)
 *   dp_k = (dQ_k.e1, dQ_k.e2) - s (dQ_k.a) - ds_k (d.a)
 *   dx_k(delta) = dp_k + delta ds_k
 * Outputs:
 *   OTF_g(delta, theta, nu)     = sum w exp(-2 pi i k.x(delta)) / sum w, as above;
 *   dOTF_g,k(delta, theta, nu)  = -2 pi i sum w (k.dx_k(delta)) exp(-2 pi i k.x(delta)) / sum w;
 *   dOTF_g / d delta            = -2 pi i sum w (k.s) exp(-2 pi i k.x(delta)) / sum w, the through-focus derivative;
 *   dC_g,k = sum w dQ_k / sum w, over the same rays: what a centre that follows the centroid adds, composed by the caller
 *   as dOTF_k + 2 pi i (k.(dC_k.e1, dC_k.e2)) OTF + (dC_k.a) dOTF / d delta.
 * Accuracy: the phasor is the MTF's (with the first-order correction folded into it once); a derivative carries, beside the
 *   phasor's error times |k.dx_k|, the roundings of k.dx_k itself: tests/mtf_gradient_reference.py derives the bound
 *   |dOTF~ - dOTF| <= 2 pi [mean_w(|g| e) + 29 2^-53 mean_w(G)] and states what is counted.
 *
 * prt_frame_mtf_gradient: rows DEVICE, ld, n_rows as above; jacobian, slopes DEVICE (K, 3, n_selected), K in [1, 16];
 * reference DEVICE (n_groups, 3) or NULL for the centroids; axes HOST 9 doubles; frequencies, azimuths_deg, focus HOST with
 * the MTF's limits; n_groups in [1, 65535]; n_groups * n_focus * n_azimuths * n_frequencies * 18 * 16 bytes (the slab of a
 * call with 16 parameters, whatever K is) may not pass the 256 MiB cap.
 * Out, DEVICE, overwritten: otf_out (n_groups, n_focus, n_azimuths, n_frequencies, 2); dotf_out (n_groups, K + 1, n_focus,
 * n_azimuths, n_frequencies, 2), index K the focus derivative; record_out (n_groups, 7 + 3 K): C_g (3), sum w, rays used,
 * n_missed, n_unfollowed, then dC_k (K vectors).  A group with no rays kept, or with sum w = 0, is NaN in otf_out, dotf_out, C_g (unless given) and
 * dC_k.  workspace: prt_frame_mtf_gradient_workspace_bytes(n_selected, n_groups, K, n_frequencies, n_azimuths, n_focus)
 * device bytes (-1 for arguments the call would refuse).
 * Passes: centre chunks of 1024 selected rows in a fixed tree; the record; staging; the sum, a grid of (ray slice, output
 * tile, chunk of at most 8 parameters) workgroups that read the ray tile through LDS; the fold in slice order.  Every
 * partition depends only on a group's count of selected rows, on the output count and on n_groups -- never on n_rows or the
 * frame's other rows, never on K --, a parameter's arithmetic does not depend on the others in the call, and there are no
 * floating-point atomics: every output is the same, bit for bit, on every run, on any frame that holds the same selected
 * rows, and for a parameter alone or among sixteen (where the kept set is the same).  All arguments are checked before a
 * device is touched.  Stream-ordered; the call returns when the stream has reached its end. */
int64_t prt_frame_mtf_gradient_workspace_bytes(int64_t n_selected, int n_groups, int n_parameters, int n_frequencies,
                                               int n_azimuths, int n_focus);
int prt_frame_mtf_gradient(int device, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                           int64_t n_selected, const int64_t* group_first, int n_groups, int weight_column,
                           const double* jacobian, const double* slopes, int n_parameters, const double* reference,
                           const double* axes, const double* frequencies, int n_frequencies, const double* azimuths_deg,
                           int n_azimuths, const double* focus, int n_focus, double* otf_out, double* dotf_out,
                           double* record_out, void* workspace, void* stream);

/* PSF sensitivities: d(PSF)/d(parameter) and d(Strehl)/d(parameter) of the diffraction PSF above, from the rows and the
 * wavefront outputs of one prt_frame_opd_sensitivity (or prt_frame_launch_sensitivity) call, without a re-trace.  The
 * definitions of prt_frame_psf and of prt_frame_opd_sensitivity (below) are reused unchanged.
 *
 * Definitions.
 * Rays: the selected rows of the sensitivity call, in its order (selected DEVICE n_selected int64 row numbers, ordered by
 *   group, generation and id; group_first HOST n_groups + 1 int64).  opd and pupil are that call's opd_out and pupil_out;
 *   group g's R and rho come from wavefront_groups (HOST (n_groups, 6), [3] and [5]); w is weight_column of rows (-1:
 *   ones), the wavelength the row's wavelength column.
 * Rays kept: a ray is kept if prt_frame_psf would keep it (OPD and pupil point finite, w finite and >= 0) and its 3 K
 *   derivative inputs are finite.  There is one kept set for all K.  The others are counted per (group, wavelength):
 *   n_missed by the PSF's rule, n_unfollowed by the second; they contribute exactly nothing.
 * Staged per ray, s = 1 / lambda_w: p = pupil * rho, c = (OPD - R) s, a = sqrt(w).  Per parameter k, from the plain
 *   arrays dphase (x_k) and dpoint (y_k, two components; NULL: zeros): e_k = x_k s, q_k = y_k rho s.  With x = dopd and
 *   y = dpupil the result is the exact derivative of the sum prt_frame_psf forms on the changed system, the sphere
 *   held fixed, each ray followed; with x = dfield and y = 0 it is the wavefront change at fixed pupil points.
 * At pixel (u, v): d = sqrt(R^2 + u^2 + v^2 - 2 (u p1 + v p2)), phi = c + d s, and
 *   g_k = e_k - (u q_k1 + v q_k2) / d, in cycles per unit parameter (d(phi)/dp_k: d moves with the ray's point p).
 * Sums over the kept rays of wavelength l:
 *   U_l     = s sum a exp(2 pi i phi)                 dU_l,k = 2 pi i s sum a g_k exp(2 pi i phi)
 *   I       = sum_l |U_l|^2 / D_g                     dI_k   = 2 sum_l Re(conj(U_l) dU_l,k) / D_g
 *   D_g     = sum_l (s_l sum a)^2, which does not depend on the parameter (the weights are held).
 * Strehl and dStrehl_k are I and dI_k at (u, v) = (0, 0), where d = R and g_k = e_k, summed with fp64 sincospi in a
 *   fixed tree, as prt_frame_psf's Strehl ratio is, whether or not P is a pixel.
 * Accuracy: the phasor is prt_frame_psf's (eps above); a derivative carries, beside eps times |g_k|, the roundings of
 *   g_k itself: tests/psf_gradient_reference.py derives |dU~ - dU| <= 2 pi s [sum a |g_k| eps + sum a gamma_k] and
 *   states what is counted.
 *
 * prt_frame_psf_gradient: rows DEVICE, ld, n_rows as above; dphase DEVICE (K, n_selected), dpoint DEVICE (K, 2, n_selected)
 * or NULL, K in [1, 16]; wavelengths_um, world_unit_um, nx, ny, du, dv, centre_uv as prt_frame_psf takes them, with its
 * refusals; n_groups * n_wavelengths <= 16383; n_groups * n_wavelengths * nx * ny * 17 * 16 bytes (the slab of a call with
 * 16 parameters, whatever K is) may not pass the 256 MiB cap.  A selected row number outside [0, n_rows), or a selected
 * row of a wavelength that is not listed: PRT_ERR_ARG once the passes have run.
 * Out, DEVICE, overwritten: amplitude_out (n_groups, n_wavelengths, nx, ny, 2), U_l; damplitude_out (n_groups, K,
 * n_wavelengths, nx, ny, 2), dU_l,k; image_out (n_groups, n_wavelengths, nx, ny), the bucket's share of I;
 * dimage_out (n_groups, K, n_wavelengths, nx, ny); strehl_out (n_groups, 1 + K): Strehl, then dStrehl_k; record_out
 * (n_groups, n_wavelengths, 5): rays kept, n_missed, n_unfollowed, sum a, (s sum a)^2.  A group without kept rays is NaN.
 * workspace: prt_frame_psf_gradient_workspace_bytes(n_selected, n_groups, K, n_wavelengths) device bytes (-1 for arguments
 * the call would refuse).
 * Passes: a stable counting sort of an index of the selected rows into (group, wavelength) buckets; the staged rays and,
 * gathered through the index, the staged parameters; the fp64 Strehl sums; the Huygens sum, a grid of (pixel tile, ray
 * slice, bucket x chunk of at most 4 parameters) workgroups that read the ray tile and its parameter chunk through LDS,
 * the phase path of prt_frame_psf run once per (ray, pixel); the fold in slice order.  The slice count follows n_selected,
 * the pixel count, the bucket count and the device's CU count, a slice's rays its bucket's kept count -- never n_rows or
 * the frame's other rows, never K --, a parameter's arithmetic does not depend on the others in the call, and there are
 * no floating-point atomics: every output is the same, bit for bit, on every run, on any frame that holds the same
 * selected rows, and for a parameter alone or among sixteen (where the kept set is the same).  All arguments are checked
 * before a device is touched.  Stream-ordered; the call reads one status word back and so returns when the stream has
 * reached its end. */
int64_t prt_frame_psf_gradient_workspace_bytes(int64_t n_selected, int n_groups, int n_parameters, int n_wavelengths);
int prt_frame_psf_gradient(int device, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                           int64_t n_selected, const int64_t* group_first, int n_groups, int weight_column,
                           const double* opd, const double* pupil, const double* wavefront_groups, const double* dphase,
                           const double* dpoint, int n_parameters, const double* wavelengths_um, int n_wavelengths,
                           double world_unit_um, int nx, int ny, double du, double dv, const double* centre_uv,
                           double* amplitude_out, double* damplitude_out, double* image_out, double* dimage_out,
                           double* strehl_out, double* record_out, void* workspace, void* stream);

/* Monte Carlo tolerancing of the wavefront: the Strehl ratio of many perturbed systems, and the second moments of the
 * OPD and its derivatives, from the rows and the wavefront outputs of one prt_frame_opd_sensitivity (or
 * prt_frame_launch_sensitivity) call, without a re-trace.  Under the linear ray model the OPD of every ray moves linearly
 * in the parameters; the merit stays nonlinear in the OPDs (this is not Strehl + dStrehl . p).
 *
 * Definitions.
 * Rays: the selected rows of the sensitivity call, in its order (selected, group_first, weight_column and the wavelength
 *   as prt_frame_psf_gradient takes them).  opd DEVICE n_selected, that call's opd_out.  columns DEVICE (C, n_selected),
 *   1 <= C <= 20: x_c, the change of a ray's OPD per unit of column c, in world units (dopd_k, dfield_k, or a column a
 *   caller composed).
 * Rays kept: OPD finite, w finite and >= 0, all C column values finite.  There is one kept set for all columns and
 *   trials.  The others are counted per (group, wavelength): n_missed by the first two (the PSF's rule), n_unfollowed by
 *   the third; they contribute exactly nothing.
 * prt_frame_tolerance.  trials DEVICE (n_groups, M, C), 1 <= M <= 65536: p_gmc, the value of column c in trial m of group
 *   g.  Staged per kept ray of bucket (g, l), s_l = 1 / (lambda_l / world_unit_um): a = sqrt(w), c0 = OPD s_l,
 *   e_c = x_c s_l.  Per trial, in cycles, the columns in their order:
 *     phi_rm  = fma(e_C, p_C, ... fma(e_2, p_2, fma(e_1, p_1, c0)))
 *     U_glm   = s_l sum_r a exp(2 pi i phi_rm)      the turn fract(phi) in fp64, its cos and sin in fp32 (prt_frame_psf's
 *                                                    phase path from there on)
 *     Strehl_gm = sum_l |U_glm|^2 / D_g,  D_g = sum_l (s_l sum a)^2
 *   which is prt_frame_psf's Strehl ratio on the moved OPDs with the reference sphere held fixed.
 *   Out, DEVICE, overwritten: strehl_out (n_groups, M); amplitude_out (n_groups, n_wavelengths, M, 2), U_glm;
 *   record_out (n_groups, n_wavelengths, 5): rays kept, n_missed, n_unfollowed, sum a, (s sum a)^2.  A group without
 *   kept rays is NaN.  workspace: prt_frame_tolerance_workspace_bytes(n_selected, n_groups, C, n_wavelengths, M) device
 *   bytes (-1 for arguments the call would refuse).
 *   Passes: a stable counting sort of an index of the kept rays into (group, wavelength) buckets; the staged planes;
 *   sum a per slice in a fixed tree; the sum, a grid of (trial tile, ray slice, bucket) workgroups whose threads own 2
 *   trials each, coefficients in registers, the slice's rays read through LDS; partial sums into a slab (bucket,
 *   slice, trial) of 16 bytes each under the 256 MiB cap, the trials in several launches past it; the fold in slice
 *   order.  The slice count follows n_selected, the bucket count and the device's CU count, a slice's rays its bucket's
 *   kept count -- never n_rows, the frame's other rows, M or C --, and a trial's arithmetic does not depend on the
 *   other trials: every output is the same, bit for bit, on every run, on any frame that holds the same selected rows,
 *   for a trial alone or among 65536 at any place, and with a finite column appended whose trial values are all 0.
 * prt_frame_tolerance_moments.  With v = (1, y_0, .. y_C), y_0 = OPD and y_c = x_c (world units, not scaled by s), per
 *   group over the kept rays (of every wavelength): moments_out DEVICE (n_groups, 3 + (C + 2)(C + 3) / 2): rays kept,
 *   n_missed, n_unfollowed, sum w, sum w y_i (C + 1 values), then sum w y_i y_j for j <= i, the lower triangle by rows.
 *   Every entry is owned by one thread, summed in row order over chunks of 2048 selected rows of the group, the chunks
 *   added in order: no floating-point atomics, the same bits on every run.  workspace:
 *   prt_frame_tolerance_moments_workspace_bytes(n_selected, n_groups, C, n_wavelengths) device bytes (-1 as above).
 * Both: wavelengths_um, world_unit_um as prt_frame_psf takes them, with its refusals; n_groups * n_wavelengths <= 16383
 * (the moments entry also n_groups <= 65535).  A selected row number outside [0, n_rows), or a selected row of a wavelength
 * that is not listed: PRT_ERR_ARG once the passes have run.  All arguments are checked before a device is touched.
 * Stream-ordered; a call reads one status word back and so returns when the stream has reached its end.
 * Accuracy: tests/tolerance_reference.py derives the bound per ray, eps = EPS_TRIG + 2 pi F32_TURN + 2 pi u (C + 2)
 * (|c0| + sum_c |e_c p_c|), and carries it to U and to the Strehl ratio. */
int64_t prt_frame_tolerance_workspace_bytes(int64_t n_selected, int n_groups, int n_columns, int n_wavelengths,
                                            int n_trials);
int prt_frame_tolerance(int device, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                        int64_t n_selected, const int64_t* group_first, int n_groups, int weight_column,
                        const double* opd, const double* columns, int n_columns, const double* wavelengths_um,
                        int n_wavelengths, double world_unit_um, const double* trials, int n_trials,
                        double* strehl_out, double* amplitude_out, double* record_out, void* workspace, void* stream);
int64_t prt_frame_tolerance_moments_workspace_bytes(int64_t n_selected, int n_groups, int n_columns, int n_wavelengths);
int prt_frame_tolerance_moments(int device, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                                int64_t n_selected, const int64_t* group_first, int n_groups, int weight_column,
                                const double* opd, const double* columns, int n_columns, const double* wavelengths_um,
                                int n_wavelengths, double world_unit_um, double* moments_out, void* workspace,
                                void* stream);

/* Monte Carlo tolerancing of the geometric MTF: the OTF through focus, the second moments of the landing points and the
 * least-squares focus of many perturbed systems, from the rows, jacobian_out and slopes_out of one
 * prt_frame_launch_sensitivity call, without a re-trace.
 *
 * Definitions.  The rays, weights, kept set, centre C_g and staging are exactly prt_frame_mtf_gradient's:
 *   - one kept set for all K: a ray the MTF keeps whose 6 K tangent entries are finite;
 *   - the others are counted as n_missed / n_unfollowed and staged with w = 0 in place;
 *   - s, p, ds_k, dp_k as defined there;
 *   - C_g is the kept rays' centroid or a given point, held fixed.
 * Under the linear ray model, trial m (parameter changes t_mk, k < K <= 16) moves a ray to
 *     P_rm = p_r + sum_k t_mk dp_rk        S_rm = s_r + sum_k t_mk ds_rk        (2-vectors, accumulated in parameter order by fma)
 * Moments, per (group, trial), over the kept rays:
 *   - sum w; sum w P (2); sum w S (2); sum w P.P; sum w P.S; sum w S.S.
 *   - From them, in the plane shifted by delta:
 *     - the centroid is c_m(delta) = mean P + delta mean S;
 *     - the mean-square radius about it is var_P + 2 delta cov_PS + delta^2 var_S;
 *     - the least-squares focus is delta*_m = -cov_PS / var_S (0 where var_S is not > 0).
 * OTF, per (group, trial, plane f, azimuth, frequency), with k = nu (cos theta, sin theta) and the trial's focus shift delta_m:
 *     OTF_gm = sum w exp(-2 pi i k.(P_rm + (delta_f + delta_m) S_rm)) / sum w
 *   - delta_m is 0 without the focus compensator, and delta*_m with it.
 *   - The merit is fully nonlinear in the moved landing points.  This is the sensitivity-based Monte Carlo, as
 *     prt_frame_tolerance is for the phase.
 *   - The phasor is mtf_phasor of prt_mtf.hpp, applied to the moved ray {fma(delta_m, S, P), S, w} with the MTF's own
 *     (kc, ks, kc delta_f, ks delta_f) table.
 *   - With every t = 0 and delta_m = 0, each fma returns its addend.  The zero trial's per-ray phasors are therefore the
 *     bits k_mtf_sum / k_mtfg_sum form.
 *
 * prt_frame_mtf_tolerance: the leading arguments up to n_focus as prt_frame_mtf_gradient takes them, with its refusals;
 * trials DEVICE (n_groups, M, K), 1 <= M <= 65536, finite: t_gmk, the change of parameter k in trial m of group g;
 * compensate_focus: 0, or non-zero for delta_m = delta*_m, formed on the device in fp64 from the folded moments.
 * Out, DEVICE, overwritten: otf_out (n_groups, M, n_focus, n_azimuths, n_frequencies, 2); moments_out (n_groups, M, 8),
 * the sums above in that order; focus_out (n_groups, M), delta_m as it was applied; record_out (n_groups, 7): C_g (3),
 * sum w, rays kept, n_missed, n_unfollowed.  A group without kept rays, or with sum w = 0, is NaN in otf_out,
 * moments_out, focus_out and C_g (unless given), with its counts.  workspace:
 * prt_frame_mtf_tolerance_workspace_bytes(n_selected, n_groups, K, n_frequencies, n_azimuths, n_focus, M) device bytes
 * (-1 for arguments the call would refuse).
 * Passes: the centre, record and staging passes of prt_frame_mtf_gradient, its own kernels; then, per launch of whole
 * tiles of 256 trials: the moments, a grid of (ray slice, trial tile) workgroups whose threads own one trial each, its
 * coefficients in registers, the slice's rays read through LDS; the moments' fold in slice order with the focus shift;
 * the sum, a grid of (ray slice, trial tile, chunk of 8 outputs) workgroups that move the ray once per chunk and form
 * the phasor per output; the fold in slice order, normalised by the moments' sum w added in the same order, so the OTF
 * at nu = 0 is exactly 1.  A launch's partial sums -- slices * trials * (64 + 16 outputs of the launch) bytes -- stay
 * under the 256 MiB slab cap: the outputs run in launches of whole chunks of 8, as many as a tile of 256 trials leaves
 * room for, the trials in launches of whole tiles, and a call whose single tile cannot fit with one chunk (65535 groups)
 * is refused with PRT_ERR_ARG naming the cap: a result is never truncated.
 * A group's slices follow its count of selected rows, n_groups and the device's CU count -- never n_rows, the frame's
 * other rows, M, K, the outputs or the trial values --, a trial's arithmetic does not depend on the other trials, and
 * there are no floating-point atomics: every output is the same, bit for bit, on every run, on any frame that holds the
 * same selected rows, for a trial alone or among 65536 at any place, and with a finite parameter appended whose trial
 * values are all 0 (where the kept set is the same).  The arguments are checked before any kernel is launched (the
 * slab cap once the device's CU count is known).  Stream-ordered; the call returns when the stream has reached its end.
 * Accuracy: tests/mtf_tolerance_reference.py derives the bound per ray -- the MTF's phasor budget over the moved ray
 * plus 2 pi u times the counted roundings of the (4 K + 2)-term chains -- and a gamma_n bound for the moments. */
int64_t prt_frame_mtf_tolerance_workspace_bytes(int64_t n_selected, int n_groups, int n_parameters, int n_frequencies,
                                                int n_azimuths, int n_focus, int n_trials);
int prt_frame_mtf_tolerance(int device, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                            int64_t n_selected, const int64_t* group_first, int n_groups, int weight_column,
                            const double* jacobian, const double* slopes, int n_parameters, const double* reference,
                            const double* axes, const double* frequencies, int n_frequencies, const double* azimuths_deg,
                            int n_azimuths, const double* focus, int n_focus, const double* trials, int n_trials,
                            int compensate_focus, double* otf_out, double* moments_out, double* focus_out,
                            double* record_out, void* workspace, void* stream);

/* Monte Carlo tolerancing of the geometric enclosed energy: the energy within given radii and the radius that holds
 * given fractions, through focus, of many perturbed systems, from the rows, jacobian_out and slopes_out of one
 * prt_frame_launch_sensitivity call, without a re-trace.  It composes prt_frame_mtf_tolerance's moved ray with
 * prt_frame_energy's exact integer count.
 *
 * Definitions.
 * Rays, groups, staging: prt_frame_mtf_tolerance's -- rays, groups, axes, weights, the kept / missed / unfollowed rule,
 *   the held centre C_g (the kept rays' centroid, or a given point), the staged (p, s, w) a ray and (dp_k, ds_k) a ray and
 *   parameter.  The ray in trial m:
 *     P_rm = p_r + sum_k t_mk dp_rk        S_rm = s_r + sum_k t_mk ds_rk
 *   by the same fma chains in parameter order (mtft_move), so with the same bits as there.
 * Moments and refocus: k_mtft_moments and k_mtft_focus run as they are on the same staging and slices, so moments_out,
 *   focus_out and the first seven doubles of the record have the bits prt_frame_mtf_tolerance gives for the same
 *   sensitivity, trials and compensate_focus.  delta_m is 0 without the focus compensator, and delta*_m with it.  Plane f of
 *   trial m lies at delta = focus[f] + delta_m (one rounded sum).
 * Centre in a plane: with follow_centroid != 0 the trial's own centroid there, from the trial's own moments,
 *     c = m_P / m_0 + delta * (m_S / m_0)
 *   per component, the two quotients, the product and the sum each rounded on their own, without fused multiply-add: a
 *   float64 line on moments_out reproduces its bits.  This is what prt_frame_energy of the perturbed system measures
 *   from.  With follow_centroid == 0, c = 0: distances are measured from the held centre C_g -- the pixel or the fibre
 *   stays where it is while the spot walks off it.
 * Distance: d_rm(delta) is prt_frame_energy's distance of the moved ray {P_rm, S_rm}: x = (P + delta S) - c per
 *   component, product, sum and difference each rounded, then the shape's rule (PRT_ENERGY_CIRCLE, SQUARE, SLIT_E1,
 *   SLIT_E2); a coordinate that comes out NaN counts as d = +inf.
 * Integer weights: prt_frame_energy's power-of-two rule, once per call -- the weights do not change with the trial.  Per
 *   group, count = the group's number of selected rows (kept or not, so the sum cannot overflow whatever is kept),
 *   w_max = the largest staged weight = f 2^E with 0.5 <= f < 1 (an integer atomic max on the bit image),
 *   B = bit_length(count); q_r = (uint64) floor(ldexp(w_r, 62 - E - B)) and W_g = sum q_r by integer adds.  A row that is
 *   left out is staged with w = 0 and counts nothing.
 * Outputs, per (group, trial, plane):
 *     count[j]  = sum over d_r <= R_j of q_r, an exact uint64
 *     energy[j] = (double) count[j] / (double) W
 *     radius[k] = the smallest d among the trial's distances in that plane with sum over d_r <= d of q_r >= T_k,
 *                 T_k = clamp((uint64) ceil(phi_k * (double) W), 1, W): a ray's own distance, as prt_frame_energy defines it
 *   A group without weight (W = 0, or no kept rays) gives NaN in energy and radius, and counts of 0.
 *
 * prt_frame_energy_tolerance: the leading arguments up to axes as prt_frame_mtf_tolerance takes them, with its refusals;
 * shape and follow_centroid as prt_frame_energy's; radii (HOST, 0..256, finite, >= 0, strictly ascending), fractions
 * (HOST, 0..16, in (0, 1]), not both empty; focus (HOST, 1..256 finite shifts); trials DEVICE (n_groups, M, K),
 * 1 <= M <= 65536; compensate_focus as prt_frame_mtf_tolerance's.  Out, DEVICE, overwritten: count_out and energy_out
 * (n_groups, M, n_focus, n_radii) (may be NULL when n_radii == 0), radius_out (n_groups, M, n_focus, n_fractions) (may
 * be NULL when n_fractions == 0), moments_out (n_groups, M, 8), focus_out (n_groups, M), record_out (n_groups, 8):
 * prt_frame_mtf_tolerance's seven doubles, then W_g as its bit image (a uint64 below 2^62 read as a double: memcpy it
 * back).  workspace: prt_frame_energy_tolerance_workspace_bytes(n_selected, n_groups, K, n_radii, n_fractions, n_focus, M)
 * device bytes (-1 for arguments the call would refuse).
 * Passes: the centre, record and staging passes of prt_frame_mtf_gradient; the largest weight and the integer weights
 * over the staging's chunks; then, per launch of whole tiles of 256 trials: prt_frame_mtf_tolerance's moments and their
 * fold with the focus shift; the curve, a grid of (ray slice, trial tile, chunk of 8 (plane, radius) outputs,
 * plane-major) workgroups whose threads own one trial each, move the ray once, form the distance once per plane of the
 * chunk and add q where d <= R into uint64 registers, and its fold over the slices; the select, 21 passes of a
 * most-significant-bits-first multiway bisection on the 63-bit image of d (for non-negative doubles, bit order is
 * numeric order): per (ray slice, trial tile, (plane, 4 fractions)) a thread counts, per fraction, sum q [key <=
 * threshold_j] for the seven thresholds that split its prefix's interval in eight, and a fold over the slices appends
 * three bits -- no atomics, no LDS windows; after the last pass the prefix is the radius.  A launch's partial counts
 * -- slices * trials * 224 bytes at the least -- stay under the 256 MiB slab cap: the trials run in launches of whole
 * tiles, under them the curve's outputs in launches of whole chunks and the select's (plane, 4 fractions) items in
 * launches of as many as fit, and a call whose single tile cannot fit (more than 4681 groups) is refused with
 * PRT_ERR_ARG naming the cap: a result is never truncated.
 * A group's slices follow its count of selected rows, n_groups and the device's CU count -- never n_rows, the frame's
 * other rows, M, K, the output counts or the trial values --, every sum that decides an output is an integer sum and
 * there are no floating-point atomics: every output is the same, bit for bit, on every run, on any frame that holds the
 * same selected rows, for a trial alone or among 65536 at any place, with a finite parameter appended whose trial values
 * are all 0 (where the kept set is the same), and however the launches fall under the cap.  The arguments are checked
 * before any kernel is launched (the slab cap once the device's CU count is known).  Stream-ordered; the call returns
 * when the stream has reached its end.
 * Accuracy: tests/energy_tolerance_reference.py derives the band of a ray's distance from the counted roundings of the
 * moved point; every check of a count or a radius is then an exact integer inequality. */
int64_t prt_frame_energy_tolerance_workspace_bytes(int64_t n_selected, int n_groups, int n_parameters, int n_radii,
                                                   int n_fractions, int n_focus, int n_trials);
int prt_frame_energy_tolerance(int device, const double* rows, int64_t ld, int64_t n_rows, const int64_t* selected,
                               int64_t n_selected, const int64_t* group_first, int n_groups, int weight_column,
                               const double* jacobian, const double* slopes, int n_parameters, const double* reference,
                               const double* axes, int shape, int follow_centroid, const double* radii, int n_radii,
                               const double* fractions, int n_fractions, const double* focus, int n_focus,
                               const double* trials, int n_trials, int compensate_focus, uint64_t* count_out,
                               double* energy_out, double* radius_out, double* moments_out, double* focus_out,
                               double* record_out, void* workspace, void* stream);

/* Ray-aberration curves of the frame: each ray's row at a surface joined by ray id with the row where the ray was
 * launched (examples/lens_design.ipynb cells 12-13 join the two cuts of the frame with isin(id)), its transverse and
 * longitudinal aberration against its pupil coordinate, a Zernike fit of the fans and the zonal curve.
 *
 * prt_frame_launch_index: the frame is whole and generation-major, as prt_frame_optical_path requires; its first
 * n_launch_rows rows are generation 0.  index_out (DEVICE, int64, one per row) receives the row number of the
 * generation-0 row with the same id, -1 when there is none; a generation-0 row maps to itself.  Ids are integers in
 * [id0, id0 + n_ids); an id outside that range, one that is not an integer, or one repeated inside generation 0 gives
 * PRT_ERR_ARG through one status word read back (so the call returns when the stream has reached its end).  Two
 * passes: generation 0 writes its row numbers into a dense per-id table in a stream-ordered scratch block, then every
 * row gathers from it.
 *
 * Definitions of prt_frame_ray_aberrations.
 * Rays: rows at surface (NaN: any), in generation (NaN: any), in group g = floor(id / rays_per_source) with
 *   0 <= g < n_groups (rays_per_source <= 0: one group).  Each has an end point Q = (x1, y1, z1), a direction
 *   u = (x_tilt, y_tilt, z_tilt), a weight w (weight_column, or ones for -1) and a launch row (launch_index, of
 *   prt_frame_launch_index: rows is the whole frame) with start point L = (x0, y0, z0) and direction v.
 * Rays left out: a ray is left out and counted (n_missed) when its launch index is -1, when a value it needs is not
 *   finite (Q, u, w, the slope, and L or v by the pupil mode), when u.a == 0, or when w is not finite and >= 0.
 * Axes: (a, e1, e2), the 9 doubles of frame.pupil_axes().  The default is a = x, e1 = y, e2 = z.
 * Launch (pupil) coordinate h: pupil_mode 0 (position, collimated sources) h = ((L - O).e1, (L - O).e2) with O =
 *   launch_origin (HOST 3 doubles, NULL: the origin); pupil_mode 1 (direction, point sources) h = (v.e1, v.e2) / (v.a),
 *   and a ray with v.a == 0 is left out.  Normalised p = h / rho, rho = pupil_radius or, when 0, the group's largest
 *   |h| over the rays used (an extent of 0 gives rho = 1).
 * Reference point C_g: reference_mode 0 the weighted centroid of the group's Q; 1 the given point per group
 *   (reference, DEVICE (n_groups, 3)); 2 the chief ray: the Q of the used ray with the smallest |h|^2, ties to the first
 *   in row order.
 * Per ray: p, the transverse aberration eps = ((Q - C_g).e1, (Q - C_g).e2), the slope s = (u.e1, u.e2) / (u.a), and
 *   the longitudinal aberration la = x0 - x_tilt * y0 / y_tilt of the row at the surface (PRT_FRAME_AXIS_INTERCEPT's
 *   own device function), NaN when that is not finite; a ray with NaN la stays in everything that does not read la.  At
 *   a plane shifted by delta along a the transverse aberration is eps + delta s (the MTF's convention).
 * Fit: weighted least squares of the four targets eps1, eps2, s1, s2 on Z_1..Z_n_terms of p (Noll's order and RMS
 *   normalisation, as prt_frame_wavefront; n_terms <= 36).
 * Zones: n_zones (0..1024) rings of equal width in |p|, zone = min(floor(|p| n_zones), n_zones - 1).
 *
 * prt_frame_ray_aberrations: Out, DEVICE, overwritten: ray_out (capacity, 7) -- p1, p2, eps1, eps2, s1, s2, la of the
 * rays used, compacted in row order -- and row_out (capacity, int64), their row numbers in the frame; more rays used
 * than capacity gives PRT_ERR_ARG.  record_out (n_groups, 16): C_g (3), rho, rays used, rays left out, rays with finite
 * la, the chief ray's row (-1: none), sum w, sum w eps (2), sum w s (2), sum w |eps|^2, sum w eps.s, sum w |s|^2 (eps
 * about C_g, s raw).  normal_out (n_groups, n_terms (n_terms + 1) / 2 + 4 n_terms + 1): the upper triangle of Z^T W Z by
 * rows, Z^T W eps1, Z^T W eps2, Z^T W s1, Z^T W s2, sum w.  zone_out (n_groups, n_zones, 6; may be NULL for n_zones 0):
 * rays, then over the zone's rays with finite la sum w, sum w la, sum w la^2, then sum w |eps|^2 over all the zone's
 * rays, then the count of rays with finite la.  workspace: prt_frame_ray_aberrations_workspace_bytes(capacity, n_groups,
 * n_terms, n_zones) device bytes (-1 for arguments the call would refuse).  n_groups * max(n_zones, 1) * 8 bytes may
 * not pass the 64 MiB cap of the sort's counts.  The rays are sorted into (group, zone) buckets in row order by a
 * stable counting sort; every sum is formed per chunk of 4096 rays of a bucket in a fixed tree and the chunks are added
 * in order.  A bucket's chunks depend only on its count of rays used, never on n_rows, and there are no floating-point
 * atomics: every output is the same, bit for bit, on every run and on any frame that holds the same selected rows and
 * launch rows in the same order.  All arguments are checked before a device is touched.  Stream-ordered; the call
 * reads two counts back on the way and returns when the stream has reached its end. */
#define PRT_PUPIL_POSITION 0
#define PRT_PUPIL_DIRECTION 1
#define PRT_REFERENCE_CENTROID 0
#define PRT_REFERENCE_POINTS 1
#define PRT_REFERENCE_CHIEF 2
int prt_frame_launch_index(int device, const double* rows, int64_t ld, int64_t n_rows, int64_t n_launch_rows, double id0,
                           int64_t n_ids, int64_t* index_out, void* stream);
int64_t prt_frame_ray_aberrations_workspace_bytes(int64_t capacity, int n_groups, int n_terms, int n_zones);
int prt_frame_ray_aberrations(int device, const double* rows, int64_t ld, int64_t n_rows, const int64_t* launch_index,
                              double surface, double generation, double rays_per_source, int n_groups,
                              const double* reference, int reference_mode, const double* axes, int pupil_mode,
                              const double* launch_origin, double pupil_radius, int n_terms, int n_zones,
                              int weight_column, int64_t capacity, double* ray_out, int64_t* row_out,
                              double* record_out, double* normal_out, double* zone_out, void* workspace, void* stream);

/* Geometric encircled / ensquared energy of the frame, through focus, and its inverse: the radius that encloses a
 * fraction of the energy.  Like prt_frame_mtf it reads only each ray's end point and direction at the surface, so it
 * works on frames that hold the detector's rows alone.
 *
 * Definitions.
 * Rays, groups, rays left out (n_missed), axes (a, e1, e2), weight column, centre C_g (the weighted centroid of the
 *   group's Q, or a given point per group), p_r, s_r and the plane at shift delta: exactly prt_frame_mtf's, computed by
 *   its device code.  Ray r meets the plane at shift delta at x_r(delta) = p_r + delta s_r.
 * Centre of a plane: with follow_centroid != 0, distances at shift delta are measured from the plane's own weighted
 *   centroid c(delta) = pbar + delta sbar, with pbar = sum w p / sum w and sbar = sum w s / sum w; each sum is formed
 *   per chunk of 4096 rays of the group in a fixed tree and the chunks are added in order.  With follow_centroid == 0,
 *   c = 0: distances are measured from C_g.
 * Distance: x = (p + delta s) - c(delta), per component, the product, the sum and the difference each rounded, in that
 *   order, without fused multiply-add.  d_r(delta) is
 *     PRT_ENERGY_CIRCLE   sqrt(x1 * x1 + x2 * x2)   (each product rounded, then the sum, then the square root)
 *     PRT_ENERGY_SQUARE   max(|x1|, |x2|), a half-width
 *     PRT_ENERGY_SLIT_E2  |x1|   (a slit along e2)
 *     PRT_ENERGY_SLIT_E1  |x2|   (a slit along e1)
 *   d lies in [0, +inf].  An overflow gives +inf, which lies outside every finite radius and sorts last.  p, s and
 *   delta are finite, so d is never NaN as long as c(delta) is finite; where c(delta) itself overflows, a coordinate
 *   that comes out NaN counts as d = +inf.
 * Integer weights: every sum that decides an output is an integer sum, exact and independent of order.  Per group,
 *   m = rays used and w_max = the largest weight = f 2^E with 0.5 <= f < 1, B = bit_length(m); then
 *   q_r = (uint64) floor(ldexp(w_r, 62 - E - B)), so q_r < 2^(62 - B) and W = sum q_r < 2^62.  The scaling is a power of
 *   two: q is w truncated below w_max 2^-(61 - B) (41 bits at 1M rays), and a weight smaller than that counts 0.  With
 *   weight_column -1, w = 1.  W == 0, or no rays, gives NaN outputs.
 * Energy: EE_g(delta, R_j) = (double)(sum over d_r <= R_j of q_r) / (double) W, for radii R_j >= 0, finite and strictly
 *   ascending.
 * Enclosed radius: for a fraction 0 < phi_k <= 1, T_k = clamp((uint64) ceil(phi_k * (double) W), 1, W); the radius is
 *   the smallest d among the group's distances at that plane with sum over d_r <= d of q_r >= T_k.  It is a ray's own
 *   distance, not an interpolation.
 *
 * prt_frame_energy: reference DEVICE (n_groups, 3) or NULL for the centroids; axes HOST 9 doubles; radii (HOST, 0..4096),
 * fractions (HOST, 0..16), not both empty; focus (HOST, 1..256 shifts delta, finite).  n_groups * n_focus * n_radii * 8
 * bytes (the radius bins) and n_groups * n_focus * n_fractions * 16 KiB (the select's digit windows) may each not pass a
 * 256 MiB cap.  Out, DEVICE, overwritten: energy_out (n_groups, n_focus, n_radii) (may be NULL when n_radii == 0),
 * radius_out (n_groups, n_focus, n_fractions) (may be NULL when n_fractions == 0), record_out (n_groups, 10): C_g (3),
 * pbar (2), sbar (2), sum w, rays used, rays left out.  workspace: prt_frame_energy_workspace_bytes(n_rows, n_groups,
 * n_radii, n_fractions, n_focus) device bytes (-1 for arguments the call would refuse).  The energy is a cumulative
 * count: each ray's d is searched in the radii and q added to a (plane, radius) bin.  The radius is an exact selection: a
 * most-significant-digit-first radix select on the bit image of d (for non-negative doubles, bit order is numeric
 * order), six digits of 11, 11, 11, 10, 10 and 10 bits, after which the selected prefix is the radius.  No
 * floating-point atomics; partitions depend on a group's count of rays used and on the output counts, never on n_rows:
 * every output is the same, bit for bit, on every run and on any frame that holds the same selected rows in the same
 * order.  All arguments are checked before a device is touched.  Stream-ordered; the call returns when the stream has
 * reached its end. */
#define PRT_ENERGY_CIRCLE 0
#define PRT_ENERGY_SQUARE 1
#define PRT_ENERGY_SLIT_E1 2
#define PRT_ENERGY_SLIT_E2 3
int64_t prt_frame_energy_workspace_bytes(int64_t n_rows, int n_groups, int n_radii, int n_fractions, int n_focus);
int prt_frame_energy(int device, const double* rows, int64_t ld, int64_t n_rows, double surface, double generation,
                     double rays_per_source, int n_groups, const double* reference, const double* axes,
                     int weight_column, int shape, int follow_centroid, const double* radii, int n_radii,
                     const double* fractions, int n_fractions, const double* focus, int n_focus, double* energy_out,
                     double* radius_out, double* record_out, void* workspace, void* stream);

/* ---- ray-path analysis of the frame: which surfaces every ray met, in order (no counterpart upstream) -----------------
 * The passes above describe the spot at a surface and take "the rays there" as given.  The engine is a non-sequential
 * tracer: a ray may miss the lens and still reach the detector, be clipped by a stop, bounce between two mirrors or leave
 * through a lens's edge.  This pass joins the frame by ray id on the device and says how every ray got where it is and
 * where the others went (on the host: results.groupby("id")["surface"].agg(tuple) and what follows from it).
 *
 * Definitions.
 * Frame: whole and generation-major, as prt_frame_optical_path requires: rows_per_generation gives the generations'
 *   runs; ids are integers in [id0, id0 + n_ids), unique within a generation.
 * Surface values: the surface column of a row must be an integer in [0, 2^31).  The frame never holds -1, since
 *   _pyrayt.py:428-435 records living rays only.
 * Path of a ray: the tuple of the surface values of its rows in generation order.  A ray with a row in generation g > 0
 *   and none in g - 1 means the frame is not whole: PRT_ERR_ARG through the status word, like a repeated id.
 * Node: a distinct non-empty prefix of some ray's path.  The root (the empty prefix) is not a node.  A node has a parent
 *   (-1 for a first surface), a surface and a depth, which is the generation of the rows at it.
 * Node numbering: nodes are numbered 0 .. n_nodes - 1 in ascending order of their sequences compared as tuples -- Python's
 *   sorted(set(prefixes)).  That is depth-first preorder with children in ascending surface id, so a node's subtree is the
 *   contiguous range [k, k + subtree_size[k]).  This numbering is the contract; it does not depend on scheduling.
 * Groups: g = floor(id / rays_per_source), as elsewhere; rays_per_source <= 0 means one group.  A row of a group outside
 *   [0, n_groups) is left out of the per-group tables; it is still given its node.
 * Counts per (group, node): through -- rows at the node, i.e. rays whose path has this prefix; ended -- rays whose last
 *   row is at the node; dark -- ended rays whose last row has sqrt(x_tilt^2 + y_tilt^2 + z_tilt^2) <= 1e-8 (np.isclose's
 *   absolute tolerance at _pyrayt.py:415, where upstream decides that a ray was absorbed).  An ended ray that is not dark
 *   escaped or ran into the generation limit.
 * Weights: weight_column is a column index, or -1 for ones.  A weight that is not finite and >= 0 counts 0 and is tallied
 *   apart as n_bad_weight (rows).
 * Energy per (group, node): energy_through and energy_ended are sums of the weight of the rows at the node, respectively
 *   of the last rows of the rays that ended there.  The weights become integers by prt_frame_energy's power-of-two rule,
 *   computed by its device function: q = floor(ldexp(w, 62 - E - B)) with w_max = f 2^E the largest weight of the frame
 *   and B = bit_length(n_rows).  Every sum that reaches an output is then an integer sum, exact in any order, and is
 *   converted back to a double once at the end: ldexp((double) sum, -(62 - E - B)).  For integer weights with a total
 *   below 2^53 (the built-in sources' intensity 100) the energy is the exact sum.
 * Too many nodes: more than max_paths distinct nodes gives PRT_ERR_ARG with a message that names the cap, never a
 *   truncated table; nothing is ever written out of bounds.
 *
 * prt_frame_paths: max_paths in [1, 65536]; the tree is a table of 2^c >= 4 * max_paths slots, and n_groups * 2^c * 40
 * bytes (the per-(group, slot) tallies) may not pass a 256 MiB cap.  Out, overwritten: row_node_out DEVICE n_rows int32
 * (the node of each row's prefix), ray_node_out DEVICE n_ids int32 (the node where the ray ended; -1: the id has no row),
 * ray_last_row_out DEVICE n_ids int64 (the ray's last row; -1), node_out DEVICE (max_paths, 4) int32 (parent, surface,
 * depth, subtree size; -1 past n_nodes), count_out DEVICE (n_groups, max_paths, 3) int64 (through, ended, dark; 0 past
 * n_nodes), energy_out DEVICE (n_groups, max_paths, 2) double (through, ended), record_out HOST 4 int64: n_nodes, rays
 * with rows, n_bad_weight, deepest depth + 1.  workspace: prt_frame_paths_workspace_bytes(n_rows, n_ids, n_groups,
 * max_paths) device bytes (-1 for arguments the call would refuse).  One launch per generation in order on the stream;
 * a node's device-side name is the slot its (parent slot, surface) key took in the table with one compare-and-swap, so
 * no lane waits for another; every loop is bounded at launch.  The call reads the status word and the nodes' keys back
 * (12 bytes a node), orders them on the host and renumbers on the device.  No floating-point atomics: every output is
 * the same, bit for bit, on every run, and unchanged by any permutation of the rows inside a generation, apart from
 * row_node_out and ray_last_row_out being permuted with them.  All arguments are checked before a device is touched.
 * Stream-ordered; the call returns when the stream has reached its end. */
int64_t prt_frame_paths_workspace_bytes(int64_t n_rows, int64_t n_ids, int n_groups, int max_paths);
int prt_frame_paths(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation, int n_generations,
                    double id0, int64_t n_ids, double rays_per_source, int n_groups, int weight_column, int max_paths,
                    int32_t* row_node_out, int32_t* ray_node_out, int64_t* ray_last_row_out, int32_t* node_out,
                    int64_t* count_out, double* energy_out, int64_t* record_out, void* workspace, void* stream);

/* ---- Fresnel transmittance and polarisation of the frame (no counterpart upstream) ------------------------------------
 * refract() (tinygfx/g3d/operations.py:110-162) bends a ray and does nothing else: the intensity column leaves the source
 * at 100 and arrives at 100 however many glass surfaces the ray crossed.  This pass joins the frame by ray id, carries
 * two field vectors per ray through every interface its rows describe and gives every row the share of the launch
 * energy that is left.  The frame holds what Fresnel's equations need: the surface normal follows from the directions
 * before and after, so none has to be recorded.
 *
 * Definitions.
 * Frame: whole and generation-major.  Ids are integers in [id0, id0 + n_ids) and unique within a generation.  These are
 *   prt_frame_optical_path's rules; a repeated id, an id out of range, and a row in generation g without one in g - 1
 *   give PRT_ERR_ARG through the status word.
 * Interface quantities: for a ray's row in generation g >= 1 and its row in g - 1, ui and ut are the two rows'
 *   directions (x_tilt, y_tilt, z_tilt), normalised; ni, nt are their index values; S is row g - 1's surface.
 * Interface kind, decided from the rows alone, with eps_dir = 1e-12:
 *   lossless: S is in the caller's list of lossless surfaces (ideally coated; at most 64 ids).  The ray is treated as
 *     one of the kinds below, but with all amplitude coefficients of magnitude 1 (ts = tp = 1).
 *   undeviated: |ui - ut|^2 <= eps_dir and ni == nt.  The field and the transmittance pass unchanged.
 *   refraction: ni != nt.  N = ni ui - nt ut, normalised and oriented so that ci = ui.N > 0; ct = ut.N.  If not
 *     (ci > 0 and ct > 0) -- which covers values that are not finite -- the interface is invalid.  Otherwise, with
 *     a = ni ci, b = nt ct, c = nt ci, d = ni ct, the power-normalised amplitude coefficients are
 *     ts = 2 sqrt(a b) / (a + b) and tp = 2 sqrt(a b) / (c + d); ts^2, tp^2 are the power transmittances T_s, T_p.
 *   reflection: ni == nt and the ray is deviated: mirrors, and total internal reflection as the reference writes it (it
 *     keeps n1, operations.py:159-161).  N = ui - ut, normalised.  An ideal reflector: rs = -1, rp = +1.  The
 *     retardance of total internal reflection and of metals is NOT modelled here (prt_frame_fresnel_coated models it at
 *     the surfaces the caller coats); such interfaces are counted.
 *   invalid, besides: a direction that cannot be normalised (zero or not finite), an index that is not finite and > 0.
 * eps_dir = 1e-12: two rows of one undeviated ray differ by roundings, |ui - ut|^2 ~ 1e-31, and a real deviation below
 *   1e-6 rad is no optical interface, so any threshold between works for `undeviated`.  For normal incidence the choice
 *   balances two errors.  Below the threshold s and p are not told apart, which is wrong by the relative difference of
 *   ts and tp, O(sin^2 theta) <= 1e-12: the suite's own bar.  Above it s = ui x N is a difference of products of size 1
 *   with a result of size sin theta, so its direction is good to 1e-16 / sin theta <= 1e-10 at the threshold and to
 *   1e-14 from sin theta = 0.01 on; within the transverse plane that error is harmless (it multiplies ts - tp), along
 *   the ray it is what |E.ut| / |E| can reach.
 * Field update: s = ui x N normalised, pi = ui x s, pt = ut x s; E' = ts (E.s) s + tp (E.pi) pt, for a reflection with
 *   rs, rp.  At normal incidence (|ui x N|^2 <= eps_dir) s and p coincide: refraction E' = ts E, reflection E' = -E.
 * Field state and transmittance: each ray carries two real field vectors Ea, Eb.
 *   Unpolarised input (the default): at generation 0 they are an orthonormal pair perpendicular to the launch
 *     direction u0: Ea = u0 x e normalised, with e the world axis of the smallest |u0| component (ties to the first),
 *     Eb = u0 x Ea.  T = (|Ea|^2 + |Eb|^2) / 2.
 *   Polarised input (a world vector v, normalised by the call): Ea = v minus its component along u0, normalised when
 *     its squared length is above eps_dir, Eb = 0.  T = |Ea|^2.  A ray with v parallel to u0 is invalid.
 *   Generation-0 rows have T = 1.  A row's T is computed from the updated fields by the formula above at a refraction
 *   that is not lossless; at every other interface (undeviated, reflection, lossless: all coefficients of magnitude 1)
 *   it is the previous row's T handed on as it is, since a rotation keeps |E| only to rounding: a mirror or a coated
 *   surface leaves T unchanged to the bit.
 *   An invalid interface makes the ray's T and field NaN from that row on, and the ray is counted once.
 * Arithmetic: every step is rounded on its own (no FMA contraction), dot products as (x x' + y y') + z z', in the order
 *   the kernel writes them, so that a numpy restatement can follow it operation for operation.
 * Counters: interfaces that are reflections, interfaces whose S is in the lossless list (of any kind), undeviated
 *   interfaces, invalid rays.
 *
 * prt_frame_fresnel: polarization HOST 3 doubles (finite, not zero) or NULL for unpolarised input; lossless HOST
 * n_lossless <= 64 surface ids.  Out, overwritten: transmittance_out DEVICE n_rows doubles; field_out DEVICE (6, n_rows)
 * doubles, Ea then Eb by component, or NULL; record_out HOST 4 int64: the counters.  workspace:
 * prt_frame_fresnel_workspace_bytes(n_rows, n_ids) device bytes (-1 for arguments the call would refuse): per id the
 * fields (six planes), its previous row and a generation stamp, 60 bytes.  Caps: n_ids in [1, 2^31], a generation's
 * rows fit one launch, at most 64 lossless surfaces; PRT_ERR_ARG otherwise, never a truncated result, and nothing is
 * ever written out of bounds.  One launch per generation in order on the stream, one row a thread; no two lanes touch
 * one ray's state, there are no floating-point atomics and no floating-point sums across rays, the only atomics are the
 * stamp and the integer counters (one add per workgroup): every output is the same, bit for bit, on every run, and
 * unchanged by any permutation of the rows inside a generation apart from being permuted with them.  All arguments are
 * checked before a device is touched.  Stream-ordered; the call reads the status word and the counters back and so
 * returns when the stream has reached its end. */
int64_t prt_frame_fresnel_workspace_bytes(int64_t n_rows, int64_t n_ids);
int prt_frame_fresnel(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation, int n_generations,
                      double id0, int64_t n_ids, const double* polarization, const int64_t* lossless, int n_lossless,
                      double* transmittance_out, double* field_out, int64_t* record_out, void* workspace, void* stream);

/* ---- Thin-film coatings, metals and the phase of total internal reflection in the Fresnel pass -------------------------
 * prt_frame_fresnel knows the bare dielectric interface and the ideal surface.  prt_frame_fresnel_coated is the same
 * pass with complex fields and, at the surfaces the caller coats, the coefficients of a layer stack.  prt_frame_fresnel
 * and its outputs are left exactly as they are.
 *
 * Definitions.
 * Coating: belongs to one or more surface ids and has three parts.  layers: 0 to 16 pairs (material, thickness), listed
 *   from the AMBIENT side to the SUBSTRATE side; thickness in the unit of the frame's wavelength column (micrometres, as
 *   the Sellmeier glasses take them).  ambient: a material, default the constant 1.0.  substrate: a material or none.
 *   A material is a real or complex constant n + ik, with k >= 0 absorbing (fields as exp(-i omega t)), or a function of
 *   the wavelength.  The host evaluates materials on the distinct wavelengths of the frame; their values travel as a
 *   table, and the kernel looks a row's wavelength up in it exactly.
 * Coated interface: a refraction or a reflection (the kinds of prt_frame_fresnel, decided as there) at a surface S that
 *   has a coating.  An undeviated ray passes a coated surface as it passes any other.  The wavelength is that of the
 *   ray's row in generation g - 1.
 * Which side the ray comes from: the ray arrives from the ambient side iff its ni equals the real part of ambient at its
 *   wavelength; an exact comparison.  Otherwise it arrives from the substrate side and the layers are traversed in
 *   reverse.
 * The far medium: refraction (ni != nt): nt from the rows.  Reflection (ni == nt, deviated) from the ambient side:
 *   substrate; if there is none the interface is invalid.  Reflection from the substrate side: ambient.  So a bare face
 *   of total internal reflection is a coating without layers and with ambient 1.0 on a prism face; an aluminium mirror
 *   is a coating without layers and with substrate 1.2 + 7.0i; a protected-silver mirror is one layer over a complex
 *   substrate.
 * Coefficients: the Snell invariant is ni sin thetai, with N and cos thetai = ui.N as prt_frame_fresnel has them and
 *   sin^2 thetai = |ui x N|^2.  Per layer j, cos thetaj = sqrt(1 - (ni sin thetai / nj)^2): the square root is complex,
 *   on the branch with Im(nj cos thetaj) >= 0; the far medium's cosine likewise.  The phase is
 *   deltaj = 2 pi nj dj cos thetaj / lambda.  The tilted admittances are eta_s = n cos theta and eta_p = n / cos theta.
 *   Per polarisation, (B, C) = M_1 ... M_L (1, eta_far) with the characteristic matrix of a layer
 *   M_j = [[cos deltaj, -i sin deltaj / eta_j], [-i eta_j sin deltaj, cos deltaj]], layer 1 next to the near medium;
 *   r = (eta_near B - C) / (eta_near B + C), t = 2 eta_near / (eta_near B + C), eta_near of the real ni.
 *   Transmitted coefficients are power-normalised, as ts, tp of prt_frame_fresnel are: ts, tp = t sqrt(Re eta_far /
 *   Re eta_near) of their polarisation; then |E|^2 carries power and the phase is kept.  Reflected coefficients are
 *   rs = r_s and rp = -r_p: the signs in the basis s, pi, pt, in which a substrate of infinite |n| gives the ideal
 *   mirror of prt_frame_fresnel, rs = -1, rp = +1.  Without layers ts, tp are those of prt_frame_fresnel.
 *   A finite stack never makes an interface invalid by its thickness or absorption: the kernel carries every M_j scaled
 *   by exp(-Im deltaj), which r does not see, and multiplies t by exp(-sum Im deltaj) at the end; a layer that is opaque
 *   many times over (a metal film of micrometres, an evanescent gap of many waves) gives the r of its bulk material and
 *   t = 0, not NaN.  Conditioning: the far medium's n cos theta is sqrt(n^2 - q) of the Snell invariant, not the cosine
 *   of the transmitted row, so next to the far medium's critical angle, and for a ray that leaves at grazing exit, one
 *   ulp of q moves n cos theta by 1.1e-16 n^2 / (2 n cos theta), and r, t with it (t, which goes with its square
 *   root, by more): at 1e-9 relative from the critical angle the coefficients are defined to some 1e-9, no better.
 *   A layer next to ITS critical angle is no such case: M_j is even in n cos thetaj.
 * Fields: Ea, Eb are complex 3-vectors.  The field update is prt_frame_fresnel's with complex cs, cp:
 *   E' = cs (E.s) s + cp (E.pi) pt, the dot products without conjugation (s, pi, pt are real); at normal incidence
 *   E' = ts E, respectively E' = rs E.  T = (|Ea|^2 + |Eb|^2) / 2, respectively |Ea|^2, with complex moduli.  T is
 *   computed from the fields at every coated interface.
 * Surfaces without a coating follow prt_frame_fresnel's rules and arithmetic, operation for operation, on the real and
 *   on the imaginary parts, `lossless` and the handing-on of T included; |E|^2 is the real parts' sum plus the imaginary
 *   parts' sum.  Without coatings and with a real polarization, T and the real parts are prt_frame_fresnel's bits and the
 *   imaginary parts are zero.
 * Polarised input: polarization is a complex 3-vector, (0, 1, i) for circular input.  It is normalised with the complex
 *   norm; the transverse part is taken as in prt_frame_fresnel, on both parts, and normalised with the complex norm.
 * Invalid interfaces, besides prt_frame_fresnel's: a reflection that needs a substrate and has none; a NaN or
 *   non-positive (or infinite) wavelength at a coated interface; a table value of the far medium or of a layer crossed
 *   that is not finite, or coefficients that are not finite (a far medium exactly at its critical angle, an index
 *   whose square overflows: never a finite thickness or absorption, see Coefficients).  The ray is NaN from there on and
 *   counted once.
 * Refused calls: a row's wavelength that is not in the table at a coated interface sets a status bit and the call
 *   returns PRT_ERR_ARG: the caller's table was wrong.
 * Counters: prt_frame_fresnel's four, then coated interfaces, then interfaces of total internal reflection: a valid
 *   coated reflection whose far index is real and below the Snell invariant, so that |r| = 1 by construction.
 * Caps, PRT_ERR_ARG beyond them, never a truncated result: 64 coated surface ids, 16 coatings, 16 layers, 256 distinct
 *   wavelengths (a continuous Monte-Carlo spectrum is out of scope).
 *
 * prt_frame_fresnel_coated: the arguments of prt_frame_fresnel, except: polarization HOST 6 doubles (real part, then
 * imaginary part) or NULL.  The HOST tables: coated_surfaces n_coated <= 64 surface ids, none listed twice, none also
 * lossless; surface_coating n_coated int32, the coating of each, in [0, n_coatings); n_coatings <= 16; layer_counts
 * n_coatings int32 in [0, 16]; has_substrate n_coatings int32; thicknesses (n_coatings, 16) doubles, finite and >= 0 for
 * the layers counted; wavelengths n_wavelengths <= 256 doubles, finite, > 0, ascending and distinct; indices
 * (n_coatings, 18, n_wavelengths, 2) doubles: per coating the slots ambient, layer 0..15, substrate, per wavelength
 * (real, imaginary).  Out, overwritten: transmittance_out DEVICE n_rows doubles; field_out DEVICE (12, n_rows) doubles or
 * NULL: the real parts of Ea then Eb by component, then the imaginary parts; record_out HOST 6 int64: the counters.
 * workspace: prt_frame_fresnel_coated_workspace_bytes(n_rows, n_ids) device bytes (-1 for arguments the call would
 * refuse): the tables at their caps, and per id the fields (twelve planes), its previous row and a generation stamp, 108
 * bytes.  The guarantees of prt_frame_fresnel hold: one launch per generation in order on the stream, one row a thread,
 * no two lanes touch one ray's state, no floating-point atomics and no sums across rays, nothing read or written out of
 * bounds on a refused frame, every output the same bits on every run and under any permutation of a generation's rows.
 * All arguments, the tables included, are checked before a device is touched. */
int64_t prt_frame_fresnel_coated_workspace_bytes(int64_t n_rows, int64_t n_ids);
int prt_frame_fresnel_coated(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                             int n_generations, double id0, int64_t n_ids, const double* polarization,
                             const int64_t* lossless, int n_lossless, const int64_t* coated_surfaces,
                             const int32_t* surface_coating, int n_coated, int n_coatings, const int32_t* layer_counts,
                             const int32_t* has_substrate, const double* thicknesses, const double* wavelengths,
                             int n_wavelengths, const double* indices, double* transmittance_out, double* field_out,
                             int64_t* record_out, void* workspace, void* stream);

/* ---- Ghost rays: Fresnel reflections spawned from the frame (no counterpart upstream) ---------------------------------
 * prt_frame_fresnel says how much energy every refracting surface takes from a ray; this pass says where it goes.  At
 * every refraction a ray's rows describe, at the surfaces the caller lists, one reflected child ray leaves with the
 * energy that did not go through.  The children are an ordinary (13, n) ray set for prt_trace, ordered so that every
 * (parent group, surface) is a "source" of the per-source frame passes.  The trace is not touched.
 *
 * Definitions.
 * Frame: whole and generation-major, ids as prt_frame_fresnel wants them; k = id - id0 is the ray's number.
 * transmittance: n_rows doubles, what prt_frame_fresnel or prt_frame_fresnel_coated wrote for this frame.  The pass
 *   takes 1 - T for R: it holds for the bare interface and for stacks of real layer indices, not for absorbing ones.
 * Interface: for a ray's row j in generation g >= 1 and its row p in g - 1 (the join of prt_frame_fresnel: per id a stamp
 *   and its last row), ni = index[p], nt = index[j], S = surface[p].  A child is spawned at the end of row p when the join
 *   is good; ni and nt are finite, > 0 and unequal (a refraction: mirrors, total internal reflection and undeviated rays
 *   spawn nothing); S is in the list; t[p] and t[j] are finite; and e = intensity[p] * (t[p] - t[j]) has e > 0 and
 *   e >= min_intensity.
 * Child, every product and sum rounded on its own (no FMA contraction), dot products as (x x' + y y') + z z':
 *     ui = unit(tilt[p]); ut = unit(tilt[j]); m = ni ui - nt ut; N = unit(m); ci = dot(ui, N)
 *     ur = ui - (2.0 ci) N                                    (not renormalised)
 *     origin = (x1, y1, z1)[p] + ray_offset ur, w = 1; direction = (ur, 0)
 *     generation 0, intensity e, wavelength[p], index ni
 *   A child with a component that is not finite is not spawned and is counted (invalid).
 * Buckets, groups, ids: bucket = parent_group * n_surfaces + (position of S in the list), parent_group =
 *   floor(k / rays_per_group) (0 when rays_per_group <= 0, which needs n_groups = 1); a parent_group >= n_groups is
 *   PRT_ERR_ARG.  The marked rows p are put in order of their buckets, in frame order inside a bucket, by the stable
 *   counting sort of the image passes.  The non-empty buckets, numbered 0 .. G' - 1 in bucket order, are the groups of the
 *   child set; stride = the largest bucket's count; a child's id = group * stride + (its rank in its bucket).  Child c
 *   of the ray set stands at column c in that order.
 * Open rows: a ray that leaves the system has no later row, so the interface at the end of its last row is not seen.
 *   Rows that end on a listed surface and have no successor are counted as open.
 * Counters (record_out, HOST 8 int64): spawned; dropped (0 < e < min_intensity); dark (e <= 0 at a listed refraction with
 *   finite t); invalid; open; then G', stride, 0.
 *
 * prt_frame_ghosts_count: surfaces HOST n_surfaces in [1, 64] distinct ids; n_groups * n_surfaces <= 65535;
 * min_intensity finite >= 0, ray_offset finite.  Out: bucket_count_out HOST n_groups * n_surfaces int64, the children of
 * every bucket; record_out.  workspace: prt_frame_ghosts_count_workspace_bytes(n_rows, n_ids, n_buckets) device bytes
 * (-1 for arguments the call would refuse); it keeps what prt_frame_ghosts_emit needs and must be handed to it unchanged.
 * prt_frame_ghosts_emit: the same rows, n_rows (all generations), n_ids, transmittance, ray_offset and n_buckets; n_children
 * = the sum of bucket_count_out (anything else: PRT_ERR_ARG, as is a count_workspace of another call).  Out, overwritten:
 * rays_out DEVICE (13, ld_rays) doubles, ld_rays >= n_children; parent_row_out DEVICE n_children int64, the row p of
 * every child.  workspace: prt_frame_ghosts_emit_workspace_bytes(n_rows, n_buckets) device bytes of its own; the count's
 * workspace is only read, so it serves any number of emits.
 * Guarantees: the marking is one launch per generation in order on the stream, one row a thread, 256 threads a
 * workgroup; no two lanes write one row's mark; no floating-point atomics, no floating-point sums across rows; the
 * counters are integers, summed by ballot and LDS and added with one atomic per workgroup: every output is the same
 * bits on every run, and a permutation of the rows inside a generation permutes the children inside their buckets and
 * changes nothing else.  Nothing is read or written out of bounds on a refused frame.  All arguments are checked before
 * a device is touched.  Stream-ordered; both calls return when the stream has reached their end. */
int64_t prt_frame_ghosts_count_workspace_bytes(int64_t n_rows, int64_t n_ids, int n_buckets);
int prt_frame_ghosts_count(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                           int n_generations, double id0, int64_t n_ids, const double* transmittance,
                           const int64_t* surfaces, int n_surfaces, double rays_per_group, int n_groups,
                           double min_intensity, double ray_offset, int64_t* bucket_count_out, int64_t* record_out,
                           void* workspace, void* stream);
int64_t prt_frame_ghosts_emit_workspace_bytes(int64_t n_rows, int n_buckets);
int prt_frame_ghosts_emit(int device, const double* rows, int64_t ld, int64_t n_rows, int64_t n_ids,
                          const double* transmittance, double ray_offset, int n_buckets, int64_t n_children,
                          const void* count_workspace, double* rays_out, int64_t ld_rays, int64_t* parent_row_out,
                          void* workspace, void* stream);

/* ---- Scattered rays: stray light spawned from the frame by BSDF (no counterpart upstream) --------------------------------
 * The ghost pass follows the specular reflections of refracting surfaces; this pass follows surface scatter.  Every row
 * that lands on a listed surface sends N = rays_per_hit child rays back into the half space it came from (reflective
 * scatter, BRDF), each with the energy its surface's BSDF gives the direction drawn for it.  The children are an ordinary
 * (13, n) ray set for prt_trace, ordered so that every (parent group, surface) is a "source" of the per-source frame
 * passes.  The trace is not touched.
 *
 * Definitions.  Every product and sum is rounded on its own (no FMA contraction), in the order written; dot(a, b) =
 * (ax bx + ay by) + az bz; unit(v) = v / sqrt(dot(v, v)) component by component.
 * Which rows spawn: row p spawns when surface[p] is in the list, whatever happens to its ray afterwards (absorbed,
 *   refracted, reflected): no join by ray id, no open rows.  id[p] and generation[p] of such a row are integers >= 0
 *   (id < 2^53, generation < 2^31), PRT_ERR_ARG otherwise.  The frame need not be whole.
 * Geometry of row p: x = (x1, y1, z1)[p]; ui = unit(tilt[p]); n = the world normal of the surface's primitive at
 *   (x, 1) as the trace computes it (its 4x4 products are fma chains, the normalisations IEEE divisions by one length),
 *   times normal_scale, negated when dot(n, ui) > 0; I = intensity[p].  The primitive is the entry of `prims` (HOST
 *   n_prims prt_prim sorted by surface_id, ids distinct: the table of prt_frame_sensitivity) with the surface's id,
 *   found by bisection; a listed surface that is not there is PRT_ERR_ARG.
 * BSDF: shift-invariant, f(b), b = |beta - beta0|, beta and beta0 the projections of the scattered and of the specular
 *   direction on the tangent plane; beta0 is the projection of ui, so with d = uo - ui, dn = dot(d, n),
 *   w = d - dn n:  b = sqrt(dot(w, w)) in [0, 2].  A model is a table of T + 1 = 1025 doubles, finite and >= 0, uniform
 *   in u = sqrt(b / 2):  q = sqrt(0.5 b) * 1024.0; k = (int)q when q < 1023.0, else 1023;
 *   f = tab[k] + (q - k) * (tab[k + 1] - tab[k]); f = NaN when q is not >= 0 (b not a number).  tables: HOST
 *   n_models x 1025 doubles, n_models in [1, 16]; models[s] in [0, n_models) is the model of surfaces[s].
 * Random numbers: Philox4x32-10 (multipliers D2511F53, CD9E8D57; key increments 9E3779B9, BB67AE85) on the counter
 *   (low 32 bits of id, high 32 bits of id, generation, child) under the key (low, high 32 bits of seed); from its
 *   output words x0..x3:  u1 = (((x0 << 32) | x1) >> 11) * 2^-53, u2 likewise from x2, x3;  a = 2.0 u1 - 1.0,
 *   b = 2.0 u2 - 1.0.  A child's sample depends on (seed, id, generation, child) alone.
 * Sampling: s = a a + b b; a sample with s >= 1 (not s < 1) is rejected: counted, no child.  The basis of a unit vector
 *   m (Duff et al. 2017):  sg = copysign(1.0, mz); h = -1.0 / (sg + mz); g = (mx my) h; sx = sg mx;
 *   t1 = (1.0 + (sx mx) h, sg g, -sx); t2 = (g, sg + (my my) h, -my).
 * target == NULL, the cosine-weighted hemisphere: c = sqrt(1.0 - s), rejected when c is not > 0; (t1, t2) of n;
 *   uo = (a t1 + b t2) + c n per component (not renormalised); E = ((4.0 I) f) / N.  With the rejections the density is
 *   cos(theta_o) / 4 per solid angle; for f = rho / pi the expected sum of the children's energies is rho I.
 * target != NULL (HOST 13 doubles: centre (3), normal (3), e1 (3), e2 (3), radius R), a disk: (e1, e2) is the basis
 *   above of the normal, formed by the caller; the normal is a unit vector to 1e-12, R > 0.
 *   y = centre + R (a e1 + b e2) per component; v = y - x; r2 = dot(v, v); uo = v / sqrt(r2) per component;
 *   cos_o = dot(n, uo); a child with cos_o <= 0 is below the horizon: counted, no child; cos_t = |dot(normal, uo)|;
 *   E = ((((I f) cos_o) cos_t) (4.0 (R R))) / (N r2).
 * Child: origin = x + ray_offset uo, w = 1; direction = (uo, 0); generation 0; intensity E; wavelength[p]; index[p]
 *   (the medium the ray travelled in).  Fates, in this order: rejected; below; dark (E <= 0); dropped (E <
 *   min_intensity); invalid (E, the wavelength, the index or a component of origin or direction is not finite: a cube
 *   normal on an edge, a row without a direction); spawned.
 * Items, buckets, groups, ids: item p N + c is child c of row p.  bucket = parent_group * n_surfaces + (place of the
 *   surface in the list), parent_group = floor(id / rays_per_group) (0 when rays_per_group <= 0, which needs n_groups
 *   = 1); a parent_group that is not below n_groups is PRT_ERR_ARG.  The spawned items are put in order of their
 *   buckets, in item order (row, then child) inside a bucket, by the stable counting sort of the image passes.  The
 *   non-empty buckets, numbered 0 .. G' - 1, are the groups of the child set; stride = the largest bucket's count; a
 *   child's id = group * stride + (its rank in its bucket).
 * Counters (record_out, HOST 8 int64): spawned, rejected, below, dark, dropped, invalid; then G', stride.
 *
 * prt_frame_scatter_count: rows DEVICE (15, ld), n_rows <= ld; rays_per_hit in [1, 64], n_rows * rays_per_hit < 2^31 - 1;
 * surfaces HOST n_surfaces in [1, 64] distinct ids; n_groups * n_surfaces <= 65535; min_intensity finite >= 0,
 * ray_offset finite.  Out: bucket_count_out HOST n_groups * n_surfaces int64, the children of every bucket; record_out.
 * workspace: prt_frame_scatter_count_workspace_bytes(n_rows, rays_per_hit, n_buckets, n_models) device bytes (-1 for
 * arguments the call would refuse); it keeps what prt_frame_scatter_emit needs -- the marks, the arguments, the listed
 * primitives and the tables -- and must be handed to it unchanged.
 * prt_frame_scatter_emit: the same rows, n_rows, rays_per_hit, n_buckets and n_models; n_children = the sum of
 * bucket_count_out (anything else: PRT_ERR_ARG, as is a count_workspace of another call).  Out, overwritten: rays_out
 * DEVICE (13, ld_rays) doubles, ld_rays >= n_children; parent_row_out DEVICE n_children int64 and child_out DEVICE
 * n_children int32: the row p and the number c of every child.  workspace:
 * prt_frame_scatter_emit_workspace_bytes(n_rows, rays_per_hit, n_buckets) device bytes of its own; the count's
 * workspace is only read, so it serves any number of emits.
 * Guarantees: one item a thread, 256 threads a workgroup; no floating-point atomics, no floating-point sums across
 * items; the counters are integers, summed by ballot and LDS and added with one atomic per workgroup: every output is
 * the same bits on every run, a child's bits (its id apart) do not depend on where its row stands in the frame or on
 * the other rows, and its direction does not depend on N.  All arguments are checked before a device is touched.
 * Stream-ordered; both calls return when the stream has reached their end. */
int64_t prt_frame_scatter_count_workspace_bytes(int64_t n_rows, int rays_per_hit, int n_buckets, int n_models);
int prt_frame_scatter_count(int device, const double* rows, int64_t ld, int64_t n_rows, const prt_prim* prims,
                            int n_prims, const int64_t* surfaces, const int* models, int n_surfaces,
                            const double* tables, int n_models, const double* target, int rays_per_hit, uint64_t seed,
                            double rays_per_group, int n_groups, double min_intensity, double ray_offset,
                            int64_t* bucket_count_out, int64_t* record_out, void* workspace, void* stream);
int64_t prt_frame_scatter_emit_workspace_bytes(int64_t n_rows, int rays_per_hit, int n_buckets);
int prt_frame_scatter_emit(int device, const double* rows, int64_t ld, int64_t n_rows, int rays_per_hit, int n_buckets,
                           int n_models, int64_t n_children, const void* count_workspace, double* rays_out,
                           int64_t ld_rays, int64_t* parent_row_out, int* child_out, void* workspace, void* stream);

/* ---- Sensitivities of the frame: differential ray tracing (no counterpart upstream) -----------------------------------
 * d(landing point)/d(parameter) of every ray, for K rigid motions of surfaces, from ONE trace: the rows of a ray, joined
 * by id, are its whole path, `surface` names the primitive each segment ended on, and the surface table below says what
 * that primitive is.  A tangent (do, dd) per ray and parameter is pushed through the recorded interfaces.  The result is
 * the derivative AT FIXED PATH, as in every differential ray trace: a ray whose sequence of surfaces changes under the
 * motion (the edge of an aperture) is outside it.  Sources do not move here.  Shape and index parameters:
 * prt_frame_design_sensitivity, below; the optical path, the OPD and its Zernike terms: prt_frame_opd_sensitivity, below
 * that; motions of the rays' launch and changes of their wavelength: prt_frame_launch_sensitivity, below that.
 *
 * Definitions.
 * Frame: whole and generation-major, ids as prt_frame_optical_path wants them (a repeated id, an id out of range, a row
 *   in generation g without one in g - 1: PRT_ERR_ARG through the status word).
 * Surface table: n_surfaces prt_prim records (type, normal_scale, params, minv; `material` is not read), ascending in
 *   surface_id, ids distinct.
 * Parameter k: a twist (v, w, c), 9 doubles, and a list of at most 64 surface ids of the table (parameter_ids
 *   [parameter_first[k], parameter_first[k + 1])).  A moved surface has the velocity u = v + w x (x - c) at x per unit
 *   parameter; every other surface has u = 0.
 * A row: start o = (x0, y0, z0), unit direction d = tilt / |tilt|, landing point x = (x1, y1, z1), t = (x - o).d, and n
 *   the world normal of the row's primitive at x, as the trace computes it, turned against d (n.d < 0).
 * Landing, per parameter, from the segment's (do, dd):  dt = n.(u - do - t dd) / (n.d),  dx = do + t dd + d dt.
 *   Generation 0: do = dd = 0.
 * Normal: dn = w x n (only where the surface is moved) + W (dx - u), W = s (I - n n^T) A^T H A / |A^T g|, A the 3x3 of
 *   minv, g half the gradient of the primitive's implicit function in object coordinates at A x + b, H half its Hessian
 *   (sphere: I; cylinder wall and paraboloid: diag(1, 1, 0); planes, cube faces and end caps: 0), s = normal_scale,
 *   negated where n was turned.
 * Interface between a ray's row in g - 1 (d, n, dn there, index ni) and its row in g (d', index nt), eps_dir = 1e-12:
 *   refraction, ni != nt: mu = ni / nt, ci = -n.d, ct = sqrt(1 - mu^2 (1 - ci^2)), gamma = mu ci - ct;
 *     dci = -(dn.d + n.dd), dct = mu^2 ci dci / ct, dd' = mu dd + (mu dci - dct) n + gamma dn;
 *   reflection, ni == nt and |d - d'|^2 > eps_dir: dd' = dd - 2 [(dd.n + d.dn) n + (d.n) dn];
 *   undeviated: dd' = dd.
 *   The rows must fit the rule: |mu d + gamma n - d'|^2 <= eps_dir for a refraction, |d + 2 ci n - d'|^2 <= eps_dir for
 *   a reflection; a ray whose rows fit neither (a caller-shaded surface) is NaN from there on and counts as unfit.
 * Next segment: it starts at x + 1e-6 d', so do' = dx + 1e-6 dd'.  dd' is tangent to the unit sphere analytically and is
 *   not renormalised.
 * Rays that end: a ray absent from a generation ends; its state is never read again.  A row whose surface is not in the
 *   table makes the ray NaN from there on (unknown); so does a row that is not finite or has n.d = 0, or an index that
 *   is not finite and > 0 (invalid).  Each ray is counted once.
 * Selection: row_slot DEVICE n_rows int64: the position of a selected row in the outputs, -1 for the others;
 *   selected DEVICE n_selected int64: the rows in output order; group_first HOST n_groups + 1 int64: the outputs of
 *   group q are [group_first[q], group_first[q + 1]).  The sums run in that order, so a caller that orders the selection
 *   by (group, generation, id) gets the same bits under any order of the rows inside a generation.
 * Sums, per group, E = 6 + 4 K + K (K + 1) / 2 doubles, over the selected rows whose weight, landing point and 3 K
 *   derivatives are all finite, w = the weight column's value or 1 (weight_column < 0):  count, sum w, sum w x (3),
 *   sum w |x - pivot|^2, sum w dx_k (k-major, 3 K), sum w (x - pivot).dx_k (K; pivots HOST (n_groups, 3)), sum w dx_j.dx_k for k <= j (row-major
 *   lower triangle).  Each workgroup writes the partial sums of its 256 outputs; a second kernel adds a group's partials
 *   in a fixed order (a wave an entry: lane l takes partials l, l + 64, ..., then the lanes are added pairwise).
 *
 * prt_frame_sensitivity: out, overwritten: jacobian_out DEVICE (K, 3, n_selected) doubles; sums_out DEVICE (n_groups, E);
 * record_out HOST 4 int64: unknown, invalid, unfit rays, reflections.  workspace:
 * prt_frame_sensitivity_workspace_bytes(n_ids, n_surfaces, K, n_groups, max rows of a group) device bytes (-1 for
 * arguments the call would refuse): the table, per id 48 K bytes of state, its previous row and a stamp, the partials.
 * Caps: K in [1, 16], n_ids in [1, 2^31], n_groups in [1, 65535], a generation's rows fit one launch; PRT_ERR_ARG
 * otherwise, never a truncated result, nothing written out of bounds.  One launch per generation in order on the stream,
 * one row a thread, the loop over the parameters inside the thread with its state in memory; no two lanes touch one
 * ray's state; no floating-point atomics; every output is the same bits on every run, and the result for a parameter does
 * not depend on which others are in the call.  All arguments are checked before a device is touched.  Stream-ordered; the
 * call reads the status word and the counters back and so returns when the stream has reached its end. */
int64_t prt_frame_sensitivity_workspace_bytes(int64_t n_ids, int n_surfaces, int n_parameters, int n_groups,
                                              int64_t max_group_rows);
int prt_frame_sensitivity(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                          int n_generations, double id0, int64_t n_ids, const prt_prim* surfaces, int n_surfaces,
                          const double* twists, const int64_t* parameter_ids, const int32_t* parameter_first,
                          int n_parameters, const int64_t* row_slot, const int64_t* selected, int64_t n_selected,
                          const int64_t* group_first, int n_groups, int weight_column, const double* pivots,
                          double* jacobian_out, double* sums_out, int64_t* record_out, void* workspace, void* stream);

/* ---- Sensitivities to shape and index parameters: the design form of the pass above -----------------------------------
 * The same pass, the same notation, for parameters that deform a surface or change the index of a glass: what a lens
 * designer varies (radii, thicknesses, indices).  Every shape parameter of the five primitives is an affine deformation
 * of the primitive in its own frame (sphere radius: uniform scaling about the centre; cylinder radius: scaling of x and y;
 * paraboloid focus f: scaling of x and y at the rate 1 / (2 f); cylinder height, cuboid side: scaling along one axis; lens
 * thickness: translation of one face), so parameter k gets, beside its twist, a 3x3 matrix S in world coordinates
 * (linear, K x 9, row-major) and, for the index, a rate (index_rates, K) and a second list of at most 64 surface ids
 * (index_ids [index_first[k], index_first[k + 1])).
 * Velocity of a moved surface under parameter k: u = v + w x (x - c) + S (x - c).  S = 0 is the rigid motion above.
 * Normal of a material point of a moved surface: dn_moved = w x n - (I - n n^T) S^T n (the normal transforms with the
 *   inverse transpose of I + eps (W + S)); dn = dn_moved + W (dx - u).  The curvature term keeps its form: the change of
 *   W itself is of second order.  The landing dt = n.(u - do - t dd) / (n.d) keeps its form with the general u.
 * Index: each ray carries dnu, d(index of its current segment)/dp_k, 0 in generation 0.  At a refraction, with ni, nt,
 *   mu = ni / nt, ci, ct and gamma as above:
 *     dnt = index_rates[k] if the ray ENTERS a surface that index parameter k names, else 0 (a ray that leaves goes into
 *       the ambient index, which is constant).  The ray enters where the trace's own world normal (normal_scale
 *       included) did not have to be turned against the ray.
 *     dmu = (dnu - mu dnt) / nt,  dct = (mu^2 ci dci - mu (1 - ci^2) dmu) / ct,  dgamma = ci dmu + mu dci - dct,
 *     dd' = dmu d + mu dd + dgamma n + gamma dn;  after the refraction dnu' = dnt.
 *   A reflection (total internal reflection included) and an undeviated interface keep dnu.
 *   The index behind the named surfaces grows by the rate at every wavelength (the index following the wavelength by the
 *   glass's dispersion: prt_frame_launch_sensitivity).  Known limit: an interface with ni == nt to the bit is differentiated as none (or as a reflection), as
 *   above, whatever the index parameter says.
 * Order of the arithmetic: the terms of S and of the index are added behind a per-parameter bit (S not zero; an index
 *   list that is not empty), after the rigid terms, which are computed as prt_frame_sensitivity computes them.  So a
 *   parameter with S = 0 and no index list gets the bits it gets from prt_frame_sensitivity, and every parameter the bits
 *   it gets alone.
 * Still out of scope: rays whose path changes.  The optical path and the OPD: prt_frame_opd_sensitivity, below; moving
 * a source: prt_frame_launch_sensitivity, below that.
 *
 * prt_frame_design_sensitivity: the arguments of prt_frame_sensitivity with linear, index_rates, index_ids and index_first
 * after parameter_first; outputs, selection, sums, counters, caps and guarantees as there.  Every entry of linear and
 * index_rates must be finite, K <= 16, at most 64 ids in either list of a parameter, every id in the table: PRT_ERR_ARG
 * with a message otherwise, before a device is touched.  workspace:
 * prt_frame_design_sensitivity_workspace_bytes(same arguments as above): the state is seven planes, 56 K bytes a ray
 * (the seventh, dnu, is read and written for index parameters alone). */
int64_t prt_frame_design_sensitivity_workspace_bytes(int64_t n_ids, int n_surfaces, int n_parameters, int n_groups,
                                                     int64_t max_group_rows);
int prt_frame_design_sensitivity(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                                 int n_generations, double id0, int64_t n_ids, const prt_prim* surfaces, int n_surfaces,
                                 const double* twists, const int64_t* parameter_ids, const int32_t* parameter_first,
                                 const double* linear, const double* index_rates, const int64_t* index_ids,
                                 const int32_t* index_first, int n_parameters, const int64_t* row_slot,
                                 const int64_t* selected, int64_t n_selected, const int64_t* group_first, int n_groups,
                                 int weight_column, const double* pivots, double* jacobian_out, double* sums_out,
                                 int64_t* record_out, void* workspace, void* stream);

/* ---- Wavefront sensitivities: d(OPD) and the Zernike right-hand sides per parameter ------------------------------------
 * The design form above with one more plane of state per ray and parameter, dL: the derivative of the row's cumulative
 * optical path as prt_frame_optical_path defines it (index * |x - o|, the 1e-6 relaunch offset part of o).  With the
 * notation above, len = |x - o|, n the index of the row's segment and dnu its derivative, start = do (0 in generation 0):
 *     dL = dL_prev + dnu len + n d.(dx - start),   dL_prev = 0 in generation 0.
 * (d(n len) = dnu len + n d.(dx - do): the segment's unit vector is d.)
 * At a selected row the reference sphere of a wavefront pass is HELD FIXED: per group P, R, the pivot and the pupil
 * radius (wavefront_groups HOST (n_groups, 6), as prt_frame_wavefront's group records have them in [0..5]), and the basis
 * (axes HOST 9 doubles: a, e1, e2).  Q = x is the landing point, u = d, s the larger root of |Q - s u - P| = R and
 * E = Q - s u, as prt_frame_wavefront computes them; OPD = (L - n s) - pivot, L the row's cumulative optical path (opl
 * DEVICE n_rows, from prt_frame_optical_path).  Per parameter:
 *   dfield = dL - s dnu - n (u.dx)          the wavefront change at a FIXED pupil point (Hopkins and Tiziani 1966): to first
 *                                           order the OPD along the ray through E is stationary in E (Fermat), so ds drops out
 *   dE     = dx - ds u - s dd,  ds = (E - P).(dx - s dd) / ((E - P).u)      the motion of the ray's point on the sphere
 *   dpupil = (dE.e1, dE.e2) / pupil radius
 *   dopd   = dfield + n (u.dE)              the derivative of this ray's own OPD, following the ray (= dL - s dnu - n ds, as
 *                                           u.dd = 0)
 * A reference that follows the group's centroid P(p) is not computed here: it is dfield - n (u.dP_k), linear in the three
 * columns n u_c, whose Zernike right-hand sides are among the sums.
 * A ray that misses the sphere, or that the pass cannot follow, is NaN in dfield, dopd and dpupil (and in opd_out and
 * pupil_out), and is left out of the sums below; the counters are those of prt_frame_sensitivity.
 * Order of the arithmetic: the terms of dL and of the sphere come after those of the design form, behind a compile-time
 * flag: jacobian_out and sums_out have the bits of prt_frame_design_sensitivity (for parameters with S = 0 and no index
 * list: of prt_frame_sensitivity).
 * Wavefront sums, per group, F = 5 + J (K + 3) + 4 K + K (K + 1) / 2 doubles (opd_sums_out DEVICE (n_groups, F)), over the
 * selected rows that are finite in w, x, dx, OPD, the pupil point, dfield and dopd; Z the J <= 36 Noll terms of
 * prt_frame_wavefront at the row's nominal pupil point:
 *   count, rows followed that miss the sphere, sum w, sum w OPD, sum w OPD^2 (OPD about the pivot);
 *   Z^T W y, column-major (column c at [5 + c J, 5 + (c + 1) J)), for y = dfield_k (K columns), then n u_c (3 columns);
 *   sum w dopd_k, sum w OPD dopd_k, sum w dfield_k, sum w OPD dfield_k (K each);
 *   sum w dfield_j dfield_k for k <= j (row-major lower triangle).
 *   Each workgroup writes the partial sums of its 256 outputs, each entry owned by one thread that walks the rows in
 *   order; the partials are added as those of prt_frame_sensitivity are.  Same bits on every run.
 *
 * prt_frame_opd_sensitivity: the arguments of prt_frame_design_sensitivity up to pivots; then opl, wavefront_groups, axes,
 * n_terms (J); then out, overwritten: jacobian_out, sums_out (as there), dfield_out, dopd_out DEVICE (K, n_selected),
 * dpupil_out DEVICE (K, 2, n_selected), opd_out DEVICE n_selected (about the pivot, piston not removed), pupil_out DEVICE
 * (n_selected, 2) (normalised), opd_sums_out, record_out.  A group with rows must have a pupil radius > 0; J in [1, 36];
 * otherwise the refusals of prt_frame_design_sensitivity.  workspace:
 * prt_frame_opd_sensitivity_workspace_bytes(the arguments of the others, then J): eight planes, 64 K bytes a ray, the group
 * records and the partials of the wavefront sums. */
int64_t prt_frame_opd_sensitivity_workspace_bytes(int64_t n_ids, int n_surfaces, int n_parameters, int n_groups,
                                                  int64_t max_group_rows, int n_terms);
int prt_frame_opd_sensitivity(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                              int n_generations, double id0, int64_t n_ids, const prt_prim* surfaces, int n_surfaces,
                              const double* twists, const int64_t* parameter_ids, const int32_t* parameter_first,
                              const double* linear, const double* index_rates, const int64_t* index_ids,
                              const int32_t* index_first, int n_parameters, const int64_t* row_slot,
                              const int64_t* selected, int64_t n_selected, const int64_t* group_first, int n_groups,
                              int weight_column, const double* pivots, const double* opl, const double* wavefront_groups,
                              const double* axes, int n_terms, double* jacobian_out, double* sums_out, double* dfield_out,
                              double* dopd_out, double* dpupil_out, double* opd_out, double* pupil_out,
                              double* opd_sums_out, int64_t* record_out, void* workspace, void* stream);

/* ---- Launch and wavelength sensitivities: the ray itself as the parameter ---------------------------------------------
 * The design form (or, with opl, the wavefront form) above with two more kinds of parameter, which close the differential
 * ray tracer: a rigid motion of the rays' launch, and a change of their wavelength.  Both name rays, not surfaces: per
 * parameter k an id range [lo, hi) (launch_ranges HOST (K, 2) doubles, compared with the row's id column as doubles;
 * -inf and +inf are allowed, lo <= hi), flags (launch_flags HOST K int32: bit 0 "seeds the launch", bit 1 "changes the
 * wavelength"; 0 for a parameter of the other kinds) and a wavelength rate (wavelength_rates HOST K, micrometres per unit
 * parameter, finite).  A parameter with a flag has an empty list of surface ids; its twist (v, w, c) is the launch twist.
 * Seed: in generation 0, for a parameter with bit 0 whose range holds the ray's id, with o the row's start and d its unit
 *   direction:  do = v + w x (o - c),  dd = w x d  (v + (w x (o - c)), the cross products as everywhere above).  For every
 *   other ray and parameter do = dd = 0 as before.  The landing that follows, and dL = dnu len + n d.(dx - do), are the
 *   forms above with this do: d(n |x - o|) = dnu len + n d.(dx - do).
 * Dispersion: materials HOST n_materials prt_material records, what prt_prim.material of the surface table indexes (here
 *   it IS read).  At a refraction in which the ray ENTERS (as above) a surface whose material is PRT_MAT_SELLMEIER, with
 *   wl the wavelength column of the ray's row in the glass, w2 = wl * wl, t_i = w2 - c_i:
 *     n2   = ((1 + (b1 w2) / t1) + (b2 w2) / t2) + (b3 w2) / t3                       (the trace's own index, squared)
 *     down = (((b1 c1) wl) / (t1 t1) + ((b2 c2) wl) / (t2 t2)) + ((b3 c3) wl) / (t3 t3)
 *     dn/dlambda = -down / sqrt(n2)                     (= (sum_i -b_i c_i wl / (wl^2 - c_i)^2) / n, per micrometre)
 *   evaluated once a row; for a parameter with bit 1 whose range holds the ray, dnt = wavelength_rates[k] * dn/dlambda
 *   in the dmu terms above, and dnu' = dnt.  On leaving dnt = 0, as for an index parameter; a surface whose material is
 *   NONE, ABSORBER, MIRROR or CONST_INDEX has no dispersion (dnt = 0).  With a bit 1 anywhere in the call a surface of
 *   any other kind (TABLE, HOST: their index is host code) is refused, PRT_ERR_ARG.
 *   Known limit: dnu is 0 in generation 0, so a ray launched inside a glass keeps dnu = 0 on its first segment.
 * slopes_out DEVICE (K, 3, n_selected): dd of the selected row's segment per parameter, NaN where jacobian_out is NaN.
 * Order of the arithmetic: the seed and the dispersion sit behind their bits and the ray's range, after everything else: a
 *   parameter without flags has the bits it has through prt_frame_design_sensitivity (with S = 0 and no index list: through
 *   prt_frame_sensitivity), jacobian_out and sums_out are the same bits with and without opl, and every parameter has the
 *   bits it has alone.  A ray outside a launch parameter's range has +0.0 in that parameter's jacobian and slopes.
 *
 * prt_frame_launch_sensitivity: the arguments of prt_frame_opd_sensitivity up to n_terms; then launch_ranges, launch_flags,
 * wavelength_rates, materials, n_materials; then out, overwritten: jacobian_out, sums_out, slopes_out, and the wavefront
 * outputs and record_out as there.  opl == NULL selects the form without the wavefront: wavefront_groups, axes, n_terms and
 * the six wavefront outputs are not read or written, the state is seven planes.  The frame needs its wavelength column
 * where a parameter has bit 1.  workspace: prt_frame_launch_sensitivity_workspace_bytes(the arguments of
 * prt_frame_opd_sensitivity_workspace_bytes; n_terms = 0 for the form without the wavefront): what that form needs and 56
 * bytes a surface for the dispersion table.  Caps, refusals and guarantees as above. */
int64_t prt_frame_launch_sensitivity_workspace_bytes(int64_t n_ids, int n_surfaces, int n_parameters, int n_groups,
                                                     int64_t max_group_rows, int n_terms);
int prt_frame_launch_sensitivity(int device, const double* rows, int64_t ld, const int64_t* rows_per_generation,
                                 int n_generations, double id0, int64_t n_ids, const prt_prim* surfaces, int n_surfaces,
                                 const double* twists, const int64_t* parameter_ids, const int32_t* parameter_first,
                                 const double* linear, const double* index_rates, const int64_t* index_ids,
                                 const int32_t* index_first, int n_parameters, const int64_t* row_slot,
                                 const int64_t* selected, int64_t n_selected, const int64_t* group_first, int n_groups,
                                 int weight_column, const double* pivots, const double* opl,
                                 const double* wavefront_groups, const double* axes, int n_terms,
                                 const double* launch_ranges, const int32_t* launch_flags, const double* wavelength_rates,
                                 const prt_material* materials, int n_materials, double* jacobian_out, double* sums_out,
                                 double* slopes_out, double* dfield_out, double* dopd_out, double* dpupil_out,
                                 double* opd_out, double* pupil_out, double* opd_sums_out, int64_t* record_out,
                                 void* workspace, void* stream);

/* statistics of the trace of this scene that ended last (prt_trace / prt_trace_end; for bench.py's roofline):
 * out[0] = generations that found rays, out[1] = sum over generations of rays alive at entry,
 * out[2] = GPU milliseconds spent in generation kernels (hipEvent, on the trace stream),
 * out[3] = number of generation-kernel launches, out[4] = sum of rows recorded,
 * out[5] = sum of rays handed to the next generation,
 * out[6] = traces of this scene, so far, whose look-back gave up and which were re-run on the
 *          three-kernel path (telemetry: such a trace is correct but about twice as slow),
 * out[7] = PRT_VARIANT_* the last trace ran on. */
#define PRT_VARIANT_FUSED 1       /* one ray per lane, one fused kernel per generation */
#define PRT_VARIANT_UNFUSED 2     /* propagate / scan / interact kernels per generation */
#define PRT_VARIANT_KLANES 3      /* ... with the surface-parallel nearest-hit kernel (K lanes per ray,
                                     shuffle min-reduce; prt_scene_options.hit_lanes = 4 | 8 | 16) */
int prt_trace_stats(const prt_scene* scene, double* out8);
/* counters of this scene since it was created: out12 = { traces re-run on the three-kernel path after a
 * look-back gave up, traces repeated because a dense-mode hint did not hold, generation launches made in
 * dense mode, traces repeated with all 13 state rows (see below; at most one per scene),
 * and from the traces run with PRT_TRACE_COUNT_PATHS: how many such traces, ray-generations whose ray was
 * not well formed (see "shortcuts" in DESIGN.md: such a ray takes none), CSG node evaluations with
 * survivors under an implied cull box, ... of which evaluated upstream's box test exactly;
 * generation launches made under a record plan, traces under a plan repeated because one of the plan's own dense
 * hints did not hold (slots 8 and 9 counted the per-tile records of 0.2.0-0.2.1, retired in 0.2.2),
 * dense-mode launches that kept their absorbed rays (sparse loss, below), launches under a plan that ran dense }.
 * Dense mode: a generation in which the previous trace of the same scene (whatever its ray count)
 * recorded every ray and carried all or none of them on is launched on the assumption that it will
 * again -- every tile then knows its output position without the look-back; each tile checks the
 * assumption on its own counts and a miss repeats the trace without assumptions (results are exact
 * either way; PRT_TRACE_NO_HINTS turns the hints off for a call).
 * Sparse loss: a generation that recorded every ray and carried on all but a few absorbed ones (at most 1 in 64)
 * is launched dense as well, with PRT_TRACE_KEEP_ABSORBED in force for that launch: the absorbed rays go on,
 * direction zeroed, the way upstream carries them (_pyrayt.py:415-428), and the next generation -- which
 * compacts -- finds them dead, records nothing for them and drops them.  The rows are the same; what is saved is
 * the look-back of a generation whose few odd rays make their tiles the slowest ones, so that every tile waited
 * for a straggler (PRT_TRACE_NO_SPARSE_KEEP turns it off for a call).  Such a launch notes, per tile, how many rays it kept (a dead list
 * in the workspace), and the generation behind it -- if it loses no ray of its own -- is launched on that list:
 * its tiles' positions are "tile index x tile size minus the dead rays in front", again without a look-back.
 * Compact state: between the generations of a trace the ray state goes without its rows 3, 7 and 8
 * (origin w, direction w, generation): in a ray set that starts like RaySet's defaults
 * (pyrayt/_pyrayt.py:29-36: w = 1 / 0, generation 0) they hold 1, +0 and the generation's number in every
 * generation, bit for bit, so they are neither written nor read (24 of 104 B each way).  Generation 0
 * checks the caller's rows, every generation checks the rays it hands on; the first ray that differs
 * makes the library repeat the trace with all rows and keep doing so for this scene
 * (PRT_TRACE_FULL_ROWS forces that form for a call).
 * Lean segments (0.2.1): three more of those rows never change on this path (no built-in material touches a ray's
 * intensity, wavelength or id) and are redundant within a wave of a ray set as sources emit it.  A wave of a
 * generation whose 64 outputs land, in lane order, on the 64 columns one wave of the next generation reads checks that
 * its rays share one intensity and one wavelength (bit for bit) and that their ids count up by one from an integer
 * in [0, 2^48); then its first lane alone writes, into the first three entries of the segment's id row, that first id
 * boxed into a NaN with the tag 0x7ffb in its top 16 bits, the intensity and the wavelength -- rows 9 and 10 of the
 * segment are not written -- and the reader takes the three numbers from there with one scalar load (24 of the
 * remaining 80 B each way).  Any other wave hands the rows on as they are, so every ray set is served.  A ray whose
 * genuine id carries that tag would be misread: it raises the same repeat with all 13 rows. */
int prt_trace_telemetry(const prt_scene* scene, int64_t* out12);
/* one more counter of the traces run with PRT_TRACE_COUNT_PATHS, per WAVE: out1 = { waves that did not finish a bare
 * plane leaf because no lane's crossing could win (prt_scene_options.no_plane_bound) } */
int prt_trace_shortcut_counts(const prt_scene* scene, int64_t* out1);

/* ---- renderers (second consumer of the intersect path) ----------
 * tinygfx/g3d/renderers.py: an OrthographicCamera grid (world_objects.py:499-537) is pushed
 * through the components, then Gooch-shaded (ShadedRenderer :129-248) or edge-detected
 * (EdgeRender :11-126).  Pixels are numbered row-major over the v_pixels x h_pixels picture;
 * images are (v, h, 4) float64 RGBA, the layout both renderers return. */
typedef struct prt_camera {
  double world[16];  /* row-major camera -> world transform (world_objects.py:97-99) */
  int64_t h_pixels, v_pixels;
  double h_width, v_width; /* camera-space span of the grid along y (h) and z (v) */
} prt_camera;

/* OrthographicCamera.generate_rays (world_objects.py:519-537): rays of pixels
 * [first, first+count) into columns [0, count) of the device (8, ld) block rays_out
 * (rows 0-3 origin, 4-7 unit direction). */
int prt_camera_rays(int device, const prt_camera* camera, int64_t first, int64_t count,
                    double* rays_out, int64_t ld, void* stream);

/* EdgeRender._st_propagate / ShadedRenderer._st_propagate (renderers.py:70-92, 187-209).
 * Differs from prt_propagate in one rule: a component without a positive hit offers its
 * smallest parameter (gather from the unmasked list at the argmin of the masked one,
 * :79-83), so t_out may be negative.  rays (>= 8, n) ld; t_out (n); surf_out (n), -1 = none. */
int prt_render_hits(prt_scene* scene, int device, const double* rays, int64_t n, int64_t ld,
                    double* t_out, int64_t* surf_out, void* stream);

/* ShadedRenderer._st_interact (renderers.py:211-236) = TracerSurface.shade
 * (world_objects.py:385-399) + GoochMaterial.shade (materials/gooch.py:30-65) with one light:
 *   gooch: device (n_prims, 8) = shade_warm[4] | shade_cool[4] per primitive (gooch.py:36-37)
 *   light: HOST double[3], world position of the light
 *   rgba_out: device (n, 4); pixels with surf == -1 get (0,0,0,0).
 * Upstream's multi-light branch (gooch.py:48-51) does not broadcast for any light count
 * but 3, where it mixes up coordinates and lights; it is not offered. */
int prt_gooch_shade(prt_scene* scene, int device, const double* rays, int64_t n, int64_t ld,
                    const double* t, const int64_t* surf, const double* gooch,
                    const double* light, double* rgba_out, void* stream);

/* GoochMaterial.shade(rays, normals, light_positions) (materials/gooch.py:30-65) on caller
 * supplied points and normals, one light:  points, normals: device (>= 3, n) ld;
 * shade: HOST double[8] = shade_warm | shade_cool; light: HOST double[3];
 * rgba_out: device (4, n) ld_out -- the (4, n) layout the method returns. */
int prt_gooch_mix(int device, const double* points, const double* normals, int64_t n, int64_t ld,
                  const double* shade, const double* light, double* rgba_out, int64_t ld_out,
                  void* stream);

/* ShadedRenderer.render() / the propagate half of EdgeRender.render() for pixels
 * [first, first+count) in one kernel: camera ray -> nearest hit -> Gooch colour, nothing read
 * from HBM but the scene.  Any of rgba_out (count,4) / t_out (count) / surf_out (count) may
 * be NULL; gooch and light are needed only with rgba_out. */
int prt_render(prt_scene* scene, int device, const prt_camera* camera, int64_t first,
               int64_t count, const double* gooch, const double* light, double* rgba_out,
               double* t_out, int64_t* surf_out, void* stream);

/* EdgeRender._st_interact (renderers.py:94-116): edge = surface id differs from the left or
 * upper neighbour (outside = -1), grown by `rings` 3x3 binary dilations (upstream:
 * max(1, int(max(v, h) / 300))); rgba_out (v, h, 4): edges (0,0,0,1), the rest (1,1,1,0).
 * workspace: device scratch of prt_edge_workspace_bytes(h, v) bytes. */
int64_t prt_edge_workspace_bytes(int64_t h_pixels, int64_t v_pixels);
int prt_edge_canvas(int device, const int64_t* surf, int64_t h_pixels, int64_t v_pixels,
                    int rings, double* rgba_out, void* workspace, void* stream);

/* ---- tinygfx/g3d/operations.py as functions -------------
 * The vector helpers the primitives and materials are written with, callable on their own like
 * upstream's (`cg.reflect`, `cg.refract`, ...).  Column vectors: (rows, n) blocks with leading
 * dimension ld, rows in 1..4 (homogeneous 4-vectors upstream). */

/* reflect(vectors, normals) (operations.py:86-107): out = v - 2 n (v.n) */
int prt_reflect(int device, const double* vectors, const double* normals, int rows, int64_t n,
                int64_t ld, double* out, int64_t ld_out, void* stream);

/* refract(vectors, normals, n1, n2, n_global) (operations.py:110-162).  `vectors` is normalised
 * IN PLACE, as upstream does (:125); n1, n2: device (n) per-ray indices; out: refracted (or
 * totally reflected) unit directions; index_out (n): n2 (n_global when leaving) or n1 on TIR. */
int prt_refract(int device, double* vectors, const double* normals, const double* n1,
                const double* n2, double n_global, int rows, int64_t n, int64_t ld, double* out,
                int64_t ld_out, double* index_out, void* stream);

/* binomial_root(a, b, c) (operations.py:28-63) -> roots_out (2, n): the degenerate branches of
 * the reference included (|a| <= 1e-8 linear, then |b| <= 1e-8 -> +-inf by the sign of c). */
int prt_binomial_root(int device, const double* a, const double* b, const double* c, int64_t n,
                      double* roots_out, int64_t ld_out, void* stream);

/* smallest_positive_root(a, b, c) (operations.py:4-25) -> out (n), +inf where there is none */
int prt_smallest_positive_root(int device, const double* a, const double* b, const double* c,
                               int64_t n, double* out, void* stream);

/* element_wise_dot(m1, m2, axis) (operations.py:66-83) in strided form:
 * out[o] = sum_{r < reduce_len} m1[o*out_stride + r*reduce_stride] * m2[same], o < out_len.
 * axis 0 of a (k, n) block: reduce_len k, reduce_stride ld, out_len n, out_stride 1. */
int prt_dot(int device, const double* m1, const double* m2, int64_t reduce_len,
            int64_t reduce_stride, int64_t out_len, int64_t out_stride, double* out, void* stream);

/* csg.array_csg(array1, array2, operation, sort_output) (tinygfx/g3d/csg.py:13-61): the interval
 * algebra of a CSG node on two (m, n) blocks of ascending hit lists (m even: enter/exit pairs), one
 * column per ray; op = PRT_NODE_UNION / INTERSECT / DIFFERENCE.  out (m_left + m_right, n): with
 * sort_output the surviving entries ascending followed by +inf, otherwise the merged order with
 * rejected entries set to +inf.  Ties merge left-first (the stable order of SURVEY.md Q8). */
int prt_array_csg(int device, const double* left, int m_left, const double* right, int m_right,
                  int64_t n, int64_t ld, int op, int sort_output, double* out, int64_t ld_out,
                  void* stream);

/* primitive.intersect(rays) / primitive.normal(points) in OBJECT space (tinygfx/g3d/primitives.py:
 * Sphere :220-296, Paraboloid :299-419, Plane :422-498, Cube :501-602, Cylinder :621-741), i.e. the
 * shape routines without a world transform: type = PRT_PRIM_*, params as in prt_prim.
 *   rays (>= 7, n) ld (rows 0-2 origin, 4-6 direction; w rows are not read) -> hits_out (2, n):
 *   the raw pair in upstream's order -- not sorted, NaN where upstream yields NaN
 *   points (>= 3, n) ld -> normals_out (4, n): unit normal, w = 0 */
int prt_primitive_intersect(int device, int type, const double* params, const double* rays,
                            int64_t n, int64_t ld, double* hits_out, int64_t ld_out, void* stream);
int prt_primitive_normal(int device, int type, const double* params, const double* points,
                         int64_t n, int64_t ld, double* normals_out, int64_t ld_out, void* stream);

/* error codes */
#define PRT_OK 0
#define PRT_ERR_ARG (-1)
#define PRT_ERR_HIP (-2)
#define PRT_ERR_SCENE (-3)
#define PRT_ERR_ROWS_CAP (-4)
#define PRT_ERR_UNTRACABLE (-5) /* a ray hit a PRT_MAT_NONE surface (AttributeError upstream) */
#define PRT_ERR_WAVELENGTH (-6) /* a ray's wavelength is not in the index table of the PRT_MAT_TABLE glass it hit */

#ifdef __cplusplus
}
#endif
#endif /* PRT_H */
