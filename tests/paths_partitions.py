"""The host's plan for the ray-path pass (pyrayt_amd/csrc/prt_paths.hpp) restated in Python, and frames built to sit on its
edges: generations whose runs of rows change key and group at chosen places, ids that leave gaps, keys aimed at the last
slots of the table.  tests/test_host_paths_partitions.py asserts that the builders make what each case claims;
tests/test_gpu_paths_partitions.py compares the device with tests/paths_reference.py on them, through check()."""
import numpy as np

import paths_reference as ref

IX = ref.IX
EPS = np.finfo(np.float64).eps
GRID, BLOCK, WAVES = 512, 256, 4  # kPathsGrid, kPathsBlock, kPathsWaves
GOLDEN, MASK = 0x9e3779b97f4a7c15, (1 << 64) - 1
# bits = 6: every one of these first surfaces starts at slot 62 or 63 ...
DEPTH0 = (21, 55, 76, 110, 144, 165, 199, 254, 288, 309, 343, 377, 398, 432, 453, 487)
# ... and so do these (at 63) under the parent of surface 7, which sits at slot 20
PARENT, DEPTH1 = 7, (64, 119, 208, 263, 297, 352, 441, 496)


# ---- the plan -------------------------------------------------------------------------------------------------------
def per_wave(count):
    """run(): the rows (or ids) one wave takes, a whole number of 64-row slices."""
    return max(1, -(-count // (GRID * BLOCK))) * 64


def workgroups(count):
    return -(-count // (per_wave(count) * WAVES))


def capacity_bits(max_paths):
    bits = 6
    while (1 << bits) < 4 * max_paths:
        bits += 1
    return bits


def slot(key, bits):
    return ((key * GOLDEN) & MASK) >> (64 - bits)


def child_key(parent_slot, surface):
    return ((parent_slot + 1) << 32) | surface


def probe(keys, bits):
    """The keys inserted one after the other: key -> slot, and whether a probe stepped from the last slot to slot 0.
    (Linear probing fills the same set of slots in any order of insertion.)"""
    capacity, taken, wrapped = 1 << bits, {}, False
    for key in keys:
        at = slot(key, bits)
        while at in taken.values():
            wrapped |= at == capacity - 1
            at = (at + 1) & (capacity - 1)
        taken[key] = at
    return taken, wrapped


# ---- the comparison (moved here from tests/test_gpu_paths.py, unchanged) --------------------------------------------
def check(got, want):
    """Exact, but for the energies of weights that are not integers: there every row's weight is truncated to a multiple
    of the unit 2^-(62 - E - B) (w_max = f 2^E, B = bit_length(n_rows): include/prt.h), so a cell of n rows lies below
    math.fsum's value by less than n units, and the one conversion to a double rounds by half an ulp."""
    import torch

    assert got.sequences == want["sequences"]
    for name in ("parent", "surface", "depth", "subtree_size", "through", "ended", "dark"):
        assert np.array_equal(getattr(got, name), want[name]), name
    for name in ("row_node", "ray_node", "ray_last_row"):
        assert np.array_equal(getattr(got, name).cpu().numpy(), want[name]), name
    assert got.row_node.dtype == torch.int32 and got.ray_node.dtype == torch.int32 and got.ray_last_row.dtype == torch.int64
    assert got.id0 == want["id0"] and got.n_bad_weight == want["n_bad_weight"] and got.n_rays == want["n_rays"]
    for name, rows in (("energy_through", "through"), ("energy_ended", "ended")):
        if want["integer_weights"]:
            assert np.array_equal(getattr(got, name), want[name]), name
        else:
            unit = 2.0 ** -want["shift"]
            short = want[name] - getattr(got, name)
            ulp = EPS * want[name]
            print(name, "largest shortfall in units of a row's truncation:", (short / np.maximum(want[rows], 1) / unit).max())
            assert np.all(short >= -ulp) and np.all(short <= want[rows] * unit + ulp), name


def fewer_groups(want, n_groups):
    """The reference of the same frame with the first n_groups groups only: a group's tables do not depend on how many
    groups there are, and nothing else depends on the groups at all."""
    cut = dict(want)
    for name in ("through", "ended", "dark", "energy_through", "energy_ended"):
        cut[name] = want[name][:n_groups]
    return cut


# ---- frames ---------------------------------------------------------------------------------------------------------
def weight_rule(generation, ids):
    """Integer weights from 1 to 199: every energy is an exact integer sum."""
    return 1.0 + (7 * np.asarray(ids, dtype=np.int64) + 13 * generation) % 199


def build(generations, weights=weight_rule):
    """A frame from [(ids, surfaces), ...], one pair of integer arrays per generation in row order: the weights by
    rule, every direction (1, 0, 0).  Groups come from the ids, through rays_per_source."""
    blocks = []
    for generation, (ids, surfaces) in enumerate(generations):
        block = np.zeros((len(ids), 15))
        block[:, IX["generation"]] = generation
        block[:, IX["id"]] = ids
        block[:, IX["surface"]] = surfaces
        block[:, IX["intensity"]] = weights(generation, ids)
        block[:, IX["x_tilt"]] = 1.0
        blocks.append(block)
    return np.concatenate(blocks)


def counts_of(frame):
    return np.bincount(frame[:, IX["generation"]].astype(int)).tolist()


# One arrangement per workgroup, in turn.  A row's place: r, its row in its wave's run; s = r // 64, its slice; v, its
# wave in the workgroup.  Each gives an index into SURFACES.
SURFACES = (3, 5, 9, 12)
ARRANGEMENTS = ("boundary", "before", "after", "alternate", "aba", "one_cell", "four_cells", "aaba")
RULES = dict(boundary=lambda r, s, v: s % 3,                         # the key changes at rows 64 and 128 of a run
             before=lambda r, s, v: ((r + 1) // 64) % 3,             # ... at rows 63 and 127
             after=lambda r, s, v: (np.maximum(r - 1, 0) // 64) % 3,  # ... at rows 65 and 129
             alternate=lambda r, s, v: r % 3,                        # every slice holds every key
             aba=lambda r, s, v: s % 2,                              # A, B, A over the slices of a run
             one_cell=lambda r, s, v: 0 * v,                         # the four waves end holding one cell
             four_cells=lambda r, s, v: v,                           # ... four different cells
             aaba=lambda r, s, v: (v == 2).astype(np.int64))         # ... A, A, B, A


def place(count):
    """(arrangement number, r, s, v) of every row of a generation of ``count`` rows."""
    run = per_wave(count)
    p = np.arange(count)
    r = p % run
    return (p // (run * WAVES)) % len(ARRANGEMENTS), r, r // 64, (p // run) % WAVES


def arranged_surfaces(count):
    which, r, s, v = place(count)
    index = np.zeros(count, dtype=np.int64)
    for number, name in enumerate(ARRANGEMENTS):
        index = np.where(which == number, RULES[name](r, s, v), index)
    return np.asarray(SURFACES)[index]


def arranged(counts, id0=0):
    """Generations of ``counts`` rows (descending: the rays at the end die), ids ascending from id0 in every one, so that
    a ray keeps its place and the surfaces of each generation follow the arrangements at that generation's per_wave."""
    assert list(counts) == sorted(counts, reverse=True)
    return build([(id0 + np.arange(count), arranged_surfaces(count)) for count in counts])


def end_frame(n_ids, id0=500):
    """Two generations over n_ids ids from id0 for k_paths_end: an id in 97 was never launched (but the first and the
    last), a ray in four dies after its first row, and the rays in the first and the last lane of a run of ids -- and
    the single ragged one, where there is one -- end dark, with a weight that does not count, or both; the ray of the
    last id does both.  Returns the frame and the indices (id - id0) of those rays."""
    run = per_wave(n_ids)
    index = np.arange(n_ids)
    marked = np.unique([0, run - 1, run, 2 * run - 1, 50 * run, 51 * run - 1, (n_ids - 1) // run * run, n_ids - 1])
    launched = index % 97 != 5
    launched[marked] = True
    first = index[launched]
    second = first[first % 4 != 1]
    frame = build([(id0 + first, np.asarray(SURFACES)[first % 3]), (id0 + second, np.asarray(SURFACES)[(second // 64) % 3])])
    last_row = {}
    for row, ray in enumerate(frame[:, IX["id"]].astype(np.int64) - id0):
        last_row[int(ray)] = row
    for k, ray in enumerate(marked):
        row = last_row[int(ray)]
        if k % 3 != 1 or ray == n_ids - 1:
            frame[row, 12:15] = 0.0
        if k % 3 != 0 or ray == n_ids - 1:
            frame[row, IX["intensity"]] = (np.nan, -1.0, np.inf, -np.inf)[k % 4]
    return frame, marked


def collisions_depth0(rows):
    """One generation whose rows name the sixteen aimed first surfaces, every wave in another rotation."""
    p = np.arange(rows)
    return build([(p, np.asarray(DEPTH0)[(p + p // 64) % len(DEPTH0)])])


def collisions_depth1(rows):
    """Every ray meets PARENT, then one of the eight aimed surfaces."""
    p = np.arange(rows)
    return build([(p, np.full(rows, PARENT)), (p, np.asarray(DEPTH1)[(p + p // 64) % len(DEPTH1)])])


def seventeen_nodes():
    """The sixteen aimed first surfaces and PARENT beside them: 17 nodes."""
    return build([(np.arange(17), np.asarray(DEPTH0 + (PARENT,)))])


def many_nodes():
    """4096 first surfaces, 64 in each of 64 waves, descending: the canonical numbering is the reverse of the making."""
    p = np.arange(4096)
    return build([(p, (4095 - p) * 1000)])


def weights_frame(weights, surfaces=None):
    """One generation, a ray a row, with the given weights (and surfaces: 2 unless given)."""
    n = len(weights)
    frame = np.zeros((n, 15))
    frame[:, IX["id"]] = np.arange(n)
    frame[:, IX["surface"]] = 2 if surfaces is None else surfaces
    frame[:, IX["intensity"]] = weights
    frame[:, IX["x_tilt"]] = 1.0
    return frame


# ---- the large frames, each with its reference (computed once in a process) -----------------------------------------
# name -> (rows per generation, rays_per_source): per_wave 192, 128 and 64 with every workgroup inside one group; 128
# and 128 with groups that change inside a slice; 128 (its last workgroup: one row), 64 and 64 with groups that change
# at slice boundaries; 192 with groups that change inside a slice.  The reference is made with groups for every id, so
# that the ragged last workgroup holds a cell; fewer_groups(want, n_groups - BEYOND) leaves the last ids beyond the groups.
LARGE = {"262145_131073_131072": ((262145, 131073, 131072), 3072),
         "262144_131073": ((262144, 131073), 100),
         "131073_131072_70000": ((131073, 131072, 70000), 192),
         "262145": ((262145,), 100)}
MAX_PATHS = 128  # (4 + 16 + 64 nodes at the most; 2600 groups x 512 slots of tallies stay below the table cap)
BEYOND = 4
END_RAYS_PER_SOURCE, END_GROUPS = 50_000, 3  # (ids 500 .. 131 572: every ray in a group; with two groups the last ones beyond)
_CACHE = {}


def large(name):
    """(frame, rays_per_source, n_groups, reference), n_groups the fewest that hold every id."""
    if name not in _CACHE:
        counts, rays_per_source = LARGE[name]
        frame = arranged(counts)
        n_groups = -(-counts[0] // rays_per_source)
        _CACHE[name] = (frame, rays_per_source, n_groups, ref.paths(frame, rays_per_source=rays_per_source, n_groups=n_groups))
    return _CACHE[name]


def ended(n_ids):
    """(frame, marked, reference) of end_frame(n_ids): three groups of 50 000 ids, which hold every ray."""
    if ("end", n_ids) not in _CACHE:
        frame, marked = end_frame(n_ids)
        _CACHE["end", n_ids] = (frame, marked, ref.paths(frame, rays_per_source=END_RAYS_PER_SOURCE, n_groups=END_GROUPS))
    return _CACHE["end", n_ids]
