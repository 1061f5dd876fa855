"""The ray-path pass on the device (DeviceFrame.paths) where its partition changes, against tests/paths_reference.py
through check(): all tables, row_node, ray_node, ray_last_row, n_rays and n_bad_weight exact.  Generations of 131 072,
131 073, 262 144 and 262 145 rows (per_wave 64, 128, 128 and 192), keys and groups that change at, beside and inside the
64-row slices of a run, the cells the four waves of a workgroup hand to paths_merge, ids that were never launched and
dark or uncounted last rows in the first, the last and the single ragged lane of k_paths_end's runs, keys aimed at the
last slots of the table so that their probes wrap, the table's capacity edge, 4096 nodes, and energy_shift at the ends
of its range.  Every case asserts the arm it is named for from the restated plan (tests/paths_partitions.py; the frames
themselves are held to their claims by tests/test_host_paths_partitions.py) before it calls the device.  No case is
sampled or filtered by its result."""
import sys

import numpy as np
import pytest

import paths_partitions as pp
import paths_reference as ref
from paths_partitions import check

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IX = ref.IX


def device_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist() if len(frame) else []
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(frame, dtype=np.float64).T)).to("cuda:0")
    return DeviceFrame(rows, counts)


def outputs(paths):
    return [torch.from_numpy(np.ascontiguousarray(getattr(paths, name))) for name in
            ("parent", "surface", "depth", "subtree_size", "through", "ended", "dark", "energy_through",
             "energy_ended")] + [paths.row_node, paths.ray_node, paths.ray_last_row]


# ---- runs of more than one slice ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, runs", [("262145_131073_131072", [192, 128, 64]), ("262144_131073", [128, 128]),
                                        ("131073_131072_70000", [128, 64, 64]), ("262145", [192])])
def test_keys_and_groups_that_change_across_the_slices_of_a_run(name, runs):
    """Every workgroup of a generation follows one of eight arrangements in turn (tests/paths_partitions.py): the key
    changes at row 64 of a run, at rows 63 and 65, row by row, A B A over three slices, and the four waves end on one
    cell, on four, on A A B A.  The groups change at run boundaries only (rays_per_source 3072), at slice boundaries
    (192) or inside the slices (100).  First with a group for every id, so that the ragged last workgroup -- at
    131 073 rows one row in its first wave and three empty waves -- holds a cell and writes it out; then with the last
    ids beyond n_groups, with three groups and with one."""
    counts, rays_per_source = pp.LARGE[name]
    assert [pp.per_wave(count) for count in counts] == runs and max(runs) > 64
    frame, _, n_groups, want = pp.large(name)
    assert (counts[0] - 1) // rays_per_source == n_groups - 1 and want["through"][n_groups - 1].sum() >= 1
    assert counts[0] > (n_groups - pp.BEYOND) * rays_per_source and len(want["sequences"]) <= pp.MAX_PATHS
    if counts[0] == 131_073:  # (the last workgroup: one row in its first wave, three empty waves)
        assert counts[0] - (pp.workgroups(counts[0]) - 1) * runs[0] * pp.WAVES == 1
    device = device_frame(frame)
    options = dict(rays_per_source=rays_per_source, n_groups=n_groups)
    check(device.paths(max_paths=pp.MAX_PATHS, **options), want)
    # the table just large enough, so that the slots are other ones; three groups; one group
    nodes = len(want["sequences"])
    assert pp.capacity_bits(nodes) < pp.capacity_bits(pp.MAX_PATHS)
    check(device.paths(max_paths=nodes, **options), want)
    fewer = n_groups - pp.BEYOND
    check(device.paths(max_paths=pp.MAX_PATHS, rays_per_source=rays_per_source, n_groups=fewer), pp.fewer_groups(want, fewer))
    check(device.paths(max_paths=pp.MAX_PATHS, rays_per_source=rays_per_source, n_groups=3), pp.fewer_groups(want, 3))
    check(device.paths(max_paths=pp.MAX_PATHS, rays_per_source=rays_per_source, n_groups=1), pp.fewer_groups(want, 1))


# ---- k_paths_end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ids, run", [(131_072, 64), (131_073, 128)])
def test_rays_that_end_in_the_first_the_last_and_the_ragged_lane(n_ids, run):
    """Ids from 500 with one in 97 never launched (stamp 0: it counts in nothing, ray_node -1); dark last rows and
    weights that do not count in the first and the last lane of a run of ids and, at 131 073, in the single lane of
    the last wave -- that ray does both.  Three groups hold every ray, so the last wave holds a cell and the last
    workgroup merges it; with two groups the ids from 100 000 lie beyond them."""
    frame, marked, want = pp.ended(n_ids)
    assert pp.per_wave(n_ids) == run and len(want["ray_node"]) == n_ids and want["id0"] == 500.0
    assert {int(m) % run for m in marked} == {0, run - 1} and n_ids - 1 in marked
    assert (want["ray_node"] < 0).sum() > 1000 and want["n_bad_weight"] >= 4 and want["dark"].sum() >= 3
    last = want["ray_last_row"][marked]
    assert np.all(frame[last, IX["id"]] // pp.END_RAYS_PER_SOURCE < pp.END_GROUPS) and marked[-1] == n_ids - 1
    weight = frame[last[-1], IX["intensity"]]
    assert np.all(frame[last[-1], 12:15] == 0.0) and not (np.isfinite(weight) and weight >= 0)
    assert want["dark"][pp.END_GROUPS - 1].sum() >= 1 and want["ended"].sum() == want["n_rays"]
    device = device_frame(frame)
    got = device.paths(rays_per_source=pp.END_RAYS_PER_SOURCE, n_groups=pp.END_GROUPS)
    check(got, want)
    check(device.paths(rays_per_source=pp.END_RAYS_PER_SOURCE, n_groups=2), pp.fewer_groups(want, 2))
    assert got.n_rays == n_ids - int((want["ray_node"] < 0).sum())


def test_the_same_bits_in_any_order_of_the_rows_at_per_wave_128():
    """131 073 ids: k_paths_step's first generation and k_paths_end both take 128 to a wave; the rows of every
    generation shuffled."""
    frame, rays_per_source, n_groups, want = pp.large("131073_131072_70000")
    options = dict(rays_per_source=rays_per_source, n_groups=n_groups, max_paths=pp.MAX_PATHS)
    first = device_frame(frame).paths(**options)
    rng = np.random.default_rng(5)
    counts = np.bincount(frame[:, 0].astype(int))
    assert pp.per_wave(int(counts[0])) == 128 and pp.per_wave(len(want["ray_node"])) == 128 and counts[0] == 131_073
    starts = np.concatenate([[0], np.cumsum(counts)])
    order = np.concatenate([starts[g] + rng.permutation(counts[g]) for g in range(len(counts))])  # new row -> old row
    shuffled = device_frame(frame[order]).paths(**options)
    for a, b in zip(outputs(first)[:9], outputs(shuffled)[:9]):
        assert torch.equal(a, b)
    assert shuffled.sequences == first.sequences
    assert torch.equal(shuffled.ray_node, first.ray_node)
    where = torch.from_numpy(order).to("cuda:0")
    assert torch.equal(shuffled.row_node, first.row_node[where])
    assert torch.equal(where[shuffled.ray_last_row.clamp(min=0)][shuffled.ray_last_row >= 0],
                       first.ray_last_row[first.ray_last_row >= 0])
    assert torch.equal(shuffled.ray_last_row < 0, first.ray_last_row < 0)


# ---- the table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", (16, 16_384))
def test_sixteen_first_surfaces_aimed_at_the_last_two_slots(rows):
    """max_paths = 16: 64 slots.  All sixteen keys start at slot 62 or 63, so their probes run on through slots 0 to
    13: in one wave one after the other, and from 64 workgroups at once, where a compare-and-swap that loses returns
    another key and the probe moves on while the neighbours fill."""
    assert pp.capacity_bits(16) == 6 and {pp.slot(surface, 6) for surface in pp.DEPTH0} == {62, 63}
    taken, wrapped = pp.probe(pp.DEPTH0, 6)
    assert wrapped and sorted(taken.values()) == list(range(14)) + [62, 63]
    assert pp.workgroups(rows) == (1 if rows == 16 else 64) and pp.per_wave(rows) == 64
    frame = pp.collisions_depth0(rows)
    want = ref.paths(frame)
    assert len(want["sequences"]) == 16
    device = device_frame(frame)
    check(device.paths(max_paths=16), want)
    check(device.paths(max_paths=16, rays_per_source=5, n_groups=3), ref.paths(frame, rays_per_source=5, n_groups=3))


@pytest.mark.parametrize("rows", (8, 16_384))
def test_eight_second_surfaces_aimed_at_the_last_slot(rows):
    """The parent (surface 7) sits at slot 20 of 64; its eight children all start at slot 63 and fill slots 0 to 6."""
    assert pp.slot(pp.PARENT, 6) == 20
    keys = [pp.child_key(20, surface) for surface in pp.DEPTH1]
    assert {pp.slot(key, 6) for key in keys} == {63}
    taken, wrapped = pp.probe([pp.PARENT] + keys, 6)
    assert wrapped and sorted(taken.values()) == list(range(7)) + [20, 63]
    frame = pp.collisions_depth1(rows)
    want = ref.paths(frame)
    assert len(want["sequences"]) == 9
    check(device_frame(frame).paths(max_paths=16), want)
    check(device_frame(frame).paths(max_paths=9), want)


def test_seventeen_nodes_at_the_capacity_edge():
    """max_paths = 16 gives 64 slots, 17 gives 128: the frame has exactly 17 nodes."""
    assert (pp.capacity_bits(16), pp.capacity_bits(17)) == (6, 7)
    frame = pp.seventeen_nodes()
    want = ref.paths(frame)
    assert len(want["sequences"]) == 17
    check(device_frame(frame).paths(max_paths=17), want)


def test_4096_nodes_and_one_too_few():
    """64 distinct keys in each of 64 waves, in descending surface order: the canonical numbering is the reverse of the
    order the nodes were made in.  max_paths = 4096 holds them exactly; 4095 is refused with the documented message and
    leaves nothing behind."""
    frame = pp.many_nodes()
    assert pp.per_wave(len(frame)) == 64 and pp.workgroups(len(frame)) == 16 and pp.capacity_bits(4096) == 14
    assert pp.capacity_bits(4095) == 14
    want = ref.paths(frame, subtree=ref.subtree_sizes_linear)
    assert len(want["sequences"]) == 4096 and np.array_equal(want["row_node"], np.arange(4096)[::-1])
    device = device_frame(frame)
    check(device.paths(max_paths=4096), want)
    with pytest.raises(ValueError, match="max_paths = 4095 "):
        device.paths(max_paths=4095)
    check(device.paths(max_paths=4096), want)
    check(device.paths(max_paths=4097), want)


# ---- energy_shift at the ends of its range --------------------------------------------------------------------------
BIGGEST = sys.float_info.max


@pytest.mark.parametrize("weights, surfaces, bad, shift", [
    ([0.0, 0.0, 0.0], [2, 2, 4], 0, 62 - 0 - 2),                                     # w_max stays 0
    ([np.nan, -1.0, np.inf, -np.inf, -0.5], [2, 4, 2, 4, 2], 5, 62 - 0 - 3),         # every weight invalid: w_max stays 0
    ([5e-324, 0.0], [2, 4], 0, 62 + 1073 - 2),                                       # a subnormal largest weight
    ([5e-324, 5e-324, 0.0, 5e-324], [2, 2, 4, 4], 0, 62 + 1073 - 3),
    ([BIGGEST, 1.0, 3.5, 1e200], [2, 4, 4, 4], 0, 62 - 1024 - 3),                    # the largest double, once
    ([1.0, BIGGEST, np.nan, 2.0, 1e-300, 7.0], [2, 2, 4, 4, 4, 2], 1, 62 - 1024 - 3),
])
def test_weights_at_the_ends_of_the_shift(weights, surfaces, bad, shift):
    frame = pp.weights_frame(weights, surfaces)
    assert 2 <= len(frame) <= 6
    want = ref.paths(frame)
    assert want["shift"] == shift and want["n_bad_weight"] == bad
    valid = [w for w in weights if np.isfinite(w) and w >= 0]
    if not valid or max(valid) == 0.0:
        assert not want["energy_through"].any() and not want["energy_ended"].any()
    if max(valid, default=0.0) == BIGGEST:   # the others truncate to 0
        assert all(np.floor(np.ldexp(w, shift)) == 0 for w in valid if w != BIGGEST)
        assert np.floor(np.ldexp(BIGGEST, shift)) < 2.0 ** 62 and np.isfinite(want["energy_through"]).all()
    got = device_frame(frame).paths()
    check(got, want)
    if not valid or max(valid) == 0.0:
        assert not got.energy_through.any() and not got.energy_ended.any()
    if max(valid, default=0.0) == 5e-324:  # (exact: one unit of the last place each)
        assert np.array_equal(got.energy_through, want["energy_through"])


@pytest.mark.parametrize("n_rows", (2 ** 6 - 1, 2 ** 6, 2 ** 17 - 1, 2 ** 17))
def test_row_counts_on_both_sides_of_a_bit_length_step(n_rows):
    """B = bit_length(n_rows) steps from k to k + 1 at 2^k rows, and the shift with it: weight 100.0, exact on both
    sides."""
    frame = pp.weights_frame(np.full(n_rows, 100.0), np.arange(n_rows) % 2)
    want = ref.paths(frame)
    k = (n_rows + 1).bit_length() - 1
    assert want["shift"] == 62 - 7 - (k if n_rows == 2 ** k - 1 else k + 1) and want["integer_weights"]
    assert want["energy_through"].tolist() == [[100.0 * ((n_rows + 1) // 2), 100.0 * (n_rows // 2)]]
    check(device_frame(frame).paths(), want)
