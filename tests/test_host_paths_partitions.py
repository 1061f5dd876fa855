"""The frames of tests/paths_partitions.py on the host (CPU): that the restated plan is the one in prt_paths.hpp, that
every builder makes what its case claims -- the per_wave values, the row of a run at which a key or a group changes, the
cells the four waves of a workgroup end on, the slots the aimed keys start at and the wrap of their probes, the node
counts -- and that tests/paths_reference.py runs on them.  tests/test_gpu_paths_partitions.py compares the device with the
same frames and the same references."""
import os
import re

import numpy as np
import pytest

import helpers
import paths_partitions as pp
import paths_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IX = ref.IX


def source():
    with open(os.path.join(ROOT, "pyrayt_amd", "csrc", "prt_paths.hpp")) as handle:
        return handle.read()


def changes(values):
    """The rows of a run (from 1) whose value differs from the row before."""
    return (np.flatnonzero(values[1:] != values[:-1]) + 1).tolist()


def test_the_restated_plan_is_the_one_in_the_source():
    text = source()
    assert re.search(r"kPathsBlock = (\d+);", text).group(1) == str(pp.BLOCK)
    assert re.search(r"kPathsGrid = (\d+);", text).group(1) == str(pp.GRID)
    assert pp.WAVES == pp.BLOCK // 64 and "kPathsWaves = kPathsBlock / 64" in text
    assert "key * 0x%xull) >> hash_shift" % pp.GOLDEN in text and "64 - bits, max_paths" in text
    assert "(slot + 1) & (unsigned)(capacity - 1)" in text
    assert "(n + kPathsGrid * kPathsBlock - 1) / (kPathsGrid * kPathsBlock)) * 64" in text
    assert "int bits = 6;" in text and "((int64_t)1 << bits) < 4 * (int64_t)max_paths" in text
    assert "((u64)(unsigned)(parent + 1) << 32) | (u64)(unsigned)(int)s" in text
    # run(): 64 rows up to 131 072, 128 from 131 073, 192 from 262 145
    assert [pp.per_wave(n) for n in (1, 64, 65, 131_072, 131_073, 262_144, 262_145, 393_216, 393_217)] == \
        [64, 64, 64, 64, 128, 128, 192, 192, 256]
    assert [pp.workgroups(n) for n in (1, 256, 257, 131_072, 131_073, 262_144, 262_145)] == [1, 1, 2, 512, 257, 512, 342]
    assert [pp.capacity_bits(n) for n in (1, 16, 17, 32, 33, 4095, 4096, 4097, 65536)] == [6, 6, 7, 7, 8, 14, 14, 15, 18]


def test_the_aimed_keys_start_where_they_are_said_to():
    assert {pp.slot(surface, 6) for surface in pp.DEPTH0} == {62, 63}
    assert pp.slot(pp.PARENT, 6) == 20
    assert {pp.slot(pp.child_key(20, surface), 6) for surface in pp.DEPTH1} == {63}
    taken, wrapped = pp.probe(pp.DEPTH0, 6)
    assert wrapped and sorted(taken.values()) == list(range(14)) + [62, 63]
    assert pp.probe(pp.DEPTH0[::-1], 6)[1] and sorted(pp.probe(pp.DEPTH0[::-1], 6)[0].values()) == sorted(taken.values())
    taken, wrapped = pp.probe([pp.PARENT] + [pp.child_key(20, surface) for surface in pp.DEPTH1], 6)
    assert wrapped and sorted(taken.values()) == list(range(7)) + [20, 63]
    # one node more: 128 slots, and the same keys no longer meet
    assert pp.capacity_bits(17) == 7 and len({pp.slot(surface, 7) for surface in pp.DEPTH0}) > 2


@pytest.mark.parametrize("name", sorted(pp.LARGE))
def test_the_large_frames_are_arranged_as_claimed(name):
    counts, rays_per_source = pp.LARGE[name]
    frame, _, n_groups, want = pp.large(name)
    assert pp.counts_of(frame) == list(counts) and len(want["sequences"]) <= pp.MAX_PATHS
    runs = [pp.per_wave(count) for count in counts]
    assert runs == {"262145_131073_131072": [192, 128, 64], "262144_131073": [128, 128],
                    "131073_131072_70000": [128, 64, 64], "262145": [192]}[name]
    assert want["integer_weights"] and frame[:, IX["intensity"]].max() < 200 and want["n_bad_weight"] == 0
    count, run = counts[0], runs[0]
    node = want["row_node"][:count]
    group = np.arange(count) // rays_per_source
    # every id in a group, the last row of the first generation -- alone in its wave where the count is odd -- too
    assert (count - 1) // rays_per_source == n_groups - 1 and np.all(want["row_node"] >= 0)
    assert want["through"].sum() == len(frame) and want["through"][n_groups - 1].sum() >= 1
    assert want["ended"].sum() == count and want["ended"][n_groups - 1].sum() >= 1
    # ... and with BEYOND groups fewer the last ids lie beyond the groups: their rows keep their nodes and leave the tables
    fewer = n_groups - pp.BEYOND
    cut = pp.fewer_groups(want, fewer)
    assert count > fewer * rays_per_source
    assert cut["through"].sum() == sum(min(c, fewer * rays_per_source) for c in counts) < len(frame)
    slices = run // 64
    expected = dict(boundary=[64, 128][:slices - 1], before=[63, 127][:slices - 1] + ([191] if slices == 3 else []),
                    after=[65, 129][:slices - 1], alternate=list(range(1, run)), aba=[64, 128][:slices - 1],
                    one_cell=[], four_cells=[], aaba=[])
    if run == 128:
        expected["before"] = [63, 127]
    for number, arrangement in enumerate(pp.ARRANGEMENTS):
        for block in (number, number + 8 * 5):
            ends = []
            for wave in range(pp.WAVES):
                first = (block * pp.WAVES + wave) * run
                assert first + run <= count
                assert changes(node[first:first + run]) == expected[arrangement], (arrangement, wave)
                ends.append((int(group[first + run - 1]), int(node[first + run - 1])))
                if arrangement == "aba" and slices == 3:
                    assert node[first] == node[first + 128] != node[first + 64]
                if arrangement == "alternate":
                    assert all(len(set(node[first + 64 * s:first + 64 * s + 64])) == 3 for s in range(slices))
            if rays_per_source == 3072:  # (every workgroup inside one group: the cells are the nodes)
                assert len({g for g, _ in ends}) == 1
                if arrangement == "one_cell":
                    assert len(set(ends)) == 1
                if arrangement == "four_cells":
                    assert len(set(ends)) == 4
                if arrangement == "aaba":
                    assert ends[0] == ends[1] == ends[3] != ends[2]
    # where the groups change within a run
    inside = [p for p in range(rays_per_source, 4096, rays_per_source) if p % run]
    if rays_per_source == 192:
        assert inside and all(p % 64 == 0 for p in inside)          # at slice boundaries
    if rays_per_source == 100:
        assert sum(p % 64 != 0 for p in inside) > 30                # inside slices
    if rays_per_source == 3072:
        assert not inside and 3072 % (run * pp.WAVES) == 0
    # the ragged end: 131 073 rows leave one row to the last workgroup (one live wave, three empty); 262 145 leave it
    # 257, a whole run and a run of one slice and one row
    left = count - (pp.workgroups(count) - 1) * run * pp.WAVES
    assert left == {131_073: 1, 262_145: 257, 262_144: 512}[count]
    # a key met again in a later generation under another parent is another node
    assert len(want["sequences"]) > 4 or len(counts) == 1


@pytest.mark.parametrize("n_ids", (131_072, 131_073))
def test_the_frames_for_the_end_of_the_rays(n_ids):
    frame, marked, want = pp.ended(n_ids)
    run = pp.per_wave(n_ids)
    assert run == (64 if n_ids == 131_072 else 128) and want["id0"] == 500.0 and len(want["ray_node"]) == n_ids
    never = np.flatnonzero(want["ray_node"] < 0)
    assert len(never) > 1000 and np.all(never % 97 == 5) and np.all(want["ray_last_row"][never] == -1)
    assert want["n_rays"] == n_ids - len(never)
    # the marked lanes: the first and the last of a run, and the single ragged one
    assert {0, run - 1, run, 2 * run - 1, n_ids - 1} <= set(marked.tolist()) and np.all(want["ray_node"][marked] >= 0)
    assert {int(m) % run for m in marked} == {0, run - 1}
    if n_ids == 131_073:
        assert (n_ids - 1) % run == 0 and pp.workgroups(n_ids) == 257     # (one id in the last wave)
    last = want["ray_last_row"][marked]
    dark = np.all(frame[last, 12:15] == 0.0, axis=1)
    bad = ~(np.isfinite(frame[last, IX["intensity"]]) & (frame[last, IX["intensity"]] >= 0))
    assert dark.sum() >= 4 and bad.sum() >= 4 and (dark & bad).sum() >= 1 and (dark & ~bad).sum() >= 1
    # every marked ray lies in a group, so its last row reaches ended, dark and energy_ended: the ray of the last id --
    # in the last wave, alone there at 131 073 -- ends dark with a weight that does not count, in the last group
    groups = (frame[last, IX["id"]] // pp.END_RAYS_PER_SOURCE).astype(int)
    assert np.all(groups < pp.END_GROUPS) and groups[-1] == pp.END_GROUPS - 1 and marked[-1] == n_ids - 1
    in_last_wave = marked // run == (n_ids - 1) // run
    assert dark[-1] and bad[-1] and in_last_wave.sum() == (2 if n_ids == 131_072 else 1)
    if n_ids == 131_072:  # (the first lane of the last wave: dark, with a weight that counts)
        assert in_last_wave[-2] and dark[-2] and not bad[-2]
    assert want["n_bad_weight"] == bad.sum() and want["dark"].sum() == dark.sum()
    assert [int(want["dark"][g].sum()) for g in range(pp.END_GROUPS)] == [int(dark[groups == g].sum()) for g in range(pp.END_GROUPS)]
    assert want["integer_weights"] and want["ended"].sum() == want["n_rays"]
    two = pp.fewer_groups(want, 2)                                             # (ids from 100 000: beyond two groups)
    assert two["ended"].sum() < want["n_rays"] and two["dark"].sum() < want["dark"].sum()
    # rays that die after one row and rays that live on, so the last rows lie in both generations
    assert 0 < (want["ray_last_row"] >= pp.counts_of(frame)[0]).sum() < want["n_rays"]


def test_the_frames_aimed_at_the_table():
    for rows in (16, 16_384):
        frame = pp.collisions_depth0(rows)
        want = ref.paths(frame)
        assert len(want["sequences"]) == 16 and want["surface"].tolist() == sorted(pp.DEPTH0)
        assert pp.per_wave(rows) == 64 and pp.workgroups(rows) == (1 if rows == 16 else 64)
    assert all(len(set(frame[64 * w:64 * w + 64, IX["surface"]])) == 16 for w in range(256))
    assert len({tuple(frame[64 * w:64 * w + 16, IX["surface"]]) for w in range(256)}) == 16   # (every rotation leads)
    for rows in (8, 16_384):
        want = ref.paths(pp.collisions_depth1(rows))
        assert want["sequences"] == [(pp.PARENT,)] + [(pp.PARENT, surface) for surface in pp.DEPTH1]
    want = ref.paths(pp.seventeen_nodes())
    assert len(want["sequences"]) == 17
    frame = pp.many_nodes()
    want = ref.paths(frame, subtree=ref.subtree_sizes_linear)
    assert len(want["sequences"]) == 4096 and pp.per_wave(4096) == 64 and pp.workgroups(4096) == 16
    assert all(len(set(frame[64 * w:64 * w + 64, IX["surface"]])) == 64 for w in range(64))
    assert np.all(np.diff(frame[:, IX["surface"]]) < 0) and np.array_equal(want["row_node"], np.arange(4096)[::-1])
    assert np.all(want["subtree_size"] == 1)


@pytest.mark.parametrize("name", ["stale_box", "mirrors_and_stops", "adv_short_b", "adv_lens", "stopped_lens",
                                  "two_mirrors", "config2"])
def test_the_linear_subtree_count_is_the_quadratic_one(name):
    want = ref.paths(helpers.load(f"scene_{name}.npz")["frame"])
    assert np.array_equal(ref.subtree_sizes_linear(want["sequences"]), want["subtree_size"])
    assert np.array_equal(ref.subtree_sizes(want["sequences"]), want["subtree_size"])


def test_fewer_groups_are_the_first_rows_of_the_tables():
    frame = pp.arranged((3000, 2000))
    full = ref.paths(frame, rays_per_source=192, n_groups=12)
    for n_groups in (1, 3):
        cut, want = pp.fewer_groups(full, n_groups), ref.paths(frame, rays_per_source=192, n_groups=n_groups)
        assert sorted(cut) == sorted(want)
        for name in want:
            assert np.array_equal(cut[name], want[name]) if isinstance(want[name], np.ndarray) else cut[name] == want[name]


def test_the_weight_frames():
    frame = pp.weights_frame([0.0, 5e-324, 0.0], surfaces=[2, 2, 4])
    want = ref.paths(frame)
    assert want["shift"] == 62 + 1073 - 2 and not want["integer_weights"]
    assert want["energy_through"].tolist() == [[5e-324, 0.0]]
