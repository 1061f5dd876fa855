"""The host side of the ray-path analysis (CPU): argument checks that come before any GPU call, the ABI entries, the
library's own refusals, the Paths object's host logic (merge, the subtree range test, find, fates) on what the numpy /
dict restatement (tests/paths_reference.py) makes of the golden frames, and the kernels' resources."""
import os
import re

import numpy as np
import pytest

import helpers
import paths_reference as ref
from pyrayt_amd.frame import DeviceFrame, Paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# fixture -> (distinct complete paths, rays, longest path): the surface sequence per id, computed on the host
KNOWN = {"stale_box": (114, 890, 6), "mirrors_and_stops": (66, 693, 6), "adv_short_b": (55, 179, 6),
         "adv_lens": (27, 1971, 6), "stopped_lens": (2, 2048, 3), "two_mirrors": (1, 10, 10), "config2": (1, 2048, 3)}
_CACHE = {}


def reference(name):
    if name not in _CACHE:
        _CACHE[name] = ref.paths_object(helpers.load(f"scene_{name}.npz")["frame"])
    return _CACHE[name]


def host_frame():
    rows = np.zeros((15, 4))
    rows[0] = [0, 0, 1, 1]
    rows[4] = [0, 1, 0, 1]
    rows[5] = [1, 1, 2, 2]
    rows[12] = 1.0
    return DeviceFrame(rows, [2, 2])


def test_paths_arguments_are_checked_before_the_gpu():
    frame = host_frame()
    with pytest.raises(ValueError, match="weights"):
        frame.paths(weights="brightness")
    for bad in (0, 65537, -1, 2.5, True, None, "many"):
        with pytest.raises(ValueError, match="max_paths"):
            frame.paths(max_paths=bad)
    with pytest.raises(ValueError, match="where"):
        frame.where(surface=1).paths()
    with pytest.raises(ValueError, match="select"):
        frame.select(np.array([True, True, False, False])).paths()
    with pytest.raises(ValueError, match="generation"):
        frame.generation(0).paths()
    cut = DeviceFrame(np.zeros((15, 4)), [2, 2])
    cut.origin = "record_only"
    with pytest.raises(ValueError, match="record_only"):
        cut.paths()
    with pytest.raises(ValueError, match="rows_per_generation"):
        DeviceFrame(np.zeros((15, 4))).paths()
    narrow = DeviceFrame(np.zeros((15, 2)), [2], columns=(0, 4, 5))
    with pytest.raises(ValueError, match="without the column"):
        narrow.paths()


def test_abi_entries_are_declared_and_bound():
    from pyrayt_amd import engine

    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("prt_frame_paths_workspace_bytes", "prt_frame_paths"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    assert engine.PRT_VERSION == 240 and "#define PRT_VERSION 240" in header
    if os.path.exists(engine.LIB_PATH):
        lib = engine.library()
        assert len(lib.prt_frame_paths.argtypes) == 20 and len(lib.prt_frame_paths_workspace_bytes.argtypes) == 4


def test_library_checks_paths_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    assert lib.prt_frame_paths_workspace_bytes(3000, 1000, 2, 4096) > 16384 * 8 * (1 + 2 * 5) + 1000 * 4
    assert lib.prt_frame_paths_workspace_bytes(0, 1, 1, 1) > 0
    assert lib.prt_frame_paths_workspace_bytes(3000, 1000, 25, 65536) > 0
    for args in ((3000, 1000, 2, 0), (3000, 1000, 2, 65537), (3000, 1000, 0, 4096), (-1, 1000, 2, 4096),
                 (3000, -1, 2, 4096), (3000, 0, 2, 4096), (3000, 2 ** 31 + 1, 2, 4096), (3000, 1000, -1, 4096),
                 (3000, 1000, 2, -1), (3000, 1000, 26, 65536), (3000, 1000, 2 ** 20, 64)):  # (the last two: the cap)
        assert lib.prt_frame_paths_workspace_bytes(*args) == -1, args
    buf = np.zeros(64)
    p = buf.ctypes.data
    counts = np.array([2, 2], dtype=np.int64)

    def call(rows=p, ld=4, counts=counts, n_generations=2, id0=0.0, n_ids=2, rays_per_source=0.0, n_groups=1, weight=1,
             max_paths=16, row_node=p, ray_node=p, last_row=p, node=p, count=p, energy=p, record=p, work=p):
        return lib.prt_frame_paths(0, rows, ld, counts.ctypes.data if counts is not None else None, n_generations, id0,
                                   n_ids, rays_per_source, n_groups, weight, max_paths, row_node, ray_node, last_row,
                                   node, count, energy, record, work, None)

    for kwargs, message in ((dict(max_paths=0), "max_paths in [1, 65536]"),
                            (dict(max_paths=65537), "max_paths in [1, 65536]"),
                            (dict(n_groups=0), "bad buffers"),
                            (dict(n_groups=2), "one group without rays_per_source"),
                            (dict(n_groups=26, rays_per_source=1.0, max_paths=65536), "256 MiB table cap"),
                            (dict(weight=15), "weight_column"),
                            (dict(weight=-2), "weight_column"),
                            (dict(n_ids=0), "n_ids in [1, 2^31]"),
                            (dict(n_ids=2 ** 31 + 1), "n_ids in [1, 2^31]"),
                            (dict(id0=float("nan")), "id0 finite"),
                            (dict(id0=float("inf")), "id0 finite"),
                            (dict(counts=np.array([2, -1], dtype=np.int64)), "counts >= 0"),
                            (dict(counts=None), "bad buffers"),
                            (dict(n_generations=-1), "bad buffers"),
                            (dict(ld=3), "bad buffers"),
                            (dict(rows=None), "bad buffers"),
                            (dict(row_node=None), "bad buffers"),
                            (dict(ray_node=None), "bad buffers"),
                            (dict(last_row=None), "bad buffers"),
                            (dict(node=None), "bad buffers"),
                            (dict(count=None), "bad buffers"),
                            (dict(energy=None), "bad buffers"),
                            (dict(record=None), "bad buffers"),
                            (dict(work=None), "bad buffers")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())


def test_paths_kernels_use_no_scratch():
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pyrayt_amd import engine

    if not os.path.exists(mod.READELF):
        pytest.skip("llvm-readelf not available")
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    kernels = {name: res for name, res in mod.kernel_resources(engine.LIB_PATH).items() if "k_paths_" in name}
    for wanted in ("weight_max", "step", "end", "remap"):
        assert any("k_paths_" + wanted in name for name in kernels), (wanted, sorted(kernels))
    for name, res in kernels.items():
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (name, res)
        assert res["sgpr_spill_count"] == 0 and res["group_segment_fixed_size"] <= 1024, (name, res)


# ---- the restatement on the golden frames, and the Paths object on the restatement -------------------------------------
@pytest.mark.parametrize("name", sorted(KNOWN))
def test_restatement_gives_the_known_paths_of_the_golden_frames(name):
    paths, raw = reference(name)
    complete, rays, longest = KNOWN[name]
    assert len(paths.complete()) == complete and raw["n_rays"] == rays == paths.n_rays
    assert raw["depth"].max() + 1 == longest
    assert paths.sequences == raw["sequences"] == sorted(raw["sequences"])
    assert paths.ended.sum() == rays and paths.through[0, paths.depth == 0].sum() == rays
    # a node's rows are its own ends plus its children's rows
    for k in range(paths.n_nodes):
        assert paths.through[0, k] == paths.ended[0, k] + paths.through[0, paths.parent == k].sum()
        assert paths.energy_through[0, k] == paths.energy_ended[0, k] + paths.energy_through[0, paths.parent == k].sum()
    assert np.array_equal(np.bincount(raw["row_node"], minlength=paths.n_nodes), paths.through[0])


def test_refusals_of_the_restatement():
    frame = helpers.load("scene_stopped_lens.npz")["frame"].copy()
    for column, row, value, message in (("id", 5, frame[6, 4], "repeats"), ("id", 5, 0.5, "id is not an integer"),
                                        ("surface", 5, 1.5, "surface"), ("surface", 5, -1.0, "surface")):
        bad = frame.copy()
        bad[row, ref.IX[column]] = value
        with pytest.raises(ValueError, match=message):
            ref.paths(bad)
    late = np.flatnonzero(frame[:, 0] == 2)[0]
    gone = np.flatnonzero((frame[:, 0] == 1) & (frame[:, 4] == frame[late, 4]))[0]
    with pytest.raises(ValueError, match="none in the one before"):
        ref.paths(np.delete(frame, gone, axis=0))


def test_subtree_is_a_range_and_rays_is_the_range_test():
    paths, raw = reference("stale_box")
    for k, sequence in enumerate(paths.sequences):
        inside = [n for n, other in enumerate(paths.sequences) if other[:len(sequence)] == sequence]
        assert inside == list(range(k, k + paths.subtree_size[k]))
    # with the per-ray array in place of the device tensor: rays() against the paths themselves
    frame = helpers.load("scene_stale_box.npz")["frame"]
    live = Paths(paths.parent, paths.surface, paths.depth, paths.subtree_size, paths.through, paths.ended, paths.dark,
                 paths.energy_through, paths.energy_ended, ray_node=raw["ray_node"], row_node=raw["row_node"],
                 ray_last_row=raw["ray_last_row"], id0=raw["id0"], ids=frame[:, ref.IX["id"]])
    rows_of = ref.ray_rows(frame)
    for k in (0, 3, int(np.argmax(paths.subtree_size)), paths.n_nodes - 1):
        sequence = paths.sequences[k]
        exact = sorted(ray for ray, rows in rows_of.items() if tuple(frame[rows, 5].astype(int)) == sequence)
        prefix = sorted(ray for ray, rows in rows_of.items() if tuple(frame[rows, 5].astype(int))[:len(sequence)] == sequence)
        assert list(np.flatnonzero(live.rays(k)) + int(raw["id0"])) == exact
        assert list(np.flatnonzero(live.rays(k, complete=False)) + int(raw["id0"])) == prefix
        assert len(prefix) == paths.through[0, k] and len(exact) == paths.ended[0, k]
        assert sorted(np.flatnonzero(live.rows(k))) == sorted(row for ray in exact for row in rows_of[ray])
    both = live.rays([0, 3])
    assert both.sum() == paths.ended[0, 0] + paths.ended[0, 3]
    with pytest.raises(ValueError, match="node"):
        live.rays(paths.n_nodes)
    with pytest.raises(ValueError, match="merge"):
        paths.rays(0)


def test_find_index_and_complete():
    paths, raw = reference("stopped_lens")
    assert paths.sequences == [(0,), (3,), (3, 4), (3, 4, 6)]
    assert list(paths.complete()) == [0, 3] and list(paths.ended[0]) == [1601, 0, 0, 447]
    assert paths.index((3, 4)) == 2 and paths.index([3, 4, 6]) == 3
    with pytest.raises(ValueError, match="no ray"):
        paths.index((4, 3))

    class Surface:
        def __init__(self, number):
            self.number = number

        def get_id(self):
            return self.number

    assert list(paths.find(through=(3, 4))) == [2, 3] and list(paths.find(through=Surface(4))) == [2, 3]
    assert list(paths.find(ends_at=6)) == [3] and list(paths.find(ends_at=Surface(6), through=[Surface(3)])) == [3]
    assert list(paths.find(avoids=3)) == [0] and list(paths.find(avoids=[0, 6])) == [1, 2]
    assert list(paths.find()) == [0, 1, 2, 3] and list(paths.find(through=7)) == []
    assert paths.index((Surface(3), 4)) == 2
    table = paths.to_pandas()
    assert list(table.columns) == ["source_id", "node", "parent", "depth", "surface", "sequence", "through", "ended",
                                   "dark", "energy_through", "energy_ended"]
    assert table.shape == (4, 11) and table["sequence"][3] == (3, 4, 6) and table["energy_ended"][3] == 44700.0


def test_fates():
    paths, raw = reference("stopped_lens")
    fates = paths.fates()
    assert fates.values.tolist() == [[0, 0, 1601, 0, 1601, 160100.0], [0, 6, 447, 0, 447, 44700.0]]
    fates = paths.fates(launched=2100)
    assert fates.values.tolist()[0] == [0, -1, 52, 0, 52, 0.0] and len(fates) == 3
    # per source, with absorbed rays: the mirrors-and-stops frame by groups of 512 ids
    # (no golden frame holds an absorbed ray's zero direction: every third last row is given one here)
    frame = helpers.load("scene_mirrors_and_stops.npz")["frame"].copy()
    frame[sorted(rows[-1] for rows in ref.ray_rows(frame).values())[::3], 12:15] = [0.0, 1e-9, 0.0]
    n_groups = int(frame[:, 4].max() // 512) + 1
    grouped, raw = ref.paths_object(frame, rays_per_source=512, n_groups=n_groups)
    fates = grouped.fates(launched=512)
    last = {ray: rows[-1] for ray, rows in ref.ray_rows(frame).items()}
    for g in range(n_groups):
        mine = [row for ray, row in last.items() if ray // 512 == g]
        lines = fates[fates["source_id"] == g].set_index("surface")
        assert lines.loc[-1, "ended"] == 512 - len(mine)
        for surface in set(frame[mine, 5]):
            at = [row for row in mine if frame[row, 5] == surface]
            is_dark = int((np.sqrt((frame[at, 12:15] ** 2).sum(1)) <= 1e-8).sum())
            assert tuple(lines.loc[int(surface), ["ended", "dark", "escaped"]]) == (len(at), is_dark, len(at) - is_dark)
        assert lines["ended"].sum() == 512
    assert fates["dark"].sum() == raw["dark"].sum() > 0


def test_merge_by_component():
    paths, raw = reference("adv_lens")
    frame = helpers.load("scene_adv_lens.npz")["frame"]
    surfaces = sorted(set(frame[:, 5].astype(int)))
    labels = {s: ("lens" if k < 3 else "rest") for k, s in enumerate(surfaces)}
    rows_of = ref.ray_rows(frame)

    def relabel(sequence, collapse):
        out = []
        for s in sequence:
            if not (collapse and out and out[-1] == labels[s]):
                out.append(labels[s])
        return tuple(out)

    for collapse in (False, True):
        merged = paths.merge(labels, collapse_repeats=collapse)
        full = {ray: relabel(tuple(frame[rows, 5].astype(int)), collapse) for ray, rows in rows_of.items()}
        prefixes = sorted({p[:k] for p in full.values() for k in range(1, len(p) + 1)})
        assert merged.sequences == prefixes and merged.ray_node is None and merged.row_node is None
        for k, sequence in enumerate(prefixes):
            assert merged.ended[0, k] == sum(1 for p in full.values() if p == sequence)
            assert merged.through[0, k] == sum(1 for p in full.values() if p[:len(sequence)] == sequence)
            assert merged.parent[k] == (prefixes.index(sequence[:-1]) if len(sequence) > 1 else -1)
            assert merged.depth[k] == len(sequence) - 1
            assert merged.subtree_size[k] == sum(1 for p in prefixes if p[:len(sequence)] == sequence)
        assert merged.ended.sum() == paths.ended.sum() and merged.dark.sum() == paths.dark.sum()
        assert merged.energy_ended.sum() == paths.energy_ended.sum()
        assert [merged.sequences[m] for m in merged.node_map] == [relabel(s, collapse) for s in paths.sequences]
    # a map that names no surface changes nothing
    same = paths.merge({})
    assert same.sequences == paths.sequences and np.array_equal(same.through, paths.through)
    assert np.array_equal(same.energy_through, paths.energy_through) and np.array_equal(same.subtree_size, paths.subtree_size)
