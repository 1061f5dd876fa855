"""Shared test helpers: fixture loading, snapshot conversion, frame comparison."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SCENE_KEYS = (
    "prim_type", "prim_material", "prim_normal_scale", "prim_surface_id", "prim_params",
    "prim_minv", "node_op", "node_left", "node_right", "node_prim", "node_aabb", "roots",
    "mat_kind", "mat_coef",
)

# parity bar of BASELINE.json's north_star: surface index bit-exact, everything else 1e-6 abs
ATOL = 1e-6


def load(name):
    with np.load(os.path.join(GOLDEN, name)) as data:
        return {k: data[k] for k in data.files}


def scene_of(fixture, prefix=""):
    """Oracle-format scene dict out of a fixture (optionally key-prefixed ``name__``)."""
    return {k: fixture[prefix + k] for k in SCENE_KEYS}


def flat_scene(snapshot):
    """pyrayt_amd.scene.SceneSnapshot -> the oracle's plain-array scene dict."""
    p, n, m = snapshot.prims, snapshot.nodes, snapshot.materials
    return {
        "prim_type": p["type"].astype(np.int32), "prim_material": p["material"].astype(np.int32),
        "prim_normal_scale": p["normal_scale"].astype(np.int32),
        "prim_surface_id": p["surface_id"].astype(np.int64),
        "prim_params": p["params"].reshape(-1, 6).astype(float),
        "prim_minv": p["minv"].reshape(-1, 16).astype(float),
        "node_op": n["op"].astype(np.int32), "node_left": n["left"].astype(np.int32),
        "node_right": n["right"].astype(np.int32), "node_prim": n["prim"].astype(np.int32),
        "node_aabb": n["aabb"].reshape(-1, 6).astype(float),
        "roots": snapshot.roots.astype(np.int32),
        "mat_kind": m["kind"].astype(np.int32), "mat_coef": m["coef"].reshape(-1, 6).astype(float),
    }


def flat_scene_with_user_materials(snapshot, ray_set_type=None):
    """flat_scene plus what the oracle needs to run a user's index_at / trace() itself: the material objects by
    slot, the surfaces whose material.trace() is user code by primitive index -- for those a stand-in whose
    get_world_normals is the oracle's own (the user's trace() must not need the GPU to be checked)."""
    from oracle import prt_oracle

    flat = flat_scene(snapshot)
    flat["user_materials"] = {slot: material for slot, material in snapshot.table_materials}
    flat["user_surfaces"] = {}
    flat["ray_set_type"] = ray_set_type

    class OracleSurface:
        def __init__(self, prim, surface):
            self._prim, self.material, self._surface = prim, surface.material, surface

        def get_id(self):
            return self._surface.get_id()

        def get_world_normals(self, positions):
            return prt_oracle.world_normals(flat, self._prim, np.asarray(positions, dtype=float).reshape(4, -1))

    for prim, surface in snapshot.host_surfaces:
        flat["user_materials"][int(snapshot.prims["material"][prim])] = surface.material
        flat["user_surfaces"][prim] = OracleSurface(prim, surface)
    return flat


class FixtureSnapshot:
    """Adapter: a fixture's plain-array scene -> the structured arrays DeviceScene uploads."""

    def __init__(self, scene):
        from pyrayt_amd.scene import MATERIAL_DTYPE, NODE_DTYPE, PRIM_DTYPE

        p = np.zeros(len(scene["prim_type"]), dtype=PRIM_DTYPE)
        p["type"], p["material"] = scene["prim_type"], scene["prim_material"]
        p["normal_scale"], p["surface_id"] = scene["prim_normal_scale"], scene["prim_surface_id"]
        p["params"], p["minv"] = scene["prim_params"], scene["prim_minv"]
        n = np.zeros(len(scene["node_op"]), dtype=NODE_DTYPE)
        n["op"], n["left"], n["right"] = scene["node_op"], scene["node_left"], scene["node_right"]
        n["prim"], n["aabb"] = scene["node_prim"], scene["node_aabb"]
        m = np.zeros(max(1, len(scene["mat_kind"])), dtype=MATERIAL_DTYPE)
        m["kind"][: len(scene["mat_kind"])] = scene["mat_kind"]
        m["coef"][: len(scene["mat_kind"])] = scene["mat_coef"]
        self.prims, self.nodes, self.materials = p, n, m
        self.roots = scene["roots"].astype(np.int32)


def device_scene(scene_dict, options=None):
    """A DeviceScene of an oracle-format scene dict."""
    from pyrayt_amd.engine import DeviceScene

    return DeviceScene(FixtureSnapshot(scene_dict), options=options)


def snapshot_of(fixture, prefix=""):
    """A fixture's scene as the structured tables the library takes."""
    return FixtureSnapshot(scene_of(fixture, prefix))


def assert_frames_match(got, want, atol=ATOL, what="frame"):
    """Result frames (R,15): same shape, `surface` (col 5), `generation` and `id` exact, the
    float columns within atol (NaN == NaN)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if got.size == 0:
        return
    for col in (0, 4, 5):
        assert np.array_equal(got[:, col], want[:, col]), f"{what}: exact column {col} differs"
    assert np.allclose(got, want, rtol=0, atol=atol, equal_nan=True), (
        f"{what}: max abs diff {np.nanmax(np.abs(got - want))}")


def _ordered(bits):
    """uint64 views of doubles -> int64 keys whose order is the doubles' order (-0.0 and +0.0 one apart)."""
    bits = bits.astype(np.uint64)
    negative = (bits >> np.uint64(63)).astype(bool)
    magnitude = (bits & np.uint64(0x7FFFFFFFFFFFFFFF)).astype(np.int64)
    return np.where(negative, -magnitude - 1, magnitude)


def differing_bits(got, want):
    """Boolean mask of the elements of two equal-shaped float64 arrays that are not the same double: another bit
    pattern, unless both are NaN (any payload).  -0.0 and +0.0 differ."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    return (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))


def assert_same_bits(got, want, what="array"):
    """Both arrays hold the same doubles: equal shapes, every element equal as a uint64 view (so a zero's sign
    counts), except that a NaN matches any NaN.  The failure message counts the differing elements, names their
    columns (last axis), lists the first few and gives the worst ulp distance over the finite ones."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if got.size == 0:
        return
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    differ = differing_bits(got, want)
    if not differ.any():
        return
    where = np.argwhere(differ)
    columns = sorted(set(where[:, -1].tolist())) if got.ndim > 1 else []
    first = [(*(int(i) for i in index), float(got[tuple(index)]), float(want[tuple(index)])) for index in where[:5]]
    finite = differ & np.isfinite(got) & np.isfinite(want)
    worst = int(np.abs(_ordered(got.view(np.uint64)[finite]) - _ordered(want.view(np.uint64)[finite])).max()) if finite.any() else None
    raise AssertionError(
        f"{what}: {int(differ.sum())} of {got.size} elements differ in their bits, columns {columns}; "
        f"first (index..., got, want): {first}; worst distance over the finite ones: {worst} ulp")


def assert_frames_identical(got, want, what="frame"):
    """Result frames (R,15) that hold the same doubles in every column (assert_same_bits)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.ndim == 2 and got.shape[1] == 15, f"{what}: not a frame, shape {got.shape}"
    assert_same_bits(got, want, what)


# the bar against values the genuine reference (or the numpy oracle, which runs numpy's own sums) wrote: what
# tests/test_c_oracle.py::test_two_oracles_agree holds the two oracles to, three orders above the worst distance
# between the C oracle and any golden frame (8.9e-16, scene_adv_short_c)
REFERENCE_RTOL = REFERENCE_ATOL = 1e-12


def assert_close_to_reference(got, want, what="array"):
    """`got` against values of the reference: finite where it is, equal where it is not finite (same infinity, NaN
    where it has NaN), and within rtol = atol = 1e-12 where it is."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if got.size == 0:
        return
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite), f"{what}: finite in other places than the reference"
    assert np.array_equal(got[~finite], want[~finite], equal_nan=True), f"{what}: differs where the reference is not finite"
    error = np.abs(got[finite] - want[finite])
    bad = error > REFERENCE_ATOL + REFERENCE_RTOL * np.abs(want[finite])
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {got.size} elements beyond rtol = atol = 1e-12 of the reference, "
                           f"max abs diff {error.max()}")


# the scene fixtures whose golden frame (written by the genuine reference) the C oracle -- and so the engine --
# reproduces in every bit, and the four on which a few elements of the float columns 6-14 differ by some ulp
# (tests/test_c_oracle.py::test_trace_matches_reference pins which, how many and why)
EXACT_SCENE_FIXTURES = ("config1", "config2", "config3", "config4", "config5", "two_mirrors", "tutorial",
                        "mirrors_and_stops", "stopped_lens", "stale_box", "adv_lens", "adv_prism", "adv_condenser",
                        "adv_still", "adv_bench_a", "adv_bench_b", "adv_bench_c")
CLOSE_SCENE_FIXTURES = ("adv_short_a", "adv_short_b", "adv_short_c", "adv_stop")


def assert_matches_golden_frame(got, name, want, what=None):
    """A frame against (rows of) the golden frame of scene fixture `name` ("config2" or "scene_config2.npz"): the
    same bits on the fixtures the reference's own frame is reproduced exactly, within 1e-12 of it on the others
    (the four above and those with user materials, which the C oracle does not trace)."""
    short = name[len("scene_"):-len(".npz")] if name.endswith(".npz") else name
    if short in EXACT_SCENE_FIXTURES:
        assert_frames_identical(got, want, what or name)
    else:
        assert_close_to_reference(got, want, what or name)


def host_rank_worker(rank, world, port, name, n, mode, result_dir, gpu_ranks):
    """A gloo rank of tests/test_gpu_distributed.py that may stay off the GPU.  Ranks below `gpu_ranks` run that
    module's _worker (trace their shard on cuda:0, assemble on the device); the others load the rows the parent traced
    for their shard (shard_rows_<rank>.npy, shard_counts_<rank>.npy) and assemble on the host.  Lives here, not in the
    test module, so that a host rank never imports that module (its skip conditions ask torch for the device count)."""
    if rank < gpu_ranks:
        from test_gpu_distributed import _worker

        return _worker(rank, world, port, name, n, mode, result_dir)
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pyrayt_amd import distributed as pdist

        rows = torch.from_numpy(np.load(os.path.join(result_dir, f"shard_rows_{rank}.npy")))
        counts = np.load(os.path.join(result_dir, f"shard_counts_{rank}.npy")).tolist()
        full, full_counts = pdist.assemble_rows(rows, counts, 10, pdist.resolve_group(None), mode)  # (LIMIT there)
        assert not full.is_cuda
        np.save(os.path.join(result_dir, f"rows_{rank}.npy"), full.numpy())
        np.save(os.path.join(result_dir, f"counts_{rank}.npy"), np.array(full_counts))
    finally:
        dist.destroy_process_group()


def psf_synthetic_frame(n=3000, seed=5):
    """Three generations of rays through an index-1.5 slab converging near a focus, two wavelengths, varied weights."""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(4 * n, n, replace=False)).astype(float)
    r, t = np.sqrt(rng.random(n)), rng.random(n) * 2 * np.pi
    p0 = np.stack([np.full(n, -5.0), r * np.cos(t), r * np.sin(t)], 1)
    p1 = p0 + np.array([4.0, 0, 0])
    p2 = p1 + np.array([0.5, 0, 0])
    focus = np.array([10.0, 0.02, -0.01])
    dirn = focus - p2
    dirn /= np.linalg.norm(dirn, axis=1)[:, None]
    p3 = p2 + dirn * ((focus[0] + 0.3 - p2[:, 0]) / dirn[:, 0])[:, None] + rng.normal(0, 2e-5, (n, 3)) * [0, 1, 1]
    wavelength = np.where(rng.random(n) < 0.5, 0.55, 0.65)
    rows = []
    for g, (a, b, index, surf) in enumerate(((p0, p1, 1.0, 1.0), (p1, p2, 1.5, 2.0), (p2, p3, 1.0, 5.0))):
        u = (b - a) / np.linalg.norm(b - a, axis=1)[:, None]
        block = np.zeros((n, 15))
        block[:, 0], block[:, 1], block[:, 2], block[:, 3] = g, 50 + 50 * rng.random(n), wavelength, index
        block[:, 4], block[:, 5], block[:, 6:9], block[:, 9:12], block[:, 12:15] = ids, surf, a, b, u
        rows.append(block)
    return np.concatenate(rows)


def mtf_synthetic_frame(n=3000, seed=7):
    """Two generations; the second ends near a focus at surface 5 along a tilted axis, varied weights, and a few rows
    that must be left out: NaN end points, a NaN weight, directions perpendicular to the axis."""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(4 * n, n, replace=False)).astype(float)
    axis = np.array([1.0, 0.2, 0.0]) / np.linalg.norm([1.0, 0.2, 0.0])  # (u = z is exactly perpendicular to it)
    start = rng.normal(0, 1, (n, 3)) * 0.5 - 5 * axis
    focus = np.array([0.01, -0.02, 0.03])
    u = focus - start + rng.normal(0, 2e-3, (n, 3))
    end = start + u * (0.98 + 0.04 * rng.random(n))[:, None]
    rows = []
    for g, (a, b, surf) in enumerate(((start - u, start, 2.0), (start, end, 5.0))):
        block = np.zeros((n, 15))
        block[:, 0], block[:, 1], block[:, 2], block[:, 3] = g, 50 + 50 * rng.random(n), 0.55, 1.0
        block[:, 4], block[:, 5], block[:, 6:9], block[:, 9:12], block[:, 12:15] = ids, surf, a, b, b - a
        rows.append(block)
    frame = np.concatenate(rows)
    last = frame[:, 0] == 1
    picks = np.flatnonzero(last)[[3, 10, 500, 2000, 2900]]
    frame[picks[0], 10] = np.nan
    frame[picks[1], 1] = np.nan
    perpendicular = np.array([0.0, 0.0, 1.0])
    frame[picks[2], 12:15] = perpendicular
    frame[picks[3], 12:15] = perpendicular * 3
    frame[picks[4], 14] = np.inf
    return frame, axis
