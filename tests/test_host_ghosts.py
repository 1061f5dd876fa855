"""The host side of the ghost pass (CPU): the numpy restatement of the definitions (tests/ghost_reference.py) on frames of
the C oracle, with tests/fresnel_reference.py for the transmittance -- its bookkeeping, the open-row rule, the energy
balance over three orders, closed forms of a plate -- and the refusals that come before any GPU call, and the ABI."""
import os
import re

import numpy as np
import pytest

import fresnel_reference as fref
import ghost_reference as ref
import ghost_scenes as gs

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IX = fref.IX
X = np.array([1.0, 0.0, 0.0])
TOL = 32 * np.finfo(np.float64).eps  # (tests/test_gpu_fresnel.py's bar against power_coefficients, per interface)


# ---- bookkeeping --------------------------------------------------------------------------------------------------------
def fan(n, seed=3):
    """n rays through a plate (surfaces 1, 2, then 3) at their own angles; every third ends inside the glass, every
    fifth on the first face; the glass differs from ray to ray."""
    rng = np.random.default_rng(seed + n)
    rays = []
    for k in range(n):
        theta, index = rng.uniform(0.05, 1.2), rng.choice([1.46, 1.5, 1.8])
        u = np.array([np.cos(theta), np.sin(theta), 0.0])
        segments = [(u, 1.0, 1), (fref.snell(u, X, 1.0, index), index, 2), (u, 1.0, 3)]
        rays.append(segments[:1 if k % 5 == 4 else 2 if k % 3 == 2 else 3])
    frame = fref.synthetic(rays)
    frame[:, IX["x1"]:IX["z1"] + 1] = rng.normal(size=(len(frame), 3))
    return frame


def test_buckets_groups_stride_ids_and_the_stable_order():
    frame = fan(40)
    t = fref.fresnel(frame)["transmittance"]
    got = ref.ghosts(frame, t, [2, 7, 1], rays_per_group=8, n_groups=5)
    # the same, row by row: the interface at the end of row p is seen through the ray's next row
    wanted = []
    for p, row in enumerate(frame):
        later = np.flatnonzero((frame[:, IX["id"]] == row[IX["id"]]) & (frame[:, IX["generation"]] == row[IX["generation"]] + 1))
        if len(later) and row[IX["surface"]] in (1, 2):
            bucket = int(row[IX["id"]] // 8) * 3 + [2, 7, 1].index(int(row[IX["surface"]]))
            wanted.append((bucket, p))
    wanted.sort()
    assert got["parent_row"].tolist() == [p for _, p in wanted] and got["n_spawned"] == len(wanted) > 40
    counts = np.bincount([b for b, _ in wanted], minlength=15)
    assert got["counts"].tolist() == counts.tolist() and got["stride"] == counts.max()
    assert got["bucket"].tolist() == np.flatnonzero(counts).tolist() and got["n_groups"] == 10  # (surface 7 is never met)
    assert got["keys"].tolist() == [[b // 3, [2, 7, 1][b % 3]] for b in np.flatnonzero(counts)]
    ids, at = [], 0
    for group, bucket in enumerate(np.flatnonzero(counts)):
        ids += [group * counts.max() + rank for rank in range(counts[bucket])]
    assert got["rays"][12].tolist() == ids and len(set(ids)) == len(ids)
    ended = [k for k in range(40) if k % 5 == 4 or k % 3 == 2]  # (on the first face, or inside the glass on the second)
    assert (got["n_open"], got["n_dropped"], got["n_dark"], got["n_invalid"]) == (len(ended), 0, 0, 0)
    # the payload: generation 0, w = 1, the parent's wavelength and the index before the surface, e = I (T[p] - T[j])
    rays, p = got["rays"], got["parent_row"]
    assert not rays[8].any() and not rays[7].any() and np.all(rays[3] == 1.0)
    assert np.array_equal(rays[10], frame[p, IX["wavelength"]]) and np.array_equal(rays[11], frame[p, IX["index"]])
    assert np.all(rays[9] > 0) and np.all(np.abs(np.linalg.norm(rays[4:7], axis=0) - 1.0) <= TOL)
    normal_part = rays[4] * frame[p, 12] / np.linalg.norm(frame[p, 12:15], axis=1)
    assert np.all(normal_part < 0)  # (reflected at faces normal to x: back towards -x)
    # a threshold drops the weak ones and counts them; groups and ids follow what is left
    cut = float(np.median(rays[9]))
    fewer = ref.ghosts(frame, t, [2, 7, 1], rays_per_group=8, n_groups=5, min_intensity=cut)
    assert fewer["n_spawned"] == int((rays[9] >= cut).sum()) and fewer["n_dropped"] == int((rays[9] < cut).sum()) > 0
    assert np.all(fewer["rays"][9] >= cut)
    with pytest.raises(ValueError, match="n_groups"):
        ref.ghosts(frame, t, [1, 2], rays_per_group=8, n_groups=4)
    with pytest.raises(ValueError, match="distinct"):
        ref.ghosts(frame, t, [1, 1])


def test_mirrors_undeviated_rays_and_lossless_surfaces_spawn_nothing():
    u = np.array([np.cos(0.3), np.sin(0.3), 0.0])
    normal = np.array([np.cos(1.1), np.sin(1.1), 0.0])
    frame = fref.synthetic([[(u, 1.0, 1), (fref.mirror(u, normal), 1.0, 2), (fref.mirror(u, normal), 1.0, 3)],
                            [(X, 1.0, 1), (X, 1.5, 2), (X, 1.0, 3)]])
    got = ref.ghosts(frame, fref.fresnel(frame)["transmittance"], [1, 2])
    assert got["parent_row"].tolist() == [1, 3] and got["n_open"] == 0
    assert np.all(np.abs(got["rays"][9] - [4.0, 3.84]) <= 100 * 3 * TOL) and got["rays"][4].tolist() == [-1.0, -1.0]
    coated = ref.ghosts(frame, fref.fresnel(frame, lossless=(1,))["transmittance"], [1, 2])
    assert coated["parent_row"].tolist() == [3] and coated["n_dark"] == 1


# ---- frames of the C oracle ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lens_orders():
    parts, rays, det = gs.lens(300)
    return parts, det, gs.reference_orders(parts, rays, 3, rays_per_group=300, n_groups=1)


def test_without_a_housing_the_reflections_are_not_seen():
    parts, rays, det = gs.lens(64, housing=False)
    orders = gs.reference_orders(parts, rays, 2, rays_per_group=64)
    assert orders[1]["ghosts"]["n_open"] == 0  # (every signal ray goes on to the detector)
    front = int(orders[0]["frame"][0, IX["surface"]])
    first = orders[1]["frame"]
    assert len(first) == 64 and set(first[:, IX["surface"]]) == {front}  # (order 1 dies unseen at the front surface)
    assert orders[2]["ghosts"]["n_open"] == 64 and orders[2]["ghosts"]["rays"].shape == (13, 0) and len(orders[2]["frame"]) == 0


def test_in_a_housing_one_path_reaches_the_detector(lens_orders):
    parts, det, orders = lens_orders
    front = int(orders[0]["frame"][0, IX["surface"]])
    back = int(orders[0]["frame"][300, IX["surface"]])
    assert front != back and all(o["ghosts"]["n_open"] == 0 for o in orders[1:])
    found = []
    for k in (1, 2):
        frame, children = orders[k]["frame"], orders[k]["ghosts"]
        on = frame[frame[:, IX["surface"]] == det.get_id()]
        found += [(k, *gs.path(orders, k, int(g))) for g in sorted(set(on[:, IX["id"]] // children["stride"]))]
    assert found == [(2, (back, front), 0)]


def test_the_energy_of_three_orders_is_the_energy_launched(lens_orders):
    parts, det, orders = lens_orders
    surfaces = gs.refracting(parts)
    launched = ref.energy(orders[0]["frame"][:300, IX["intensity"]])
    total, deepest = 0, 0
    for o in orders:
        frame, t = o["frame"], o["fresnel"]["transmittance"]
        assert not np.isnan(t).any() and o["fresnel"]["n_invalid"] == 0
        if o["ghosts"] is not None:
            assert (o["ghosts"]["n_invalid"], o["ghosts"]["n_dropped"]) == (0, 0)
        later = np.flatnonzero(frame[:, IX["generation"]] > 0)
        before = {(g, i): r for r, (g, i) in enumerate(zip(frame[:, IX["generation"]], frame[:, IX["id"]]))}
        p = np.array([before[(frame[j, IX["generation"]] - 1, frame[j, IX["id"]])] for j in later])
        assert np.all(t[later] >= t[p] / 2)  # (every T[p] - T[j] is exact)
        total = total + ref.ended_energy(frame, t)
        deepest = max(deepest, ref.interfaces_per_ray(frame))
    last = ref.ghosts(orders[-1]["frame"], orders[-1]["fresnel"]["transmittance"], surfaces,
                      rays_per_group=orders[-1]["ghosts"]["stride"], n_groups=orders[-1]["ghosts"]["n_groups"])
    assert last["n_invalid"] == 0 and last["rays"].shape[1] > 0
    total = total + ref.energy(last["rays"][9])
    residual = abs(total - launched)
    print(f"launched {launched}, residual {float(residual):.3e}, bound {deepest * 2.0 ** -53 * float(launched):.3e}")
    assert len(orders) == 4 and deepest >= 2 and residual <= deepest * np.longdouble(2.0) ** -53 * launched


def plate_ghost(thickness, theta, n=1.5):
    """(signal rows, ghost rows) on the detector of a plate: two rays each."""
    parts, rays, det = gs.plate(thickness, theta, n, rays=2)
    orders = gs.reference_orders(parts, rays, 2, rays_per_group=2)
    out = []
    for k in (0, 2):
        frame, t = orders[k]["frame"], orders[k]["fresnel"]["transmittance"]
        on = frame[:, IX["surface"]] == det.get_id()
        rows = frame[on].copy()
        rows[:, IX["intensity"]] = rows[:, IX["intensity"]] * t[on]
        out.append(rows)
    assert len(orders[1]["frame"][orders[1]["frame"][:, IX["surface"]] == det.get_id()]) == 0  # (order 1 goes back)
    return out


def test_a_plate_at_normal_incidence_has_the_textbook_ghost():
    signal, ghost = plate_ghost(0.5, 0.0)
    r = ((1.5 - 1.0) / (1.5 + 1.0)) ** 2
    assert len(signal) == 2 and len(ghost) == 2
    # four interfaces on the ghost's way, each within TOL of its T (tests/test_gpu_fresnel.py), the first difference of
    # two of them: (3 + 1 + 1 + 1) TOL on a product of factors below 1, and as many roundings of the products
    assert np.all(np.abs(ghost[:, IX["intensity"]] / 100.0 - (1 - r) ** 2 * r ** 2) <= 8 * TOL)
    assert np.all(np.abs(signal[:, IX["intensity"]] / 100.0 - (1 - r) ** 2) <= 2 * TOL)
    assert np.all(np.abs(ghost[:, IX["y1"]:IX["z1"] + 1] - signal[:, IX["y1"]:IX["z1"] + 1]) <= 4 * TOL)


@pytest.mark.parametrize("theta", [0.1, 0.4, 0.7])  # (at 0.7 both still land on the 8 x 8 detector)
def test_a_tilted_plate_puts_the_ghost_beside_the_signal(theta):
    d, n = 0.5, 1.5
    signal, ghost = plate_ghost(d, theta, n)
    theta_t = np.arcsin(np.sin(theta) / n)
    u = np.array([np.cos(theta), np.sin(theta), 0.0])
    apart = ghost[:, IX["x1"]:IX["z1"] + 1] - signal[:, IX["x1"]:IX["z1"] + 1]
    across = apart - np.outer(apart @ u, u)  # (the two rays are parallel: their distance is measured across them)
    offset = np.linalg.norm(across, axis=1)
    want = 2 * d * np.tan(theta_t) * np.cos(theta)
    print(f"theta {theta}: offset {offset}, closed form {want}, off by {np.abs(offset - want).max():.3e}")
    # positions of size <= 4 (the detector stands at x = 3), each good to the bar on values near 1
    assert np.all(np.abs(offset - want) <= 4 * TOL) and want > 0.05
    assert np.all(np.abs(ghost[:, 12:15] - u) <= TOL)
    ts, tp = fref.power_coefficients(theta, 1.0, n)
    rs, rp = 1 - ts, 1 - tp
    assert np.all(np.abs(ghost[:, IX["intensity"]] / 100.0 - (ts * ts * rs * rs + tp * tp * rp * rp) / 2) < 1e-3)


# ---- refusals, before any GPU call ------------------------------------------------------------------------------------------
def host_frame(frame):
    from pyrayt_amd.frame import DeviceFrame

    counts = np.bincount(frame[:, 0].astype(int)).tolist()
    return DeviceFrame(torch.from_numpy(np.ascontiguousarray(frame.T)), counts)


def host_fresnel(device, coatings=None):
    from pyrayt_amd.frame import Fresnel

    return Fresnel(device, torch.ones(len(device), dtype=torch.float64), None, np.zeros(6, dtype=np.int64), coatings=coatings)


def test_what_the_pass_refuses_before_it_reaches_the_library(monkeypatch):
    from pyrayt_amd import engine, ghosts
    from pyrayt_amd.materials import Coating

    monkeypatch.setattr(engine, "library", lambda: pytest.fail("the library was reached"))
    device = host_frame(fan(20))
    fresnel = host_fresnel(device)
    with pytest.raises(ValueError, match="whole frame"):
        part = device.where(surface=2)
        part.ghosts(host_fresnel(part), [1, 2])
    with pytest.raises(ValueError, match="this very frame"):
        device.ghosts(host_fresnel(host_frame(fan(20))), [1, 2])
    with pytest.raises(ValueError, match="this very frame"):
        device.ghosts(torch.ones(len(device)), [1, 2])
    with pytest.raises(ValueError, match="at most 64 surfaces"):
        device.ghosts(fresnel, range(65))
    with pytest.raises(ValueError, match="at most 65535 buckets"):
        device.ghosts(fresnel, range(64), rays_per_source=1, n_groups=1024)
    with pytest.raises(ValueError, match="system="):
        device.ghosts(fresnel)
    with pytest.raises(ValueError, match="min_intensity"):
        device.ghosts(fresnel, [1], min_intensity=-1.0)
    absorbing = Coating([(1.38 + 0.2j, 0.1)])
    with pytest.raises(ValueError, match="complex index"):
        device.ghosts(host_fresnel(device, coatings={2: absorbing}), [1, 2])
    with pytest.raises(pytest.fail.Exception, match="the library was reached"):  # (a real stack elsewhere passes the checks)
        device.ghosts(host_fresnel(device, coatings={3: absorbing, 2: Coating.quarter_wave(1.38, 0.55)}), [1, 2])
    assert ghosts.MAX_SURFACES == ref.MAX_SURFACES and ghosts.MAX_BUCKETS == ref.MAX_BUCKETS


def test_surfaces_none_takes_the_refracting_surfaces_of_the_system():
    from pyrayt_amd import ghosts
    from pyrayt_amd.scene import SceneSnapshot

    parts, _, det = gs.lens(1)
    glass = ghosts.refracting_surfaces(parts)
    assert glass == ghosts.refracting_surfaces(SceneSnapshot(parts)) and len(glass) == 3
    assert det.get_id() not in glass and parts[-1].get_id() not in glass
    assert ghosts._listed([parts[0], 9, det, 9]) == [sid for sid, _ in parts[0].surface_ids] + [9, det.get_id()]


def test_the_housing_is_an_absorbing_sphere():
    from pyrayt_amd import ghosts, materials
    from pyrayt_amd.scene import SceneSnapshot

    shell = ghosts.housing(30, centre=(1, 2, 3))
    snapshot = SceneSnapshot([shell])
    assert snapshot.materials["kind"][snapshot.prims["material"][0]] == materials.ABSORBER
    assert np.allclose(np.asarray(shell.get_world_transform())[:3, 3], (1, 2, 3)) and snapshot.prims["params"][0][0] == 30.0


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_the_header_and_the_binding_agree():
    import ctypes

    from pyrayt_amd import engine

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prt.h")).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    names = ["prt_frame_ghosts_count", "prt_frame_ghosts_count_workspace_bytes", "prt_frame_ghosts_emit",
             "prt_frame_ghosts_emit_workspace_bytes"]
    for name in names:
        result, arguments = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text).groups()
        wanted = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in arguments.split(",")]
        assert engine.SIGNATURES[name] == (kinds[result], wanted), name
        assert name in engine.EXPORTED_SYMBOLS
    assert engine.PRT_VERSION == 240 and "#define PRT_VERSION 240" in open(os.path.join(ROOT, "include", "prt.h")).read()
    lib = ctypes.CDLL(engine.LIB_PATH)
    assert all(hasattr(lib, name) for name in names)
    sizes = lib.prt_frame_ghosts_count_workspace_bytes
    sizes.restype, sizes.argtypes = engine.SIGNATURES["prt_frame_ghosts_count_workspace_bytes"]
    assert sizes(1000, 100, 128) > 1000 * 12 + 100 * 12 and sizes(1000, 100, 65536) == -1 and sizes(-1, 100, 1) == -1
    assert sizes(1000, 0, 1) == -1


def test_frame_py_only_delegates():
    """The library calls live in pyrayt_amd/ghosts.py: tests/golden/frame_calls.json pins every prt_frame_* name of
    frame.py."""
    text = open(os.path.join(ROOT, "pyrayt_amd", "frame.py")).read()
    assert "prt_frame_ghosts" not in text and "ghosts.spawn(self" in text
    assert "prt_frame_ghosts_count" in open(os.path.join(ROOT, "pyrayt_amd", "ghosts.py")).read()
