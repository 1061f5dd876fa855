"""The host side of the Fresnel pass (CPU): the numpy restatement of the definitions (tests/fresnel_reference.py) against
closed forms and on the golden frames, argument checks that come before any GPU call, the ABI entries, the library's own
refusals, and the kernel's resources."""
import os
import re

import numpy as np
import pytest

import fresnel_reference as ref
import helpers
from pyrayt_amd.frame import DeviceFrame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = np.array([1.0, 0.0, 0.0])
TOL = 32 * np.finfo(np.float64).eps  # about 30 roundings an interface, each of half an ulp at most, on values near 1
# the fixtures tests/test_gpu_fresnel.py holds the device to, and whether light is refracted in them
BUILT_IN = {"config2": True, "adv_prism": True, "two_mirrors": False, "tutorial": True}


def tilted(theta):
    return np.array([np.cos(theta), np.sin(theta), 0.0])


def plate(theta, n=1.5, surfaces=(1, 2, 3)):
    """One ray through a plane-parallel plate whose faces are normal to x, at theta to the normal."""
    u = tilted(theta)
    inside = ref.snell(u, X, 1.0, n)
    return ref.synthetic([[(u, 1.0, surfaces[0]), (inside, n, surfaces[1]), (u, 1.0, surfaces[2])]])


@pytest.mark.parametrize("ni, nt", [(1.0, 1.5), (1.5, 1.0), (1.0, 2.4), (1.33, 1.52)])
def test_normal_incidence(ni, nt):
    frame = ref.synthetic([[(X, ni, 1), (X, nt, 2)]])
    for polarization in (None, (0.0, 1.0, 0.0), (0.0, 1.0, 1.0)):
        got = ref.fresnel(frame, polarization=polarization)
        assert got["transmittance"][0] == 1.0
        assert abs(got["transmittance"][1] - 4 * ni * nt / (ni + nt) ** 2) <= TOL
        assert got["n_invalid"] == 0 and got["n_reflections"] == 0 and got["n_undeviated"] == 0


def test_a_p_polarised_ray_passes_at_brewsters_angle():
    n = 1.5
    u = tilted(np.arctan(n))
    frame = ref.synthetic([[(u, 1.0, 1), (ref.snell(u, X, 1.0, n), n, 2)]])
    p = ref.fresnel(frame, polarization=(0.0, 1.0, 0.0))  # (in the plane of incidence xy)
    assert abs(p["transmittance"][1] - 1.0) <= TOL
    s = ref.fresnel(frame, polarization=(0.0, 0.0, 1.0))
    ts, tp = ref.power_coefficients(np.arctan(n), 1.0, n)
    assert abs(tp - 1.0) <= TOL and abs(s["transmittance"][1] - ts) <= TOL and ts < 0.86


def test_forty_five_degrees_into_glass():
    frame = plate(np.pi / 4)[:2]
    s = ref.fresnel(frame, polarization=(0.0, 0.0, 1.0))["transmittance"][1]
    p = ref.fresnel(frame, polarization=(0.0, 1.0, 0.0))["transmittance"][1]
    ts, tp = ref.power_coefficients(np.pi / 4, 1.0, 1.5)
    assert abs(s - ts) <= TOL and abs(p - tp) <= TOL
    assert abs(s - 0.907987) < 1e-6 and abs(p - 0.991534) < 1e-6  # (R_s = 9.2013 %, R_p = R_s^2 at 45 degrees)
    both = ref.fresnel(frame)["transmittance"][1]
    assert abs(both - (ts + tp) / 2) <= TOL


def test_polarisation_is_carried_through_a_tilted_plate():
    ts, tp = ref.power_coefficients(np.pi / 4, 1.0, 1.5)
    got = ref.fresnel(plate(np.pi / 4))
    assert abs(got["transmittance"][2] - (ts * ts + tp * tp) / 2) <= 2 * TOL
    assert abs(got["transmittance"][2] - ((ts + tp) / 2) ** 2) > 1e-3  # (what a scalar transmittance would give)
    field = got["field"]
    for row, u in enumerate(plate(np.pi / 4)[:, 12:15]):
        for e in (field[:3, row], field[3:, row]):
            assert abs(e @ u) <= 1e-14 * np.linalg.norm(e)


def test_mirrors_coatings_and_rays_that_pass():
    u = tilted(0.3)
    normal = tilted(1.1)
    frame = ref.synthetic([[(u, 1.0, 1), (ref.mirror(u, normal), 1.0, 2), (ref.mirror(u, normal), 1.0, 3)]])
    got = ref.fresnel(frame)
    assert got["transmittance"].tolist() == [1.0, 1.0, 1.0]
    assert (got["n_reflections"], got["n_undeviated"], got["n_invalid"]) == (1, 1, 0)
    assert np.array_equal(got["field"][:, 1], got["field"][:, 2]) and not np.array_equal(got["field"][:, 0], got["field"][:, 1])
    assert np.allclose(np.linalg.norm(got["field"].reshape(2, 3, 3), axis=1), 1.0, rtol=0, atol=TOL)
    coated = ref.fresnel(plate(0.6), lossless=(1, 2))
    assert coated["transmittance"].tolist() == [1.0, 1.0, 1.0] and coated["n_lossless"] == 2
    assert not np.array_equal(coated["field"][:, 0], coated["field"][:, 1])  # (the field is still rotated)
    half = ref.fresnel(plate(0.6), lossless=(2,))
    ts, tp = ref.power_coefficients(0.6, 1.0, 1.5)
    assert abs(half["transmittance"][2] - (ts + tp) / 2) <= TOL and half["n_lossless"] == 1


def test_interfaces_the_rows_cannot_describe():
    u = tilted(0.4)
    wrong_side = ref.synthetic([[(u, 1.0, 1), (-ref.snell(u, X, 1.0, 1.5), 1.5, 2), (u, 1.0, 3)],
                                [(u, 1.0, 1), (np.zeros(3), 1.5, 2)],
                                [(u, 1.0, 1), (u, np.nan, 2)],
                                [(X, 1.0, 1), (X, 1.5, 2)]])
    got = ref.fresnel(wrong_side)
    t = got["transmittance"]
    assert got["n_invalid"] == 3 and np.isnan(t[[4, 5, 6, 8]]).all() and abs(t[7] - 0.96) <= TOL and t[:4].tolist() == [1.0] * 4
    assert np.isnan(got["field"][:, [4, 5, 6, 8]]).all() and np.isfinite(got["field"][:, 7]).all()
    along = ref.fresnel(ref.synthetic([[(X, 1.0, 1), (X, 1.5, 2)]]), polarization=X)
    assert along["n_invalid"] == 1 and np.isnan(along["transmittance"]).all()
    for bad, message in ((0, "repeats"), (2, "none in the one before")):
        frame = plate(0.2)
        frame = np.concatenate([frame, frame[bad:bad + 1]]) if bad == 0 else np.delete(frame, 1, axis=0)
        with pytest.raises(ValueError, match=message):
            ref.fresnel(frame[np.argsort(frame[:, 0], kind="stable")])


@pytest.mark.parametrize("name", sorted(BUILT_IN))
def test_the_golden_frames_can_show_a_failure(name):
    """What keeps the comparison on the device from passing on nothing: no invalid ray, every T in (0, 1], T never
    rising along a ray, and T < 1 somewhere where light is refracted."""
    frame = helpers.load(f"scene_{name}.npz")["frame"]
    got = ref.fresnel(frame)
    t = got["transmittance"]
    assert got["n_invalid"] == 0 and np.all((t > 0.0) & (t <= 1.0))
    last = {}
    for row in np.argsort(frame[:, 0], kind="stable"):
        ray = frame[row, ref.IX["id"]]
        assert t[row] <= last.get(ray, 1.0), (name, row)
        last[ray] = t[row]
    assert bool(np.any(t < 1.0)) == BUILT_IN[name]
    if not BUILT_IN[name]:
        assert got["n_reflections"] > 0


# ---- the binding and the library -----------------------------------------------------------------------------------------
def host_frame():
    return DeviceFrame(np.ascontiguousarray(plate(0.3).T), [1, 1, 1])


def test_fresnel_arguments_are_checked_before_the_gpu():
    frame = host_frame()
    with pytest.raises(ValueError, match="at most 64 lossless"):
        frame.fresnel(lossless=range(65))
    for bad in ((0, 0, 0), (1, 2), (np.nan, 0, 1), "xyz"):
        with pytest.raises(ValueError, match="polarization"):
            frame.fresnel(polarization=bad)
    with pytest.raises(ValueError, match="where"):
        frame.where(surface=1).fresnel()
    with pytest.raises(ValueError, match="select"):
        frame.select(np.array([True, True, False])).fresnel()
    with pytest.raises(ValueError, match="generation"):
        frame.generation(0).fresnel()
    cut = DeviceFrame(np.zeros((15, 3)), [1, 1, 1])
    cut.origin = "record_only"
    with pytest.raises(ValueError, match="record_only"):
        cut.fresnel()
    with pytest.raises(ValueError, match="rows_per_generation"):
        DeviceFrame(np.zeros((15, 3))).fresnel()
    with pytest.raises(ValueError, match="without the column"):
        DeviceFrame(np.zeros((15, 2)), [2], columns=(0, 1, 4, 5, 12, 13, 14)).fresnel()


def test_abi_entries_are_declared_and_bound():
    from pyrayt_amd import engine

    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("prt_frame_fresnel_workspace_bytes", "prt_frame_fresnel"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    assert "prt_frame_fresnel" in re.search(r"#define PRT_VERSION \d+ /\*(.*?)\*/", header, flags=re.S).group(1)
    assert "eps_dir = 1e-12" in header and ref.EPS_DIR == 1e-12
    if os.path.exists(engine.LIB_PATH):
        lib = engine.library()
        assert len(lib.prt_frame_fresnel.argtypes) == 15 and len(lib.prt_frame_fresnel_workspace_bytes.argtypes) == 2


def test_library_checks_fresnel_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    sizes = [lib.prt_frame_fresnel_workspace_bytes(3 * n, n) for n in (1, 2, 1000, 10 ** 6, 2 ** 31)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:])) and sizes[2] >= 1000 * 60
    assert lib.prt_frame_fresnel_workspace_bytes(0, 1) > 0
    for args in ((-1, 1), (3, 0), (3, -1), (3, 2 ** 31 + 1)):
        assert lib.prt_frame_fresnel_workspace_bytes(*args) == -1, args
    buf = np.zeros(64)
    p = buf.ctypes.data
    counts = np.array([2, 2], dtype=np.int64)
    coated = np.arange(65, dtype=np.int64)
    v = np.array([0.0, 1.0, 0.0])

    def call(rows=p, ld=4, counts=counts, n_generations=2, id0=0.0, n_ids=2, polarization=None, lossless=coated.ctypes.data,
             n_lossless=0, t=p, field=None, record=p, work=p):
        return lib.prt_frame_fresnel(0, rows, ld, counts.ctypes.data if counts is not None else None, n_generations, id0,
                                     n_ids, polarization, lossless, n_lossless, t, field, record, work, None)

    for kwargs, message in ((dict(n_lossless=65), "at most 64 lossless"),
                            (dict(n_lossless=-1), "at most 64 lossless"),
                            (dict(n_lossless=2, lossless=None), "at most 64 lossless"),
                            (dict(polarization=np.zeros(3).ctypes.data), "polarization finite and not zero"),
                            (dict(polarization=np.array([np.inf, 0, 0]).ctypes.data), "polarization finite and not zero"),
                            (dict(n_ids=0), "n_ids in [1, 2^31]"),
                            (dict(n_ids=2 ** 31 + 1), "n_ids in [1, 2^31]"),
                            (dict(id0=float("nan")), "id0 finite"),
                            (dict(id0=float("inf")), "id0 finite"),
                            (dict(counts=np.array([2, -1], dtype=np.int64)), "counts >= 0"),
                            (dict(counts=np.array([2 ** 40, 2], dtype=np.int64), ld=2 ** 41), "too many rows in a generation"),
                            (dict(counts=None), "bad buffers"),
                            (dict(n_generations=-1), "bad buffers"),
                            (dict(ld=3), "bad buffers"),
                            (dict(rows=None), "bad buffers"),
                            (dict(t=None), "bad buffers"),
                            (dict(record=None), "bad buffers"),
                            (dict(work=None), "bad buffers")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())
    record = np.full(4, 7, dtype=np.int64)  # (an empty frame is served on the host)
    assert call(counts=np.zeros(2, dtype=np.int64), rows=None, t=None, record=record.ctypes.data, polarization=v.ctypes.data) == 0
    assert record.tolist() == [0, 0, 0, 0]


def test_fresnel_kernel_uses_no_scratch_and_the_registers_design_states():
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pyrayt_amd import engine

    if not os.path.exists(mod.READELF):
        pytest.skip("llvm-readelf not available")
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    kernels = {name: res for name, res in mod.kernel_resources(engine.LIB_PATH).items() if "k_fresnel_" in name}
    assert any("k_fresnel_step" in name for name in kernels), sorted(kernels)
    stated = re.search(r"`k_fresnel_step`[^.]*?(\d+) VGPRs", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert stated, "DESIGN.md states the VGPRs of k_fresnel_step"
    for name, res in kernels.items():
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (name, res)
        assert res["sgpr_spill_count"] == 0 and res["group_segment_fixed_size"] <= 1024, (name, res)
        assert res["vgpr_count"] == int(stated.group(1)), (name, res)


@pytest.mark.parametrize("n_ids", [1, 65, 2 ** 31])
def test_the_workspaces_of_both_entries_keep_their_sizes(n_ids):
    """The two entries share their workspace's carve-up: the words, the coated entry's tables at their caps (thicknesses,
    wavelengths, complex indices per coating, slot and wavelength), per id the planes of Ea and Eb (6 real, 12 complex),
    the previous row and the stamp, and the slack to align by."""
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    for n_rows in (0, n_ids, 3 * n_ids):
        assert lib.prt_frame_fresnel_workspace_bytes(n_rows, n_ids) == 64 + n_ids * 60 + 64
        assert lib.prt_frame_fresnel_coated_workspace_bytes(n_rows, n_ids) == \
            64 + 8 * (16 * 16 + 256 + 2 * 16 * 18 * 256) + n_ids * 108 + 64
