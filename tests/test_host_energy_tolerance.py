"""The reference of the energy tolerancing pass (tests/energy_tolerance_reference.py) against closed forms; what
``energy_tolerance`` and the entry point refuse without a GPU; the Python call recorded by a stand-in library; what
``EnergyToleranceRun`` reads; the code objects of k_etol_curve and k_etol_select; and, on the CPU, the end-to-end lemma the
GPU test of the same name repeats on the device."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import diffraction_reference as R
import energy_reference as E
import energy_tolerance_reference as ET
import mtf_tolerance_reference as T

LD = np.longdouble
ROOT = R.ROOT


# ---- closed forms -----------------------------------------------------------------------------------------------------------
def disk_case(n=4000, a=0.5):
    """A vogel_disk of radius a across the axis at x = 0, rays along the axis, weights 1, and two parameters: column 0
    with dQ = Q (a magnification about the origin: dp = p), column 1 with dQ = (0, 0.7, -0.4) (a rigid shift)."""
    points, _ = E.vogel_disk(n, a)
    frame = np.zeros((n, 15))
    frame[:, 1], frame[:, 2], frame[:, 3], frame[:, 5] = 1.0, 0.55, 1.0, R.SURFACE
    frame[:, 4], frame[:, 10:12], frame[:, 12] = np.arange(n), points, 1.0
    jacobian = np.zeros((2, 3, n))
    jacobian[0, 1:] = points.T
    jacobian[1, 1:] = np.array([[0.7], [-0.4]])
    return SimpleNamespace(frame=frame, rows=np.arange(n), group=np.zeros(n, dtype=np.int64), jacobian=jacobian,
                           slopes=np.zeros_like(jacobian), rays_per_source=None, n_groups=1, n_parameters=2), a


def counts_and_radii(grp, radii, fractions):
    """The reference's own answer where no ray lies in a band: (count (M, F, R), radius (M, F, N))."""
    lower, upper = ET.count_bounds(grp, radii)
    assert np.array_equal(lower, upper), ET.undecided(grp, radii)
    return lower, ET.radius_in_float64(grp, fractions)


def test_a_magnification_scales_the_disk():
    """dp = p: the disk of radius a becomes one of a (1 + t); EE(r) = (r / (a (1 + t)))^2 within a ray's weight 1 / n,
    radius(phi) = a (1 + t) sqrt(phi) to within one ray's spacing."""
    case, a = disk_case()
    n = len(case.rows)
    t = np.array([[0.0, 0.0], [0.25, 0.0], [-0.5, 0.0]])
    radii, fractions = np.array([0.1, 0.2, 0.3]), np.array([0.1, 0.5, 0.8, 1.0])
    ref = ET.reference_of(case, t, (0.0,), "circle", False, centre=np.zeros((1, 3)))
    grp = ref.groups[0]
    assert grp.W == int(grp.q[0]) * n and len(set(grp.q.tolist())) == 1
    count, radius = counts_and_radii(grp, radii, fractions)
    for m, scale in enumerate(1 + t[:, 0]):
        energy = count[m, 0].astype(float) / grp.W
        assert np.abs(energy - np.minimum((radii / (a * scale)) ** 2, 1.0)).max() <= 1.0 / n
        k = np.ceil(fractions * n) - 1  # (the ray the count reaches the fraction at)
        spacing = a * scale * (np.sqrt((k + 1) / n) - np.sqrt(k / n))
        assert np.all(np.abs(radius[m, 0] - a * scale * np.sqrt(fractions)) <= spacing)
        assert np.all(ET.radius_conditions(grp, fractions, radius)[0]) and np.all(ET.radius_conditions(grp, fractions, radius)[1])


def test_a_rigid_shift_changes_nothing_about_the_centroid_and_walks_off_the_held_centre():
    case, a = disk_case(1500)
    t = np.array([[0.0, 0.0], [0.0, 0.1], [0.0, -0.25]])
    fractions = np.array([0.5, 0.9])
    about = ET.reference_of(case, t, (0.0,), "circle", True, centre=np.zeros((1, 3)))
    radii = ET.clear_radii(about, 4)
    count, radius = counts_and_radii(about.groups[0], radii, fractions)
    assert np.array_equal(count[1:], count[:1].repeat(2, axis=0)) and np.abs(radius[1:] - radius[:1]).max() <= 1e-15
    held = ET.reference_of(case, t, (0.0,), "square", False, centre=np.zeros((1, 3)))
    radii = ET.clear_radii(held, 5)
    count, radius = counts_and_radii(held.groups[0], radii, fractions)
    points = case.frame[:, 10:12]
    for m in range(3):  # (a direct count of the moved points in the square)
        d = np.abs(points + t[m, 1] * np.array([0.7, -0.4])).max(axis=1)
        assert np.array_equal(count[m, 0], [(d <= r).sum() * int(held.groups[0].q[0]) for r in radii])
        assert np.allclose(radius[m, 0], np.sort(d)[np.ceil(fractions * len(d)).astype(int) - 1], rtol=0, atol=1e-15)
    assert np.all(count[2, 0] <= count[0, 0]) and count[2, 0].sum() < count[0, 0].sum()  # (the spot walks off the pixel)


def test_a_focus_column_is_a_plane_shift_and_the_compensator_takes_it_back():
    from test_host_mtf_tolerance import focus_case

    case = focus_case()
    centre = np.array([[1e-4, -2e-4, 3e-4]] * 2)
    shifts = np.array([0.02, -0.035, 0.0])
    trials = np.zeros((3, 2))
    trials[:, 0] = shifts
    for shape in ET.SHAPES:
        ref = ET.reference_of(case, trials, (0.0,), shape, True, centre=centre)
        planes = ET.reference_of(case, np.zeros((1, 2)), shifts, shape, True, centre=centre)
        fit = ET.reference_of(case, trials, (0.0, 0.05), shape, True, centre=centre, compensate=True)
        for g in range(2):  # trial t at plane 0 is the zero trial at plane t; compensated, every trial is the nominal one
            assert np.abs((ref.groups[g].d[:, 0] - planes.groups[g].d[0]).astype(float)).max() <= 1e-15
            assert np.abs((fit.groups[g].d - fit.groups[g].d[2:3]).astype(float)).max() <= 1e-14
            assert np.abs(fit.groups[g].shift - (fit.groups[g].shift[2] - shifts)).max() <= 1e-13


def test_the_band_is_of_the_order_the_number_formats_give_and_the_weights_follow_the_selected_rows():
    case = ET.tolerance_case([90, 60], 3, left_out=3, unfollowed=2, seed=9)
    ref = ET.reference_of(case, ET.random_trials(3, 3), (0.0, 0.05))
    assert ref.n_rays.tolist() == [88, 58] and ET.k_x(3) == 31
    for g, grp in enumerate(ref.groups):
        assert 0 < grp.eps.max() <= 1e-15 and grp.eps.max() <= 1e-11 * np.median(grp.d.astype(float))
        n_selected = int((case.group == g).sum())
        top = 2 ** (62 - n_selected.bit_length())  # (B from the selected rows, 93 and 63 here, not from the 88 and 58 kept)
        assert grp.W < 2 ** 62 and top // 2 <= grp.q.max() < top and n_selected > len(grp.q)
        radii = ET.clear_radii(ref, 6)
        assert ET.undecided(grp, radii) == 0.0
        below, reached = ET.radius_conditions(grp, (0.5, 0.9), ET.radius_in_float64(grp, (0.5, 0.9)))
        assert np.all(below) and np.all(reached)
    centres = ET.plane_centres(np.array([[2.0, 1.0, 3.0, 0.5, -1.0, 0, 0, 0]]), np.array([[0.0, 2.0]]), True)
    assert centres.tolist() == [[[0.5, 1.5], [1.0, 0.5]]] and not ET.plane_centres(np.ones((1, 8)), np.ones((1, 2)), False).any()


def test_the_lattice_case_is_exact_in_float64():
    case, trials, focus = ET.lattice_case(300)
    for shape in ET.SHAPES:
        grp = ET.reference_of(case, trials, focus, shape, False, centre=np.zeros((1, 3))).groups[0]
        if shape != "circle":
            assert np.all(grp.d.astype(np.float64).astype(LD) == grp.d)
        p = case.frame[:, 10:12] + np.einsum("k,kcn->nc", trials[1], case.jacobian[:, 1:])
        s = case.frame[:, 13:15] + np.einsum("k,kcn->nc", trials[1], case.slopes[:, 1:])
        assert np.array_equal(E.distances(p, s, focus[1], np.zeros(2), shape), grp.d[1, 1].astype(np.float64))


# ---- the interface ------------------------------------------------------------------------------------------------------------
def test_energy_tolerance_needs_slopes_and_refuses_what_it_cannot_serve():
    from pyrayt_amd.frame import Sensitivity, Tolerances

    bare = Sensitivity(None, None, np.zeros((1, 11)), np.zeros((1, 3)), True, (0, 0, 0, 0), ["p"])
    with pytest.raises(ValueError, match=r"energy_tolerance: .*slopes=True"):
        bare.energy_tolerance(np.zeros((1, 1)), [0.1])
    plain = Sensitivity(None, None, np.zeros((1, 17)), np.zeros((1, 3)), True, (0, 0, 0, 0), ["a", "b"])
    plain.slopes = SimpleNamespace()
    for compensators in (("tilt",), ("focus", "focus"), (0,), "tilt", 3):
        with pytest.raises(ValueError, match="compensators"):
            plain.energy_tolerance(np.zeros((1, 2)), [0.1], compensators=compensators)
    for trials in (np.zeros((3, 1)), np.zeros(2), np.zeros((0, 2)), np.full((1, 2), np.nan), np.zeros((65536, 2)),
                   (Tolerances([1.0]), 5)):
        with pytest.raises(ValueError, match="trials"):
            plain.energy_tolerance(trials, [0.1])
    for radii in ([-1.0], [0.2, 0.1], [0.1, 0.1], np.zeros(257), [np.inf]):
        with pytest.raises(ValueError, match="radii"):
            plain.energy_tolerance(np.zeros((1, 2)), radii)
    with pytest.raises(ValueError, match="radii: give radii, fractions or both"):
        plain.energy_tolerance(np.zeros((1, 2)), None, fractions=None)
    for fractions in ([0.0], [1.5], np.full(17, 0.5)):
        with pytest.raises(ValueError, match="fractions"):
            plain.energy_tolerance(np.zeros((1, 2)), fractions=fractions)
    with pytest.raises(ValueError, match="shape"):
        plain.energy_tolerance(np.zeros((1, 2)), [0.1], shape="hexagon")
    with pytest.raises(ValueError, match="focus"):
        plain.energy_tolerance(np.zeros((1, 2)), [0.1], focus=[np.nan])


def test_the_pass_calls_the_library_as_the_header_declares_it(monkeypatch):
    """tests/test_host_frame_calls.py's stand-in library under ``energy_tolerance``: one size call, then the entry with 31
    arguments, the workspace and the stream; radii or fractions that are not asked for are NULL with their outputs.  The
    call lives in pyrayt_amd/energy_tolerance.py: frame.py's code does not name the entry point."""
    torch = pytest.importorskip("torch")
    import pyrayt_amd.frame as F
    from pyrayt_amd.scene import MATERIAL_DTYPE, PRIM_DTYPE
    from test_host_frame_calls import frame_entry_points, make_frame, stand_ins

    assert torch is not None and not [name for name in frame_entry_points() if "energy_tolerance" in name]
    run = stand_ins(monkeypatch)
    system = SimpleNamespace(prims=np.zeros(2, dtype=PRIM_DTYPE), materials=np.zeros(1, dtype=MATERIAL_DTYPE))
    system.prims["surface_id"] = (1, 2)
    rigid = [F.Motion(1, translate=(1, 0, 0)), F.Motion(2, rotate=(0, 0, 1))]
    trials = np.array([[0.1, 0.0], [0.0, 0.1], [0.1, 0.1]])
    frame = make_frame()
    for surface, kw, radii, more in (
            (2, dict(rays_per_source=4), (0.1, 0.2), dict(compensators=("focus",), centre=(0.0, 0.1, 0.0), shape="square")),
            (2, {}, None, dict(follow_centroid=False)), (7, {}, (0.1,), dict(fractions=None))):
        got = run(lambda: frame.sensitivity(surface, rigid, system, slopes=True, **kw).energy_tolerance(
            trials, radii, focus=(0.0, 0.1), **more))
        assert got["raised"] is None, got
        (size_name, size_args), (name, args) = got["calls"][-2:]
        assert size_name == "prt_frame_energy_tolerance_workspace_bytes" and name == "prt_frame_energy_tolerance"
        n_groups, n_radii = 2 if kw else 1, len(radii or ())
        n_fractions = 0 if "fractions" in more else 3
        assert list(size_args[1:]) == [n_groups, 2, n_radii, n_fractions, 2, 4] and len(args) == 33
        assert args[11] == 2 and args[12] == ("ptr" if "centre" in more else "NULL")
        assert list(args[14:16]) == [1 if "shape" in more else 0, 0 if "follow_centroid" in more else 1]
        assert list(args[16:22]) == ["ptr" if n_radii else "NULL", n_radii, "ptr" if n_fractions else "NULL", n_fractions,
                                     "ptr", 2]
        assert list(args[22:25]) == ["ptr", 4, int("compensators" in more)]
        assert list(args[25:28]) == ["ptr" if n_radii else "NULL"] * 2 + ["ptr" if n_fractions else "NULL"]
        assert list(args[28:]) == ["ptr"] * 4 + ["NULL"]


def run_of(radius_like, trials):
    """An EnergyToleranceRun whose radius of fraction k in plane f is radius_like[g, m] * (1 + k) * (1 + f) and whose energy
    at radius j is min(1, 0.2 (1 + j) / radius_like)."""
    from pyrayt_amd.frame import EnergyToleranceRun

    G_, M = radius_like.shape
    radius = radius_like[:, :, None, None] * np.array([1.0, 2.0])[None, None, :, None] * np.array([1.0, 2.0, 3.0])
    with np.errstate(invalid="ignore"):
        energy = np.minimum(1.0, 0.2 * np.array([1.0, 2.0])[None, None, None, :] / radius[..., :1])
    count = np.nan_to_num(energy * 1000).astype(np.uint64)
    moments = np.zeros((G_, M, 8))
    moments[..., 0], moments[..., 5], moments[..., 7] = 2.0, 8.0, 2.0
    moments[1] = np.nan
    record = np.array([[0, 0, 0, 2.0, 2, 0, 0, 0], [np.nan, np.nan, np.nan, 0, 0, 1, 1, 0]])
    record[:, 7] = np.array([1000, 0], dtype=np.uint64).view(np.float64)
    return EnergyToleranceRun(trials, count, energy, radius, moments, np.zeros((G_, M)), record, (0.2, 0.4), (0.5, 0.8, 0.9),
                              (0.0, 1.0), ("a", "b"))


def test_energy_tolerance_run_reads_its_arrays():
    from pyrayt_amd.frame import Tolerances

    tol = Tolerances([0.1, 0.2])
    trials = np.vstack([tol.sensitivity_table(), np.zeros((1, 2))])  # (the nominal trial last, as energy_tolerance() adds it)
    merit = np.vstack([np.array([0.2, 0.5, 0.25, 0.22, 0.4, 0.2]), np.full(len(trials), np.nan)])
    run = run_of(merit, trials)
    assert run.trials.shape == (5, 2) and run.radius.shape == (2, 5, 2, 3) and run.energy.shape == (2, 5, 2, 2)
    assert run.count.dtype == np.uint64 and run.total.tolist() == [1000, 0] and run.record.shape == (2, 7)
    assert run.nominal.radius[0, 0, 0] == pytest.approx(0.2) and run.n_rays.tolist() == [2, 0] and run.n_trials == 5
    assert run.yield_(0.8)[0] == 3 / 5 and np.isnan(run.yield_(0.8)[1])  # (energy at radius 0: 1, 0.4, 0.8, 0.91, 0.5)
    assert run.yield_(0.8, radius=1)[0] == 1.0 and run.yield_(0.5, plane=1)[0] == 1 / 5
    assert run.yield_radius(0.7, fraction=0)[0] == 1.0 and run.yield_radius(0.7)[0] == 2 / 5 and np.isnan(run.yield_radius(1)[1])
    assert run.percentiles((0, 100), fraction=0)[0].tolist() == pytest.approx([0.2, 0.5])
    assert run.rms_radius[0, 0].tolist() == pytest.approx([2.0, np.sqrt(5.0)]) and run.centroid.shape == (2, 5, 2)
    frame = run.to_pandas()
    assert list(frame.columns) == ["source_id", "trial", "focus_shift", "best_focus", "rms_radius_0", "rms_radius_1",
                                   "energy_0_0", "energy_0_1", "radius_0_0", "radius_0_1", "radius_0_2", "energy_1_0",
                                   "energy_1_1", "radius_1_0", "radius_1_1", "radius_1_2", "p_0", "p_1"] and len(frame) == 10
    table = run.table(fraction=0)
    assert table["parameter"].tolist() == [0, 1] and table["worst"].tolist() == pytest.approx([0.3, 0.2])
    assert table["dradius_plus"].tolist() == pytest.approx([0.05, 0.2]) and table["width"].tolist() == [0.1, 0.2]
    with pytest.raises(ValueError, match="sensitivity_table"):
        run_of(merit[:, :4], np.ones((4, 2))).table()


def test_abi_entries_are_declared_and_the_version_stays():
    import pyrayt_amd
    from pyrayt_amd import engine

    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("prt_frame_energy_tolerance_workspace_bytes", "prt_frame_energy_tolerance"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    found = re.search(r"#define PRT_VERSION (\d+) /\*(.*?)\*/", header, flags=re.S)
    assert int(found.group(1)) == 240 and "prt_frame_energy_tolerance" in found.group(2)
    assert pyrayt_amd.EnergyToleranceRun is pyrayt_amd.frame.EnergyToleranceRun and "EnergyToleranceRun" in pyrayt_amd.__all__
    assert hasattr(pyrayt_amd.RayTracer, "trace_energy_tolerance") and hasattr(pyrayt_amd.Sensitivity, "energy_tolerance")
    for line in ("c = m_P / m_0 + delta * (m_S / m_0)", "energy[j] = (double) count[j] / (double) W",
                 "T_k = clamp((uint64) ceil(phi_k * (double) W), 1, W)"):
        assert line in header, line


def test_library_checks_energy_tolerance_arguments_without_a_gpu():
    from pyrayt_amd import engine
    from test_host_selection import FAULTS

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    assert lib.prt_frame_energy_tolerance_workspace_bytes(1000, 2, 16, 256, 16, 1, 1000) >= 1000 * (48 + 16 * 32 + 8)
    for args in ((1000, 2, 0, 8, 3, 1, 10), (1000, 2, 17, 8, 3, 1, 10), (1000, 2, 4, 257, 3, 1, 10),
                 (1000, 2, 4, 8, 17, 1, 10), (1000, 2, 4, 0, 0, 1, 10), (1000, 2, 4, 8, 3, 257, 10), (1000, 2, 4, 8, 3, 0, 10),
                 (1000, 0, 4, 8, 3, 1, 10), (-1, 1, 4, 8, 3, 1, 10), (1000, 65536, 4, 8, 3, 1, 10), (1000, 2, 4, 8, 3, 1, 0),
                 (1000, 2, 4, 8, 3, 1, 65537), (1000, 2, 4, -1, 3, 1, 10)):
        assert lib.prt_frame_energy_tolerance_workspace_bytes(*args) == -1, args
    buf = np.zeros(64)
    p = buf.ctypes.data
    unit = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
    edges, phi, planes = np.array([0.1, 0.2]), np.array([0.5, 0.9]), np.array([0.0])
    sound = np.array([0, 4], dtype=np.int64)

    def call(radii=edges, n_r=2, fractions=phi, n_f=2, focus=planes, n_p=1, weight=1, n_groups=1, axes=unit, K=2,
             first=sound, n_selected=4, n_rows=4, jacobian=p, count=p, radius=p, trials=p, M=3, moments=p, shape=0):
        pointer = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return lib.prt_frame_energy_tolerance(0, p, 4, n_rows, p, n_selected, first.ctypes.data, n_groups, weight, jacobian,
                                              p, K, None, axes.ctypes.data, shape, 1, pointer(radii), n_r,
                                              pointer(fractions), n_f, pointer(focus), n_p, trials, M, 0, count, p, radius,
                                              moments, p, p, p, None)

    for kwargs, message in ((dict(radii=np.array([-1.0, 1.0])), "radii finite, >= 0 and strictly ascending"),
                            (dict(radii=np.array([0.2, 0.2])), "radii finite, >= 0 and strictly ascending"),
                            (dict(n_r=257, radii=np.arange(257.0)), "0 to 256 radii"),
                            (dict(count=None), "0 to 256 radii, with count_out and energy_out"),
                            (dict(fractions=np.array([0.0, 0.5])), "fractions in (0, 1]"),
                            (dict(n_f=17, fractions=np.full(17, 0.5)), "0 to 16 fractions"),
                            (dict(radius=None), "0 to 16 fractions, with radius_out"),
                            (dict(n_r=0, n_f=0), "radii or fractions, not neither"),
                            (dict(focus=np.array([np.nan])), "focus shifts finite"),
                            (dict(n_p=257, focus=np.zeros(257)), "1 to 256 focus shifts"),
                            (dict(shape=4), "shape is PRT_ENERGY_CIRCLE"),
                            (dict(axes=np.full(9, np.nan)), "axes: finite"),
                            (dict(K=0), "1 to 16 parameters"),
                            (dict(K=17), "1 to 16 parameters"),
                            (dict(M=0), "1 to 65536 trials"),
                            (dict(M=65537), "1 to 65536 trials"),
                            (dict(trials=None), "bad buffers"),
                            (dict(moments=None), "bad buffers"),
                            (dict(jacobian=None), "jacobian and slopes"),
                            # 4682 groups, a slice each at the least: 4682 * 256 trials * 224 bytes
                            (dict(n_groups=4682, first=np.concatenate([np.zeros(4682), [4]]).astype(np.int64)),
                             "256 MiB slab cap")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())
        assert lib.prt_last_error().decode().startswith(("energy_tolerance", "axes")), lib.prt_last_error()
    for fault, message in FAULTS:  # (selection_check's faults in this pass's name)
        given = dict(n_selected=4, first=(0, 4), n_groups=1, weight=1)
        given.update(fault)
        assert call(n_selected=given["n_selected"], first=np.array(given["first"], dtype=np.int64),
                    n_groups=given["n_groups"], weight=given["weight"]) == -1, fault
        assert lib.prt_last_error().decode() == message.format(name="energy_tolerance"), (fault, lib.prt_last_error())


def test_the_kernels_use_no_scratch_and_have_the_resources_design_md_states():
    """Every k_etol_curve and k_etol_select instantiation keeps its trial's coefficients and counters in registers: no
    private segment, no spills; its VGPR count and LDS bytes are the ones of DESIGN.md's table, and the waves per SIMD
    stated there follow from the VGPR count (granule 8, 512 a SIMD lane, 8 waves at most)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pyrayt_amd import engine

    if not os.path.exists(mod.READELF):
        pytest.skip("llvm-readelf not available")
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for kernel, extra in (("k_etol_curve", 64 * 8 + 8 * 8), ("k_etol_select", 64 * 8)):
        kernels = {name: res for name, res in mod.kernel_resources(engine.LIB_PATH).items() if kernel in name}
        assert len(kernels) == 4, sorted(kernels)
        stated = {int(cp): (int(v), int(lds), int(waves)) for cp, v, lds, waves in
                  re.findall(rf"\| `{kernel}<(\d+)>` \| (\d+) \| (\d+) \| (\d+) \|", design)}
        assert sorted(stated) == [4, 8, 12, 16], (kernel, stated)
        for name, res in kernels.items():
            cp = int(re.search(rf"{kernel}ILi(\d+)E", name).group(1))
            assert res["private_segment_fixed_size"] == 0, (name, res)
            assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0, (name, res)
            assert res["group_segment_fixed_size"] == T.K.kMtftRays * (48 + cp * 32) + extra == stated[cp][1], (name, res)
            assert res["vgpr_count"] == stated[cp][0], (name, res, stated[cp])
            assert min(8, 512 // (-(-res["vgpr_count"] // 8) * 8)) == stated[cp][2], (name, res, stated[cp])


# ---- end to end on the CPU: the reference and the linear ray model against the oracle's re-traces -------------------------------
E2E_FRACTIONS, E2E_PLANES, E2E_TOP = (0.5, 0.8, 0.9), (0.0, 0.5), 1.2
E2E_SCENES = ("singlet", "two_fields")


def e2e_radii(rays):
    """Two radii from the nominal spot alone: the median and the 90th percentile of the staged |p| over all groups."""
    d = np.concatenate([np.hypot(ray.p[0].astype(float), ray.p[1].astype(float)) for ray in rays])
    return np.percentile(d, (50, 90))


@pytest.mark.parametrize("name", E2E_SCENES)
def test_reference_end_to_end_the_error_of_the_linear_ray_model_is_of_second_order(name):
    """The lemma the GPU test of the same name asserts on the device, here with the reference alone: 4 trials with every
    applicable parameter moved at once (the MTF tolerancing's ``e2e_trials`` and its h, at its top frequency 1.2), no
    compensator, planes 0 and 0.5, distances about the held nominal centroid.  eps(h) = max_r |d_lin,r - d_retraced,r|
    over the rays, planes and trials, d_retraced from the C oracle's re-trace of the perturbed system (no trial loses or
    gains a ray).  An order statistic moves by no more than its largest element, so |radius_lin - radius_retraced| <=
    eps(h) and EE_retraced(R - eps) <= EE_lin(R) <= EE_retraced(R + eps) hold exactly; and eps(h / 2) <= eps(h) / 3:
    the model's error is of second order.  dish_axial is left out as the MTF tolerancing's test leaves it out: its image
    is stigmatic and the h the rule asks for there loses rays."""
    import tolerance_scenes
    from test_host_mtf_tolerance import e2e_setup, e2e_trials

    case, rows, group, n_groups, jacobian, slopes = e2e_setup(name)
    f = case.frame
    q, u, w = f[rows, 9:12], f[rows, 12:15], f[rows, 1]
    n_par, live = len(case.parameters), tolerance_scenes.applicable(case.parameters)
    rays, rec = T.staged(q, u, w, group, n_groups, jacobian, slopes)
    dp = np.concatenate([ray.dp.astype(float) for ray in rays], axis=2)
    direction, h = e2e_trials(dp, group, n_groups, live, n_par, E2E_TOP)
    centre = rec.centre.astype(np.float64)
    radii = e2e_radii(rays)
    per = getattr(case, "rays_per_source", None)

    def error(scale):
        trials = direction * (h * scale)
        ref = ET.energy_tolerance_reference(q, u, w, group, n_groups, jacobian, slopes, trials, E2E_PLANES, "circle", False,
                                            centre=centre)
        worst = 0.0
        for m in range(4):
            moved = tolerance_scenes.build(name, 257, trials[m])
            assert moved.counts == case.counts and np.array_equal(moved.frame[:, 4], case.frame[:, 4]), "rays lost or gained"
            staged = E.stage(moved.frame[rows], None, rays_per_source=per, n_groups=n_groups, reference=centre)
            for g, (p, s, weights, _, used, _) in enumerate(staged):
                grp = ref.groups[g]
                assert used == rec.n_rays[g] and np.array_equal(weights, w[group == g])
                for k, delta in enumerate(E2E_PLANES):
                    d = E.distances(p, s, delta, np.zeros(2), "circle")
                    lin = grp.d[m, k].astype(np.float64)
                    eps = float(np.abs(lin - d).max())
                    worst = max(worst, eps)
                    order = np.argsort(d, kind="stable")
                    run = np.cumsum(grp.q[order], dtype=np.uint64)
                    need = ET.needs(grp.W, E2E_FRACTIONS)
                    retraced = d[order][np.searchsorted(run, need, side="left")]
                    one = SimpleNamespace(d=grp.d[m:m + 1, k:k + 1], eps=grp.eps[m:m + 1, k:k + 1], q=grp.q, W=grp.W)
                    mine = ET.radius_in_float64(one, E2E_FRACTIONS)[0, 0]
                    assert np.all(np.abs(mine - retraced) <= eps), (name, m, g, k)
                    count = lambda dist, edge: np.array([grp.q[dist <= r].sum(dtype=np.uint64) for r in edge])  # noqa: E731
                    assert np.all(count(d, radii - eps) <= count(lin, radii)), (name, m, g, k)
                    assert np.all(count(lin, radii) <= count(d, radii + eps)), (name, m, g, k)
        return worst

    e1, e2 = error(1.0), error(0.5)
    print(f"[energy tolerance] {name} on the CPU: h {h:.4f}, eps(h) {e1:.3e}, eps(h/2) {e2:.3e} (ratio {e2 / e1:.3f})")
    assert e2 <= e1 / 3, (name, e1, e2)
