"""The host side of the coated Fresnel pass (CPU): the numpy restatement (tests/coating_reference.py) against closed forms
and against a second formulation, argument and table checks that come before any GPU call, the ABI entries, the Python
argument errors and the kernel's resources."""
import os
import re

import numpy as np
import pytest

import coating_reference as cr
import fresnel_reference as ref
from pyrayt_amd.frame import DeviceFrame
from pyrayt_amd.materials import Coating, glass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 0.633
ANGLES = np.radians([0.0, 30.0, 56.3, 80.0])
KERNEL = "k_coated_fresnel_step"


def coefficients(stack, ni, nt, theta, reflection=False, lam=LAM, formulation=cr.matrix_coefficients):
    return cr.interface_coefficients(stack, ni, nt, np.cos(theta), reflection, lam, formulation)


# ---- the reference against closed forms, each to 1e-12 ------------------------------------------------------------------
@pytest.mark.parametrize("n1, ns", [(1.38, 1.52), (np.sqrt(1.52), 1.52), (2.0, 1.7)])
def test_a_quarter_wave_layer_at_normal_incidence(n1, ns):
    stack = cr.Stack([(n1, LAM / (4 * n1))], substrate=ns)
    cs, cp, _ = coefficients(stack, 1.0, ns, 0.0)
    want = ((ns - n1 * n1) / (ns + n1 * n1)) ** 2
    assert abs(1.0 - abs(cs) ** 2 - want) <= 1e-12 and abs(abs(cp) ** 2 - abs(cs) ** 2) <= 1e-12
    rs, rp, _ = coefficients(stack, 1.0, 1.0, 0.0, reflection=True)
    assert abs(abs(rs) ** 2 - want) <= 1e-12 and abs(abs(rp) ** 2 - want) <= 1e-12
    if n1 * n1 == ns or abs(n1 * n1 - ns) < 1e-15:
        assert abs(abs(cs) ** 2 - 1.0) <= 1e-12
    made = Coating.quarter_wave(n1, LAM, substrate=ns)
    assert made.layers[0][1] == LAM / (4.0 * n1) and made.substrate == ns


def test_a_half_wave_layer_equals_the_bare_surface():
    half = cr.Stack([(2.1, LAM / (2 * 2.1))], substrate=1.5)
    for got, want in zip(coefficients(half, 1.0, 1.5, 0.0)[:2], coefficients(cr.Stack(), 1.0, 1.5, 0.0)[:2]):
        assert abs(got + want) <= 1e-12  # (half a wave: the phase is pi, the transmittance the bare surface's)
        assert abs(abs(got) ** 2 - 0.96) <= 1e-12


@pytest.mark.parametrize("theta", ANGLES)
@pytest.mark.parametrize("ni, nt", [(1.0, 1.5), (1.5, 1.0)])
def test_no_layers_equal_todays_coefficients(theta, ni, nt):
    if ni > nt:
        theta = np.arcsin(np.sin(theta) / ni)  # (the same ray, the other way through)
    ci, ct = np.cos(theta), np.sqrt(1 - (ni * np.sin(theta) / nt) ** 2)
    a, b, c, e = ni * ci, nt * ct, nt * ci, ni * ct
    cs, cp, tir = coefficients(cr.Stack(), ni, nt, theta)
    assert abs(cs - 2 * np.sqrt(a * b) / (a + b)) <= 1e-12 and abs(cp - 2 * np.sqrt(a * b) / (c + e)) <= 1e-12 and not tir
    u = cr.tilted(theta, 0.4)
    frame = ref.synthetic([[(u, ni, 1), (ref.snell(u, cr.X, ni, nt), nt, 2)]])
    for polarization in (None, (0.2, 1.0, -0.4)):
        want, got = ref.fresnel(frame, polarization), cr.fresnel(frame, polarization, coatings={1: cr.Stack()})
        assert np.max(np.abs(got["transmittance"] - want["transmittance"])) <= 1e-12
        assert np.max(np.abs(got["field"] - want["field"])) <= 1e-12 and cr.counters(got)[4:] == (1, 0)


@pytest.mark.parametrize("seed, n_layers", cr.RANDOM_STACKS)
def test_lossless_stacks_keep_the_energy_and_pass_the_same_from_both_sides(seed, n_layers):
    stack = cr.random_stack(seed, n_layers, absorbing=False, substrate=1.5)
    absorbing = cr.random_stack(seed, n_layers, absorbing=True, substrate=1.5)
    for theta in ANGLES[1:]:
        inner = np.arcsin(np.sin(theta) / 1.5)
        there = coefficients(stack, 1.0, 1.5, theta)
        back = coefficients(stack, 1.5, 1.0, inner)
        bounced = coefficients(stack, 1.0, 1.0, theta, reflection=True)
        for k in range(2):
            assert abs(abs(there[k]) ** 2 + abs(bounced[k]) ** 2 - 1.0) <= 1e-12
            assert abs(abs(there[k]) ** 2 - abs(back[k]) ** 2) <= 1e-12
        there, back = coefficients(absorbing, 1.0, 1.5, theta), coefficients(absorbing, 1.5, 1.0, inner)
        bounced = coefficients(absorbing, 1.0, 1.0, theta, reflection=True)
        for k in range(2):  # (an absorbing stack passes the same from both sides too, and loses energy)
            assert abs(abs(there[k]) ** 2 - abs(back[k]) ** 2) <= 1e-12
            assert abs(there[k]) ** 2 + abs(bounced[k]) ** 2 < 1.0 or n_layers < 2


def test_a_metal_at_normal_incidence_and_the_perfect_conductor():
    n, k = 1.2, 7.0
    rs, rp, tir = coefficients(cr.Stack((), substrate=complex(n, k)), 1.0, 1.0, 0.0, reflection=True)
    want = ((n - 1) ** 2 + k * k) / ((n + 1) ** 2 + k * k)
    assert abs(abs(rs) ** 2 - want) <= 1e-12 and abs(rs + rp) <= 1e-12 and not tir
    for theta in ANGLES:
        rs, rp, _ = coefficients(cr.Stack((), substrate=1e9j), 1.0, 1.0, theta, reflection=True)
        bound = 2 * max(np.cos(theta), 1 / np.cos(theta)) / 1e9 * 1.01
        assert abs(rs + 1.0) <= bound and abs(rp - 1.0) <= bound and abs(rs + 1.0) > 1e-10


@pytest.mark.parametrize("degrees", [42.0, 45.0, 54.6, 70.0, 89.0])
def test_total_internal_reflection_keeps_the_energy_and_shifts_the_phase(degrees):
    theta, n = np.radians(degrees), 1 / 1.5
    rs, rp, tir = coefficients(cr.Stack(), 1.5, 1.5, theta, reflection=True)
    assert tir and abs(abs(rs) - 1.0) <= 1e-12 and abs(abs(rp) - 1.0) <= 1e-12
    delta = np.angle(rs / rp)  # (the basis of include/prt.h: rp = +1 for a perfect conductor, as Born & Wolf's r_par)
    assert abs(np.tan(delta / 2) - np.cos(theta) * np.sqrt(np.sin(theta) ** 2 - n * n) / np.sin(theta) ** 2) <= 1e-12
    assert not coefficients(cr.Stack(), 1.5, 1.5, np.radians(30.0), reflection=True)[2]


# ---- the reference against itself ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, n_layers", cr.RANDOM_STACKS)
def test_rouards_recursion_agrees_on_the_random_stacks(seed, n_layers):
    frame, coatings = cr.random_case(seed, n_layers)
    stack = coatings[1]
    assert len(stack.layers) == n_layers <= 16
    for lam in cr.WAVELENGTHS:
        for material, d in stack.layers:
            n = cr.index(material, lam)
            assert n.real * d / 0.633 <= 1.0 and n.imag * d / 0.633 <= 0.25
    for polarization in (None, (0.3, 1.0, -0.2), (0.0, 1.0, 1.0j)):
        one = cr.fresnel(frame, polarization, coatings=coatings)
        two = cr.fresnel(frame, polarization, coatings=coatings, formulation=cr.rouard_coefficients)
        assert cr.counters(one) == cr.counters(two) and one["n_invalid"] == 0 and one["n_tir"] >= 1
        assert np.max(np.abs(one["transmittance"] - two["transmittance"])) <= 1e-13
        assert np.max(np.abs(one["field"] - two["field"])) <= 1e-13
        assert np.all(one["transmittance"] <= 1.0 + 1e-13) and np.min(one["transmittance"]) < 0.9


def test_invalid_interfaces_in_the_reference():
    rays = cr.four_ways(0.4)
    frame = cr.with_wavelengths(ref.synthetic(rays), [LAM])
    no_substrate = cr.fresnel(frame, coatings={1: cr.Stack()})
    assert no_substrate["n_invalid"] == 1 and np.isnan(no_substrate["transmittance"][6])
    assert np.isfinite(np.delete(no_substrate["transmittance"], 6)).all()
    bad = frame.copy()
    bad[:, ref.IX["wavelength"]] = np.nan
    assert cr.fresnel(bad, coatings={1: cr.Stack(substrate=1.5)})["n_invalid"] == 4
    assert cr.fresnel(bad, coatings={7: cr.Stack()})["n_invalid"] == 0
    assert cr.fresnel(frame, coatings={1: cr.Stack([(np.inf, 0.1)], substrate=1.5)})["n_invalid"] == 4


# ---- the binding and the library -------------------------------------------------------------------------------------------
def host_frame():
    frame = cr.with_wavelengths(ref.synthetic(cr.four_ways(0.3)[:1]), [LAM])
    return DeviceFrame(np.ascontiguousarray(frame.T), [1, 1, 1])


def test_coating_and_fresnel_arguments_are_checked_before_the_gpu():
    with pytest.raises(ValueError, match="at most 16 layers"):
        Coating([(1.38, 0.1)] * 17)
    for bad in ([(1.38, -0.1)], [(1.38, np.nan)], [(1.38,)], [("glass", 0.1)], [1.38]):
        with pytest.raises(ValueError, match="Coating"):
            Coating(bad)
    with pytest.raises(ValueError, match="Coating"):
        Coating((), substrate="silver")
    coating = Coating([(glass["BK7"], 0.1), (lambda w: 1.38 + 0 * w, 0.2), (2.0 + 0.1j, 0.0)], substrate=glass["SF5"])
    table = coating.table(np.array([0.5, 0.6]))
    assert table.shape == (18, 2) and table.dtype == np.complex128
    assert table[1, 0] == glass["BK7"].index_at(0.5) and table[2, 1] == 1.38 and table[3, 0] == 2.0 + 0.1j
    assert table[17, 1] == glass["SF5"].index_at(np.array([0.6]))[0] and table[0, 0] == 1.0 and table[4, 0] == 1.0
    frame = host_frame()
    with pytest.raises(ValueError, match="both lossless and coated"):
        frame.fresnel(lossless=[1, 2], coatings={2: Coating()})
    with pytest.raises(ValueError, match="at most 64 coated"):
        frame.fresnel(coatings={k: coating for k in range(65)})
    with pytest.raises(ValueError, match="at most 16 coatings"):
        frame.fresnel(coatings={k: Coating() for k in range(17)})
    with pytest.raises(ValueError, match="maps a surface to a Coating"):
        frame.fresnel(coatings={1: 1.38})
    with pytest.raises(ValueError, match="mapping"):
        frame.fresnel(coatings=[1, 2])
    with pytest.raises(ValueError, match="at most 64 lossless"):
        frame.fresnel(lossless=range(65), coatings={})
    for bad in ((0, 0, 0j), (1, 2j), (np.nan, 0, 1j), (np.inf * 1j, 0, 1)):
        with pytest.raises(ValueError, match="polarization"):
            frame.fresnel(polarization=bad, coatings={})
    with pytest.raises(ValueError, match="where"):
        frame.where(surface=1).fresnel(coatings={})
    with pytest.raises(ValueError, match="without the column"):
        DeviceFrame(np.zeros((15, 2)), [2], columns=(0, 1, 3, 4, 5, 12, 13, 14)).fresnel(coatings={1: Coating()})


def test_abi_entries_are_declared_and_bound():
    from pyrayt_amd import engine

    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("prt_frame_fresnel_coated_workspace_bytes", "prt_frame_fresnel_coated"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    assert "prt_frame_fresnel_coated" in re.search(r"#define PRT_VERSION \d+ /\*(.*?)\*/", header, flags=re.S).group(1)
    assert "Im(nj cos θj) >= 0" in header or "Im(nj cos thetaj) >= 0" in header
    if os.path.exists(engine.LIB_PATH):
        lib = engine.library()
        assert len(lib.prt_frame_fresnel_coated.argtypes) == 25
        assert len(lib.prt_frame_fresnel_coated_workspace_bytes.argtypes) == 2


def test_library_checks_coated_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    sizes = [lib.prt_frame_fresnel_coated_workspace_bytes(3 * n, n) for n in (1, 2, 1000, 10 ** 6, 2 ** 31)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:])) and sizes[3] - sizes[2] == (10 ** 6 - 1000) * 108
    for args in ((-1, 1), (3, 0), (3, -1), (3, 2 ** 31 + 1)):
        assert lib.prt_frame_fresnel_coated_workspace_bytes(*args) == -1, args
    buf = np.zeros(64)
    p = buf.ctypes.data
    counts = np.array([2, 2], dtype=np.int64)
    many = np.arange(65, dtype=np.int64)
    zeros32 = np.zeros(65, dtype=np.int32)
    thick = np.zeros((16, 16))
    waves = np.linspace(0.4, 0.7, 257)
    table = np.ones((16, 18, 257, 2))
    base = dict(rows=p, ld=4, counts=counts, n_generations=2, id0=0.0, n_ids=2, polarization=None, lossless=many, n_lossless=0,
                surfaces=many, coating_of=zeros32, n_coated=1, n_coatings=1, layers=zeros32, substrate=zeros32, thick=thick,
                waves=waves, n_waves=2, table=table, t=p, field=None, record=p, work=p)

    def ptr(value):
        return value.ctypes.data if isinstance(value, np.ndarray) else value

    def call(**changes):
        a = {**base, **changes}
        return lib.prt_frame_fresnel_coated(
            0, a["rows"], a["ld"], ptr(a["counts"]), a["n_generations"], a["id0"], a["n_ids"], ptr(a["polarization"]),
            ptr(a["lossless"]), a["n_lossless"], ptr(a["surfaces"]), ptr(a["coating_of"]), a["n_coated"], a["n_coatings"],
            ptr(a["layers"]), ptr(a["substrate"]), ptr(a["thick"]), ptr(a["waves"]), a["n_waves"], ptr(a["table"]), a["t"],
            a["field"], a["record"], a["work"], None)

    def int32(*values):
        return np.array(values, dtype=np.int32)

    bad_thick, nan_thick = thick.copy(), thick.copy()
    bad_thick[0, 1], nan_thick[0, 0] = -1e-3, np.nan
    for kwargs, message in ((dict(n_lossless=65), "at most 64 lossless"),
                            (dict(polarization=np.zeros(6)), "polarization finite and not zero"),
                            (dict(polarization=np.array([0, 1, 0, np.inf, 0, 0])), "polarization finite and not zero"),
                            (dict(n_ids=0), "n_ids in [1, 2^31]"),
                            (dict(id0=float("nan")), "id0 finite"),
                            (dict(counts=np.array([2, -1], dtype=np.int64)), "counts >= 0"),
                            (dict(counts=np.array([2 ** 40, 2], dtype=np.int64), ld=2 ** 41), "too many rows in a generation"),
                            (dict(counts=None), "bad buffers"),
                            (dict(ld=3), "bad buffers"),
                            (dict(rows=None), "bad buffers"),
                            (dict(t=None), "bad buffers"),
                            (dict(record=None), "bad buffers"),
                            (dict(work=None), "bad buffers"),
                            (dict(n_coated=65), "at most 64 coated surfaces"),
                            (dict(n_coated=-1), "at most 64 coated surfaces"),
                            (dict(surfaces=None), "at most 64 coated surfaces"),
                            (dict(coating_of=None), "at most 64 coated surfaces"),
                            (dict(n_coatings=17), "at most 16 coatings"),
                            (dict(n_coatings=-1), "at most 16 coatings"),
                            (dict(table=None), "at most 16 coatings"),
                            (dict(thick=None), "at most 16 coatings"),
                            (dict(n_waves=257), "at most 256 wavelengths"),
                            (dict(n_waves=2, waves=None), "at most 256 wavelengths"),
                            (dict(waves=np.array([0.5, 0.5])), "ascending and distinct"),
                            (dict(waves=np.array([0.6, 0.5])), "ascending and distinct"),
                            (dict(waves=np.array([0.0, 0.5])), "ascending and distinct"),
                            (dict(waves=np.array([0.5, np.inf])), "ascending and distinct"),
                            (dict(waves=np.array([np.nan, 0.5])), "ascending and distinct"),
                            (dict(layers=int32(17)), "at most 16 layers"),
                            (dict(layers=int32(-1)), "at most 16 layers"),
                            (dict(layers=int32(2), thick=bad_thick), "thicknesses finite and >= 0"),
                            (dict(layers=int32(2), thick=nan_thick), "thicknesses finite and >= 0"),
                            (dict(coating_of=int32(1)), "names a coating that is not there"),
                            (dict(coating_of=int32(-1)), "names a coating that is not there"),
                            (dict(n_coated=1, n_coatings=0), "names a coating that is not there"),
                            (dict(n_coated=3, surfaces=np.array([4, 5, 4], dtype=np.int64)), "listed twice"),
                            (dict(n_lossless=2, n_coated=2), "both lossless and coated")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())
    record = np.full(6, 7, dtype=np.int64)  # (an empty frame is served on the host; the caps themselves pass)
    empty = dict(counts=np.zeros(2, dtype=np.int64), rows=None, t=None, record=record.ctypes.data)
    assert call(**empty, polarization=np.array([0.0, 1.0, 0.0, 0.0, 0.0, 1.0])) == 0 and record.tolist() == [0] * 6
    assert call(**empty, n_coated=64, n_coatings=16, layers=np.full(16, 16, dtype=np.int32), n_waves=256,
                waves=np.ascontiguousarray(waves[:256]), table=np.ones((16, 18, 256, 2))) == 0


def test_the_coated_kernel_uses_no_scratch_and_what_design_states():
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pyrayt_amd import engine

    if not os.path.exists(mod.READELF):
        pytest.skip("llvm-readelf not available")
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    kernels = {name: res for name, res in mod.kernel_resources(engine.LIB_PATH).items() if KERNEL in name}
    assert len(kernels) == 1, sorted(kernels)
    stated = re.search(rf"`{KERNEL}`: (\d+) VGPRs, (\d+) bytes of LDS, no\s+scratch", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert stated, f"DESIGN.md states the VGPRs and LDS of {KERNEL}"
    for name, res in kernels.items():
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, res  # (no memory behind a lane)
        assert res["vgpr_count"] == int(stated.group(1)) and res["group_segment_fixed_size"] == int(stated.group(2)), res
