"""The host side of the polarised diffraction PSF (CPU): the argument checks that come before the library is loaded, the
ABI entries and their own checks, the VectorPSF's host-side sums, and the longdouble reference of
tests/vector_psf_reference.py against cases whose answer is known."""
import os
import re

import numpy as np
import pytest

import diffraction_reference as R
import vector_psf_reference as V
from pyrayt_amd.frame import PSF, DeviceFrame, Fresnel, VectorPSF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def host_frame():
    rows = np.zeros((15, 2))
    rows[0], rows[2], rows[4], rows[5] = [0, 1], 0.633, [0, 0], [1, 2]
    return DeviceFrame(rows, [1, 1])


def test_psf_fresnel_arguments_are_checked_before_the_library_is_loaded(monkeypatch):
    from pyrayt_amd import engine

    def loaded():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(engine, "library", loaded)
    frame, other = host_frame(), host_frame()
    field, record = np.zeros((6, 2)), np.zeros(4, dtype=np.int64)
    with pytest.raises(ValueError, match="another frame"):
        frame.psf(2, world_unit_um=1000, fresnel=Fresnel(other, np.ones(2), field, record, polarization=np.ones(3)))
    with pytest.raises(ValueError, match="fields=True"):
        frame.psf(2, world_unit_um=1000, fresnel=Fresnel(frame, np.ones(2), None, record))
    with pytest.raises(ValueError, match="Fresnel of this frame"):
        frame.psf(2, world_unit_um=1000, fresnel=dict(polarization=(0, 1, 0)))
    with pytest.raises(NotImplementedError):
        frame.psf(2, world_unit_um=1000, group=object(), fresnel=Fresnel(frame, np.ones(2), field, record))
    # the scalar call's own checks still come first
    with pytest.raises(ValueError, match="pixels"):
        frame.psf(2, world_unit_um=1000, pixels=0, fresnel=Fresnel(frame, np.ones(2), field, record))


def test_trace_psf_checks_its_fresnel_keywords_before_the_trace():
    import pyrayt_amd as pyrayt

    tracer = pyrayt.RayTracer(pyrayt.components.LineOfRays(), pyrayt.components.baffle((1, 1)).move_x(1))
    for bad in (dict(fields=True), dict(polarisation=(0, 1, 0)), (0, 1, 0)):
        with pytest.raises(ValueError, match="polarization, lossless and coatings"):
            tracer.trace_psf(1, world_unit_um=1000, fresnel=bad)


def test_abi_entries_are_declared_and_documented():
    from pyrayt_amd import engine

    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("prt_frame_vector_psf_workspace_bytes", "prt_frame_vector_psf"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    assert "prt_frame_vector_psf" in re.search(r"#define PRT_VERSION \d+ /\*(.*?)\*/", header, flags=re.S).group(1)
    for phrase in ("A_r = sqrt(w_r) E_r", "S2 = 2 Re(conj(U1) U2)", "strehl_apodized is the image at P over D'_g",
                   "throughput_g = sum_r w_r |E_r|^2 / sum_r w_r"):
        assert phrase in header, phrase


def test_library_checks_vector_psf_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    ray = 72 + 16  # (a staged and a sorted ray with what lies beside it, per state)
    assert lib.prt_frame_vector_psf_workspace_bytes(1000, 2, 3, 1) > 1000 * 2 * ray
    assert lib.prt_frame_vector_psf_workspace_bytes(1000, 2, 3, 2) > 1000 * 4 * ray
    assert lib.prt_frame_vector_psf_workspace_bytes(1000, 2, 17, 1) == -1
    assert lib.prt_frame_vector_psf_workspace_bytes(1000, 2, 3, 3) == -1
    assert lib.prt_frame_vector_psf_workspace_bytes(1000, 2, 3, 0) == -1
    buf = np.zeros(64)
    lam = np.array([0.5, 0.6] + [0.7 + 0.01 * k for k in range(17)])
    centre, axes = np.zeros(2), R.default_axes()
    p = buf.ctypes.data

    def call(n_w=2, nx=8, ny=8, du=1e-3, unit=1000.0, n_groups=1, planes=6, states=1, field_ld=4, field=p, frame=axes):
        return lib.prt_frame_vector_psf(0, p, 4, 4, 1.0, float("nan"), float(n_groups > 1), n_groups, p, p, p, -1,
                                        lam.ctypes.data, n_w, unit, nx, ny, du, du, centre.ctypes.data, field, field_ld,
                                        planes, states, frame.ctypes.data, p, p, p, p, None)

    bad_axes = axes.copy()
    bad_axes[4] = np.nan
    for kwargs, message in ((dict(n_w=17), "16 distinct"), (dict(nx=0), "1..1024"), (dict(ny=1025), "1..1024"),
                            (dict(du=0.0), "du, dv"), (dict(unit=0.0), "world_unit_um"), (dict(planes=7), "field_planes"),
                            (dict(planes=3), "field_planes"), (dict(states=0), "n_states"), (dict(states=3), "n_states"),
                            (dict(field_ld=3), "field_ld"), (dict(field=None), "bad buffers"),
                            (dict(frame=bad_axes), "axes finite"),
                            (dict(nx=1024, ny=1024, n_groups=3, n_w=2), "slab cap"),
                            (dict(nx=1024, ny=1024, n_groups=3, n_w=1, states=2), "slab cap")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())


def test_the_partition_rules_are_the_headers_own():
    """vpsf_slices restates lines of psf_plan as prt_frame_vector_psf calls it and the GPU tests place their cases by it; the constants are
    read from the header."""
    for name, lines in V.HOST_RULES.items():
        text = open(os.path.join(ROOT, "pyrayt_amd", "csrc", name)).read()
        for line in lines:
            assert line in text, (name, line)
    text = open(os.path.join(ROOT, "pyrayt_amd", "csrc", "prt_vector_psf.hpp")).read()
    K = V.K
    assert K.kVpsfPix in (2, 4) and K.kVpsfTile == K.kPsfBlock * K.kVpsfPix and K.kVpsfPixelBytes == 6 * 8
    assert "struct VpsfRay { double p1, p2, c, re[3], im[3]; };" in text and K.kPsfBlock * 72 == 18 * 1024
    assert V.vpsf_slices(20_000, 2, 1, 63, 256) == 4 and V.vpsf_slices(20_000, 2, 2, 63, 256) == 4
    assert V.vpsf_slices(2049, 1, 2, 63, 256) == 1 and V.vpsf_slices(10 ** 7, 1, 2, 512 * 512, 256) == 2
    # the kernels of the scalar PSF are not touched: the new header only adds
    psf = open(os.path.join(ROOT, "pyrayt_amd", "csrc", "prt_psf.hpp")).read()
    assert "vpsf" not in psf.lower()


def small_case(counts=((40,),), **kw):
    options = dict(pixels=(5, 3), pixel_size=(0.4 * R.LAMBDA_F, 0.45 * R.LAMBDA_F), centre=(0.3 * R.LAMBDA_F, 0.0),
                   opd_waves=0.2, seed=3)
    options.update(kw)
    case = R.psf_case([list(c) for c in counts], **options)
    u, v = R.pixel_centres(case.options["pixels"], case.options["pixel_size"], case.options["centre"])
    return case, case.inputs(u, v)


def close(got, want, scale=1.0, ulps=64):
    """Equal to a few longdouble ulps of ``scale``: the two references add the same terms in another order."""
    eps = float(np.finfo(LD).eps)
    assert np.all(np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)) <= ulps * eps * scale + 4e-16 * np.abs(want))


def test_the_same_unit_vector_on_every_ray_gives_the_scalar_reference():
    """Field e1 on every ray: c = (sqrt(w), 0, 0), so S0 = S1 = the scalar image, S2 = S3 = axial = 0, both Strehl ratios
    are the scalar one and the throughput is 1.  (4e-16 of the value: sqrt(w) is rounded to fp64 on the way in.)"""
    case, inp = small_case(((40, 25),), wavelengths=(0.5, 0.6))
    n = len(inp.opd)
    field = np.zeros((1, n, 3))
    field[0] = V.world_field(np.array([[1.0, 0.0, 0.0]]))
    scalar, vector = R.psf_reference(inp), V.vector_psf_reference(inp, field, 1)
    close(vector.stokes_by_wavelength[:, :, 0], scalar.image_by_wavelength)
    close(vector.stokes_by_wavelength[:, :, 1], scalar.image_by_wavelength)
    assert not vector.stokes_by_wavelength[:, :, 2:].any()
    close(vector.image, scalar.image)
    close(vector.strehl, scalar.strehl)
    close(vector.strehl_apodized, scalar.strehl)
    close(vector.throughput, np.ones(1))
    assert np.array_equal(vector.n_rays, scalar.n_rays) and not vector.n_missed.any()
    # and the same bound as the scalar image has: f_1 is the bucket's share, f_2 = f_3 = 0
    np.testing.assert_allclose(vector.image_bound, scalar.bound, rtol=1e-12)
    np.testing.assert_allclose(vector.bound[:, 0], scalar.bound, rtol=1e-12)
    assert not vector.bound[:, 2:].any()


def test_a_phase_in_the_field_adds_to_the_opd():
    """Field exp(i phi_r) e1 is the scalar sum with phi_r / 2 pi turns added to every ray's phase."""
    case, inp = small_case()
    n = len(inp.opd)
    phi = np.random.default_rng(4).uniform(-np.pi, np.pi, n)
    field = (np.exp(1j * phi)[:, None] * V.world_field(np.array([[1.0, 0.0, 0.0]])))[None]
    scalar = R.psf_reference(inp, offset=lambda b, count: phi.astype(LD) / R.TWO_PI)
    vector = V.vector_psf_reference(inp, field, 1)
    close(vector.stokes[:, 0], scalar.image, ulps=2 ** 14)  # (exp(i phi) enters rounded to fp64: 1e-16 of the amplitude)
    close(vector.strehl, scalar.strehl, ulps=2 ** 14)
    assert float(scalar.strehl[0]) < 0.2  # (random phases: nothing like the unaberrated image)


def test_radial_polarisation_has_a_dark_centre():
    case, field = V.radial_case()
    u, v = R.pixel_centres((5, 5), 0.5 * R.LAMBDA_F, (0.0, 0.0))
    inp = case.inputs(u, v)
    rows = V.selected_rows(case.frame, R.SURFACE, case.options["rays_per_source"], 1)
    vector = V.vector_psf_reference(inp, V.field_of_rows(field, rows), 1)
    n = len(rows)
    assert u[2] == 0.0 and v[2] == 0.0
    assert 0 <= float(vector.stokes[0, 0, 2, 2]) < 1.2 / n ** 2 and float(vector.strehl[0]) < 1.2 / n ** 2
    assert float(vector.strehl_apodized[0]) < 1.2 / n ** 2 and abs(float(vector.throughput[0]) - 1) < 1e-15
    assert float(R.psf_reference(inp).image[0, 2, 2]) > 0.999  # (the scalar sum of the same amplitudes)
    assert float(vector.stokes[0, 0].max()) > 0.1            # (the ring around it)
    assert vector.bound[0, 0, 2, 2] < 1e-9                      # eps^2 f + 2 eps sqrt(I f): eps 5e-7, I < 1e-7, f < 1


def test_the_unpolarised_image_is_the_mean_of_the_two_polarised_ones():
    case, inp = small_case(((30,), (20,)))
    n = len(inp.opd)
    field = np.stack([V.random_field(n, True, 7)[0:3].T, V.random_field(n, True, 8)[0:3].T])
    both = V.vector_psf_reference(inp, field, 2)
    first, second = V.vector_psf_reference(inp, field[:1], 1), V.vector_psf_reference(inp, field[1:], 1)
    for name in ("stokes_by_wavelength", "stokes", "image", "strehl", "throughput"):
        a, b, c = (getattr(x, name) for x in (both, first, second))
        close(a, 0.5 * b + 0.5 * c, scale=float(np.nanmax(np.abs(b))) + float(np.nanmax(np.abs(c))))
    close(both.bound, 0.5 * first.bound + 0.5 * second.bound, scale=1e-3)
    assert np.array_equal(both.n_rays, first.n_rays)
    assert float(both.strehl_apodized[0]) <= 1 + 1e-15 and float(both.throughput[0]) > 0.5


def test_a_ray_without_a_finite_field_is_left_out_and_counted():
    case, inp = small_case()
    n = len(inp.opd)
    field = np.stack([V.random_field(n, False, 9)[0:3].T, V.random_field(n, False, 10)[0:3].T])
    field[1, 3, 2] = np.nan
    field[0, 11, 0] = np.inf
    got = V.vector_psf_reference(inp, field, 2)
    assert got.n_rays.tolist() == [[n - 2]] and got.n_missed.tolist() == [[2]] and np.all(np.isfinite(got.stokes.astype(float)))
    assert V.vector_psf_reference(inp, field, 1).n_missed.tolist() == [[1]]  # (Eb is not read with one state)


def vector_psf(stokes, strehl=None, states=1):
    G, L = stokes.shape[:2]
    record = np.zeros((G, L, states, 6))
    record[..., 0], record[..., 1] = 7, 2
    strehl = np.tile([0.5, 0.8, 0.9, 4.0], (G, 1)) if strehl is None else strehl
    return VectorPSF(stokes, strehl, record, [0.5, 0.6][:L], 1000.0, stokes.shape[3:], (0.1, 0.1), (0.0, 0.0), np.ones(G), None)


def test_vector_psf_object():
    rng = np.random.default_rng(0)
    u = rng.normal(size=(2, 2, 3, 4, 3)) + 1j * rng.normal(size=(2, 2, 3, 4, 3))  # (G, L, component, nx, ny)
    p = np.abs(u) ** 2
    cross = np.conj(u[:, :, 0]) * u[:, :, 1]
    stokes = np.stack([p[:, :, 0] + p[:, :, 1], p[:, :, 0] - p[:, :, 1], 2 * cross.real, 2 * cross.imag, p[:, :, 2]], axis=2)
    got = vector_psf(stokes, states=2)
    assert isinstance(got, PSF) and got.n_states == 2
    assert got.stokes.shape == (2, 4, 4, 3) and got.stokes_by_wavelength.shape == (2, 2, 4, 4, 3)
    assert got.axial.shape == got.image.shape == (2, 4, 3) and got.image_by_wavelength.shape == (2, 2, 4, 3)
    np.testing.assert_allclose(got.image, (p[:, :, 0] + p[:, :, 1] + p[:, :, 2]).sum(axis=1))
    assert got.n_rays.tolist() == [14, 14] and got.n_missed.tolist() == [4, 4]
    assert got.strehl.tolist() == [0.5, 0.5] and got.strehl_apodized.tolist() == [0.8, 0.8]
    assert got.throughput.tolist() == [0.9, 0.9] and got.denominator.tolist() == [4.0, 4.0]
    assert got.peak.shape == (2,) and got.u.shape == (4,) and got.v.shape == (3,)
    table = got.to_pandas()
    assert list(table.columns)[-2:] == ["strehl_apodized", "throughput"] and "strehl" in table.columns
    assert got.encircled_energy(0.15).shape == (2,) and got.mtf([0.0, 1.0]).otf.shape == (2, 1, 2, 2)
    # an analyser is linear in the Stokes images: |conj(j) . U|^2 / |j|^2, wavelength by wavelength
    for jones in ((1, 0), (0, 1), (1, 1), (1, -1), (1, 1j), (1, -1j), (0.3 + 0.2j, -1.1j)):
        j = np.asarray(jones, dtype=complex)
        want = (np.abs(np.conj(j[0]) * u[:, :, 0] + np.conj(j[1]) * u[:, :, 1]) ** 2).sum(axis=1) / (abs(j[0]) ** 2 + abs(j[1]) ** 2)
        np.testing.assert_allclose(got.analyzed(jones), want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got.analyzed((1, 0)) + got.analyzed((0, 1)), got.stokes[:, 0], rtol=1e-12)
    for bad in ((1, 0, 0), (0, 0), (np.nan, 1), "xy"):
        with pytest.raises(ValueError, match="jones"):
            got.analyzed(bad)
    # one wavelength and one state: fully polarised; two wavelengths mixed: no more than that
    single = vector_psf(stokes[:, :1])
    np.testing.assert_allclose(single.degree_of_polarization(), 1.0, rtol=1e-12)
    mixed = got.degree_of_polarization()
    assert mixed.shape == (2, 4, 3) and np.all(mixed <= 1 + 1e-12) and np.any(mixed < 0.99)


def test_uniform_states_turn_the_per_ray_launch_basis_into_states_of_the_beam():
    """fresnel(polarization=None) launches a ray with u x e and u x (u x e), e the world axis of u's smallest component:
    across a cone Ea jumps between y and z.  uniform_states((0, 1, 0)) must give, on every row of a ray, the field of the
    launch state 'y taken perpendicular to u0, normalised' and u0 x that (here the fields are carried unchanged)."""
    torch = pytest.importorskip("torch")
    n = 6
    rng = np.random.default_rng(0)
    u = np.stack([np.ones(n), 0.1 * rng.normal(size=n), 0.1 * rng.normal(size=n)])
    rows = np.zeros((15, 2 * n))
    rows[0], rows[4] = [0] * n + [1] * n, list(range(n)) + list(range(n))[::-1]
    rows[12:15, :n], rows[12:15, n:] = u, u[:, ::-1]
    frame = DeviceFrame(torch.from_numpy(rows), [n, n])
    unit = u / np.linalg.norm(u, axis=0)
    ea, eb = np.zeros((3, n)), np.zeros((3, n))
    for k in range(n):
        a = np.cross(unit[:, k], np.eye(3)[np.argmin(np.abs(unit[:, k]))])
        ea[:, k], eb[:, k] = a / np.linalg.norm(a), np.cross(unit[:, k], a / np.linalg.norm(a))
    assert len({int(np.argmax(np.abs(ea[:, k]))) for k in range(n)}) == 2  # (Ea along z on some rays, along y on others)
    field = np.concatenate([np.concatenate([ea, ea[:, ::-1]], 1), np.concatenate([eb, eb[:, ::-1]], 1)])
    record = np.zeros(6, dtype=np.int64)
    for tensor in (torch.from_numpy(field), torch.from_numpy(field).to(torch.complex128)):
        made = Fresnel(frame, torch.ones(2 * n, dtype=torch.float64), tensor, record)
        assert made.launch_states is None
        got = made.uniform_states((0, 1, 0))
        g1 = np.array([[0.0], [1.0], [0.0]]) - unit[1] * unit
        g1 /= np.linalg.norm(g1, axis=0)
        g2 = np.cross(unit.T, g1.T).T
        want = np.concatenate([np.concatenate([g1, g1[:, ::-1]], 1), np.concatenate([g2, g2[:, ::-1]], 1)])
        assert got.launch_states == "uniform" and got.polarization is None and got.transmittance is made.transmittance
        assert np.abs(got.field.numpy() - want).max() < 1e-15
        assert made.uniform_states().launch_states == "uniform"
    with pytest.raises(ValueError, match="one state"):
        Fresnel(frame, torch.ones(2 * n), torch.from_numpy(field), record, polarization=np.ones(3)).uniform_states()
    with pytest.raises(ValueError, match="fields=True"):
        Fresnel(frame, torch.ones(2 * n), None, record).uniform_states()
