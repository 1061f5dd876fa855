"""The longdouble reference of the PSF sensitivities (tests/psf_gradient_reference.py) against central differences of the
PSF's own reference and against closed forms; the Python copies of the partition rules against the header's text; what
``psf_gradient`` and the entry point refuse without a GPU; the code objects of k_psfg_huygens and k_psf_huygens."""
import os
import re

import numpy as np
import pytest

import diffraction_reference as R
import psf_gradient_reference as P

LD = np.longdouble
ROOT = R.ROOT
GRID = dict(pixels=(7, 5), pixel_size=(2.5e-3, 3.0e-3), centre=(1e-3, -2e-3))
STEP = 2.0 ** -8  # of a parameter whose dopd is a few waves per unit at the rim: 2 pi h |g| stays under 0.1 rad


def grid_inputs(case):
    return case.inputs(*R.pixel_centres(GRID["pixels"], GRID["pixel_size"], GRID["centre"]))


def central_difference(inp, dphase, dpoint, k, h):
    """(I(+h) - I(-h)) / (2 h) and the same of the Strehl ratio, of diffraction_reference.psf_reference on the inputs
    moved along parameter k: longdouble."""
    plus, minus = (R.psf_reference(P.moved_inputs(inp, dphase, dpoint, k, s * h)) for s in (1, -1))
    return ((plus.image_by_wavelength - minus.image_by_wavelength) / (2 * LD(h)), (plus.strehl - minus.strehl) / (2 * LD(h)))


def richardson(name, ref, coarse, fine):
    """|ref - D(h/2)| <= |D(h) - D(h/2)| at every value, and |D(h) - D(h/2)| <= 1 % of the largest |derivative|."""
    gap, miss = np.abs(coarse - fine).astype(float), np.abs(ref - fine).astype(float)
    scale = float(np.abs(ref).max())
    print(f"[psf gradient] {name}: largest |d| {scale:.3e}, |D(h) - D(h/2)| <= {gap.max():.3e}, |ref - D(h/2)| <= {miss.max():.3e}")
    assert scale > 0
    assert np.all(miss <= gap), (name, float((miss - gap).max()))
    assert gap.max() <= 0.01 * scale, (name, gap.max(), scale)


@pytest.mark.parametrize("follow", ("ray", "pupil"))
@pytest.mark.parametrize("counts", ([[120]], [[40, 70], [0, 0]]), ids=("one_bucket", "two_wavelengths_one_group_empty"))
def test_reference_against_central_differences_of_the_psf_reference(counts, follow):
    wavelengths = (0.55,) if len(counts[0]) == 1 else (0.45, 0.65)
    case = P.gradient_case(counts, 3, seed=11, wavelengths=wavelengths)
    inp = grid_inputs(case)
    dphase, dpoint = (case.dopd, case.dpupil) if follow == "ray" else (case.dfield, None)
    ref = P.gradient_reference(inp, dphase, dpoint)
    plain = R.psf_reference(inp)
    full = [g for g, c in enumerate(counts) if sum(c)]
    # the gradient's image and Strehl ratio are the PSF reference's own
    assert np.abs(ref.image_by_wavelength[full] - plain.image_by_wavelength[full]).astype(float).max() <= 1e-17
    assert np.abs(ref.strehl[full] - plain.strehl[full]).astype(float).max() <= 1e-17
    assert np.all(np.isnan(ref.dimage[[g for g, c in enumerate(counts) if not sum(c)]].astype(float)))
    for k in range(3):
        (ci, cs), (fi, fs) = (central_difference(inp, dphase, dpoint, k, h) for h in (STEP, STEP / 2))
        richardson(f"{follow} parameter {k} image", ref.dimage_by_wavelength[full, k], ci[full], fi[full])
        richardson(f"{follow} parameter {k} strehl", ref.dstrehl[full, k], cs[full], fs[full])


def test_a_piston_changes_no_image_and_a_tilt_shifts_it():
    """dopd constant, dpupil zero: dU = 2 pi i e U, so dI = 0 and dStrehl = 0.  dopd = -(t.p) / R adds -(t.p) / R to a
    phase whose pixel term is -(u p1 + v p2) / R to first order in rho / R: the image moves by -t, dI = t.grad I; held
    on a fine grid against the central difference of the image along u (its truncation is under 1 % there)."""
    case = P.gradient_case([[150]], 2, seed=12, piston=0, tilt=(1, (1.0, 0.0)))
    du = 2e-4
    inp = case.inputs(*R.pixel_centres((9, 1), (du, du), (1e-3, -2e-3)))
    ref = P.gradient_reference(inp, case.dopd, case.dpupil)
    assert np.abs(ref.dimage[:, 0]).astype(float).max() <= 1e-15 * float(np.abs(ref.damplitude[0][:, 0]).max())
    assert abs(float(ref.dstrehl[0, 0])) <= 1e-15
    slope = (ref.image[0, 2:] - ref.image[0, :-2]) / (2 * LD(du))
    moved = ref.dimage[0, 1, 1:-1]
    assert np.abs(slope).astype(float).max() > 1.0
    assert np.abs(moved - slope).astype(float).max() <= 0.02 * np.abs(slope).astype(float).max()


def test_rays_left_out_are_counted_and_contribute_nothing():
    case = P.gradient_case([[90, 60]], 4, seed=13, wavelengths=(0.5, 0.6), missed=2, unfollowed=3)
    inp = grid_inputs(case)
    ref = P.gradient_reference(inp, case.dopd, case.dpupil)
    assert ref.n_missed.tolist() == [[2, 2]] and ref.n_unfollowed.tolist() == [[3, 3]] and ref.n_rays.tolist() == [[85, 55]]
    usable, followed = P.kept_rays(inp, case.dopd, case.dpupil)
    keep = usable & followed
    fewer = R.psf_inputs(inp.group[keep], inp.wavelength[keep], inp.opd[keep], inp.pupil[keep], inp.weight[keep], inp.radius,
                         inp.rho, inp.wavelengths, inp.unit, inp.u, inp.v, 1)
    without = P.gradient_reference(fewer, case.dopd[:, keep], case.dpupil[:, :, keep])
    assert np.array_equal(without.dimage.astype(float), ref.dimage.astype(float)) and np.all(np.isfinite(ref.dimage.astype(float)))
    assert np.array_equal(without.dstrehl.astype(float), ref.dstrehl.astype(float))


def test_step_solves_the_linearised_residuals():
    from pyrayt_amd.frame import PSF, PSFGradient

    rng = np.random.default_rng(14)
    G, K, L, nx, ny = 2, 3, 2, 5, 4
    image, dimage = rng.random((G, L, nx, ny)), rng.normal(size=(G, K, L, nx, ny))
    strehl, record = rng.random((G, 1 + K)), np.ones((G, L, 5))
    zeros = np.zeros((G, L, nx, ny), dtype=complex)
    made = PSFGradient(zeros, np.zeros((G, K, L, nx, ny), dtype=complex), image, dimage, strehl, record, (0.5, 0.6), 1000.0,
                       (nx, ny), (1e-3, 1e-3), (0.0, 0.0), np.ones(G), None, ("a", "b", "c"), "ray")
    assert made.image.shape == (G, nx, ny) and made.dimage.shape == (G, K, nx, ny) and made.dstrehl.shape == (G, K)
    wanted = rng.normal(0.0, 0.01, (G, K))
    target = made.image + np.einsum("gkij,gk->gij", made.dimage, wanted)
    np.testing.assert_allclose(made.step(target=target), wanted, rtol=1e-9, atol=1e-12)
    damped = made.step(damping=0.5, target=target)
    assert np.all(np.abs(damped) < np.abs(wanted).max() * 2) and not np.allclose(damped, wanted)
    star = PSF(target[:, None], np.zeros(G), np.ones((G, 1, 4)), (0.5,), 1000.0, (nx, ny), (1e-3, 1e-3), (0.0, 0.0),
               np.ones(G), None)
    np.testing.assert_allclose(made.step(target=star), wanted, rtol=1e-9, atol=1e-12)
    elsewhere = PSF(target[:, None], np.zeros(G), np.ones((G, 1, 4)), (0.5,), 1000.0, (nx, ny), (2e-3, 1e-3), (0.0, 0.0),
                    np.ones(G), None)
    for bad in (dict(target=elsewhere), dict(target=target[:, :-1]), dict(target=None), dict(damping=-1.0, target=target)):
        with pytest.raises(ValueError):
            made.step(**bad)
    table = made.to_pandas()
    assert list(table.columns) == ["strehl", "dstrehl_0", "dstrehl_1", "dstrehl_2", "f_number", "n_rays", "n_missed", "n_unfollowed"]
    assert len(table) == G and table["n_rays"].tolist() == [2, 2]


def test_the_partition_rules_are_the_headers_own_lines():
    for name, lines in P.HOST_RULES.items():
        text = " ".join(open(os.path.join(ROOT, "pyrayt_amd", "csrc", name)).read().split())
        for line in lines:
            assert " ".join(line.split()) in text, (name, line)
    assert (P.K.kPsfgParams, P.K.kPsfgMinSlice, R.K.kPsfBlock, R.K.kPsfTile) == (4, 2048, 256, 1024)
    assert [P.slices(n, 1, 15, 256) for n in (0, 1, 2048, 4095, 4096, 4097, 10 ** 6)] == [1, 1, 1, 1, 2, 2, 488]
    assert P.slices(10 ** 6, 1, 128 * 128, 256) == (256 << 20) // (128 * 128 * 17 * 16) == 60  # (the slab cap, for 16 parameters)
    assert P.parameter_chunks(1) == [(1, 1, 0)] and P.parameter_chunks(3) == [(4, 1, 0)] and P.parameter_chunks(4) == [(4, 1, 0)]
    assert P.parameter_chunks(5) == [(4, 1, 0), (1, 1, 4)] and P.parameter_chunks(9) == [(4, 2, 0), (1, 1, 8)]
    assert P.parameter_chunks(16) == [(4, 4, 0)] and P.parameter_chunks(6) == [(4, 1, 0), (2, 1, 4)]
    assert P.PARAMETER_COUNTS == (1, 3, 4, 5, 9, 16)


def test_psf_gradient_needs_the_wavefront_and_refuses_a_wavelength_change():
    from types import SimpleNamespace

    from pyrayt_amd.frame import Motion, Sensitivity, WavelengthChange

    bare = Sensitivity(None, None, np.zeros((1, 11)), np.zeros((1, 3)), True, (0, 0, 0, 0), ["p"])
    assert bare.wavefront is None
    with pytest.raises(ValueError, match=r"psf_gradient: .*sensitivity\(wavefront=\)"):
        bare.psf_gradient(world_unit_um=1000.0)
    coloured = Sensitivity(None, None, np.zeros((1, 11)), np.zeros((1, 3)), True, (0, 0, 0, 0), [WavelengthChange()])
    coloured.wavefront = SimpleNamespace()
    with pytest.raises(ValueError, match="WavelengthChange"):
        coloured.psf_gradient(world_unit_um=1000.0)
    with pytest.raises(ValueError, match="follow"):
        coloured.psf_gradient(world_unit_um=1000.0, follow="centroid")
    assert Motion is not None


def test_abi_entries_are_declared_and_the_version_stays():
    import pyrayt_amd
    from pyrayt_amd import engine

    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("prt_frame_psf_gradient_workspace_bytes", "prt_frame_psf_gradient"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    found = re.search(r"#define PRT_VERSION (\d+) /\*(.*?)\*/", header, flags=re.S)
    assert int(found.group(1)) == 240
    assert re.search(r"\bprt_frame_psf_gradient\b", found.group(2)) and "prt_frame_psf_gradient_workspace_bytes" in found.group(2)
    assert pyrayt_amd.PSFGradient is pyrayt_amd.frame.PSFGradient and "PSFGradient" in pyrayt_amd.__all__
    assert hasattr(pyrayt_amd.RayTracer, "trace_psf_gradient") and hasattr(pyrayt_amd.Sensitivity, "psf_gradient")


def test_library_checks_psf_gradient_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    assert lib.prt_version() == 240
    assert lib.prt_frame_psf_gradient_workspace_bytes(1000, 2, 16, 3) >= 1000 * (2 * 32 + 8 + 4 + 16 * 24)
    for args in ((1000, 2, 0, 3), (1000, 2, 17, 3), (1000, 2, 4, 0), (1000, 2, 4, 17), (1000, 0, 4, 1), (-1, 1, 4, 1),
                 (1000, 16384, 4, 1)):
        assert lib.prt_frame_psf_gradient_workspace_bytes(*args) == -1, args
    buf = np.zeros(64)
    p = buf.ctypes.data
    lam, uv = np.array([0.55, 0.65]), np.zeros(2)
    first = np.array([0, 4], dtype=np.int64)

    def call(wavelengths=lam, n_w=2, unit=1000.0, nx=8, ny=8, du=1e-3, dv=1e-3, centre=uv, weight=1, n_groups=1, K=2,
             first=first, n_selected=4, n_rows=4, dphase=p, dpoint=None, out=p, groups=p):
        return lib.prt_frame_psf_gradient(0, p, 4, n_rows, p, n_selected, first.ctypes.data, n_groups, weight, p, p, groups,
                                          dphase, dpoint, K, wavelengths.ctypes.data, n_w, unit, nx, ny, du, dv,
                                          centre.ctypes.data, p, out, p, p, p, p, p, None)

    for kwargs, message in ((dict(K=0), "1 to 16 parameters"),
                            (dict(K=17), "1 to 16 parameters"),
                            (dict(dphase=None), "opd, pupil and dphase"),
                            (dict(out=None), "bad buffers"),
                            (dict(groups=None), "bad buffers"),
                            (dict(n_selected=5, first=np.array([0, 5], dtype=np.int64)), "more selected rows than rows"),
                            (dict(first=np.array([0, 3], dtype=np.int64)), "group_first runs from 0 to n_selected"),
                            (dict(n_groups=2, first=np.array([0, 5, 4], dtype=np.int64)), "group_first does not decrease"),
                            (dict(weight=15), "weight_column"),
                            (dict(n_w=17, wavelengths=np.arange(1.0, 18.0)), "1 to 16 distinct wavelengths"),
                            (dict(wavelengths=np.array([0.55, 0.55])), "wavelengths: distinct"),
                            (dict(wavelengths=np.array([0.55, -1.0])), "wavelengths: finite and > 0"),
                            (dict(unit=0.0), "world_unit_um"),
                            (dict(nx=0), "nx, ny in 1..1024"),
                            (dict(ny=1025), "nx, ny in 1..1024"),
                            (dict(du=0.0), "du, dv finite and > 0"),
                            (dict(centre=np.array([np.nan, 0.0])), "centre finite"),
                            (dict(nx=1024, ny=1024), "slab cap")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())


def test_the_huygens_kernel_uses_no_scratch():
    """Every k_psfg_huygens instantiation, and the scalar k_psf_huygens that shares their phase path, keeps its fp64
    accumulators in registers: no private segment, no spills; the scalar kernel fits seven waves per SIMD."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pyrayt_amd import engine

    if not os.path.exists(mod.READELF):
        pytest.skip("llvm-readelf not available")
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    kernels = {name: res for name, res in mod.kernel_resources(engine.LIB_PATH).items() if "k_psfg_huygens" in name or "k_psf_huygens" in name}
    assert len(kernels) == 4, sorted(kernels)  # (P = 1, 2, 4 and the scalar kernel)
    scalar = [res for name, res in kernels.items() if "k_psf_huygens" in name]
    assert len(scalar) == 1 and scalar[0]["vgpr_count"] <= 72, kernels  # (512 / 72: seven waves per SIMD)
    for name, res in kernels.items():
        assert res["private_segment_fixed_size"] == 0, (name, res)
        assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0, (name, res)
        assert res["vgpr_count"] <= 256, (name, res)  # (two waves per SIMD at the least)
