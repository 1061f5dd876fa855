"""The longdouble reference of the MTF sensitivities (tests/mtf_gradient_reference.py) against central differences of the
OTF's own reference and against closed forms; the Python copies of the partition rules against the header's text; what
``mtf_gradient`` and the entry point refuse without a GPU; the code object of k_mtfg_sum."""
import os
import re

import numpy as np
import pytest

import diffraction_reference as R
import mtf_gradient_reference as M

LD = np.longdouble
ROOT = R.ROOT
FREQUENCIES, AZIMUTHS, FOCUS = (0.0, 3.0, 30.0, 100.0), (0.0, 90.0, 33.0), (0.0, 0.05, -0.03)
STEP = 1e-4  # of a parameter whose dQ is of order 1 and duh of order 0.3: 2 pi nu |dx| h <= 0.1 rad at nu = 100


def central_difference(case, k, h, centre, focus=FOCUS):
    """(OTF(+h) - OTF(-h)) / (2 h) of diffraction_reference.mtf_reference on (q + h dQ_k, uh + h duh_k), built in
    longdouble: (re, im) longdouble."""
    frame = case.frame
    q, u, w = frame[case.rows, 9:12].astype(LD), frame[case.rows, 12:15].astype(LD), frame[case.rows, 1]
    unit = u / np.sqrt((u * u).sum(axis=1))[:, None]
    dq, du = case.jacobian[k].T.astype(LD), case.slopes[k].T.astype(LD)
    sides = []
    for sign in (1, -1):
        step = LD(sign) * LD(h)
        sides.append(R.mtf_reference(q + step * dq, unit + step * du, w, case.group, case.n_groups, FREQUENCIES, AZIMUTHS,
                                     focus, centre=centre))
    return (sides[0].re - sides[1].re) / (2 * LD(h)), (sides[0].im - sides[1].im) / (2 * LD(h))


def richardson(name, dre, dim, coarse, fine):
    """|ref - D(h/2)| <= |D(h) - D(h/2)| at every output, and |D(h) - D(h/2)| <= 1 % of the largest |dOTF|."""
    gap = np.hypot(coarse[0] - fine[0], coarse[1] - fine[1]).astype(float)
    miss = np.hypot(dre - fine[0], dim - fine[1]).astype(float)
    scale = float(np.hypot(dre, dim).max())
    print(f"[mtf gradient] {name}: largest |dOTF| {scale:.3e}, |D(h) - D(h/2)| <= {gap.max():.3e}, "
          f"|ref - D(h/2)| <= {miss.max():.3e}")
    assert scale > 0
    assert np.all(miss <= gap), (name, float((miss - gap).max()))
    assert gap.max() <= 0.01 * scale, (name, gap.max(), scale)


@pytest.mark.parametrize("counts", ([300], [40, 0, 170]), ids=("one_group", "three_groups_one_empty"))
def test_reference_against_central_differences(counts):
    case = M.gradient_case(counts, 3, seed=4)
    centre = np.array([[1e-4, -2e-4, 3e-4]] * len(counts))
    ref = M.reference_of(case, FREQUENCIES, AZIMUTHS, FOCUS, centre=centre)
    full = [g for g, c in enumerate(counts) if c]
    assert np.all(np.isnan(ref.dre[[g for g, c in enumerate(counts) if not c]].astype(float)))
    for k in range(3):
        coarse, fine = (central_difference(case, k, h, centre) for h in (STEP, STEP / 2))
        richardson(f"parameter {k}", ref.dre[full, k], ref.dim[full, k], [x[full] for x in coarse], [x[full] for x in fine])


def test_focus_derivative_against_neighbouring_planes():
    case = M.gradient_case([300], 1, seed=5)
    centre = np.zeros((1, 3))
    planes = (-0.02, 0.0, 0.04)
    ref = M.reference_of(case, FREQUENCIES, AZIMUTHS, planes, centre=centre)
    frame = case.frame
    q, u, w = frame[case.rows, 9:12], frame[case.rows, 12:15], frame[case.rows, 1]
    differences = []
    for h in (2e-4, 1e-4):
        shifted = [R.mtf_reference(q, u, w, case.group, 1, FREQUENCIES, AZIMUTHS, [p + s * h for p in planes], centre=centre)
                   for s in (1, -1)]
        differences.append(((shifted[0].re - shifted[1].re) / (2 * LD(h)), (shifted[0].im - shifted[1].im) / (2 * LD(h))))
    richardson("focus", ref.dre[:, 1], ref.dim[:, 1], *differences)


def test_a_ray_moved_along_itself_changes_nothing():
    """dQ = lambda u with duh = 0: the line is the same line, so every derivative vanishes."""
    case = M.gradient_case([200], 2, seed=6)
    u = case.frame[case.rows, 12:15]
    rng = np.random.default_rng(7)
    jacobian = np.stack([(u * rng.normal(0, 2.0, (len(u), 1))).T for _ in range(2)])
    ref = M.reference_of(case, FREQUENCIES, AZIMUTHS, FOCUS, jacobian=jacobian, slopes=np.zeros_like(jacobian))
    # dp = lambda (u.e - s (u.a)) is zero but for the rounding of u's own slopes in longdouble: 2^-63 of |lambda| |k| 2 pi
    size = np.hypot(ref.dre[:, :2], ref.dim[:, :2]).astype(float)
    assert size.max() <= 2 * np.pi * 100.0 * 8.0 * 2.0 ** -60, size.max()


def test_a_common_shift_is_a_phase_ramp_and_follows_the_centroid():
    """dQ = t for every ray with duh = 0 and t across the axis: dOTF = -2 pi i (k.t) OTF, and 0 when the centre follows
    the centroid -- from the reference, and from MTFGradient's own composition on the same numbers."""
    from pyrayt_amd.frame import MTFGradient

    case = M.gradient_case([150, 90], 2, seed=8)
    n = len(case.rows)
    shifts = np.array([[0.0, 0.7, -0.4], [0.0, -1.1, 0.2]])
    jacobian = np.repeat(shifts[:, :, None], n, axis=2)
    ref = M.reference_of(case, FREQUENCIES, AZIMUTHS, FOCUS, jacobian=jacobian, slopes=np.zeros_like(jacobian))
    kc, ks = (x.astype(LD) for x in R.frequency_table(FREQUENCIES, AZIMUTHS))
    for k, t in enumerate(shifts):
        ramp = -R.TWO_PI * (kc * LD(t[1]) + ks * LD(t[2]))  # (dOTF = i ramp OTF)
        want_re, want_im = -ramp * ref.im, ramp * ref.re
        assert np.hypot(ref.dre[:, k] - want_re, ref.dim[:, k] - want_im).astype(float).max() <= 1e-13
        assert np.abs(ref.dcentroid[:, k].astype(float) - t).max() <= 1e-15
    dre, dim = M.follow_centroid(ref, FREQUENCIES, AZIMUTHS)
    assert np.hypot(dre, dim).astype(float).max() <= 1e-13
    record = np.concatenate([ref.centre.astype(float), ref.sum_weights.astype(float)[:, None], ref.n_rays[:, None],
                             ref.n_missed[:, None], ref.n_unfollowed[:, None],
                             ref.dcentroid.astype(float).reshape(2, -1)], axis=1)
    for reference, largest in (("fixed", None), ("centroid", 1e-9)):
        made = MTFGradient(ref.otf, ref.dotf, record, FREQUENCIES, AZIMUTHS, FOCUS, R.default_axes(), ("p0", "p1"), reference)
        assert made.dotf.shape == (2, 2, 3, 3, 4) and made.dotf_dfocus.shape == (2, 3, 3, 4)
        assert made.n_rays.tolist() == [150, 90] and made.centroid_gradient.shape == (2, 2, 3)
        if largest is not None:
            assert np.abs(made.dotf).max() <= largest  # (fp64 parts of a longdouble cancellation of terms of order 500)
        # |OTF| does not see where the centre is: dmtf is 0 either way (NaN where |otf| = 0, and nowhere else)
        assert np.array_equal(np.isnan(made.dmtf), np.broadcast_to((made.mtf == 0)[:, None], made.dmtf.shape))
        assert np.nanmax(np.abs(made.dmtf)) <= 1e-9
    table = made.to_pandas()
    assert list(table.columns) == ["source_id", "focus", "azimuth", "frequency", "mtf", "dmtf_dfocus", "dmtf_0", "dptf_0",
                                   "dmtf_1", "dptf_1"]
    assert len(table) == 2 * 3 * 3 * 4


def test_step_solves_the_linearised_residuals():
    """step(): with dmtf exactly linear in the parameters the Gauss-Newton step lands on the target."""
    from pyrayt_amd.frame import MTFGradient

    rng = np.random.default_rng(9)
    otf = (0.4 + 0.3 * rng.random((1, 2, 2, 3))) * np.exp(1j * rng.normal(size=(1, 2, 2, 3)))
    jac = rng.normal(size=(1, 2, 2, 2, 3))  # (G, K, F, A, N): the dmtf wanted
    dotf = np.concatenate([jac * otf[:, None] / np.abs(otf)[:, None], np.zeros((1, 1, 2, 2, 3))], axis=1)
    record = np.zeros((1, 7 + 6))
    record[0, 3:5] = 1.0, 10
    made = MTFGradient(otf, dotf, record, [1.0, 2.0, 3.0], [0.0, 90.0], [0.0, 0.1], R.default_axes(), ("a", "b"))
    np.testing.assert_allclose(made.dmtf, jac, rtol=0, atol=1e-12)
    wanted = np.array([0.02, -0.01])
    target = made.mtf[0, 1] + np.einsum("kan,k->an", jac[0, :, 1], wanted)
    # (a target per output is not the interface: one number is; check the normal equations through a uniform target)
    step = made.step(target=0.9, focus=0.1)
    design = jac[0, :, 1].reshape(2, -1).T
    want = np.linalg.lstsq(design, (0.9 - made.mtf[0, 1]).reshape(-1), rcond=None)[0]
    np.testing.assert_allclose(step[0], want, rtol=1e-9, atol=1e-12)
    assert target.shape == (2, 3)
    with pytest.raises(ValueError, match="focus"):
        made.step(focus=0.2)
    with pytest.raises(ValueError, match="damping"):
        made.step(damping=-1.0)


def test_the_partition_rules_are_the_headers_own_lines():
    for name, lines in M.HOST_RULES.items():
        text = " ".join(open(os.path.join(ROOT, "pyrayt_amd", "csrc", name)).read().split())
        for line in lines:
            assert " ".join(line.split()) in text, (name, line)
    K = M.K
    assert (K.kMtfgBlock, K.kMtfgTile, K.kMtfgOut, K.kMtfgParams, K.kMtfgChunk, K.kMtfgMinSlice, K.kMtfgMaxSlices) == (
        256, 128, 2, 8, 1024, 2048, 256)
    assert [M.slices(n, 1, 256) for n in (0, 1, 2048, 2049, 3 * 2048 + 1, 10 ** 6)] == [1, 1, 1, 2, 4, 256]
    assert M.slices(10 ** 6, 2, 2 ** 16) == (256 << 20) // (2 * 2 ** 16 * 18 * 16) == 7
    assert [M.lanes(n) for n in (1, 128, 129, 256, 257, 512, 513)] == [4, 4, 2, 2, 1, 1, 1]
    assert [M.tile(n) for n in (128, 256, 512)] == [128, 256, 512]
    assert M.parameter_chunks(1) == [(1, 1, 0)] and M.parameter_chunks(7) == [(8, 1, 0)]
    assert M.parameter_chunks(8) == [(8, 1, 0)] and M.parameter_chunks(9) == [(8, 1, 0), (1, 1, 8)]
    assert M.parameter_chunks(16) == [(8, 2, 0)] and M.parameter_chunks(11) == [(8, 1, 0), (4, 1, 8)]
    for outputs in M.OUTPUT_COUNTS:
        assert np.prod(outputs) in (127, 128, 129, 256, 257, 512, 513), outputs


def test_mtf_gradient_needs_slopes():
    from pyrayt_amd.frame import Sensitivity

    bare = Sensitivity(None, None, np.zeros((1, 11)), np.zeros((1, 3)), True, (0, 0, 0, 0), ["p"])
    assert bare.slopes is None
    with pytest.raises(ValueError, match=r"mtf_gradient: .*slopes=True"):
        bare.mtf_gradient([10.0])


def test_abi_entries_are_declared():
    import pyrayt_amd
    from pyrayt_amd import engine

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "prt.h")).read(), flags=re.S)
    for name in ("prt_frame_mtf_gradient_workspace_bytes", "prt_frame_mtf_gradient"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    assert "prt_frame_mtf_gradient" in re.search(r"#define PRT_VERSION \d+ /\*(.*?)\*/", header, flags=re.S).group(1)
    assert pyrayt_amd.MTFGradient is pyrayt_amd.frame.MTFGradient and "MTFGradient" in pyrayt_amd.__all__


def test_library_checks_mtf_gradient_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    assert lib.prt_frame_mtf_gradient_workspace_bytes(1000, 2, 16, 128, 2, 1) >= 1000 * (48 + 16 * 32)
    for args in ((1000, 2, 0, 128, 2, 1), (1000, 2, 17, 128, 2, 1), (1000, 2, 4, 4097, 2, 1), (1000, 2, 4, 128, 17, 1),
                 (1000, 2, 4, 128, 2, 257), (1000, 0, 4, 128, 2, 1), (-1, 1, 4, 128, 2, 1), (1000, 65536, 4, 128, 2, 1)):
        assert lib.prt_frame_mtf_gradient_workspace_bytes(*args) == -1, args
    buf = np.zeros(64)
    p = buf.ctypes.data
    axes = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
    nu, theta, focus = np.array([0.0, 10.0]), np.array([0.0, 90.0]), np.array([0.0])
    first = np.array([0, 4], dtype=np.int64)

    def call(frequencies=nu, n_f=2, azimuths=theta, n_a=2, planes=focus, n_p=1, weight=1, n_groups=1, axes=axes, K=2,
             first=first, n_selected=4, n_rows=4, jacobian=p, out=p):
        return lib.prt_frame_mtf_gradient(0, p, 4, n_rows, p, n_selected, first.ctypes.data, n_groups, weight, jacobian, p,
                                          K, None, axes.ctypes.data, frequencies.ctypes.data, n_f, azimuths.ctypes.data,
                                          n_a, planes.ctypes.data, n_p, p, out, p, p, None)

    big = np.zeros(4097)
    for kwargs, message in ((dict(frequencies=np.array([-1.0, 1.0])), "frequencies finite and >= 0"),
                            (dict(frequencies=np.array([np.nan, 1.0])), "frequencies finite and >= 0"),
                            (dict(frequencies=big, n_f=4097), "1 to 4096 frequencies"),
                            (dict(n_a=17, azimuths=np.zeros(17)), "1 to 16 azimuths"),
                            (dict(azimuths=np.array([0.0, np.inf])), "azimuths finite"),
                            (dict(n_p=257, planes=np.zeros(257)), "1 to 256 focus shifts"),
                            (dict(planes=np.array([np.nan])), "focus shifts finite"),
                            (dict(weight=15), "weight_column"),
                            (dict(axes=np.full(9, np.nan)), "axes: finite"),
                            (dict(K=0), "1 to 16 parameters"),
                            (dict(K=17), "1 to 16 parameters"),
                            (dict(jacobian=None), "jacobian and slopes"),
                            (dict(out=None), "bad buffers"),
                            (dict(n_selected=5, first=np.array([0, 5], dtype=np.int64)), "more selected rows than rows"),
                            (dict(first=np.array([0, 3], dtype=np.int64)), "group_first runs from 0 to n_selected"),
                            (dict(n_groups=2, first=np.array([0, 5, 4], dtype=np.int64)), "group_first does not decrease"),
                            (dict(frequencies=np.zeros(4096), n_f=4096, azimuths=np.zeros(16), n_a=16,
                                  planes=np.zeros(256), n_p=256), "slab cap")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())


def test_the_sum_kernel_uses_no_scratch():
    """Every k_mtfg_sum instantiation keeps its fp64 accumulators in registers: no private segment, no spills."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pyrayt_amd import engine

    if not os.path.exists(mod.READELF):
        pytest.skip("llvm-readelf not available")
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    kernels = {name: res for name, res in mod.kernel_resources(engine.LIB_PATH).items() if "k_mtfg_sum" in name}
    assert len(kernels) == 4, sorted(kernels)
    for name, res in kernels.items():
        assert res["private_segment_fixed_size"] == 0, (name, res)
        assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0, (name, res)
        assert res["vgpr_count"] <= 256, (name, res)  # (two waves per SIMD at the least)
