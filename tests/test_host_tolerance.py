"""Tolerancing without a GPU: ``Tolerances`` sampling; the compensator solve against numpy.linalg.lstsq; the longdouble
reference of tests/tolerance_reference.py against the PSF's own reference, against ``gradient_reference`` and against
closed forms; the Python copies of the partition rules against the header's text; what ``Sensitivity.tolerance``, the
classes and the two entry points refuse; the code objects of k_tol_sum against what DESIGN.md states."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import diffraction_reference as R
import psf_gradient_reference as P
import tolerance_reference as T

LD = np.longdouble
ROOT = R.ROOT


# ---- Tolerances -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distribution, variance", (("uniform", 1 / 3), ("normal", 1.0), ("parabolic", 3 / 5)))
def test_tolerances_sampling(distribution, variance):
    from pyrayt_amd import Tolerances

    widths = np.array([0.5, 2.0, 0.0, 1e-3])
    tol = Tolerances(widths, distribution, seed=7)
    a, b = tol.sample(20000), Tolerances(widths, distribution, seed=7).sample(20000)
    assert a.shape == (20000, 4) and a.dtype == np.float64 and np.array_equal(a, b)
    assert np.array_equal(tol.sample(20000), a)  # (the same object, asked again)
    assert not np.array_equal(Tolerances(widths, distribution, seed=8).sample(20000), a)
    assert np.all(a[:, 2] == 0.0)
    if distribution != "normal":
        assert np.all(np.abs(a) <= widths)
    live = [0, 1, 3]
    # the sample variance of 20000 draws is within 5 % (its standard error is under 1.2 % for all three)
    np.testing.assert_allclose(a[:, live].var(axis=0), variance * widths[live] ** 2, rtol=0.05)
    assert np.all(np.abs(a[:, live].mean(axis=0)) <= 0.03 * widths[live])
    if distribution == "parabolic":  # (the ends are favoured: more than half the draws beyond 0.79 of the width)
        assert np.mean(np.abs(a[:, 0]) > 0.5 ** (1 / 3) * widths[0]) == pytest.approx(0.5, abs=0.02)


def test_tolerances_table_layout_and_refusals():
    from pyrayt_amd import Tolerances

    table = Tolerances([0.1, 0.2, 0.3]).sensitivity_table()
    assert table.shape == (7, 3) and not np.any(table[0])
    for k, w in enumerate((0.1, 0.2, 0.3)):
        want = np.zeros(3)
        want[k] = w
        assert np.array_equal(table[1 + 2 * k], -want) and np.array_equal(table[2 + 2 * k], want)
    for bad in (dict(widths=[]), dict(widths=[-1.0]), dict(widths=[np.nan]), dict(widths="wide"),
                dict(widths=[1.0], distribution="triangular")):
        with pytest.raises(ValueError):
            Tolerances(**bad)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError):
            Tolerances([1.0]).sample(bad)


# ---- the compensator solve --------------------------------------------------------------------------------------------------
def covariance_of(y, w):
    mean = (y * w).sum(axis=1) / w.sum()
    d = y - mean[:, None]
    return (d * w) @ d.T / w.sum()


@pytest.mark.parametrize("deficient", (False, True), ids=("full_rank", "rank_deficient"))
def test_compensator_solve_against_lstsq(deficient):
    """The variance of y_0 + sum_c q_c y_c over 400 weighted samples, minimised over three of six columns: against
    numpy.linalg.lstsq on the weighted, centred samples themselves.  Rank-deficient: one free column is the sum of the
    two others, the minimiser is not unique -- the minimum itself is, and the free columns' combined contribution."""
    from pyrayt_amd.frame import moment_covariance, solve_compensators

    rng = np.random.default_rng(3 + deficient)
    n, C, free = 400, 6, [1, 3, 4]
    y = rng.normal(size=(C + 1, n)) * rng.uniform(0.01, 10.0, C + 1)[:, None] + rng.normal(size=(C + 1, 1))
    if deficient:
        y[1 + 4] = y[1 + 1] + y[1 + 3]
    w = rng.uniform(0.2, 1.0, n)
    cov = covariance_of(y.astype(LD), w.astype(LD))
    trials = rng.normal(size=(5, C))
    q, rank = solve_compensators(cov, trials, free)
    assert q.dtype == LD and rank == (2 if deficient else 3)
    fixed = [c for c in range(C) if c not in free]
    assert np.array_equal(q[:, fixed].astype(float), trials[:, fixed])
    root = np.sqrt(w)
    centred = y - ((y * w).sum(axis=1) / w.sum())[:, None]
    for m in range(len(trials)):
        target = -(centred[0] + trials[m, fixed] @ centred[1:][fixed]) * root
        design = (centred[1:][free] * root).T
        want, _, lstsq_rank, _ = np.linalg.lstsq(design, target, rcond=1e-10)
        assert lstsq_rank == rank
        v = np.concatenate([[LD(1)], q[m]])
        least = float(np.sum((design @ want - target) ** 2) / w.sum())
        assert float(v @ cov @ v) == pytest.approx(least, rel=1e-9)
        # what the free columns add to the samples is unique either way
        np.testing.assert_allclose(design @ q[m, free].astype(float), design @ want, rtol=1e-7, atol=1e-9 * np.abs(target).max())
        if not deficient:
            np.testing.assert_allclose(q[m, free].astype(float), want, rtol=1e-8)
    # no free column: the trials come back; moment_covariance reads the layout of include/prt.h
    assert np.array_equal(solve_compensators(cov, trials, [])[0].astype(float), trials)
    sums = [n, 0, 0, w.sum()] + list((y * w).sum(axis=1)) + list(((y * w) @ y.T)[np.tril_indices(C + 1)])
    np.testing.assert_allclose(moment_covariance(np.array(sums), C).astype(float), cov.astype(float), rtol=1e-9, atol=1e-12)
    assert moment_covariance(np.zeros(len(sums)), C) is None


# ---- the reference against what it must agree with ------------------------------------------------------------------------
def test_reference_zero_trial_is_the_psf_references_strehl_and_one_hot_trials_follow_dstrehl():
    """The all-zero trial has the Strehl ratio of diffraction_reference.psf_reference (and of gradient_reference) on the
    same inputs; one-hot trials of size h give (S(h) - S(-h)) / 2h inside the Richardson gap of h and h / 2 about
    gradient_reference's dStrehl: the rule of test_host_psf_gradient.richardson."""
    case = T.tolerance_case([[70, 50], [0, 0]], 3, seed=21, wavelengths=(0.45, 0.65))
    inp = case.tolerance_inputs()
    grad = P.gradient_reference(case.inputs(np.zeros(1), np.zeros(1)), case.dopd, None)
    h = 2.0 ** -8
    trials = np.zeros((2, 1 + 4 * 3, 3))
    for k in range(3):
        for j, step in enumerate((h, -h, h / 2, -h / 2)):
            trials[:, 1 + 4 * k + j, k] = step
    ref = T.tolerance_reference(inp, trials)
    assert abs(float(ref.strehl[0, 0] - grad.strehl[0])) <= 1e-17 and np.all(np.isnan(ref.strehl[1].astype(float)))
    assert np.array_equal(ref.n_rays, grad.n_rays)
    for k in range(3):
        s = ref.strehl[0, 1 + 4 * k:5 + 4 * k]
        coarse, fine = (s[0] - s[1]) / (2 * LD(h)), (s[2] - s[3]) / LD(h)
        gap, miss = abs(float(coarse - fine)), abs(float(grad.dstrehl[0, k] - fine))
        print(f"[tolerance] reference one-hot {k}: dstrehl {float(grad.dstrehl[0, k]):.4e}, gap {gap:.3e}, miss {miss:.3e}")
        assert miss <= gap <= 0.01 * float(np.abs(grad.dstrehl[0]).max())


def test_reference_rays_left_out_a_zero_column_and_the_quadratic_form():
    """Rays left out are counted and contribute nothing; a column whose trial values are 0 changes nothing; the
    variance from the moments' covariance is the sample statistic on the moved OPDs."""
    from pyrayt_amd.frame import moment_covariance

    case = T.tolerance_case([[90, 60]], 4, seed=13, wavelengths=(0.5, 0.6), missed=2, unfollowed=3)
    inp = case.tolerance_inputs()
    trials = T.random_trials(1, 6, 4)
    ref = T.tolerance_reference(inp, trials)
    assert ref.n_missed.tolist() == [[2, 2]] and ref.n_unfollowed.tolist() == [[3, 3]] and ref.n_rays.tolist() == [[85, 55]]
    usable, followed = T.kept_rays(inp)
    keep = usable & followed
    fewer = T.tolerance_inputs(inp.group[keep], inp.wavelength[keep], inp.opd[keep], inp.weight[keep], inp.columns[:, keep],
                               inp.wavelengths, inp.unit, 1)
    without = T.tolerance_reference(fewer, trials)
    assert np.array_equal(without.strehl.astype(float), ref.strehl.astype(float)) and np.all(np.isfinite(ref.strehl.astype(float)))
    wider = T.tolerance_inputs(fewer.group, fewer.wavelength, fewer.opd, fewer.weight,
                               np.vstack([fewer.columns, np.ones((1, keep.sum()))]), fewer.wavelengths, fewer.unit, 1)
    padded = T.tolerance_reference(wider, np.concatenate([trials, np.zeros((1, 6, 1))], axis=2))
    assert np.array_equal(padded.strehl.astype(float), without.strehl.astype(float))
    moments, bound = T.moments_reference(inp)
    assert moments[0, :3].astype(float).tolist() == [140, 4, 6] and np.all(bound[0, 3:] > 0)
    cov = moment_covariance(moments[0], 4)
    v = np.concatenate([np.ones((6, 1), dtype=LD), trials[0].astype(LD)], axis=1)
    rms = np.sqrt(np.einsum("mi,ij,mj->m", v, cov, v))
    np.testing.assert_allclose(rms.astype(float), T.rms_opd_reference(inp, trials)[0].astype(float), rtol=1e-12)


def test_the_bound_is_of_the_order_the_number_formats_give():
    """One bucket, C columns, trials that move the phase by a few cycles: eps per ray is EPS_TRIG + 2 pi 2^-25 plus a
    term of (C + 2) u times the phase -- the Strehl bound lies between 2 eps_0 sqrt(S) and a few times that."""
    case = T.tolerance_case([[200]], 5, seed=9)
    ref = T.tolerance_reference(case.tolerance_inputs(), T.random_trials(1, 8, 5))
    eps0 = R.EPS_TRIG + 2 * np.pi * R.F32_TURN
    low = 2 * eps0 * np.sqrt(ref.strehl[0].astype(float))
    assert np.all(ref.strehl_bound[0] >= low) and np.all(ref.strehl_bound[0] <= 1.5 * low + 4 * eps0 ** 2 + 1e-12)


def test_the_partition_rules_are_the_headers_own_lines():
    for name, lines in T.HOST_RULES.items():
        text = " ".join(open(os.path.join(ROOT, "pyrayt_amd", "csrc", name)).read().split())
        for line in lines:
            assert " ".join(line.split()) in text, (name, line)
    assert (T.K.kTolTrials, T.K.kTolTile, T.K.kTolRays, T.K.kTolMinSlice, T.K.kTolMomentChunk) == (2, 512, 128, 2048, 2048)
    assert [T.slices(n, 1, 256) for n in (0, 1, 2048, 4095, 4096, 4097, 10 ** 6)] == [1, 1, 1, 1, 2, 2, 488]
    assert T.slices(10 ** 6, 4, 256) == 122 and T.slices(10 ** 7, 1, 256) == 1024
    assert T.trial_chunk(1, 1024) == 16384 and T.trial_chunk(16383, 1) >= T.K.kTolTile
    assert [T.template_columns(c) for c in (1, 4, 5, 16, 17, 20)] == [4, 4, 8, 16, 20, 20]
    assert T.TRIAL_COUNTS == (1, 2, 3, 510, 511, 512, 513, 1024, 1025) and T.COLUMN_COUNTS == (1, 3, 4, 5, 16, 19, 20)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_tolerance_needs_the_wavefront_and_refuses_what_it_cannot_serve():
    from pyrayt_amd.frame import Sensitivity, Tolerances, WavelengthChange

    bare = Sensitivity(None, None, np.zeros((1, 11)), np.zeros((1, 3)), True, (0, 0, 0, 0), ["p"])
    with pytest.raises(ValueError, match=r"tolerance: .*sensitivity\(wavefront=\)"):
        bare.tolerance(np.zeros((1, 1)), world_unit_um=1000.0)
    coloured = Sensitivity(None, None, np.zeros((1, 11)), np.zeros((1, 3)), True, (0, 0, 0, 0), [WavelengthChange()])
    coloured.wavefront = SimpleNamespace()
    with pytest.raises(ValueError, match="WavelengthChange"):
        coloured.tolerance(np.zeros((1, 1)), world_unit_um=1000.0)
    with pytest.raises(ValueError, match="follow"):
        coloured.tolerance(np.zeros((1, 1)), world_unit_um=1000.0, follow="centroid")
    plain = Sensitivity(None, None, np.zeros((1, 17)), np.zeros((1, 3)), True, (0, 0, 0, 0), ["a", "b"])
    plain.wavefront = SimpleNamespace()
    for trials in (np.zeros((3, 1)), np.zeros(2), np.zeros((0, 2)), np.full((1, 2), np.nan), "many", np.zeros((65536, 2)),
                   (Tolerances([1.0]), 5)):
        with pytest.raises(ValueError, match="trials"):
            plain.tolerance(trials, world_unit_um=1000.0)
    with pytest.raises(ValueError, match="world_unit_um"):
        plain.tolerance(np.zeros((1, 2)), world_unit_um=0.0)
    for compensators in (("defocus",), (2,), (-1,), (0.5,), (True,)):
        with pytest.raises(ValueError, match="compensators"):
            plain.tolerance(np.zeros((1, 2)), world_unit_um=1000.0, compensators=compensators)
    with pytest.raises(ValueError, match="each one once"):
        plain.tolerance(np.zeros((1, 2)), world_unit_um=1000.0, compensators=("tilt", 1, "tilt"))


def test_tolerance_run_reads_its_arrays():
    from pyrayt_amd.frame import ToleranceRun, Tolerances

    tol = Tolerances([0.1, 0.2])
    trials = np.vstack([tol.sensitivity_table(), np.zeros((1, 2))])  # (the nominal trial last, as tolerance() adds it)
    G, M = 2, len(trials)
    strehl = np.vstack([np.array([0.9, 0.5, 0.85, 0.88, 0.7, 0.9]), np.full(M, np.nan)])
    rms = np.vstack([np.arange(M, dtype=float), np.full(M, np.nan)])
    run = ToleranceRun(trials, ("tilt", 1), np.zeros((G, M, 3)), rms, strehl, np.zeros((G, 1, M), dtype=complex), rms * 2,
                       np.ones((G, 1, 5)), np.zeros((G, 9)), (0.55,), 1000.0, ("a", "b"), "ray")
    assert run.trials.shape == (5, 2) and run.strehl.shape == (2, 5) and run.nominal.strehl[0] == 0.9
    assert run.yield_(0.8).tolist()[0] == 3 / 5 and np.isnan(run.yield_()[1])
    assert run.percentiles((0, 100))["strehl"][0].tolist() == [0.5, 0.9]
    frame = run.to_pandas()
    assert list(frame.columns) == ["source_id", "trial", "strehl", "rms_opd", "rms_radius", "p_0", "p_1", "c_tilt_u",
                                   "c_tilt_v", "c_1"] and len(frame) == 10
    table = run.table()
    assert table["parameter"].tolist() == [0, 1] and table["worst"].tolist() == pytest.approx([-0.4, -0.2])
    assert table["dstrehl_plus"].tolist() == pytest.approx([-0.05, -0.2]) and table["width"].tolist() == [0.1, 0.2]
    other = ToleranceRun(np.ones((4, 2)), (), np.zeros((G, 4, 0)), rms[:, :4], strehl[:, :4], np.zeros((G, 1, 4), dtype=complex),
                         rms[:, :4], np.ones((G, 1, 5)), np.zeros((G, 9)), (0.55,), 1000.0, ("a", "b"), "ray")
    with pytest.raises(ValueError, match="sensitivity_table"):
        other.table()


def test_abi_entries_are_declared_and_the_version_stays():
    import pyrayt_amd
    from pyrayt_amd import engine

    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("prt_frame_tolerance_workspace_bytes", "prt_frame_tolerance", "prt_frame_tolerance_moments_workspace_bytes",
                 "prt_frame_tolerance_moments"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    found = re.search(r"#define PRT_VERSION (\d+) /\*(.*?)\*/", header, flags=re.S)
    assert "prt_frame_tolerance_moments" in found.group(2)
    assert pyrayt_amd.Tolerances is pyrayt_amd.frame.Tolerances and pyrayt_amd.ToleranceRun is pyrayt_amd.frame.ToleranceRun
    assert "Tolerances" in pyrayt_amd.__all__ and "ToleranceRun" in pyrayt_amd.__all__
    assert hasattr(pyrayt_amd.RayTracer, "trace_tolerance") and hasattr(pyrayt_amd.Sensitivity, "tolerance")
    stub = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "prt_frame_tolerance_moments" in stub and "prt_frame_tolerance_workspace_bytes" in stub


def test_library_checks_tolerance_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    assert lib.prt_frame_tolerance_workspace_bytes(1000, 2, 20, 3, 65536) >= 1000 * (22 * 8 + 8 + 4)
    assert lib.prt_frame_tolerance_moments_workspace_bytes(10 ** 6, 2, 20, 3) >= (10 ** 6 // 2048) * 253 * 8
    for args in ((1000, 2, 0, 3, 10), (1000, 2, 21, 3, 10), (1000, 2, 4, 0, 10), (1000, 2, 4, 17, 10), (1000, 0, 4, 1, 10),
                 (-1, 1, 4, 1, 10), (1000, 16384, 4, 1, 10), (1000, 2, 4, 3, 0), (1000, 2, 4, 3, 65537)):
        assert lib.prt_frame_tolerance_workspace_bytes(*args) == -1, args
        if args[4] == 10:
            assert lib.prt_frame_tolerance_moments_workspace_bytes(*args[:4]) == -1, args
    buf = np.zeros(64)
    p = buf.ctypes.data
    lam = np.array([0.55, 0.65])
    first = np.array([0, 4], dtype=np.int64)

    def call(entry, wavelengths=lam, n_w=2, unit=1000.0, weight=1, n_groups=1, C=2, first=first, n_selected=4, n_rows=4,
             columns=p, out=p, trials=p, M=3, work=p):
        head = (0, p, 4, n_rows, p, n_selected, first.ctypes.data, n_groups, weight, p, columns, C, wavelengths.ctypes.data,
                n_w, unit)
        if entry == "tolerance":
            return lib.prt_frame_tolerance(*head, trials, M, out, p, p, work, None)
        return lib.prt_frame_tolerance_moments(*head, out, work, None)

    shared = ((dict(C=0), "1 to 20 columns"),
              (dict(C=21), "1 to 20 columns"),
              (dict(columns=None), "selected, opd and columns"),
              (dict(out=None), "bad buffers"),
              (dict(work=None), "bad buffers"),
              (dict(n_selected=5, first=np.array([0, 5], dtype=np.int64)), "more selected rows than rows"),
              (dict(first=np.array([0, 3], dtype=np.int64)), "group_first runs from 0 to n_selected"),
              (dict(n_groups=2, first=np.array([0, 5, 4], dtype=np.int64)), "group_first does not decrease"),
              (dict(weight=15), "weight_column"),
              (dict(n_w=17, wavelengths=np.arange(1.0, 18.0)), "1 to 16 distinct wavelengths"),
              (dict(wavelengths=np.array([0.55, 0.55])), "wavelengths: distinct"),
              (dict(wavelengths=np.array([0.55, -1.0])), "wavelengths: finite and > 0"),
              (dict(unit=0.0), "world_unit_um"),
              (dict(n_groups=8192, first=np.concatenate([np.zeros(8192), [4]]).astype(np.int64)), "<= 16383"))
    for entry in ("tolerance", "moments"):
        for kwargs, message in shared:
            assert call(entry, **kwargs) == -1, (entry, kwargs)
            assert message in lib.prt_last_error().decode(), (entry, kwargs, lib.prt_last_error())
            assert lib.prt_last_error().decode().startswith(("tolerance", "weight_column", "world_unit_um", "wavelengths")), entry
    for kwargs, message in ((dict(M=0), "1 to 65536 trials"), (dict(M=65537), "1 to 65536 trials"),
                            (dict(trials=None), "bad buffers")):
        assert call("tolerance", **kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())


def test_the_sum_kernel_uses_no_scratch_and_has_the_resources_design_md_states():
    """Every k_tol_sum instantiation keeps its trials' coefficients and accumulators in registers: no private segment, no
    spills; its VGPR count and LDS bytes are the ones of DESIGN.md's table, and the waves per SIMD stated there follow
    from the VGPR count (the allocation granule is 8 registers, 512 per SIMD lane, 8 waves at most)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from pyrayt_amd import engine

    if not os.path.exists(mod.READELF):
        pytest.skip("llvm-readelf not available")
    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    kernels = {name: res for name, res in mod.kernel_resources(engine.LIB_PATH).items() if "k_tol_sum" in name}
    assert len(kernels) == 5, sorted(kernels)
    stated = {int(cp): (int(v), int(lds), int(waves)) for cp, v, lds, waves in
              re.findall(r"\| `k_tol_sum<(\d+)>` \| (\d+) \| (\d+) \| (\d+) \|", open(os.path.join(ROOT, "DESIGN.md")).read())}
    assert sorted(stated) == [4, 8, 12, 16, 20], stated
    for name, res in kernels.items():
        cp = int(re.search(r"k_tol_sumILi(\d+)E", name).group(1))
        assert res["private_segment_fixed_size"] == 0, (name, res)
        assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0, (name, res)
        assert res["group_segment_fixed_size"] == T.K.kTolRays * (cp + 2) * 8 == stated[cp][1], (name, res, stated[cp])
        assert res["vgpr_count"] == stated[cp][0], (name, res, stated[cp])
        assert min(8, 512 // (-(-res["vgpr_count"] // 8) * 8)) == stated[cp][2], (name, res, stated[cp])


# ---- the spot radius of a trial -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centred", (True, False), ids=("about_the_centroid", "about_a_fixed_point"))
def test_rms_radius_is_the_rms_radius_of_the_jacobian_moved_landing_points(centred):
    """``Sensitivity.rms_radius_at`` (what ``ToleranceRun.rms_radius`` is) from sums built as include/prt.h lays them
    out, against the weighted RMS radius of the points x + sum_k J_k p_k themselves: about their own centroid, or about
    the fixed pivot."""
    from pyrayt_amd.frame import Sensitivity

    rng = np.random.default_rng(31)
    n, K = 200, 3
    x = rng.normal(0.0, 0.05, (n, 3)) + np.array([1.0, 0.2, -0.1])
    jac = rng.normal(0.0, 1.0, (K, 3, n))
    w = rng.uniform(0.5, 1.5, n)
    pivot = np.array([1.0, 0.19, -0.08])
    tri = np.tril_indices(K)
    sums = np.concatenate([[n, w.sum()], x.T @ w, [(w * ((x - pivot) ** 2).sum(axis=1)).sum()], (jac * w).sum(axis=2).ravel(),
                           np.einsum("n,nc,kcn->k", w, x - pivot, jac), np.einsum("n,jcn,kcn->jk", w, jac, jac)[tri]])
    sens = Sensitivity(None, None, sums[None], pivot[None], centred, (0, 0, 0, 0), ["a", "b", "c"])
    trials = rng.normal(0.0, 0.02, (1, 6, K))
    trials[0, 0] = 0.0
    got = sens.rms_radius_at(trials)
    for m in range(6):
        moved = x + np.einsum("kcn,k->nc", jac, trials[0, m])
        about = (moved * w[:, None]).sum(axis=0) / w.sum() if centred else pivot
        want = np.sqrt((w * ((moved - about) ** 2).sum(axis=1)).sum() / w.sum())
        assert got[0, m] == pytest.approx(want, rel=1e-11), (m, got[0, m], want)
    assert got[0, 0] == pytest.approx(np.sqrt(sens.mean_square[0]), rel=1e-14) and got[0, 1:].std() > 1e-3


# ---- end to end on the CPU: the reference and the linear ray model against the oracle's re-traces -------------------------------
E2E_UNIT = {"singlet": 1000.0, "two_fields": 1000.0, "dish_axial": 1e6}  # (micrometres per world unit, as the GPU tests take them)


def e2e_setup(name, n=257):
    """The scene's rows by group, their fixed spheres, and the reference's inputs from the CPU wavefront sensitivities
    (tests/opd_sensitivity_reference.py): OPD and dopd of the nominal frame."""
    import design_reference as dref
    import opd_scenes
    import opd_sensitivity_reference as oref
    from pyrayt_amd.scene import SceneSnapshot

    case = opd_scenes.build(name, n)
    tangents = oref.trace(case.frame, dref.table_of(SceneSnapshot(case.parts).prims), [dref.parameter(m) for m in case.parameters])
    assert not any(tangents["count"][key] for key in ("n_unknown", "n_invalid", "n_unfit"))
    at = np.flatnonzero(case.frame[:, 5] == case.surface.get_id())
    per = getattr(case, "rays_per_source", None)
    groups = [at[case.frame[at, 4] // per == g] for g in range(2)] if per else [at]
    balls = [oref.default_sphere(case.frame, rows) for rows in groups]
    waves = [oref.wavefront(case.frame, rows, tangents, ball) for rows, ball in zip(groups, balls)]
    assert all(np.all(wave["met"]) and np.all(wave["followed"]) for wave in waves)
    rows = np.concatenate(groups)
    group = np.concatenate([np.full(len(r), g) for g, r in enumerate(groups)])
    return case, groups, balls, rows, group, waves


def e2e_inputs(frame, rows, group, opd, columns, unit, n_groups):
    return T.tolerance_inputs(group, frame[rows, 2], np.asarray(opd, dtype=np.float64), frame[rows, 1],
                              np.asarray(columns, dtype=np.float64), np.unique(frame[rows, 2]), unit, n_groups)


@pytest.mark.parametrize("name", ("singlet", "two_fields", "dish_axial"))
def test_reference_end_to_end_the_error_of_the_linear_ray_model_is_of_second_order(name):
    """The check the GPU test of the same name repeats on the device, here with the longdouble reference alone: 4 trials
    with every parameter that can be applied to a built system non-zero at once (an IndexChange cannot and stays 0: the
    fifth parameter of singlet and two_fields; no other parameter had to be left out, no trial loses or gains a ray),
    against the Strehl ratio of the C oracle's re-trace of each perturbed system -- its OPD against the nominal
    system's sphere, held (``opd_of``), through ``tolerance_reference`` at a zero trial.  e(h) = max |linear model -
    oracle| over the trials scaled by h: e(h/2) <= e(h) / 3 and e(h) >= 10 x the device's bound.  h from the
    sensitivities alone: every parameter scaled by the spread of its dopd, four sign patterns, the largest phase
    change of a ray about its group's mean 0.4 rad (between 0.25 and 0.5)."""
    import opd_sensitivity_reference as oref
    import tolerance_scenes

    case, groups, balls, rows, group, waves = e2e_setup(name)
    G, unit = len(groups), E2E_UNIT[name]
    lam = float(np.unique(case.frame[rows, 2])[0])
    s = unit / lam
    opd = np.concatenate([wave["opd"] for wave in waves]).astype(np.float64)
    dopd = np.concatenate([wave["dopd"] for wave in waves], axis=1).astype(np.float64)
    K, live = len(case.parameters), tolerance_scenes.applicable(case.parameters)
    assert len(live) >= 2 and len(live) == K - (name != "dish_axial")

    def spread(x):
        return max(np.abs(x[group == g] - x[group == g].mean()).max() for g in range(G))

    signs = np.random.default_rng(11).choice([-1.0, 1.0], (4, len(live)))
    direction = np.zeros((4, K))
    direction[:, live] = signs / np.array([spread(dopd[k]) for k in live])
    h = 0.4 / (2 * np.pi * s * max(spread(direction[m] @ dopd) for m in range(4)))
    linear = e2e_inputs(case.frame, rows, group, opd, dopd, unit, G)

    def error(scale):
        trials = direction * (h * scale)
        model = T.tolerance_reference(linear, np.broadcast_to(trials[None], (G, 4, K)))
        want = np.empty((G, 4), dtype=LD)
        for m in range(4):
            moved = tolerance_scenes.build(name, 257, trials[m])
            assert moved.counts == case.counts and np.array_equal(moved.frame[:, 4], case.frame[:, 4]), f"trial {m}: rays lost or gained"
            traced = np.concatenate([oref.opd_of(moved.frame, r, ball)[0] for r, ball in zip(groups, balls)]).astype(np.float64)
            exact = e2e_inputs(moved.frame, rows, group, traced, np.zeros((1, len(rows))), unit, G)
            want[:, m] = T.tolerance_reference(exact, np.zeros((G, 1, 1))).strehl[:, 0]
        return float(np.abs(model.strehl - want).max()), float(model.strehl_bound.max())

    (e1, bound), (e2, _) = error(1.0), error(0.5)
    print(f"[tolerance] {name} on the CPU: e(h) {e1:.3e}, e(h/2) {e2:.3e} (ratio {e2 / e1:.3f}), device bound {bound:.3e}")
    assert e1 >= 10 * bound, (name, e1, bound)
    assert e2 <= e1 / 3, (name, e1, e2)
