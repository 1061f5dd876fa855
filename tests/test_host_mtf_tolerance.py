"""The longdouble reference of the MTF tolerancing pass (tests/mtf_tolerance_reference.py) against closed forms and against
central differences held to mtf_gradient_reference's dOTF; the Python copies of the partition rules against the header's
text; what ``mtf_tolerance`` and the entry point refuse without a GPU; what ``MTFToleranceRun`` reads; the code objects of
k_mtft_sum and k_mtft_moments; and, on the CPU, the end-to-end check the GPU test of the same name repeats."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import diffraction_reference as R
import mtf_gradient_reference as G
import mtf_tolerance_reference as T

LD = np.longdouble
ROOT = R.ROOT
FREQUENCIES, AZIMUTHS, FOCUS = (0.0, 3.0, 30.0, 100.0), (0.0, 90.0, 33.0), (0.0, 0.05, -0.03)


def size(re, im):
    return np.hypot(re, im).astype(float)


# ---- closed forms -----------------------------------------------------------------------------------------------------------
def focus_case(seed=6):
    """Two parameters on gradient_case's rays: column 0 with dQ = -a and duh = 0, that is dp = s and ds = 0, a pure focus
    shift; column 1 with dQ = (0, 0.7, -0.4) and duh = 0, a pure translation across the axis."""
    case = T.tolerance_case([150, 90], 2, seed=seed)
    n = len(case.rows)
    moves = np.array([[-1.0, 0.0, 0.0], [0.0, 0.7, -0.4]])
    case.jacobian = np.repeat(moves[:, :, None], n, axis=2)
    case.slopes = np.zeros_like(case.jacobian)
    return case


def test_a_focus_column_is_a_plane_shift_and_the_compensator_takes_it_back():
    case = focus_case()
    centre = np.array([[1e-4, -2e-4, 3e-4]] * 2)
    shifts = np.array([0.02, -0.035, 0.0])
    trials = np.zeros((3, 2))
    trials[:, 0] = shifts
    ref = T.reference_of(case, trials, FREQUENCIES, AZIMUTHS, (0.0,), centre=centre)
    planes = T.reference_of(case, np.zeros((1, 2)), FREQUENCIES, AZIMUTHS, shifts, centre=centre)
    # trial t at plane 0 is the zero trial at plane t
    assert size(ref.re[:, :, 0] - planes.re[:, 0], ref.im[:, :, 0] - planes.im[:, 0]).max() <= 1e-15
    # delta* of a trial is the nominal's less its shift, so with ("focus",) every trial has the nominal's compensated OTF
    fit = T.reference_of(case, trials, FREQUENCIES, AZIMUTHS, FOCUS, centre=centre, compensate=True)
    assert np.abs((fit.best_focus - (fit.best_focus[:, 2:3] - shifts.astype(LD))).astype(float)).max() <= 1e-15
    assert np.all(fit.focus_shift == fit.best_focus)
    assert size(fit.re - fit.re[:, 2:3], fit.im - fit.im[:, 2:3]).max() <= 1e-14
    # and the compensated plane is the one of least RMS radius: the quadratic of the moments has its minimum there
    m = fit.moments[:, 2]
    var = lambda d: ((m[:, 5] + 2 * d * m[:, 6] + d * d * m[:, 7]) / m[:, 0]  # noqa: E731
                     - (((m[:, 1:3] + d[:, None] * m[:, 3:5]) / m[:, 0, None]) ** 2).sum(axis=1))
    best = fit.best_focus[:, 2]
    assert np.all(var(best) < var(best + LD(1e-3))) and np.all(var(best) < var(best - LD(1e-3)))


def test_a_translation_changes_no_mtf_and_moves_the_ptf_under_fixed_only():
    from pyrayt_amd.frame import MTFToleranceRun

    case = focus_case()
    trials = np.zeros((3, 2))
    trials[:2, 1] = 0.01, -0.004
    ref = T.reference_of(case, trials, FREQUENCIES, AZIMUTHS, FOCUS)
    kc, ks = (x.astype(LD) for x in R.frequency_table(FREQUENCIES, AZIMUTHS))
    for m in range(2):
        ramp = -R.TWO_PI * LD(trials[m, 1]) * (kc * LD(0.7) + ks * LD(-0.4))  # (OTF_m = exp(i ramp) OTF_0)
        c, s = np.cos(ramp), np.sin(ramp)
        want_re, want_im = c * ref.re[:, 2] - s * ref.im[:, 2], s * ref.re[:, 2] + c * ref.im[:, 2]
        assert size(ref.re[:, m] - want_re, ref.im[:, m] - want_im).max() <= 1e-15
    followed = T.about_centroid(ref, FREQUENCIES, AZIMUTHS, FOCUS)
    assert np.abs(followed - followed[:, 2:3]).max() <= 1e-13
    assert np.abs(np.abs(ref.otf) - np.abs(ref.otf[:, 2:3])).max() <= 1e-14
    # MTFToleranceRun composes the same on the same numbers
    record = np.concatenate([ref.centre.astype(float), ref.sum_weights.astype(float)[:, None], ref.n_rays[:, None],
                             ref.n_missed[:, None], ref.n_unfollowed[:, None]], axis=1)
    for reference in ("fixed", "centroid"):
        run = MTFToleranceRun(trials, ref.otf, ref.moments.astype(float), ref.focus_shift.astype(float), record,
                              FREQUENCIES, AZIMUTHS, FOCUS, ("focus", "shift"), (), reference)
        assert run.otf.shape == (2, 2, 3, 3, 4) and run.nominal.otf.shape == (2, 3, 3, 4)
        want = ref.otf if reference == "fixed" else followed
        assert np.abs(run.otf - want[:, :2]).max() <= 1e-12 and np.abs(run.nominal.otf - want[:, 2]).max() <= 1e-12
        assert np.abs(run.mtf - run.nominal.mtf[:, None]).max() <= 1e-12
    assert np.abs(run.centroid - run.nominal.centroid[:, None]
                  - trials[None, :2, 1, None] * np.array([0.7, -0.4])).max() <= 1e-15
    assert np.abs(run.rms_radius - run.nominal.rms_radius[:, None]).max() <= 1e-13


def test_rms_radius_centroid_and_best_focus_are_the_sample_statistics_of_the_moved_points():
    from pyrayt_amd.frame import MTFToleranceRun

    case = T.tolerance_case([130], 3, seed=12)
    trials = np.vstack([T.random_trials(4, 3, 5e-3), np.zeros((1, 3))])
    ref = T.reference_of(case, trials, (10.0,), (0.0,), FOCUS, compensate=True)
    record = np.array([[0.0, 0.0, 0.0, float(ref.sum_weights[0]), 130, 0, 0]])
    run = MTFToleranceRun(trials, ref.otf, ref.moments.astype(float), ref.focus_shift.astype(float), record, (10.0,),
                          (0.0,), FOCUS, "abc", ("focus",))
    rays, _ = T.staged_of(case)
    centroid, radius = T.sample_statistics(rays[0], trials, ref.focus_shift[0], FOCUS)
    whole = np.concatenate([run.rms_radius, run.nominal.rms_radius[:, None]], axis=1)
    assert np.abs(whole[0] - radius.astype(float)).max() <= 1e-12 * radius.astype(float).max()
    assert np.abs(run.centroid_at(1)[0] - centroid[:, 1].astype(float)).max() <= 1e-15
    assert np.abs(run.best_focus[0] - ref.best_focus[0, :-1].astype(float)).max() <= 1e-14
    # the compensated plane is the best one: no plane of the trial has a smaller radius
    assert np.all(whole[0, :, 0] <= whole[0, :, 1]) and np.all(whole[0, :, 0] <= whole[0, :, 2])


# ---- central differences ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", ([300], [40, 0, 170]), ids=("one_group", "three_groups_one_empty"))
def test_one_hot_trials_follow_the_gradient_references_dotf(counts):
    """D(h) = (OTF(+h e_k) - OTF(-h e_k)) / (2 h) of this reference against dOTF_k of mtf_gradient_reference, about the same
    held centre: |dOTF - D(h/2)| <= |D(h) - D(h/2)|, the gap at most 1 % of the largest |dOTF|, and Richardson's
    (4 D(h/2) - D(h)) / 3 ten times closer."""
    n_par, h = 3, 1e-4  # (dQ of order 1, duh of 0.3: 2 pi nu |dx| h <= 0.1 rad at nu = 100)
    case = T.tolerance_case(counts, n_par, seed=4)
    centre = np.array([[1e-4, -2e-4, 3e-4]] * len(counts))
    grad = G.reference_of(case, FREQUENCIES, AZIMUTHS, FOCUS, centre=centre)
    full = [g for g, c in enumerate(counts) if c]
    steps = np.concatenate([s * step * np.eye(n_par) for step in (h, h / 2) for s in (1, -1)])
    ref = T.reference_of(case, steps, FREQUENCIES, AZIMUTHS, FOCUS, centre=centre)
    assert np.all(np.isnan(ref.re[[g for g, c in enumerate(counts) if not c]].astype(float)))
    for k in range(n_par):
        D = [((ref.re[full, at + k] - ref.re[full, at + n_par + k]) / (2 * LD(step)),
              (ref.im[full, at + k] - ref.im[full, at + n_par + k]) / (2 * LD(step)))
             for at, step in ((0, h), (2 * n_par, h / 2))]
        dre, dim = grad.dre[full, k], grad.dim[full, k]
        gap, miss = size(D[0][0] - D[1][0], D[0][1] - D[1][1]), size(dre - D[1][0], dim - D[1][1])
        rich = size(dre - (4 * D[1][0] - D[0][0]) / 3, dim - (4 * D[1][1] - D[0][1]) / 3)
        scale = float(size(dre, dim).max())
        print(f"[mtf tolerance] parameter {k}: largest |dOTF| {scale:.3e}, gap {gap.max():.3e}, |ref - D(h/2)| "
              f"{miss.max():.3e}, Richardson {rich.max():.3e}")
        assert scale > 0 and np.all(miss <= gap) and gap.max() <= 0.01 * scale
        assert rich.max() <= 0.1 * gap.max()


def test_rays_left_out_a_zero_column_and_the_bounds():
    """Rays the MTF leaves out and rays that were not followed are counted and contribute nothing; a zero column changes
    nothing; the bound is of the order the number formats give (EPS_TRIG and a few thousand u of the phase)."""
    case = T.tolerance_case([90, 60], 3, left_out=3, unfollowed=2, seed=9)
    trials = T.random_trials(3, 3)
    ref = T.reference_of(case, trials, FREQUENCIES, AZIMUTHS, FOCUS)
    assert ref.n_rays.tolist() == [88, 58] and ref.n_missed.tolist() == [3, 3] and ref.n_unfollowed.tolist() == [2, 2]
    wide_j = np.concatenate([case.jacobian, np.ones_like(case.jacobian[:1])])
    wide_s = np.concatenate([case.slopes, np.zeros_like(case.slopes[:1])])
    wide = T.reference_of(case, np.hstack([trials, np.zeros((3, 1))]), FREQUENCIES, AZIMUTHS, FOCUS, jacobian=wide_j,
                          slopes=wide_s, centre=ref.centre.astype(float))
    # (longdouble sums of four terms for three: the order of einsum's additions may differ, 2^-64 of phases of 100 cycles)
    assert float(np.abs(wide.re - ref.re).max()) <= 1e-15 and float(np.abs(wide.moments - ref.moments).max()) <= 1e-15
    eps0 = R.EPS_TRIG + (2 * np.pi * R.F32_TURN) ** 2 / 2
    assert np.all(ref.otf_bound >= eps0) and ref.otf_bound.max() <= eps0 + 1e-10
    assert np.all(ref.moments_bound[..., 0] <= 450 * R.U64 * ref.moments[..., 0].astype(float))
    assert np.all(np.isfinite(ref.best_focus_bound)) and ref.best_focus_bound.max() <= 1e-9


# ---- the rules and the interface --------------------------------------------------------------------------------------------
def test_the_partition_rules_are_the_headers_own_lines():
    for name, lines in T.HOST_RULES.items():
        text = " ".join(open(os.path.join(ROOT, "pyrayt_amd", "csrc", name)).read().split())
        for line in lines:
            assert " ".join(line.split()) in text, (name, line)
    K = T.K
    assert (K.kMtftBlock, K.kMtftTrials, K.kMtftTile, K.kMtftOut, K.kMtftRays, K.kMtftColumnStep, K.kMtftSlicesPerCu) == (
        256, 1, 256, 8, 64, 4, 4)
    assert K.kMtftSlabBytes == K.kMtfSlabBytes == 256 << 20 and (K.kMtfMinSlice, K.kMtfMaxSlices) == (2048, 256)
    assert [T.slices(n, 1, 256) for n in (0, 1, 2048, 2049, 3 * 2048 + 1, 10 ** 6)] == [1, 1, 1, 2, 4, 256]
    assert T.max_slices(256, 1) == 256 and T.max_slices(256, 8) == 128 and T.max_slices(8, 3) == 11
    assert T.max_slices(1, 65535) == 1 and T.slices(10 ** 6, 8, 256) == 128
    # 1M rays in one group on 256 CUs, 256 slices: 8 outputs in launches of 5376 trials; 256 outputs do not fit beside a
    # tile of 256 trials (268 MB), so the outputs go in launches of 248; 65535 groups of a slice each are refused
    assert T.launches(256, 8, 10 ** 4) == (8, 5376) and T.launches(256, 256, 10 ** 4) == (248, 256)
    assert T.launches(256, 8, 33) == (8, 256) and T.launches(1, 3, 65536) == (8, 65536) and T.launches(65535, 8, 1) is None
    assert [T.template_columns(k) for k in (1, 4, 5, 8, 9, 12, 13, 16)] == [4, 4, 8, 8, 12, 12, 16, 16]
    assert {np.prod(o) for o in T.OUTPUT_COUNTS} == {1, 7, 8, 9, 30}
    assert T.k_t(6) == 34


def test_mtf_tolerance_needs_slopes_and_refuses_what_it_cannot_serve():
    from pyrayt_amd.frame import Sensitivity, Tolerances, WavelengthChange

    bare = Sensitivity(None, None, np.zeros((1, 11)), np.zeros((1, 3)), True, (0, 0, 0, 0), ["p"])
    with pytest.raises(ValueError, match=r"mtf_tolerance: .*slopes=True"):
        bare.mtf_tolerance(np.zeros((1, 1)), [10.0])
    plain = Sensitivity(None, None, np.zeros((1, 17)), np.zeros((1, 3)), True, (0, 0, 0, 0), ["a", WavelengthChange()])
    plain.slopes = SimpleNamespace()
    with pytest.raises(ValueError, match="reference"):
        plain.mtf_tolerance(np.zeros((1, 2)), [10.0], reference="moving")
    for compensators in (("tilt",), ("focus", "focus"), (0,), "tilt", ("focus", 1), 3):
        with pytest.raises(ValueError, match="compensators"):
            plain.mtf_tolerance(np.zeros((1, 2)), [10.0], compensators=compensators)
    for trials in (np.zeros((3, 1)), np.zeros(2), np.zeros((0, 2)), np.full((1, 2), np.nan), "many", np.zeros((65536, 2)),
                   (Tolerances([1.0]), 5)):
        with pytest.raises(ValueError, match="trials"):
            plain.mtf_tolerance(trials, [10.0], compensators=("focus",))
    with pytest.raises(ValueError, match="frequenc"):
        plain.mtf_tolerance(np.zeros((1, 2)), [-1.0])


def test_the_pass_calls_the_library_as_the_header_declares_it(monkeypatch):
    """tests/test_host_frame_calls.py's stand-in library (every argument checked against the binding's ctypes kinds)
    under ``mtf_tolerance``: one size call, then the entry with 27 arguments, the workspace and the stream -- on a frame
    with rows and on a selection of nothing, with the centroid and with a given centre.  The call is
    frame.py's own, and that file's golden record holds these three cases too."""
    torch = pytest.importorskip("torch")
    import pyrayt_amd.frame as F
    from pyrayt_amd.scene import MATERIAL_DTYPE, PRIM_DTYPE
    from test_host_frame_calls import make_frame, stand_ins

    assert torch is not None
    run = stand_ins(monkeypatch)
    system = SimpleNamespace(prims=np.zeros(2, dtype=PRIM_DTYPE), materials=np.zeros(1, dtype=MATERIAL_DTYPE))
    system.prims["surface_id"] = (1, 2)
    rigid = [F.Motion(1, translate=(1, 0, 0)), F.Motion(2, rotate=(0, 0, 1))]
    trials = np.array([[0.1, 0.0], [0.0, 0.1], [0.1, 0.1]])
    frame = make_frame()
    for surface, kw, more in ((2, dict(rays_per_source=4), dict(compensators=("focus",), centre=(0.0, 0.1, 0.0))),
                              (2, {}, {}), (7, {}, dict(reference="fixed"))):
        got = run(lambda: frame.sensitivity(surface, rigid, system, slopes=True, **kw).mtf_tolerance(
            trials, (0.0, 1.0, 2.0), azimuths=(0.0,), focus=(0.0, 0.1), **more))
        assert got["raised"] is None, got
        (size_name, size_args), (name, args) = got["calls"][-2:]
        assert size_name == "prt_frame_mtf_tolerance_workspace_bytes" and name == "prt_frame_mtf_tolerance"
        n_groups = 2 if kw else 1
        assert list(size_args[1:]) == [n_groups, 2, 3, 1, 2, 4] and len(args) == 29
        assert list(args[11:12]) == [2] and list(args[15:16]) == [3] and list(args[17:18]) == [1] and list(args[19:23]) == [
            2, "ptr", 4, int("compensators" in more)]
        assert args[12] == ("ptr" if "centre" in more else "NULL") and args[-1] == "NULL" and args[-2] == "ptr"


def run_of(strehl_like, trials, azimuths=(0.0, 90.0)):
    """An MTFToleranceRun whose MTF at (plane 0, azimuth a, frequency 0) is strehl_like[g, m] * (1 - 0.1 a)."""
    from pyrayt_amd.frame import MTFToleranceRun

    G_, M = strehl_like.shape
    otf = strehl_like[:, :, None, None, None] * (1 - 0.1 * np.arange(len(azimuths)))[None, None, None, :, None] * np.exp(0.3j)
    otf = np.broadcast_to(otf, (G_, M, 2, len(azimuths), 1)).copy()
    otf[:, :, 1] *= 0.5
    moments = np.zeros((G_, M, 8))
    moments[..., 0], moments[..., 5], moments[..., 7] = 2.0, 8.0, 2.0
    moments[1] = np.nan
    record = np.array([[0, 0, 0, 2.0, 2, 0, 0], [np.nan, np.nan, np.nan, 0, 0, 1, 1]])
    return MTFToleranceRun(trials, otf, moments, np.zeros((G_, M)), record, (25.0,), azimuths, (0.0, 1.0), ("a", "b"))


def test_mtf_tolerance_run_reads_its_arrays():
    from pyrayt_amd.frame import Tolerances

    tol = Tolerances([0.1, 0.2])
    trials = np.vstack([tol.sensitivity_table(), np.zeros((1, 2))])  # (the nominal trial last, as mtf_tolerance() adds it)
    M = len(trials)
    merit = np.vstack([np.array([0.9, 0.5, 0.85, 0.88, 0.7, 0.9]), np.full(M, np.nan)])
    run = run_of(merit, trials)
    assert run.trials.shape == (5, 2) and run.mtf.shape == (2, 5, 2, 2, 1) and run.nominal.mtf[0, 0, 0, 0] == pytest.approx(0.9)
    assert run.n_rays.tolist() == [2, 0] and run.n_unfollowed.tolist() == [0, 1] and run.n_trials == 5
    assert run.yield_(0.8, azimuth=0).tolist()[0] == 3 / 5 and np.isnan(run.yield_(0.8)[1])
    assert run.yield_(0.8)[0] == 1 / 5  # (azimuth 1 is 0.9 of azimuth 0: 0.81, 0.765, 0.792 -- every output must pass)
    assert run.yield_(0.3, plane=1, frequency=0, azimuth=[0])[0] == 4 / 5
    assert run.percentiles((0, 100), frequency=0, azimuth=0)[0].tolist() == pytest.approx([0.5, 0.9])
    assert run.rms_radius[0, 0].tolist() == pytest.approx([2.0, np.sqrt(5.0)]) and np.all(np.isnan(run.rms_radius[1]))
    assert run.best_focus[0].tolist() == [0.0] * 5 and run.centroid.shape == (2, 5, 2)
    frame = run.to_pandas()
    assert list(frame.columns) == ["source_id", "trial", "focus_shift", "best_focus", "rms_radius_0", "rms_radius_1",
                                   "mtf_0_0_0", "mtf_0_1_0", "mtf_1_0_0", "mtf_1_1_0", "p_0", "p_1"] and len(frame) == 10
    table = run.table()
    assert table["parameter"].tolist() == [0, 1] and table["worst"].tolist() == pytest.approx([-0.4, -0.2])
    assert table["dmtf_plus"].tolist() == pytest.approx([-0.05, -0.2]) and table["width"].tolist() == [0.1, 0.2]
    assert run.table(plane=1)["worst"].tolist() == pytest.approx([-0.2, -0.1])
    other = run_of(merit[:, :4], np.ones((4, 2)))
    with pytest.raises(ValueError, match="sensitivity_table"):
        other.table()


def test_abi_entries_are_declared_and_the_version_stays():
    import pyrayt_amd
    from pyrayt_amd import engine

    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("prt_frame_mtf_tolerance_workspace_bytes", "prt_frame_mtf_tolerance"):
        assert name in engine.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", text), name
    found = re.search(r"#define PRT_VERSION (\d+) /\*(.*?)\*/", header, flags=re.S)
    assert int(found.group(1)) == 240 and "prt_frame_mtf_tolerance" in found.group(2)
    assert pyrayt_amd.MTFToleranceRun is pyrayt_amd.frame.MTFToleranceRun and "MTFToleranceRun" in pyrayt_amd.__all__
    assert hasattr(pyrayt_amd.RayTracer, "trace_mtf_tolerance") and hasattr(pyrayt_amd.Sensitivity, "mtf_tolerance")
    # the model goes word for word into the header
    for line in ("P_rm = p_r + sum_k t_mk dp_rk", "S_rm = s_r + sum_k t_mk ds_rk",
                 "OTF_gm = sum w exp(-2 pi i k.(P_rm + (delta_f + delta_m) S_rm)) / sum w",
                 "the least-squares focus is delta*_m = -cov_PS / var_S (0 where var_S is not > 0)"):
        assert line in header, line


def test_library_checks_mtf_tolerance_arguments_without_a_gpu():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    assert lib.prt_frame_mtf_tolerance_workspace_bytes(1000, 2, 16, 128, 2, 1, 1000) >= 1000 * (48 + 16 * 32) + 256 * 32
    for args in ((1000, 2, 0, 128, 2, 1, 10), (1000, 2, 17, 128, 2, 1, 10), (1000, 2, 4, 4097, 2, 1, 10),
                 (1000, 2, 4, 128, 17, 1, 10), (1000, 2, 4, 128, 2, 257, 10), (1000, 0, 4, 128, 2, 1, 10),
                 (-1, 1, 4, 128, 2, 1, 10), (1000, 65536, 4, 128, 2, 1, 10), (1000, 2, 4, 128, 2, 1, 0),
                 (1000, 2, 4, 128, 2, 1, 65537)):
        assert lib.prt_frame_mtf_tolerance_workspace_bytes(*args) == -1, args
    buf = np.zeros(64)
    p = buf.ctypes.data
    axes = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
    nu, theta, focus = np.array([0.0, 10.0]), np.array([0.0, 90.0]), np.array([0.0])
    first = np.array([0, 4], dtype=np.int64)

    def call(frequencies=nu, n_f=2, azimuths=theta, n_a=2, planes=focus, n_p=1, weight=1, n_groups=1, axes=axes, K=2,
             first=first, n_selected=4, n_rows=4, jacobian=p, out=p, trials=p, M=3, moments=p):
        return lib.prt_frame_mtf_tolerance(0, p, 4, n_rows, p, n_selected, first.ctypes.data, n_groups, weight, jacobian, p,
                                           K, None, axes.ctypes.data, frequencies.ctypes.data, n_f, azimuths.ctypes.data,
                                           n_a, planes.ctypes.data, n_p, trials, M, 0, out, moments, p, p, p, None)

    for kwargs, message in ((dict(frequencies=np.array([-1.0, 1.0])), "frequencies finite and >= 0"),
                            (dict(n_a=17, azimuths=np.zeros(17)), "1 to 16 azimuths"),
                            (dict(planes=np.array([np.nan])), "focus shifts finite"),
                            (dict(weight=15), "weight_column"),
                            (dict(axes=np.full(9, np.nan)), "axes: finite"),
                            (dict(K=0), "1 to 16 parameters"),
                            (dict(K=17), "1 to 16 parameters"),
                            (dict(M=0), "1 to 65536 trials"),
                            (dict(M=65537), "1 to 65536 trials"),
                            (dict(trials=None), "bad buffers"),
                            (dict(moments=None), "bad buffers"),
                            (dict(jacobian=None), "jacobian and slopes"),
                            (dict(out=None), "bad buffers"),
                            (dict(n_selected=5, first=np.array([0, 5], dtype=np.int64)), "more selected rows than rows"),
                            (dict(first=np.array([0, 3], dtype=np.int64)), "group_first runs from 0 to n_selected"),
                            (dict(n_groups=2, first=np.array([0, 5, 4], dtype=np.int64)), "group_first does not decrease"),
                            # 8192 groups, a slice each at the least: 8192 * 256 trials * (8 outputs * 16 + 64) bytes
                            (dict(n_groups=8192, first=np.concatenate([np.zeros(8192), [4]]).astype(np.int64)),
                             "256 MiB slab cap")):
        assert call(**kwargs) == -1, kwargs
        assert message in lib.prt_last_error().decode(), (kwargs, lib.prt_last_error())
        assert lib.prt_last_error().decode().startswith(("mtf_tolerance", "weight_column", "axes")), lib.prt_last_error()


def test_the_kernels_use_no_scratch_and_have_the_resources_design_md_states():
    """Every k_mtft_sum and k_mtft_moments instantiation keeps its trial's coefficients and accumulators in registers: no
    private segment, no spills; its VGPR count and LDS bytes are the ones of DESIGN.md's table, and the waves per SIMD
    stated there follow from the VGPR count (the allocation granule is 8 registers, 512 per SIMD lane, 8 waves at most)."""
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
    for kernel, extra in (("k_mtft_sum", T.K.kMtftOut * 16), ("k_mtft_moments", 0)):
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
E2E_FREQUENCIES, E2E_AZIMUTHS, E2E_PLANES = (0.4, 0.8, 1.2), (0.0, 90.0), (0.0, 0.5)
E2E_SCENES = ("singlet", "two_fields")


def e2e_setup(name, n=257):
    """The scene's selected rows in the pass's order with their groups, and jacobian and slopes (K, 3, n_selected) from
    the CPU tangents (tests/opd_sensitivity_reference.py)."""
    import design_reference as dref
    import opd_scenes
    import opd_sensitivity_reference as oref
    from pyrayt_amd.scene import SceneSnapshot

    case = opd_scenes.build(name, n)
    tangents = oref.trace(case.frame, dref.table_of(SceneSnapshot(case.parts).prims), [dref.parameter(m) for m in case.parameters])
    assert not any(tangents["count"][key] for key in ("n_unknown", "n_invalid", "n_unfit"))
    per = getattr(case, "rays_per_source", None)
    n_groups = 2 if per else 1
    rows, group = G.selection(case.frame, case.surface.get_id(), per, n_groups)
    jacobian = np.asarray(tangents["dx"][:, rows], dtype=np.float64).transpose(0, 2, 1)
    slopes = np.asarray(tangents["dd"][:, rows], dtype=np.float64).transpose(0, 2, 1)
    assert np.all(np.isfinite(jacobian)) and np.all(np.isfinite(slopes))
    return case, rows, group, n_groups, jacobian, slopes


def e2e_trials(dp, group, n_groups, live, n_parameters, top):
    """4 sign patterns with every applicable parameter moved at once, from the sensitivities alone.  ``dp`` (K, 2, n): the
    staged derivative of the landing points.  A parameter is moved in proportion to its own effect on the spot -- the
    spread of its dp about the group's mean, relative to the largest --, since the MTF of these blurs is so insensitive to
    the weakest (the front radius) that equal effects would ask for a radius changed by its own size; then h sets the
    largest 2 pi |k.dx| about the group's mean, over the patterns and both axes, to 0.4 rad at the top frequency."""
    def spread(x):
        return max(np.abs(x[group == g] - x[group == g].mean()).max() for g in range(n_groups))

    own = np.array([max(spread(dp[k, 0]), spread(dp[k, 1])) for k in live])
    direction = np.zeros((4, n_parameters))
    direction[:, live] = np.random.default_rng(11).choice([-1.0, 1.0], (4, len(live))) * own / own.max()
    h = 0.4 / (2 * np.pi * top * max(spread(direction[m] @ dp[:, c]) for m in range(4) for c in range(2)))
    return direction, h


def retraced_mtf(name, case, rows, group, n_groups, trial):
    """|OTF| of the C oracle's re-trace of the perturbed system, from the MTF's own reference; the counts must be those of
    the nominal system, or the trial is a failure of the test's inputs."""
    import tolerance_scenes

    moved = tolerance_scenes.build(name, 257, trial)
    assert moved.counts == case.counts and np.array_equal(moved.frame[:, 4], case.frame[:, 4]), "rays lost or gained"
    f = moved.frame
    want = R.mtf_reference(f[rows, 9:12], f[rows, 12:15], f[rows, 1], group, n_groups, E2E_FREQUENCIES, E2E_AZIMUTHS,
                           E2E_PLANES)
    return want, np.hypot(want.re, want.im)


@pytest.mark.parametrize("name", E2E_SCENES)
def test_reference_end_to_end_the_error_of_the_linear_ray_model_is_of_second_order(name):
    """The check the GPU test of the same name repeats on the device, here with the longdouble reference alone: 4 trials
    with every parameter that can be applied to a built system non-zero at once (an IndexChange cannot and stays 0), no
    compensator, the planes 0 and 0.5, against |OTF| of the C oracle's re-trace of each perturbed system
    (diffraction_reference.mtf_reference of its rows; no trial loses or gains a ray).  Frequencies 0.4, 0.8 and 1.2 cycles
    per world unit at azimuths 0 and 90: the nominal MTF at 1.2 is 0.71 to 0.73 (singlet) and 0.73 to 0.79 (two_fields) in
    plane 0, between 0.2 and 0.9 as asked.  e(h) = max | |OTF| of the linear model - |OTF| of the oracle | over the trials
    scaled by h: e(h/2) <= e(h) / 3 and e(h) >= 10 x the device's bound; h from the sensitivities alone (``e2e_trials``).
    Measured here: singlet e(h) 7.0e-2, e(h/2) 2.0e-2 (ratio 0.29); two_fields 6.6e-2, 2.1e-2 (0.31); the bound 3.0e-7.
    dish_axial is left out: its image is stigmatic (a parabola on its axis: spot radius 4e-19), so its MTF is 1 at every
    frequency in plane 0 and no frequency puts the nominal MTF between 0.2 and 0.9; the trial h asks for there moves
    the mirror by 53 units and loses rays.  ``mtf + dmtf . t`` is printed beside it, not asserted."""
    import tolerance_scenes

    case, rows, group, n_groups, jacobian, slopes = e2e_setup(name)
    f = case.frame
    q, u, w = f[rows, 9:12], f[rows, 12:15], f[rows, 1]
    n_par, live = len(case.parameters), tolerance_scenes.applicable(case.parameters)
    assert len(live) == n_par - 1 >= 2
    rays, _ = T.staged(q, u, w, group, n_groups, jacobian, slopes)
    dp = np.concatenate([ray.dp.astype(float) for ray in rays], axis=2)
    direction, h = e2e_trials(dp, group, n_groups, live, n_par, E2E_FREQUENCIES[-1])
    nominal = R.mtf_reference(q, u, w, group, n_groups, E2E_FREQUENCIES, E2E_AZIMUTHS, E2E_PLANES)
    top = np.hypot(nominal.re, nominal.im)[:, 0, :, -1].astype(float)
    assert np.all((top >= 0.2) & (top <= 0.9)), top
    grad = G.gradient_reference(q, u, w, group, n_groups, jacobian, slopes, E2E_FREQUENCIES, E2E_AZIMUTHS, E2E_PLANES)
    mtf0 = np.hypot(grad.re, grad.im)
    dmtf = (grad.re[:, None] * grad.dre[:, :n_par] + grad.im[:, None] * grad.dim[:, :n_par]) / mtf0[:, None]

    def error(scale):
        trials = direction * (h * scale)
        model = T.tolerance_reference(q, u, w, group, n_groups, jacobian, slopes, trials, E2E_FREQUENCIES, E2E_AZIMUTHS,
                                      E2E_PLANES)
        worst = first_order = 0.0
        for m in range(4):
            want, size_ = retraced_mtf(name, case, rows, group, n_groups, trials[m])
            assert np.array_equal(want.n_rays, model.n_rays)
            worst = max(worst, float(np.abs(np.hypot(model.re[:, m], model.im[:, m]) - size_).max()))
            linear = mtf0 + np.einsum("k,gkfan->gfan", trials[m].astype(LD), dmtf)
            first_order = max(first_order, float(np.abs(linear - size_).max()))
        return worst, float(model.otf_bound.max()), first_order

    (e1, bound, l1), (e2, _, l2) = error(1.0), error(0.5)
    print(f"[mtf tolerance] {name} on the CPU: h {h:.4f}, e(h) {e1:.3e}, e(h/2) {e2:.3e} (ratio {e2 / e1:.3f}), device "
          f"bound {bound:.3e}; mtf + dmtf . t misses by {l1:.3e} and {l2:.3e}")
    assert e1 >= 10 * bound, (name, e1, bound)
    assert e2 <= e1 / 3, (name, e1, e2)
