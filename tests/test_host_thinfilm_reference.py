"""The extended-precision reference of a layer stack (tests/thinfilm_reference.py) on the CPU: against the two complex128
restatements of tests/coating_reference.py where those are well behaved, against a 60-digit evaluation of the
characteristic matrices (another formulation than the reference's) in every regime the device is held to it, against
closed forms of its own, and the caps on its margin that keep the margin from hiding a failure of the device."""
import numpy as np
import pytest

import coating_reference as cr
import thinfilm_reference as tf

LD = tf.LD
SMALL = [name for name in tf.CASES if "rays" not in name]  # (one frame of every regime; the two large ladders repeat one)


def all_four(arguments):
    ni, cos_i, sin2, far, layers, lam, _ = arguments
    return tf.stack_coefficients(float(ni), float(cos_i), float(sin2), complex(far),
                                 tuple((complex(n), float(d)) for n, d in layers), float(lam))


# ---- against the existing restatements ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, n_layers", cr.RANDOM_STACKS)
def test_the_reference_agrees_with_both_restatements_on_the_random_stacks(seed, n_layers):
    frame, coatings = cr.random_case(seed, n_layers)
    seen = tf.interfaces(frame, coatings)
    assert len(seen) == 24
    worst = 0.0
    for ni, cos_i, _, far, layers, lam, reflection in seen:
        # (the restatements take sin^2 as 1 - cos^2: the reference is given the same number here)
        want, _ = all_four((ni, cos_i, 1.0 - cos_i * cos_i, far, layers, lam, reflection))
        for formulation in (cr.matrix_coefficients, cr.rouard_coefficients):
            raw = formulation(ni, cos_i, complex(far), layers, lam)
            got = cr.project_coefficients(raw, True) + cr.project_coefficients(raw, False)
            worst = max(worst, max(abs(complex(w) - g) for w, g in zip(want, got)))
    print(f"stack {seed} of {n_layers}: largest difference from the restatements {worst:.3e}")
    assert worst <= 1e-14


# ---- against mpmath ------------------------------------------------------------------------------------------------------------
def matrices_in_mpmath(mp, ni, cos_i, sin2, far, layers, lam):
    """(r_s, r_p, t_s, t_p) from the characteristic matrices as include/prt.h writes them, in mpmath's arithmetic: its
    exponents are unbounded, so exp(Im delta) is no trouble there."""
    mpf, mpc = mp.mpf, mp.mpc
    q = mpf(ni) ** 2 * mpf(sin2)

    def ncos(n):
        w = mp.sqrt(mpc(n.real, n.imag) ** 2 - q)
        return -w if w.imag < 0 or (w.imag == 0 and w.real < 0) else w

    out = []
    for pol in (0, 1):
        def eta(n):
            return ncos(n) if pol == 0 else mpc(n.real, n.imag) ** 2 / ncos(n)

        near = mpf(ni) * mpf(cos_i) if pol == 0 else mpf(ni) / mpf(cos_i)
        b, c = mpc(1), eta(far)
        for n, d in reversed(layers):
            delta = 2 * mp.pi * ncos(n) * mpf(d) / mpf(lam)
            b, c = (mp.cos(delta) * b - 1j * mp.sin(delta) / eta(n) * c, -1j * eta(n) * mp.sin(delta) * b + mp.cos(delta) * c)
        r = (near * b - c) / (near * b + c)
        t = 2 * near / (near * b + c) * mp.sqrt(max(eta(far).real, 0) / near)
        out.append((r if pol == 0 else -r, t))
    return out[0][0], out[1][0], out[0][1], out[1][1]


@pytest.mark.parametrize("name", SMALL)
def test_the_reference_agrees_with_sixty_digits_in_every_regime(name):
    mpmath = pytest.importorskip("mpmath")
    frame, stacks = tf.case(name)
    worst = 0.0
    with mpmath.workdps(60):
        for arguments in tf.interfaces(frame, stacks):
            ni, cos_i, sin2, far, layers, lam, _ = arguments
            got, _ = all_four(arguments)
            want = matrices_in_mpmath(mpmath, float(ni), float(cos_i), float(sin2), complex(far),
                                      [(complex(n), float(d)) for n, d in layers], float(lam))
            for g, w in zip(got, want):
                assert abs(w) <= 1 + 1e-15
                # (a longdouble goes into mpmath exactly as the sum of two doubles)
                re = mpmath.mpf(float(g.real)) + mpmath.mpf(float(g.real - LD(float(g.real))))
                im = mpmath.mpf(float(g.imag)) + mpmath.mpf(float(g.imag - LD(float(g.imag))))
                worst = max(worst, float(abs(mpmath.mpc(re, im) - w)))
    print(f"{name}: largest difference from 60 digits {worst:.3e}")
    assert worst <= 1e-17


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1, ns", [(1.38, 1.52), (1.25, 1.5625), (2.0, 1.7)])
def test_a_quarter_wave_layer(n1, ns):
    lam = 4.0 * n1  # (then the thickness is 1 and the phase pi / 2 to the reference's last bit)
    (rs, rp, ts, tp), margin = tf.stack_coefficients(1.0, 1.0, 0.0, complex(ns), ((complex(n1), 1.0),), lam)
    want = ((LD(ns) - LD(n1) ** 2) / (LD(ns) + LD(n1) ** 2)) ** 2
    for r, t in ((rs, ts), (rp, tp)):
        assert abs(abs(r) ** 2 - want) <= 1e-18 and abs(abs(t) ** 2 - (1 - want)) <= 1e-18
    assert abs(rs + rp) <= 1e-18 and margin <= 1e-14  # (eight ulps of the phase)
    if n1 * n1 == ns:
        assert abs(rs) <= 1e-18


@pytest.mark.parametrize("metal", sorted(tf.METALS))
@pytest.mark.parametrize("im_delta", [1.2e4, 1e5, 1e9])
def test_an_opaque_layer_is_the_bare_interface_to_its_material(metal, im_delta):
    m = tf.METALS[metal]
    theta = tf.LADDER_ANGLE
    arguments = (1.0, float(np.cos(theta)), float(np.sin(theta) ** 2))
    layer = ((m, float(tf.thickness_for(m, theta, im_delta))),)
    for far in (1.5 + 0j, 1.0 + 0j, 0.2 + 3.4j):
        coated, margin = tf.stack_coefficients(*arguments, far, layer, tf.LAM)
        bare, _ = tf.stack_coefficients(*arguments, m, (), tf.LAM)
        assert coated[0] == bare[0] and coated[1] == bare[1]  # (exactly the bulk metal's r)
        assert coated[2] == 0 and coated[3] == 0 and margin <= 1e-14
    n, k = m.real, m.imag  # (and the bulk value is the textbook's at normal incidence)
    (rs, _, _, _), _ = tf.stack_coefficients(1.0, 1.0, 0.0, m, (), tf.LAM)
    assert abs(abs(rs) ** 2 - (LD((n - 1) ** 2) + LD(k * k)) / (LD((n + 1) ** 2) + LD(k * k))) <= 1e-15


def sinh_law(n_near, gap, n_far, cos_i, sin2, d_over_lam):
    """T_s of one evanescent gap between two media: with eta0, eta2 the s admittances outside and kappa = sqrt(q - n^2)
    in the gap, (B, C) = (cosh a - i (eta2 / kappa) sinh a, i kappa sinh a + eta2 cosh a) for a = 2 pi kappa d / lambda, so
    |eta0 B + C|^2 = (eta0 + eta2)^2 cosh^2 a + (kappa - eta0 eta2 / kappa)^2 sinh^2 a
                   = (eta0 + eta2)^2 + (eta0^2 + kappa^2) (eta2^2 + kappa^2) / kappa^2 sinh^2 a     (cosh^2 = 1 + sinh^2)
    and T = 4 eta0 eta2 / |.|^2 = T0 / (1 + A sinh^2 a), T0 = 4 eta0 eta2 / (eta0 + eta2)^2,
    A = (eta0^2 + kappa^2) (eta2^2 + kappa^2) / (kappa^2 (eta0 + eta2)^2); between equal media T0 = 1 and
    A = (eta0^2 + kappa^2)^2 / (4 kappa^2 eta0^2).  In longdouble."""
    q = LD(n_near) ** 2 * LD(sin2)
    eta0, eta2, kappa = LD(n_near) * LD(cos_i), np.sqrt(LD(n_far) ** 2 - q), np.sqrt(q - LD(gap) ** 2)
    a = tf.TWO_PI * kappa * LD(d_over_lam)
    big = (eta0 ** 2 + kappa ** 2) * (eta2 ** 2 + kappa ** 2) / (kappa ** 2 * (eta0 + eta2) ** 2)
    return 4 * eta0 * eta2 / (eta0 + eta2) ** 2 / (1 + big * np.sinh(a) * np.sinh(a))  # (sinh^2 of 5.2e3 is 1e4524: in range)


@pytest.mark.parametrize("degrees", [45.0, 60.0])
@pytest.mark.parametrize("far", [1.5, 1.6])
def test_a_frustrated_total_reflection_follows_the_sinh_law(degrees, far):
    cos_i, sin2 = float(np.cos(np.radians(degrees))), float(np.sin(np.radians(degrees)) ** 2)
    for gap in tf.GAPS:
        # (the wavelength is 1 and the thickness the gap in waves: the law gets the numbers the reference gets)
        (rs, rp, ts, tp), margin = tf.stack_coefficients(1.5, cos_i, sin2, complex(far), ((1.0 + 0j, float(gap)),), 1.0)
        want = sinh_law(1.5, 1.0, far, cos_i, sin2, gap)
        got = abs(ts) ** 2
        assert abs(got - want) <= 1e-17 and abs(got / want - 1) <= 1e-14, (gap, got, want)  # (a is up to 5e3: times 2^-64)
        assert abs(abs(rs) ** 2 + got - 1) <= 4e-17 and abs(abs(rp) ** 2 + abs(tp) ** 2 - 1) <= 4e-17
        assert margin <= tf.TIGHT_CAP


@pytest.mark.parametrize("name", SMALL)
def test_lossless_stacks_keep_the_energy(name):
    frame, stacks = tf.case(name)
    checked = 0
    for arguments in tf.interfaces(frame, stacks):
        far, layers = complex(arguments[3]), arguments[4]
        if far.imag == 0 and all(complex(n).imag == 0 for n, _ in layers):
            (rs, rp, ts, tp), _ = all_four(arguments)
            # (each coefficient is good to 1e-17: |r|^2 + |t|^2 to 2 (|r| + |t|) 1e-17 <= 4e-17)
            assert abs(abs(rs) ** 2 + abs(ts) ** 2 - 1) <= 4e-17 and abs(abs(rp) ** 2 + abs(tp) ** 2 - 1) <= 4e-17
            checked += 1
    assert checked or CASE_IS_ABSORBING[name]


CASE_IS_ABSORBING = {name: tf.CASES[name][0] in ("attenuation", "grazing") for name in tf.CASES}


# ---- the margin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tf.CASES))
def test_the_margin_of_every_case_the_device_is_held_to_is_under_its_cap(name):
    regime, _, cap = tf.CASES[name]
    assert cap == (tf.TIGHT_CAP if regime in ("attenuation", "evanescent") else tf.CAP) and tf.CAP == 1e-9 and tf.TIGHT_CAP == 1e-13
    frame, stacks = tf.case(name)
    for polarization in tf.POLARIZATIONS:
        want = tf.reference(name, polarization)
        assert want["n_invalid"] == 0 and not np.isnan(want["transmittance"]).any() and not np.isnan(want["field"]).any()
        assert want["n_coated"] > 0 and len(frame) <= 600
        print(f"{name}: largest margin {want['margin'].max():.3e} (cap {cap:.0e})")
        assert want["margin"].max() <= cap


def test_what_the_cases_leave_out_is_over_the_cap():
    """The far medium next to its critical angle, and a ray that leaves the glass next to grazing: the margins of the
    offsets the issue's list has and the frames do not.  The definition is ill-conditioned there (include/prt.h)."""
    for off, ways in tf.FAR_LEFT_OUT:
        frame = tf.frame_of(tf.far_rays(off, ways))
        assert tf.fresnel(frame, coatings={1: tf.FAR_STACK})["margin"].max() > tf.CAP, off
    frame = tf.frame_of([tf.four_ways(np.pi / 2 - 1e-6, 0.7)[k] for k in (1, 3)])
    assert tf.fresnel(frame, coatings={1: tf.GRAZING_STACK})["margin"].max() > tf.CAP


def test_the_margin_is_nothing_where_the_stack_is_well_conditioned_and_grows_with_the_phase():
    thin, _ = all_four((1.0, 0.9, 0.19, 1.5, ((1.38, 0.1),), 0.55, False)), None
    thick, _ = all_four((1.0, 0.9, 0.19, 1.5, ((1.38, 25000.0),), 0.55, False)), None
    assert thin[1] <= 1e-14 and 1e-11 <= thick[1] <= 1e-9
