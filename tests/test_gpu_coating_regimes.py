"""The coated Fresnel pass on the device in the regimes the random stacks of tests/coating_reference.py leave out: layers
that are opaque many times over, evanescent gaps, angles next to a critical one and next to grazing, phases of 1e5 rad, a
resonant cavity of 15 layers.  The reference is tests/thinfilm_reference.py: longdouble, another formulation than the
kernel's, held to 60 digits by tests/test_host_thinfilm_reference.py.

The bar: the counters equal the reference's, NaN only where the reference has NaN, and every component of T and of the
fields within 1e-12 + margin of it: 1e-12 is the bar of tests/test_gpu_coatings.py, the margin is the reference's own
statement of how far eight ulps of the thicknesses and of the Snell invariant move the coefficients a ray has met, capped
on the CPU at 1e-9 and, in the attenuation and evanescent regimes, at 1e-13."""
import numpy as np
import pytest

import thinfilm_reference as tf
from test_gpu_coatings import counters, run

pytestmark = pytest.mark.gpu

TOL = 1e-12
_SEEN = {}


def held(name, polarization):
    """The device's result for a case held to the reference's; (T, field, reference) for what a regime adds."""
    regime = tf.CASES[name][0]
    frame, stacks = tf.case(name)
    want = tf.reference(name, polarization)
    got, t, field = run(frame, stacks, polarization=polarization)
    bound = TOL + want["margin"]
    seen = _SEEN.setdefault(regime, [0.0, 0.0])
    for mine, theirs, label in ((t, want["transmittance"], "T"), (field, want["field"], "field")):
        off = np.abs(mine - theirs)
        both = ~(np.isnan(mine) | np.isnan(theirs))
        seen[0] = max(seen[0], float(np.max(off, where=both, initial=0.0)))
        seen[1] = max(seen[1], float(np.max(off / bound, where=both, initial=0.0)))
    print(f"{name}, {polarization}: invalid {got.n_invalid}; regime '{regime}' so far: largest deviation {seen[0]:.3e}, "
          f"largest deviation to bound {seen[1]:.3f}")
    assert counters(got) == tf.cr.counters(want), name
    for mine, theirs, label in ((t, want["transmittance"], "T"), (field, want["field"], "field")):
        assert np.array_equal(np.isnan(mine), np.isnan(theirs)), (name, label)
        assert np.all(np.abs(mine - theirs) <= bound), (name, label, float(np.nanmax(np.abs(mine - theirs) / bound)))
    return t, field, want


@pytest.mark.parametrize("name", [name for name in tf.CASES if tf.CASES[name][0] == "attenuation"])
def test_opaque_layers_reflect_as_their_bulk_and_pass_nothing(name):
    frame, stacks = tf.case(name)
    for polarization in tf.POLARIZATIONS:
        t, field, want = held(name, polarization)
        assert want["n_invalid"] == 0 and not np.isnan(t).any() and not np.isnan(field).any()
    if name.startswith("ladder") and "rays" not in name:
        # rays 4 k .. 4 k + 3 are the four ways through the layer of Im delta = LADDER[k]
        ids, generation = frame[:, tf.ref.IX["id"]].astype(int) - 3, frame[:, 0].astype(int)
        for k, im_delta in enumerate(tf.LADDER):
            passed = t[(ids // 4 == k) & (ids % 4 < 2) & (generation >= 1)]
            assert len(passed) == 3 and np.all(passed <= 4.0 * np.exp(-2.0 * im_delta) + TOL)  # (|t|^2 <= |t_in t_out|^2 e^-2 Im d)
            bounced = t[(ids // 4 == k) & (ids % 4 >= 2) & (generation == 1)]
            bulk = t[(ids // 4 == len(tf.LADDER) - 1) & (ids % 4 >= 2) & (generation == 1)]
            assert im_delta < 40 or np.all(np.abs(bounced - bulk) <= 2 * TOL)  # (the bulk metal's R from 40 on)


def test_evanescent_gaps_keep_the_energy_and_follow_the_sinh_law():
    from test_host_thinfilm_reference import sinh_law

    frame, _ = tf.case("evanescent gap")
    ambient, gap, substrate = tf.GAP_MEDIA
    ids, generation = frame[:, tf.ref.IX["id"]].astype(int), frame[:, 0].astype(int)
    for polarization in tf.POLARIZATIONS:
        t, field, want = held("evanescent gap", polarization)
        assert want["n_tir"] == 0  # (the far medium, 1.6 or 1.5, propagates: the gap does not make it total)
        bound = TOL + want["margin"].max()
        # the plane of incidence is xy, so s is z: |Ea_z|^2 + |Eb_z|^2 is the s power, the rest of |E|^2 the p power
        power_s = np.abs(field[2]) ** 2 + np.abs(field[5]) ** 2
        power_p = np.abs(field[0]) ** 2 + np.abs(field[1]) ** 2 + np.abs(field[3]) ** 2 + np.abs(field[4]) ** 2
        for k in range(len(tf.GAPS) * len(tf.GAP_ANGLES)):
            row = {(way, g): np.flatnonzero((ids == 4 * k + way) & (generation == g))[0] for way in range(4) for g in (0, 1)}
            theta = tf.GAP_ANGLES[k % 2]
            for power in (power_s, power_p):  # (R + T = 1 per polarisation, from either side; at most eight components,
                # each within the bound and of modulus <= 1, squared: 2 * 8 bounds)
                assert abs(power[row[0, 1]] + power[row[2, 1]] - power[row[0, 0]]) <= 16 * bound
                assert abs(power[row[1, 1]] + power[row[3, 1]] - power[row[1, 0]]) <= 16 * bound
            law = float(sinh_law(ambient, gap, substrate, np.cos(theta), np.sin(theta) ** 2, tf.GAPS[k // 2]))
            if power_s[row[0, 0]] > 0.01:
                assert abs(power_s[row[0, 1]] / power_s[row[0, 0]] - law) <= 16 * bound / power_s[row[0, 0]] + 1e-13
                assert abs(power_s[row[1, 1]] / power_s[row[1, 0]] - law) <= 16 * bound / power_s[row[1, 0]] + 1e-13


@pytest.mark.parametrize("name", [name for name in tf.CASES if tf.CASES[name][0] in ("critical", "grazing", "thick", "cavity")])
def test_ill_conditioned_stacks_within_the_margin_of_the_reference(name):
    for polarization in tf.POLARIZATIONS:
        t, field, want = held(name, polarization)
        assert want["n_invalid"] == 0 and not np.isnan(t).any()
    if name == "the far medium at its critical angle":
        assert want["n_tir"] == len(tf.FAR_ABOVE)  # (above the far medium's critical angle and nowhere else)
    if name == "a layer at its critical angle":
        assert want["n_tir"] == 0  # (the far medium decides, not the layer)
    if name == "cavity of 15 layers":
        frame, _ = tf.case(name)
        through = t[(frame[:, tf.ref.IX["id"]].astype(int) % 8 == 0) & (frame[:, 0] == 1)]  # (normal incidence, into the glass)
        assert through[2] > 0.95 and np.all(through[[0, 4]] < 0.5) and np.all(through[[1, 3]] > 0.7)  # (across the passband)
