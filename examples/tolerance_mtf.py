"""The MTF yield of a singlet from ONE trace: a point source imaged one to one, the detector near the paraxial focus.  Given
that the lens is only good to a decentre, a tilt, a front radius and an index tolerance, what share of the built lenses
keeps the MTF above a threshold at one frequency -- with the detector where it is, and with every lens refocused?
``trace_mtf_tolerance`` traces once with ``slopes=True`` and evaluates every trial on the device under the linear ray model,
the MTF itself fully nonlinear in the moved landing points.

    python examples/tolerance_mtf.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyrayt_amd as pyrayt  # noqa: E402


def main():
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    source = pyrayt.components.ConeOfRays(cone_angle=3).move_x(-4.0)
    detector = pyrayt.components.baffle((1, 1)).move_x(4.2)
    tracer = pyrayt.RayTracer(source, [lens, detector], rays_per_source=100_000)
    parameters = [pyrayt.Motion(lens, translate=(0, 1, 0)), pyrayt.Motion(lens, rotate=(0, 0, 1)),
                  pyrayt.Deformation.radius(lens.surface_ids[0][1], keep=(-0.125, 0, 0)), pyrayt.IndexChange(lens)]
    names = ("decentre", "tilt", "front radius", "index")
    tolerances = pyrayt.Tolerances([0.02, 0.01, 0.02, 0.002], distribution="normal", seed=1)
    # the frequency: the highest of a ladder at which the lens as designed still has an MTF of 0.6 in both azimuths
    ladder = np.geomspace(0.5, 2000.0, 37)
    nominal = tracer.trace_mtf(detector, ladder).mtf[0, 0].min(axis=0)
    good = np.flatnonzero(nominal >= 0.6)
    frequency = float(ladder[good[-1]]) if len(good) else float(ladder[0])
    threshold = 0.5
    print(f"MTF >= {threshold} at {frequency:.1f} cycles per unit (as designed: {nominal[good[-1] if len(good) else 0]:.3f})")
    for compensators in ((), ("focus",)):
        run = tracer.trace_mtf_tolerance(detector, parameters, tolerances, [frequency], trials=2000, azimuths=(0.0, 90.0),
                                         compensators=compensators)
        low, median, high = run.percentiles((5, 50, 95), frequency=0, azimuth=0)[0]
        print(f"compensators {compensators or 'none'}: nominal MTF {run.nominal.mtf[0, 0, :, 0].round(4)}, yield "
              f"{run.yield_(threshold)[0]:.3f}; MTF percentiles 5 / 50 / 95: {low:.3f} / {median:.3f} / {high:.3f}; RMS radius "
              f"{run.rms_radius[0, :, 0].mean():.5f}; refocus of {np.abs(run.focus_shift[0]).mean():.4f} on average")
    table = tracer.trace_mtf_tolerance(detector, parameters, None, [frequency],
                                       trials=tolerances.sensitivity_table()).table()
    table["parameter"] = [names[k] for k in table["parameter"]]
    print(table.to_string(index=False))


if __name__ == "__main__":
    main()
