"""The enclosed-energy yield of a singlet from ONE trace: a point source imaged one to one, the detector near the
paraxial focus.  Given that the lens is only good to a decentre, a front radius and an index tolerance, what share of the
built lenses puts 80 % of the energy inside a pixel -- once about every lens's own centroid (the pixel follows the spot,
what ``enclosed_energy()`` of each built lens reports) and once about the fixed pixel (the spot walks off it: the case a
decentre tolerance is about)?  ``trace_energy_tolerance`` traces once with ``slopes=True`` and evaluates every trial on the
device under the linear ray model, the energy itself counted exactly on the moved landing points.

    python examples/tolerance_energy.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyrayt_amd as pyrayt  # noqa: E402


def main():
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    source = pyrayt.components.ConeOfRays(cone_angle=3).move_x(-4.0)
    detector = pyrayt.components.baffle((1, 1)).move_x(4.2)
    tracer = pyrayt.RayTracer(source, [lens, detector], rays_per_source=100_000)
    parameters = [pyrayt.Motion(lens, translate=(0, 1, 0)), pyrayt.Deformation.radius(lens.surface_ids[0][1], keep=(-0.125, 0, 0)),
                  pyrayt.IndexChange(lens)]
    names = ("decentre", "front radius", "index")
    tolerances = pyrayt.Tolerances([0.02, 0.02, 0.002], distribution="normal", seed=1)
    # the pixel: a square whose half-width is 1.25 x the half-width that holds 80 % of the energy of the lens as designed
    nominal = tracer.trace_enclosed_energy(detector, fractions=(0.8,), shape="square")
    pixel = 1.25 * float(nominal.radius[0, 0, 0])
    print(f"pixel half-width {pixel:.5f} (as designed 80 % of the energy lies within {nominal.radius[0, 0, 0]:.5f})")
    for follow, what in ((True, "about each lens's own centroid"), (False, "about the fixed pixel")):
        run = tracer.trace_energy_tolerance(detector, parameters, tolerances, [pixel], trials=2000, fractions=(0.8, 0.9),
                                            shape="square", follow_centroid=follow)
        low, median, high = run.percentiles((10, 50, 90), fraction=0)[0]
        print(f"{what}: as designed {run.nominal.energy[0, 0, 0]:.4f} inside; yield of '80 % inside the pixel' "
              f"{run.yield_(0.8)[0]:.3f}; EE80 half-width percentiles 10 / 50 / 90: {low:.5f} / {median:.5f} / {high:.5f}")
    table = tracer.trace_energy_tolerance(detector, parameters, None, trials=tolerances.sensitivity_table(), fractions=(0.8,),
                                          shape="square", follow_centroid=False).table()
    table["parameter"] = [names[k] for k in table["parameter"]]
    print(table.to_string(index=False))


if __name__ == "__main__":
    main()
