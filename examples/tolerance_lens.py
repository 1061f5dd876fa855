"""Can this system be built?  Monte Carlo tolerancing of a parabolic mirror from one trace.

An f/2 parabolic mirror brings a collimated beam to its focus (a section of the beam beside the small detector, so the
nominal system is stigmatic: Strehl ratio 1).  Three things are only good to a tolerance: the mirror's place along its axis,
its decentre and its tilt about the vertex.  ``trace_tolerance`` traces the nominal system once, differentiates every
ray's optical path in the three parameters (``sensitivity(wavefront=True)``) and then evaluates thousands of perturbed
systems on the device under the linear ray model: each ray's OPD moves linearly in the parameters, the Strehl ratio of a
trial is the full coherent sum over the moved OPDs (not ``strehl + dstrehl . p``, which fails at the phase changes
tolerances produce).

It prints ``psf()``'s Strehl ratio of the nominal system beside the run's own nominal trial, then the share of the built
systems that reach a Strehl ratio of 0.8 when nothing is re-adjusted, when the detector may be re-centred on the image
("tilt") and when it may also be refocused ("tilt" and "focus") -- almost none, somewhat over half, and all of them -- and,
from a one-at-a-time sensitivity table at the tolerance's edge, which tolerance costs the most.

usage: python examples/tolerance_lens.py [--rays N] [--trials M] [--distribution uniform|normal|parabolic] [--seed S]
(needs an AMD GPU and the built library)"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyrayt_amd as pyrayt  # noqa: E402

UNIT = 1000.0  # (world units are millimetres)
NAMES = ("axial shift", "decentre y", "tilt about z")
WIDTHS = (0.05, 0.1, 0.01)  # mm, mm, radians


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=20_000)
    ap.add_argument("--trials", type=int, default=2000)
    ap.add_argument("--distribution", default="uniform", choices=pyrayt.Tolerances.DISTRIBUTIONS)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    mirror = pyrayt.components.parabolic_mirror(3.0, 0.5, aperture=1.5)  # (focus at the origin, vertex at x = -3)
    detector = pyrayt.components.baffle((0.1, 0.1))
    # a line of parallel rays along -x over y = 0.1 .. 0.7: it passes beside the detector on its way to the mirror
    source = pyrayt.components.LineOfRays(spacing=0.6).rotate_z(180).move(2.0, 0.4, 0.0)
    tracer = pyrayt.RayTracer(source, [mirror, detector], rays_per_source=args.rays)
    print(f"nominal system: psf() Strehl {tracer.trace_psf(detector, world_unit_um=UNIT, pixels=1).strehl[0]:.4f}")
    parameters = [pyrayt.Motion(mirror, translate=(1, 0, 0)), pyrayt.Motion(mirror, translate=(0, 1, 0)),
                  pyrayt.Motion(mirror, rotate=(0, 0, 1), pivot=(-3.0, 0.0, 0.0))]
    tolerances = pyrayt.Tolerances(WIDTHS, args.distribution, seed=args.seed)
    for compensators in ((), ("tilt",), ("tilt", "focus")):
        run = tracer.trace_tolerance(detector, parameters, tolerances, trials=args.trials, world_unit_um=UNIT,
                                     compensators=compensators)
        low, median = run.percentiles((2, 50))["strehl"][0]
        print(f"compensators {compensators}: nominal trial Strehl {run.nominal.strehl[0]:.4f}, yield at Strehl 0.8 "
              f"{100 * run.yield_(0.8)[0]:.1f} % of {run.n_trials} trials, median {median:.4f}, 2nd percentile {low:.4f}, "
              f"median RMS OPD {1e3 * float(run.percentiles((50,))['rms_opd'][0, 0]):.4f} um")
    table = tracer.trace_tolerance(detector, parameters, None, trials=tolerances.sensitivity_table(), world_unit_um=UNIT,
                                   compensators=("tilt",)).table()
    print("worst offenders (change of the Strehl ratio at -width / +width, the image re-centred):")
    for _, row in table.iterrows():
        k = int(row["parameter"])
        print(f"  {NAMES[k]:>14s} +-{WIDTHS[k]:g}: {row['dstrehl_minus']:+.4f} / {row['dstrehl_plus']:+.4f}")


if __name__ == "__main__":
    main()
