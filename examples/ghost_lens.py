#!/usr/bin/env python3
"""Ghost images of a singlet (RayTracer.trace_ghosts).  An uncoated glass surface reflects about 4 % of
the light; what is reflected twice travels towards the imager again and lands there as a ghost.  This puts the biconvex
lens of the README and its detector inside an absorbing housing (every ray then ends on a surface, so every reflection
is seen), follows the light through two reflections, and prints the ranked table of ghost paths -- which pair of
surfaces, how much energy, how tightly focused -- for the bare lens and with a quarter-wave layer of MgF2 on it.

    python examples/ghost_lens.py [rays]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyrayt_amd as pyrayt  # noqa: E402


def main():
    rays = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    source = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-2)
    detector = pyrayt.components.baffle((1, 1)).move_x(1)
    housing = pyrayt.ghosts.housing(30.0)
    tracer = pyrayt.RayTracer(source, [lens, detector, housing], rays_per_source=rays)
    names = {sid: f"lens surface {sid}" for sid, _ in lens.surface_ids}

    def report(label, analysis):
        table = analysis.table()
        print(f"{label}: signal on the detector {analysis.signal_energy():.1f}, {len(table)} ghost path(s)")
        for _, line in table.iterrows():
            path = " -> ".join(names.get(s, str(s)) for s in line["surfaces"])
            print(f"  order {line['order']}  {path:<36} rays {line['rays']:>8}  energy {line['energy']:12.4f}  "
                  f"share {line['share']:.3e}  centroid ({line['y']:+.4f}, {line['z']:+.4f})  rms radius {line['rms_radius']:.4f}")
        for order, entry in enumerate(analysis.orders[1:], start=1):
            g = entry.ghosts
            print(f"  order {order}: {g.n_spawned} children in {g.n_groups} group(s), {g.n_dropped} dropped, {g.n_dark} dark, "
                  f"{g.n_invalid} invalid, {g.n_open} open")

    report("bare lens", tracer.trace_ghosts(detector, order=2))
    layer = pyrayt.materials.Coating.quarter_wave(1.38, 0.55)  # (MgF2, a quarter wave thick at 0.55 um)
    report("quarter-wave MgF2", tracer.trace_ghosts(detector, order=2, fresnel=dict(coatings={lens: layer})))
    try:
        pyrayt.RayTracer(source, [lens, detector], rays_per_source=rays).trace_ghosts(detector, order=2)
    except ValueError as error:
        print(f"without the housing: {error}")


if __name__ == "__main__":
    main()
