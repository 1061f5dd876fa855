#!/usr/bin/env python3
"""Ray paths of a stopped lens: which surfaces every ray met, in order (DeviceFrame.paths / RayTracer.trace_paths,
DESIGN.md §4.5).  Three fans of different width light a plano-convex lens behind an aperture stop that clips the wider
ones, and a detector.  The path tree answers what a spot figure silently leaves out:

  * what fraction of each field is vignetted, and by which surface (Paths.fates);
  * which rays arrived at the detector without passing both lens surfaces (Paths.find);
  * the spot size of "all rays at the detector" against "rays that passed both lens surfaces", the frame cut by path
    (frame.select(paths.rows(...))) and handed to group_stats.

    python examples/ray_paths.py [rays per source]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyrayt_amd as pyrayt  # noqa: E402


def build(rays):
    c = pyrayt.components
    stop = c.aperture((3.0, 3.0), 0.5).move_x(-0.5)
    lens = c.plano_convex_lens(1.5, 0.3, aperture=1.2)
    detector = c.baffle((4, 4)).move_x(2.5)
    fields = [c.WedgeOfRays(angle).move_x(-3) for angle in (10, 24, 40)]
    return pyrayt.RayTracer(fields, [stop, lens, detector], rays_per_source=rays), stop, lens, detector


def main():
    rays = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    tracer, stop, lens, detector = build(rays)
    names = {sid: "stop" for sid, _ in stop.surface_ids}
    names.update({sid: "lens" for sid, _ in lens.surface_ids})
    names.update({sid: "detector" for sid, _ in detector.surface_ids})

    paths = tracer.trace_paths()
    print(f"{paths.n_rays} rays with rows, {paths.n_nodes} nodes, {len(paths.complete())} complete paths")
    table = paths.to_pandas()
    print(table[table["ended"] > 0][["source_id", "sequence", "ended", "dark", "energy_ended"]].to_string(index=False))

    print("\nwhere the rays of each field ended (surface -1: never met a surface):")
    fates = paths.fates()
    fates["where"] = [names.get(s, "nothing") for s in fates["surface"]]
    print(fates.to_string(index=False))
    at_detector = fates[fates["where"] == "detector"].groupby("source_id")["ended"].sum()
    for g in range(paths.n_groups):
        print(f"field {g}: {1.0 - at_detector.get(g, 0) / rays:.1%} vignetted")

    print("\nby component, consecutive surfaces of one component taken together:")
    merged = paths.merge(names, collapse_repeats=True)
    for k in merged.complete():
        print(f"  {' > '.join(merged.sequences[k])}: {merged.ended[:, k].tolist()} rays per field")

    # the frame cut by path, for the passes that take "the rays at the detector" as given
    frame = tracer.trace_device()
    paths = frame.paths(rays_per_source=rays, n_groups=paths.n_groups)
    lens_ids = [sid for sid, _ in lens.surface_ids]
    reached = paths.find(ends_at=detector)
    both = [k for k in reached if sum(s in lens_ids for s in paths.sequences[k]) >= 2]
    everything = frame.group_stats(surface=detector.get_id(), rays_per_source=rays, n_groups=paths.n_groups)
    print(f"\n{len(reached)} paths end at the detector, {len(both)} of them through both lens surfaces")
    if len(both):
        through = frame.select(paths.rows(both)).group_stats(surface=detector.get_id(), rays_per_source=rays,
                                                             n_groups=paths.n_groups)
        for g in range(paths.n_groups):
            print(f"field {g}: rms spot radius {everything['rms_radius'][g]:.6f} over all rays at the detector, "
                  f"{through['rms_radius'][g]:.6f} over the rays that passed both lens surfaces")
    stray = [k for k in reached if k not in both]
    print(f"rays at the detector that did not pass both lens surfaces: {int(np.sum(paths.ended[:, stray]))}")


if __name__ == "__main__":
    main()
