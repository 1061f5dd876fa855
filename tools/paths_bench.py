#!/usr/bin/env python3
"""Ray-path analysis of the frame on the device (DeviceFrame.paths), timed with device events after warm-up, on two
frames of the same size:

  one_path      BASELINE config 2 at --rays rays: 3 generations, every ray the same three surfaces (3 nodes)
  many_paths    a frame made by hand with the same rows per generation: the surface of every row drawn from five, so
                5 + 25 + 125 = 155 nodes and every wave holding all the keys of several parents

  paths         DeviceFrame.paths() end to end (the launches, the read-back of the nodes, the host's ordering, the remap)
  optical_path  the yardstick: DeviceFrame.optical_path(), the other per-generation pass over a dense per-id table
  host          the host route: copy id / surface / generation / intensity, pandas groupby("id")["surface"].agg(tuple)
                and the per-path counts and sums (wall time, one core)

Prints one JSON line per figure.  usage: tools/paths_bench.py [--rays N] [--steps K] [--no-host]
(run under rocprofv3 --kernel-trace --stats for per-kernel times: k_paths_step against k_frame_optical_path)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402
from mtf_bench import device_ms  # noqa: E402
from pyrayt_amd.frame import _INDEX, DeviceFrame  # noqa: E402


def host_paths(frame):
    """The host route: four columns brought over, the surface sequence per id, rays and energy per complete path."""
    table = pd.DataFrame({name: frame[name].cpu().numpy() for name in ("generation", "id", "surface", "intensity")})
    table = table.sort_values(["id", "generation"], kind="stable")
    sequence = table.groupby("id")["surface"].agg(tuple)
    last = table.groupby("id")["intensity"].last()
    return pd.DataFrame({"sequence": sequence, "energy": last}).groupby("sequence")["energy"].agg(["size", "sum"])


def many_paths_frame(like, surfaces=5, seed=1):
    rows = like.rows.clone()
    generator = torch.Generator(device=rows.device).manual_seed(seed)
    rows[_INDEX["surface"]] = torch.randint(0, surfaces, (rows.shape[1],), device=rows.device, generator=generator).double()
    return DeviceFrame(rows, like.rows_per_generation)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    one = tracer.trace_device()
    frames = {"one_path": one, "many_paths": many_paths_frame(one)}
    for name, frame in frames.items():
        common = {"device": torch.cuda.get_device_name(0), "frame": name, "rays": args.rays, "rows": len(frame),
                  "generations": len(frame.rows_per_generation)}
        got = frame.paths()
        ms = device_ms(lambda: frame.paths(), args.steps)
        print(json.dumps({**common, "what": "paths", "ms": ms, "nodes": got.n_nodes, "complete": len(got.complete()),
                          "rays_ended": int(got.ended.sum())}), flush=True)
        ms = device_ms(lambda: frame.paths(weights=None), args.steps)
        print(json.dumps({**common, "what": "paths_unweighted", "ms": ms}), flush=True)
        ms = device_ms(lambda: frame.optical_path(), args.steps)
        print(json.dumps({**common, "what": "optical_path", "ms": ms}), flush=True)
        if not args.no_host:
            t = time.perf_counter()
            table = host_paths(frame)
            print(json.dumps({**common, "what": "host", "copy_groupby_ms": (time.perf_counter() - t) * 1e3,
                              "complete": len(table), "rays_ended": int(table["size"].sum())}), flush=True)


if __name__ == "__main__":
    main()
