#!/usr/bin/env python3
"""Histograms of the frame on the device (DeviceFrame.histogram2d / RayTracer.trace_histogram), timed with device events
after warm-up.

  kernel    one prt_frame_histogram call over 1M rows at 64^2, 256^2 and 1024^2 bins, 1 and 8 groups, for a concentrated
            spot (BASELINE config 2's detector rows: most rows in a few bins) and a uniform spread (a seeded synthetic
            frame); and the prt_frame_range pass behind range=None.  Device time of the library call alone (the edges
            are made once; nothing crosses PCIe but them).
  loop      a move-a-part iteration at 1M rays, 256^2 bins: trace_histogram against record_only(det, columns=("y1",
            "z1")) + trace_device() alone, and against the host path (copy the two columns, np.histogram2d).

Prints one JSON line per figure.  usage: tools/histogram_bench.py [--rows N] [--steps K] [--loop-steps K]
(run the kernel part under rocprofv3 --kernel-trace --stats for per-kernel times)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402
from pyrayt_amd import engine  # noqa: E402
from pyrayt_amd.frame import DeviceFrame, histogram_edges  # noqa: E402


def device_ms(fn, steps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def spot_frame(rays):
    """Config 2's detector rows, ids over eight groups."""
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=rays)
    tracer.record_only(det)
    frame = tracer.trace_device()
    return DeviceFrame(frame.rows.clone(), None), tracer, det


def uniform_frame(rows):
    gen = torch.Generator(device="cuda").manual_seed(7)
    block = torch.zeros((15, rows), dtype=torch.float64, device="cuda")
    block[10] = torch.rand(rows, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    block[11] = torch.rand(rows, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    block[4] = torch.arange(rows, dtype=torch.float64, device="cuda")
    return DeviceFrame(block)


def kernel_call(frame, bins, n_groups, box, rays_per_source):
    """The library call DeviceFrame.histogram2d makes, without the host conversion of its result."""
    lib = engine.library()
    rows = frame.rows
    dev = rows.device
    edges, uniform = histogram_edges(bins, box, 2, None)
    nx, ny = len(edges[0]) - 1, len(edges[1]) - 1
    counts = torch.empty((n_groups, nx, ny), dtype=torch.int64, device=dev)
    work = torch.empty(int(lib.prt_frame_histogram_workspace_bytes(n_groups, nx, ny, 0)), dtype=torch.uint8, device=dev)
    rps = float(rays_per_source) if n_groups > 1 else 0.0
    stream = engine._stream_ptr(torch, dev)
    nan = float("nan")

    def run():
        engine._check(lib.prt_frame_histogram(0, rows.data_ptr(), rows.stride(0), rows.shape[1], nan, nan, rps, n_groups,
                                              10, edges[0].ctypes.data, nx, 1, 11, edges[1].ctypes.data, ny, 1, -1,
                                              counts.data_ptr(), None, work.data_ptr(), stream))
    return run


def range_call(frame):
    lib = engine.library()
    rows = frame.rows
    box = torch.empty(2, dtype=torch.float64, device=rows.device)
    stream = engine._stream_ptr(torch, rows.device)
    nan = float("nan")

    def run():
        engine._check(lib.prt_frame_range(0, rows.data_ptr(), rows.stride(0), rows.shape[1], nan, nan, 10,
                                          box.data_ptr(), stream))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--loop-steps", type=int, default=30)
    args = ap.parse_args()
    spot, tracer, det = spot_frame(args.rows)
    frames = {"spot": spot, "uniform": uniform_frame(len(spot))}
    y, z = spot["y1"], spot["z1"]
    boxes = {"spot": ((float(y.min()), float(y.max())), (float(z.min()), float(z.max()))), "uniform": ((-1, 1), (-1, 1))}
    for bins in (64, 256, 1024):
        for n_groups in (1, 8):
            for name, frame in frames.items():  # (interleaved: both distributions at each size)
                ms = device_ms(kernel_call(frame, bins, n_groups, boxes[name], args.rows // 8), args.steps)
                print(json.dumps({"figure": "kernel", "rows": len(frame), "bins": f"{bins}x{bins}", "groups": n_groups,
                                  "distribution": name, "us": round(ms * 1e3, 2)}), flush=True)
    for name, frame in frames.items():
        ms = device_ms(range_call(frame), args.steps)
        print(json.dumps({"figure": "range", "rows": len(frame), "distribution": name, "us": round(ms * 1e3, 2)}),
              flush=True)

    # the design loop: move a part, trace, bin
    lens = tracer.get_system()[0]
    box = ((-0.05, 0.05), (-0.05, 0.05))

    def wall_ms(fn, steps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    step = [0]

    def nudge():
        step[0] += 1
        lens.move_x(1e-4 if step[0] % 2 else -1e-4)

    def with_histogram():
        nudge()
        tracer.trace_histogram("y1", "z1", surface=det, bins=256, range=box)

    def trace_alone():
        nudge()
        tracer.record_only(det, columns=("y1", "z1"))
        tracer.trace_device()
        tracer.record_only()

    def host_path():
        nudge()
        tracer.record_only(det, columns=("y1", "z1"))
        cols = tracer.trace_device().to_numpy()
        tracer.record_only()
        np.histogram2d(cols[:, 0], cols[:, 1], bins=256, range=box)

    results = {}
    for _ in range(2):  # (interleaved A / B / C, twice; the last round is reported)
        for label, fn in (("trace_histogram", with_histogram), ("record_only_trace", trace_alone), ("host_histogram2d", host_path)):
            results[label] = wall_ms(fn, args.loop_steps if label != "host_histogram2d" else max(3, args.loop_steps // 5))
    print(json.dumps({"figure": "loop", "rays": args.rows, "bins": "256x256",
                      **{k: round(v, 4) for k, v in results.items()},
                      "histogram_over_trace_ms": round(results["trace_histogram"] - results["record_only_trace"], 4),
                      "host_over_device": round(results["host_histogram2d"] / results["trace_histogram"], 1)}), flush=True)


if __name__ == "__main__":
    main()
