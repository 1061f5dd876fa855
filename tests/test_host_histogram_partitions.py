"""The restated plan of the frame histograms (tests/histogram_partitions.py) on the host (CPU): held to the text of
prt_histogram.hpp, to the measured point the source quotes, and to the arms the GPU cases name, at the CU counts of a
whole MI355X and of others."""
import os

import pytest

from histogram_partitions import BLOCK, FOLD_CHUNKS, arm_rows, last_packed_rows, plan, slab_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_restated_plan_is_the_one_in_the_source():
    with open(os.path.join(ROOT, "pyrayt_amd", "csrc", "prt_histogram.hpp")) as handle:
        text = handle.read()
    for line in ("kHistBlock = 1024;", "kHistLdsBytes = 128 * 1024;", "kHistMaxBlocksPerCu = 2;", "kHistFoldChunks = 8;",
                 "const int packed = !weights_out && per_thread * kHistBlock < 65536;",
                 "packed ? 2 * kHistLdsBytes / 4 : kHistLdsBytes / (weights_out ? 12 : 4)",
                 "(size_t)(160 * 1024) / std::max<size_t>(lds, 1)",
                 "std::min<int64_t>(blocks, (int64_t)cus * per_cu)",
                 "1.0 - std::exp(-8.0 * per_window_rows / window), share = window / 65536.0",
                 "!weights_out && 90.0 * touched * share > 10.0 + 20.0 * share",
                 "hipDeviceAttributeMultiprocessorCount"):
        assert line in text, line
    # the measured point the source quotes: 1M rows, 256 x 256 bins, 256 CUs -- packed, 4096 rows a workgroup, slab
    p = plan(1 << 20, 65536, 256)
    assert p.packed and p.window == 65536 and p.grid == 256 and p.share_rows == 4096 and p.slab


@pytest.mark.parametrize("cus", (256, 304, 32, 20))
def test_the_arms_the_gpu_cases_name(cus):
    n = last_packed_rows(cus)
    assert plan(n, 2, cus).packed and plan(n, 2, cus).share_rows == 64512 and not plan(n + 1, 2, cus).packed
    assert plan(64 * BLOCK * cus, 65536, cus).share_rows == 65536 and not plan(64 * BLOCK * cus, 65536, cus).packed
    for arm in ("packed, atomic", "packed, slab", "packed, slab, last window of one bin", "unpacked, atomic",
                "unpacked, slab"):
        rows, bins = arm_rows(arm, cus)
        p = plan(rows, bins, cus)
        assert p.packed == arm.startswith("packed") and p.slab == ("slab" in arm), arm
        assert p.ratio >= 2 if p.slab else p.ratio <= 0.5, arm
    assert plan(200_000, 10_923, cus, weighted=True).window == 10_922


@pytest.mark.parametrize("cus", (256, 20))
def test_a_slab_flush_runs_on_a_grid_of_one_workgroup_a_cu(cus):
    """A grid below the CU count has at most 1024 rows a workgroup and never reaches the slab, so the fold's eight
    chunks are ragged only where the CU count is no multiple of 8."""
    for blocks in range(1, cus):
        for bins in (2, 64, 1024, 4096, 16384, 32768, 65536, 65537, 1 << 20):
            for n in ((blocks - 1) * BLOCK + 1, blocks * BLOCK):
                assert plan(n, bins, cus).grid == blocks and not plan(n, bins, cus).slab
    p = plan(slab_rows(cus, 65536), 65536, cus)
    assert p.slab and p.grid == cus and (p.grid % FOLD_CHUNKS != 0) == (cus == 20)
