"""prt_frame_histogram's plan (pyrayt_amd/csrc/prt_histogram.hpp) restated in Python: whether two 16-bit tallies share a
word, the window, the workgroups per CU, the grid and the flush, for a given CU count; and the row counts that enter each
arm.  tests/test_host_histogram_partitions.py holds it to the source text; tests/test_gpu_histogram_partitions.py asserts
every case's arm from it before it calls the device."""
import collections
import math

BLOCK, LDS_BYTES, MAX_PER_CU, FOLD_CHUNKS = 1024, 128 * 1024, 2, 8   # kHistBlock, kHistLdsBytes, ..., kHistFoldChunks
Plan = collections.namedtuple("Plan", "packed window windows per_cu grid slab ratio share_rows")



def plan(n_rows, bins, cus, weighted=False):
    """What prt_frame_histogram decides for n_rows rows and ``bins`` bins in all: two 16-bit tallies a word or not, the
    window, the workgroups per CU and the grid, and the flush -- the slab where 90 touched share > 10 + 20 share
    (ratio: the left side over the right).  share_rows: the most rows one workgroup counts."""
    blocks = -(-n_rows // BLOCK)
    one_per_cu = min(blocks, cus)
    per_thread = -(-n_rows // (one_per_cu * BLOCK))
    packed = not weighted and per_thread * BLOCK < 65536
    window = min(bins, 2 * LDS_BYTES // 4 if packed else LDS_BYTES // (12 if weighted else 4))
    lds = window * 12 if weighted else ((window + 1) // 2 * 4 if packed else window * 4)
    per_cu = 1 if packed else max(1, min(MAX_PER_CU, 160 * 1024 // max(lds, 1)))
    grid = min(blocks, cus * per_cu)
    per_window_rows = n_rows / grid * (window / bins)
    touched, share = 1.0 - math.exp(-8.0 * per_window_rows / window), window / 65536.0
    ratio = 90.0 * touched * share / (10.0 + 20.0 * share)
    return Plan(packed, window, -(-bins // window), per_cu, grid, not weighted and ratio > 1, ratio,
                -(-n_rows // (grid * BLOCK)) * BLOCK)


def last_packed_rows(cus):
    return 63 * BLOCK * cus


def slab_rows(cus, bins):
    """The smallest k * 1024 * cus + 513 rows at which packed tallies of ``bins`` bins go to the slab with the
    predicate a factor of two clear."""
    for k in range(1, 63):
        n = k * BLOCK * cus + 513
        p = plan(n, bins, cus)
        if p.slab and p.ratio >= 2:
            assert p.packed
            return n
    raise AssertionError("no packed row count reaches the slab")


def arm_rows(arm, cus):
    """(n_rows, bins) that enter the arm on this CU count."""
    if arm == "packed, atomic":           # a full packed window thinly filled
        return 1171 * cus + 37, 65536
    if arm == "packed, slab":
        return slab_rows(cus, 65536), 65536
    if arm == "packed, slab, last window of one bin":  # 65 537 bins: the last window is half a word
        return slab_rows(cus, 65537), 65537
    if arm == "unpacked, atomic":
        return last_packed_rows(cus) + 1, 64
    assert arm == "unpacked, slab"
    return last_packed_rows(cus) + 1, 65536
