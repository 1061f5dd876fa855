"""The selection check that the five passes over the selected rows of a sensitivity call share (selection_check of
pyrayt_amd/csrc/prt_selection.hpp), through each entry point of the built library, without a device: each of its four
faults, alone in a call that is otherwise sound, is refused with -1 and the message that names the entry."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAULTS = (  # (what changes in the sound call: 4 rows, 4 of them selected, one group, weights in column 1; the message)
    (dict(n_selected=5, first=(0, 5)), "{name}: more selected rows than rows"),
    (dict(first=(0, 3)), "{name}: group_first runs from 0 to n_selected"),
    (dict(first=(1, 4)), "{name}: group_first runs from 0 to n_selected"),
    (dict(n_groups=2, first=(0, 5, 4)), "{name}: group_first does not decrease"),
    (dict(weight=15), "weight_column: 0..14 or -1"),
    (dict(weight=-2), "weight_column: 0..14 or -1"),
)


def entries(lib):
    """``{name: call(n_selected, first, n_groups, weight)}``: every entry on 4 rows with every buffer in place."""
    buf = np.zeros(64)
    p = buf.ctypes.data
    lam, uv, axes, nu, theta = np.array([0.55, 0.65]), np.zeros(2), np.eye(3).ravel(), np.array([0.0, 1.0]), np.zeros(1)

    def head(n_selected, first, n_groups, weight):
        return 0, p, 4, 4, p, n_selected, first.ctypes.data, n_groups, weight

    sampling = (axes.ctypes.data, nu.ctypes.data, 2, theta.ctypes.data, 1, theta.ctypes.data, 1)
    colours = (lam.ctypes.data, 2, 1000.0)
    return {
        "mtf_gradient": lambda *s: lib.prt_frame_mtf_gradient(*head(*s), p, p, 2, None, *sampling, p, p, p, p, None),
        "psf_gradient": lambda *s: lib.prt_frame_psf_gradient(*head(*s), p, p, p, p, None, 2, *colours, 8, 8, 1e-3, 1e-3,
                                                              uv.ctypes.data, p, p, p, p, p, p, p, None),
        "tolerance_moments": lambda *s: lib.prt_frame_tolerance_moments(*head(*s), p, p, 2, *colours, p, p, None),
        "tolerance": lambda *s: lib.prt_frame_tolerance(*head(*s), p, p, 2, *colours, p, 3, p, p, p, p, None),
        "mtf_tolerance": lambda *s: lib.prt_frame_mtf_tolerance(*head(*s), p, p, 2, None, *sampling, p, 3, 1, p, p, p, p, p,
                                                                None),
    }


def test_every_pass_over_selected_rows_refuses_a_bad_selection_in_the_same_words():
    from pyrayt_amd import engine

    if not os.path.exists(engine.LIB_PATH):
        pytest.skip("libprt_hip.so is not built")
    lib = engine.library()
    table = entries(lib)
    assert sorted(table) == ["mtf_gradient", "mtf_tolerance", "psf_gradient", "tolerance", "tolerance_moments"]
    for name, call in table.items():
        for fault, message in FAULTS:
            sound = dict(n_selected=4, first=(0, 4), n_groups=1, weight=1)
            sound.update(fault)
            first = np.array(sound["first"], dtype=np.int64)
            assert call(sound["n_selected"], first, sound["n_groups"], sound["weight"]) == -1, (name, fault)
            assert lib.prt_last_error().decode() == message.format(name=name), (name, fault, lib.prt_last_error())


def test_the_selection_check_is_written_once():
    csrc = os.path.join(ROOT, "pyrayt_amd", "csrc")
    holders = [name for name in sorted(os.listdir(csrc)) if name.endswith((".hpp", ".hip"))
               and "group_first does not decrease" in open(os.path.join(csrc, name)).read()]
    assert holders == ["prt_selection.hpp"]
