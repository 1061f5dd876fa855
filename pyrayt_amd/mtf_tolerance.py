"""``device_run``: ``prt_frame_mtf_tolerance`` on per-group trials.  The call itself is frame.py's, where every other
``prt_frame_*`` call is; this name is kept for those who hand the entry point trials that differ by group."""
from .frame import _mtf_tolerance_run as device_run  # noqa: F401
