"""ROCm runtime setting the hipGraph replay of the guidance networks depends on.

ROCm 7's HIP runtime pre-forms the AQL packets of a graph's kernel nodes when the graph is instantiated
("graph packet capture", flag DEBUG_CLR_GRAPH_PACKET_CAPTURE, on by default).  With it on, replays of the captured
SD-2.1 UNet / VAE graphs were observed to run kernels with corrupted arguments -- NaN or all-zero outputs from
kernels that are bit-exact when launched eagerly or from the same graph in a fresh process -- once the process
had done other GPU work before the capture (an earlier, smaller guidance instance followed by a render call;
DESIGN.md section 6, tools/graph_replay_check.py reproduces it).  With the flag off the same graphs replay
correctly and the step time is unchanged (54.5 ms either way), so the package turns it off.

The HIP runtime reads the flag once, when it initialises (first HIP call, e.g. torch.cuda.is_available()).
``configure()`` therefore runs at package import and only claims success if the flag is in place before the
HSA runtime has opened /dev/kfd; otherwise ``graph_replay_safe()`` is False and the guidance runs eagerly.
"""
from __future__ import annotations

import contextlib
import gc
import os

FLAG = "DEBUG_CLR_GRAPH_PACKET_CAPTURE"
_safe = None


def _hsa_runtime_started() -> bool:
    try:
        for fd in os.listdir("/proc/self/fd"):
            try:
                if os.readlink(os.path.join("/proc/self/fd", fd)) == "/dev/kfd":
                    return True
            except OSError:
                continue
    except OSError:
        pass
    return False


def configure() -> bool:
    """Idempotent; returns whether hipGraph replay may be used in this process."""
    global _safe
    if _safe is not None:
        return _safe
    value = os.environ.get(FLAG)
    if value is None:
        if _hsa_runtime_started():
            _safe = False          # too late: the runtime has already read its flags
        else:
            os.environ[FLAG] = "0"
            _safe = True
    else:
        _safe = value == "0"       # set by the launcher / bench.py / conftest before any HIP call, or a user override
    if os.environ.get("GD_HIP_GRAPHS_FORCE") == "1":
        _safe = True
    return _safe


def graph_replay_safe() -> bool:
    return configure()


@contextlib.contextmanager
def capture_guard():
    """Around a hipGraph capture (``torch.cuda.graph`` / ``make_graphed_callables``): collect Python's cyclic garbage
    BEFORE the capture and keep the cyclic collector off during it.  torch no longer collects on entering a capture, and
    a collection that happens to run while a stream is capturing may free what a dead cycle still holds -- other
    CUDAGraphs with their memory pools, streams, events -- from inside the capture; the HIP runtime aborts on that.
    When a collection runs depends on allocation counts only, so any unrelated change can move it into a capture."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()
