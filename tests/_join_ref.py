"""NumPy reference of the segment join stage (``fq3_join_*``, include/fq3hip.h), straight from the contract and on the whole stream
at once: a list of (segment samples, pause) -> the joined array.  It knows nothing of pushes, queues or state."""
from __future__ import annotations

import numpy as np


def hop_activity(x: np.ndarray, H: int, threshold: float) -> np.ndarray:
    """bool[ceil(n / H)]: some sample of the hop has |x| >= threshold (a NaN compares false)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n_hops = -(-x.size // H)
    with np.errstate(invalid="ignore"):
        hit = np.abs(x) >= np.float32(threshold)
    return np.array([bool(hit[h * H: (h + 1) * H].any()) for h in range(n_hops)], dtype=bool)


def segment_span(x: np.ndarray, H: int, threshold: float, lead_hops: int, tail_hops: int, hold_hops: int):
    """``(first, stop)`` sample range a segment contributes, or None when it has no active hop."""
    act = hop_activity(x, H, threshold)
    if not act.any():
        return None
    idx = np.flatnonzero(act)
    a, b, last = int(idx[0]), int(idx[-1]), act.size - 1
    L = last - b
    R = min(max(0, L - tail_hops), hold_hops)
    return max(0, a - lead_hops) * H, min(np.asarray(x).size, (last - R + 1) * H)


def join(segments, in_rate: int, threshold: float, lead_hops: int, tail_hops: int, hold_hops: int, last_pause: bool = False) -> np.ndarray:
    """``segments``: [(float32 array, pause_samples), ...].  The last segment ends the stream (``end == 2``: its pause is not
    written) unless ``last_pause``."""
    H = in_rate // 100
    out = []
    for k, (x, pause) in enumerate(segments):
        x = np.asarray(x, dtype=np.float32).reshape(-1)
        span = segment_span(x, H, threshold, lead_hops, tail_hops, hold_hops)
        if span is None:
            continue
        out.append(x[span[0]: span[1]])
        if k + 1 < len(segments) or last_pause:
            out.append(np.zeros(int(pause), dtype=np.float32))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.float32)


def bound(in_rate: int, lead_hops: int, hold_hops: int, n_in: int, pause: int) -> int:
    """``fq3_join_bound``: the push's samples, everything the object may still hold, the pause"""
    return n_in + (hold_hops + lead_hops + 1) * (in_rate // 100) + pause
