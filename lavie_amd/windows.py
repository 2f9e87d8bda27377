"""Frame-window schedules for sampling a clip longer than the model's window (MultiDiffusion along the frame axis, the context
windows of AnimateDiff-style tools): which frames each UNet forward sees and how much each of its frames weighs where windows
overlap.  Host arithmetic only; the fusion itself is `ops.window_step` (csrc/sampler_window.hip)."""
from typing import List

from ._lib import WINDOW_MAX_COVER, WINDOW_MAX_LENGTH, WINDOW_MAX_WINDOWS

PROFILES = ("uniform", "triangle")


def window_starts(total: int, length: int, stride: int) -> List[int]:
    """First frames of the windows of `length` frames that tile `total` frames at `stride`: 0, stride, 2 stride, ...; the last
    start is clamped to total - length (so the last window ends on the last frame) and duplicates are dropped.  Raises ValueError
    when the schedule leaves the step kernel's limits (`check_schedule`)."""
    total, length, stride = int(total), int(length), int(stride)
    if length < 1 or total < length:
        raise ValueError(f"window length={length} must lie in 1..total={total}")
    if stride < 1:
        raise ValueError(f"window stride={stride} must be >= 1")
    if stride > length:
        raise ValueError(f"window stride={stride} above length={length} would leave frames uncovered")
    last = total - length
    starts = []
    for s in range(0, last + stride, stride):
        s = min(s, last)
        if not starts or s != starts[-1]:
            starts.append(s)
    check_schedule(total, length, starts)
    return starts


def cover_counts(total: int, length: int, starts) -> List[int]:
    """How many windows cover each of the `total` frames."""
    return [sum(1 for s in starts if s <= f < s + length) for f in range(total)]


def check_schedule(total: int, length: int, starts) -> None:
    """ValueError unless the step kernel takes the schedule: 1..32 windows of 1..64 frames, strictly ascending starts inside the
    clip, every frame covered by at least one and at most 4 windows."""
    starts = list(starts)
    if not 1 <= length <= WINDOW_MAX_LENGTH:
        raise ValueError(f"window length={length} outside 1..{WINDOW_MAX_LENGTH}")
    if not 1 <= len(starts) <= WINDOW_MAX_WINDOWS:
        raise ValueError(f"{len(starts)} windows, the step kernel takes 1..{WINDOW_MAX_WINDOWS}: use a longer stride")
    if starts[0] < 0 or any(b <= a for a, b in zip(starts, starts[1:])) or starts[-1] + length > total:
        raise ValueError(f"window starts {starts} must be strictly ascending and stay inside 0..{total - length}")
    counts = cover_counts(total, length, starts)
    if min(counts) < 1:
        raise ValueError(f"frame {counts.index(0)} is covered by no window (starts {starts}, length {length})")
    if max(counts) > WINDOW_MAX_COVER:
        raise ValueError(f"frame {counts.index(max(counts))} would be covered by {max(counts)} windows, at most {WINDOW_MAX_COVER}: "
                         f"use a stride of at least {-(-length // WINDOW_MAX_COVER)}")


def window_profile(length: int, kind: str = "triangle") -> List[float]:
    """The weight of a window's i-th frame: "uniform" = 1 everywhere; "triangle" = min(i + 1, length - i), largest in the middle
    of the window, where its temporal attention sees the most context on both sides.  Positive and symmetric."""
    if length < 1:
        raise ValueError(f"window length={length} must be >= 1")
    if kind == "uniform":
        return [1.0] * length
    if kind == "triangle":
        return [float(min(i + 1, length - i)) for i in range(length)]
    raise ValueError(f"window_weights={kind!r} must be one of {PROFILES}")
