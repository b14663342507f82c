"""Reference of the span store's expiry (include/zkspans.h, "Expiry") in plain Python integers, on top of
tests/spref.py's rows. Nothing of the library's span-store code is imported."""
from tests.spref import INT64_MIN, TIMED


def ends(rows):
    """trace id -> its end: the maximum last_ts over its TIMED rows, INT64_MIN for a trace without one.
    The times of an untimed row are never read."""
    out = {}
    for r in rows:
        e = r[4] if r[6] & TIMED else INT64_MIN
        out[r[0]] = max(out.get(r[0], INT64_MIN), e)
    return out


def survivors(rows, min_end, pins=None):
    """The rows that stay, in their order: a trace stays whole exactly when its end is >= its cutoff,
    min_end or the pin's own value."""
    pins = pins or {}
    end = ends(rows)
    return [r for r in rows if end[r[0]] >= pins.get(r[0], min_end)]


def timed_ids(rows):
    """The trace ids with a timed row: the ones a duration index holds."""
    return {r[0] for r in rows if r[6] & TIMED}
