"""Reference of the annotation store's expiry (include/zkannots.h, "Expiry") in plain Python integers, on top
of tests/anref.py's row tuples (trace_id, span_id, ts, value, ipv4, service_id, bits). Nothing of the library
is imported."""
from tests.anref import INT64_MIN


def ends(rows):
    """trace id -> its end: the maximum ts over its rows. Every row is timed."""
    out = {}
    for r in rows:
        out[r[0]] = max(out.get(r[0], INT64_MIN), r[2])
    return out


def survivors(rows, min_end, pins=None):
    """The rows that stay, in their order: a trace stays whole exactly when its end is >= its cutoff,
    min_end or the pin's own value."""
    pins = pins or {}
    end = ends(rows)
    return [r for r in rows if end[r[0]] >= pins.get(r[0], min_end)]
