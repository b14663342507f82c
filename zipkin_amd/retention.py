"""Index retention: one time-to-live applied to the three trace indices (TraceNameIndex,
TraceAnnotationIndex, TraceDurationIndex).

Every index column the reference's Cassandra store writes carries indexTtl, 3 days by default
(CassieSpanStore.scala:48; CassandraIndex.scala:42), and its Storage trait exposes getDataTimeToLive
(QueryService.scala:357-360). IndexRetention is that policy for the device indices: expire(now_us) cuts
all three at now_us - ttl. The cut is by an entry's own timestamp (a trace's own end), not by the time it
was written: see "Expiry" in include/zkindex.h, zkannindex.h and zkduration.h. With ONE cutoff on all
three, every (trace_id, ts) the name or annotation index still returns has its trace in the duration
index (an entry's ts is at most its trace's end), so sortTraceIds loses none of them.

The job drivers are not wired to it: the caller decides when to expire.
"""
from __future__ import annotations

from typing import List

INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
DEFAULT_TTL_SECONDS = 3 * 24 * 3600  # the reference's IndexTtl: 3 days


def _handles(x) -> List:
    """None, one handle or a sequence of (sharded) handles -> a list."""
    if x is None:
        return []
    if isinstance(x, (list, tuple)):
        return list(x)
    return [x]


class IndexRetention:
    """ttl_seconds over `names`, `annotations` and `durations`: each None, one handle or a list of
    sharded handles (anything with expire(cutoff) -> int)."""

    def __init__(self, ttl_seconds: int = DEFAULT_TTL_SECONDS, names=None, annotations=None, durations=None):
        ttl = int(ttl_seconds)
        if ttl <= 0 or ttl != ttl_seconds:
            raise ValueError("ttl_seconds is a positive whole number of seconds")
        self.ttl_seconds = ttl
        self.names = _handles(names)
        self.annotations = _handles(annotations)
        self.durations = _handles(durations)

    def getDataTimeToLive(self) -> int:
        """Storage.getDataTimeToLive: the time to live in seconds."""
        return self.ttl_seconds

    def cutoff(self, now_us: int) -> int:
        """now_us - ttl in microseconds, held inside int64 (below INT64_MIN nothing is older)."""
        return max(INT64_MIN, min(INT64_MAX, int(now_us) - self.ttl_seconds * 1_000_000))

    def expire(self, now_us: int) -> dict:
        """Apply cutoff(now_us) to every handle: {"cutoff", "names", "annotations", "durations"}, the
        cutoff and the entries (traces) removed from each kind of index, summed over its shards. The
        duration indices go last, so the invariant holds at every point in between."""
        c = self.cutoff(now_us)
        out = {"cutoff": c}
        for kind in ("names", "annotations", "durations"):
            out[kind] = sum(int(h.expire(c)) for h in getattr(self, kind))
        return out
