"""Index and span retention: one time-to-live applied to the three trace indices (TraceNameIndex,
TraceAnnotationIndex, TraceDurationIndex).

Every index column the reference's Cassandra store writes carries indexTtl, 3 days by default
(CassieSpanStore.scala:48; CassandraIndex.scala:42), and its Storage trait exposes getDataTimeToLive
(QueryService.scala:357-360). IndexRetention is that policy for the device indices: expire(now_us) cuts
all three at now_us - ttl. The cut is by an entry's own timestamp (a trace's own end), not by the time it
was written: see "Expiry" in include/zkindex.h, zkannindex.h and zkduration.h. With ONE cutoff on all
three, every (trace_id, ts) the name or annotation index still returns has its trace in the duration
index (an entry's ts is at most its trace's end), so sortTraceIds loses none of them.

SpanRetention is the same for the span data (TraceSpanStore): spanTtl, 7 days by default, whole traces by
their end, and a ttl of its own for a pinned trace (setTimeToLive / getTimeToLive). Given annotation stores
(TraceAnnotationStore) as well, it cuts them with the same cutoff and the same pins, after the span stores:
a trace's end is the same in both (the maximum ts of its annotations is the decoder's last_ts), so stores fed
from the same decode_annotated batches keep holding the same traces ("Expiry" in include/zkannots.h).

The job drivers are not wired to either: the caller decides when to expire.
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


SPAN_TTL_SECONDS = 7 * 24 * 3600  # the reference's spanTtl: 7 days


def _ttl(ttl_seconds) -> int:
    ttl = int(ttl_seconds)
    if ttl <= 0 or ttl != ttl_seconds:
        raise ValueError("ttl_seconds is a positive whole number of seconds")
    return ttl


def _cutoff(now_us: int, ttl: int) -> int:
    return max(INT64_MIN, min(INT64_MAX, int(now_us) - ttl * 1_000_000))


class SpanRetention:
    """The span data's time to live over one TraceSpanStore or a list of sharded ones (anything with
    tracesExist(ids) -> set and expire(min_end, pins) -> int): the reference writes every span column with
    spanTtl, 7 days (CassieSpanStore.scala:47), and lets one trace's ttl be set and read
    (SpanStore.setTimeToLive / getTimeToLive, the query service's setTraceTimeToLive / getTraceTimeToLive:
    the web UI's "pin this trace").

    expire(now_us) removes every trace whose END (see "Expiry" in include/zkspans.h) is below
    now_us - ttl, whole; a pinned trace is judged by its own ttl. Every shard gets every pin; a shard
    ignores the pins of traces it does not hold. With this ttl at or above IndexRetention's, every id an
    index returns has its whole trace in the store.

    Stated departure: a pin covers the whole trace, fragments observed later included. Cassandra gives
    later columns spanTtl again and getTimeToLive answers the minimum over the columns.

    annotations: None, one TraceAnnotationStore or a list of sharded ones (anything with
    expire(min_end, pins) -> int). expire(now_us) gives each of them the span stores' cutoff and pins, after
    the span stores. The pins' bookkeeping (which traces exist, whose pins are dropped) stays with the span
    stores."""

    MAX_PINS = 4096  # ZK_SP_MAX_PINS (= ZK_AN_MAX_PINS)

    def __init__(self, ttl_seconds: int = SPAN_TTL_SECONDS, spans=None, annotations=None):
        self.ttl_seconds = _ttl(ttl_seconds)
        self.spans = _handles(spans)
        self.annotations = _handles(annotations)
        self.pins = {}  # trace id -> ttl in seconds

    def _exists(self, trace_id: int) -> bool:
        return any(trace_id in h.tracesExist([trace_id]) for h in self.spans)

    def setTimeToLive(self, trace_id: int, ttl_seconds: int) -> None:
        """SpanStore.setTimeToLive: pin the trace to a ttl of its own. A trace that is in no shard gets
        no pin (a Cassandra row without columns takes no ttl either). At most MAX_PINS traces are pinned
        at a time (one expiry carries them all: ZK_SP_MAX_PINS); one more is a ValueError."""
        ttl = _ttl(ttl_seconds)
        if self._exists(int(trace_id)):
            if int(trace_id) not in self.pins and len(self.pins) >= self.MAX_PINS:
                raise ValueError("more than ZK_SP_MAX_PINS pinned traces")
            self.pins[int(trace_id)] = ttl

    def getTimeToLive(self, trace_id: int) -> int:
        """SpanStore.getTimeToLive: the trace's pin, else the default; ValueError when the trace is not in
        the store (the reference's exception and message)."""
        if not self._exists(int(trace_id)):
            raise ValueError(f"The trace {trace_id} does not have any ttl set!")
        return self.pins.get(int(trace_id), self.ttl_seconds)

    def cutoff(self, now_us: int) -> int:
        """now_us - ttl in microseconds, held inside int64 (below INT64_MIN nothing is older)."""
        return _cutoff(now_us, self.ttl_seconds)

    def expire(self, now_us: int) -> dict:
        """Apply cutoff(now_us), and now_us - ttl_i for every pin, to every shard: {"cutoff", "spans"}, the
        default cutoff and the entries (fragments) removed, summed over the shards. The pins of traces that
        no longer exist are dropped afterwards. With annotation stores, every one of them gets the same
        cutoff and pins after the span stores, and the result gains "annotations", the rows removed, summed
        over their shards."""
        c = self.cutoff(now_us)
        pins = {t: _cutoff(now_us, ttl) for t, ttl in self.pins.items()}
        removed = sum(int(h.expire(c, pins)) for h in self.spans)
        rows = sum(int(h.expire(c, pins)) for h in self.annotations)
        ids = list(self.pins)
        alive = set()
        for h in self.spans:
            alive |= set(h.tracesExist(ids)) if ids else set()
        self.pins = {t: ttl for t, ttl in self.pins.items() if t in alive}
        out = {"cutoff": c, "spans": removed}
        if self.annotations:
            out["annotations"] = rows
        return out


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
