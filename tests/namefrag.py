"""Stored span fragments WITH span names (test infrastructure): a small SpanColumns batch whose
flags carry name ids in bits 16..31 (tests/rpc_rows.py assign_names) -> one thrift Span per record
through tests/thriftenc.py, optionally Snappy-compressed, as the ingest decoders read them.

Record i becomes the Span {traceId, name, id, [parentId], two core annotations}: "sr" at first_ts and
"ss" at last_ts with the host {127.0.0.1:9410, service_name(service_id)} when the record's service is
the server side, "cs" / "cr" when it is the client side, and two host-less "custom" annotations when
it has no service. The name is names[id - 1] for a name id > 0; id 0 alternates between "" and
"Unknown" (the two names mergeSpan never selects), by record index. What the bytes decode to is
whatever the HOST decoder says: the device tests compare against it on the same bytes, by name."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from oracle.spans import Annotation, Endpoint, Span
from tests import thriftenc
from tests.bulkfrag import service_name
from zipkin_amd import _abi

NO_NAMES = ("", "Unknown")


def span_of(cols, i: int, name) -> Span:
    f = int(cols.flags[i])
    first, last = int(cols.first_ts[i]), int(cols.last_ts[i])
    assert 0 < first <= last, "annotation timestamps must be positive"
    if f & (_abi.ZK_F_SVC_SERVER | _abi.ZK_F_SVC_CLIENT):
        host = Endpoint(0x7F000001, 9410, service_name(int(cols.service_id[i])))
        a, b = ("sr", "ss") if f & _abi.ZK_F_SVC_SERVER else ("cs", "cr")
        anns = (Annotation(first, a, host), Annotation(last, b, host))
    else:
        anns = (Annotation(first, "custom", None), Annotation(last, "custom", None))
    parent = int(cols.parent_id[i]) if f & _abi.ZK_F_HAS_PARENT else None
    return Span(int(cols.trace_id[i]), name, int(cols.span_id[i]), parent, anns)


def record_names(cols, names: Sequence) -> List:
    """the name each record's fragment carries"""
    ids = (cols.flags.astype(np.uint32) >> np.uint32(16)).tolist()
    return [names[k - 1] if k else NO_NAMES[i & 1] for i, k in enumerate(ids)]


def blobs(cols, names: Sequence, *, snappy: bool = True) -> List[bytes]:
    out = []
    for i, nm in enumerate(record_names(cols, names)):
        b = thriftenc.span(span_of(cols, i, nm))
        out.append(thriftenc.snappy(b) if snappy else b)
    return out


def pack(blobs_: Sequence[bytes]):
    """-> (buf uint8, offsets int64[n + 1]) host arrays"""
    offsets = np.zeros(len(blobs_) + 1, np.int64)
    if blobs_:
        offsets[1:] = np.cumsum([len(b) for b in blobs_])
    return np.frombuffer(b"".join(blobs_) or b"\0", dtype=np.uint8).copy(), offsets
