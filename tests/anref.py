"""Reference of the annotation store by trace id (include/zkannots.h) in plain Python integers.

The store is a list (a multiset) of row tuples (trace_id, span_id, ts, value, ipv4, service_id, bits): every
row of every observed batch. Nothing of the library's annotation-store code is imported."""
import numpy as np

from tests.spref import INT64_MAX, INT64_MIN, M64, bucket, id_in_bucket  # noqa: F401  (the span store's bucket function)

COLS = ("trace_id", "span_id", "ts", "value", "ipv4", "service_id", "bits")
DTYPES = (np.uint64, np.uint64, np.int64, np.uint64, np.uint32, np.uint32, np.uint32)
KIND_MASK, HAS_HOST, PORT_SHIFT = 7, 8, 16
OTHER, CS, CR, SR, SS = 0, 1, 2, 3, 4


def key(r):
    """The header's canonical order inside a trace."""
    _, span, ts, value, ipv4, svc, bits = r
    return (span, ts, bits & KIND_MASK, value, ipv4, bits >> PORT_SHIFT, svc, bits & HAS_HOST, bits)


def rows_of(batches):
    """The store after observing the batches (one batch or a sequence): a list of row tuples."""
    if hasattr(batches, "trace_id"):
        batches = [batches]
    out = []
    for c in batches:
        out += list(zip(*[getattr(c, k).tolist() for k in COLS]))
    return out


def gather(store, ids):
    """(counts, rows): per asked id its rows in canonical order, the asked ids' rows one after another."""
    by = {}
    for r in store:
        by.setdefault(r[0], []).append(r)
    counts, rows = [], []
    for i in ids:
        mine = sorted(by.get(i, []), key=key)
        counts.append(len(mine))
        rows += mine
    return counts, rows


def by_trace_ids(store, ids):
    """getAnnotationsByTraceIds: one row list per asked id, [] for an id without rows."""
    by = {}
    for r in store:
        by.setdefault(r[0], []).append(r)
    return [sorted(by.get(i, []), key=key) for i in ids]


def noise(trace_id, seed=0):
    """Seven numpy columns with the given trace ids; every other column is noise over its whole range, a few
    span ids and timestamps per trace so that the order's later keys decide."""
    trace_id = np.asarray(trace_id, np.uint64)
    n = len(trace_id)
    rng = np.random.default_rng(seed + 11 * n)
    return [trace_id,
            rng.integers(0, 4, n, dtype=np.uint64) * np.uint64(2 ** 62 + 1),
            rng.integers(-2, 2, n, dtype=np.int64) * np.int64(2 ** 62),
            rng.integers(0, 3, n, dtype=np.uint64) * np.uint64(2 ** 63 - 5),
            rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
            rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
            rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)]
