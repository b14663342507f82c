"""TEST INFRASTRUCTURE ONLY -- held traces (ZK_BATCH_CONTINUES) and max_trace_records at their bounds.

Three things, none of which touches the GPU or the library's device code:

`expected`: the whole-stream semantics. The stream is trace-clustered, so its traces are the maximal
runs of equal traceId over the concatenation of all batches; every run longer than L is removed
(`trace_too_large` = the number removed), the CPU oracle aggregates what is left. It knows nothing
of where a reader cut the stream, which is the contract: the result does not depend on the cuts.

`trace_of`: a trace of an exact record count whose every child changes a cell when it is lost,
doubled or joined with half of its fragments.

`classify`: a host walk over the batches of a stream that names, from the inputs alone (run lengths,
traceIds, flags, L), the branch each batch must take in k_carry_plan (zipkin_amd/csrc/zk_cluster.hip),
so that tests/test_carry_cases.py can say which branches CASES reaches."""
from __future__ import annotations

import numpy as np

from oracle import oracle
from zipkin_amd import _abi
from zipkin_amd.columns import COLUMNS, SpanColumns, tracegen_host

SERVER = _abi.ZK_F_HAS_ANNOTATIONS | _abi.ZK_F_SVC_SERVER | (1 << _abi.ZK_F_SR_SHIFT) | (1 << _abi.ZK_F_SS_SHIFT)
CLIENT = _abi.ZK_F_HAS_ANNOTATIONS | _abi.ZK_F_SVC_CLIENT | (1 << _abi.ZK_F_CS_SHIFT) | (1 << _abi.ZK_F_CR_SHIFT)
U64 = (1 << 64) - 1
ROUND = 256  # records per search round of the plan (one workgroup)


def runs(trace_id):
    """(starts, lengths) of the maximal runs of equal traceId."""
    t = np.asarray(trace_id)
    if t.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    starts = np.flatnonzero(np.r_[True, t[1:] != t[:-1]])
    return starts, np.diff(np.r_[starts, t.size])


def reduced(stream_cols, L):
    """(the stream without its runs longer than L, the number of runs removed)."""
    cols = stream_cols if isinstance(stream_cols, SpanColumns) else SpanColumns.concat(stream_cols)
    starts, lens = runs(cols.trace_id)
    keep = np.ones(len(cols), bool)
    for s, n in zip(starts[lens > L], lens[lens > L]):
        keep[s:s + n] = False
    return cols.take(keep), int((lens > L).sum())


def expected(stream_cols, S, L):
    """The job over the whole stream (one SpanColumns or a list of batches): an oracle result whose
    `trace_too_large` counts the traces longer than L, none of which is aggregated."""
    kept, removed = reduced(stream_cols, L)
    ref = oracle.aggregate(kept, S)
    ref.stats["trace_too_large"] = removed
    return ref


def expected_cells(ref):
    """{(parent, child): (n, S1..S4)} of an oracle result, the form zipkin_amd.table.decode gives."""
    S = ref.S
    return {(int(c) // S, int(c) % S): ref.power_sums(int(c)) for c in ref.present_cells()}


def trace_of(tid, records, S, svc_root=0, t0=1_000_000):
    """A trace of exactly `records` records as SpanColumns: a root, then children of two fragments
    each (the server's, then the client's, so a cut can fall between them), and one single-fragment
    child when the parity needs it. Child i hangs off child i - 1 unless i % 4 == 0 (then off the
    root), so any six consecutive records hold a parent with a child: a piece of the trace joined on
    its own makes links of its own. Child i has service 1 + i % (S - 1) and a merged duration of
    1000 + 3 i, its server fragment alone 100 + i: a lost, doubled or half-joined child changes a
    cell."""
    assert records >= 1 and S >= 3
    root = (tid ^ 0xABCDEF) & U64
    rows = [(tid, root, 0, t0, t0 + 10_000_000, svc_root, SERVER)]
    pairs, single = divmod(records - 1, 2)
    prev = root
    for i in range(pairs + single):
        sid = (tid * 1_000_003 + i * 7919 + 1) & U64
        parent = root if i % 4 == 0 else prev
        svc = 1 + i % (S - 1)
        cs = t0 + 10 + 2 * i
        rows.append((tid, sid, parent, cs + 5, cs + 105 + i, svc, SERVER | _abi.ZK_F_HAS_PARENT))
        if i < pairs:
            rows.append((tid, sid, parent, cs, cs + 1000 + 3 * i, svc, CLIENT | _abi.ZK_F_HAS_PARENT))
        prev = sid
    assert len(rows) == records
    c = SpanColumns.empty(records)
    for (k, dt), v in zip(COLUMNS, zip(*rows)):
        getattr(c, k)[:] = np.array(v, dtype=np.uint64 if dt == np.uint64 else dt)
    return c


# ---------------------------------------------------------------------------------------------
# the classifier
CLASSES = (
    "lead_round1", "lead_round2", "lead_unknown", "tail_round1", "tail_round2", "tail_unknown",
    "one_run_short_fresh", "one_run_short_held", "one_run_long_fresh", "one_run_long_held",
    "append_to_L", "append_to_L_plus_1", "held_L", "held_L_plus_1",
    "dropped_rest_leading", "dropped_whole_batch", "dropped_then_other_trace",
    "long_tail_continues", "n1", "n2", "empty_continues", "empty_plain",
)


def classify(L, parts, flags):
    """-> one set of class names per batch, then one for the end of the stream (finalize).

    parts: the batches (SpanColumns), flags: ZK_BATCH_CONTINUES of each. The walk keeps what the
    contract says must be remembered between batches: the traceId whose trace is open, how many of its
    records are held (`n`), whether it was already found longer than L (`dropped`) and whether the
    held records came from one batch's tail alone (`plain`).

    lead_* / tail_*: where the first / last trace boundary of a batch of several runs lies: within
      the first 256-record search round from that end, in a later round, or beyond the L + 1 records
      searched (the run is then only known to be long).
    one_run_*: the batch is one run, of at most L + 1 records (short) or more (long), while a trace
      of the same traceId is open (held) or not (fresh).
    append_to_L / append_to_L_plus_1: the held records plus the batch's leading run are exactly L
      (the trace still fits) or L + 1 (it no longer does).
    held_L / held_L_plus_1: a batch's last run of exactly that length was held back and is joined as
      it is (the largest trace that fits, and the largest run that is held at all).
    dropped_*: the leading run belongs to a trace already found too long: the run is skipped; it is
      the whole batch, or the batch goes on to another trace.
    long_tail_continues: a batch that continues ends in a run of more than L + 1 records, so the run
      is not held; the trace is too long already and its rest arrives in the next batch.
    n1, n2, empty_*: batches of one, two and no records."""
    out = []
    tid, n_held, dropped, plain = None, 0, False, False

    def flush(cls):
        nonlocal tid, n_held, dropped, plain
        if n_held and plain and n_held in (L, L + 1):
            cls.add("held_L" if n_held == L else "held_L_plus_1")
        tid, n_held, dropped, plain = None, 0, False, False

    for p, cont in zip(parts, flags):
        cls = set()
        out.append(cls)
        n = len(p)
        if n == 0:
            cls.add("empty_continues" if cont else "empty_plain")
            if not cont:
                flush(cls)
            continue
        if n <= 2:
            cls.add(f"n{n}")
        starts, lens = runs(p.trace_id)
        first, last, one_run = int(lens[0]), int(lens[-1]), len(lens) == 1
        t0, tn = int(p.trace_id[0]), int(p.trace_id[-1])
        same = (n_held > 0 or dropped) and t0 == tid
        if one_run:
            cls.add(f"one_run_{'short' if n <= L + 1 else 'long'}_{'held' if same else 'fresh'}")
        else:
            cls.add("lead_round1" if first <= ROUND else "lead_round2" if first <= L else "lead_unknown")
            cls.add("tail_round1" if last <= ROUND else "tail_round2" if last <= L + 1 else "tail_unknown")
        whole = False
        if same:
            if dropped:
                cls.add("dropped_rest_leading")
                if not one_run:
                    cls.add("dropped_then_other_trace")
            elif n_held + first > L:
                if n_held + first == L + 1:
                    cls.add("append_to_L_plus_1")
                n_held, dropped = 0, True
            else:
                if n_held + first == L:
                    cls.add("append_to_L")
                n_held, plain = n_held + first, False
            whole = one_run and cont
            if whole and dropped:
                cls.add("dropped_whole_batch")
        if whole:
            continue
        flush(cls)  # the open trace ended (or the batch does not continue): joined or forgotten
        if not cont or (one_run and same):
            continue
        if last <= L + 1:
            tid, n_held, plain = tn, last, True
        else:
            cls.add("long_tail_continues")
            tid, dropped = tn, True
    end = set()
    flush(end)
    out.append(end)
    return out


# ---------------------------------------------------------------------------------------------
# the cases
LS = (512, 1000)
TARGETS = ("L-1", "L", "L+1", "L+2", "2L+5")
TARGET_TID = 0x7A26E7_0000_0001


def target_len(L, name):
    return {"L-1": L - 1, "L": L, "L+1": L + 1, "L+2": L + 2, "2L+5": 2 * L + 5}[name]


_SHORT = {}


def short_traces(seed, S):
    """A few hundred records of short TraceGen traces (every trace far below 256 records)."""
    if (seed, S) not in _SHORT:
        c = tracegen_host(seed, 60, max_depth=4, num_services=S)
        assert runs(c.trace_id)[1].max() < 128 and not (c.trace_id == np.uint64(TARGET_TID)).any()
        _SHORT[(seed, S)] = c
    return _SHORT[(seed, S)]


def cut(cols, points):
    bounds = [0, *sorted(points), len(cols)]
    return [cols.take(slice(a, b)) for a, b in zip(bounds[:-1], bounds[1:])]


class Case:
    """name; L; S; parts and the CONTINUES flag of each; end: how a trace still held after the last
    batch is flushed ("finalize", "empty": an empty batch without the flag, "partial":
    zk_deps_partial); key: the uncut stream's name (cases of one key share their expected result)."""

    def __init__(self, name, L, S, key, stream, points, end="finalize", last_continues=False, empties=()):
        self.name, self.L, self.S, self.key, self.stream, self.end = name, L, S, key, stream, end
        self.parts = cut(stream, points)
        self.flags = [True] * (len(self.parts) - 1) + [last_continues or end != "finalize"]
        for at in sorted(empties, reverse=True):  # empty CONTINUES batches between the parts
            self.parts.insert(at, SpanColumns.empty(0))
            self.flags.insert(at, True)
        if end == "empty":
            self.parts.append(SpanColumns.empty(0))
            self.flags.append(False)

    def __repr__(self):
        return self.name


def _cut_sets(a, b, L):
    """Cut points around a target trace at [a, b): the plan's search rounds are 256 records, so both
    sides of 256 from either end, the ends themselves and one record inside them; then pairs, one-
    and two-record batches, and a batch inside the trace."""
    edge = [a, a + 1, a + 255, a + 256, a + 257, b - 257, b - 256, b - 255, b - 1, b]
    singles = sorted({x for x in edge if a <= x <= b})
    sets = [(x,) for x in singles]
    sets += [(a + 1, b - 1), (a + 255, b - 255), (a + 256, b - 256), (a + 257, b - 257), (a, b),
             (a, a + 1), (b - 1, b), (a + 1, a + 3), (a + 100, a + 300), (a + 100, a + 101, a + 300)]
    if b - a > L + 3:  # a batch inside the trace, short and long, and long runs at either edge
        sets += [(a + 10, a + 10 + L + 1), (a + 10, a + 10 + L + 2), (a, a + L + 1), (a, a + L + 2),
                 (a + 1, a + L + 3, b), (a + 3, b - 300, b)]
    return list(dict.fromkeys(tuple(sorted(set(s))) for s in sets if all(a <= x <= b for x in s)))


_STREAMS = {}


def stream(L, S, target, tail=True):
    """short traces, the target trace at [a, b), short traces (tail=False: the target ends the
    stream) -> (key, SpanColumns, a, b)."""
    key = f"L{L}-{target}" + ("" if tail else "-last")
    if key not in _STREAMS:
        pre = short_traces(11, S)
        t = trace_of(TARGET_TID, target_len(L, target), S)
        parts = [pre, t] + ([short_traces(12, S)] if tail else [])
        _STREAMS[key] = (key, SpanColumns.concat(parts), len(pre), len(pre) + len(t))
    return _STREAMS[key]


S_OF = {512: 7, 1000: 41}
_CASES = None


def cases():
    """The deterministic case list (built once; the inputs are never written to)."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    for L in LS:
        S = S_OF[L]
        for target in TARGETS:
            key, cols, a, b = stream(L, S, target)
            for pts in _cut_sets(a, b, L):
                rel = "_".join(f"a+{x - a}" if x - a <= b - x else f"b-{b - x}" for x in pts)
                out.append(Case(f"{key}:{rel}", L, S, key, cols, pts))
            # every batch continues, empty CONTINUES batches in between, the last trace flushed at finalize
            out.append(Case(f"{key}:a+100_b:empties", L, S, key, cols, (a + 100, b), last_continues=True,
                            empties=(1, 2)))
            # the target ends the stream and is held whole (cut at a) or in part: flushed by finalize,
            # by an empty batch without the flag, by zk_deps_partial
            key, cols, a, b = stream(L, S, target, tail=False)
            for end in ("finalize", "empty", "partial"):
                out.append(Case(f"{key}:a:{end}", L, S, key, cols, (a,), end=end, last_continues=True))
                out.append(Case(f"{key}:a+100:{end}", L, S, key, cols, (a + 100,), end=end, last_continues=True))
    _CASES = out
    return out


def family(L, target):
    """The cases of one target length (both streams: with and without traces after the target)."""
    return [c for c in cases() if c.L == L and c.key in (f"L{L}-{target}", f"L{L}-{target}-last")]


_EXPECTED = {}


def expected_of(case):
    """`expected` of the case's stream, computed once per stream."""
    if case.key not in _EXPECTED:
        _EXPECTED[case.key] = expected(case.stream, case.S, case.L)
    return _EXPECTED[case.key]
