"""The meaning of zk_sp_summaries' heads and entries, before any device runs: the TraceSummary assembled
from the model's output (tests/spsumref.py) is spref.summary, for the reference's vectors
(tests/golden/trace_summaries.json) and a few shapes the vectors do not have. No GPU."""
import pytest

from tests import spref as R
from tests import spsumref as M
from zipkin_amd import SUMMARY_HEAD, _abi

G = R.golden()
MAX_ROWS = _abi.ZK_SP_SUM_MAX_ROWS


def test_the_models_constants_are_the_bindings():
    assert (M.FOUND, M.TIMED, M.OVERFLOW) == (_abi.ZK_SP_SUM_FOUND, _abi.ZK_SP_SUM_TIMED, _abi.ZK_SP_SUM_OVERFLOW)
    assert M.HEAD == SUMMARY_HEAD.names


@pytest.mark.parametrize("case", G["cases"], ids=[c["name"] for c in G["cases"]])
@pytest.mark.parametrize("names", (False, True), ids=("ids", "names"))
def test_golden_cases(case, names):
    services = G["services"] if names else None
    rows = R.golden_rows(case, G["services"])
    tid = case["trace_id"]
    heads, entries = M.summaries(rows, [tid], MAX_ROWS)
    want = R.summary(rows, services)
    assert M.assemble(heads, entries, services) == ([] if want is None else [want])
    e = case["expect"]
    if rows:
        assert heads[0][3] == len(rows) and heads[0][4] == len(e["span_order"]) and heads[0][6] & M.FOUND
        assert bool(heads[0][6] & M.TIMED) == (e["start_end"] is not None)
        if e["start_end"] is not None:
            assert list(heads[0][1:3]) == e["start_end"]
            assert M.assemble(heads, entries)[0][3] == e["duration_micro"]
    else:
        assert heads == [M.ZERO] and entries == []


def test_heads_of_absent_untimed_duplicated_and_long_traces():
    T, S = R.TIMED, R.SVC_SERVER
    store = [(7, 1, 0, 5, 9, 2, T | S), (7, 1, 0, 3, 4, 1, T | S), (7, 1, 0, 100, 200, 1, S),  # span 1: services 1, 2
             (7, 2, 0, 1, 2, 0, T),                                                            # timed, no service
             (7, 3, 0, 0, R.INT64_MAX, 4, S),                                                  # untimed, a service
             (8, 1, 0, 0, R.INT64_MAX, 4, S)]                                                  # an untimed trace
    heads, entries = M.summaries(store, [8, 7, 404, 7], MAX_ROWS)
    seven = (7, 1, 9, 5, 3, 2, M.FOUND | M.TIMED)
    assert heads == [(8, 0, 0, 1, 1, 0, M.FOUND), seven, M.ZERO, seven]
    assert entries == [(1, 3, 9), (2, 3, 9)] * 2
    rows7 = [r for r in store if r[0] == 7]
    assert M.assemble(heads, entries) == [R.summary(rows7)] * 2 and R.summary([store[-1]]) is None
    # a trace above the bound keeps its reductions and loses its merge
    heads, entries = M.summaries(store, [7], 4)
    assert heads == [(7, 1, 9, 5, 0, 0, M.FOUND | M.TIMED | M.OVERFLOW)] and entries == []
    # the wrapping duration
    wide = [(9, 1, 0, R.INT64_MIN, R.INT64_MAX, 0, T | S)]
    heads, entries = M.summaries(wide, [9], MAX_ROWS)
    assert M.assemble(heads, entries) == [R.summary(wide)] and R.summary(wide)[3] == -1
