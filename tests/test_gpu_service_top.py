"""The top of the service range: S = 4096 (kMaxServices), where a link's cell takes all 24 bits above
its 40-bit duration. The link of cell (4095, 4095) with d = 2^40 - 1 is the all-ones word, and the
realtime link store's key range of server 4095 ends at the all-ones key. One ctx of this size, the
expectation from tests/exactref.py alone (no dense oracle at 2^24 cells); finalize writes into
device tensors and only the cells in question come back to the host."""
import numpy as np
import pytest

from tests import exactref
from tests.exactref import DMAX
from tests.test_gpu_exact_bounds import star_batch
from zipkin_amd import DepsContext
from zipkin_amd.realtime import RealtimeLinks

pytestmark = pytest.mark.gpu

S = 4096
TOP = S - 1
DURATIONS = (0, 1 << 21, DMAX)
CELLS = {(TOP, TOP): DURATIONS, (TOP, 0): DURATIONS, (0, TOP): DURATIONS}
_RUN = {}


def top_run():
    """Two star traces (roots of service 4095 and 0), then a shuffled batch of > 2^18 records over
    the same services, through ONE ctx with a bound link store -> per step the finalized cells, the
    number of present cells and the counters; for the first step also the store's answers."""
    if _RUN:
        return _RUN
    import torch

    few = star_batch([TOP, 0], [6, 3], [TOP, 0, TOP, 0, TOP, 0, TOP, TOP, TOP],
                     [DMAX, 0, 0, 1 << 21, 1 << 21, DMAX, *DURATIONS])
    rng = np.random.default_rng(4096)
    T, K = (1 << 14) + 3, 15
    root_svc = rng.choice(np.array([0, TOP]), T)
    child_svc = rng.choice(np.array([0, TOP]), T * K)
    d = np.asarray(DURATIONS, np.int64)[rng.integers(0, 3, T * K)]
    parents = np.repeat(root_svc, K)
    many_cells = {(p, c): d[(parents == p) & (child_svc == c)] for p in (0, TOP) for c in (0, TOP)}
    many = star_batch(root_svc, [K] * T, child_svc, d, tid0=100)
    assert len(many) > 1 << 18
    many = many.take(rng.permutation(len(many)))

    out = {k: torch.zeros(S * S, dtype=torch.float64, device="cuda") for k in ("m1", "m2", "m3", "m4")}
    out["m0"] = torch.zeros(S * S, dtype=torch.int64, device="cuda")
    out["present"] = torch.zeros(S * S, dtype=torch.uint8, device="cuda")

    def finalized(ctx, cells):
        ctx.finalize(out_device=out)
        ctx.sync()
        torch.cuda.synchronize()
        idx = torch.tensor([p * S + c for p, c in cells], device="cuda")
        got = {k: out[k][idx].cpu().numpy() for k in out}
        return {"cells": cells, "got": got, "present": int(out["present"].sum().item()), "stats": ctx.stats()}

    with DepsContext(S) as ctx, RealtimeLinks(S) as rl:
        rl.bind(ctx)
        ctx.accumulate(few, clustered=True)
        run = {"few": finalized(ctx, CELLS), "count": rl.count(),
               "servers": {s: rl.server_links(s) for s in (0, 1, TOP - 1, TOP)}}
        rl.unbind()
        ctx.reset()
        ctx.accumulate(many, clustered=False, verify=False)  # the group join
        run["many"] = finalized(ctx, many_cells)
    run["tid_of_root"] = {int(few.service_id[i]): int(few.trace_id[i]) for i in np.flatnonzero(few.parent_id == 0)}
    _RUN.update(run)
    return _RUN


def check_cells(step, links):
    assert step["stats"]["joined_links"] == links and step["stats"]["duration_range"] == 0
    cells, got = step["cells"], step["got"]
    assert step["present"] == len(cells) and got["present"].tolist() == [1] * len(cells)
    for i, ((p, c), ds) in enumerate(cells.items()):
        want = exactref.moments(exactref.multiset(ds))
        assert int(got["m0"][i]) == want[0], f"cell ({p}, {c}): m0 {int(got['m0'][i])} != {want[0]}"
        for k in (1, 2, 3, 4):
            x = got[f"m{k}"][i]
            assert x.view(np.uint64) == np.float64(want[k]).view(np.uint64), f"cell ({p}, {c}) m{k}: {x!r} != {want[k]!r}"


def test_dependency_cells_at_the_top_of_the_service_range(gpu):
    """Cells (4095, 4095), (4095, 0), (0, 4095) with durations {0, 2^21, 2^40 - 1} through the
    streaming join: among them the link whose word is all ones."""
    check_cells(top_run()["few"], 9)


def test_group_join_at_the_top_of_the_service_range(gpu):
    """The same cells (and (0, 0)) with ~61k links each from a shuffled, unverified batch of > 2^18
    records: the group join emits the all-ones link thousands of times."""
    step = top_run()["many"]
    assert DMAX in step["cells"][(TOP, TOP)]
    check_cells(step, sum(len(v) for v in step["cells"].values()))


def test_realtime_link_store_returns_the_last_server(gpu):
    """zk_rl_server_links(4095) at S = 4096: the upper key of the server's range, (4096 * 4096) << 40,
    does not fit 64 bits; its rows (parents 0 and 4095, the all-ones key among them) must come back
    like any other server's."""
    run = top_run()
    assert run["count"] == (9, 0)
    tid = run["tid_of_root"]

    def rows(parents):
        want = sorted((p, d, tid[p]) for p in parents for d in DURATIONS)
        return [list(x) for x in zip(*want)] if want else [[], [], []]

    for server, parents in ((TOP, (0, TOP)), (0, (TOP,)), (1, ()), (TOP - 1, ())):
        par, dur, tids = run["servers"][server]
        want = rows(parents)
        assert par.tolist() == want[0], f"server {server}: parents"
        assert dur.tolist() == want[1], f"server {server}: durations"
        assert tids.tolist() == want[2], f"server {server}: traceIds"
