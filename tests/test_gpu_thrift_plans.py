"""Thrift wire-form conformance on the device: the planned encodings of tests/thriftplan.py through
the three builds of the device decoder -- plain, with items, with items and span names -- as raw
thrift and as Snappy streams, against the host decoder and against thriftref's reading of the bytes
(tests/test_thrift_plans_host.py, where the families and the expectation are described).

What the families reach on the device that canonical encodings do not: both sides of every comparison
of the window-matched fast path (S1, S2: the broken forms must land on exactly what the generic walk
gives; A: every window at every address residue, the empty-string forms), the generic walk and its
item iterators on reordered, repeated and retyped fields (O), the three skip routines (K), the depth
limit (KD) and the same walks over global memory (G, GD: fragments past the LDS budget). The nesting
cases (KD, GD) are compared against thriftref with the cases past the device's limit rejected; every
other family three ways. All comparisons are exact."""
import functools

import pytest

from tests import thriftplan as TP
from tests.test_snappy_plans_host import project, view
from tests.test_thrift_plans_host import expected_view, family_view, host_view, readings, strict_batches
from zipkin_amd import ZkError, _abi
from zipkin_amd.ingest import DeviceSpanDecoder

pytestmark = pytest.mark.gpu

BUILDS = {"plain": dict(items=False, span_names=False), "items": dict(items=True, span_names=False),
          "names": dict(items=True, span_names=True)}
MAX_NAMES = 8192  # services and span names: S1 has ~3700 fragments, an edit inside a name makes a new one


def device(build):
    return DeviceSpanDecoder(MAX_NAMES, max_span_names=MAX_NAMES if BUILDS[build]["span_names"] else 0)


def device_view(dec, cases, build, snappy):
    blobs = [c.stream if snappy else c.raw for c in cases]
    return view(dec, dec.decode(blobs, snappy=snappy, strict=False, **BUILDS[build]), **BUILDS[build])


@functools.lru_cache(maxsize=None)
def host_reference(fam):
    v = host_view(TP.FAMILIES[fam](), snappy=False)
    v.pop("span_names")
    return v


def assert_same(got, ref, build, name):
    ref = project(ref, **BUILDS[build])
    assert got["rejected"] == ref["rejected"], name
    assert got.keys() == ref.keys(), name
    for k in got:
        assert got[k] == ref[k], (k, name)


@pytest.mark.parametrize("snappy", [False, True], ids=["raw", "snappy"])
@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("fam", sorted(TP.FAMILIES))
def test_family(gpu, fam, build, snappy):
    cases = TP.FAMILIES[fam]()
    dd = device(build)
    try:
        got = device_view(dd, cases, build, snappy)
        assert_same(got, family_view(fam, "device"), build, "thriftref")
        if fam not in TP.DEPTH_FAMILIES:
            assert family_view(fam, "device") == family_view(fam, "host")
            assert_same(got, host_reference(fam), build, "host decoder")
        # again on the same decoder: every service name, span name and string is known now (resolved
        # inside the decode kernel instead of published for the dictionary kernels)
        assert device_view(dd, cases, build, snappy) == got
    finally:
        dd.close()


def one_by_one(cases, results, snappy):
    dd = device("plain")
    try:
        for c, r in zip(cases, results):
            got = device_view(dd, [c], "plain", snappy)
            want = project(expected_view([c], [r], "device"), **BUILDS["plain"])
            assert got == want, c.id
    finally:
        dd.close()


@pytest.mark.parametrize("snappy", [False, True], ids=["raw", "snappy"])
@pytest.mark.parametrize("fam", ["S1", "S2"])
def test_truncations_alone(gpu, fam, snappy):
    """every truncation as a batch of its own: one live lane, nothing after the fragment's last byte
    but what the decoder itself put there (the fast path's windows read whole dwords past the end)"""
    picked = [(c, r) for c, r in zip(TP.FAMILIES[fam](), readings(fam)) if "-trunc" in c.id]
    assert len(picked) == len(TP.RAW_B1 if fam == "S1" else TP.RAW_B2)
    one_by_one([c for c, _ in picked], [r for _, r in picked], snappy)


@pytest.mark.parametrize("snappy", [False, True], ids=["raw", "snappy"])
def test_nesting_cases_alone(gpu, snappy):
    """accept or reject of every nesting case alone (in a batch the counts could cancel)"""
    one_by_one(TP.family_kd(), readings("KD"), snappy)


def test_strict_names_the_bad_fragment(gpu):
    for cid, at, msg, blobs in strict_batches():
        dd = device("plain")
        try:
            with pytest.raises(ZkError) as e:
                dd.decode(blobs, snappy=False, strict=True)
            assert e.value.status == _abi.ZK_ERR_INVALID_SPAN and "span %d:" % at in e.value.message, (cid, at, e.value.message)
        finally:
            dd.close()
