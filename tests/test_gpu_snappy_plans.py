"""Snappy element conformance on the device: the hand-planned streams of
tests/test_snappy_plans_host.py (families A..G there) through the three builds of the device decoder
-- plain, with items, with items and span names; between them the prefetching and the non-prefetching
instantiation of the LDS decode kernel -- against the device on the uncompressed thrift of the same
Spans, the host decoder, and the span-level expectation that never passes through Snappy code.

What the families reach in the device's in-place LDS Snappy decoder, which libsnappy's streams do not:
copy-4 elements, literal tags 62 and 63, every copy length at offsets below 16 (its 16-byte source
reads and whole 8-byte steps), copies ending on the last output byte, padded header varints, and
fragments on either side of the in-place safety check (family C; those it refuses go to the
global-memory decoder, as do all of family E). All comparisons are exact."""
import functools

import pytest

from tests import namefrag
from tests import snappyplan as P
from tests.test_snappy_plans_host import (FAMILIES, aligned, assert_payloads, expected_view, family_c, family_d,
                                          family_g, host_view, project, strict_batches, view)
from zipkin_amd import ZkError, _abi
from zipkin_amd.ingest import DeviceSpanDecoder

pytestmark = pytest.mark.gpu

BUILDS = {"plain": dict(items=False, span_names=False), "items": dict(items=True, span_names=False),
          "names": dict(items=True, span_names=True)}
MAX_NAMES = 8192  # services and span names: family A has ~3300 Spans, some with a name of their own each


def device(build):
    return DeviceSpanDecoder(MAX_NAMES, max_span_names=MAX_NAMES if BUILDS[build]["span_names"] else 0)


def device_view(dec, cases, build, snappy=True):
    blobs = [c.stream if snappy else c.raw for c in cases]
    return view(dec, dec.decode(blobs, snappy=snappy, strict=False, **BUILDS[build]), **BUILDS[build])


@functools.lru_cache(maxsize=None)
def reference(fam):
    """(host decoder's view, span-level expectation) of a family, with items and span names"""
    cases = FAMILIES[fam]()
    return host_view(cases)[1], expected_view(cases, items=True, span_names=True)


def assert_family(got, fam, build):
    host, want = reference(fam)
    for name, ref in (("host decoder", host), ("span-level expectation", want)):
        ref = project(ref, **BUILDS[build])
        assert got["rejected"] == ref["rejected"], name
        assert got.keys() == ref.keys()
        for k in got:
            assert got[k] == ref[k], (k, name)


@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_family(gpu, fam, build):
    cases = FAMILIES[fam]()
    dd, dt = device(build), device(build)
    got = device_view(dd, cases, build)
    assert got == device_view(dt, cases, build, snappy=False)  # the device on the raw thrift
    assert_family(got, fam, build)
    assert_payloads(dd, cases, **BUILDS[build])
    if fam == "G":
        assert got["rejected"] == sum(P.decode(c.stream) is None for c in cases) == len(family_g())
    if fam == "C":
        # again on the same decoder: every service name, span name and string is known (resolved in
        # the decode kernel); then as three batches cut off the 64-fragment grid, in one multi-batch call
        assert device_view(dd, cases, build) == got
        import torch

        cuts = [0, 1000 + 37, 2 * len(cases) // 3 + 1, len(cases)]
        assert all(c % 64 for c in cuts[1:3])
        batches = []
        for lo, hi in zip(cuts, cuts[1:]):
            buf, off = namefrag.pack([c.stream for c in cases[lo:hi]])
            batches.append((torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda(), hi - lo))
        many = device(build)
        res = many.decode_device_many(batches, strict=False, **BUILDS[build])
        assert view(many, res, **BUILDS[build]) == got
        many.close()
    dd.close()
    dt.close()


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_family_d_alone(gpu, build):
    """every size around the region thresholds as a batch of its own (a round with one lane)"""
    dd, dt = device(build), device(build)
    for c in family_d():
        got = device_view(dd, [c], build)
        assert got == device_view(dt, [c], build, snappy=False), c.id
        assert got == project(host_view([c])[1], **BUILDS[build]), c.id
        assert got == project(expected_view([c], items=True, span_names=True), **BUILDS[build]), c.id
        assert_payloads(dd, [c], **BUILDS[build])
    dd.close()
    dt.close()


def test_family_c_unaligned_only(gpu):
    """family C without the fillers (64 lanes of run-then-literal streams side by side in a round)"""
    cases = family_c()
    dd = device("names")
    got = device_view(dd, cases, "names")
    assert got == host_view(cases)[1] == expected_view(cases, items=True, span_names=True)
    dd.close()


def test_strict_names_the_first_bad_fragment(gpu):
    for cid, at, blobs in strict_batches():
        dd = device("plain")
        with pytest.raises(ZkError) as e:
            dd.decode(blobs, strict=True)
        assert e.value.status == _abi.ZK_ERR_INVALID_SPAN and "span %d:" % at in e.value.message, (cid, e.value.message)
        dd.close()


def test_aligned_batch_really_is(gpu):
    """the upload keeps the batch's first byte 16-byte aligned, so `aligned` places what it says"""
    import torch

    buf, _ = namefrag.pack([c.stream for c in aligned(family_c()[:2])])
    assert torch.from_numpy(buf).cuda().data_ptr() % 16 == 0
