"""The device decoder's binary-annotation rows (zk_ingest_dev_spans_annotated_binary and its multi twin) against
the host decoder's (zk_ingest_spans_annotated_binary) and tests/binref.py's restatement.

Device service ids follow hash-table slot order, so rows are compared as (trace_id, span_id, key, value, ipv4,
service NAME, bits) lists, IN ORDER. Every comparison is exact equality. The floors were counted with the host
decoder on the CPU (tests/test_ingest_binary.py asserts them there too)."""
import ctypes as C

import numpy as np
import pytest

from tests import binref as B
from tests import thriftenc as T
from tests.test_gpu_ingest_rows import dev_rows, device, greedy_slices, upload
from tests.test_ingest import bad_spans
from tests.test_ingest_annotated import named_records, named_rows
from zipkin_amd import ZkError, _abi
from zipkin_amd.ingest import SpanDecoder, hash_string

pytestmark = pytest.mark.gpu

K_ING_WG = 256  # zk_ingest_dev.hip kIngWG: fragments per workgroup of the rows pass


def host_binary(blobs, snappy=True, strict=False):
    hd = SpanDecoder()
    cap = max(16, sum(len(b) for b in blobs))
    cols, rej, rows, brows = hd.decode_annotated(blobs, snappy=snappy, strict=strict, row_cap=cap, binary=True, binary_cap=cap)
    return hd, cols, rej, named_rows(rows, hd), B.named_binary_rows(brows, hd.service_names())


def dev_brows(dd, brows):
    got = brows.to_host()
    n = dd.num_services
    assert all(r[5] < n for r in got.rows() if r[6] & 8), "a row's service id is not in the dictionary"
    return B.named_binary_rows(got, dd.service_names())


# ---- 1. parity over batch shapes, both codecs ------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, K_ING_WG - 1, K_ING_WG, K_ING_WG + 1])
def test_batch_shapes_equal_the_host_decoder(gpu, n):
    frags = B.gen_frags(300 + n, n)
    want_b = B.expected_binary_rows(frags)
    fl = B.floors(frags)
    if n >= 63:
        assert min(fl["per_type"]) >= 4 and fl["hostless"] >= 10 and fl["binary_only"] >= 5 and fl["time_only"] >= 2 and fl["two_lists"] >= 3
    for snappy in (True, False):
        blobs = B.encode_all(frags, snappy)
        hd, hcols, hrej, want, hb = host_binary(blobs, snappy)
        assert hb == want_b and hrej == 0
        dd = device()(64)
        dcols, drej, rows, brows = dd.decode(blobs, snappy=snappy, strict=False, annotated=True, binary=True)
        assert drej == 0 and dcols.n == n
        assert dev_brows(dd, brows) == want_b
        assert dev_rows(dd, rows) == want
        assert named_records(dcols.to_host(), dd) == named_records(hcols, hd)


# ---- 2. rejected fragments between accepted ones ---------------------------------------------------------------
def test_rejected_fragments_between_accepted_ones(gpu):
    frags = B.gen_frags(401, 300)
    blobs = B.encode_all(frags)
    ok, bads = bad_spans()
    at = []
    for k in range(40):
        at.append(7 * k + 3)
        blobs.insert(7 * k + 3, T.snappy(bads[k % len(bads)][1]) if k % 4 else b"\x7f\x00garbage")
    hd, hcols, hrej, want, hb = host_binary(blobs)
    assert hrej == 40 and hb == B.expected_binary_rows(frags) and len(hb) >= 1000
    dd = device()(64)
    dcols, drej, rows, brows = dd.decode(blobs, strict=False, annotated=True, binary=True)
    assert drej == 40
    assert dev_brows(dd, brows) == hb  # (the records were compacted: a row's trace and span id are its own record's)
    assert dev_rows(dd, rows) == want
    # strict mode fails the batch before any row is written
    with pytest.raises(ZkError) as err:
        dd.decode(blobs, strict=True, annotated=True, binary=True)
    assert err.value.status == _abi.ZK_ERR_INVALID_SPAN


# ---- 3. slices --------------------------------------------------------------------------------------------------
def test_slices_over_a_small_scratch(gpu):
    frags = B.gen_frags(402, 200)
    raw = [len(B.encode(f)) for f in frags]  # every accepted fragment is walked, with or without time annotations
    budget = 8192
    assert 6000 < max(raw) < budget < sum(raw)  # (a fragment with two values of 3000 bytes is the largest)
    want_slices = greedy_slices(raw, budget)
    assert want_slices >= 3
    blobs = B.encode_all(frags)
    hd, hcols, hrej, want, hb = host_binary(blobs)
    small, big = device()(64, scratch_bytes=budget), device()(64)
    dcols, drej, rows, brows = small.decode(blobs, strict=False, annotated=True, binary=True)
    bcols, brej, rows2, brows2 = big.decode(blobs, strict=False, annotated=True, binary=True)
    assert drej == brej == 0
    assert dev_brows(small, brows) == dev_brows(big, brows2) == hb
    assert dev_rows(small, rows) == dev_rows(big, rows2) == want
    assert small.rows_stats()["slices"] == want_slices and big.rows_stats()["slices"] == 1
    for h, b in B.strings_of(frags).items():
        assert small.bytes(h) == big.bytes(h) == b


# ---- 4. multi ---------------------------------------------------------------------------------------------------
def test_multi_equals_one_decode_of_the_joined_fragments(gpu):
    frags = B.gen_frags(403, 240)
    blobs = B.encode_all(frags)
    blobs.insert(50, b"\x7f\x00garbage")
    batches = [upload(blobs[:80]), upload([]), upload(blobs[80:])]
    hd, hcols, hrej, want, hb = host_binary(blobs)
    assert hrej == 1 and len(hb) >= 800
    d1, d2 = device()(64), device()(64)
    c1, r1, e1, b1 = d1.decode(blobs, strict=False, annotated=True, binary=True)
    c2, r2, e2, b2 = d2.decode_device_many(batches, strict=False, annotated=True, binary=True)
    assert r1 == r2 == 1
    assert dev_brows(d2, b2) == dev_brows(d1, b1) == hb
    assert dev_rows(d2, e2) == dev_rows(d1, e1) == want
    assert named_records(c2.to_host(), d2) == named_records(hcols, hd)


# ---- 5. strings -------------------------------------------------------------------------------------------------
def test_keys_and_values_answer_as_on_the_host(gpu):
    frags = B.gen_frags(404, 150)
    blobs = B.encode_all(frags)
    hd, hcols, hrej, want, hb = host_binary(blobs)
    texts = B.strings_of(frags)
    assert len(texts) >= 40 and any(b"\0" in b for b in texts.values()) and any(len(b) == 3000 for b in texts.values())
    dd, quiet = device()(64), device()(64)
    dcols, drej, rows, brows = dd.decode(blobs, strict=False, annotated=True, binary=True)
    assert dev_brows(dd, brows) == hb
    for h, b in texts.items():
        assert dd.bytes(h) == hd.bytes(h) == b
        assert dd.string(h) == hd.string(h)
    assert dd.bytes(hash_string(b"")) == b""
    # the same batch again: every name and string is known now
    _, _, rows2, brows2 = dd.decode(blobs, strict=False, annotated=True, binary=True)
    assert dev_brows(dd, brows2) == hb and dev_rows(dd, rows2) == want
    # without the capture the rows are the same and the decoder learns no text from them
    qcols, qrej, qrows, qbrows = quiet.decode(blobs, strict=False, annotated=True, binary=True, row_strings=False)
    assert dev_brows(quiet, qbrows) == hb and dev_rows(quiet, qrows) == want
    for h in texts:
        with pytest.raises(ZkError):
            quiet.bytes(h)


# ---- 6. unchanged paths -----------------------------------------------------------------------------------------
def test_the_annotated_output_is_the_same_with_and_without_the_binary_rows(gpu):
    frags = B.gen_frags(405, 200)
    blobs = B.encode_all(frags)
    da, db = device()(64, max_span_names=256), device()(64, max_span_names=256)
    ca, ra, kva, ana, rows_a = da.decode(blobs, strict=False, items=True, span_names=True, annotated=True)
    cb, rb, kvb, anb, rows_b, brows = db.decode(blobs, strict=False, items=True, span_names=True, annotated=True, binary=True)
    assert ra == rb == 0 and len(brows) == B.floors(frags)["rows"]
    assert dev_rows(da, rows_a) == dev_rows(db, rows_b) and len(rows_a) >= 300
    assert named_records(ca.to_host(), da) == named_records(cb.to_host(), db)

    def bag(dd, pair):
        n = dd.service_names()
        return sorted(zip((n[i] for i in pair[0].cpu().tolist()), pair[1].cpu().tolist()))

    assert bag(da, kva) == bag(db, kvb) and bag(da, ana) == bag(db, anb) and len(bag(db, kvb)) >= 100

    def name_of(dd, cols):
        return [None if not (f >> 16) else dd.span_name((int(f) >> 16) - 1) for f in cols.to_host().flags]

    assert name_of(da, ca) == name_of(db, cb) and any(name_of(db, cb))
    with pytest.raises(ValueError):
        db.decode(blobs, binary=True)


# ---- 7. capacity ------------------------------------------------------------------------------------------------
def test_capacity_keeps_the_first_binary_rows(gpu):
    import torch

    from zipkin_amd.binannotstore import DeviceBinaryAnnotationRows
    from zipkin_amd.columns import DeviceColumns

    frags = B.gen_frags(406, 100)
    blobs = B.encode_all(frags)
    hd, hcols, hrej, want, hb = host_binary(blobs)
    total, time_total = len(hb), len(want)
    assert total >= 300 and time_total >= 150
    buf, off, n = upload(blobs)
    L = _abi.lib()
    PAD, MARK8, MARK4 = 16, 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
    for bcap, rcap, status in ((total - 1, time_total, _abi.ZK_ERR_CAPACITY), (1, time_total, _abi.ZK_ERR_CAPACITY),
                               (total, time_total - 1, _abi.ZK_ERR_CAPACITY), (7, 5, _abi.ZK_ERR_CAPACITY), (total, time_total, _abi.ZK_OK)):
        dd = device()(64)
        row = [torch.zeros(rcap, dtype=torch.int64 if k < 4 else torch.int32, device="cuda") for k in range(7)]
        brow = [torch.full((bcap + PAD,), MARK8 if k < 4 else MARK4, dtype=torch.int64 if k < 4 else torch.int32, device="cuda")
                for k in range(7)]
        an = _abi.zk_ingest_annotation_rows(*[t.data_ptr() for t in row], rcap, 0)
        bn = _abi.zk_ingest_binary_rows(*[t.data_ptr() for t in brow], bcap, 0)
        cols = DeviceColumns(n)
        nout, nrej = C.c_uint64(), C.c_uint64()
        st = L.zk_ingest_dev_spans_annotated_binary(dd._h, buf.data_ptr(), off.data_ptr(), n, _abi.ZK_CODEC_SNAPPY_THRIFT, 0,
                                                    C.byref(cols.abi(n)), C.byref(nout), C.byref(nrej), None, C.byref(an), C.byref(bn))
        assert st == status, (bcap, rcap)
        assert bn.n == bcap and an.n == rcap and nout.value == n
        assert dev_brows(dd, DeviceBinaryAnnotationRows(*[t[:bcap] for t in brow])) == hb[:bcap]
        for k, t in enumerate(brow):  # nothing behind the capacity is written
            assert t[bcap:].cpu().tolist() == [MARK8 if k < 4 else MARK4] * PAD
    # the wrapper decodes again with 4x the room until the rows fit
    dd = device()(64)
    dcols, drej, rows, brows = dd.decode(blobs, strict=False, annotated=True, binary=True, binary_cap=3)
    assert dev_brows(dd, brows) == hb and dev_rows(dd, rows) == want
