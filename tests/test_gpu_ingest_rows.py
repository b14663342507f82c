"""The device decoder's annotation-store rows (zk_ingest_dev_spans_annotated and its multi twin) against the
host decoder's (zk_ingest_spans_annotated) and tests/test_ingest_annotated.py's restatement.

Device service ids follow hash-table slot order, so rows are compared as (trace_id, span_id, ts, value,
ipv4, service NAME, bits) lists, IN ORDER (the device call promises the host decoder's order). Every
comparison is exact equality. The floors on row counts were counted with the host decoder on the CPU:
they make sure a case exercises what it is there for."""
import ctypes as C
import dataclasses
import random
from collections import Counter

import numpy as np
import pytest

from oracle.spans import UNKNOWN_SERVICE_NAME, Annotation, BinaryAnnotation, Endpoint, Span
from tests import thriftenc as T
from tests import tsaref
from tests.richgen import gen_traces
from tests.test_gpu_ingest_items import _odd_spans
from tests.test_ingest import _fuzz, bad_spans, encode_all
from tests.test_ingest_annotated import (_ann, _i16, _i32, _name, _span, expected_rows, named_records, named_rows)
from zipkin_amd import AnnotationRows, ZkError, _abi
from zipkin_amd.annotstore import ROW_COLUMNS
from zipkin_amd.ingest import SpanDecoder, hash_string

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
SET_CAPACITY = 1 << 16  # zk_ingest_dev.hip rows_pass / ingest_batch: grow_string_set(g, 1u << 16), the set's first size
EXTRA_CAPACITY = 4096   # ... size_extra(g, 4096, 0), the extra-name list's first size


def device():
    from zipkin_amd.ingest import DeviceSpanDecoder

    return DeviceSpanDecoder


def upload(blobs):
    import torch

    offs = np.zeros(len(blobs) + 1, np.int64)
    if blobs:
        offs[1:] = np.cumsum([len(b) for b in blobs])
    buf = torch.from_numpy(np.frombuffer(b"".join(blobs) or b"\0", np.uint8).copy()).cuda()
    return buf, torch.from_numpy(offs).cuda(), len(blobs)


def host_of(rows):
    """a DeviceAnnotationRows as host AnnotationRows"""
    return AnnotationRows(*[getattr(rows, k).cpu().numpy().view(dt) for k, dt in ROW_COLUMNS])


def dev_rows(dd, rows):
    got = host_of(rows)
    n = dd.num_services
    assert all(r[5] < n for r in got.rows() if r[6] & 8), "a row's service id is not in the dictionary"
    return named_rows(got, dd)


def host_annotated(blobs, snappy=True, strict=False):
    hd = SpanDecoder()
    cols, rej, rows = hd.decode_annotated(blobs, snappy=snappy, strict=strict, row_cap=max(16, sum(len(b) for b in blobs)))
    return hd, cols, rej, named_rows(rows, hd)


def same_records(dd, dcols, hd, hcols):
    assert named_records(dcols.to_host(), dd) == named_records(hcols, hd)


# ---- 1. parity on rich traces ----------------------------------------------------------------------------
@pytest.mark.parametrize("seed,anomalies,snappy", [(201, 0.0, True), (202, 0.4, True), (203, 0.4, False)])
def test_rich_traces_equal_the_host_decoder(gpu, seed, anomalies, snappy):
    spans = gen_traces(seed, 300, max_depth=5, anomalies=anomalies) + _odd_spans()
    blobs = encode_all(spans, snappy)
    hd, hcols, hrej, want = host_annotated(blobs, snappy)
    assert want == expected_rows(spans)
    assert len(want) >= 10_000 and sum(1 for r in want if r[5] is None) >= 2 and sum(1 for r in want if not r[6] & 7) >= 1_000
    dd, plain = device()(256), device()(256)
    dcols, drej, rows = dd.decode(blobs, snappy=snappy, strict=False, annotated=True)
    assert drej == hrej == 0
    assert dev_rows(dd, rows) == want
    pcols, prej = plain.decode(blobs, snappy=snappy, strict=False)
    assert named_records(dcols.to_host(), dd) == named_records(pcols.to_host(), plain)
    same_records(dd, dcols, hd, hcols)
    assert dd.rows_stats()["slices"] == 1
    # every value's text is kept, as on the host
    for h in {r[3] for r in want}:
        assert dd.string(h) == hd.string(h)
    # the same batch again: every name and string is known now
    _, _, rows2 = dd.decode(blobs, snappy=snappy, strict=False, annotated=True)
    assert dev_rows(dd, rows2) == want


# ---- 2. items and span names untouched -------------------------------------------------------------------
def test_items_and_span_names_are_untouched_by_the_rows_pass(gpu):
    spans = gen_traces(204, 100, max_depth=4, anomalies=0.3) + _odd_spans()
    blobs = encode_all(spans)
    hd, hcols, hrej, want = host_annotated(blobs)
    da, db = device()(256), device()(256)
    ca, ra, kva, ana = da.decode(blobs, strict=False, items=True)
    cb, rb, kvb, anb, rows = db.decode(blobs, strict=False, items=True, annotated=True)
    assert dev_rows(db, rows) == want

    def bag(dd, pair):
        n = dd.service_names()
        return Counter(zip((n[i] for i in pair[0].cpu().tolist()), pair[1].cpu().tolist()))

    assert bag(db, kvb) == bag(da, kva) and bag(db, anb) == bag(da, ana)
    assert sum(bag(db, kvb).values()) > 100 and sum(bag(db, anb).values()) > 20
    na, nb = device()(256, max_span_names=4096), device()(256, max_span_names=4096)
    ca, ra = na.decode(blobs, strict=False, span_names=True)
    cb, rb, rows = nb.decode(blobs, strict=False, span_names=True, annotated=True)
    assert dev_rows(nb, rows) == want

    def name_of(dd, cols):
        return [None if not (f >> 16) else dd.span_name((int(f) >> 16) - 1) for f in cols.to_host().flags]

    assert name_of(na, ca) == name_of(nb, cb) and any(name_of(nb, cb))
    ha, hb = ca.to_host(), cb.to_host()
    assert np.array_equal(ha.flags & 0xFFFF, hb.flags & 0xFFFF)
    for k in ("trace_id", "span_id", "parent_id", "first_ts", "last_ts"):
        assert np.array_equal(getattr(ha, k), getattr(hb, k))
    assert [na.service_name(i) for i in ha.service_id.tolist()] == [nb.service_name(i) for i in hb.service_id.tolist()]


# ---- 3. endpoint wire forms ------------------------------------------------------------------------------
I32_MIN, I32_MAX, I16_MIN, I16_MAX = -2 ** 31, 2 ** 31 - 1, -2 ** 15, 2 ** 15 - 1


def wire_form_blobs():
    anns = [
        _ann(10, "cs", _i32(1, I32_MIN) + _i16(2, I16_MIN) + _name("a") + b"\0"),            # 0 ipv4 0x80000000
        _ann(11, "cr", _i32(1, I32_MAX) + _i16(2, I16_MAX) + _name("a") + b"\0"),            # 1 port 0x7FFF
        _ann(12, "sr", _i32(1, -1) + _i16(2, -1) + _name("b") + b"\0"),                      # 2 all ones
        _ann(13, "ss"),                                                                      # 3 no host
        _ann(14, "custom", _name("b") + b"\0"),                                              # 4 a host without ipv4 or port
        _ann(15, "cs", _i32(1, 7) + _i16(2, 8) + _name("a") + b"\0", _name("c") + b"\0"),    # 5 a later struct keeps both
        _ann(16, "cs", _i32(1, 7) + _i16(2, 8) + _name("a") + b"\0", _i32(1, 9) + b"\0"),    # 6 ... and the name
        _ann(17, "cs", _i32(1, 7) + _i32(1, 70) + _i16(2, 8) + _i16(2, 80) + b"\0"),         # 7 last wins; no name
        _ann(18, "cs", T._fh(T.T_I64, 1) + T._i64(5) + T._fh(T.T_I32, 2) + (6).to_bytes(4, "big") + _name("a") + b"\0"),  # 8 wrong types
        _ann(19, "cs", _i32(1, 3) + T._fh(T.T_I16, 1) + (4).to_bytes(2, "big") + _i16(2, 5) + _i32(2, 6) + b"\0"),        # 9 ... after right ones
        _ann(20, "x", _name("") + b"\0"),                                                    # 10 a host named ""
        T._fh(T.T_I64, 1) + T._i64(21) + T._fh(T.T_STRUCT, 3) + _name("a") + b"\0" + b"\0",  # 11 no value field
    ]
    one = _span(2 ** 63, 2 ** 64 - 1, anns)
    # two field-6 lists in one span: both appended
    body = T._fh(T.T_I64, 1) + T._i64(5) + T._fh(T.T_STRING, 3) + T._str("n") + T._fh(T.T_I64, 4) + T._i64(6)
    lst = lambda xs: T._fh(T.T_LIST, 6) + bytes([T.T_STRUCT]) + len(xs).to_bytes(4, "big") + b"".join(xs)
    two = body + lst(anns[:2]) + lst(anns[4:6]) + b"\0"
    e = Endpoint(1, 2, "svc")
    only_binary = T.span(Span(9, "n", 8, 7, (), (BinaryAnnotation("k", b"v", "BYTES", e), BinaryAnnotation("k2", b"v", "BYTES", None))))
    return [one, two, only_binary]


@pytest.mark.parametrize("snappy", (False, True), ids=("thrift", "snappy"))
def test_endpoint_wire_forms(gpu, snappy):
    blobs = [T.snappy(b) if snappy else b for b in wire_form_blobs()]
    hd, hcols, hrej, want = host_annotated(blobs, snappy, strict=True)
    assert len(want) == 12 + 4 + 0 and hrej == 0
    dd = device()(64)
    dcols, drej, rows = dd.decode(blobs, snappy=snappy, strict=True, annotated=True)
    assert drej == 0 and dcols.n == 3
    got = dev_rows(dd, rows)
    assert got == want
    # and what the rows are, stated here (ipv4, port, bits & 0xFFFF, name)
    assert [(r[4], r[6] >> 16, r[6] & 0xFFFF, r[5]) for r in got[:12]] == [
        (0x80000000, 0x8000, 1 | 8, "a"), (0x7FFFFFFF, 0x7FFF, 2 | 8, "a"), (0xFFFFFFFF, 0xFFFF, 3 | 8, "b"),
        (0, 0, 4, None), (0, 0, 0 | 8, "b"), (7, 8, 1 | 8, "c"), (9, 8, 1 | 8, "a"), (70, 80, 1 | 8, UNKNOWN_SERVICE_NAME),
        (0, 0, 1 | 8, "a"), (3, 5, 1 | 8, UNKNOWN_SERVICE_NAME), (0, 0, 0 | 8, UNKNOWN_SERVICE_NAME), (0, 0, 0 | 8, "a")]
    assert got[11][3] == hash_string("") and dd.string(hash_string("")) == ""
    assert [r[2] for r in got[12:]] == [10, 11, 14, 15] and {r[:2] for r in got[12:]} == {(5, 6)}
    same_records(dd, dcols, hd, hcols)


# ---- 4. batch shapes -------------------------------------------------------------------------------------
def shaped_spans(n):
    """fragments cycling through 1, 2, 5 and 0 annotations; with more than one fragment, one has 300"""
    e, f = Endpoint(0x0A000001, 80, "front"), Endpoint(0x0A000002, 8080, "back")
    cyc = (0, 1, 2, 5)
    out = []
    for k in range(n):
        m = 300 if (n > 1 and k == n // 2) else cyc[(k + 1) % 4]
        anns = tuple(Annotation(1000 + 10 * k + j, ("sr", "v%d" % (k % 7), "ss", "cs", "w%d" % j)[j % 5],
                                (e, f, None)[(k + j) % 3]) for j in range(m))
        out.append(Span(7000 + k // 3, "op", k + 1, None, anns))
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_batch_shapes(gpu, n):
    spans = shaped_spans(n)
    blobs = encode_all(spans)
    hd, hcols, hrej, want = host_annotated(blobs)
    assert want == expected_rows(spans)
    assert len(want) == sum(len(s.annotations) for s in spans) >= (1 if n == 1 else 300 + 2 * (n - 1) - 4)
    dd = device()(64)
    dcols, drej, rows = dd.decode(blobs, strict=False, annotated=True)
    assert drej == 0 and dcols.n == n
    assert dev_rows(dd, rows) == want
    same_records(dd, dcols, hd, hcols)


# ---- 5. rejected and undecodable fragments between accepted ones ------------------------------------------
def test_rejected_fragments_between_accepted_ones(gpu):
    import torch

    from zipkin_amd.columns import DeviceColumns

    spans = gen_traces(205, 200, max_depth=5, anomalies=0.4) + _odd_spans()
    blobs = _fuzz(encode_all(spans), 205)
    ok, bads = bad_spans()
    for k, (_, b) in enumerate(bads):
        blobs.insert(11 * k + 5, T.snappy(b))
    hd, hcols, hrej, want = host_annotated(blobs)
    assert hrej >= 1_000 and len(want) >= 2_000 and len(hcols) + hrej == len(blobs)
    dd = device()(512)
    dcols, drej, rows = dd.decode(blobs, strict=False, annotated=True)
    assert drej == hrej
    assert dev_rows(dd, rows) == want  # (D5 compacted: a row's trace and span id are its own record's)
    same_records(dd, dcols, hd, hcols)
    # strict mode fails the batch before any row is written
    buf, off, n = upload(blobs)
    row = [torch.zeros(64, dtype=torch.int64 if k < 4 else torch.int32, device="cuda") for k in range(7)]
    an = _abi.zk_ingest_annotation_rows(*[t.data_ptr() for t in row], 64, 99)
    nout, nrej = C.c_uint64(), C.c_uint64()
    st = _abi.lib().zk_ingest_dev_spans_annotated(dd._h, buf.data_ptr(), off.data_ptr(), n, _abi.ZK_CODEC_SNAPPY_THRIFT,
                                                  _abi.ZK_INGEST_STRICT, C.byref(DeviceColumns(n).abi(n)), C.byref(nout),
                                                  C.byref(nrej), None, C.byref(an))
    assert st == _abi.ZK_ERR_INVALID_SPAN and an.n == 0
    assert all(int(t.abs().sum()) == 0 for t in row)


# ---- 6. slices -------------------------------------------------------------------------------------------
def greedy_slices(raw, budget):
    """k_ing_index_slices: the longest runs of fragments whose decompressed bytes fit the budget"""
    out, lo = 0, 0
    while lo < len(raw):
        hi, used = lo + 1, raw[lo]
        while hi < len(raw) and used + raw[hi] <= budget:
            used += raw[hi]
            hi += 1
        out, lo = out + 1, hi
    return out


def test_slices_over_a_small_scratch(gpu):
    rnd = random.Random(206)
    spans = gen_traces(206, 150, max_depth=4, anomalies=0.3)
    assert len(spans) >= 400
    giant = BinaryAnnotation("blob", bytes(rnd.getrandbits(8) for _ in range(22000)), "BYTES", Endpoint(1, 2, "giant-host"))
    spans[37] = dataclasses.replace(spans[37], binary_annotations=spans[37].binary_annotations + (giant,))
    late = Span(424242, "late", 1, None, (Annotation(5, "sr", Endpoint(9, 9, "first-seen-late-host")),
                                           Annotation(6, "first-seen-late-value", Endpoint(9, 9, "first-seen-late-host"))))
    spans.append(late)
    raw = [len(T.span(s)) if s.annotations else 0 for s in spans]
    budget = max(raw)  # the scratch asked for is smaller than the largest fragment: a slice holds that much
    assert budget > 22000 > 4096
    want_slices = greedy_slices(raw, budget)
    first = greedy_slices(raw[:-1], budget)  # the slices before the late span's
    assert want_slices >= 3 and first >= 2 and sum(raw[:-1]) > budget
    blobs = encode_all(spans)
    hd, hcols, hrej, want = host_annotated(blobs)
    assert len(want) >= 4_000
    small, big = device()(512, scratch_bytes=4096), device()(512)
    dcols, drej, rows = small.decode(blobs, strict=False, annotated=True)
    bcols, brej, brows = big.decode(blobs, strict=False, annotated=True)
    assert drej == brej == hrej == 0
    assert dev_rows(small, rows) == dev_rows(big, brows) == want
    assert small.rows_stats()["slices"] == want_slices and big.rows_stats()["slices"] == 1
    assert want[-1][5] == "first-seen-late-host" and want[-1][3] == hash_string("first-seen-late-value")
    for h in {r[3] for r in want}:
        assert small.string(h) == big.string(h) == hd.string(h)
    assert small.string(want[-1][3]) == "first-seen-late-value"
    same_records(small, dcols, hd, hcols)


# ---- 7. the dictionary -----------------------------------------------------------------------------------
def row_host_spans(k, first=0):
    e = Endpoint(1, 2, "svc")
    return [Span(1000 + j // 7, "op", j + 1, None, (Annotation(10 + j, "sr", e), Annotation(20 + j, "note", Endpoint(3, 4, "row-host-%d" % j)),
                                                    Annotation(30 + j, "ss", e))) for j in range(first, first + k)]


def test_row_hosts_enter_the_dictionary(gpu):
    spans = row_host_spans(5000)
    assert 5000 > EXTRA_CAPACITY
    blobs = encode_all(spans)
    hd, hcols, hrej, want = host_annotated(blobs)
    assert len(want) == 15000 and len({r[5] for r in want}) == 5001
    dd = device()(8192)
    dcols, drej, rows = dd.decode(blobs, strict=False, annotated=True)
    assert drej == 0 and dd.rows_stats()["slices"] == 1
    assert dev_rows(dd, rows) == want  # every id resolves to its name
    assert dd.num_services == 5001
    same_records(dd, dcols, hd, hcols)


def test_too_many_row_hosts_is_a_service_range_error(gpu):
    import torch

    from zipkin_amd.columns import DeviceColumns

    blobs = encode_all(row_host_spans(100))
    buf, off, n = upload(blobs)
    dd = device()(64)
    row = [torch.zeros(1024, dtype=torch.int64 if k < 4 else torch.int32, device="cuda") for k in range(7)]
    an = _abi.zk_ingest_annotation_rows(*[t.data_ptr() for t in row], 1024, 0)
    nout, nrej = C.c_uint64(), C.c_uint64()
    st = _abi.lib().zk_ingest_dev_spans_annotated(dd._h, buf.data_ptr(), off.data_ptr(), n, _abi.ZK_CODEC_SNAPPY_THRIFT, 0,
                                                  C.byref(DeviceColumns(n).abi(n)), C.byref(nout), C.byref(nrej), None,
                                                  C.byref(an))
    assert st == _abi.ZK_ERR_SERVICE_RANGE and an.n == 0
    with pytest.raises(ZkError) as err:
        dd.decode(blobs, strict=False, annotated=True)
    assert err.value.status == _abi.ZK_ERR_SERVICE_RANGE
    # a batch whose names the decoder took before it ran out still decodes
    e = Endpoint(1, 2, "svc")
    fits = [Span(5, "op", 1, None, (Annotation(1, "sr", e), Annotation(2, "again", e), Annotation(3, "ss", None)))]
    hd, hcols, hrej, want = host_annotated(encode_all(fits))
    dcols, drej, rows = dd.decode(encode_all(fits), annotated=True)
    assert drej == 0 and dev_rows(dd, rows) == want and len(want) == 3


# ---- 8. strings ------------------------------------------------------------------------------------------
def test_more_new_values_than_the_string_set_holds_and_no_row_strings(gpu):
    per, k = 100, 700
    assert per * k > SET_CAPACITY
    e = Endpoint(1, 2, "svc")
    spans = [Span(1 + j // 5, "op", j + 1, None, tuple(Annotation(1 + i, "value-%d-%d" % (j, i), e if i % 2 else None) for i in range(per)))
             for j in range(k)]
    blobs = encode_all(spans, False)  # (the thrift codec is read in place: one slice)
    hd, hcols, hrej, want = host_annotated(blobs, snappy=False)
    values = {r[3] for r in want}
    assert len(want) == per * k and len(values) == per * k > SET_CAPACITY
    dd, quiet = device()(64), device()(64)
    dcols, drej, rows = dd.decode(blobs, snappy=False, annotated=True, row_cap=per * k)
    assert drej == 0 and dd.rows_stats()["slices"] == 1
    assert dev_rows(dd, rows) == want
    for h in values:
        assert dd.string(h) == hd.string(h)
    # without the capture the rows are the same and the decoder learns no text from them
    qcols, qrej, qrows = quiet.decode(blobs[:50], snappy=False, annotated=True, row_cap=per * 50, row_strings=False)
    assert dev_rows(quiet, qrows) == want[: per * 50]
    for h in (want[0][3], want[per * 50 - 1][3]):
        with pytest.raises(ZkError):
            quiet.string(h)
    core = encode_all([Span(3, "op", 4, None, (Annotation(1, "cs", e), Annotation(2, "cr", e)))])
    quiet.decode(core, annotated=True, row_strings=False)
    with pytest.raises(ZkError):
        quiet.string(hash_string("cs"))
    quiet.decode(core, annotated=True)
    assert quiet.string(hash_string("cs")) == "cs" and quiet.string(hash_string("cr")) == "cr"
    with pytest.raises(ZkError):
        quiet.string(hash_string("sr"))  # (no row carried it)


# ---- 9. capacity -----------------------------------------------------------------------------------------
def test_capacity_keeps_the_first_rows_and_the_wrapper_retries(gpu):
    import torch

    from zipkin_amd.annotstore import DeviceAnnotationRows
    from zipkin_amd.columns import DeviceColumns

    spans = gen_traces(209, 40) + _odd_spans()
    blobs = encode_all(spans)
    hd, hcols, hrej, want = host_annotated(blobs)
    total = len(want)
    assert total > 300
    buf, off, n = upload(blobs)
    L = _abi.lib()
    PAD, MARK8, MARK4 = 16, 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
    for cap, status in ((total - 1, _abi.ZK_ERR_CAPACITY), (1, _abi.ZK_ERR_CAPACITY), (total, _abi.ZK_OK)):
        dd = device()(256)
        row = [torch.full((cap + PAD,), MARK8 if k < 4 else MARK4, dtype=torch.int64 if k < 4 else torch.int32, device="cuda")
               for k in range(7)]
        an = _abi.zk_ingest_annotation_rows(*[t.data_ptr() for t in row], cap, 0)
        cols = DeviceColumns(n)
        nout, nrej = C.c_uint64(), C.c_uint64()
        st = L.zk_ingest_dev_spans_annotated(dd._h, buf.data_ptr(), off.data_ptr(), n, _abi.ZK_CODEC_SNAPPY_THRIFT, 0,
                                             C.byref(cols.abi(n)), C.byref(nout), C.byref(nrej), None, C.byref(an))
        assert st == status, cap
        assert an.n == cap and nout.value == n
        assert dev_rows(dd, DeviceAnnotationRows(*[t[:cap] for t in row])) == want[:cap]
        for k, t in enumerate(row):  # nothing behind the capacity is written
            assert t[cap:].cpu().tolist() == [MARK8 if k < 4 else MARK4] * PAD
        cols.n = n
        same_records(dd, cols, hd, hcols)
    # the wrapper decodes again with 4x the room until the rows fit
    dd = device()(256)
    dcols, drej, rows = dd.decode(blobs, strict=False, annotated=True, row_cap=3)
    assert dev_rows(dd, rows) == want


# ---- 10. multi -------------------------------------------------------------------------------------------
def test_multi_equals_one_decode_of_the_joined_fragments(gpu):
    spans = gen_traces(210, 120, max_depth=4, anomalies=0.3) + _odd_spans()
    blobs = _fuzz(encode_all(spans), 210)
    cut = len(blobs) // 3
    batches = [upload(blobs[:cut]), upload([]), upload(blobs[cut:])]
    hd, hcols, hrej, want = host_annotated(blobs)
    assert len(want) > 1_000
    d1, d2 = device()(512), device()(512)
    c1, r1, e1 = d1.decode(blobs, strict=False, annotated=True)
    c2, r2, e2 = d2.decode_device_many(batches, strict=False, annotated=True)
    assert r1 == r2 == hrej
    assert dev_rows(d2, e2) == dev_rows(d1, e1) == want
    same_records(d2, c2, hd, hcols)


# ---- 11. end to end --------------------------------------------------------------------------------------
def golden_cases():
    """the hand-worked traces a decoder accepts: thrift.scala rejects an annotation with a timestamp <= 0"""
    return [c for c in tsaref.golden()["cases"] if all(a[0] > 0 and a[1] for s in c["spans"] for a in s["annotations"])]


def golden_spans():
    out = []
    for case in golden_cases():
        for s in case["spans"]:
            anns = tuple(Annotation(t, text, None if ip is None else Endpoint(ip - (1 << 32) if ip >= 1 << 31 else ip, 80, "svc-%d" % (ip & 0xFF)))
                         for t, text, ip in s["annotations"])
            out.append(Span(case["trace_id"], "rpc", s["id"], s["parent"], anns))
    return out


def test_stores_fed_on_the_device_answer_as_stores_fed_through_the_host(gpu):
    from zipkin_amd import DeviceAnnotationRows, SpanRetention, TraceAnnotationStore, TraceSpanStore
    from zipkin_amd.columns import DeviceColumns

    gold = golden_spans()
    spans = gold + gen_traces(211, 60, max_depth=4)
    ids = sorted({s.trace_id & U64 for s in spans})
    blobs = encode_all(spans)
    parts = [blobs[: len(blobs) // 2], blobs[len(blobs) // 2:]]
    dd, hd = device()(256), SpanDecoder()
    with TraceAnnotationStore(device=gpu) as dan, TraceSpanStore(device=gpu) as dsp, \
            TraceAnnotationStore(device=gpu) as han, TraceSpanStore(device=gpu) as hsp:
        total = 0
        for p in parts:
            buf, off, n = upload(p)
            cols, rej, m = dan.observe_stored(dd, buf, off, n, spans=dsp)  # (no column leaves the device)
            assert rej == 0 and cols.n == n and dan._held is not None and dan._held.trace_id.is_cuda and dsp._held is cols
            hcols, hrej, hrows = hd.decode_annotated(p, row_cap=16 * len(p))
            assert hrej == 0 and m == len(hrows)
            total += m
            han.observe(DeviceAnnotationRows.from_host(hrows, gpu))
            hsp.observe(DeviceColumns.from_host(hcols))
        assert dan.info()["entries"] == han.info()["entries"] == total == len(expected_rows(spans)) > 1_000
        assert dsp.info()["entries"] == hsp.info()["entries"] == len(spans)
        assert dan._held is None and dsp._held is None
        dsp.services, hsp.services = dd.service_names(), hd.service_names()

        def summaries(sp, an):
            # (a span's entries come ascending by service id, and ids are each decoder's own: compared as a bag)
            return [(s.trace_id, s.start, s.end, s.duration_micro, sorted(tuple(x) for x in s.span_timestamps), s.endpoints)
                    for s in sp.getTraceSummariesByIds(ids, adjust=("TIME_SKEW",), annotations=an, adjust_on_device=True)]

        def timelines(sp, an, dec):
            return [(t.trace_id, t.root_span_id, [tuple(a) for a in t.annotations])
                    for t in sp.getTraceTimelinesByIds(ids, adjust=("TIME_SKEW",), annotations=an, decoder=dec)]

        got = summaries(dsp, dan)
        assert got == summaries(hsp, han) and len(got) == len(ids)
        by_id = {g[0]: g for g in got}
        assert len(golden_cases()) >= 8
        for case in golden_cases():  # the hand-worked answers, from bytes that never left the device
            assert list(by_id[case["trace_id"]][1:3]) == case["expect"]["start_end"]
        lines = timelines(dsp, dan, dd)
        assert lines == timelines(hsp, han, hd) and len(lines) == len(ids)
        assert any(isinstance(a[1], str) and a[1] not in ("cs", "cr", "sr", "ss") for t in lines for a in t[2])
        # retention at a cutoff inside the data: both pairs hold the same traces afterwards
        ends = sorted(g[2] for g in got)
        now = ends[len(ends) // 2] + 3600 * 1_000_000
        out_d = SpanRetention(ttl_seconds=3600, spans=dsp, annotations=dan).expire(now)
        out_h = SpanRetention(ttl_seconds=3600, spans=hsp, annotations=han).expire(now)
        assert out_d == out_h and out_d["spans"] > 0 and out_d["annotations"] > 0
        alive = dsp.tracesExist(ids)
        assert alive == hsp.tracesExist(ids) and 0 < len(alive) < len(ids)
        held = lambda an: {i for i, rows in zip(ids, an.getAnnotationsByTraceIds(ids)) if rows}
        assert held(dan) == held(han) == alive
