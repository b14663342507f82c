"""The host decoder's binary-annotation rows (include/zkingest.h, zk_ingest_spans_annotated_binary) against
tests/binref.py's restatement over oracle.spans, the wire forms of a BinaryAnnotation, the capacity prefix, the
thread-count independence and the captured bytes. No GPU: the host decoder is the device decoder's oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle.spans import UNKNOWN_SERVICE_NAME, Annotation, BinaryAnnotation, Endpoint, Span
from tests import binref as B
from tests import thriftenc as T
from tests.richgen import gen_traces
from tests.test_ingest import bad_spans, encode_all, records
from tests.test_ingest_annotated import expected_rows, named_records, named_rows
from zipkin_amd import SpanColumns, ZkError, _abi
from zipkin_amd.annotstore import AnnotationRows
from zipkin_amd.binannotstore import BINARY_ROW_COLUMNS, BinaryAnnotationRows
from zipkin_amd.ingest import DeviceSpanDecoder, SpanDecoder, _pack, hash_string


@pytest.mark.parametrize("seed,snappy", [(21, True), (22, False)])
def test_rows_of_generated_fragments(seed, snappy):
    frags = B.gen_frags(seed, 400)
    fl = B.floors(frags)
    assert fl["rows"] >= 1200 and min(fl["per_type"]) >= 40 and fl["hostless"] >= 300 and fl["binary_only"] >= 80
    assert fl["time_only"] >= 20 and fl["two_lists"] >= 40 and fl["unknown_hosts"] >= 100
    blobs = B.encode_all(frags, snappy)
    dec, plain = SpanDecoder(), SpanDecoder()
    cols, rej, rows, brows = dec.decode_annotated(blobs, snappy=snappy, binary=True, binary_cap=fl["rows"])
    assert rej == 0 and len(cols) == len(frags)
    assert B.named_binary_rows(brows, dec.service_names()) == B.expected_binary_rows(frags)
    # records and time rows are zk_ingest_spans_annotated's (service ids through names: the binary rows' hosts
    # enter the dictionary too, after each record's time rows)
    cols0, rej0, rows0 = plain.decode_annotated(blobs, snappy=snappy)
    assert named_records(cols, dec) == named_records(cols0, plain) and rej0 == 0
    assert named_rows(rows, dec) == named_rows(rows0, plain) == expected_rows([f.span for f in frags])
    # every key's and value's bytes are kept, with their length
    texts = B.strings_of(frags)
    assert any(b"\0" in b for b in texts.values()) and any(len(b) == 3000 for b in texts.values())
    for h, b in texts.items():
        assert dec.bytes(h) == b
        assert dec.string(h) == b.decode("utf-8", "surrogateescape")


def test_rich_traces_and_the_plain_annotated_call_on_the_same_bytes():
    """tests/richgen.py's spans (their binaries are all b"v" / String / hosted) through both calls with item
    buffers and ZK_INGEST_SPAN_NAMES: records, rejected, items, names, time rows and dictionary ids are equal."""
    ok, bads = bad_spans()
    spans = gen_traces(32, 60, max_depth=4, anomalies=0.3)
    blobs = encode_all(spans, False)
    for k, (_, b) in enumerate(bads):
        blobs.insert(7 * k + 3, b)
    buf, offsets, n = _pack(blobs)
    L = _abi.lib()
    out = []
    for binary in (False, True):
        dec = SpanDecoder()
        cols = SpanColumns.empty(n)
        arrs = (np.zeros(8 * n, np.uint32), np.zeros(8 * n, np.uint64), np.zeros(8 * n, np.uint32), np.zeros(8 * n, np.uint64))
        it = _abi.zk_ingest_items(arrs[0].ctypes.data, arrs[1].ctypes.data, 8 * n, 0, arrs[2].ctypes.data, arrs[3].ctypes.data, 8 * n, 0)
        nout, nrej, ab = C.c_uint64(), C.c_uint64(), cols.abi()
        rows = AnnotationRows.empty(16 * n)
        an = rows.ingest_abi(cap=16 * n, n=0)
        args = (dec._h, buf.ctypes.data, offsets.ctypes.data, n, _abi.ZK_CODEC_THRIFT, _abi.ZK_INGEST_SPAN_NAMES, C.byref(ab),
                C.byref(nout), C.byref(nrej), C.byref(it), C.byref(an))
        if binary:
            brows = BinaryAnnotationRows.empty(16 * n)
            bn = brows.ingest_abi(cap=16 * n, n=0)
            st = L.zk_ingest_spans_annotated_binary(*args, C.byref(bn))
        else:
            st = L.zk_ingest_spans_annotated(*args)
        assert st == _abi.ZK_OK
        kept = cols.take(slice(0, nout.value))
        # (the RAW ids too: on these spans every binary host is a time-row host of its record already, so the
        # dictionaries of the two calls are equal id for id)
        out.append((records(kept), int(nrej.value), dec.span_names(), dec.service_names(), arrs[0][:it.kv_n].tolist(),
                    arrs[1][:it.kv_n].tolist(), arrs[2][:it.ann_n].tolist(), arrs[3][:it.ann_n].tolist(),
                    rows.take(slice(0, int(an.n))).rows()))
    assert out[0] == out[1] and out[0][1] == len(bads) and len(out[0][4]) and len(out[0][6]) and len(out[0][8]) > 100
    want = B.expected_binary_rows(spans)
    assert B.named_binary_rows(brows.take(slice(0, int(bn.n))), out[1][3]) == want and len(want) > 50


def test_wire_forms():
    e = Endpoint(1, 2, "a")
    H = B.HostPart
    bs = (
        BinaryAnnotation("k", b"v", "BOOL", e),                                   # 0 every type by its ordinal
        BinaryAnnotation("k", b"v", "BYTES", e), BinaryAnnotation("k", b"v", "I16", e), BinaryAnnotation("k", b"v", "I32", e),
        BinaryAnnotation("k", b"v", "I64", e), BinaryAnnotation("k", b"v", "DOUBLE", e), BinaryAnnotation("k", b"v", "STRING", e),
        BinaryAnnotation("k", b"v", 7, e), BinaryAnnotation("k", b"v", -1, e),    # 7, 8 out of range
        BinaryAnnotation("k", b"v", None, e),                                     # 9 no type
        BinaryAnnotation(None, b"v", 6, e), BinaryAnnotation("k", None, 6, e),    # 10, 11 no key, no value
        BinaryAnnotation("k", b"v", 6, None),                                     # 12 no host
        BinaryAnnotation("k", b"v", ("i16", 6), e),                               # 13 field 3 as another wire type
        BinaryAnnotation("k", b"v", [3, ("i64", 5)], e),                          # 14 ... behind a right one
        BinaryAnnotation("k", b"v", [1, 2], e),                                   # 15 the last occurrence wins
        BinaryAnnotation("k", b"v", 6, (H(7, 8, "first"), H(name="second"))),      # 16 a later struct keeps ipv4 and port
        BinaryAnnotation("k", b"v", 6, (H(7, 8, "first"), H(ipv4=9))),             # 17 ... and the name
        BinaryAnnotation("k", b"v", 6, (H(-2 ** 31, -2 ** 15, ""),)),             # 18 the bounds, an empty name
        BinaryAnnotation("k", b"v", 6, (H(),)),                                   # 19 a bare host struct
    )
    span = Span(2 ** 63, "n", -1, None, (Annotation(5, "sr", Endpoint(3, 4, "own")),), bs)
    for snappy in (False, True):
        for split in (None, 10):
            dec = SpanDecoder()
            blob = B.encode(B.Frag(span, split))
            cols, rej, rows, brows = dec.decode_annotated([T.snappy(blob) if snappy else blob], snappy=snappy, binary=True, binary_cap=64)
            assert rej == 0 and len(cols) == 1 and len(rows) == 1 and len(brows) == len(bs)
            assert set(brows.trace_id.tolist()) == {2 ** 63} and set(brows.span_id.tolist()) == {2 ** 64 - 1}
            names = dec.service_names()
            # the record's own service, its time row's host, then the binary rows' hosts in row order
            assert names == ["own", "a", "second", "first", UNKNOWN_SERVICE_NAME]
            got = B.named_binary_rows(brows, names)
            assert got == B.expected_binary_rows([span])
            assert [r[6] & 7 for r in got] == [0, 1, 2, 3, 4, 5, 6, 7, 7, 0, 6, 6, 6, 0, 3, 2, 6, 6, 6, 6]
            assert [(r[4], r[6] >> 16, r[5]) for r in got[16:]] == [(7, 8, "second"), (9, 8, "first"), (0x80000000, 0x8000, UNKNOWN_SERVICE_NAME),
                                                                     (0, 0, UNKNOWN_SERVICE_NAME)]
            assert got[12][4:] == (0, None, 6) and got[10][2] == got[11][3] == hash_string("") != hash_string("k")
            assert got[0][3] == hash_string("v") and got[0][3] & 1 == hash_string("v") & 1  # (no `| 1`: the plain hash)
            # the plain calls read the same bytes to the same record and time rows
            cols0, _, rows0 = SpanDecoder().decode_annotated([T.snappy(blob) if snappy else blob], snappy=snappy)
            assert records(cols0) == records(cols) and rows0.rows()[0][:5] == rows.rows()[0][:5]
    assert any(hash_string(x) & 1 == 0 for x in ("v", "k", "a", "b"))  # (an even hash exists: `| 1` would show)


def test_one_thread_against_many():
    frags = B.gen_frags(23, 3 * 2048 + 100)
    blobs = B.encode_all(frags, False)
    ok, bads = bad_spans()
    for k in range(12):
        blobs.insert(len(blobs) * k // 12 + 5, bads[k % len(bads)][1] if k % 3 else b"\x7f\x00garbage")
    out = []
    for one in (True, False):
        dec = SpanDecoder()
        cols, rej, rows, brows = dec.decode_annotated(blobs, snappy=False, strict=False, one_thread=one, span_names=True,
                                                      row_cap=4 * len(blobs), binary=True, binary_cap=8 * len(blobs))
        out.append((records(cols), rej, rows.rows(), brows.rows(), dec.service_names(), dec.span_names()))
    assert out[0] == out[1] and out[0][1] == 12 and len(out[0][3]) > 20000
    assert B.named_binary_rows(brows, out[1][4]) == B.expected_binary_rows(frags)


def test_a_cap_that_is_too_small():
    frags = B.gen_frags(24, 40)
    blobs = B.encode_all(frags)
    _, _, full, bfull = SpanDecoder().decode_annotated(blobs, binary=True)
    nt, nb = len(full), len(bfull)
    assert nt >= 60 and nb >= 100
    for rcap, bcap in ((nt, nb - 1), (nt, 1), (nt - 1, nb), (1, nb), (3, 5), (nt, 0)):
        dec = SpanDecoder()
        with pytest.raises(ZkError) as ex:
            dec.decode_annotated(blobs, row_cap=rcap, binary=True, binary_cap=bcap)
        assert ex.value.status == _abi.ZK_ERR_CAPACITY
        # the two capacities are judged independently: each list is the prefix that fitted; the records are all there
        assert len(ex.value.rows) == rcap and len(ex.value.brows) == bcap and len(ex.value.cols) == len(frags)
        assert [r[:5] + r[6:] for r in ex.value.rows.rows()] == [r[:5] + r[6:] for r in full.rows()[:rcap]]
        assert [r[:5] + r[6:] for r in ex.value.brows.rows()] == [r[:5] + r[6:] for r in bfull.rows()[:bcap]]
        names = dec.service_names()
        assert B.named_binary_rows(ex.value.brows, names) == B.expected_binary_rows(frags)[:bcap]
    dec = SpanDecoder()
    cols, rej, rows, brows = dec.decode_annotated(blobs, row_cap=nt, binary=True, binary_cap=nb)
    assert rows.rows() == full.rows() and brows.rows() == bfull.rows() and len(cols) == len(frags)


def test_null_arguments_layouts_and_an_empty_batch():
    L, dec = _abi.lib(), SpanDecoder()
    cols, nout, nrej = SpanColumns.empty(1), C.c_uint64(), C.c_uint64()
    rows, brows = AnnotationRows.empty(4), BinaryAnnotationRows.empty(4)
    ab, buf, off = cols.abi(), np.zeros(1, np.uint8), np.zeros(2, np.uint64)
    an, bn = rows.ingest_abi(), brows.ingest_abi()
    args = (dec._h, buf.ctypes.data, off.ctypes.data, 1, 0, 0, C.byref(ab), C.byref(nout), C.byref(nrej), None)
    assert L.zk_ingest_spans_annotated_binary(*args, C.byref(an), None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_spans_annotated_binary(*args, None, C.byref(bn)) == _abi.ZK_ERR_INVALID_ARG
    for k, _ in BINARY_ROW_COLUMNS:
        bad = brows.ingest_abi()
        setattr(bad, k, None)
        assert L.zk_ingest_spans_annotated_binary(*args, C.byref(an), C.byref(bad)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_spans_annotated_binary(None, *args[1:], C.byref(an), C.byref(bn)) == _abi.ZK_ERR_INVALID_ARG
    bn = brows.ingest_abi(cap=4, n=99)
    assert L.zk_ingest_spans_annotated_binary(dec._h, None, None, 0, 0, 0, C.byref(ab), C.byref(nout), C.byref(nrej), None,
                                              C.byref(an), C.byref(bn)) == _abi.ZK_OK
    assert int(bn.n) == 0
    assert C.sizeof(_abi.zk_ingest_binary_rows) == C.sizeof(_abi.zk_ingest_annotation_rows) == 72
    assert [f[0] for f in _abi.zk_ingest_binary_rows._fields_] == [k for k, _ in BINARY_ROW_COLUMNS] + ["cap", "n"]
    cols, rej, rows, brows = dec.decode_annotated([], binary=True)
    assert len(cols) == 0 and rej == 0 and len(rows) == 0 and len(brows) == 0


FAKE = C.c_void_p(0x1000)  # stands for a device decoder's handle: the argument check comes before any use of it


def test_the_device_calls_refuse_nulls_before_any_device_is_touched():
    L = _abi.lib()
    an, brows = AnnotationRows.empty(4).ingest_abi(cap=4, n=0), BinaryAnnotationRows.empty(4)
    n, r = C.c_uint64(), C.c_uint64()

    def calls(handle, a, b):
        yield L.zk_ingest_dev_spans_annotated_binary(handle, None, None, 0, 0, 0, None, C.byref(n), C.byref(r), None, a, b)
        yield L.zk_ingest_dev_spans_multi_annotated_binary(handle, 0, None, None, None, 0, 0, None, C.byref(n), C.byref(r), None, a, b)

    bn = brows.ingest_abi(cap=4, n=0)
    assert list(calls(None, C.byref(an), C.byref(bn))) == [_abi.ZK_ERR_INVALID_ARG] * 2
    assert list(calls(FAKE, None, C.byref(bn))) == [_abi.ZK_ERR_INVALID_ARG] * 2
    assert list(calls(FAKE, C.byref(an), None)) == [_abi.ZK_ERR_INVALID_ARG] * 2
    for k, _ in BINARY_ROW_COLUMNS:
        bad = brows.ingest_abi(cap=4, n=0)
        setattr(bad, k, None)
        assert list(calls(FAKE, C.byref(an), C.byref(bad))) == [_abi.ZK_ERR_INVALID_ARG] * 2
    for sym in ("zk_ingest_dev_spans_annotated_binary", "zk_ingest_dev_spans_multi_annotated_binary", "zk_ingest_spans_annotated_binary"):
        assert sym in list(_abi.SYMBOLS)


@pytest.mark.parametrize("method", ["decode", "decode_device", "decode_device_many"])
def test_binary_without_annotated_is_a_value_error_before_any_library_call(method):
    dd = DeviceSpanDecoder.__new__(DeviceSpanDecoder)  # (no handle: the check comes first)
    args = {"decode": ([b"x"],), "decode_device": (None, None, 1), "decode_device_many": ([],)}[method]
    with pytest.raises(ValueError, match="annotated=True"):
        getattr(dd, method)(*args, binary=True)
