"""Span-name ids from the DEVICE decoder (ZK_INGEST_SPAN_NAMES on a decoder made by
zk_ingest_dev_create_names; include/zkingest.h). The reference is always the host decoder on the same
bytes, compared BY NAME: device ids follow hash-table slot order, the host's first appearance. Covered:
both codecs; name lengths around the 16-byte inline prefix of a table slot; every decode path (the
canonical layout, the generic walk, a fragment deferred to the global-memory decoder, a batch decoded
again after the scratch ran out); the multi-batch and the items entry points; a 16-slot table with its
capacity error and rollback; the 65535-name hard cap; and the realtime store fed from stored bytes."""
import numpy as np
import pytest

from oracle.spans import Annotation, Endpoint, Span
from tests import namefrag, rpc_rows, thriftenc
from tests.bulkfrag import service_name
from tests.rpc_rows import R, assign_names
from tests.test_span_names import NAMES, _blobs, _span
from zipkin_amd import ZkError, _abi, tracegen_host
from zipkin_amd.aggregates import DecoderDictionary, GpuRealtimeAggregates
from zipkin_amd.ingest import DeviceSpanDecoder, SpanDecoder

pytestmark = pytest.mark.gpu

COLS = ("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "service_id", "flags")
NONE = ("", "Unknown")


def by_name(dec, cols):
    """every record's span name ("" for id 0) and service name (None without a service)"""
    ids = cols.name_ids().tolist()
    names = dec.span_names()
    snames = dec.service_names()
    has = (cols.flags & np.uint32(_abi.ZK_F_SVC_SERVER | _abi.ZK_F_SVC_CLIENT)) != 0
    return ([names[k - 1] if k else "" for k in ids],
            [snames[int(s)] if h else None for s, h in zip(cols.service_id.tolist(), has.tolist())])


def assert_same_records(dd, dcols, hd, hcols):
    """device records == host records, names and services compared by name, the rest exactly"""
    assert len(dcols) == len(hcols)
    assert by_name(dd, dcols) == by_name(hd, hcols)
    for k in ("trace_id", "span_id", "parent_id", "first_ts", "last_ts"):
        assert np.array_equal(getattr(dcols, k), getattr(hcols, k)), k
    assert np.array_equal(dcols.flags & np.uint32(0xFFFF), hcols.flags & np.uint32(0xFFFF))


def decode_both(dd, hd, blobs, snappy=True, strict=True, **kw):
    dcols, drej = dd.decode(blobs, snappy=snappy, strict=strict, span_names=True, **kw)
    hcols, hrej = hd.decode(blobs, snappy=snappy, strict=strict, span_names=True)
    dcols = dcols.to_host()
    assert drej == hrej
    assert_same_records(dd, dcols, hd, hcols)
    ids = dcols.name_ids()
    assert ids.max(initial=0) <= dd.num_span_names
    return dcols, hcols


def test_a_plain_decoder_has_no_span_names(gpu):
    dd = DeviceSpanDecoder(64)
    assert dd.num_span_names == 0 and dd.span_names() == []
    with pytest.raises(ZkError) as e:
        dd.span_name(0)
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG
    with pytest.raises(ZkError) as e:
        dd.decode(_blobs(NAMES), span_names=True)
    assert e.value.status == _abi.ZK_ERR_UNSUPPORTED
    dd.close()


@pytest.mark.parametrize("snappy", [True, False])
def test_the_host_tests_list(gpu, snappy):
    blobs = [thriftenc.span(_span(i, nm, parent=7 if i % 3 else None)) for i, nm in enumerate(NAMES)]
    if snappy:
        blobs = [thriftenc.snappy(b) for b in blobs]
    dd, hd = DeviceSpanDecoder(64, max_span_names=100), SpanDecoder()
    dcols, _ = decode_both(dd, hd, blobs, snappy)
    assert sorted(dd.span_names()) == sorted(hd.span_names()) == sorted(["get", "put", "post", "unknown", "delete"])
    got = by_name(dd, dcols)[0]
    assert got == ["" if nm in NONE else nm for nm in NAMES]
    # every column equals the flag-less decode once bits 16..31 are masked; the flag-less decode on
    # the same decoder has zero high halves and leaves the dictionary alone
    plain, _ = dd.decode(blobs, snappy=snappy)
    plain = plain.to_host()
    assert not (plain.flags >> np.uint32(16)).any() and dd.num_span_names == 5
    masked = dcols.without_names()
    for k in COLS:
        assert np.array_equal(getattr(masked, k), getattr(plain, k)), k
    fresh = DeviceSpanDecoder(64, max_span_names=100)
    fresh.decode(blobs, snappy=snappy)
    assert fresh.num_span_names == 0
    # a second batch reuses put's id and adds one
    put = dd.span_names().index("put")
    more = [thriftenc.span(_span(i, nm)) for i, nm in enumerate(["head", "put"])]
    if snappy:
        more = [thriftenc.snappy(b) for b in more]
    mcols, _ = dd.decode(more, snappy=snappy, span_names=True)
    assert dd.num_span_names == 6 and dd.span_name(5) == "head"
    assert mcols.to_host().name_ids().tolist() == [6, put + 1]
    for d in (dd, fresh):
        d.close()


SHAPES = [b"x", b"a" * 15, b"b" * 16, b"c" * 17,
          b"0123456789abcdefX", b"0123456789abcdefY",      # equal in their first 16 bytes
          b"0123456789abcdef", b"0123456789abcde",          # differ only in length (16 / 15)
          b"L" * 300, b"nul\x00and\xff\xfe", "app", "web", b"Unknown!", b"Unknow", b"unknown"]


@pytest.mark.parametrize("snappy", [True, False])
def test_name_shapes(gpu, snappy):
    """the edges of the slot's 16-byte inline prefix, a long name, arbitrary bytes, a name that is also a
    service name of the batch ("app", "web"), and near misses of "Unknown"; twice, so that the second
    batch resolves every name inside the decode kernel"""
    names = SHAPES + ["Unknown", ""] + SHAPES[::-1]
    blobs = [thriftenc.span(_span(i, nm)) for i, nm in enumerate(names)]
    if snappy:
        blobs = [thriftenc.snappy(b) for b in blobs]
    dd, hd = DeviceSpanDecoder(64, max_span_names=64), SpanDecoder()
    for _ in range(2):
        dcols, _ = decode_both(dd, hd, blobs, snappy)
        assert dd.num_span_names == len(SHAPES) == hd.num_span_names
        assert sorted(dd.span_names()) == sorted(hd.span_names())
        assert len(set(dcols.name_ids().tolist())) == len(SHAPES) + 1
    # the two dictionaries are separate: "app" is in both, with unrelated ids
    assert "app" in dd.service_names() and "app" in dd.span_names()
    dd.close()


def _out_of_order(i, name):
    """a Span with its fields out of id order (name last, after a second, earlier name field)"""
    s = _span(i, name)
    body = thriftenc.span(s, name=None)[:-1]  # no name, STOP removed
    return body + thriftenc._fh(thriftenc.T_STRING, 3) + thriftenc._str("earlier") + \
        thriftenc._fh(thriftenc.T_STRING, 3) + thriftenc._str(name) + bytes([thriftenc.T_STOP])


@pytest.mark.parametrize("snappy", [True, False])
def test_every_decode_path(gpu, snappy):
    """canonical layout (fast path), fields out of order (generic walk: the last name field wins), and a
    fragment with one annotation value longer than the LDS decoder's 20480-byte budget, which goes to
    the global-memory decoder"""
    rng = np.random.default_rng(7)
    big = bytes(rng.integers(97, 123, 30000, dtype=np.uint8))  # (poorly compressible: > 20480 B compressed too)
    giant = Span(5, "giant-name", 6, None, (Annotation(10, big.decode(), Endpoint(1, 2, "app")),
                                            Annotation(11, "sr", Endpoint(1, 2, "app"))))
    raw = [thriftenc.span(_span(0, "fast")), _out_of_order(1, "generic"), thriftenc.span(giant),
           thriftenc.span(_span(2, "Unknown")), _out_of_order(3, ""), thriftenc.span(_span(4, "fast")),
           _out_of_order(5, "a-name-longer-than-sixteen-bytes")]
    blobs = [thriftenc.snappy(b) for b in raw] if snappy else raw
    assert len(blobs[2]) > 20480
    dd, hd = DeviceSpanDecoder(64, max_span_names=16), SpanDecoder()
    for _ in range(2):  # new names, then known names, on every path
        dcols, _ = decode_both(dd, hd, blobs, snappy)
        assert by_name(dd, dcols)[0] == ["fast", "generic", "giant-name", "", "", "fast",
                                         "a-name-longer-than-sixteen-bytes"]
    assert dd.num_span_names == 4
    dd.close()


def test_scratch_runs_out_and_the_batch_is_decoded_again(gpu):
    """~3000 Snappy fragments with 500 distinct new names and a 64-byte scratch: the copy-out of most
    names fails on the first attempt (kStNoScratch), the scratch grows and those fragments are decoded
    again. Every fragment ends with one id, ids and names are a bijection, records equal the host's."""
    pool = ["name-%03d-%s" % (k, "x" * (k % 23)) for k in range(500)]
    rng = np.random.default_rng(8)
    names = pool + [pool[k] for k in rng.integers(0, 500, 2500)] + ["", "Unknown"]
    blobs = _blobs(names)
    dd, hd = DeviceSpanDecoder(64, max_span_names=600, scratch_bytes=64), SpanDecoder()
    dcols, _ = decode_both(dd, hd, blobs)
    got = dd.span_names()
    assert len(got) == 500 and sorted(got) == sorted(pool)
    ids = dcols.name_ids().tolist()
    pairs = {(k, nm) for k, nm in zip(ids, names) if k}
    assert len(pairs) == 500 and len({k for k, _ in pairs}) == 500
    decode_both(dd, hd, blobs)  # and again, every name known
    assert dd.num_span_names == 500
    dd.close()


def test_multi_batch_equals_the_joined_single_decode(gpu):
    import torch

    parts = [NAMES[:7], [], NAMES[7:] + ["head", "a-seventeen-b-name"]]
    blobs = [_blobs(p) for p in parts]
    # distinct span ids across the parts
    blobs[2] = [thriftenc.snappy(thriftenc.span(_span(20 + i, nm))) for i, nm in enumerate(parts[2])]
    dd, one, hd = (DeviceSpanDecoder(64, max_span_names=32), DeviceSpanDecoder(64, max_span_names=32), SpanDecoder())
    batches = []
    for b in blobs:
        buf, off = namefrag.pack(b)
        batches.append((torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda(), len(b)))
    mcols, mrej = dd.decode_device_many(batches, span_names=True)
    mcols = mcols.to_host()
    joined = [x for b in blobs for x in b]
    scols, _ = one.decode(joined, span_names=True)
    hcols, _ = hd.decode(joined, span_names=True)
    assert mrej == 0
    assert_same_records(dd, mcols, one, scols.to_host())
    assert_same_records(dd, mcols, hd, hcols)
    assert sorted(dd.span_names()) == sorted(hd.span_names())
    for d in (dd, one):
        d.close()


def test_items_with_names(gpu):
    """items=True with the flag: the same item multisets as without it, the same names as items=False"""
    from collections import Counter

    from tests.richgen import gen_traces
    from tests.test_ingest import encode_all

    spans = gen_traces(111, 200, max_depth=5, anomalies=0.3)
    blobs = encode_all(spans, True)

    def items_of(dec, span_names):
        cols, rej, (ks, kh), (as_, ah) = dec.decode(blobs, strict=False, items=True, span_names=span_names)
        sv = dec.service_names()
        kv = Counter((sv[int(s)], dec.string(int(h))) for s, h in zip(ks.cpu().numpy(), kh.cpu().numpy()))
        an = Counter((sv[int(s)], dec.string(int(h))) for s, h in zip(as_.cpu().numpy(), ah.cpu().numpy()))
        return cols.to_host(), rej, kv, an

    a, b, c = (DeviceSpanDecoder(256, max_span_names=4096) for _ in range(3))
    hd = SpanDecoder()
    with_names = items_of(a, True)
    without = items_of(b, False)
    assert with_names[1:] == without[1:] and sum(with_names[2].values()) > 50
    assert not (without[0].flags >> np.uint32(16)).any() and b.num_span_names == 0
    ccols, crej = c.decode(blobs, strict=False, span_names=True)
    hcols, hrej = hd.decode(blobs, strict=False, span_names=True)
    assert crej == hrej == with_names[1]
    assert_same_records(a, with_names[0], c, ccols.to_host())
    assert_same_records(a, with_names[0], hd, hcols)
    assert a.num_span_names == hd.num_span_names >= 2
    # the second time every name resolves in the decode kernel
    again = items_of(a, True)
    assert again[1:] == with_names[1:]
    assert_same_records(a, again[0], hd, hcols)
    for d in (a, b, c):
        d.close()


def test_small_table_capacity_and_rollback(gpu):
    """max_span_names = 8: a 16-slot table (probe chains and the wrap are certain). Exactly 8 names fit; a
    batch needing a 9th fails as a whole with ZK_ERR_CAPACITY and leaves the dictionary as it was; known
    names then decode; a lenient batch's rejected fragment does not add its never-seen name."""
    eight = ["n%d" % k for k in range(8)]
    dd, hd = DeviceSpanDecoder(64, max_span_names=8), SpanDecoder()
    decode_both(dd, hd, _blobs(eight[:5] + ["", eight[0]]))
    decode_both(dd, hd, _blobs(eight[3:] + ["Unknown"]))
    before = dd.span_names()
    assert sorted(before) == eight
    for extra in (["ninth"], ["n1", "ninth", "tenth", "n2"], ["x%d" % k for k in range(40)]):
        with pytest.raises(ZkError) as e:
            dd.decode(_blobs(extra), span_names=True)
        assert e.value.status == _abi.ZK_ERR_CAPACITY and "max_span_names" in str(e.value)
        assert dd.span_names() == before
    # without the flag the same bytes are no error; known names decode and equal the host's
    cols, _ = dd.decode(_blobs(["ninth"]))
    assert cols.n == 1 and dd.span_names() == before
    dcols, _ = decode_both(dd, hd, _blobs(eight[::-1] + ["", "n3", "Unknown"]))
    assert by_name(dd, dcols)[0] == eight[::-1] + ["", "n3", ""]
    # lenient: the fragment with a non-positive timestamp is rejected and its name never enters
    few = DeviceSpanDecoder(64, max_span_names=8)
    bad = Span(9, "never-seen", 10, None, (Annotation(0, "sr", Endpoint(1, 2, "app")),))
    blobs = _blobs(["n0"]) + [thriftenc.snappy(thriftenc.span(bad))] + _blobs(["n1"])
    cols, rej = few.decode(blobs, strict=False, span_names=True)
    assert (cols.n, rej) == (2, 1) and sorted(few.span_names()) == ["n0", "n1"]
    assert sorted(by_name(few, cols.to_host())[0]) == ["n0", "n1"]  # (compacted: the flags moved with the records)
    for d in (dd, few):
        d.close()


def test_the_hard_cap(gpu):
    """one batch of 65535 distinct names fills the dictionary (id 65535 present in flags); one more new
    name is ZK_ERR_CAPACITY"""
    import torch

    n = 65535
    body = thriftenc.span(_span(1, "#####"))
    at = body.index(b"#####")
    mat = np.tile(np.frombuffer(body, np.uint8), (n, 1))
    digits = np.array([list(b"%05d" % k) for k in range(n)], np.uint8)
    mat[:, at:at + 5] = digits
    buf = torch.from_numpy(mat.reshape(-1).copy()).cuda()
    off = torch.from_numpy(np.arange(n + 1, dtype=np.int64) * len(body)).cuda()
    dd = DeviceSpanDecoder(64, max_span_names=65535)
    cols, rej = dd.decode_device(buf, off, n, snappy=False, span_names=True)
    ids = cols.to_host().name_ids()
    assert rej == 0 and dd.num_span_names == n
    assert sorted(ids.tolist()) == list(range(1, n + 1))  # every id once, 65535 among them
    names = dd.span_names()
    assert [names[k - 1] for k in ids[:50].tolist()] == ["%05d" % k for k in range(50)]
    with pytest.raises(ZkError) as e:
        dd.decode(_blobs(["00000", "one-too-many"]), span_names=True)
    assert e.value.status == _abi.ZK_ERR_CAPACITY
    assert dd.num_span_names == n
    cols, _ = dd.decode(_blobs(["65534", "", "00000"]), span_names=True)
    assert [names[k - 1] if k else "" for k in cols.to_host().name_ids().tolist()] == ["65534", "", "00000"]
    dd.close()


def in_dictionaries_of(dec, hd, hcols):
    """the host-decoded records with their service ids and name ids translated, BY NAME, into the
    device decoder's dictionaries"""
    dsvc, drpc = dec.service_names(), dec.span_names()
    smap = np.array([dsvc.index(n) for n in hd.service_names()], np.int64)
    nmap = np.array([0] + [drpc.index(n) + 1 for n in hd.span_names()], np.int64)
    out = hcols.take(np.arange(len(hcols)))
    out.service_id[:] = smap[hcols.service_id.astype(np.int64)].astype(out.service_id.dtype)
    out.set_name_ids(nmap[hcols.name_ids().astype(np.int64)])
    return out


def test_realtime_store_from_stored_bytes(gpu):
    """tracegen records with name ids (S = 11, 800 traces, rpc_rows.assign_names) -> stored fragments
    (tests/namefrag.py) -> accumulate_stored through a names-capable device decoder. For every server and
    every rpc name, "" and "Unknown", both trait answers equal those of rpc_rows over the HOST-decoded
    columns, keyed by service and rpc names.

    assign_names makes ~850 of the ~10300 spans of this batch carry two different names on their
    fragments, and the merged span takes the largest ID (K1 kModeLinks). Which name that is depends on
    the dictionary, so the host-decoded records are first translated by name into the store's
    dictionaries -- the device decoder's, which `services` and `rpcs` view (in_dictionaries_of); nothing
    else of them changes. The same store fed those host-decoded records through accumulate() gives the
    same answers as the one fed the stored bytes."""
    import torch

    S = 11
    rpc_names = ["rpc-%d" % k for k in range(R)]
    src = assign_names(tracegen_host(85, 800, max_depth=6, num_services=S), 85)
    blobs = namefrag.blobs(src, rpc_names)
    hd = SpanDecoder()
    hcols, hrej = hd.decode(blobs, span_names=True)
    assert hrej == 0 and len(hcols) == len(src) and sorted(hd.span_names()) == rpc_names

    hour = 3_600_000_000
    dec = DeviceSpanDecoder(64, max_span_names=32)
    store = GpuRealtimeAggregates(DecoderDictionary(dec), rpcs=DecoderDictionary(dec, "span_names"),
                                  num_services=dec.max_services)
    buf, off = namefrag.pack(blobs)
    rej = store.accumulate_stored(dec, torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda(), len(blobs), 5 * hour)
    assert rej == 0 and sorted(dec.span_names()) == rpc_names
    assert sorted(dec.service_names()) == [service_name(i) for i in range(S)]

    tcols = in_dictionaries_of(dec, hd, hcols)
    rows = rpc_rows.rpc_rows(tcols, dec.max_services)
    rpc_rows.assert_tied_to_oracle(rows, tcols, dec.max_services)
    dsvc, drpc = dec.service_names(), dec.span_names()
    assert len({r[4] for r in rows}) == R + 1

    def answers(server, rpc):  # rpc: None = any, "" = no name, else a name
        durs, tids = {}, {}
        for p, c, d, t, n in rows:
            if dsvc[c] == server and (rpc is None or (drpc[n - 1] if n else "") == rpc):
                durs.setdefault(dsvc[p], []).append(d)
                tids.setdefault(dsvc[p], set()).add(t - (1 << 64) if t >= 1 << 63 else t)
        return {k: sorted(v) for k, v in durs.items()}, {k: sorted(v) for k, v in tids.items()}

    twin = GpuRealtimeAggregates(DecoderDictionary(dec), rpcs=DecoderDictionary(dec, "span_names"),
                                 num_services=dec.max_services)
    twin.accumulate(tcols, 5 * hour)
    seen = 0
    for server in [service_name(i) for i in range(S)]:
        for rname, key in [("", None), ("Unknown", "")] + [(r, r) for r in rpc_names] + [("no-such-rpc", "?")]:
            want = answers(server, key)
            seen += bool(want[0])
            for st in (store, twin):
                assert st.getSpanDurations(5 * hour + 1, server, rname) == want[0], (server, rname)
                assert st.getServiceNamesToTraceIds(5 * hour + 1, server, rname) == want[1], (server, rname)
    assert seen > 3 * S  # several rpcs per server, and the nameless rows
    assert store.getSpanDurations(5 * hour, "no-such-service", "") == {}
    store.close()
    twin.close()
    dec.close()
