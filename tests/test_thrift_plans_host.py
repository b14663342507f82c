"""Thrift wire-form conformance, host side: the planned encodings of tests/thriftplan.py through the
independent reader (tests/thriftref.py) and the host decoder of include/zkingest.h.

The families (S1, S2 single-byte edits; Z truncations in front of zero bytes; A the alignment sweep;
O order / absence / duplication / wire types; K unknown fields; KD nesting depth; G and GD the same
behind 21000 bytes) are described in tests/thriftplan.py. The expectation of every case is thriftref's reading of the bytes, taken through
the span-level oracle (span_to_record, expected_items); the only cases it does not decide are KD's:
  containers open inside one skipped value   device   host
  <= 16                                      accepts  accepts
  17 .. 64                                   rejects  accepts   (the one documented divergence)
  65, the innermost empty                    rejects  accepts   (Rd::skip rejects a VALUE inside more than
  65 around a value; 66 and more             rejects  rejects    64 containers: an empty 65th holds none)
tests/test_gpu_thrift_plans.py runs the same cases through the three builds of the device decoder.
All comparisons are exact."""
import functools
from collections import Counter
from pathlib import Path

import pytest

from tests import thriftplan as TP
from tests import thriftref as R
from tests.test_ingest import expected_items, expected_records
from tests.test_snappy_plans_host import view
from zipkin_amd import ZkError, _abi
from zipkin_amd.ingest import SpanDecoder

FAMILY_NAMES = sorted(TP.FAMILIES)
TP_ROOT = Path(__file__).resolve().parent.parent


@functools.lru_cache(maxsize=None)
def readings(fam):
    """thriftref's result for every case of a family"""
    return [R.decode(c.raw) for c in TP.FAMILIES[fam]()]


def outcome(c, reading, who):
    """the reading as decoder `who` ("host" / "device") must see it: a nesting case past its limit is
    undecodable"""
    if c.depth is not None and reading[0] == "ok":
        accepts = TP.host_accepts if who == "host" else TP.device_accepts
        if not accepts(*c.depth):
            return ("undecodable",)
    return reading


def expected_view(cases, results, who):
    """what a decode with items and span names gives, from thriftref's Spans alone"""
    spans = [r[1] for c, r in zip(cases, results) for r in (outcome(c, r, who),) if r[0] == "ok"]
    want, ids = expected_records(spans)
    names = list(ids)
    for r, s in zip(want, spans):
        r["service"] = names[r.pop("service_id")] if r["flags"] & 12 else None
        r["name"] = s.name if s.name not in ("", "Unknown") else ""
    kv, ann = R.items(spans, expected_items)
    return {"records": want, "rejected": len(cases) - len(spans), "kv": kv, "ann": ann}


@functools.lru_cache(maxsize=None)
def family_view(fam, who):
    return expected_view(TP.FAMILIES[fam](), readings(fam), who)


def host_view(cases, snappy):
    dec = SpanDecoder()
    blobs = [c.stream if snappy else c.raw for c in cases]
    v = view(dec, dec.decode(blobs, snappy=snappy, strict=False, items=True, span_names=True), items=True, span_names=True)
    v["span_names"] = Counter(dec.span_names())
    return v


def name_set(v):
    return Counter({r["name"] for r in v["records"] if r["name"]})


# ---- the generators -----------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_constructed_cases_read_back(fam):
    """every case built from a Span reads back as that Span, every case built to be rejected is rejected
    for the planned reason, and a nesting case is as deep as its id says"""
    cases = TP.FAMILIES[fam]()
    assert len({c.id for c in cases}) == len(cases) <= 6000
    planned = 0
    for c, r in zip(cases, readings(fam)):
        if isinstance(c.want, str):
            assert R.why(r) == c.want, c.id
        elif c.want is not None:
            assert r[0] == "ok" and r[1] == R.comparable(c.want), (c.id, r)
        if c.depth is not None:
            assert r[0] == "ok" and r[2]["skip_depth"] == c.depth[0], c.id
        planned += c.want is not None
    assert planned == {"S1": 0, "S2": 0, "Z": len(cases) // 2}.get(fam, len(cases))


@pytest.mark.parametrize("fam", ["S1", "S2"])
def test_family_s_is_neither_all_accept_nor_all_reject(fam):
    kinds = Counter(r[0] for r in readings(fam))
    n = sum(kinds.values())
    assert kinds["ok"] >= 0.10 * n, kinds
    assert kinds["invalid"] + kinds["undecodable"] >= 0.30 * n, kinds
    assert kinds["invalid"] and kinds["undecodable"]
    whys = {R.why(r) for r in readings(fam)}
    # (no single-byte edit empties a value and leaves the bytes decodable: families A and O hold that form)
    assert whys >= {None, R.UNDECODABLE, R.NO_NAME, R.NO_TIMESTAMP}, whys


def test_family_a_puts_every_window_at_every_residue():
    """each window of the device's fast path (parse_record_fast) at every offset & 3 from the
    fragment's first byte, with and without parent_id (w1 is the fragment's first byte: its address
    is the batch layout's doing, 64 different ones per wave)"""
    seen = {}
    for c in TP.family_a():
        w = TP.fast_windows(c.raw)
        at = w["w2"][0] + 11
        parent = c.raw[at:at + 3] == TP.fh(TP.I64, 5)
        for name, offs in w.items():
            seen.setdefault((name, bool(parent)), set()).update(o & 3 for o in offs)
    assert len(seen) == 22
    for key, residues in seen.items():
        assert residues == ({0} if key[0] == "w1" else {0, 1, 2, 3}), key
    empties = Counter()
    for c, r in zip(TP.family_a(), readings("A")):
        if r[0] == "ok":
            sp = r[1]
            empties["name"] += sp.name == ""
            empties["key"] += any(b.key == "" for b in sp.binary_annotations)
            empties["host"] += sp.annotations[0].host.service_name == R.UNKNOWN_SERVICE_NAME
            empties["bhost"] += sp.binary_annotations[0].host.service_name == R.UNKNOWN_SERVICE_NAME
        else:
            empties["value"] += R.why(r) == R.NO_VALUE
    assert all(empties[k] >= 50 for k in ("name", "key", "host", "bhost", "value")), empties


def test_family_g_is_past_the_lds_budget():
    both = TP.family_g() + TP.family_gd()
    big = [c for c in both if not c.id.startswith("G-small")]
    assert 120 <= len(big) <= 200
    assert all(len(c.raw) > TP.G_BUDGET and len(c.stream) > TP.G_BUDGET for c in big)
    assert all(len(c.stream) < 640 for c in both if c.id.startswith("G-small"))
    assert all((c.depth is not None) == (fam in TP.DEPTH_FAMILIES) for fam in TP.FAMILIES for c in TP.FAMILIES[fam]()
               if not c.id.startswith("G-small"))


def test_nesting_limits_are_the_decoders_own():
    """the limits the KD expectations use, read from the sources: `depth > 64` in Rd::skip (host), a
    16-entry stack and `sp + open == 16` in DRdT::skip (device); include/zkingest.h states both"""
    import re

    host = (TP_ROOT / "zipkin_amd" / "csrc" / "zk_ingest.cpp").read_text()
    dev = (TP_ROOT / "zipkin_amd" / "csrc" / "zk_ingest_dev.hip").read_text()
    assert int(re.search(r"if \(depth > (\d+)\)", host).group(1)) == TP.HOST_SKIP_DEPTH
    assert int(re.search(r"kSkipDepth = (\d+);", dev).group(1)) == TP.DEVICE_SKIP_DEPTH
    header = (TP_ROOT / "include" / "zkingest.h").read_text()
    assert "at most 16 containers" in header and "inside at most 64 containers" in header
    assert [TP.host_accepts(d, "scalar") for d in (64, 65)] == [True, False]
    assert [TP.host_accepts(d, "empty") for d in (65, 66)] == [True, False]
    assert [TP.device_accepts(d, "empty") for d in (16, 17)] == [True, False]


# ---- the host decoder ---------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_host_decoder(fam):
    """the host decoder on the raw thrift == on the Snappy streams == thriftref's reading: records by
    name, rejected counts, item multisets, span names"""
    cases = TP.FAMILIES[fam]()
    want = family_view(fam, "host")
    for snappy in (False, True):
        got = host_view(cases, snappy)
        assert got["rejected"] == want["rejected"], snappy
        for k in ("records", "kv", "ann"):
            if got[k] != want[k] and k == "records":  # name the first case that differs
                ok = [c.id for c, r in zip(cases, readings(fam)) if outcome(c, r, "host")[0] == "ok"]
                bad = [(i, g, w) for i, g, w in zip(ok, got[k], want[k]) if g != w][:3]
                assert not bad, bad
            assert got[k] == want[k], (k, snappy)
        assert got["span_names"] == name_set(want), snappy


def test_host_decoder_nesting_cases_one_by_one():
    """accept or reject of every KD case alone (in a batch the counts could cancel)"""
    dec = SpanDecoder()
    for c in TP.family_kd() + [c for c in TP.family_gd() if c.depth]:
        _, rej = dec.decode([c.raw], snappy=False, strict=False)
        assert rej == (0 if TP.host_accepts(*c.depth) else 1), c.id


@functools.lru_cache(maxsize=None)
def strict_batches():
    """[(id, index of the bad fragment, its message, [raw fragments])]: one fragment of each rejection
    class at positions 0, 1 and n - 1 of a batch of 70 (n - 1 lies in a second wave of 64), the rest
    accepted forms of family O"""
    good = [c.raw for c in TP.family_o() if isinstance(c.want, TP.Span)][:69]
    s1 = dict((c.id, c) for c in TP.family_s1())
    o = dict((c.id, c) for c in TP.family_o())
    bad = [s1["S1-trunc%d" % (len(TP.RAW_B1) - 9)], o["O-type-3-i64"], o["O-two-timestamps-second-zero"],
           o["O-two-values-second-empty"], s1["S1-sub0-0b"]]
    out = []
    for c in bad:
        msg = R.why(R.decode(c.raw))
        assert msg is not None
        for at in (0, 1, len(good)):
            out.append((c.id, at, msg, good[:at] + [c.raw] + good[at:]))
    assert {m for _, _, m, _ in out} == {R.UNDECODABLE, R.NO_NAME, R.NO_TIMESTAMP, R.NO_VALUE}
    return out


def test_host_decoder_strict_names_the_bad_fragment_and_the_reason():
    for cid, at, msg, blobs in strict_batches():
        for snappy in (False, True):
            with pytest.raises(ZkError) as e:
                SpanDecoder().decode([TP.T.snappy(b) for b in blobs] if snappy else blobs, snappy=snappy, strict=True)
            assert e.value.status == _abi.ZK_ERR_INVALID_SPAN, cid
            assert e.value.message == "span %d: %s" % (at, msg), (cid, at, e.value.message)
