"""The device decoder's span-name calls (include/zkingest.h zk_ingest_dev_create_names,
zk_ingest_dev_num_span_names, zk_ingest_dev_span_name) without a device: argument checks that come
before any device is touched, and the read-only DecoderDictionary view over a stand-in decoder."""
import ctypes as C

import pytest

from zipkin_amd import _abi
from zipkin_amd.aggregates import DecoderDictionary


def test_create_names_rejects_bad_arguments_without_a_device():
    L = _abi.lib()
    h = C.c_void_p()
    for bad in (0, 65536, 1 << 20):
        assert L.zk_ingest_dev_create_names(0, None, 64, bad, C.byref(h)) == _abi.ZK_ERR_INVALID_ARG, bad
    assert L.zk_ingest_dev_create_names(0, None, 64, 8, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_dev_create_names(0, None, 0, 8, C.byref(h)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_dev_create_names(0, None, (1 << 20) + 1, 8, C.byref(h)) == _abi.ZK_ERR_INVALID_ARG
    assert not h.value


def test_accessors_reject_null_handles_and_null_outputs():
    L = _abi.lib()
    n32, n64 = C.c_uint32(), C.c_uint64()
    assert L.zk_ingest_dev_num_span_names(None, C.byref(n32)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_dev_span_name(None, 0, None, 0, C.byref(n64)) == _abi.ZK_ERR_INVALID_ARG
    # a non-null handle is never read before the output pointer is checked
    fake = C.c_void_p(C.addressof(C.create_string_buffer(8)))
    assert L.zk_ingest_dev_num_span_names(fake, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_dev_span_name(fake, 0, None, 0, None) == _abi.ZK_ERR_INVALID_ARG


class FakeDecoder:
    """the accessors DecoderDictionary reads, over two growing lists"""

    def __init__(self):
        self.services, self.spans, self.reads = [], [], 0

    @property
    def num_services(self):
        return len(self.services)

    @property
    def num_span_names(self):
        return len(self.spans)

    def service_name(self, i):
        self.reads += 1
        return self.services[i]

    def span_name(self, i):
        self.reads += 1
        return self.spans[i]


def test_decoder_dictionary_is_a_growing_read_only_view():
    dec = FakeDecoder()
    svc, rpc = DecoderDictionary(dec), DecoderDictionary(dec, "span_names")
    assert len(svc) == 0 and len(rpc) == 0 and "web" not in svc and svc.get("web") is None
    with pytest.raises(KeyError):
        rpc.id("get")
    dec.services += ["web", "app"]
    dec.spans += ["get"]
    assert (len(svc), len(rpc)) == (2, 1)
    assert svc.id("app") == 1 and svc.name(0) == "web" and "web" in svc and "get" not in svc
    assert rpc.id("get") == 0 and rpc.get("get") == 0 and "get" in rpc and "web" not in rpc
    # growth: the new names appear, the old ones keep their ids and are not read again
    reads = dec.reads
    dec.spans += ["put", "web"]  # the same string as a service, with an unrelated id
    assert rpc.id("web") == 2 and svc.id("web") == 0 and rpc.name(1) == "put" and len(rpc) == 3
    assert dec.reads == reads + 2
    # a lookup never adds
    with pytest.raises(KeyError):
        rpc.id("delete")
    assert rpc.get("delete") is None and len(rpc) == 3 and dec.spans == ["get", "put", "web"]
    assert not hasattr(rpc, "add")
    with pytest.raises(ValueError):
        DecoderDictionary(dec, "annotations")
