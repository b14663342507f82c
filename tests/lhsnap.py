"""Independent reference of the link-histogram snapshot format (TEST INFRASTRUCTURE ONLY): written
from the format text of include/zksketch.h, with no import of the library.

Little-endian. Header, 64 bytes: u32 magic "ZKLH", u32 version = 1, u32 sub_bits m, u32 bins,
u64 rows, u64 entries, u64 links (the sum of all counts), u64 dropped, zero padding. Then `rows`
descriptors of 16 bytes {u32 parent, u32 child, u64 first}, strictly ascending by (parent, child),
`first` = the index of the row's first entry. Then `entries` u64 words (bin << 32) | count, ascending by
bin inside a row, count >= 1. One histogram state has exactly one byte string."""
from __future__ import annotations

import struct

import numpy as np

MAGIC = b"ZKLH"
HEADER = 64
ROW = np.dtype([("parent", "<u4"), ("child", "<u4"), ("first", "<u8")])


def nbins(m: int) -> int:
    return (41 - m) << m


def header(m: int, rows: int, entries: int, links: int, dropped: int = 0, *, magic: bytes = MAGIC, version: int = 1,
           bins: int | None = None) -> bytes:
    return magic + struct.pack("<IIIQQQQ", version, m, nbins(m) if bins is None else bins, rows, entries, links,
                               dropped) + bytes(16)


def pack(m: int, rows, entries, dropped: int = 0, links: int | None = None) -> bytes:
    """A blob from explicit rows [(parent, child, first)] and entries [(bin, count)], valid or not."""
    body = b"".join(struct.pack("<IIQ", p, c, f) for p, c, f in rows)
    body += b"".join(struct.pack("<Q", (b << 32) | n) for b, n in entries)
    total = sum(n for _, n in entries) if links is None else links
    return header(m, len(rows), len(entries), total, dropped) + body


def encode(dense, S: int, m: int, dropped: int = 0) -> bytes:
    """The canonical snapshot of a dense uint32[S * S, bins] table (cell = parent * S + child)."""
    dense = np.asarray(dense)
    assert dense.shape == (S * S, nbins(m)), dense.shape
    cell, b = np.nonzero(dense)  # row-major: ascending by cell, then by bin
    counts = dense[cell, b].astype(np.uint64)
    present, first = np.unique(cell, return_index=True)
    rows = np.zeros(len(present), ROW)
    rows["parent"], rows["child"], rows["first"] = present // S, present % S, first
    entries = (b.astype(np.uint64) << np.uint64(32)) | counts
    return header(m, len(rows), len(entries), int(counts.sum(dtype=np.uint64)), dropped) + rows.tobytes() + \
        entries.astype("<u8").tobytes()


def decode(blob: bytes, S: int):
    """(dense uint32[S * S, bins], m, dropped) of a well-formed blob."""
    assert blob[:4] == MAGIC
    version, m, bins, nrows, nent, links, dropped = struct.unpack_from("<IIIQQQQ", blob, 4)
    assert version == 1 and bins == nbins(m) and len(blob) == HEADER + 16 * nrows + 8 * nent
    rows = np.frombuffer(blob, ROW, nrows, HEADER)
    entries = np.frombuffer(blob, "<u8", nent, HEADER + 16 * nrows)
    dense = np.zeros((S * S, bins), np.uint32)
    ends = np.r_[rows["first"][1:], np.uint64(nent)].astype(np.int64)
    for r, e1 in zip(rows, ends.tolist()):
        e = entries[int(r["first"]):e1]
        dense[int(r["parent"]) * S + int(r["child"]), (e >> np.uint64(32)).astype(np.int64)] = \
            (e & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert int(dense.sum(dtype=np.uint64)) == links
    return dense, m, dropped
