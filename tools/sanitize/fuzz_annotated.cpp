// fuzz_annotated.cpp — ASan/UBSan driver for zk_ingest_spans_annotated (CPU only).
//
// Built by tools/sanitize/Makefile (target `annotated`) from the product source zk_ingest.cpp with
// -fsanitize=address,undefined and no recovery: any out-of-bounds access, use-after-free, leak or undefined
// behaviour aborts the run. The seed fragments are written here, by a small TBinaryProtocol writer: spans
// whose annotations carry hosts with ipv4 and port at the i32 / i16 bounds, repeated host structs, fields of
// the wrong wire type, no host at all. Every seed is decoded as is and under deterministic mutations (bit
// flips, truncation, splices, random bytes), through the plain codec, strict and lenient, with row buffers
// that are large enough, one short and empty, with and without the item buffers; large batches go through
// the decoder's thread pool and must give the rows of the one-thread decode. A corpus file in fuzz_host's
// format (u32 little-endian length, then the bytes) may be given to add its fragments to the seeds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "zkingest.h"

namespace {

uint64_t g_rng = 0xD1B54A32D192ED03ull;
uint64_t rnd() {
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

typedef std::vector<uint8_t> Bytes;

void be(Bytes& b, uint64_t v, int bytes) {
    for (int i = bytes - 1; i >= 0; --i) b.push_back((uint8_t)(v >> (8 * i)));
}
void field(Bytes& b, uint8_t type, int16_t id) {
    b.push_back(type);
    be(b, (uint16_t)id, 2);
}
void str(Bytes& b, int16_t id, const std::string& s) {
    field(b, 11, id);
    be(b, s.size(), 4);
    b.insert(b.end(), s.begin(), s.end());
}

Bytes endpoint(int variant) {
    Bytes b;
    const int32_t ips[] = {INT32_MIN, INT32_MAX, -1, 0, 0x0A000001, 0x7F000001};
    const int16_t ports[] = {INT16_MIN, INT16_MAX, -1, 0, 80};
    if (variant % 7 != 6) {
        field(b, 8, 1);
        be(b, (uint32_t)ips[rnd() % 6], 4);
    }
    if (variant % 5 != 4) {
        field(b, 6, 2);
        be(b, (uint16_t)ports[rnd() % 5], 2);
    }
    if (variant % 11 == 3) {  // a known id with another wire type
        field(b, 10, 1);
        be(b, rnd(), 8);
        field(b, 8, 2);
        be(b, (uint32_t)rnd(), 4);
    }
    if (variant % 3) str(b, 3, variant % 4 ? "service-" + std::to_string(variant % 9) : "");
    b.push_back(0);
    return b;
}

Bytes seed_span(int k) {
    static const char* const values[] = {"cs", "cr", "sr", "ss", "custom", "a longer annotation value", "x"};
    Bytes b;
    field(b, 10, 1);
    be(b, k % 13 ? rnd() : (k % 2 ? ~0ull : 0ull), 8);
    str(b, 3, k % 17 ? "name-" + std::to_string(k % 5) : "Unknown");
    field(b, 10, 4);
    be(b, rnd(), 8);
    if (k % 3) {
        field(b, 10, 5);
        be(b, rnd(), 8);
    }
    const int lists = 1 + (k % 19 == 0);  // now and then two field-6 lists: the second is appended
    for (int l = 0; l < lists; ++l) {
        const uint32_t n = (uint32_t)(rnd() % 7);
        field(b, 15, 6);
        b.push_back(12);
        be(b, n, 4);
        for (uint32_t i = 0; i < n; ++i) {
            field(b, 10, 1);
            be(b, 1 + rnd() % (1ull << 62), 8);
            if (rnd() % 16) str(b, 2, values[rnd() % 7]);
            const int hosts = (int)(rnd() % 8 == 0 ? 2 : rnd() % 4 != 0);
            for (int h = 0; h < hosts; ++h) {
                field(b, 12, 3);
                const Bytes e = endpoint((int)(rnd() % 1000));
                b.insert(b.end(), e.begin(), e.end());
            }
            b.push_back(0);
        }
    }
    if (k % 4 == 0) {  // a binary annotation with a host: no row
        field(b, 15, 8);
        b.push_back(12);
        be(b, 1, 4);
        str(b, 1, "key");
        str(b, 2, "value");
        field(b, 12, 4);
        const Bytes e = endpoint(k);
        b.insert(b.end(), e.begin(), e.end());
        b.push_back(0);
    }
    b.push_back(0);
    return b;
}

struct Batch {
    Bytes buf;
    std::vector<uint64_t> off{0};
    void add(const Bytes& b) {
        buf.insert(buf.end(), b.begin(), b.end());
        off.push_back(buf.size());
    }
};

struct Rows {
    std::vector<uint64_t> tid, sid, val;
    std::vector<int64_t> ts;
    std::vector<uint32_t> ip, svc, bits;
    uint64_t n = 0;
    zk_status st = ZK_OK;
    uint64_t records = 0;
};

// cap: the rows' capacity; the arrays hold exactly that many, so a row past it is an overflow ASan sees
Rows decode(zk_ingest* g, const Batch& b, uint32_t flags, uint64_t cap, bool items) {
    const uint64_t n = b.off.size() - 1;
    std::vector<uint64_t> tid(n), sid(n), pid(n);
    std::vector<int64_t> f(n), l(n);
    std::vector<uint32_t> svc(n), fl(n);
    zk_span_cols out{tid.data(), sid.data(), pid.data(), f.data(), l.data(), svc.data(), fl.data(), n};
    const uint64_t icap = 4 * n + 4;
    std::vector<uint32_t> ks(icap), as(icap);
    std::vector<uint64_t> kk(icap), av(icap);
    zk_ingest_items it{ks.data(), kk.data(), icap, 0, as.data(), av.data(), icap, 0};
    Rows r;
    const uint64_t room = cap ? cap : 1;  // (a vector of 0 entries has no address to give)
    r.tid.resize(room), r.sid.resize(room), r.val.resize(room), r.ts.resize(room), r.ip.resize(room), r.svc.resize(room),
        r.bits.resize(room);
    zk_ingest_annotation_rows an{r.tid.data(), r.sid.data(), r.ts.data(), r.val.data(), r.ip.data(), r.svc.data(), r.bits.data(), cap, 99};
    uint64_t nout = 0, nrej = 0;
    const uint8_t* p = b.buf.empty() ? (const uint8_t*)"" : b.buf.data();
    r.st = zk_ingest_spans_annotated(g, p, b.off.data(), n, ZK_CODEC_THRIFT, flags, &out, &nout, &nrej, items ? &it : nullptr, &an);
    if (nout > n || an.n > cap || (r.st == ZK_ERR_CAPACITY && !items && an.n != cap)) abort();
    if (r.st == ZK_OK && nout + nrej != n) abort();
    uint32_t nsvc = 0;
    if (zk_ingest_num_services(g, &nsvc) != ZK_OK) abort();
    for (uint64_t i = 0; i < an.n; ++i) {
        const uint32_t bits = r.bits[i];
        if ((bits & 7u) > 4u || (bits & 0xFFF0u)) abort();                                  // the kind, the reserved bits
        if (!(bits & 8u) && (bits >> 16 || r.ip[i] || r.svc[i])) abort();                  // no host: zeros
        if ((bits & 8u) && r.svc[i] >= nsvc) abort();                                      // a host: a service of the dictionary
        uint64_t len = 0;
        if (zk_ingest_string(g, r.val[i], nullptr, 0, &len) != ZK_OK) abort();             // the value's string is kept
        if ((bits & 7u) && len != 2) abort();
        if (r.ts[i] <= 0) abort();                                                         // an accepted span's annotation
    }
    r.n = an.n;
    r.records = nout;
    return r;
}

bool same(const Rows& a, const Rows& b) {
    if (a.n != b.n || a.st != b.st || a.records != b.records) return false;
    for (uint64_t i = 0; i < a.n; ++i)
        if (a.tid[i] != b.tid[i] || a.sid[i] != b.sid[i] || a.ts[i] != b.ts[i] || a.val[i] != b.val[i] || a.ip[i] != b.ip[i] ||
            a.svc[i] != b.svc[i] || a.bits[i] != b.bits[i])
            return false;
    return true;
}

Bytes mutate(const Bytes& in) {
    Bytes b = in;
    switch (rnd() % 4) {
        case 0:
            for (int k = 0, m = 1 + (int)(rnd() % 6); k < m && !b.empty(); ++k) b[rnd() % b.size()] ^= (uint8_t)rnd();
            break;
        case 1:
            if (!b.empty()) b.resize(rnd() % b.size());
            break;
        case 2:  // splice a random window over another position
            if (b.size() > 4) {
                const size_t a = rnd() % b.size(), c = rnd() % b.size(), len = rnd() % (b.size() - (a > c ? a : c));
                memmove(&b[c], &b[a], len);
            }
            break;
        default:  // random bytes
            b.resize(rnd() % 64);
            for (auto& x : b) x = (uint8_t)rnd();
    }
    return b;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s iterations [corpus]\n", argv[0]);
        return 2;
    }
    const long iters = atol(argv[1]);
    std::vector<Bytes> corpus;
    for (int k = 0; k < 400; ++k) corpus.push_back(seed_span(k));
    if (argc > 2) {
        FILE* fp = fopen(argv[2], "rb");
        if (!fp) return 2;
        for (;;) {
            uint32_t len;
            if (fread(&len, 4, 1, fp) != 1) break;
            Bytes b(len);
            if (len && fread(b.data(), 1, len, fp) != len) return 2;
            corpus.push_back(std::move(b));
        }
        fclose(fp);
    }
    uint64_t rows = 0, short_caps = 0;
    // the seeds as they are: every one decodes; the exact cap, one short, none
    {
        zk_ingest* g = nullptr;
        if (zk_ingest_create(&g) != ZK_OK) return 2;
        Batch b;
        for (int k = 0; k < 400; ++k) b.add(corpus[k]);
        const Rows full = decode(g, b, ZK_INGEST_STRICT, 8 * 400, true);
        if (full.st != ZK_OK || full.records != 400 || full.n == 0) abort();
        rows += full.n;
        const Rows exact = decode(g, b, 0, full.n, false);
        if (!same(full, exact)) abort();
        for (uint64_t cap : {full.n - 1, (uint64_t)1, (uint64_t)0}) {
            const Rows few = decode(g, b, ZK_INGEST_SPAN_NAMES, cap, true);
            if (few.st != ZK_ERR_CAPACITY || few.n != cap || few.records != 400) abort();
            ++short_caps;
        }
        zk_ingest_destroy(g);
    }
    // large batches: the thread pool against the one-thread decode, clean and with mutated fragments
    for (int rep = 0; rep < 3; ++rep) {
        Batch b;
        while (b.off.size() < 20001) {
            const Bytes& c = corpus[rnd() % corpus.size()];
            b.add(rep && rnd() % 8 == 0 ? mutate(c) : c);
        }
        zk_ingest *g1 = nullptr, *g2 = nullptr;
        if (zk_ingest_create(&g1) != ZK_OK || zk_ingest_create(&g2) != ZK_OK) return 2;
        const Rows many = decode(g1, b, ZK_INGEST_SPAN_NAMES, 8 * 20000, rep == 1);
        const Rows one = decode(g2, b, ZK_INGEST_SPAN_NAMES | ZK_INGEST_ONE_THREAD, 8 * 20000, rep == 1);
        if (!same(many, one)) abort();
        rows += many.n;
        const Rows strict1 = decode(g1, b, ZK_INGEST_STRICT, 8 * 20000, false);
        const Rows strict2 = decode(g2, b, ZK_INGEST_STRICT | ZK_INGEST_ONE_THREAD, 8 * 20000, false);
        if (strict1.st != strict2.st) abort();
        zk_ingest_destroy(g1);
        zk_ingest_destroy(g2);
    }
    // mutated fragments in small batches
    zk_ingest* g = nullptr;
    if (zk_ingest_create(&g) != ZK_OK) return 2;
    for (long it = 0; it < iters; ++it) {
        Batch b;
        const int m = 1 + (int)(rnd() % 16);
        for (int k = 0; k < m; ++k) b.add(rnd() % 4 ? mutate(corpus[rnd() % corpus.size()]) : corpus[rnd() % corpus.size()]);
        const uint64_t cap = rnd() % 3 ? 8 * (uint64_t)m + 64 : rnd() % 8;
        const Rows r = decode(g, b, (uint32_t)(rnd() & 1) | ((rnd() & 1) ? ZK_INGEST_SPAN_NAMES : 0u), cap, (rnd() & 1) != 0);
        rows += r.n;
        short_caps += r.st == ZK_ERR_CAPACITY;
    }
    zk_ingest_destroy(g);
    printf("sanitized run ok: %zu seed fragments, %ld mutated batches, %llu rows written, %llu short buffers\n", corpus.size(), iters,
           (unsigned long long)rows, (unsigned long long)short_caps);
    return 0;
}
