// CPU check of shadow_amd/csrc/evq_merge.h (the key form, compare, merge-path search and dead-prefix
// count of the device-resident event queues): the partition + per-tile, per-thread sequential merge
// that k_evq_partition / k_evq_merge run, replayed on the host and compared with std::merge over
// the live events.  Prints "ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../shadow_amd/csrc/evq_merge.h"

using srg::EvqKey;

namespace {

constexpr uint64_t TILE = 64, ITEMS = 4;  // small, so that a few hundred events cross many tiles

struct Keys {
    const std::vector<EvqKey>* v;
    uint64_t base;
    EvqKey operator()(uint64_t i) const { return (*v)[base + i]; }
};

bool lessk(const EvqKey& x, const EvqKey& y) { return srg::evq_less(x, y); }

int failures = 0;
void expect(bool c, const char* what, int line) {
    if (!c) {
        std::fprintf(stderr, "FAILED line %d: %s\n", line, what);
        ++failures;
    }
}
#define EXPECT(c) expect((c), #c, __LINE__)

// A: sorted resident array with host segments and dead prefixes; B: sorted batch.  Replays the
// device algorithm; returns the merged live array and whether an equal live pair was seen.
std::vector<EvqKey> device_merge(const std::vector<EvqKey>& A, const std::vector<uint64_t>& host_off,
                                 const std::vector<uint64_t>& head, uint32_t H, const std::vector<EvqKey>& B,
                                 bool& dup) {
    const uint64_t na = A.size(), nb = B.size(), n = na + nb;
    std::vector<uint64_t> dead_excl(H + 1, 0);
    for (uint32_t h = 0; h < H; ++h) dead_excl[h + 1] = dead_excl[h] + (head[h] - host_off[h]);
    const uint64_t n_out = n - dead_excl[H];
    const uint64_t ntiles = (n + TILE - 1) / TILE;
    std::vector<uint64_t> part_a(ntiles + 1), part_live(ntiles + 1);
    const Keys fa{&A, 0}, fb{&B, 0};
    for (uint64_t i = 0; i <= ntiles; ++i) {
        const uint64_t diag = std::min(i * TILE, n);
        const uint64_t a = srg::evq_merge_path(fa, na, fb, nb, diag);
        const uint32_t dst = a < na ? srg::evq_dst(A[a].w0) : 0;
        part_a[i] = a;
        part_live[i] = diag - srg::evq_dead_before(a, na, dst, host_off.data(), head.data(), dead_excl.data(), H);
    }
    EXPECT(part_live[ntiles] == n_out);
    std::vector<EvqKey> out(n_out, EvqKey{~0ull, ~0ull, ~0ull});
    dup = false;
    for (uint64_t t = 0; t < ntiles; ++t) {
        const uint64_t d0 = t * TILE, d1 = std::min(d0 + TILE, n);
        const uint64_t a0 = part_a[t], a1 = part_a[t + 1], b0 = d0 - a0, b1 = d1 - a1;
        const uint64_t tna = a1 - a0, tnb = b1 - b0, total = tna + tnb;
        EXPECT(a1 >= a0 && b1 >= b0 && total == d1 - d0);
        const Keys ta{&A, a0}, tb{&B, b0};
        uint64_t pos = part_live[t];
        for (uint64_t th = 0; th < TILE / ITEMS; ++th) {
            const uint64_t diag = std::min(th * ITEMS, total);
            uint64_t a = srg::evq_merge_path(ta, tna, tb, tnb, diag), b = diag - a;
            for (uint64_t it = 0; it < ITEMS && a + b < total; ++it) {
                if (b >= tnb || (a < tna && !lessk(tb(b), ta(a)))) {
                    const uint64_t g = a0 + a;
                    if (g >= head[srg::evq_dst(A[g].w0)]) out[pos++] = A[g];
                    ++a;
                } else {
                    const uint64_t g = a0 + a;  // the A event merged right in front: A[g - 1]
                    if (g > 0 && g - 1 >= head[srg::evq_dst(A[g - 1].w0)] && srg::evq_equal(A[g - 1], tb(b))) dup = true;
                    out[pos++] = tb(b);
                    ++b;
                }
            }
        }
        EXPECT(pos == part_live[t + 1]);
    }
    return out;
}

struct Case {
    std::vector<EvqKey> A, B;
    std::vector<uint64_t> host_off, head;
    uint32_t H;
};

// sorts, derives host_off, and kills a prefix of each host's segment (dead_frac of it)
Case make_case(std::vector<EvqKey> A, std::vector<EvqKey> B, uint32_t H, double dead_frac, std::mt19937_64& rng) {
    std::sort(A.begin(), A.end(), lessk);
    A.erase(std::unique(A.begin(), A.end(), srg::evq_equal), A.end());
    std::sort(B.begin(), B.end(), lessk);
    B.erase(std::unique(B.begin(), B.end(), srg::evq_equal), B.end());
    Case c{A, B, std::vector<uint64_t>(H + 1, 0), std::vector<uint64_t>(H, 0), H};
    for (const EvqKey& k : A) ++c.host_off[srg::evq_dst(k.w0) + 1];
    for (uint32_t h = 0; h < H; ++h) c.host_off[h + 1] += c.host_off[h];
    for (uint32_t h = 0; h < H; ++h) {
        const uint64_t len = c.host_off[h + 1] - c.host_off[h];
        uint64_t dead = 0;
        if (dead_frac > 0 && len) dead = (uint64_t)(dead_frac * (double)(rng() % (len + 1)));
        c.head[h] = c.host_off[h] + dead;
    }
    return c;
}

void check(const Case& c, bool expect_dup = false) {
    std::vector<EvqKey> liveA;
    for (uint64_t g = 0; g < c.A.size(); ++g)
        if (g >= c.head[srg::evq_dst(c.A[g].w0)]) liveA.push_back(c.A[g]);
    std::vector<EvqKey> want(liveA.size() + c.B.size());
    std::merge(liveA.begin(), liveA.end(), c.B.begin(), c.B.end(), want.begin(), lessk);
    bool dup = false;
    const std::vector<EvqKey> got = device_merge(c.A, c.host_off, c.head, c.H, c.B, dup);
    EXPECT(got.size() == want.size());
    bool same = got.size() == want.size();
    for (size_t i = 0; same && i < got.size(); ++i) same = srg::evq_equal(got[i], want[i]);
    EXPECT(same);
    EXPECT(dup == expect_dup);
}

std::vector<EvqKey> random_keys(size_t n, uint32_t H, uint64_t t_span, uint32_t src_span, uint64_t id_span,
                                std::mt19937_64& rng) {
    std::vector<EvqKey> v(n);
    for (EvqKey& k : v)
        k = srg::evq_pack((uint32_t)(rng() % H), 1000 + rng() % t_span, (uint32_t)(rng() % src_span), rng() % id_span);
    return v;
}

}  // namespace

int main() {
    std::mt19937_64 rng(12345);
    // pack / unpack and full-width compares
    {
        const EvqKey k = srg::evq_pack(0x80000001u, 0xFEDCBA9876543210ull, 0xDEADBEEFu, 0x0123456789ABCDEFull);
        EXPECT(srg::evq_dst(k.w0) == 0x80000001u && srg::evq_time(k.w0, k.w1) == 0xFEDCBA9876543210ull);
        EXPECT(srg::evq_src(k.w1) == 0xDEADBEEFu && k.w2 == 0x0123456789ABCDEFull);
        EXPECT(lessk(srg::evq_pack(1, 5, 9, 9), srg::evq_pack(1, 5 + (1ull << 40), 0, 0)));  // time bits >= 32
        EXPECT(lessk(srg::evq_pack(1, 5, 9, 3), srg::evq_pack(1, 5, 9, 3 + (1ull << 40))));  // id bits >= 32
        EXPECT(lessk(srg::evq_pack(1, 5, 2, 9), srg::evq_pack(1, 5, 3, 0)));                 // src at equal time
        EXPECT(lessk(srg::evq_pack(1, ~0ull, ~0u, ~0ull), srg::evq_pack(2, 0, 0, 0)));       // dst first
        EXPECT(lessk(srg::evq_pack(0x7FFFFFFFu, 9, 9, 9), srg::evq_pack(0x80000000u, 0, 0, 0)));
        EXPECT(!lessk(k, k) && srg::evq_equal(k, k));
    }
    // random inputs, with and without dead prefixes, sizes around the tile
    const size_t sizes[] = {0, 1, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 7, 700};
    for (size_t na : sizes)
        for (size_t nb : sizes)
            for (double dead : {0.0, 1.0}) {
                Case c = make_case(random_keys(na, 7, 5000, 5, 1u << 20, rng), random_keys(nb, 7, 5000, 5, 1u << 20, rng),
                                   7, dead, rng);
                // a dead A event may equal a B event: only live pairs count
                bool dup = false;
                for (uint64_t g = 0; g < c.A.size(); ++g)
                    if (g >= c.head[srg::evq_dst(c.A[g].w0)] &&
                        std::binary_search(c.B.begin(), c.B.end(), c.A[g], lessk))
                        dup = true;
                check(c, dup);
            }
    // all of A before B, and the reverse
    {
        std::vector<EvqKey> lo, hi;
        for (uint64_t i = 0; i < 3 * TILE + 5; ++i) lo.push_back(srg::evq_pack(1, 100 + i, 0, i));
        for (uint64_t i = 0; i < 2 * TILE + 1; ++i) hi.push_back(srg::evq_pack(2, 100 + i, 0, i));
        check(make_case(lo, hi, 4, 0.0, rng));
        check(make_case(hi, lo, 4, 0.0, rng));
        check(make_case(lo, hi, 4, 1.0, rng));
        check(make_case(hi, lo, 4, 1.0, rng));
    }
    // long runs equal in the leading words: one host, one time, one source, ids interleaved
    {
        std::vector<EvqKey> a, b;
        for (uint64_t i = 0; i < 4 * TILE; ++i) (i % 3 ? a : b).push_back(srg::evq_pack(3, 777, 5, i));
        check(make_case(a, b, 4, 0.0, rng));
        check(make_case(a, b, 4, 1.0, rng));
        // ... and differing only above bit 32 of the id
        a.clear();
        b.clear();
        for (uint64_t i = 0; i < 4 * TILE; ++i) (i % 2 ? a : b).push_back(srg::evq_pack(3, 777, 5, i << 33));
        check(make_case(a, b, 4, 0.0, rng));
    }
    // an equal live pair is flagged wherever it falls, also across a tile boundary; an equal pair
    // whose resident half is dead is not
    for (uint64_t at : {uint64_t(0), TILE / 2 - 1, TILE / 2, TILE - 1, TILE, 3 * TILE}) {
        std::vector<EvqKey> a, b;
        for (uint64_t i = 0; i < 4 * TILE; ++i) a.push_back(srg::evq_pack(0, 100 + i, 0, i));
        b.push_back(a[at]);
        Case c = make_case(a, b, 1, 0.0, rng);
        check(c, true);
        c.head[0] = at + 1;  // popped
        check(c, false);
    }
    // a pushed event that sorts in front of a dead one (time == last popped, smaller source)
    {
        std::vector<EvqKey> a, b;
        for (uint64_t i = 0; i < TILE + 3; ++i) a.push_back(srg::evq_pack(1, 100 + i / 2, 7, i));
        b.push_back(srg::evq_pack(1, 100 + (TILE / 2) / 2, 1, 0));
        b.push_back(srg::evq_pack(0, 5, 0, 0));
        Case c = make_case(a, b, 3, 0.0, rng);
        c.head[1] = c.host_off[1] + TILE / 2 + 2;
        check(c);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
