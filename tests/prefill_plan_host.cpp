// prefill_plan_host.cpp -- the planner of batched prefill (rwkv.cppy_amd/csrc/prefill_plan.hpp) under
// the host sanitizers: a stand-alone program, built by tests/test_prefill_batch_cpu.py with
// -fsanitize=address,undefined.  The output arrays are heap blocks of exactly max_segs entries, so a
// write past them is a report; the plan's properties are checked again here.  Exit status 0: all held.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "prefill_plan.hpp"

using rwkvmi::prefill_plan;

static int failures = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);            \
            failures++;                                                \
        }                                                              \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void check(const std::vector<size_t> & lengths, size_t cap) {
    size_t total = 0;
    for (size_t n : lengths) total += n;
    const size_t chunks = (total + cap - 1) / cap, bound = lengths.size() + chunks - 1;
    std::vector<uint32_t> row(bound), begin(bound), len(bound), chunk(bound);
    const long long n = prefill_plan(lengths.data(), lengths.size(), cap, row.data(), begin.data(), len.data(), chunk.data(), bound);
    CHECK(n > 0 && (size_t)n <= bound);
    if (n <= 0) return;
    size_t r = 0, in_row = 0, pos = 0, c = 0;
    for (long long j = 0; j < n; j++) {
        CHECK(row[j] == r && chunk[j] == c && begin[j] == pos && len[j] >= 1);
        in_row += len[j];
        pos += len[j];
        CHECK(pos <= cap && in_row <= lengths[r]);
        if (in_row == lengths[r]) r++, in_row = 0;
        else CHECK(pos == cap);  // a row is cut only where its chunk is full
        if (pos == cap) pos = 0, c++;
    }
    CHECK(r == lengths.size() && in_row == 0);
    CHECK(c + (pos ? 1 : 0) == chunks);
    // one entry short: reported, and the blocks of n - 1 entries are not overrun
    if (n > 1) {
        std::vector<uint32_t> a(n - 1), b(n - 1), d(n - 1), e(n - 1);
        CHECK(prefill_plan(lengths.data(), lengths.size(), cap, a.data(), b.data(), d.data(), e.data(), (size_t)n - 1) == -1);
    }
    CHECK(prefill_plan(lengths.data(), lengths.size(), cap, nullptr, nullptr, nullptr, nullptr, 0) == -1);
}

int main() {
    const size_t caps[] = {1, 8, 1024};
    for (size_t cap : caps) {
        check({1}, cap);
        check({cap}, cap);
        check({cap + 1}, cap);
        check({3 * cap + 1}, cap);
        check(std::vector<size_t>(256, 1), cap);
        for (int it = 0; it < 40; it++) {
            std::vector<size_t> lengths(1 + rnd() % 256);
            for (size_t & n : lengths) n = 1 + rnd() % (it % 2 ? 3 * cap + 2 : 9);
            check(lengths, cap);
        }
    }
    const size_t zero[] = {3, 0, 2};
    uint32_t o[4][8];
    CHECK(prefill_plan(zero, 3, 8, o[0], o[1], o[2], o[3], 8) == -2);
    CHECK(prefill_plan(zero, 0, 8, o[0], o[1], o[2], o[3], 8) == -2);
    CHECK(prefill_plan(zero, 1, 0, o[0], o[1], o[2], o[3], 8) == -2);
    CHECK(prefill_plan(nullptr, 1, 8, o[0], o[1], o[2], o[3], 8) == -2);
    if (failures) return 1;
    printf("prefill_plan: ok\n");
    return 0;
}
