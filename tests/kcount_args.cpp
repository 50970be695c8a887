// The entry points of the k-mer count -- zngamd_kmer_counter_new, _reserve, _add, _describe, _histogram, _export, _free and
// zngamd_bgzf_count_kmers[_dev] -- with hostile rules, rooms, pairs, configurations, delimiters, flags and NULL pointers, and no context:
// every call must answer ZNGAMD_E_ARG before it touches anything.  A stand-alone program: tests/test_cpu_bgzf_kcount.py builds the
// library's host side and this file under AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a plain child process.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>

#include "zng_amd.h"

static int failures = 0;
static uint8_t not_a_context = 0;      // one byte where a context would be: a call that touched it before judging the arguments is a report

static bool untouched(const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; i++) if (b[i] != 0x5A) return false;
    return true;
}

// ---- the counter
static void expect_new(const char *what, uint32_t k, uint32_t flags, uint64_t room, bool with_out, bool ctx_too = true)
{
    for (int with_ctx = 0; with_ctx <= (ctx_too ? 1 : 0); with_ctx++) {
        zngamd_kmer_counter *out = (zngamd_kmer_counter *)(uintptr_t)0x5A5A;
        const int r = zngamd_kmer_counter_new(with_ctx ? (zngamd_ctx *)&not_a_context : nullptr, k, flags, room, with_out ? &out : nullptr);
        if (r != ZNGAMD_E_ARG) { printf("FAIL new, %s (context %d): %d\n", what, with_ctx, r); failures++; }
        if (out != (zngamd_kmer_counter *)(uintptr_t)0x5A5A) { printf("FAIL new, %s: a refused call wrote\n", what); failures++; }
    }
}

// No counter can exist without a context, so the counter is NULL: every call on it must refuse and write nothing.
static void counter_calls()
{
    uint64_t codes[2] = {1, 2}, counts[2] = {1, 1}, hist[4], n = 0x5A5A5A5A5A5A5A5Aull;
    memset(hist, 0x5A, sizeof hist);
    zngamd_kmer_counter_info info;
    memset(&info, 0x5A, sizeof info);
    struct { const char *what; int r; } calls[] = {
        {"reserve", zngamd_kmer_counter_reserve(nullptr, 0)},
        {"reserve, a room beyond any table", zngamd_kmer_counter_reserve(nullptr, ~0ull)},
        {"add", zngamd_kmer_counter_add(nullptr, codes, counts, 2)},
        {"add, no pair", zngamd_kmer_counter_add(nullptr, nullptr, nullptr, 0)},
        {"add, no arrays", zngamd_kmer_counter_add(nullptr, nullptr, nullptr, 2)},
        {"describe", zngamd_kmer_counter_describe(nullptr, &info)},
        {"describe, no info", zngamd_kmer_counter_describe(nullptr, nullptr)},
        {"histogram", zngamd_kmer_counter_histogram(nullptr, hist, 4)},
        {"histogram, one bin", zngamd_kmer_counter_histogram(nullptr, hist, 1)},
        {"histogram, too many bins", zngamd_kmer_counter_histogram(nullptr, hist, ZNGAMD_KMER_HIST_MAX_BINS + 1u)},
        {"histogram, no array", zngamd_kmer_counter_histogram(nullptr, nullptr, 4)},
        {"export", zngamd_kmer_counter_export(nullptr, 1, 0, codes, counts, 2, &n)},
        {"export, min_count 0", zngamd_kmer_counter_export(nullptr, 0, 0, codes, counts, 2, &n)},
        {"export, no arrays", zngamd_kmer_counter_export(nullptr, 1, 0, nullptr, nullptr, 2, &n)},
        {"export, no n", zngamd_kmer_counter_export(nullptr, 1, 0, codes, counts, 2, nullptr)},
    };
    for (const auto &c : calls) if (c.r != ZNGAMD_E_ARG) { printf("FAIL %s: %d\n", c.what, c.r); failures++; }
    if (!untouched(&info, sizeof info) || !untouched(hist, sizeof hist) || !untouched(&n, sizeof n) || codes[0] != 1 || counts[1] != 1) {
        printf("FAIL a refused counter call wrote\n"); failures++;
    }
    zngamd_kmer_counter_free(nullptr);                      // nothing happens
}

// ---- the count of a window
struct Args {
    zngamd_bgzf_count_conf conf;
    bool with_conf = true, with_totals = true;
    int delim = '\n';
    uint32_t flags = ZNGAMD_BGZF_GREP_FINAL;
};

static Args good()
{
    Args a;
    memset(&a.conf, 0, sizeof a.conf);
    a.conf.record_lines = 4; a.conf.seq_line = 1; a.conf.first_byte = '@';
    return a;
}

// form 0: host, 1: device
static int call(int form, zngamd_ctx *ctx, const Args &a, const char *what)
{
    zngamd_bgzf_count_totals t;
    memset(&t, 0x5A, sizeof t);
    int32_t status = 0x5A5A5A5A;
    const zngamd_bgzf_count_conf *cf = a.with_conf ? &a.conf : nullptr;
    zngamd_bgzf_count_totals *tp = a.with_totals ? &t : nullptr;
    const int r = form == 0 ? zngamd_bgzf_count_kmers(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, nullptr, 0, &status, tp)
                            : zngamd_bgzf_count_kmers_dev(ctx, nullptr, 0, nullptr, 0, 0, 0, a.delim, a.flags, cf, nullptr, 0, nullptr, 0, nullptr, tp);
    if (!untouched(&t, sizeof t) || status != 0x5A5A5A5A) { printf("FAIL count form %d, %s: a refused call wrote\n", form, what); failures++; }
    return r;
}

static void expect_count(const char *what, const std::function<void(Args &)> &change)
{
    Args a = good();
    change(a);
    for (int form = 0; form < 2; form++)
        for (int with_ctx = 0; with_ctx < 2; with_ctx++) {
            const int r = call(form, with_ctx ? (zngamd_ctx *)&not_a_context : nullptr, a, what);
            if (r != ZNGAMD_E_ARG) { printf("FAIL count form %d, %s (context %d): %d\n", form, what, with_ctx, r); failures++; }
        }
}

int main()
{
    static_assert(sizeof(zngamd_bgzf_count_conf) == 64 && sizeof(zngamd_bgzf_count_totals) == 88 && sizeof(zngamd_kmer_counter_info) == 64, "layout");
    static_assert(offsetof(zngamd_bgzf_count_totals, kmers) == sizeof(zngamd_bgzf_key_totals) && offsetof(zngamd_bgzf_count_totals, tail_off) ==
                  offsetof(zngamd_bgzf_key_totals, tail_off) && offsetof(zngamd_bgzf_count_totals, bad) == offsetof(zngamd_bgzf_key_totals, bad), "totals");
    expect_new("k 0", 0, 1, 0, true);
    expect_new("k 32", 32, 1, 0, true);
    expect_new("k 2^31", 1u << 31, 1, 0, true);
    expect_new("flags 2", 31, 2, 0, true);
    expect_new("flags 3", 31, 3, 0, true);
    expect_new("flags 2^31", 31, 1u << 31, 0, true);
    expect_new("a room beyond the largest table", 31, 1, ZNGAMD_KMER_COUNTER_MAX_CAP / 2u + 1u, true);
    expect_new("a room of all ones", 31, 1, ~0ull, true);
    expect_new("no out", 31, 1, 0, false);
    expect_new("everything in order but the context", 31, 1, 100, true, false);
    counter_calls();
    expect_count("record_lines 0", [](Args &a) { a.conf.record_lines = 0; });
    expect_count("record_lines 65", [](Args &a) { a.conf.record_lines = 65; });
    expect_count("seq_line -1", [](Args &a) { a.conf.seq_line = -1; });
    expect_count("seq_line 4", [](Args &a) { a.conf.seq_line = 4; });
    expect_count("first_byte -2", [](Args &a) { a.conf.first_byte = -2; });
    expect_count("first_byte 256", [](Args &a) { a.conf.first_byte = 256; });
    expect_count("conf.flags 1", [](Args &a) { a.conf.flags = 1; });
    expect_count("conf.flags 2^31", [](Args &a) { a.conf.flags = 1u << 31; });
    expect_count("reserved[0]", [](Args &a) { a.conf.reserved[0] = 1; });
    expect_count("reserved[11]", [](Args &a) { a.conf.reserved[11] = 1; });
    expect_count("delimiter -1", [](Args &a) { a.delim = -1; });
    expect_count("delimiter 256", [](Args &a) { a.delim = 256; });
    expect_count("flags FINAL | 1", [](Args &a) { a.flags |= 1; });
    expect_count("flags FINAL | 2", [](Args &a) { a.flags |= 2; });
    expect_count("flags FINAL | 8", [](Args &a) { a.flags |= 8; });
    expect_count("flags 2^31", [](Args &a) { a.flags = 1u << 31; });
    expect_count("no totals", [](Args &a) { a.with_totals = false; });
    expect_count("no conf", [](Args &a) { a.with_conf = false; });
    expect_count("everything in order but the counter", [](Args &) {});
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("bgzf count arguments clean\n");
    return 0;
}
