// The two zngamd_bgzf_trim_records entry points with hostile configurations, adapters, drop masks, delimiters, flags and NULL pointers,
// and no context: every call must answer ZNGAMD_E_ARG before it touches anything.  A stand-alone program:
// tests/test_cpu_bgzf_trim.py builds the library's host side and this file under AddressSanitizer + UndefinedBehaviorSanitizer and runs
// it as a plain child process.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "zng_amd.h"

static int failures = 0;

struct Args {
    zngamd_bgzf_trim_conf conf;
    bool with_conf = true, with_totals = true, with_patterns = true, with_table = true;
    std::vector<uint8_t> patterns;              // exactly as many bytes as the table names: a read behind them is a report
    std::vector<zngamd_bgzf_pattern> table;
    uint32_t n_patterns = 0;
    int delim = '\n';
    uint32_t flags = ZNGAMD_BGZF_GREP_FINAL;
    std::vector<uint8_t> drop;
    bool with_drop = false;
    uint64_t n_drop = 0;
};

static Args good()
{
    Args a;
    memset(&a.conf, 0, sizeof a.conf);
    a.conf.record_lines = 4; a.conf.seq_line = 1; a.conf.qual_line = 3; a.conf.first_byte = '@'; a.conf.qual_back = 20; a.conf.quality_base = 33;
    a.conf.max_mismatch = 2; a.conf.min_overlap = 3; a.conf.min_length = 20;
    const char *ads[] = {"AGATCGGAAGAGCACACGTC", "CTGTCTCTTATACACATCT", "TGGAATTCTCGG"};
    for (const char *s : ads) {
        a.table.push_back({(uint32_t)a.patterns.size(), (uint32_t)strlen(s)});
        a.patterns.insert(a.patterns.end(), s, s + strlen(s));
    }
    a.n_patterns = 3;
    return a;
}

// form 0: host, 1: device
static int call(int form, zngamd_ctx *ctx, const Args &a, const char *what)
{
    zngamd_bgzf_trim_totals t;
    memset(&t, 0x5A, sizeof t);
    const uint8_t *pat = a.with_patterns ? a.patterns.data() : nullptr;
    const zngamd_bgzf_pattern *tab = a.with_table ? a.table.data() : nullptr;
    const uint8_t *drop = a.with_drop ? a.drop.data() : nullptr;
    const zngamd_bgzf_trim_conf *cf = a.with_conf ? &a.conf : nullptr;
    int r;
    if (form == 0)
        r = zngamd_bgzf_trim_records(ctx, nullptr, 0, nullptr, 0, 0, 0, pat, (uint32_t)a.patterns.size(), tab, a.n_patterns, a.delim, a.flags, cf, 0, nullptr, drop,
                                     a.n_drop, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, a.with_totals ? &t : nullptr);
    else
        r = zngamd_bgzf_trim_records_dev(ctx, nullptr, 0, nullptr, 0, 0, 0, pat, (uint32_t)a.patterns.size(), tab, a.n_patterns, a.delim, a.flags, cf, 0, nullptr, 0,
                                         nullptr, drop, a.n_drop, nullptr, 0, nullptr, 0, nullptr, 0, a.with_totals ? &t : nullptr);
    const uint8_t *b = (const uint8_t *)&t;
    for (size_t i = 0; i < sizeof t; i++)
        if (b[i] != 0x5A) { printf("FAIL %s (form %d): a refused call wrote the totals\n", what, form); failures++; break; }
    return r;
}

static void expect_arg(const char *what, const std::function<void(Args &)> &change, bool ctx_too = true)
{
    Args a = good();
    change(a);
    uint8_t not_a_context = 0;      // one byte where a context would be: a call that touched it before judging the arguments is a report
    for (int form = 0; form < 2; form++) {
        int r = call(form, nullptr, a, what);
        if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d): %d\n", what, form, r); failures++; }
        if (!ctx_too) continue;
        r = call(form, (zngamd_ctx *)&not_a_context, a, what);
        if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d, with a context): %d\n", what, form, r); failures++; }
    }
}

int main()
{
    expect_arg("conf = NULL", [](Args &a) { a.with_conf = false; });
    expect_arg("totals = NULL", [](Args &a) { a.with_totals = false; });
    expect_arg("record_lines 0", [](Args &a) { a.conf.record_lines = 0; });
    expect_arg("record_lines 65", [](Args &a) { a.conf.record_lines = 65; });
    expect_arg("record_lines 2^31", [](Args &a) { a.conf.record_lines = 1u << 31; });
    expect_arg("seq_line -1", [](Args &a) { a.conf.seq_line = -1; });
    expect_arg("seq_line 4", [](Args &a) { a.conf.seq_line = 4; });
    expect_arg("qual_line -2", [](Args &a) { a.conf.qual_line = -2; });
    expect_arg("qual_line 4", [](Args &a) { a.conf.qual_line = 4; });
    expect_arg("qual_line == seq_line", [](Args &a) { a.conf.qual_line = 1; });
    expect_arg("first_byte -2", [](Args &a) { a.conf.first_byte = -2; });
    expect_arg("first_byte 256", [](Args &a) { a.conf.first_byte = 256; });
    expect_arg("qual_front 94", [](Args &a) { a.conf.qual_front = 94; });
    expect_arg("qual_back 2^32 - 1", [](Args &a) { a.conf.qual_back = 0xFFFFFFFFu; });
    expect_arg("a cutoff without a qual_line", [](Args &a) { a.conf.qual_line = -1; });
    expect_arg("quality_base 256", [](Args &a) { a.conf.quality_base = 256; });
    expect_arg("max_mismatch 17", [](Args &a) { a.conf.max_mismatch = 17; });
    expect_arg("max_mismatch = the shortest adapter", [](Args &a) { a.conf.max_mismatch = 12; });
    expect_arg("min_overlap 0", [](Args &a) { a.conf.min_overlap = 0; });
    expect_arg("min_overlap 256", [](Args &a) { a.conf.min_overlap = 256; });
    expect_arg("conf.flags 2", [](Args &a) { a.conf.flags = 2; });
    expect_arg("reserved[0]", [](Args &a) { a.conf.reserved[0] = 1; });
    expect_arg("reserved[2]", [](Args &a) { a.conf.reserved[2] = 1u << 31; });
    expect_arg("65 adapters", [](Args &a) { a.patterns.assign(65, 'A'); a.table.clear(); for (uint32_t i = 0; i < 65; i++) a.table.push_back({i, 1}); a.n_patterns = 65; a.conf.max_mismatch = 0; });
    expect_arg("an adapter of 0 bytes", [](Args &a) { a.table[1].len = 0; });
    expect_arg("an adapter of 256 bytes", [](Args &a) { a.patterns.assign(256, 'A'); a.table = {{0, 256}}; a.n_patterns = 1; });
    expect_arg("an adapter behind the bytes", [](Args &a) { a.table[2].off = (uint32_t)a.patterns.size() - 11; });
    expect_arg("an adapter at 2^32 - 1", [](Args &a) { a.table[2].off = 0xFFFFFFFFu; });
    expect_arg("an adapter with the delimiter", [](Args &a) { a.patterns[25] = '\n'; });
    expect_arg("patterns = NULL with 3 adapters", [](Args &a) { a.with_patterns = false; });
    expect_arg("table = NULL with 3 adapters", [](Args &a) { a.with_table = false; });
    expect_arg("drop = NULL with n_drop 4", [](Args &a) { a.n_drop = 4; });
    expect_arg("drop = NULL with n_drop 2^63", [](Args &a) { a.n_drop = 1ull << 63; });
    expect_arg("delimiter -1", [](Args &a) { a.delim = -1; });
    expect_arg("delimiter 256", [](Args &a) { a.delim = 256; });
    expect_arg("_INVERT", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_INVERT; });
    expect_arg("_LINE_START", [](Args &a) { a.flags |= ZNGAMD_BGZF_GREP_LINE_START; });
    expect_arg("_COUNT_ONLY", [](Args &a) { a.flags = ZNGAMD_BGZF_CLASSIFY_GROUP | ZNGAMD_BGZF_GREP_COUNT_ONLY; });
    expect_arg("flag 32", [](Args &a) { a.flags |= 32u; });
    expect_arg("flag 2^31", [](Args &a) { a.flags = 1u << 31; });
    expect_arg("ctx = NULL with everything else in order", [](Args &) {}, false);
    expect_arg("ctx = NULL, grouped, with a mask", [](Args &a) { a.flags |= ZNGAMD_BGZF_CLASSIFY_GROUP; a.drop = {0, 1, 0}; a.with_drop = true; a.n_drop = 3; a.conf.flags = ZNGAMD_BGZF_TRIM_KEEP_SHORT; }, false);
    expect_arg("ctx = NULL, no adapters, no qualities", [](Args &a) { a.n_patterns = 0; a.with_patterns = a.with_table = false; a.conf.qual_line = -1; a.conf.qual_back = 0; a.conf.max_mismatch = 16; }, false);
    if (sizeof(zngamd_bgzf_trim_totals) != 632 || sizeof(zngamd_bgzf_trim_row) != 12 || sizeof(zngamd_bgzf_trim_conf) != 64) { printf("FAIL layout\n"); failures++; }
    if (failures) return 1;
    printf("bgzf trim arguments clean\n");
    return 0;
}
