// The two zngamd_bgzf_partition_records entry points with hostile class counts, labels, record models, delimiters, flags and NULL
// pointers, and no context: every call must answer ZNGAMD_E_ARG before it touches anything.  A stand-alone program:
// tests/test_cpu_bgzf_partition.py builds the library's host side and this file under AddressSanitizer + UndefinedBehaviorSanitizer and
// runs it as a plain child process.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zng_amd.h"

static int failures = 0;

struct Case {
    const char *what;
    int delim;
    uint32_t flags, record_lines;
    int32_t first_byte;
    const uint16_t *labels;
    uint64_t n_labels;
    uint32_t n_classes;
    bool records, bytes, totals;
};

// form 0: host, 1: device.  The count arrays hold exactly n_classes entries (one when that is 0 or hostile): a write behind them is a report
static int call(int form, zngamd_ctx *ctx, const Case &c)
{
    zngamd_bgzf_partition_totals t;
    memset(&t, 0, sizeof t);
    const size_t n = c.n_classes >= 1 && c.n_classes <= ZNGAMD_BGZF_PARTITION_MAX_CLASSES ? c.n_classes : 1;
    std::vector<uint64_t> rec(n, 7), byt(n, 7);
    int r;
    if (form == 0)
        r = zngamd_bgzf_partition_records(ctx, nullptr, 0, nullptr, 0, 0, 0, c.delim, c.flags, c.record_lines, c.first_byte, 0, nullptr, nullptr, 0, nullptr, 0,
                                          nullptr, nullptr, c.labels, c.n_labels, c.n_classes, c.records ? rec.data() : nullptr, c.bytes ? byt.data() : nullptr,
                                          c.totals ? &t : nullptr);
    else
        r = zngamd_bgzf_partition_records_dev(ctx, nullptr, 0, nullptr, 0, 0, 0, c.delim, c.flags, c.record_lines, c.first_byte, 0, nullptr, 0, nullptr, nullptr, 0,
                                              nullptr, 0, c.labels, c.n_labels, c.n_classes, c.records ? rec.data() : nullptr, c.bytes ? byt.data() : nullptr,
                                              c.totals ? &t : nullptr);
    for (size_t i = 0; i < n; i++)
        if (rec[i] != 7 || byt[i] != 7) { printf("FAIL %s (form %d): a refused call wrote the counts\n", c.what, form); failures++; break; }
    return r;
}

static void expect_arg(const Case &c, zngamd_ctx *ctx)
{
    for (int form = 0; form < 2; form++) {
        const int r = call(form, ctx, c);
        if (r != ZNGAMD_E_ARG) { printf("FAIL %s (form %d): %d\n", c.what, form, r); failures++; }
    }
}

int main()
{
    // the labels are exactly as many as n_labels says: a read behind them is a report
    std::vector<uint16_t> lab = {0, 1, ZNGAMD_BGZF_PARTITION_DROP, 2};
    const uint16_t *L = lab.data();
    const uint32_t F = ZNGAMD_BGZF_GREP_FINAL, G = ZNGAMD_BGZF_CLASSIFY_GROUP;
    const Case cases[] = {
        {"n_classes 0", '\n', F, 4, '@', L, 4, 0, true, true, true},
        {"n_classes 1025", '\n', F, 4, '@', L, 4, 1025, true, true, true},
        {"n_classes 2^16", '\n', F, 4, '@', L, 4, 1u << 16, true, true, true},
        {"n_classes 2^32 - 1", '\n', F | G, 4, '@', L, 4, 0xFFFFFFFFu, true, true, true},
        {"labels = NULL with n_labels 4", '\n', F, 4, '@', nullptr, 4, 3, true, true, true},
        {"labels = NULL with n_labels 2^63", '\n', F, 4, '@', nullptr, 1ull << 63, 3, true, true, true},
        {"record_lines 0", '\n', F, 0, '@', L, 4, 3, true, true, true},
        {"record_lines 65", '\n', F, 65, '@', L, 4, 3, true, true, true},
        {"record_lines 2^31", '\n', F, 1u << 31, '@', L, 4, 3, true, true, true},
        {"first_byte -2", '\n', F, 4, -2, L, 4, 3, true, true, true},
        {"first_byte 256", '\n', F, 4, 256, L, 4, 3, true, true, true},
        {"delimiter -1", -1, F, 4, '@', L, 4, 3, true, true, true},
        {"delimiter 256", 256, F, 4, '@', L, 4, 3, true, true, true},
        {"_INVERT", '\n', F | ZNGAMD_BGZF_GREP_INVERT, 4, '@', L, 4, 3, true, true, true},
        {"_LINE_START", '\n', F | ZNGAMD_BGZF_GREP_LINE_START, 4, '@', L, 4, 3, true, true, true},
        {"_COUNT_ONLY", '\n', G | ZNGAMD_BGZF_GREP_COUNT_ONLY, 4, '@', L, 4, 3, true, true, true},
        {"flag 32", '\n', G | 32u, 4, '@', L, 4, 3, true, true, true},
        {"flag 2^31", '\n', 1u << 31, 4, '@', L, 4, 3, true, true, true},
        {"totals = NULL", '\n', F, 4, '@', L, 4, 3, true, true, false},
        {"class_records = NULL", '\n', F, 4, '@', L, 4, 3, false, true, true},
        {"class_bytes = NULL", '\n', F | G, 4, '@', L, 4, 3, true, false, true},
        {"ctx = NULL with everything else in order", '\n', F | G, 4, '@', L, 4, 3, true, true, true},
        {"ctx = NULL, no labels, 1024 classes", '\n', 0, 1, -1, nullptr, 0, 1024, true, true, true},
    };
    uint8_t not_a_context = 0;      // one byte where a context would be: a call that touched it before judging the arguments is a report
    for (const Case &c : cases) {
        expect_arg(c, nullptr);
        if (strncmp(c.what, "ctx = NULL", 10)) expect_arg(c, (zngamd_ctx *)&not_a_context);
    }
    if (sizeof(zngamd_bgzf_partition_totals) != 72 || ZNGAMD_BGZF_PARTITION_MAX_CLASSES != 1024u || ZNGAMD_BGZF_PARTITION_DROP != 0xFFFFu) { printf("FAIL layout\n"); failures++; }
    if (failures) return 1;
    printf("bgzf partition arguments clean\n");
    return 0;
}
